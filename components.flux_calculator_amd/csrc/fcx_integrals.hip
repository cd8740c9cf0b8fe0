// fcx_integrals.hip -- exact (area-weighted) field sums on the device: fcx_field_integrals,
// fcx_atmos_integrals.  A translation unit of its own: nothing here is shared with the flux
// kernels of fcx_kernels.hip but the descriptor's addressing rule.
//
// field_sum_kernel streams the fields like field_range_kernel and adds every finite term
// exactly into a 68-limb fixed-point accumulator (fcx_exactsum.h); field_sum_finish_kernel, the
// next launch on the stream, folds the per-block partials.  Every addition is an integer
// addition, so the bits of the result depend neither on the number of blocks nor on the order
// the lanes arrive in; there is no global atomic, no arrival counter and no float atomic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include "fcx_internal.h"
#include "fcx_exactsum.h"

#pragma clang fp contract(off)

namespace fcx {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
// global address space: GLOBAL loads, counted in vmcnt alone (see fcx_kernels.hip)
#define FCX_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ const FCX_GLOBAL T *gptr(const T *p) {
  return (const FCX_GLOBAL T *)p;
}

using u64 = unsigned long long;
constexpr int kWin = 6;  // limbs of a lane's register window: 2^139 of dynamic range

// A lane's state.  WIN: a window of kWin consecutive limbs in registers, opened two limbs below
// the lane's first non-zero term (64 bits of room below it, 32 above); a term whose three
// digits fall inside is added with plain integer VALU work, any other term goes to the block's
// LDS accumulator.  Without WIN (the baseline) every term goes to LDS.  A lane adds at most
// 2^16 + 16 terms, each below 2^32 per limb: no carry inside a lane (fcx_exactsum.h).
template <bool WIN>
struct SumLane {
  int64_t w[WIN ? kWin : 1];
  int32_t wb;  // the window's first limb, -1 while it is closed
  int32_t n_fin, n_nan, n_pinf, n_ninf;  // (a lane adds at most 2^16 + 16 terms)
};

template <bool WIN>
__device__ __forceinline__ void sum_take(SumLane<WIN> &ln, u64 *acc, double t) {
  const uint64_t bits = (uint64_t)__double_as_longlong(t);
  const int cls = exsum_class(bits);
  ln.n_nan += cls == 1, ln.n_pinf += cls == 2, ln.n_ninf += cls == 3;
  if (cls) return;
  ++ln.n_fin;
  if (!(bits << 1)) return;  // a zero of either sign
  const ExsumDigits d = exsum_digits(bits);
  const bool neg = bits >> 63;
  const int64_t s0 = neg ? -(int64_t)d.d0 : (int64_t)d.d0, s1 = neg ? -(int64_t)d.d1 : (int64_t)d.d1,
                s2 = neg ? -(int64_t)d.d2 : (int64_t)d.d2;
  if constexpr (WIN) {
    if (ln.wb < 0) ln.wb = min(max(d.limb - 2, 0), kExsumLimbs - kWin);
    const int o = d.limb - ln.wb;
    if ((unsigned)o <= (unsigned)(kWin - 3)) {
      // the three digits moved up by o = 0..3 limbs in two steps (by one, then by two)
      static_assert(kWin == 6, "three digits shifted by at most three limbs");
      const bool by1 = o & 1, by2 = o & 2;
      const int64_t a0 = by1 ? 0 : s0, a1 = by1 ? s0 : s1, a2 = by1 ? s1 : s2, a3 = by1 ? s2 : 0;
      ln.w[0] += by2 ? 0 : a0;
      ln.w[1] += by2 ? 0 : a1;
      ln.w[2] += by2 ? a0 : a2;
      ln.w[3] += by2 ? a1 : a3;
      ln.w[4] += by2 ? a2 : 0;
      ln.w[5] += by2 ? a3 : 0;
      return;
    }
  }
  atomicAdd(&acc[d.limb], (u64)s0);  // LDS: d.limb + 2 <= 66
  atomicAdd(&acc[d.limb + 1], (u64)s1);
  if (s2) atomicAdd(&acc[d.limb + 2], (u64)s2);
}

// the term of cell j: x widened exactly, times the area in one IEEE multiply (no FMA)
template <bool W, class S>
__device__ __forceinline__ double sum_term(S x, double a) {
  return W ? __dmul_rn(a, (double)x) : (double)x;
}

// exsum_normalise of the 68 limbs at `limb` (LDS) by a whole block (at least 68 threads, every
// thread calls): the same result, without the 67 dependent LDS round trips.  Carries are
// propagated one after the other only from the lowest non-zero limb to one past the highest
// (a physical field occupies a handful of limbs); past that limb the carry is 0 or -1 (a
// zero limb plus a carry below 2^31 in magnitude leaves floor(carry / 2^32)), so every higher
// limb becomes carry & (2^32 - 1) and limb 67 takes the carry: stored side by side.  span: 3 ints
// of LDS.  Ends with a barrier.
__device__ __forceinline__ void block_normalise(int64_t *limb, int *span) {
  const int t = threadIdx.x;
  if (t == 0) span[0] = kExsumLimbs, span[1] = -1;
  __syncthreads();
  if (t < kExsumLimbs - 1 && limb[t] != 0) {
    atomicMin(&span[0], t);
    atomicMax(&span[1], t);
  }
  __syncthreads();
  const int last = min(span[1] + 1, kExsumLimbs - 2);
  if (t == 0) {
    int64_t carry = 0;
    for (int k = span[0]; k <= last; ++k) {
      const int64_t v = limb[k] + carry;
      limb[k] = v & 0xffffffffLL;
      carry = v >> 32;
    }
    limb[kExsumLimbs - 1] += carry;  // (last < 66: 0 or -1, and the limbs in between follow)
    span[2] = (int)carry;
  }
  __syncthreads();
  if (t > last && t < kExsumLimbs - 1 && span[2]) limb[t] = 0xffffffffLL;
  __syncthreads();
}

}  // namespace

// Grid (blocks, fields), block x of field y takes the layout tiles x, x + blocks, ... exactly as
// field_range_kernel does; when weighted the areas (contiguous, the engine's own 16-B aligned
// allocation) are loaded beside the field, and all loads of a whole tile are issued before the
// first use.  The partial last tile goes vector by vector, its partial last vector cell by
// cell; nothing at or past n is read, of the field or of the areas.  Record fields, unaligned
// arrays and uniform constants (no array: every cell is fd.cval) go value by value.
template <class S, bool W, bool WIN>
__global__ __launch_bounds__(256) void field_sum_kernel(const SumArgs a) {
  constexpr int C = 16 / sizeof(S);
  constexpr int kTrips = (int)(kLayoutTile / (256 * C));
  static_assert(kTrips >= 1 && kTrips * 256 * C == kLayoutTile, "a block's trips cover one layout tile");
  using V = typename std::conditional<sizeof(S) == 8, d2, f4>::type;
  __shared__ u64 acc[kSumWords];  // 68 limbs, then n_terms, n_nan, n_pinf, n_ninf
  __shared__ int span[3];
  if (threadIdx.x < kSumWords) acc[threadIdx.x] = 0;
  __syncthreads();
  const SumField &sf = a.f[blockIdx.y];
  const RangeField &fd = sf.r;
  const S *__restrict__ base = reinterpret_cast<const S *>(fd.p);
  const double *__restrict__ ar = sf.area;
  const int64_t n = fd.n, tiles = (n + kLayoutTile - 1) >> kLayoutShift;
  SumLane<WIN> ln{};
  ln.wb = -1;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t j0 = t << kLayoutShift;
    const S *__restrict__ tp = base + (j0 + t * fd.tpad) * fd.stride;  // tiled(j0, tpad) * stride
    if (sf.uniform) {
      const S x = (S)sf.cval;
      for (int64_t u = threadIdx.x; u < kLayoutTile && j0 + u < n; u += 256)
        sum_take(ln, acc, sum_term<W>(x, W ? gptr(ar)[j0 + u] : 0.0));
    } else if (fd.vec && j0 + kLayoutTile <= n) {
      V v[kTrips];
      d2 av[W ? kTrips * C / 2 : 1];
#pragma unroll
      for (int k = 0; k < kTrips; ++k) v[k] = gptr(reinterpret_cast<const V *>(tp))[k * 256 + threadIdx.x];
      if constexpr (W) {
#pragma unroll
        for (int k = 0; k < kTrips; ++k)
#pragma unroll
          for (int h = 0; h < C / 2; ++h)
            av[k * (C / 2) + h] = gptr(reinterpret_cast<const d2 *>(ar + j0))[(k * 256 + threadIdx.x) * (C / 2) + h];
      }
#pragma unroll
      for (int k = 0; k < kTrips; ++k)
#pragma unroll
        for (int i = 0; i < C; ++i)
          sum_take(ln, acc, sum_term<W>((S)v[k][i], W ? (double)av[W ? k * (C / 2) + i / 2 : 0][i & 1] : 0.0));
    } else if (fd.vec) {
      for (int k = 0; k < kTrips; ++k) {
        const int64_t u = (int64_t)(k * 256 + threadIdx.x) * C, j = j0 + u;
        if (j + C <= n) {
          const V x = *gptr(reinterpret_cast<const V *>(tp + u));
          d2 aw[W ? C / 2 : 1];
          if constexpr (W) {
#pragma unroll
            for (int h = 0; h < C / 2; ++h) aw[h] = gptr(reinterpret_cast<const d2 *>(ar + j))[h];
          }
#pragma unroll
          for (int i = 0; i < C; ++i) sum_take(ln, acc, sum_term<W>((S)x[i], W ? (double)aw[W ? i / 2 : 0][i & 1] : 0.0));
        } else {
          for (int i = 0; i < C; ++i)
            if (j + i < n) sum_take(ln, acc, sum_term<W>(gptr(tp)[u + i], W ? gptr(ar)[j + i] : 0.0));
        }
      }
    } else {
      for (int64_t u = threadIdx.x; u < kLayoutTile && j0 + u < n; u += 256)
        sum_take(ln, acc, sum_term<W>(gptr(tp)[u * fd.stride], W ? gptr(ar)[j0 + u] : 0.0));
    }
  }
  // the lane's window and counts into the block's accumulator, once
  if constexpr (WIN) {
    if (ln.wb >= 0) {
#pragma unroll
      for (int i = 0; i < kWin; ++i)
        if (ln.w[i]) atomicAdd(&acc[ln.wb + i], (u64)ln.w[i]);  // wb + 5 <= 67
    }
  }
  if (ln.n_fin) atomicAdd(&acc[kExsumLimbs], (u64)ln.n_fin);
  if (ln.n_nan) atomicAdd(&acc[kExsumLimbs + 1], (u64)ln.n_nan);
  if (ln.n_pinf) atomicAdd(&acc[kExsumLimbs + 2], (u64)ln.n_pinf);
  if (ln.n_ninf) atomicAdd(&acc[kExsumLimbs + 3], (u64)ln.n_ninf);
  __syncthreads();
  // a block's limbs stay below 2^57 (fcx_exactsum.h); 2048 partials would not: canonical first
  block_normalise(reinterpret_cast<int64_t *>(acc), span);
  if (threadIdx.x < kSumWords)
    a.partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kSumWords + threadIdx.x] = (int64_t)acc[threadIdx.x];
}

// One block per field folds the field's `blocks` canonical partials (at most 2048) and writes the
// canonical sum.  A single wave would add 2048 partials one dependent load after the other (0.7 ms
// measured at 10M cells, where the range call takes 45 us), so kFinishGroups groups of 72 lanes
// each take every kFinishGroups-th partial, one lane per word: a group's loads of a partial are
// 576 contiguous bytes.  At most 147 canonical partials per lane (< 2^40), 2048 in all (< 2^43).
constexpr int kFinishGroups = 14;
__global__ __launch_bounds__(1024) void field_sum_finish_kernel(const SumArgs a, int32_t blocks) {
  __shared__ int64_t s[kFinishGroups][kSumWords];
  __shared__ int span[3];
  const int64_t *__restrict__ p = a.partial + (int64_t)blockIdx.x * blocks * kSumWords;
  const int g = threadIdx.x / kSumWords, w = threadIdx.x % kSumWords;
  if (g < kFinishGroups) {
    int64_t sum = 0;
    for (int b = g; b < blocks; b += kFinishGroups) sum += gptr(p)[(int64_t)b * kSumWords + w];
    s[g][w] = sum;
  }
  __syncthreads();
  if (threadIdx.x < kSumWords) {
    int64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kFinishGroups; ++k) sum += s[k][threadIdx.x];
    s[0][threadIdx.x] = sum;
  }
  __syncthreads();
  block_normalise(s[0], span);
  int64_t *out = reinterpret_cast<int64_t *>(a.out + blockIdx.x);
  if (threadIdx.x < kSumWords) out[threadIdx.x] = s[0][threadIdx.x];
}

template <class S, bool W>
static void launch_sum(const SumArgs &a, int blocks, hipStream_t s) {
  if (a.baseline)
    hipLaunchKernelGGL((field_sum_kernel<S, W, false>), dim3(blocks, a.nf), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((field_sum_kernel<S, W, true>), dim3(blocks, a.nf), dim3(256), 0, s, a);
}

// The range launches' grid: enough blocks to fill the device, shared by the fields of the launch
// so that the partials stay within kRangePartials, never more than the longest field's tiles.
// kRangePartials / kMaxRangeFields = 128 blocks per field at least, which the carry invariant
// of fcx_exactsum.h relies on.
int launch_field_sums(SumArgs a, void *stream) {
  static_assert(kRangePartials / kMaxRangeFields >= 128, "a block takes at most 2^31 / 4096 / 128 + 1 tiles");
  static_assert(sizeof(fcx_exact_sum) == kSumWords * sizeof(int64_t), "a partial is an fcx_exact_sum");
  if (a.nf <= 0) return 0;
  if (a.nf > kMaxRangeFields || !a.partial || !a.out) return (int)hipErrorInvalidValue;
  const size_t es = a.f32 ? 4 : 8;
  int64_t tiles = 1;
  for (int f = 0; f < a.nf; ++f) {
    SumField &sf = a.f[f];
    RangeField &fd = sf.r;
    if (fd.n < 0 || fd.tpad < 0 || fd.stride < 1 || (fd.n > 0 && !fd.p && !sf.uniform) ||
        reinterpret_cast<uintptr_t>(fd.p) % es || (fd.n > 0 && a.weighted && !sf.area) ||
        reinterpret_cast<uintptr_t>(sf.area) % 16)
      return (int)hipErrorInvalidValue;
    fd.vec = !sf.uniform && fd.stride == 1 && reinterpret_cast<uintptr_t>(fd.p) % 16 == 0 && (fd.tpad * es) % 16 == 0;
    tiles = std::max(tiles, (fd.n + kLayoutTile - 1) >> kLayoutShift);
  }
  const int blocks = (int)std::min<int64_t>(tiles, kRangePartials / a.nf);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a.f32 && a.weighted)
    launch_sum<float, true>(a, blocks, s);
  else if (a.f32)
    launch_sum<float, false>(a, blocks, s);
  else if (a.weighted)
    launch_sum<double, true>(a, blocks, s);
  else
    launch_sum<double, false>(a, blocks, s);
  if (hipError_t r = hipGetLastError()) return (int)r;
  hipLaunchKernelGGL(field_sum_finish_kernel, dim3(a.nf), dim3(1024), 0, s, a, (int32_t)blocks);
  return (int)hipGetLastError();
}

}  // namespace fcx
