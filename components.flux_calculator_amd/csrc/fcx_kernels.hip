// fcx_kernels.hip -- CDNA4 (gfx950) kernels of the exchange-grid flux engine.
//
// cells_kernel: ONE fused pass over the exchange-grid cells for every flux of a coupling
// step (flux_calculator.F90:902-991): RBBR, QSUR(t,u,v), MEVA(+bias), HLAT, HSEN, UMOM,
// VMOM, RSDR and the type-0 averages.  The reference makes one pass over memory per flux
// and per surface type (7+ passes, one scalar call per cell); here every input array is
// read once and every output written once, so the kernel is HBM-bandwidth bound
// (arithmetic intensity ~1.5-2 flop/B, well below the fp64-vector/HBM ridge).
//
// Layout: struct-of-arrays, one contiguous fp64 array per (surface type, grid, var) --
// exactly the reference data model (flux_calculator_basic.F90:86-103), so a wave reads
// 64 x 16 B = 1 KiB per array per load instruction (two cells per lane, dwordx4).
// Method dispatch (namelist which_* strings, calc:37-48 etc.) is a per-type int8 read
// from the parameter block: wave-uniform, so it is a scalar branch and costs no
// divergence.  Surface types are processed type-major per cell; every cross-type effect
// the reference's flux-major order has (the 'copy' aliases, the bias added once more per
// aliased copy, calc:112-116) is resolved by the planner in fcx_engine.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include "fcx_internal.h"
#include "fcx_physics.h"

#pragma clang fp contract(off)

namespace fcx {

// C cells of one lane.  The fp64 path holds 2 cells per lane and the fp32 path 4, so one
// lane's access to an array is a single 16-B dwordx4 either way.
template <int C, class R = double>
struct Vec {
  R v[C];
};

// The precision of a cell kernel is the pair (storage type S, arithmetic type R).  S is what
// the arrays, the LDS flux rows and every layout decision (cells per 16 B, tile sizes, the
// compacted map, which family takes wave-uniform inputs or skips stores) go by; R is what the
// formulas of fcx_physics.h are instantiated with.  double and float name themselves twice (the
// fp64 and the fp32 engine); F32Wide is the fp32 engine with FCX_OPT_F32_MATH: float arrays,
// every flux computed in double from its inputs widened after the load (the inputs stay held
// as floats, the conversion is exact and free of state) and rounded to float once where it is
// stored or parked.  A value consumed inside the launch is consumed in double, unrounded.
struct F32Wide {};
template <class P>
struct Prec {
  using arith = P;
  using store = P;
};
template <>
struct Prec<F32Wide> {
  using arith = double;
  using store = float;
};
// F64Cr is the fp64 engine with FCX_OPT_CR_MATH: double arrays, double arithmetic, and the three
// transcendental sites of fcx_physics.h (the exp of QSUR and of RCO's MEVA, the Exner power)
// correctly rounded (fcx_crmath.h).  Every other operation, layout and launch shape is the
// fp64 engine's.
struct F64Cr {};
template <>
struct Prec<F64Cr> {
  using arith = double;
  using store = double;
};
template <class PR>
constexpr bool is_wide() { return std::is_same<PR, F32Wide>::value; }
template <class PR>
constexpr bool is_cr() { return std::is_same<PR, F64Cr>::value; }
// x in the element type T (the one rounding of a wide flux on its way to memory, or the exact
// widening of a loaded float); the same object where the types agree
template <class T, int C>
__device__ __forceinline__ const Vec<C, T> &cvt(const Vec<C, T> &x) {
  return x;
}
template <class T, int C, class F, class = typename std::enable_if<!std::is_same<T, F>::value>::type>
__device__ __forceinline__ Vec<C, T> cvt(const Vec<C, F> &x) {
  Vec<C, T> r;
#pragma unroll
  for (int i = 0; i < C; ++i) r.v[i] = (T)x.v[i];
  return r;
}

typedef double d2 __attribute__((ext_vector_type(2)));
#if FCX_WAVE_TRACE
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
#endif
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef int i2v __attribute__((ext_vector_type(2)));
typedef int i4v __attribute__((ext_vector_type(4)));

// Field, map and output pointers reach the kernels through the parameter block as generic
// pointers, which the compiler lowers to FLAT loads and stores.  A FLAT access counts in
// both vmcnt and lgkmcnt, so every s_waitcnt lgkmcnt(0) that waits for a scalar load (the
// next array pointer out of the parameter block) also waits for all of the wave's loads in
// flight.  These are device (or host-mapped) arrays, never LDS or scratch: addressing them
// in the global address space gives GLOBAL instructions, counted in vmcnt alone.
// (Round 3: step -0.4 % fp64, -0.7 % fp32, -1.0 % at T = 2 against FLAT, profiles/r03/global_as_ab/.)
#define FCX_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ const FCX_GLOBAL T *gptr(const T *p) {
  return (const FCX_GLOBAL T *)p;
}
template <class T>
__device__ __forceinline__ FCX_GLOBAL T *gptr(T *p) {
  return (FCX_GLOBAL T *)p;
}

// NT: streamed once -> non-temporal hint (the arrays are read once and written once per
// step; the 256 MB Infinity Cache cannot hold a 10M-cell step anyway).  Out-of-range lanes
// of a partial vector read 1 (keeps exp/pow/division of the dead lanes finite).
template <int C, bool NT, class R>
__device__ __forceinline__ Vec<C, R> ld(const R *__restrict__ p, int64_t j0, int64_t n) {
  Vec<C, R> r;
  if constexpr (C * sizeof(R) == 16 || (C == 2 && sizeof(R) == 4)) {
    if (j0 + C <= n) {
      using V = typename std::conditional<sizeof(R) == 8, d2, typename std::conditional<C == 4, f4, f2v>::type>::type;
      const FCX_GLOBAL V *q = gptr(reinterpret_cast<const V *>(p + j0));
      const V t = NT ? __builtin_nontemporal_load(q) : *q;
#pragma unroll
      for (int i = 0; i < C; ++i) r.v[i] = t[i];
      return r;
    }
  }
#pragma unroll
  for (int i = 0; i < C; ++i) r.v[i] = (j0 + i < n) ? gptr(p)[j0 + i] : R(1);
  return r;
}

template <int C, bool NT, class R>
__device__ __forceinline__ void st(R *__restrict__ p, int64_t j0, int64_t n, const Vec<C, R> &x) {
  if constexpr (C * sizeof(R) == 16 || (C == 2 && sizeof(R) == 4)) {
    if (j0 + C <= n) {
      using V = typename std::conditional<sizeof(R) == 8, d2, typename std::conditional<C == 4, f4, f2v>::type>::type;
      FCX_GLOBAL V *q = gptr(reinterpret_cast<V *>(p + j0));
      V t;
#pragma unroll
      for (int i = 0; i < C; ++i) t[i] = x.v[i];
      // (write-through sc1 / sc1 nt stores instead of nt: step +9 to +27 %,
      // profiles/r03/store_wt_ab/ -- the L2 write-back merges the output lines)
      if (NT)
        __builtin_nontemporal_store(t, q);
      else
        *q = t;
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < C; ++i)
    if (j0 + i < n) gptr(p)[j0 + i] = x.v[i];
}

template <int C, class R>
__device__ __forceinline__ Vec<C, R> splat(R a) {
  Vec<C, R> r;
#pragma unroll
  for (int i = 0; i < C; ++i) r.v[i] = a;
  return r;
}

// The value of a 'zero' method, formed where it is used.  As a plain constant the compiler
// builds the 16-B register tuple of a zero store once, outside the tile loop, and keeps it
// live through the whole flux pass for a branch that hardly ever runs: at the 128-VGPR cap of
// the fp32 MOM5 fused kernel it was the one value spilled to scratch.  The empty asm makes
// the zero opaque, so it is materialised inside the method's branch.  OPAQUE = false: the
// plain constant (the multi-type kernels: there the opaque zero cost the C = 1 register-average
// kernels 9-11 VGPRs and a wave per SIMD).
template <int C, class R, bool OPAQUE>
__device__ __forceinline__ Vec<C, R> zeros() {
  R z = R(0);
  if constexpr (OPAQUE) asm volatile("" : "+v"(z));
  return splat<C, R>(z);
}

// The parameter block holds every field pointer as double*; in the fp32 engine the same
// pointers address float arrays, so every access reinterprets them as S* (the storage type;
// ST rounds a Vec of the arithmetic type to it).
#define FOR_C _Pragma("unroll") for (int i = 0; i < C; ++i)
// Field arrays may be tile-blocked (fcx_internal.h, FCX_OPT_TILED_LAYOUT): cell j is at
// p + j + D_ with D_ = (j >> kLayoutShift) * tpad, the same shift for every array and for
// the C cells of one lane (j0 is a multiple of C, C divides the tile).  D_ is in scope
// wherever these are used; D_ = 0 for contiguous arrays.
#define LD(p, j, n) ld<C, NT, S>(reinterpret_cast<const S *>(p) + D_, j, n)
#define ST(p, j, n, ...) st<C, NT, S>(reinterpret_cast<S *>(p) + D_, j, n, cvt<S>(__VA_ARGS__))

// The wave-uniform method bytes of one surface type.  gfx950 has no byte-sized scalar load:
// read as int8_t members, each byte is a vector load, a wait for it (and for every load and
// store of the wave in flight) and a v_readfirstlane in the middle of the flux pass.  Read as
// the two aligned 64-bit words the layout guarantees (fcx_internal.h), they are scalar loads
// and the bytes are shifts.
struct Methods {
  int8_t qsur[3], meva, hlat, hsen, mom, rbbr;
  int8_t bias_adds;
  uint32_t cmask;  // TypeParams::cmask: which inputs are wave-uniform values
  uint32_t want;   // TypeParams::want: outputs computed though not stored (WantBit)
};

// The parameter block is not written while a launch runs, so its words may be read in the
// constant address space: a uniform load there is a scalar load whatever the compiler can
// prove about the stores around it.  (Read as global memory, the same words came back as
// global_load_dwordx4 with a wait and v_readfirstlane: the char-typed copy may alias every
// store of the kernel, and only a load known not to be clobbered is made scalar.)
#define FCX_CONSTANT __attribute__((address_space(4)))
typedef uint64_t __attribute__((aligned(8), may_alias)) word8_t;
typedef uint32_t __attribute__((aligned(4), may_alias)) word4_t;
template <class T>
__device__ __forceinline__ const FCX_CONSTANT word8_t *cptr(const T *p) {
  return (const FCX_CONSTANT word8_t *)p;
}
__device__ __forceinline__ int8_t byte_of(uint64_t w, int k) { return (int8_t)(uint8_t)(w >> (8 * k)); }
__device__ __forceinline__ Methods type_methods(const TypeParams &tp) {
  const uint64_t w = *cptr(&tp.m_qsur[0]), b = *cptr(&tp.bias_adds);
  return Methods{{byte_of(w, 0), byte_of(w, 1), byte_of(w, 2)}, byte_of(w, 3), byte_of(w, 4),
                 byte_of(w, 5),  byte_of(w, 6), byte_of(w, 7),  byte_of(b, 0),
                 (uint32_t)(b >> 32),
                 (uint32_t)(uint8_t)(b >> 8)};
}
__device__ __forceinline__ uint32_t type_cmask(const TypeParams &tp) {
  return (uint32_t)(*cptr(&tp.bias_adds) >> 32);
}
// An input that may be a wave-uniform value (TypeParams::cmask): c set = the member's bytes are
// the value, splat from the scalar registers, no vector load.  Lanes at or past n get 1 like
// ld()'s partial vector, so a constant differs from an array holding the value in nothing but
// the load, dead lanes included.
template <int C, bool NT, class R>
__device__ __forceinline__ Vec<C, R> ldu(const double *p, bool c, int64_t j0, int64_t n, int64_t D_) {
  if (c) {
    const uint64_t w = (uint64_t) reinterpret_cast<uintptr_t>(p);
    R v;
    if constexpr (sizeof(R) == 8)
      v = __builtin_bit_cast(double, w);
    else
      v = __builtin_bit_cast(float, (uint32_t)w);
    Vec<C, R> r;
#pragma unroll
    for (int i = 0; i < C; ++i) r.v[i] = (j0 + i < n) ? v : R(1);
    return r;
  }
  return ld<C, NT, R>(reinterpret_cast<const R *>(p) + D_, j0, n);
}
#define LDU(p, c, j, n) ldu<C, NT, S>(p, c, j, n, D_)
// The instantiations that take wave-uniform inputs: the fp64 generic and CCLM kernels without
// register averages.  In the fp32 kernels and the MOM5 and RCO kernels the uniform path cost
// scratch or a wave per SIMD when it was compiled in (DESIGN.md section 3,
// profiles/r10/isa/registers_uniform_everywhere.txt); in the register-average kernels it fit
// the registers but the T = 2 bench step lost 2.6 % with it (profiles/r10/pairs/
// t2_uniform_in_ravg_kernels.txt; the fp32 and wide register-average kernels with the fused
// accumulation are register-average kernels like the others).  There the mask is a
// compile-time zero and the planner
// binds a constant's filled mirror instead (fcx_engine.hip, build_plan: the same rule).
template <class S, int VAR, bool RAVG>
constexpr bool uniform_inputs() {
  return uniform_family(sizeof(S) == 4, VAR, RAVG);  // (fcx_internal.h: the planner's rule too)
}
__device__ __forceinline__ bool cbit(uint32_t m, int bit) { return (m >> bit) & 1u; }
// The wait of the single-type kernels for a type's inputs: vmcnt(0) alone (expcnt and lgkmcnt
// left at their maxima), as a builtin so that the compiler's wait-count pass sees it.
__device__ __forceinline__ void wait_inputs() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// Momentum of one (type, u- or v-grid) cell group; `north` selects VMOM.
struct NoEmit {
  template <int C, class R>
  __device__ __forceinline__ void operator()(int, const Vec<C, R> &) const {}
};

template <int C, bool NT, class R, class S, class Emit>
__device__ __forceinline__ void momentum(int8_t m, bool north, const UVGridPtrs &g,
                                         const Vec<C, S> &ts, const Vec<C, S> &ps, const Vec<C, S> &u,
                                         const Vec<C, S> &v, const Vec<C, R> &vel, const Vec<C, R> &qs,
                                         const Vec<C, S> &a, int64_t j0, int64_t n, int64_t D_, Emit &emit, int slot);

template <int C, bool NT, class R, class S>
__device__ __forceinline__ void momentum(int8_t m, bool north, const UVGridPtrs &g,
                                         const Vec<C, S> &ts, const Vec<C, S> &ps, const Vec<C, S> &u,
                                         const Vec<C, S> &v, const Vec<C, R> &vel, const Vec<C, R> &qs,
                                         const Vec<C, S> &a, int64_t j0, int64_t n, int64_t D_) {
  NoEmit none;
  momentum<C, NT, R, S>(m, north, g, ts, ps, u, v, vel, qs, a, j0, n, D_, none, -1);
}

template <int C, bool NT, class R, class S, class Emit>
__device__ __forceinline__ void momentum(int8_t m, bool north, const UVGridPtrs &g,
                                         const Vec<C, S> &ts, const Vec<C, S> &ps, const Vec<C, S> &u,
                                         const Vec<C, S> &v, const Vec<C, R> &vel, const Vec<C, R> &qs,
                                         const Vec<C, S> &a, int64_t j0, int64_t n, int64_t D_, Emit &emit, int slot) {
  // (the callers decide: g.mom is bound, or its value is wanted though not stored -- WantBit)
  Vec<C, R> out;
  if (m == FCX_ZERO) {
    out = splat<C, R>(R(0));
  } else if (m == FCX_CCLM || m == FCX_MOM5) {
    FOR_C {
      const R rate = mom_cclm_rate<R>(a.v[i], ps.v[i], qs.v[i], ts.v[i], vel.v[i]);
      out.v[i] = -(rate * R(north ? v.v[i] : u.v[i]));
    }
  } else if (m == FCX_RCO) {
    FOR_C {
      const R rate = mom_rco_rate<R>(vel.v[i]);
      out.v[i] = -(rate * R(north ? v.v[i] : u.v[i]));
    }
  } else {
    return;
  }
  if (g.mom) ST(g.mom, j0, n, out);
  if (slot >= 0) emit(slot, out);
}

// QSUR + momentum on one separate u or v grid (non-merged layout).
// TM = 1: one wait for the grid's inputs before its first store (process, wait_inputs).
// SKIP: QSUR of the grid may be wanted (by its momentum) though not stored (Methods::want).
template <int C, bool NT, class R, class S, int TM, bool UNI, bool SKIP, bool CR = false>
__device__ __forceinline__ void uv_grid(const TypeParams &tp, const Methods &mt, int k, uint32_t stages, int64_t j0,
                                        int64_t n, int64_t D_) {
  const UVGridPtrs &g = tp.uv[k];
  const uint32_t s_qsur = k == 0 ? S_QSUR_U : S_QSUR_V;
  const uint32_t s_mom = k == 0 ? S_UMOM : S_VMOM;
  const bool want_q = SKIP && (mt.want & (k == 0 ? W_QSUR_U : W_QSUR_V));
  const bool do_q = (stages & s_qsur) && mt.qsur[1 + k] == FCX_CCLM && (g.qsur || want_q);
  const bool do_m = (stages & s_mom) && g.mom;
  if (!do_q && !do_m) return;
  Vec<C, S> ts = {}, fi = {}, ps = {}, u = {}, v = {}, a = {};
  Vec<C, R> qs = {};
  const uint32_t cm = UNI ? mt.cmask >> (kUvBit0 + kUvBits * k) : 0u;  // this grid's bits
  if (g.tsur || cbit(cm, KU_TSUR)) ts = LDU(g.tsur, cbit(cm, KU_TSUR), j0, n);
  if (g.psur || cbit(cm, KU_PSUR)) ps = LDU(g.psur, cbit(cm, KU_PSUR), j0, n);
  // every load is guarded by its own pointer, whatever the method says: a method whose input
  // the planner left unbound reads nothing (plan_audit at plan build names that case as an
  // error before any launch; round-5 fault: 'zero' momentum loaded unbound winds)
  if (do_q && (g.fice || cbit(cm, KU_FICE))) fi = LDU(g.fice, cbit(cm, KU_FICE), j0, n);
  if (do_m) {  // ('zero' momentum binds no wind: the planner leaves uatm / vatm unset)
    if (g.uatm || cbit(cm, KU_UATM)) u = LDU(g.uatm, cbit(cm, KU_UATM), j0, n);
    if (g.vatm || cbit(cm, KU_VATM)) v = LDU(g.vatm, cbit(cm, KU_VATM), j0, n);
    if (mt.mom == FCX_CCLM && (g.amom || cbit(cm, KU_AMOM))) a = LDU(g.amom, cbit(cm, KU_AMOM), j0, n);
    if (mt.mom == FCX_MOM5 && (g.cmom || cbit(cm, KU_CMOM))) a = LDU(g.cmom, cbit(cm, KU_CMOM), j0, n);
    if (g.qsur_in && !do_q) qs = cvt<R>(LD(g.qsur_in, j0, n));
  }
  if constexpr (TM == 1) wait_inputs();
  if (do_q) {
    FOR_C qs.v[i] = qsur_cclm<R, CR>(fi.v[i], ps.v[i], ts.v[i]);
    if (g.qsur) ST(g.qsur, j0, n, qs);
  }
  if (do_m) {
    Vec<C, R> vel;
    FOR_C vel.v[i] = wind<R>(u.v[i], v.v[i]);
    momentum<C, NT, R, S>(mt.mom, k == 1, g, ts, ps, u, v, vel, qs, a, j0, n, D_);
  }
}

// LDS accumulators of the register-average slots: each lane owns C contiguous values per
// slot (16 B), slot k at base + k * stride.  Private to the lane, so no synchronisation;
// they keep 7 x C values out of the VGPR budget of the multi-type kernels.
template <int C, class R>
struct AccLds {
  R *base;
  int stride;  // elements between slots
  __device__ __forceinline__ Vec<C, R> get(int k) const {
    Vec<C, R> r;
#pragma unroll
    for (int i = 0; i < C; ++i) r.v[i] = base[k * stride + i];
    return r;
  }
  __device__ __forceinline__ void set(int k, const Vec<C, R> &x) const {
#pragma unroll
    for (int i = 0; i < C; ++i) base[k * stride + i] = x.v[i];
  }
};

// Where a produced flux goes besides its own array.  RAVG: X_s * FARE_s is added to the
// type-0 accumulator of its slot (type order, from 0.0 -- calc:377-383) and the averages
// go to the emitter (the fused atmosphere accumulation) once all types are done; without
// RAVG the value of the single surface type goes to the emitter.
template <int C, class R, class S, bool RAVG, class Emit>
struct Sink {
  const Emit &emit;
  const AvgRegs &ra;
  AccLds<C, R> acc;
  Vec<C, S> fare;
  __device__ __forceinline__ Sink(const Emit &e, const AvgRegs &r, AccLds<C, R> a) : emit(e), ra(r), acc(a) {
    if constexpr (RAVG) {
#pragma unroll
      for (int k = 0; k < kAvgSlots; ++k)
        if (ra.out[k]) acc.set(k, splat<C, R>(R(0)));
    }
  }
  template <class X>  // X: R (a flux just computed) or S (a held input: TSUR)
  __device__ __forceinline__ void operator()(int k, const Vec<C, X> &x) {
    if constexpr (RAVG) {
      if (ra.out[k]) {
        Vec<C, R> a = acc.get(k);
#pragma unroll
        for (int i = 0; i < C; ++i) a.v[i] = a.v[i] + R(x.v[i]) * R(fare.v[i]);
        acc.set(k, a);
      }
    } else {
      if (k < kFusedFields) emit(k, x);
    }
  }
};

// Remap records (Params::rec): every flux of register slot k the T=1 launch produces is also
// stored at position rec_pos[k] of its cell's record, so that a remap of those fields
// gathers one record per link without a packing pass (fcx_engine.hip plan_fused_records).
template <int C, class R, class Inner>
struct RecEmit {
  const Inner &inner;
  R *rec;             // record of the lane's first cell
  int P;              // elements per record
  uint64_t posw;      // Params::rec_pos (wave-uniform) as one word, position k in byte k
  int nv;             // cells of the lane inside the grid
  mutable R vals[6][C];  // the values stay in registers and each record goes out as 16-B stores
  __device__ __forceinline__ int pos(int k) const { return byte_of(posw, k); }
  template <int CC, class RR>
  __device__ __forceinline__ void operator()(int k, const Vec<CC, RR> &x) const {
    inner(k, x);
    if (k < 6) {
#pragma unroll
      for (int i = 0; i < CC; ++i) vals[k][i] = x.v[i];
    }
  }
  __device__ __forceinline__ void flush() const {
    constexpr int V = 16 / sizeof(R);
#pragma unroll
    for (int i = 0; i < C; ++i) {
      if (i >= nv) break;
#pragma unroll
      for (int q = 0; q < 6 / V; ++q) {
        if (q * V >= P) break;
        using VecT = typename std::conditional<sizeof(R) == 8, d2, f4>::type;
        VecT t;
#pragma unroll
        for (int h = 0; h < V; ++h) {
          R v = R(0);
#pragma unroll
          for (int k = 0; k < 6; ++k)
            if (pos(k) == q * V + h) v = vals[k][i];
          t[h] = v;
        }
        *gptr(reinterpret_cast<VecT *>(rec + i * P + q * V)) = t;
      }
    }
  }
};

// VAR: 0 = generic (methods read from the parameter block); 1/2/3 = the CCLM / MOM5 / RCO
// variant with the QSUR/MEVA/HSEN/momentum methods of every surface type fixed at compile
// time, so the other method paths vanish from the code and its register budget.  Any T.
// Inputs shared by consecutive surface types (the atmosphere fields are aliased into every
// type, basic:334-358) are loaded once: a type reloads an input only when its pointer
// differs from the previous type's (wave-uniform scalar compare).  Inputs are never written
// by the pass, so a held value is the array's value.
// TM: 1 = one surface type, fixed at compile time (the held inputs and the type loop
// vanish); 0 = T from the parameter block.  RAVG (register averages) needs TM = 0; every
// precision has it, with and without the fused accumulation.
// HALO: cells at or past st_end are a halo tile's head cells -- their fluxes are computed for
// the fused accumulation's products, nothing of them is stored (the next tile's wave stores).
// PR: the precision (double, float or F32Wide): R its arithmetic and S its storage type.  The
// inputs are held in S and widened where a formula takes them (the formulas are called as
// f<R>(...), so a float argument converts on the way in); what the pass computes is held in R.
template <int C, bool MERGED, int VAR, bool NT, class PR = double, int TM = 1, bool RAVG = false,
          class Emit = NoEmit, bool REC = false, bool HALO = false>
__device__ __forceinline__ void process(const Params *__restrict__ P, const double *__restrict__ corr_m,
                                        int64_t j0, const Emit &emit_in = Emit(),
                                        AccLds<C, typename Prec<PR>::arith> acc_lds =
                                            AccLds<C, typename Prec<PR>::arith>{nullptr, 0},
                                        int64_t st_end = 0) {
  using R = typename Prec<PR>::arith;
  using S = typename Prec<PR>::store;
  constexpr bool kCr = is_cr<PR>();  // the transcendental sites: correctly rounded
  static_assert(!(RAVG && TM), "register averages need more than one surface type");
  static_assert(!REC || (TM == 1 && !RAVG), "remap records: the T=1 launch");
  static_assert(!REC || std::is_same<R, S>::value, "remap records: the fp64 engine");
  static_assert(!HALO || (TM == 1 && !RAVG), "halo tiles: the T=1 launch");
  const uint32_t stages = P->stages;
  const int T = TM ? 1 : P->num_types;
  const int64_t nt = P->n[0];
  const int64_t ns = HALO ? min(nt, st_end) : nt;  // stores of the t-grid (and merged u/v) cells
  const bool do_t = j0 < nt;
  using SinkEmit = typename std::conditional<REC, RecEmit<C, R, Emit>, const Emit &>::type;
  SinkEmit emit = [&]() -> SinkEmit {
    if constexpr (REC) {
      // (4-B aligned: two scalar words, like type_methods)
      const FCX_CONSTANT word4_t *pw = (const FCX_CONSTANT word4_t *)&P->rec_pos[0];
      const uint64_t posw = (uint64_t)pw[0] | ((uint64_t)pw[1] << 32);
      return RecEmit<C, R, Emit>{emit_in, reinterpret_cast<S *>(P->rec) + j0 * P->rec_p, P->rec_p, posw,
                                 (int)max((int64_t)0, min((int64_t)C, ns - j0))};
    } else {
      return emit_in;
    }
  }();
  const int64_t D_ = (j0 >> kLayoutShift) * P->tpad;  // field layout shift of this lane's cells
  Vec<C, S> corr = {};  // the month slice is a plain contiguous array
  if (do_t && corr_m && (stages & S_MEVA)) corr = ld<C, NT, S>(reinterpret_cast<const S *>(corr_m), j0, nt);
  Vec<C, S> rsdd = {};
  if (do_t && P->rsdd0 && (stages & S_RSDR)) rsdd = LD(P->rsdd0, j0, nt);
  Sink<C, R, S, RAVG, typename std::remove_cv<typename std::remove_reference<SinkEmit>::type>::type> sink(
      emit, P->ravg, acc_lds);

  // inputs held across surface types, with the pointer they were loaded from
  Vec<C, S> ts = {}, fi = {}, ps = {}, pa = {}, qa = {}, ta = {}, u = {}, v = {}, amoi = {}, cmoi = {},
            chea = {}, amom = {}, cmom = {};
  Vec<C, R> vel = {};
  const double *h_ts = nullptr, *h_fi = nullptr, *h_ps = nullptr, *h_pa = nullptr, *h_qa = nullptr,
               *h_ta = nullptr, *h_u = nullptr, *h_v = nullptr, *h_amoi = nullptr, *h_cmoi = nullptr,
               *h_chea = nullptr, *h_amom = nullptr, *h_cmom = nullptr;
  // With T from the parameter block (TM = 0) the bottom-side inputs (TSUR FICE CMOI CHEA
  // CMOM) are reloaded for every type, and the atmosphere-side inputs (PSUR PATM QATM TATM
  // UATM VATM AMOI AMOM, aliased into every surface type by distribute_input_field,
  // basic:334-358) are held across the types and reloaded only when a type binds another
  // array (a wave-uniform pointer compare).  Measured at T = 2 (profiles/r02/t2_reload_ab):
  // the per-type reloads of the shared fields cost 8 % of the step; holding them costs 36
  // VGPRs, so the multi-type fused kernels run 3 instead of 4 waves per SIMD and still gain
  // 6-7 % per step.  Holding every input (round 1) kept ~56 VGPRs live and lost.
  constexpr bool kReload = TM == 0;  // bottom-side inputs: loaded per type
  // grp.member names the pointer in TypeParams.  ATM: an atmosphere-side input (held).
  // A held input is the pair (member bytes, constant bit): an array and a constant never compare
  // equal even where a value's bits look like an address, and two constants differ by their
  // bits.  h_cm holds the constant bits of the held inputs (wave-uniform, scalar registers).
  constexpr bool kUni = uniform_inputs<S, VAR, RAVG>();
  // (fcx_internal.h: the planner's rule too)
  constexpr bool kSkip = skip_family(sizeof(S) == 4, VAR, RAVG, TM == 1, MERGED, HALO);
  uint32_t h_cm = 0, cm = 0;  // cm: the current type's TypeParams::cmask
  auto is_new = [&](const double *ptr_, const double *held, int bit) {
    if constexpr (!kUni) return ptr_ && ptr_ != held;
    const bool c_ = cbit(cm, bit);
    return (ptr_ || c_) && (ptr_ != held || c_ != cbit(h_cm, bit));
  };
  auto hold = [&](int bit) {
    if constexpr (kUni) h_cm = (h_cm & ~(1u << bit)) | ((uint32_t)cbit(cm, bit) << bit);
  };
#define HOLDX(var, grp, member, ATM, bit)             \
  {                                                   \
    const double *ptr_ = tp.grp.member;               \
    if constexpr (kReload && !ATM) {                  \
      if (ptr_ || cbit(cm, bit)) var = LDU(ptr_, cbit(cm, bit), j0, nt); \
    } else if (is_new(ptr_, h_##var, bit)) {          \
      var = LDU(ptr_, cbit(cm, bit), j0, nt);         \
      h_##var = ptr_;                                 \
      hold(bit);                                      \
    }                                                 \
  }
#define HOLD(var, grp, member, bit) HOLDX(var, grp, member, false, bit)
#define HOLDA(var, grp, member, bit) HOLDX(var, grp, member, true, bit)
  // Next-type prefetch (multi-type kernels): the bottom-side inputs of type s+1 (TSUR FICE
  // CMOI CHEA CMOM and the FARE of the averages) are loaded when type s starts, so that the
  // wave does not stall on memory between two types.  The fused T = 2 kernels then hold
  // 162 / 166 / 124 VGPRs (CCLM / MOM5 / RCO, was 150 / 144 / 116): still 3 / 3 / 4 waves per
  // SIMD, no spills.  In one process over the same arrays (profiles/r03/ab_t2_prefetch.json,
  // random map): T = 2 step 1.672 -> 1.625 ms, CCLM 5.14 -> 5.26 TB/s, MOM5 5.54 -> 5.67,
  // RCO 5.26 -> 5.50.
  constexpr bool kPrefetch = kReload;
  // Multi-type CCLM / MOM5 kernels: the atmosphere-only terms of the formulas are formed once
  // per cell, when the type's atmosphere fields are (re)loaded, instead of once per type:
  // T_a * EF (HSEN's pow, ta_exner) and, for CCLM, whose coefficients AMOI / AMOM are
  // atmosphere fields too, a * max(vel, u_min) * p_s (MEVA, HSEN) and a * vel * p_s
  // (momentum).  Same operations on the same values, so the same bits (fcx_physics.h); the
  // type loop loses its pow and PATM / AMOI / AMOM / the wind speed need not stay live.
  // (round 4, in one process over the same arrays, profiles/r04/ab/ab_derive_t2.json: T = 2 step
  // 1.665 -> 1.628 ms, MOM5 0.616 -> 0.582 ms, CCLM 0.595 -> 0.588 ms)
  constexpr bool kDerive = TM == 0 && (VAR == 1 || VAR == 2);
  Vec<C, R> taef = {}, amv = {}, mvp = {};
  Vec<C, S> n_ts = {}, n_fi = {}, n_cmoi = {}, n_chea = {}, n_cmom = {}, n_fare = {};
  auto prefetch = [&](int s2) {
    const TypeParams &q = P->type[s2];
    const uint32_t qm = kUni ? type_cmask(q) : 0u;
    if (q.t.tsur || cbit(qm, K_TSUR)) n_ts = LDU(q.t.tsur, cbit(qm, K_TSUR), j0, nt);
    if (q.t.fice || cbit(qm, K_FICE)) n_fi = LDU(q.t.fice, cbit(qm, K_FICE), j0, nt);
    if (q.t.cmoi || cbit(qm, K_CMOI)) n_cmoi = LDU(q.t.cmoi, cbit(qm, K_CMOI), j0, nt);
    if (q.t.chea || cbit(qm, K_CHEA)) n_chea = LDU(q.t.chea, cbit(qm, K_CHEA), j0, nt);
    if constexpr (MERGED) {
      if (q.uv[0].cmom || cbit(qm, kUvBit0 + KU_CMOM)) n_cmom = LDU(q.uv[0].cmom, cbit(qm, kUvBit0 + KU_CMOM), j0, nt);
    }
    if constexpr (RAVG) {
      if (P->ravg_on && P->ravg.fare[s2]) n_fare = LD(P->ravg.fare[s2], j0, nt);
    }
  };
  if constexpr (kPrefetch) {
    if (do_t) prefetch(0);
  }

  // The wide fused register-average kernels: the type index said wave-uniform to the compiler
  // (readfirstlane, as cells_atmos_group_kernel says of its member index).  Left to itself it
  // kept the loop counter of these instantiations in a VGPR, and every pointer of P->type[s] --
  // the inputs' and outputs' addresses, the next type's for the prefetch -- was an 8-B vector
  // load from the parameter block with a full vmcnt(0) wait behind it, a dependent round trip
  // per array: 75 vector loads per wave and type pair where the fp64 kernel issues 22, and a
  // T = 2 group launch of 2.065 ms against the fp64 engine's 1.571.
  constexpr bool kUniformType = RAVG && is_wide<PR>() && !std::is_same<Emit, NoEmit>::value;
  for (int s_ = 0; s_ < T; ++s_) {
    const int s = kUniformType ? __builtin_amdgcn_readfirstlane(s_) : s_;
    if constexpr (kReload) {  // no bottom-side input of the previous type stays live
      ts = fi = cmoi = chea = cmom = Vec<C, S>{};
    }
    const TypeParams &tp = P->type[s];
    const TGridPtrs &g = tp.t;
    const Methods mt = type_methods(tp);
    cm = kUni ? mt.cmask : 0u;
    // outputs of this type a consumer in the launch wants though their store pointer is null
    // (wave-uniform, in scalar registers with the method bytes; a compile-time zero elsewhere)
    const uint32_t want = kSkip ? mt.want : 0u;
    constexpr int8_t kVarMethod = VAR == 1 ? FCX_CCLM : VAR == 2 ? FCX_MOM5 : FCX_RCO;
    const int8_t m_q = VAR ? (VAR == 3 ? FCX_NONE : FCX_CCLM) : mt.qsur[0];
    const int8_t m_qu = VAR ? m_q : mt.qsur[1];
    const int8_t m_qv = VAR ? m_q : mt.qsur[2];
    const int8_t m_me = VAR ? kVarMethod : mt.meva;
    const int8_t m_hs = VAR ? kVarMethod : mt.hsen;
    const int8_t m_mo = VAR ? kVarMethod : mt.mom;
    if (do_t) {
      // ---- every t-grid input this type needs (before any store of this type)
      Vec<C, R> qs = {}, me = {};
      if constexpr (kPrefetch) {
        ts = n_ts;
        fi = n_fi;
        cmoi = n_cmoi;
        chea = n_chea;
        cmom = n_cmom;
        if constexpr (RAVG) sink.fare = n_fare;
        if (s + 1 < T) prefetch(s + 1);
      } else {
        HOLD(ts, t, tsur, K_TSUR)
        HOLD(fi, t, fice, K_FICE)
      }
      // which derived atmosphere terms this type must (re)form: its fields differ from the held ones
      const bool wind_new = is_new(g.uatm, h_u, K_UATM) || is_new(g.vatm, h_v, K_VATM);
      bool d_ef = false, d_amv = false, d_mvp = false;
      if constexpr (kDerive) {
        const bool ps_new = is_new(g.psur, h_ps, K_PSUR);
        d_ef = ps_new || is_new(g.patm, h_pa, K_PATM) || is_new(g.tatm, h_ta, K_TATM);
        if constexpr (VAR == 1) {
          d_amv = ps_new || wind_new || is_new(g.amoi, h_amoi, K_AMOI);
          d_mvp = ps_new || wind_new || is_new(tp.uv[0].amom, h_amom, kUvBit0 + KU_AMOM);
        }
      }
      HOLDA(ps, t, psur, K_PSUR)
      if constexpr (!kDerive) HOLDA(pa, t, patm, K_PATM)
      HOLDA(qa, t, qatm, K_QATM)
      HOLDA(ta, t, tatm, K_TATM)
      HOLDA(u, t, uatm, K_UATM)
      HOLDA(v, t, vatm, K_VATM)
      if constexpr (!(kDerive && VAR == 1)) HOLDA(amoi, t, amoi, K_AMOI)
      if constexpr (kDerive) {
        if (d_ef) {
          Vec<C, S> pa_l = {};
          if (g.patm || cbit(cm, K_PATM)) pa_l = LDU(g.patm, cbit(cm, K_PATM), j0, nt);
          h_pa = g.patm;
          hold(K_PATM);
          FOR_C taef.v[i] = ta_exner<R, kCr>(ta.v[i], ps.v[i], pa_l.v[i]);
        }
        if constexpr (VAR == 1) {
          if (d_amv || d_mvp) {
            Vec<C, R> w;  // the wind speed, only to form the two factors
            FOR_C w.v[i] = wind<R>(u.v[i], v.v[i]);
            if (d_amv) {
              Vec<C, S> am = {};
              if (g.amoi || cbit(cm, K_AMOI)) am = LDU(g.amoi, cbit(cm, K_AMOI), j0, nt);
              h_amoi = g.amoi;
              hold(K_AMOI);
              FOR_C amv.v[i] = rate_num<R>(am.v[i], w.v[i], ps.v[i]);
            }
            if (d_mvp) {
              Vec<C, S> am = {};
              if (tp.uv[0].amom || cbit(cm, kUvBit0 + KU_AMOM))
                am = LDU(tp.uv[0].amom, cbit(cm, kUvBit0 + KU_AMOM), j0, nt);
              h_amom = tp.uv[0].amom;
              hold(kUvBit0 + KU_AMOM);
              FOR_C mvp.v[i] = mom_num<R>(am.v[i], w.v[i], ps.v[i]);
            }
          }
        }
      }
      if constexpr (!kPrefetch) {
        HOLD(cmoi, t, cmoi, K_CMOI)
        HOLD(chea, t, chea, K_CHEA)
      }
      if (g.qsur_in) qs = cvt<R>(LD(g.qsur_in, j0, nt));  // may be written by this pass: never held
      if (g.meva_in) me = cvt<R>(LD(g.meva_in, j0, nt));
      if constexpr (MERGED) {
        if constexpr (!(kDerive && VAR == 1)) HOLDA(amom, uv[0], amom, kUvBit0 + KU_AMOM)
        if constexpr (!kPrefetch) HOLD(cmom, uv[0], cmom, kUvBit0 + KU_CMOM)
      }
      if constexpr (!(kDerive && VAR == 1)) {
        if (wind_new) FOR_C vel.v[i] = wind<R>(u.v[i], v.v[i]);
      }
      if constexpr (RAVG) {
        if constexpr (!kPrefetch) {
          if (P->ravg_on && P->ravg.fare[s]) sink.fare = LD(P->ravg.fare[s], j0, nt);
        }
        sink(A_TSUR, ts);
      }

      // ---- every input of the type has been requested.  The loads above sit in conditional code
      // (null pointers, the partial-vector path), so in each conditional flux block below the
      // compiler still counts them as possibly pending and, stores counting in vmcnt like
      // loads, waits vmcnt(0) at the block's first use of an input: for the stores of the
      // blocks before it as well.  One wait here, in code that dominates every flux block of
      // the type, and the blocks need none: the stores issue with the arithmetic.  (TM = 0
      // keeps the compiler's waits: a full wait here would also retire the next-type prefetch.)
      if constexpr (TM == 1) wait_inputs();
      // ---- calc_flux_radiation_blackbody (calc:331-343)
      // (every flux block below: run when its output is stored OR wanted though not stored --
      // WantBit --, and only the store is guarded by the pointer)
      if ((stages & S_RBBR) && (g.rbbr || (want & W_RBBR))) {
        Vec<C, R> r;
        if (mt.rbbr == FCX_STBO) {
          FOR_C r.v[i] = rbbr_stbo<R>(ts.v[i]);
          if (g.rbbr) ST(g.rbbr, j0, ns, r);
          sink(A_RBBR, r);
        } else if (mt.rbbr == FCX_ZERO) {
          r = zeros<C, R, TM == 1>();
          if (g.rbbr) ST(g.rbbr, j0, ns, r);
          sink(A_RBBR, r);
        }
      }
      // ---- calc_spec_vapor_surface(t) (calc:37-49)
      if ((stages & S_QSUR_T) && m_q == FCX_CCLM) {
        FOR_C qs.v[i] = qsur_cclm<R, kCr>(fi.v[i], ps.v[i], ts.v[i]);
        if (g.qsur) ST(g.qsur, j0, ns, qs);
      }
      // ---- calc_flux_mass_evap (calc:75-118), P2: TATM in the T_s slot
      if (stages & S_MEVA) {
        const int8_t m = m_me;
        bool have = true;
        if (m == FCX_ZERO) {
          me = zeros<C, R, TM == 1>();
        } else if (m == FCX_CCLM || m == FCX_MOM5) {
          if constexpr (kDerive && VAR == 1) {
            FOR_C me.v[i] = meva_cclm_num<R>(amv.v[i], qa.v[i], qs.v[i], ta.v[i]);
          } else {
            const Vec<C, S> &a = (m == FCX_CCLM) ? amoi : cmoi;
            FOR_C me.v[i] = meva_cclm<R>(a.v[i], ps.v[i], qa.v[i], qs.v[i], ta.v[i], vel.v[i]);
          }
        } else if (m == FCX_RCO) {
          FOR_C me.v[i] = meva_rco<R, kCr>(qa.v[i], ts.v[i], vel.v[i]);
        } else {
          have = false;  // none / copy
        }
        if (have) {
          for (int b = 0; b < mt.bias_adds; ++b) {
            FOR_C me.v[i] = me.v[i] + R(corr.v[i]);
          }
          if (g.meva) ST(g.meva, j0, ns, me);
          sink(A_MEVA, me);
        }
      }
      // ---- calc_flux_heat_latent (calc:135-152)
      if ((stages & S_HLAT) && (g.hlat || (want & W_HLAT))) {
        Vec<C, R> h;
        if (mt.hlat == FCX_WATER) {
          FOR_C h.v[i] = me.v[i] * R(kLv);
          if (g.hlat) ST(g.hlat, j0, ns, h);
        } else if (mt.hlat == FCX_ICE) {
          FOR_C h.v[i] = me.v[i] * R(kLs);
          if (g.hlat) ST(g.hlat, j0, ns, h);
        } else if (mt.hlat == FCX_ZERO) {
          h = zeros<C, R, TM == 1>();
          if (g.hlat) ST(g.hlat, j0, ns, h);
        }
        if (mt.hlat == FCX_WATER || mt.hlat == FCX_ICE || mt.hlat == FCX_ZERO) sink(A_HLAT, h);
      }
      // ---- calc_flux_heat_sensible (calc:167-206), P3: QATM in the q_s slot
      if ((stages & S_HSEN) && (g.hsen || (want & W_HSEN))) {
        const int8_t m = m_hs;
        Vec<C, R> h;
        if (m == FCX_CCLM || m == FCX_MOM5) {
          if constexpr (kDerive && VAR == 1) {
            FOR_C h.v[i] = hsen_cclm_num<R>(amv.v[i], qa.v[i], ts.v[i], taef.v[i]);
          } else if constexpr (kDerive) {
            FOR_C h.v[i] = hsen_cclm_num<R>(rate_num<R>(chea.v[i], vel.v[i], ps.v[i]), qa.v[i], ts.v[i], taef.v[i]);
          } else {
            const Vec<C, S> &a = (m == FCX_CCLM) ? amoi : chea;
            FOR_C h.v[i] = hsen_cclm<R, kCr>(a.v[i], pa.v[i], ps.v[i], qa.v[i], ta.v[i], ts.v[i], vel.v[i]);
          }
          if (g.hsen) ST(g.hsen, j0, ns, h);
        } else if (m == FCX_RCO) {
          FOR_C h.v[i] = hsen_rco<R>(ta.v[i], ts.v[i], vel.v[i]);
          if (g.hsen) ST(g.hsen, j0, ns, h);
        } else if (m == FCX_ZERO) {
          h = zeros<C, R, TM == 1>();
          if (g.hsen) ST(g.hsen, j0, ns, h);
        }
        if (m == FCX_CCLM || m == FCX_MOM5 || m == FCX_RCO || m == FCX_ZERO) sink(A_HSEN, h);
      }
      if constexpr (MERGED) {
        // u and v grids ARE the t grid: QSUR(u/v) = QSUR(t) (same inputs, same method),
        // one wind speed and one exchange rate serve UMOM and VMOM.
        for (int k = 0; k < 2; ++k) {
          const UVGridPtrs &gk = tp.uv[k];
          const uint32_t s_qsur = k == 0 ? S_QSUR_U : S_QSUR_V;
          if ((stages & s_qsur) && (k == 0 ? m_qu : m_qv) == FCX_CCLM &&
              (gk.qsur || (want & (k == 0 ? W_QSUR_U : W_QSUR_V)))) {
            if (!((stages & S_QSUR_T) && m_q == FCX_CCLM)) {
              FOR_C qs.v[i] = qsur_cclm<R, kCr>(fi.v[i], ps.v[i], ts.v[i]);
            }
            if (gk.qsur) ST(gk.qsur, j0, ns, qs);
          }
        }
        const bool do_u = (stages & S_UMOM) && (tp.uv[0].mom || (want & W_UMOM));
        const bool do_v = (stages & S_VMOM) && (tp.uv[1].mom || (want & W_VMOM));
        if (do_u || do_v) {
          if constexpr (kDerive && VAR == 1) {  // CCLM: the rate from a * vel * p_s formed once
            Vec<C, R> rate;
            FOR_C rate.v[i] = mom_cclm_rate_num<R>(mvp.v[i], qs.v[i], ts.v[i]);
            for (int k = 0; k < 2; ++k) {
              if (!(k ? do_v : do_u)) continue;
              Vec<C, R> out;
              FOR_C out.v[i] = -(rate.v[i] * R(k ? v.v[i] : u.v[i]));
              if (tp.uv[k].mom) ST(tp.uv[k].mom, j0, ns, out);
              sink(k ? A_VMOM : A_UMOM, out);
            }
          } else {
            const Vec<C, S> &a = (m_mo == FCX_MOM5) ? cmom : amom;
            if (do_u) momentum<C, NT, R, S>(m_mo, false, tp.uv[0], ts, ps, u, v, vel, qs, a, j0, ns, D_, sink, A_UMOM);
            if (do_v) momentum<C, NT, R, S>(m_mo, true, tp.uv[1], ts, ps, u, v, vel, qs, a, j0, ns, D_, sink, A_VMOM);
          }
        }
      }
      // ---- distribute_shortwave_radiation_flux (calc:355-362): RSDR_s = RSDD_0
      if ((stages & S_RSDR) && g.rsdr) ST(g.rsdr, j0, ns, rsdd);
    }
    if constexpr (!MERGED) {
      if (j0 < P->n[1]) uv_grid<C, NT, R, S, TM, kUni, kSkip, kCr>(tp, mt, 0, stages, j0, P->n[1], D_);
      if (j0 < P->n[2]) uv_grid<C, NT, R, S, TM, kUni, kSkip, kCr>(tp, mt, 1, stages, j0, P->n[2], D_);
    }
  }
#undef HOLD
#undef HOLDA
#undef HOLDX

  if constexpr (REC) emit.flush();
  // ---- average_across_surface_types (calc:376-383), summed in type order
  if constexpr (RAVG) {
    if (do_t) {
#pragma unroll
      for (int k = 0; k < kAvgSlots; ++k) {
        if (!P->ravg.out[k]) continue;
        const Vec<C, R> avg = sink.acc.get(k);
        ST(P->ravg.out[k], j0, ns, avg);
        if (k < kFusedFields) emit(k, avg);  // the type-0 field OASIS sends on
      }
    }
  }
  if (stages & S_AVG) {
    for (int e = 0; e < P->num_avg; ++e) {
      const AvgEntry &ae = P->avg[e];
      const int64_t n = P->n[ae.grid];
      if (j0 >= n) continue;
      Vec<C, R> acc = splat<C, R>(R(0));
      if (!ae.x0) continue;  // (plan_audit: every entry binds x0, x[s] and fare[s])
      for (int s = 0; s < T; ++s) {
        if (!ae.x[s] || !ae.fare[s]) continue;
        const Vec<C, S> x = LD(ae.x[s], j0, n);  // (the stored value, widened)
        const Vec<C, S> f = LD(ae.fare[s], j0, n);
        FOR_C acc.v[i] = acc.v[i] + R(x.v[i]) * R(f.v[i]);
      }
      ST(ae.x0, j0, HALO ? min(n, st_end) : n, acc);
    }
  }
}

// cells [lo, hi) of the plan (lo a multiple of C), grid-stride over C-cell units
template <int C, bool MERGED, int VAR, bool NT, class PR, int TM, bool RAVG, bool REC = false>
// (wide register averages: 56 KiB of fp64 accumulators per block at 4 cells per lane, 2 blocks per CU)
// (F64Cr: the double-double sites of two cells hold ~240 VGPRs; 2 = at most 256, no scratch)
__global__ __launch_bounds__(256, RAVG ? ((is_wide<PR>() && C == 4) || (is_cr<PR>() && VAR != 3) ? 2 : 3) : 1) void cells_kernel(const Params *__restrict__ P,
                                                    const double *__restrict__ corr_m, int64_t lo,
                                                    int64_t hi) {
  const int64_t u_end = (hi + C - 1) / C;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // register-average accumulators: [slot][thread][C] (16 B per lane and slot, conflict-free;
  // in the arithmetic type: a wide average is formed from the unrounded fluxes, 32 B per lane)
  using R = typename Prec<PR>::arith;
  __shared__ R s_acc[RAVG ? kAvgSlots * 256 * C : 1];
  const AccLds<C, R> acc{s_acc + threadIdx.x * C, 256 * C};
  for (int64_t u = lo / C + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < u_end; u += stride)
    process<C, MERGED, VAR, NT, PR, TM, RAVG, NoEmit, REC>(P, corr_m, u * C, NoEmit(), acc);
}

// The T=1 hot path with the exchange -> atmosphere accumulation fused in (AtmosFused).
// Wave-uniform loop over 128-cell wave tiles (lane l: cells 2l, 2l+1).  Each flux is
// turned into the product w*x the moment it is produced and parked in the wave's own LDS
// region (nothing extra stays live in registers).  Segment boundaries come from two wave
// ballots of "this cell's atmosphere cell differs from the previous one": the lane holding
// a segment's first cell finds the segment end with a count-trailing-zeros, so after a
// wave-local fence it sums the segment's products from LDS in link order with a known trip
// count (no index re-reads, no dependent loop exit).  A segment that runs past the wave
// tile leaves its prefix in carry[tile].
// LDS row of one field: the products of cell e sit at slot(e) = e + 2*(e/16), i.e. one
// 16-B pad slot after every 16 cells.  Unpadded, cells 16 apart share a bank pair of the
// 16-lane ds_read2_b64 groups and the segment-start lanes (3-5 cells apart) collide; the
// pad shifts every 16-cell block by 2 banks and keeps the pair (2l, 2l+1) 16-B aligned.
// The fp32 engine's fused kernel holds C = 4 cells per lane: 256-cell wave tiles, rows of
// row_len<4>() products (the products and sums stay fp64, as in atmos_kernel).
template <int C>
constexpr int tile_cells() { return 64 * C; }
template <int C>
constexpr int row_len() { return tile_cells<C>() + 2 * (tile_cells<C>() / 16); }
__device__ __forceinline__ int lds_slot(int e) { return e + 2 * (e >> 4); }

// fp32 fields (the fp32 engine): the wave's LDS holds the fluxes themselves, [kFusedFields]
// rows of tile_cells<C>() floats, and one row of weights (fp64, lds_slot layout) behind them;
// the segment sums form w * (double)x as they read them -- the same products in the same
// order, in 4 instead of 6 row-lengths of fp64 per wave (more waves per CU).
// Several types with register averages (RAVG): the accumulators of the type-0 averages live in
// the same region, and a lane's write of its row entry may touch only what that lane has read.
//  - float arithmetic (PR = float): an accumulator is C floats, exactly the lane's row entry, so
//    the accumulators ARE the rows -- slot k of lane l at float k * tile_cells + C * l, TSUR's
//    slot 6 a seventh row -- and parking the average of slot k overwrites the lane's own
//    accumulator k in place.  The weights row and the segment list sit behind the seventh row.
//  - double arithmetic on float rows (F32Wide): an accumulator is C doubles, twice its row
//    entry, so a row write would land on other lanes' accumulators; the accumulators get a region
//    of their own behind everything else ([kAvgSlots][64 lanes][C] doubles), the six rows, the
//    weights row and the list stay where the single-type kernels have them.
// xrows: the float rows in front of the weights row (kFusedFields, or kAvgSlots in place).
template <class PR, bool RAVG>
constexpr int flux_rows() { return RAVG && !is_wide<PR>() ? kAvgSlots : kFusedFields; }
template <int C>
constexpr int xrows_doubles(int xrows = kFusedFields) { return xrows * tile_cells<C>() / 2; }
// fp32 (C = 4, up to 4 segment starts per lane): the tile's segments are summed by ordinal --
// segment s of the tile by lane s % 64 in round s / 64 -- so that each round's atmosphere
// stores are ONE contiguous run of atmosphere cells per field.  Summed by the lane holding
// its first cell (the fp64 rule, at most one start per lane there) the rounds interleave:
// round 1 takes every lane's first segment, round 2 the second ones in between, and each
// 128-B output line is written piecewise by two store instructions.  The list of the tile's
// segments sits behind the weights row: per segment its first cell and length - 1 (one byte
// each: a tile has 256 cells) and its atmosphere cell, room for one segment per cell (6 B x
// 256 = 192 doubles).  16 waves per CU then hold 156 KiB of LDS.
constexpr int kSegCap = 192;  // doubles of the list (tile_cells<4>() x (2 + 4) bytes)
// (S: the storage type -- the rows hold what the arrays hold)
template <class S, int C>
constexpr bool seg_ordinal() { return sizeof(S) == 4 && C == 4; }
// float rows: the doubles in front of the wide kernels' accumulator region (rows, weights, list)
template <class PR, int C, bool RAVG>
constexpr int acc_region_doubles() {
  return xrows_doubles<C>(flux_rows<PR, RAVG>()) + row_len<C>() +
         (seg_ordinal<typename Prec<PR>::store, C>() ? kSegCap : 0);
}
// one wave's LDS region.  fp64 rows: the product rows, which first serve as the accumulators
// (slot k = row k, TSUR in a seventh row).  float rows: see flux_rows.
template <class PR, int C, bool RAVG>
constexpr int wave_lds_doubles() {
  if (sizeof(typename Prec<PR>::store) == 8) return (RAVG ? kAvgSlots : kFusedFields) * row_len<C>();
  return acc_region_doubles<PR, C, RAVG>() + (RAVG && is_wide<PR>() ? kAvgSlots * 64 * C : 0);
}
// blocks per CU x waves x bytes per wave of a fused kernel fit the CU's 160 KiB of LDS
template <class PR, int C, bool RAVG>
constexpr bool lds_fits(int blocks, int waves) {
  return (int64_t)blocks * waves * wave_lds_doubles<PR, C, RAVG>() * 8 <= 160 * 1024;
}

// S: the storage type of the engine's fields.  A flux arrives in the arithmetic type; a float
// row parks it rounded to float (the value its array holds), whatever it was computed in.
template <int C, class S = double>
struct LdsEmitT {
  double *p;    // this wave's [kFusedFields][row_len<C>()] products (fp32: flux rows, weights)
  double w[C];  // the weights of the lane's cells
  int s;        // lds_slot(C * lane)
  template <int CC, class R>
  __device__ __forceinline__ void operator()(int k, const Vec<CC, R> &x) const {
    static_assert(CC == C, "one emitter per cell width");
    if (FCX_DBG_ATM_NOLDS) return;
    if constexpr (sizeof(S) == 4 && C == 4) {  // one 16-B store of the lane's four fluxes
      const int lane = threadIdx.x & 63;
      *reinterpret_cast<f4 *>(reinterpret_cast<float *>(p) + k * tile_cells<C>() + C * lane) =
          f4{(float)x.v[0], (float)x.v[1], (float)x.v[2], (float)x.v[3]};
      return;
    } else if constexpr (sizeof(S) == 4 && C == 2) {  // (the wide kernels' two cells: one 8-B store)
      const int lane = threadIdx.x & 63;
      *reinterpret_cast<f2v *>(reinterpret_cast<float *>(p) + k * tile_cells<C>() + C * lane) =
          f2v{(float)x.v[0], (float)x.v[1]};
      return;
    }
#pragma unroll
    for (int h = 0; h < C / 2; ++h) {  // 16-B LDS stores, w * x in fp64
      const d2 q = {w[2 * h] * (double)x.v[2 * h], w[2 * h + 1] * (double)x.v[2 * h + 1]};
      *reinterpret_cast<d2 *>(p + k * row_len<C>() + s + 2 * h) = q;
    }
  }
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lowest set bit index of m, 64 if none
__device__ __forceinline__ int first_bit(uint64_t m) { return m ? __builtin_ctzll(m) : 64; }

// XCD-aware block order.  Workgroups are dispatched round-robin over the 8 XCDs (block b on
// XCD b % 8), each XCD with its own L2.  Neighbouring tiles share the 128-B lines of the
// atmosphere outputs their segments end in; mapped to the same XCD, the two partial lines
// merge in that L2 before write-back instead of reaching memory as two partial writes.
// XCD runs (round 3): XCD x takes runs of kXcdChunk = 64 consecutive workgroups (256
// tiles), the 8 XCDs' runs side by side, so that only one tile edge in 256 is shared between
// two XCDs AND the chip streams from one window of the arrays, as the dispatch order
// advances.  Rounds 1-2 gave each XCD one contiguous eighth of the grid, b -> x * (nb / 8) +
// min(x, nb % 8) + b / 8: eight windows 1/8 of the arrays apart.  In one process over the
// same arrays, runs against eighths (profiles/r03/xcd_map_ab/): step -2.4 / -6.1 % fp64 (two
// boxes), -2.7 / -2.2 % fp32, -3.1 / -0.8 % at T = 2, -5.4 % on the periodic map.
constexpr uint32_t kXcds = 8;
constexpr uint32_t kXcdChunk = 64;  // workgroups per XCD run (fp64 kernels, 128-cell tiles)
// ... and of the fp32 kernels (256-cell tiles): 16 against 64, step -0.7 % (shared arrays) /
// -4.0 % (own mirrors), profiles/r03/xcd_map_ab/f32_*; round 5, the fp32 group launch: 32 against
// 16 -1.0 / -1.2 % (two boxes), 64 -0.2 %, and with the ordinal segment rounds -2.1 %
// (profiles/r05/ord/)
constexpr uint32_t kXcdChunkF32 = 32;
template <uint32_t K>
__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t nb) {
  constexpr uint32_t row = K * kXcds;  // runs of K workgroups per XCD, the XCDs side by side
  const uint32_t full = nb / row * row;
  if (b >= full) return b;
  const uint32_t x = b % kXcds, i = b / kXcds;
  return i / K * row + x * K + i % K;
}

// Where a finished segment sum goes: a segment that continues into the next tile leaves its
// prefix in the next tile's crossing record for atmos_fixup_kernel; a complete one is the
// atmosphere value (and the boundary slot of a first/last atmosphere cell shared with a
// neighbour rank).
// R: the engine's output type (an fp32 engine's atmosphere outputs are float, rounded once)
template <class R>
__device__ __forceinline__ void segment_done(const AtmosFused &af, int64_t tile, int32_t a, const double *acc,
                                             bool cont) {
  if (cont) {  // the next tile's crossing record: the six prefix sums, 16-B stores
#pragma unroll
    for (int q = 0; q < kFusedFields / 2; ++q)
      gptr(reinterpret_cast<d2 *>(af.xrec + (tile + 1) * kXRec))[q] = d2{acc[2 * q], acc[2 * q + 1]};
    return;
  }
  if (FCX_DBG_ATM_NOSTORE) return;
// Non-temporal atmosphere-output stores for fp64 outputs.  Since the segment sums run in
// rounds, a round writes the tile's values of a field with one instruction, and for fp64
// outputs NT stores gained 3.4-4.4 % per step (periodic / random map); fp32 outputs lost 7 %
// with them, and NT only for the lines a tile owns whole changed nothing
// (profiles/r02/nt_atm_ab/; round 1, with one store instruction per cell position, all-NT
// had lost 6.8 %).
#pragma unroll
  for (int k = 0; k < kFusedFields; ++k) {
    if (!af.out[k]) continue;
    FCX_GLOBAL R *o = gptr(reinterpret_cast<R *>(af.out[k]) + atm_at(a, af.out_stride, af.out_tpad));
    if constexpr (sizeof(R) == 8)
      __builtin_nontemporal_store((R)acc[k], o);
    else
      *o = (R)acc[k];
    if (a == 0 && af.left >= 0) gptr(af.shared)[(int64_t)af.left * af.stride + af.scol[k]] = acc[k];
    if (a == af.n_atmos - 1 && af.right >= 0) gptr(af.shared)[(int64_t)af.right * af.stride + af.scol[k]] = acc[k];
  }
}

// One round of segment sums of a halo wave tile into per-cell records (AtmosFused::rec_dense):
// lane `act` holds the six sums of the segment of atmosphere cell a.  Measured on the fused
// step's access shape (bench/map_probe.hip, profiles/r07/map_probe_records.txt): the run
// parked in the wave's LDS rows by segment ordinal and stored densely, 16 B per lane, 6.35
// TB/s against 6.20 for the six per-field runs; every start lane storing its own record as
// three 16-B stores, 5.61.  So: dense when the round's segments are consecutive atmosphere
// cells (a map without empty atmosphere cells inside the wave) and the product rows are free
// (`last`: no further round reads them); the per-lane records otherwise.
__device__ __forceinline__ void record_round(const AtmosFused &af, int32_t a, const double *acc, bool act, bool last,
                                             double *wp) {
  if (FCX_DBG_ATM_NOSTORE) return;
  const int lane = threadIdx.x & 63;
  const uint64_t am = __ballot(act);
  const int ord = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(am >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)am, 0u));
  const int cnt = __popcll(am);
  const int32_t a_first = __builtin_amdgcn_readlane(a, __builtin_amdgcn_readfirstlane(first_bit(am) & 63));
  const bool dense = last && __ballot(act && a != a_first + ord) == 0;
  if (dense) {
    wave_sync();  // every lane has read its products: the rows are free
    if (act) {
#pragma unroll
      for (int q = 0; q < kFusedFields / 2; ++q)
        reinterpret_cast<d2 *>(wp)[ord * (kFusedFields / 2) + q] = d2{acc[2 * q], acc[2 * q + 1]};
    }
    wave_sync();
    FCX_GLOBAL d2 *run = gptr(reinterpret_cast<d2 *>(af.out[0] + (int64_t)a_first * kFusedFields));
    for (int c = lane; c < cnt * (kFusedFields / 2); c += 64)
      __builtin_nontemporal_store(reinterpret_cast<const d2 *>(wp)[c], run + c);
  } else if (act) {
    FCX_GLOBAL d2 *rec = gptr(reinterpret_cast<d2 *>(af.out[0] + (int64_t)a * kFusedFields));
#pragma unroll
    for (int q = 0; q < kFusedFields / 2; ++q) __builtin_nontemporal_store(d2{acc[2 * q], acc[2 * q + 1]}, rec + q);
  }
  if (act) {
#pragma unroll
    for (int k = 0; k < kFusedFields; ++k) {
      if (a == 0 && af.left >= 0) gptr(af.shared)[(int64_t)af.left * af.stride + af.scol[k]] = acc[k];
      if (a == af.n_atmos - 1 && af.right >= 0) gptr(af.shared)[(int64_t)af.right * af.stride + af.scol[k]] = acc[k];
    }
  }
}

// blocks per CU the multi-type (RAVG) fused kernel is compiled for: 3 -> <= 168 VGPRs, room
// for the held atmosphere-side inputs (4 -> <= 128 spills them: T = 2 step +24 %).  2 gives
// the same 3 waves per SIMD (+1 VGPR): -0.7 % in one process over shared arrays, +0.5 % in
// alternating bench processes on one box (profiles/r03/ravg_blocks_ab/): 3 stays.
constexpr int kRavgAtmosBlocks = 3;
// blocks per CU the T=1 fused kernels are compiled for (1: no register cap)
constexpr int kT1AtmosBlocks = 1;
// ... and the fp32 T=1 fused CCLM / MOM5 kernels (4 cells per lane): 4 = at most 128 VGPRs,
// 4 waves per SIMD, no spills (uncapped they take 132 / 137 VGPRs and 3 waves); in one
// process over the same arrays (profiles/r03/ab_f32_4waves.json) CCLM 4.81 -> 5.19 TB/s,
// MOM5 4.73 -> 5.08.  The fp32 RCO kernel (105 VGPRs, 4 waves either way) lost 5 % under the
// cap and keeps none.
constexpr int kF32AtmosBlocks = 4;
// waves per block of the fused kernel
constexpr int kAtmosWaves = 4;
// ... and of the fp32 ones (2 paid while the fp32 rows held fp64 products, 13.8 KB/wave)
constexpr int kF32AtmosWaves = 4;
template <int C>
constexpr int atmos_waves() { return C == 4 ? kF32AtmosWaves : kAtmosWaves; }
// HALO (T = 1, full-range launches, maps whose segments are at most halo * C + 1 cells): a
// wave owns the first 64 - halo lanes' cells of its tile and computes the last `halo` lanes'
// cells -- the head of the next tile -- only for their products (nothing of them is stored),
// so every segment that starts in its own cells is summed inside the wave: no crossing
// records, no fix-up launch.  Tiles are (64 - halo) * C cells apart.
// One wave tile of the fused kernel: the fluxes of the tile's cells (process), their
// products w * x parked in the wave's LDS rows, the segment sums in rounds, the crossing
// record.  wp: the wave's LDS region.
// (HALO: 0 no, 1 halo tiles, 2 halo tiles storing per-cell records densely -- record_round)
template <int C, class PR, int VAR, bool NT, int TM, bool RAVG, bool REC, int HALO>
__device__ __forceinline__ void atmos_tile(const Params *__restrict__ P, const double *__restrict__ corr_m,
                                           const AtmosFused &af, int64_t tile, double *wp) {
  using R = typename Prec<PR>::arith;
  using S = typename Prec<PR>::store;
  constexpr int kT = tile_cells<C>();  // cells per wave tile (lane l: cells C*l .. C*l+C-1)
  constexpr int kR = row_len<C>();
  constexpr bool kXF = sizeof(S) == 4;  // LDS holds fp32 fluxes + fp64 weights
  constexpr int kWOff = xrows_doubles<C>(flux_rows<PR, RAVG>());  // float rows: the weights row
  const int64_t n = P->n_max;
  const int own_lanes = HALO ? 64 - af.halo : 64;
  const int64_t kO = (int64_t)C * own_lanes;  // cells a tile owns (HALO: lo == 0)
  const int lane = threadIdx.x & 63;
  const uint64_t at_or_above = ~0ull << lane;
  const uint64_t above = lane == 63 ? 0ull : (~0ull << (lane + 1));
    const int64_t t0 = tile * kO;
    const int64_t j0 = t0 + C * lane;
    LdsEmitT<C, S> emit{wp, {}, lds_slot(C * lane)};
    // the lane's cells in the compacted map: which start a segment (cells past the grid end
    // count as starts: they end the last real segment) and, for those, the segment's
    // atmosphere cell; the lane's C cells share one bit word (j0 is a multiple of C)
    // fp32 and fp64 halo tiles (kCompact): the compacted map -- the bit word and prefix
    // count are loaded with the inputs, the dependent loads of the segments' atmosphere cells
    // follow the flux pass, so they add no round trip before it.  fp64 with crossing records:
    // one 4-B index per cell, loaded with the inputs (the compacted map measured -2.3 % per
    // fp32 step, -0.4 / -1.1 % at T = 1 fp64 and +1.7 % at T = 2 -- its records' first-cell
    // load is a fourth dependent one -- in one process over the same arrays: profiles/r05/seg/)
    constexpr bool kCompact = compact_map(sizeof(S) == 4, HALO);
    const int sh = (int)(j0 & 31);
    uint32_t word = 0;
    int32_t before = 0;  // kCompact: segments starting before cell j0
    int32_t a[C];        // atmosphere cell (kCompact: of a segment-start cell only; -1 elsewhere)
#pragma unroll
    for (int i = 0; i < C; ++i) a[i] = -1;
    int32_t a0_tile = 0;  // kCompact, crossing records: the tile's first cell's atmosphere cell
    if constexpr (kCompact) {
      if (j0 < n) {
        word = gptr(af.seg_bits)[j0 >> 5];
        before = gptr(af.seg_pre)[j0 >> 5];
      }
      if (!HALO && af.xrec_on) a0_tile = gptr(af.tile_a0)[tile];
    } else if (j0 + C <= n) {
      const i2v ii = *gptr(reinterpret_cast<const i2v *>(af.idx + j0));
      a[0] = ii.x;
      a[1] = ii.y;
    } else {
#pragma unroll
      for (int i = 0; i < C; ++i)
        if (j0 + i < n) a[i] = gptr(af.idx)[j0 + i];
    }
    if (j0 + C <= n) {
#pragma unroll
      for (int h = 0; h < C / 2; ++h) {
        const d2 ww = __builtin_nontemporal_load(gptr(reinterpret_cast<const d2 *>(af.w + j0) + h));
        emit.w[2 * h] = ww[0];
        emit.w[2 * h + 1] = ww[1];
      }
    } else {
#pragma unroll
      for (int i = 0; i < C; ++i)
        if (j0 + i < n) emit.w[i] = gptr(af.w)[j0 + i];
    }
    const int64_t tend = t0 + kT;
    // the segment running to the tile end continues past it (wave-uniform loads)
    bool next_cont;
    int32_t prev_tile = -2;
    if constexpr (kCompact) {
      next_cont = tend < n && !((gptr(af.seg_bits)[tend >> 5] >> (tend & 31)) & 1u);
    } else {
      prev_tile = t0 > 0 ? gptr(af.idx)[t0 - 1] : -2;
      next_cont = tend < n && gptr(af.idx)[tend] == gptr(af.idx)[tend - 1];
    }
    // kCompact: the atmosphere cells of the lane's segment starts, a load that depends on the
    // bit word and the prefix count, issued after the flux pass (issued right behind the inputs'
    // wait, in flight during the arithmetic, it measured no gain: DESIGN.md section 3).
    // Kept as a lambda so that the load sequence is formed ahead of the flux pass.
    auto seg_atm_loads = [&]() {
      int32_t ord = before + __builtin_popcount(word & ((1u << sh) - 1u));
#pragma unroll
      for (int i = 0; i < C; ++i)
        if (j0 + i < n && ((word >> (sh + i)) & 1u)) a[i] = gptr(af.seg_atm)[ord++];
    };
    if (j0 < n) {
      // the lane's accumulators (RAVG; flux_rows): fp64 rows -- slot k is the lane's entry of
      // product row k; float rows, float arithmetic -- slot k is the lane's entry of flux row k;
      // float rows, double arithmetic -- a region of its own behind the rows, weights and list
      const AccLds<C, R> acc = [&]() {
        if constexpr (!kXF)
          return AccLds<C, R>{reinterpret_cast<R *>(wp + emit.s), kR};
        else if constexpr (sizeof(R) == 4)
          return AccLds<C, R>{reinterpret_cast<R *>(wp) + C * lane, kT};
        else
          return AccLds<C, R>{wp + acc_region_doubles<PR, C, RAVG>() + C * lane, 64 * C};
      }();
      process<C, true, VAR, NT, PR, TM, RAVG, LdsEmitT<C, S>, REC, (HALO != 0)>(P, corr_m, j0, emit, acc, t0 + kO);
    }
    if constexpr (kXF) {  // the weights row of the fp32 fluxes (dead cells: weight 0)
#pragma unroll
      for (int h = 0; h < C / 2; ++h)
        *reinterpret_cast<d2 *>(wp + kWOff + emit.s + 2 * h) = d2{emit.w[2 * h], emit.w[2 * h + 1]};
    }
    // cell e of the tile added to a segment sum, in link order: its products w * x
    auto add_cell = [&](double *acc, int e) {
      if constexpr (kXF) {
        const float *xr = reinterpret_cast<const float *>(wp);
        const double we = wp[kWOff + lds_slot(e)];
#pragma unroll
        for (int k = 0; k < kFusedFields; ++k) acc[k] = acc[k] + we * (double)xr[k * kT + e];
      } else {
        const double *q = wp + lds_slot(e);
#pragma unroll
        for (int k = 0; k < kFusedFields; ++k) acc[k] = acc[k] + q[k * kR];
      }
    };
    // segment starts: cell C*l+i begins a segment when its atmosphere cell differs from the
    // previous cell's (cells past the grid end also "start", which ends the last real segment)
    bool st[C];
    uint64_t m[C];
    if constexpr (kCompact) {
      seg_atm_loads();
#pragma unroll
      for (int i = 0; i < C; ++i) {
        st[i] = !(j0 + i < n) || ((word >> (sh + i)) & 1u);
        m[i] = __ballot(st[i]);
      }
    } else {
      int32_t prev = __shfl_up(a[C - 1], 1);
      if (lane == 0) prev = prev_tile;
#pragma unroll
      for (int i = 0; i < C; ++i) {
        st[i] = a[i] != (i ? a[i - 1] : prev);
        m[i] = __ballot(st[i]);
      }
    }
    wave_sync();  // the wave's LDS products are visible to all its lanes
    // Rounds of one segment start per lane (round 2): every lane with a start sums its
    // segment and stores the six values in the same round, so a tile's atmosphere stores are
    // six store instructions per round (one round when every run is >= C cells long, as on an
    // intersection grid), not six per cell position of the lane as in round 1
    // (profiles/r02/seg_rounds_ab/).
    uint32_t rem = 0;  // bit i: cell C*lane+i starts a segment not summed yet (an own cell)
#pragma unroll
    for (int i = 0; i < C; ++i)
      if (st[i] && j0 + i < n && (!HALO || lane < own_lanes)) rem |= 1u << i;
    // the end of the segment starting at cell C*lane+i: the next start of any kind (own,
    // halo, past the grid end), or the tile end
    auto seg_end = [&](int i) {
      int e_end = kT;
#pragma unroll
      for (int q = 0; q < C; ++q) e_end = min(e_end, C * first_bit(m[q] & (q > i ? at_or_above : above)) + q);
      return min(e_end, kT);
    };
    // ... of the segment starting at any cell c of the tile (the lane summing it need not hold it)
    auto seg_end_of = [&](int c) {
      const int l = c / C, i = c % C;
      const uint64_t ge = ~0ull << l, gt = l == 63 ? 0ull : (~0ull << (l + 1));
      int e_end = kT;
#pragma unroll
      for (int q = 0; q < C; ++q) e_end = min(e_end, C * first_bit(m[q] & (q > i ? ge : gt)) + q);
      return min(e_end, kT);
    };
    if constexpr (seg_ordinal<S, C>()) {
      static_assert(kT == 256 && kSegCap * 8 == kT * 6, "one list entry per cell of the tile");
      uint16_t *seg = reinterpret_cast<uint16_t *>(wp + kWOff + row_len<C>());  // [kT]
      int32_t *seg_a = reinterpret_cast<int32_t *>(seg + kT);                                 // [kT]
      const uint64_t lower = (1ull << lane) - 1;
      int total = 0, o = 0;  // the tile's segments; this lane's first one's ordinal
#pragma unroll
      for (int q = 0; q < C; ++q) {
        const uint64_t b = __ballot((rem >> q) & 1u);
        total += __popcll(b);
        o += __popcll(b & lower);
      }
#pragma unroll
      for (int i = 0; i < C; ++i)
        if ((rem >> i) & 1u) {
          seg[o] = (uint16_t)(C * lane + i);
          seg_a[o] = a[i];
          ++o;
        }
      wave_sync();
      for (int base = 0; base < total; base += 64) {
        const int sg = base + lane;
        if (sg < total) {
          const int c = seg[sg];
          const int end = seg_end_of(c);
          const int32_t ai = seg_a[sg];
          double acc[kFusedFields];
#pragma unroll
          for (int k = 0; k < kFusedFields; ++k) acc[k] = 0.0;
          for (int e = c; e < end; ++e) add_cell(acc, e);
          segment_done<S>(af, tile, ai, acc, !HALO && end == kT && next_cont);
        }
      }
      rem = 0;
    }
    // Per-cell records (AtmosFused::rec_dense, halo tiles): the round's sums are one record per
    // segment, and the segments of a wave are as a rule consecutive atmosphere cells, so the
    // wave's stores are ONE contiguous run of records (two partial 128-B lines, not two per
    // field).  record_round stores it.
    constexpr bool kDense = HALO == 2;
    static_assert(!kDense || (sizeof(S) == 8 && C == 2 && !REC && !RAVG), "dense records: the fp64 T = 1 halo launch");
    while (__ballot(rem != 0)) {
      if constexpr (kDense) {
        // every lane takes part in record_round, so the sum is written without a branch: a
        // lane without a start sums nothing that is stored (its first product is read and
        // dropped); the first cell's 0.0 + product is the loop's first step
        const bool act = rem != 0;
        const int i = act ? __builtin_ctz(rem) : 0;
        rem &= rem - 1;
        const int32_t ai = i ? a[C - 1] : a[0];
        const int c = C * lane + i;
        const int end = act ? seg_end(i) : c;
        double acc[kFusedFields];
        const double *q0 = wp + lds_slot(c);
#pragma unroll
        for (int k = 0; k < kFusedFields; ++k) acc[k] = 0.0 + q0[k * kR];
        for (int e = c + 1; e < end; ++e) add_cell(acc, e);
        record_round(af, ai, acc, act, __ballot(rem != 0) == 0, wp);
      } else if (rem) {
        const int i = __builtin_ctz(rem);
        rem &= rem - 1;
        int32_t ai = a[0];
#pragma unroll
        for (int q = 1; q < C; ++q)
          if (q == i) ai = a[q];
        const int c = C * lane + i;
        // next start after cell c: cell C*j+i' with j > l, or j == l and i' > i
        const int end = seg_end(i);
        double acc[kFusedFields];
#pragma unroll
        for (int k = 0; k < kFusedFields; ++k) acc[k] = 0.0;
        for (int e = c; e < end; ++e) add_cell(acc, e);
        // (HALO: the segment ends inside the wave's own + halo cells by the engine's rule)
        segment_done<S>(af, tile, ai, acc, !HALO && end == kT && next_cont);
      }
    }
    // the number of head cells (continuing the previous tile's segment) for
    // atmos_fixup_kernel; 0 when the tile starts a segment
    if (!HALO && af.xrec_on) {  // (a map whose segments never cross a tile needs no records)
      int head = kT;
#pragma unroll
      for (int q = 0; q < C; ++q) head = min(head, C * first_bit(m[q]) + q);
      if (FCX_DBG_NO_HEAD >= 2) head = 0;
      double *xr0 = af.xrec + tile * kXRec;
      if (lane == 0 && FCX_DBG_NO_HEAD < 2) {  // the tile's first cell: its atmosphere cell
        const int32_t a0 = kCompact ? a0_tile : a[0];
        *gptr(reinterpret_cast<i2v *>(xr0 + 30)) = i2v{head, a0};
      }
      if (FCX_DBG_NO_HEAD) head = 0;
      // the products of the first kRecHead head cells, one lane per cell, 16-B stores
      if (lane < min(head, kRecHead)) {
        double hp[kFusedFields];
        if constexpr (kXF) {
          const float *xr = reinterpret_cast<const float *>(wp);
          const double we = wp[kWOff + lds_slot(lane)];
#pragma unroll
          for (int k = 0; k < kFusedFields; ++k) hp[k] = we * (double)xr[k * kT + lane];
        } else {
#pragma unroll
          for (int k = 0; k < kFusedFields; ++k) hp[k] = wp[k * kR + lds_slot(lane)];
        }
#pragma unroll
        for (int q = 0; q < kFusedFields / 2; ++q)
          gptr(reinterpret_cast<d2 *>(xr0 + kFusedFields + lane * kFusedFields))[q] = d2{hp[2 * q], hp[2 * q + 1]};
      }
    }
    wave_sync();  // every lane is done reading before the next tile overwrites the region
}

// ... and the wide ones (F32Wide, kWideCpl = 2 cells per lane): 2 = at most 256 VGPRs, which
// leaves the compiler free -- at two cells per lane they take 79-125 VGPRs, 4 waves or more per
// SIMD, no scratch (profiles/r13/f32_math/isa/).  At four cells per lane (kWideCpl 4, measured)
// they took 172-197 and 2 waves, and 20-88 B of scratch under a cap of 3 blocks.
constexpr int kWideAtmosBlocks = 2;
template <int C, class R, int VAR, bool NT, int TM, bool RAVG, bool REC = false, int HALO = 0>
// (REC: the record stores took CCLM to 129 VGPRs and 3 waves per SIMD; capped at 4 blocks = 4 waves)
// (F64Cr, CCLM and MOM5: 2 as for the wide ones -- the correctly rounded sites of two cells
// take 241-251 VGPRs left free, and 180-250 B of scratch under the fp64 caps of 3 and 4)
__global__ __launch_bounds__(64 * atmos_waves<C>(), (is_cr<R>() && VAR != 3) ? kWideAtmosBlocks
                                                  : RAVG  ? kRavgAtmosBlocks
                                                  : REC ? 4
                                                  : is_wide<R>() ? kWideAtmosBlocks
                                                  : (C == 4 && VAR != 3) ? kF32AtmosBlocks
                                                                         : kT1AtmosBlocks) void cells_atmos_kernel(const Params *__restrict__ P,
                                                          const double *__restrict__ corr_m,
                                                          const AtmosFused af, int64_t lo, int64_t hi) {
  using S = typename Prec<R>::store;  // (R: the precision -- double, float or F32Wide)
  static_assert(sizeof(S) == 8 ? C == 2 : (C == 4 || C == 2), "fp64 rows: 2 cells per lane; fp32 flux rows: 4 or 2");
  // product rows [kFusedFields][kR]; with RAVG they first serve as the accumulators of
  // the type-0 averages (slot k = row k, TSUR in an extra row), then hold w * average
  // (float rows: the averages themselves; their accumulators: flux_rows)
  __shared__ double s_p[atmos_waves<C>()][wave_lds_doubles<R, C, RAVG>()];
  static_assert(!RAVG || lds_fits<R, C, RAVG>(kRavgAtmosBlocks, atmos_waves<C>()),
                "register averages: the launch bound's blocks per CU hold at most 160 KiB of LDS");
  static_assert(!HALO || (TM == 1 && !RAVG), "halo tiles: the T=1 launch");
  const int own_lanes = HALO ? 64 - af.halo : 64;
  const int64_t kO = (int64_t)C * own_lanes;  // cells a tile owns (HALO: lo == 0)
  const int64_t n_tiles = af.n_tiles;  // (hi + kO - 1) / kO, from the host
  const int wv = threadIdx.x >> 6;
  double *wp = s_p[wv];
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t wave0 =
      (int64_t)xcd_block<C == 4 ? kXcdChunkF32 : kXcdChunk>(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + wv;
#if FCX_WAVE_TRACE
  const int lane = threadIdx.x & 63;
  const uint64_t trace_start = (uint64_t)wall_clock64();
  uint64_t trace_loop = 0;
#endif
  for (int64_t tile = lo / kO + wave0; tile < n_tiles; tile += waves) {
#if FCX_WAVE_TRACE
    if (!trace_loop) trace_loop = (uint64_t)wall_clock64();
#endif
    atmos_tile<C, R, VAR, NT, TM, RAVG, REC, HALO>(P, corr_m, af, tile, wp);
  }
#if FCX_WAVE_TRACE
  if (af.trace) {
    __builtin_amdgcn_s_waitcnt(0);  // the wave's stores have completed
    const uint64_t trace_end = (uint64_t)wall_clock64();
    if (lane == 0) {
      const uint64_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
      const uint64_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
      u64x2 *t = reinterpret_cast<u64x2 *>(af.trace + ((int64_t)blockIdx.x * (blockDim.x >> 6) + wv) * 4);
      t[0] = u64x2{trace_start, trace_end};
      t[1] = u64x2{hw | (xcc << 32), trace_loop};
    }
  }
#endif
}


// Several engines' fused launches as ONE launch (fcx_run_group): the members' wave
// tiles side by side in one grid, [member 0's tiles][member 1's]..., each wave running the
// tile of its member with that member's parameter block, variant and accumulation.  One
// launch instead of one per engine: the ramp-up and the drain tail of a launch (~20-25 us
// each) are paid once per step, and the tail of one member's tiles
// overlaps the next member's.  Per tile the same code as cells_atmos_kernel, so the same bits.
// Blocks per CU the fp64 T = 1 group kernel is compiled for: 4 = 128 VGPRs, 4 waves per SIMD
// like the members' own kernels (left free, the three inlined bodies take 139-146 VGPRs and
// 3 waves; at 128 one 8-B value of the preamble spills: one store and two reloads per wave).
// The multi-type group (RAVG) keeps the members' kRavgAtmosBlocks, in every precision.
constexpr int kGroupBlocks = 4;
template <int C, class R, bool NT, int HALO, int TM = 1, bool RAVG = false>
__global__ __launch_bounds__(64 * atmos_waves<C>(), is_cr<R>() ? kWideAtmosBlocks
                                                    : RAVG ? kRavgAtmosBlocks
                                                    : is_wide<R>() ? kWideAtmosBlocks
                                                    : C == 4 ? kF32AtmosBlocks : kGroupBlocks) void
cells_atmos_group_kernel(const GroupArgs g, const Params *__restrict__ P0, const Params *__restrict__ P1,
                         const Params *__restrict__ P2, const Params *__restrict__ P3) {
  // The members' parameter blocks are separate const __restrict__ kernel arguments (not the
  // pointers inside GroupArgs): the compiler then knows the blocks are not written by the
  // launch and reads them with scalar loads, as in cells_atmos_kernel.  Read through a
  // pointer out of the argument struct, every field was a vector load (and a dependent
  // round trip before the field loads): the group kernel took 1.156 ms against 0.783 ms
  // for the three launches it replaced (a round-4 diagnostic build, not kept).
  __shared__ double s_p[atmos_waves<C>()][wave_lds_doubles<R, C, RAVG>()];
  static_assert(!RAVG || lds_fits<R, C, RAVG>(kRavgAtmosBlocks, atmos_waves<C>()),
                "register averages: the launch bound's blocks per CU hold at most 160 KiB of LDS");
  const int wv = threadIdx.x >> 6;
  double *wp = s_p[wv];
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t wave0 =
      (int64_t)xcd_block<C == 4 ? kXcdChunkF32 : kXcdChunk>(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + wv;
  for (int64_t t = wave0; t < g.total_tiles; t += waves) {
    // the range and member of tile t: wave-uniform, said so to the compiler (readfirstlane),
    // so that their parameters are scalar loads -- derived from threadIdx.x >> 6, the index
    // would be taken for a per-lane value and every member field would occupy VGPRs
    int q = 0;
    for (int j = 1; j < g.n_ranges; ++j)
      if (t >= g.r[j].t0) q = j;
    q = __builtin_amdgcn_readfirstlane(q);
    const GroupRange &rg = g.r[q];
    const int k = __builtin_amdgcn_readfirstlane(rg.member);
    const GroupMember &m = g.m[k];
    const Params *__restrict__ P = k == 0 ? P0 : k == 1 ? P1 : k == 2 ? P2 : P3;
    const int64_t tile = t - rg.t0 + rg.first;
    switch (m.var) {
      case 1: atmos_tile<C, R, 1, NT, TM, RAVG, false, HALO>(P, m.corr_m, m.af, tile, wp); break;
      case 2: atmos_tile<C, R, 2, NT, TM, RAVG, false, HALO>(P, m.corr_m, m.af, tile, wp); break;
      default: atmos_tile<C, R, 3, NT, TM, RAVG, false, HALO>(P, m.corr_m, m.af, tile, wp); break;
    }
    // launch_cells_group launches a wave per tile.  Said to the compiler for the dense-record
    // variant: as a loop, it kept loop-invariant constants in registers across the body and
    // spilled six of them at the 128-VGPR cap
    if constexpr (HALO == 2) break;
  }
}

// Segments that straddle a tile boundary: the launch leaves, in the crossing record of every tile t, the prefix sum of tile t-1's last
// segment, the number of head cells of tile t (cells that continue that segment) with their
// atmosphere cell, and the products of the first kRecHead of them; this kernel continues each
// carry over the head cells, one thread per (tile, field), in link order: the same bits as
// the in-launch sum.  Cells of a longer head are recomputed from the stored fluxes with the
// kernel's own operation (w * x, fp32 fluxes widened).
// Segments are at most half a tile (the fused path's rule), so a carry never spans a tile.
// field k of the segment across tile boundary t (tile t's crossing record)
template <class R, int kT>
__device__ __forceinline__ void fixup_one(const AtmosFused &af, int64_t t, int k) {
  // one crossing record (two lines) holds everything of the common case: every load issued
  // before the head count is known, one memory round trip.  (One thread per boundary with
  // the whole record in 16-B loads measured the same: profiles/r04/crossings/inproc3/.)
  const int64_t x0 = t * kT;
  const double *rec = af.xrec + t * kXRec;
  const int2 ha = *reinterpret_cast<const int2 *>(rec + 30);
  double acc = rec[k];
  double p[kRecHead];
#pragma unroll
  for (int e = 0; e < kRecHead; ++e) p[e] = rec[kFusedFields + e * kFusedFields + k];
  const int h = ha.x;
  const int32_t a = ha.y;
  if (h == 0) return;
#pragma unroll
  for (int e = 0; e < kRecHead; ++e)
    if (e < h) acc = acc + p[e];
  const R *xk = reinterpret_cast<const R *>(af.x[k]);
  for (int e = kRecHead; e < h; ++e) acc = acc + af.w[x0 + e] * (double)xk[tiled(x0 + e, af.tpad)];
  reinterpret_cast<R *>(af.out[k])[atm_at(a, af.out_stride, af.out_tpad)] = (R)acc;
  if (a == 0 && af.left >= 0) af.shared[(int64_t)af.left * af.stride + af.scol[k]] = acc;
  if (a == af.n_atmos - 1 && af.right >= 0) af.shared[(int64_t)af.right * af.stride + af.scol[k]] = acc;
}

template <class R, int kT>
__global__ __launch_bounds__(256) void atmos_fixup_kernel(const AtmosFused af, int64_t n_tiles) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t t = 1 + i / kFusedFields;
  const int k = (int)(i % kFusedFields);
  if (t >= n_tiles || !af.out[k]) return;
  fixup_one<R, kT>(af, t, k);
}

// The fix-ups of a group launch's members (fcx_run_group) as ONE launch: member m's
// (boundary, field) threads are [first[m], first[m + 1]).  Each dependent launch costs the
// step its predecessor's drain, the dispatch and the ramp on top of its work: in one process
// over the same arrays, T = 2 group step 1.560 against 1.566 ms with one fix-up launch per
// member, T = 1 without halo tiles 0.759 against 0.766 ms (profiles/r04/crossings/inproc1/).
template <class R, int kT>
__global__ __launch_bounds__(256) void atmos_fixup_group_kernel(const FixupGroup g) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.first[g.n]) return;
  int m = 0;
  for (int q = 1; q < g.n; ++q)
    if (i >= g.first[q]) m = q;
  const int64_t j = i - g.first[m];
  const int64_t t = 1 + j / kFusedFields;
  const int k = (int)(j % kFusedFields);
  if (!g.af[m].out[k]) return;
  fixup_one<R, kT>(g.af[m], t, k);
}

// do_regridding (basic:463-522) as CSR-by-destination: row d holds the links with
// dst_index == d in their original link order, so the sequential sum from 0.0 reproduces
// the reference's scatter-add order exactly (bit-identical) without atomics.
// R = float: the single-precision build's REAL(4) arithmetic.
template <class R>
__global__ __launch_bounds__(256) void regrid_csr_kernel(const int32_t *__restrict__ row_ptr,
                                                         const int32_t *__restrict__ col,
                                                         const R *__restrict__ w,
                                                         const R *__restrict__ src,
                                                         R *__restrict__ dst, int64_t n_dst, int64_t tpad) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_dst) return;
  R acc = R(0);
  for (int32_t k = row_ptr[d]; k < row_ptr[d + 1]; ++k) acc = acc + src[tiled(col[k], tpad)] * w[k];
  dst[tiled(d, tpad)] = acc;
}

// exchange -> atmosphere accumulation (SCRIP weight application of the type-0 fields).
// One thread per local atmosphere cell, 256 cells per block.  The block's exchange range
// [row_ptr[a0], row_ptr[a0 + 256]) is streamed through LDS in chunks of kAtmChunk cells:
// the whole block loads weights and fields with coalesced loads (16-B vectors of consecutive
// links when the links are the exchange cells in order, `vec`) and stores the
// products w*x per field, then every lane adds the products of its own segment in link
// order.  acc = acc + w*x from 0.0 in increasing link order is exactly the sequential
// weight application, so the result is bit-identical to it (no atomics, no tree order).
constexpr int kAtmChunk = 512;

// R: element type of the fields and outputs (float in the fp32 engine; the weights, the
// products and the sums are fp64 either way, and an fp32 output is rounded once).
template <class R>
__global__ __launch_bounds__(256) void atmos_kernel(const AtmosArgs a) {
  extern __shared__ double lds[];  // [nf][kAtmChunk] products
  const int64_t a0 = (int64_t)blockIdx.x * blockDim.x;
  const int64_t c = a0 + threadIdx.x;
  const int64_t a_end = min(a0 + (int64_t)blockDim.x, a.n_atmos);
  const int32_t K0 = a.row_ptr[a0], K1 = a.row_ptr[a_end];
  constexpr int V = 16 / sizeof(R);  // elements per 16-B vector (2 fp64, 4 fp32)
  using VecT = typename std::conditional<sizeof(R) == 8, d2, f4>::type;
  const int32_t n_links = a.vec ? a.row_ptr[a.n_atmos] : 0;
  const bool mine = c < a.n_atmos;
  const int32_t k_lo = mine ? a.row_ptr[c] : 0, k_hi = mine ? a.row_ptr[c + 1] : 0;
  double acc[kMaxAtmosFields];
#pragma unroll
  for (int f = 0; f < kMaxAtmosFields; ++f) acc[f] = 0.0;
  for (int32_t C0 = K0; C0 < K1; C0 += kAtmChunk) {
    const int32_t len = min(kAtmChunk, K1 - C0);
    __syncthreads();
    if (a.vec) {  // link k = exchange cell k: 16-B loads of V consecutive weights and fields
      const int32_t hi_k = C0 + len;
      for (int32_t v = (C0 & ~(V - 1)) + (int32_t)threadIdx.x * V; v < hi_k; v += (int32_t)blockDim.x * V) {
        const bool full = v + V <= n_links;  // v..v+V-1 share a layout tile (V divides it)
        double wv[V];
        if (full) {
#pragma unroll
          for (int h = 0; h < V / 2; ++h) {
            const d2 t = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(a.w + v) + h);
            wv[2 * h] = t[0];
            wv[2 * h + 1] = t[1];
          }
        } else {
#pragma unroll
          for (int i = 0; i < V; ++i) wv[i] = v + i < n_links ? a.w[v + i] : 0.0;
        }
        const int64_t xo = tiled(v, a.tpad);
        for (int f = 0; f < a.nf; ++f) {
          const R *xf = reinterpret_cast<const R *>(a.x[f]) + xo;
          R xv[V];
          if (full) {
            const VecT t = __builtin_nontemporal_load(reinterpret_cast<const VecT *>(xf));
#pragma unroll
            for (int i = 0; i < V; ++i) xv[i] = t[i];
          } else {
#pragma unroll
            for (int i = 0; i < V; ++i) xv[i] = v + i < n_links ? xf[i] : R(0);
          }
#pragma unroll
          for (int i = 0; i < V; ++i)
            if (v + i >= C0 && v + i < hi_k) lds[f * kAtmChunk + (v + i - C0)] = wv[i] * (double)xv[i];
        }
      }
    } else if (a.rec) {  // remap gather of packed records: nf values of a link in rec_p / V 16-B loads
      for (int32_t i = threadIdx.x; i < len; i += blockDim.x) {
        const int32_t k = C0 + i;
        const int32_t xi = __builtin_nontemporal_load(a.col + k);
        const double wk = __builtin_nontemporal_load(a.w + k);
        const VecT *r = reinterpret_cast<const VecT *>(reinterpret_cast<const R *>(a.rec) + (int64_t)xi * a.rec_p);
#pragma unroll
        for (int q = 0; q < kMaxAtmosFields / V; ++q) {
          if (q * V >= a.nf) break;
          const VecT t = r[q];
#pragma unroll
          for (int h = 0; h < V; ++h)
            if (q * V + h < a.nf) lds[(q * V + h) * kAtmChunk + i] = wk * (double)t[h];
        }
      }
    } else {
      for (int32_t i = threadIdx.x; i < len; i += blockDim.x) {
        const int32_t k = C0 + i;
        const int32_t xi = a.col ? a.col[k] : k;
        const double wk = __builtin_nontemporal_load(a.w + k);
#pragma unroll
        for (int f = 0; f < kMaxAtmosFields; ++f)
          if (f < a.nf) lds[f * kAtmChunk + i] = wk * (double)reinterpret_cast<const R *>(a.x[f])[tiled(xi, a.tpad)];
      }
    }
    __syncthreads();
    const int32_t lo = max(k_lo, C0), hi = min(k_hi, C0 + len);
    for (int32_t k = lo; k < hi; ++k) {
#pragma unroll
      for (int f = 0; f < kMaxAtmosFields; ++f)
        if (f < a.nf) acc[f] = acc[f] + lds[f * kAtmChunk + (k - C0)];
    }
  }
  if (!mine) return;
#pragma unroll
  for (int f = 0; f < kMaxAtmosFields; ++f) {
    if (f >= a.nf) break;
    reinterpret_cast<R *>(a.out[f])[atm_at(c, a.out_stride, a.out_tpad)] = (R)acc[f];
    if (c == 0 && a.left >= 0) a.shared[(int64_t)a.left * a.stride + a.scol[f]] = acc[f];
    if (c == a.n_atmos - 1 && a.right >= 0) a.shared[(int64_t)a.right * a.stride + a.scol[f]] = acc[f];
  }
}

// Remap records (row f3).  A remap link gathers the nf sent fields of one scattered exchange
// cell; from nf separate arrays that is nf scattered 8-B reads, each of which costs the
// memory a whole 32-B sector (PMC: 4x the algorithmic read bytes on a shuffled 2-link map).
// Packed cell-major, the nf values of a cell are one record of P = nf rounded up to 16 B,
// read by P / V 16-B loads that share its sectors.  One block packs 256 * V cells: the
// fields are staged in LDS with coalesced 16-B loads (the block's cells lie in one layout
// tile), then the block's contiguous record region is written with 16-B stores.
template <class R>
__global__ __launch_bounds__(256) void pack_records_kernel(const AtmosArgs a, int64_t n, int32_t flags, R *rec) {
  constexpr int V = 16 / sizeof(R);
  constexpr int CB = 256 * V;  // cells per block (divides kLayoutTile)
  using VecT = typename std::conditional<sizeof(R) == 8, d2, f4>::type;
  extern __shared__ unsigned char lds_raw[];
  R *lds = reinterpret_cast<R *>(lds_raw);  // [nf][CB]
  const int64_t c0 = (int64_t)blockIdx.x * CB;
  const int64_t cn = min((int64_t)CB, n - c0);
  const int t = threadIdx.x;
  for (int f = 0; f < a.nf; ++f) {
    const R *x = reinterpret_cast<const R *>(a.x[f]) + tiled(c0, a.tpad);
    const int64_t j = (int64_t)t * V;
    if ((flags & 1) && j + V <= cn) {  // 16-B aligned fields
      const VecT *p = reinterpret_cast<const VecT *>(x + j);
      const VecT v = (flags & 2) ? __builtin_nontemporal_load(p) : *p;  // not for host-mapped fields
#pragma unroll
      for (int h = 0; h < V; ++h) lds[f * CB + j + h] = v[h];
    } else {
#pragma unroll
      for (int h = 0; h < V; ++h)
        if (j + h < cn) lds[f * CB + j + h] = x[j + h];
    }
  }
  __syncthreads();
  const int P = a.rec_p;
  const int64_t nvec = cn * P / V;  // P is a multiple of V: a vector never spans two records
  VecT *out = reinterpret_cast<VecT *>(rec + c0 * P);
  for (int64_t q = t; q < nvec; q += 256) {
    const int64_t e = q * V;
    const int64_t cell = e / P;
    const int f0 = (int)(e - cell * P);
    VecT v;
#pragma unroll
    for (int h = 0; h < V; ++h) v[h] = f0 + h < a.nf ? lds[(f0 + h) * CB + cell] : R(0);
    __builtin_nontemporal_store(v, out + q);  // +1 % over plain stores (profiles/r02/remap/)
  }
}

// FCX_OPT_ATMOS_INVARIANT: the ordered finish of one engine (a.terms_k = K > 0).  After the
// all-reduce the term columns of a boundary slot hold the terms w[x] * field[x] of ALL the ranks'
// cells of the shared atmosphere cell, each at its link position (fcx_atmos_terms.hip).  Thread
// t = (boundary side, field) adds the K positions in order from +0.0 -- the sequential sum of a
// one-rank engine -- and stores it rounded once to R.  Positions past the cell's last link hold
// +0.0, and a -0.0 term arrives as +0.0 through the sum all-reduce (-0.0 + 0.0 = +0.0): adding
// either changes nothing, because the sum starts from +0.0 and so is never -0.0 (x + 0.0 = x for
// every x but -0.0).  The partial-sum columns scol[f] the accumulation kernels wrote are ignored.
template <class R>
__device__ __forceinline__ void finish_ordered(const AtmosArgs &a, int t) {
  if (t >= 2 * a.nf) return;
  const int side = t >= a.nf, f = side ? t - a.nf : t;
  const int32_t slot = side ? a.right : a.left;
  if (slot < 0) return;
  const int32_t K = a.terms_k;
  const double *term = a.shared + (int64_t)slot * a.stride + a.term0 + (int64_t)a.scol[f] * K;
  double acc = 0.0;
  for (int32_t p = 0; p < K; ++p) acc = acc + term[p];
  reinterpret_cast<R *>(a.out[f])[side ? atm_at(a.n_atmos - 1, a.out_stride, a.out_tpad) : 0] = (R)acc;
}

// after the all-reduce: completed boundary sums back into the outputs, then every slot of
// this engine's region is zeroed for the next step (one block)
template <class R>
__global__ void atmos_finish_kernel(const AtmosArgs a, int32_t n_boundaries) {
  const int t = threadIdx.x;
  if (a.terms_k > 0) {
    finish_ordered<R>(a, t);
  } else if (t < a.nf) {
    R *out = reinterpret_cast<R *>(a.out[t]);
    if (a.left >= 0) out[0] = (R)a.shared[(int64_t)a.left * a.stride + a.scol[t]];
    if (a.right >= 0) out[atm_at(a.n_atmos - 1, a.out_stride, a.out_tpad)] = (R)a.shared[(int64_t)a.right * a.stride + a.scol[t]];
  }
  __syncthreads();
  for (int64_t i = t; i < (int64_t)n_boundaries * a.stride; i += blockDim.x) a.shared[i] = 0.0;
}

// the finishes of several engines after one exchange, one block per engine (one launch: each
// launch is ~5 us on the step's critical path after the all-reduce)
template <class R>
__global__ void atmos_finish_group_kernel(const FinishGroup g) {
  const AtmosArgs &a = g.a[blockIdx.x];
  const int32_t n_boundaries = g.nb[blockIdx.x];
  const int t = threadIdx.x;
  if (a.terms_k > 0) {
    finish_ordered<R>(a, t);
  } else if (t < a.nf) {
    R *out = reinterpret_cast<R *>(a.out[t]);
    if (a.left >= 0) out[0] = (R)a.shared[(int64_t)a.left * a.stride + a.scol[t]];
    if (a.right >= 0) out[atm_at(a.n_atmos - 1, a.out_stride, a.out_tpad)] = (R)a.shared[(int64_t)a.right * a.stride + a.scol[t]];
  }
  __syncthreads();
  for (int64_t i = t; i < (int64_t)n_boundaries * a.stride; i += blockDim.x) a.shared[i] = 0.0;
}

// One value in every cell j < n of an engine buffer, cell j at x[tiled(j, tpad)]: the mirror of
// a constant field (fcx_bind_constant), written once at commit.  A lane stores the 16 B of its
// C consecutive cells (C divides the layout tile, so they share one tile shift; engine buffers
// are 256-B aligned); the cells of a partial last vector go out one by one, none past n.
template <class R>
__global__ __launch_bounds__(256) void fill_kernel(R *x, int64_t n, R value, int64_t tpad) {
  constexpr int C = 16 / sizeof(R);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u * C < n; u += stride) {
    const int64_t j0 = u * C;
    st<C, false, R>(x + (j0 >> kLayoutShift) * tpad, j0, n, splat<C, R>(value));
  }
}

// Model grid -> exchange grid gather of the received fields (fcx_bind_received), injection form:
// every exchange cell has at most one link, so the map is one source cell per exchange cell
// (idx[j], -1 = no link; the array is padded with -1 to a whole vector) and, only where some
// weight is not 1.0, one weight per cell.  A lane owns the C consecutive cells of one 16-B
// destination vector (C divides the layout tile, so they share one tile shift; the destinations
// are engine buffers, 256-B aligned): its index load is one 8- or 16-B load, the index and the
// weight are read once for all the fields of the launch, and the field loop is wave-uniform.
// The source loads are plain cached loads -- a source value is re-read by the 4-9 cells of its
// run -- and the destination stores are plain too: the flux pass reads the arrays right after.
// out = 0.0 + w * x in double, no contraction (so -0.0 becomes +0.0); fp32: w * (double)x32
// summed in double, rounded to float once.  Cells past n are not written.
template <class R, bool W>
__global__ __launch_bounds__(256) void receive_inject_kernel(const ReceiveArgs a) {
  constexpr int C = 16 / sizeof(R);
  using IV = typename std::conditional<C == 2, i2v, i4v>::type;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u * C < a.n; u += stride) {
    const int64_t j0 = u * C;
    const IV sv = *gptr(reinterpret_cast<const IV *>(a.idx + j0));  // (padded: in bounds)
    int32_t s[C];
    double w[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
      s[i] = sv[i];
      w[i] = 1.0;
      if (W && j0 + i < a.n) w[i] = gptr(a.w)[j0 + i];
    }
    const int64_t shift = (j0 >> kLayoutShift) * a.tpad;
    for (int f = 0; f < a.nf; ++f) {
      const R *__restrict__ src = reinterpret_cast<const R *>(a.src[f]);
      const int64_t stp = ((a.src_plain >> f) & 1u) ? 0 : a.tpad;
      Vec<C, R> o;
#pragma unroll
      for (int i = 0; i < C; ++i) {
        double acc = 0.0;
        if (s[i] >= 0) {
          const double x = (double)gptr(src)[tiled(s[i], stp)];
          acc = acc + (W ? w[i] * x : x);
        }
        o.v[i] = (R)acc;
      }
      st<C, false, R>(reinterpret_cast<R *>(a.dst[f]) + shift, j0, a.n, o);
    }
  }
}

// ... general form: CSR by exchange cell in stable link order, one lane per exchange cell, the
// row loop of atmos_kernel with a tiled destination (several links per cell: a bilinear or
// conservative map onto an exchange grid that is not an intersection grid).
template <class R>
__global__ __launch_bounds__(256) void receive_csr_kernel(const ReceiveArgs a) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < a.n; d += stride) {
    const int32_t k0 = gptr(a.row_ptr)[d], k1 = gptr(a.row_ptr)[d + 1];
    for (int f = 0; f < a.nf; ++f) {
      const R *__restrict__ src = reinterpret_cast<const R *>(a.src[f]);
      const int64_t stp = ((a.src_plain >> f) & 1u) ? 0 : a.tpad;
      double acc = 0.0;
      for (int32_t k = k0; k < k1; ++k) acc = acc + gptr(a.w)[k] * (double)gptr(src)[tiled(gptr(a.col)[k], stp)];
      gptr(reinterpret_cast<R *>(a.dst[f]))[tiled(d, a.tpad)] = (R)acc;
    }
  }
}

// The wide instantiations (F32Wide) are compiled in a translation unit of their own
// (fcx_kernels_wide.hip includes this file with FCX_KERNELS_WIDE_TU set), beside this one: the
// templates above are shared, each unit instantiates its own precisions, and these three
// launchers are the seam.  Shapes as computed by launch_cells / launch_cells_group.
#ifndef FCX_KERNELS_WIDE_TU
#define FCX_KERNELS_WIDE_TU 0
#endif
int launch_wide_fused(int variant, bool halo, bool ravg, bool nt, int blocks, hipStream_t s, const Params *dp,
                      const double *corr_m, const AtmosFused &af, int64_t lo, int64_t hi);
void launch_wide_cells(int c, const Params *hp, const LaunchConfig &lc, int blocks, hipStream_t s, const Params *dp,
                       const double *corr_m, int64_t lo, int64_t hi);
void launch_wide_group(bool nt, bool halo, bool ravg, int blocks, hipStream_t s, const GroupArgs &g);
// ... and the F64Cr instantiations (FCX_OPT_CR_MATH) in a third unit, fcx_kernels_cr.hip
// (FCX_KERNELS_CR_TU): the sibling of every fp64 launch, behind four launchers.
#ifndef FCX_KERNELS_CR_TU
#define FCX_KERNELS_CR_TU 0
#endif
#define FCX_KERNELS_MAIN_TU (!FCX_KERNELS_WIDE_TU && !FCX_KERNELS_CR_TU)
int launch_cr_fused(int variant, const Params *hp, const LaunchConfig &lc, int blocks, hipStream_t s, const Params *dp,
                    const double *corr_m, const AtmosFused &af, int64_t lo, int64_t hi);
void launch_cr_cells(int c, const Params *hp, const LaunchConfig &lc, int blocks, hipStream_t s, const Params *dp,
                     const double *corr_m, int64_t lo, int64_t hi);
void launch_cr_rec(int variant, bool nt, int blocks, hipStream_t s, const Params *dp, const double *corr_m, int64_t lo,
                   int64_t hi);
void launch_cr_group(bool nt, bool halo, bool ravg, int blocks, hipStream_t s, const GroupArgs &g);

static int grid_for(int64_t units, int max_blocks = 256 * 8) {
  // memory-bound grid-stride: enough waves to fill 256 CUs, capped (0 = one unit per thread)
  int64_t blocks = (units + 255) / 256;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

template <int C, bool MERGED, int VAR, bool NT, class R, int TM, bool RAVG>
static void launch_one(int blocks, hipStream_t s, const Params *dp, const double *corr_m, int64_t lo,
                       int64_t hi) {
  hipLaunchKernelGGL((cells_kernel<C, MERGED, VAR, NT, R, TM, RAVG>), dim3(blocks), dim3(256), 0, s, dp,
                     corr_m, lo, hi);
}

template <int C, bool MERGED, int VAR, class R, int TM, bool RAVG>
static void launch_nt(bool nt, int blocks, hipStream_t s, const Params *dp, const double *corr_m,
                      int64_t lo, int64_t hi) {
  if (nt)
    launch_one<C, MERGED, VAR, true, R, TM, RAVG>(blocks, s, dp, corr_m, lo, hi);
  else
    launch_one<C, MERGED, VAR, false, R, TM, RAVG>(blocks, s, dp, corr_m, lo, hi);
}

template <int C, class R, int TM, bool RAVG>
static void launch_c(const LaunchConfig &lc, int blocks, hipStream_t s, const Params *dp,
                     const double *corr_m, int64_t lo, int64_t hi) {
  if (!lc.merged) {
    launch_nt<C, false, 0, R, TM, RAVG>(lc.nontemporal, blocks, s, dp, corr_m, lo, hi);
    return;
  }
  switch (lc.variant) {
    case 1: launch_nt<C, true, 1, R, TM, RAVG>(lc.nontemporal, blocks, s, dp, corr_m, lo, hi); break;
    case 2: launch_nt<C, true, 2, R, TM, RAVG>(lc.nontemporal, blocks, s, dp, corr_m, lo, hi); break;
    case 3: launch_nt<C, true, 3, R, TM, RAVG>(lc.nontemporal, blocks, s, dp, corr_m, lo, hi); break;
    default: launch_nt<C, true, 0, R, TM, RAVG>(lc.nontemporal, blocks, s, dp, corr_m, lo, hi); break;
  }
}

// (PR: double or F64Cr)
template <int VAR, class PR = double>
static void launch_rec(bool nt, int blocks, hipStream_t s, const Params *dp, const double *corr_m, int64_t lo,
                       int64_t hi) {
  if (nt)
    hipLaunchKernelGGL((cells_kernel<2, true, VAR, true, PR, 1, false, true>), dim3(blocks), dim3(256), 0, s, dp,
                       corr_m, lo, hi);
  else
    hipLaunchKernelGGL((cells_kernel<2, true, VAR, false, PR, 1, false, true>), dim3(blocks), dim3(256), 0, s, dp,
                       corr_m, lo, hi);
}

// type mode: one surface type (compile-time), several, several with register averages
template <int C, class R>
static void launch_r(const Params *hp, const LaunchConfig &lc, int blocks, hipStream_t s, const Params *dp,
                     const double *corr_m, int64_t lo, int64_t hi) {
  if (hp->num_types == 1)
    launch_c<C, R, 1, false>(lc, blocks, s, dp, corr_m, lo, hi);
  else if (lc.ravg)
    launch_c<C, R, 0, true>(lc, blocks, s, dp, corr_m, lo, hi);
  else
    launch_c<C, R, 0, false>(lc, blocks, s, dp, corr_m, lo, hi);
}

template <int C, class R, int VAR, int TM, bool RAVG, bool REC = false, int HALO = 0>
static void launch_atm(bool nt, int blocks, hipStream_t s, const Params *dp, const double *corr_m,
                       const AtmosFused &af, int64_t lo, int64_t hi) {
  if (nt)
    hipLaunchKernelGGL((cells_atmos_kernel<C, R, VAR, true, TM, RAVG, REC, HALO>), dim3(blocks),
                       dim3(64 * atmos_waves<C>()), 0, s, dp, corr_m, af, lo, hi);
  else
    hipLaunchKernelGGL((cells_atmos_kernel<C, R, VAR, false, TM, RAVG, REC, HALO>), dim3(blocks),
                       dim3(64 * atmos_waves<C>()), 0, s, dp, corr_m, af, lo, hi);
}

// the fused launches of double fields (PR: double, or F64Cr in its own unit)
template <int VAR, class PR>
static int launch_atm_f64(const Params *hp, const LaunchConfig &lc, int blocks, hipStream_t s, const Params *dp,
                          const double *corr_m, const AtmosFused &af, int64_t lo, int64_t hi) {
  const bool halo = lc.halo > 0;
  if (hp->num_types == 1 && lc.rec) {
    if (halo)
      launch_atm<2, PR, VAR, 1, false, true, true>(lc.nontemporal, blocks, s, dp, corr_m, af, lo, hi);
    else
      launch_atm<2, PR, VAR, 1, false, true>(lc.nontemporal, blocks, s, dp, corr_m, af, lo, hi);
  } else if (hp->num_types == 1) {
    if (halo && af.rec_dense)
      launch_atm<2, PR, VAR, 1, false, false, 2>(lc.nontemporal, blocks, s, dp, corr_m, af, lo, hi);
    else if (halo)
      launch_atm<2, PR, VAR, 1, false, false, true>(lc.nontemporal, blocks, s, dp, corr_m, af, lo, hi);
    else
      launch_atm<2, PR, VAR, 1, false>(lc.nontemporal, blocks, s, dp, corr_m, af, lo, hi);
  } else if (lc.ravg) {  // (crossing records: halo tiles are the T = 1 launches')
    launch_atm<2, PR, VAR, 0, true>(lc.nontemporal, blocks, s, dp, corr_m, af, lo, hi);
  } else
    return (int)hipErrorInvalidValue;
  return 0;
}

#if FCX_KERNELS_MAIN_TU
// fused accumulation: one surface type (its fluxes), or several with the type-0 averages in
// registers (what OASIS sends), in every precision; several types without register averages
// are not fused
template <int VAR>
static int launch_atm_r(const Params *hp, const LaunchConfig &lc, int blocks, hipStream_t s, const Params *dp,
                        const double *corr_m, const AtmosFused &af, int64_t lo, int64_t hi) {
  const bool halo = lc.halo > 0;
  if (halo && (hp->num_types != 1 || lo != 0)) return (int)hipErrorInvalidValue;
  if (lc.wide && !lc.f32) return (int)hipErrorInvalidValue;
  if (lc.cr && lc.f32) return (int)hipErrorInvalidValue;
  if (lc.cr) return launch_cr_fused(VAR, hp, lc, blocks, s, dp, corr_m, af, lo, hi);
  if (hp->num_types == 1 && lc.wide) {  // fp32 engine computing in double: the wide kernels
    return launch_wide_fused(VAR, halo, false, lc.nontemporal, blocks, s, dp, corr_m, af, lo, hi);
  } else if (hp->num_types == 1 && lc.f32) {  // fp32 engine: 4 cells per lane
    if (halo)
      launch_atm<kF32Cpl, float, VAR, 1, false, false, true>(lc.nontemporal, blocks, s, dp, corr_m, af, lo, hi);
    else
      launch_atm<kF32Cpl, float, VAR, 1, false>(lc.nontemporal, blocks, s, dp, corr_m, af, lo, hi);
  } else if (lc.f32) {  // several types: the register averages, crossing records (no halo tiles)
    if (!lc.ravg || halo) return (int)hipErrorInvalidValue;
    if (lc.wide) return launch_wide_fused(VAR, false, true, lc.nontemporal, blocks, s, dp, corr_m, af, lo, hi);
    launch_atm<kF32Cpl, float, VAR, 0, true>(lc.nontemporal, blocks, s, dp, corr_m, af, lo, hi);
  } else {
    return launch_atm_f64<VAR, double>(hp, lc, blocks, s, dp, corr_m, af, lo, hi);
  }
  return 0;
}

#if FCX_WAVE_TRACE
// measurement builds: launch k of the fused kernel writes its wave timestamps into slot
// k % slots of a device buffer of slots x stride words (bench/wave_trace.py)
static struct {
  uint64_t *base = nullptr;
  int64_t stride = 0;
  int64_t slots = 1;
  int64_t launches = 0;
} g_trace;
}  // namespace fcx
extern "C" int fcx_debug_wave_trace(uint64_t *base, int64_t stride_words, int64_t slots, int64_t *wall_khz) {
  fcx::g_trace.base = base;
  fcx::g_trace.stride = stride_words;
  fcx::g_trace.slots = slots > 0 ? slots : 1;
  fcx::g_trace.launches = 0;
  int rate = 0, dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, dev) != hipSuccess)
    return 1;
  if (wall_khz) *wall_khz = rate;
  return 0;
}
namespace fcx {
#endif

int launch_cells(const Params *hp, const Params *dp, const double *corr_m, const LaunchConfig &lc,
                 void *stream, const AtmosFused *atm) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t lo = lc.lo, hi = lc.hi < 0 ? hp->n_max : std::min<int64_t>(lc.hi, hp->n_max);
  if (lo % kChunkAlign || lo < 0) return (int)hipErrorInvalidValue;
  if (hi <= lo) return 0;
  AtmosFused afl;  // this launch's copy: its tile count (and, in trace builds, its trace slot)
  if (atm) {
    afl = *atm;
    const int64_t own = fused_cpl(lc.f32, lc.wide) * (64 - lc.halo);
    afl.n_tiles = (hi + own - 1) / own;
#if FCX_WAVE_TRACE
    afl.trace = g_trace.base ? g_trace.base + (g_trace.launches++ % g_trace.slots) * g_trace.stride : nullptr;
#endif
    atm = &afl;
  }
  if (atm) {  // fused accumulation: T=1 specialised merged kernel, 2 cells per lane
    // four waves per block (fp32: two), one 128-cell (fp32: 256-cell) tile per wave and trip.  Default: one trip (full
    // grid) -- +2 % per T=1 step over the 8192-block cap, equal at T=2 (profiles/r01/grid_ab)
    const int64_t kt = fused_cpl(lc.f32, lc.wide) * (64 - lc.halo);  // cells a wave tile owns
    const int64_t kw = lc.wide ? atmos_waves<kWideCpl>() : lc.f32 ? atmos_waves<kF32Cpl>() : atmos_waves<2>();
    const int64_t tiles = (hi - lo + kt - 1) / kt;
    const int64_t full = (tiles + kw - 1) / kw;
    const int blocks = (int)std::max<int64_t>(1, lc.max_blocks > 0 ? std::min<int64_t>(full, lc.max_blocks) : full);
    int r = 0;
    switch (lc.variant) {
      case 1: r = launch_atm_r<1>(hp, lc, blocks, s, dp, corr_m, *atm, lo, hi); break;
      case 2: r = launch_atm_r<2>(hp, lc, blocks, s, dp, corr_m, *atm, lo, hi); break;
      case 3: r = launch_atm_r<3>(hp, lc, blocks, s, dp, corr_m, *atm, lo, hi); break;
      default: return (int)hipErrorInvalidValue;
    }
    if (r) return r;
    return (int)hipGetLastError();
  }
  // vector width: 16 B per lane and array (2 fp64 or 4 fp32 cells), or 1 cell when the
  // caller's arrays are not 16-B aligned
  const int c = lc.cells_per_thread == 1 ? 1 : lc.f32 ? 4 : 2;
  const int64_t units = (hi - lo + c - 1) / c;
  const int blocks = grid_for(units, lc.max_blocks < 0 ? 8192 : lc.max_blocks);
  if (lc.rec) {  // remap records: the T=1 specialised fp64 kernels only (the planner's rule)
    if (lc.f32 || c != 2 || hp->num_types != 1 || !lc.merged || lc.variant < 1 || lc.variant > 3)
      return (int)hipErrorInvalidValue;
    if (lc.cr) {
      launch_cr_rec(lc.variant, lc.nontemporal, blocks, s, dp, corr_m, lo, hi);
      return (int)hipGetLastError();
    }
    switch (lc.variant) {
      case 1: launch_rec<1>(lc.nontemporal, blocks, s, dp, corr_m, lo, hi); break;
      case 2: launch_rec<2>(lc.nontemporal, blocks, s, dp, corr_m, lo, hi); break;
      default: launch_rec<3>(lc.nontemporal, blocks, s, dp, corr_m, lo, hi); break;
    }
    return (int)hipGetLastError();
  }
  if ((lc.wide && !lc.f32) || (lc.cr && lc.f32)) return (int)hipErrorInvalidValue;
  if (lc.cr) {
    launch_cr_cells(c, hp, lc, blocks, s, dp, corr_m, lo, hi);
  } else if (lc.wide) {
    launch_wide_cells(c, hp, lc, blocks, s, dp, corr_m, lo, hi);
  } else if (lc.f32) {
    if (c == 4)
      launch_r<4, float>(hp, lc, blocks, s, dp, corr_m, lo, hi);
    else
      launch_r<1, float>(hp, lc, blocks, s, dp, corr_m, lo, hi);
  } else if (c == 2) {
    launch_r<2, double>(hp, lc, blocks, s, dp, corr_m, lo, hi);
  } else {
    launch_r<1, double>(hp, lc, blocks, s, dp, corr_m, lo, hi);
  }
  return (int)hipGetLastError();
}

#endif
template <int C, class R, bool NT>
static void launch_group_h(bool halo, bool ravg, int blocks, hipStream_t s, const GroupArgs &g) {
  const Params *p[kMaxGroup];
  for (int k = 0; k < kMaxGroup; ++k) p[k] = g.m[k < g.n ? k : 0].P;
  if (ravg) {  // several surface types, the type-0 averages in registers (no halo tiles)
    hipLaunchKernelGGL((cells_atmos_group_kernel<C, R, NT, false, 0, true>), dim3(blocks),
                       dim3(64 * atmos_waves<C>()), 0, s, g, p[0], p[1], p[2], p[3]);
    return;
  }
  if constexpr (C == 2 && sizeof(typename Prec<R>::store) == 8) {
    bool dense = halo;  // every member keeps per-cell records of the six fluxes
    for (int k = 0; k < g.n; ++k) dense = dense && g.m[k].af.rec_dense;
    if (dense) {
      hipLaunchKernelGGL((cells_atmos_group_kernel<C, R, NT, 2>), dim3(blocks), dim3(64 * atmos_waves<C>()), 0, s, g,
                         p[0], p[1], p[2], p[3]);
      return;
    }
  }
  if (halo)
    hipLaunchKernelGGL((cells_atmos_group_kernel<C, R, NT, true>), dim3(blocks), dim3(64 * atmos_waves<C>()), 0, s, g,
                       p[0], p[1], p[2], p[3]);
  else
    hipLaunchKernelGGL((cells_atmos_group_kernel<C, R, NT, false>), dim3(blocks), dim3(64 * atmos_waves<C>()), 0, s,
                       g, p[0], p[1], p[2], p[3]);
}

#if FCX_KERNELS_MAIN_TU
int launch_cells_group(GroupMember *members, int n, const LaunchConfig &lc, void *stream) {
  if (n < 1 || n > kMaxGroup) return (int)hipErrorInvalidValue;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GroupArgs g{};
  g.n = n;
  int64_t total = 0;
  for (int k = 0; k < n; ++k) {  // (af.n_tiles: set by the caller from the member's cells)
    GroupMember &m = members[k];
    if (m.var < 1 || m.var > 3 || (m.af.halo > 0) != (lc.halo > 0) || m.af.n_tiles < 0)
      return (int)hipErrorInvalidValue;
    m.tile0 = total;
    g.m[k] = m;
    g.r[k] = GroupRange{total, 0, k, 0};
    total += m.af.n_tiles;
  }
  g.n_ranges = n;
  g.total_tiles = total;
  if (total == 0) return 0;
  const int64_t kw = lc.wide ? atmos_waves<kWideCpl>() : lc.f32 ? atmos_waves<kF32Cpl>() : atmos_waves<2>();
  const int blocks = (int)std::max<int64_t>(1, (total + kw - 1) / kw);
  if (lc.ravg && lc.halo > 0) return (int)hipErrorInvalidValue;
  if ((lc.wide && !lc.f32) || (lc.cr && lc.f32)) return (int)hipErrorInvalidValue;
  if (lc.cr) {
    launch_cr_group(lc.nontemporal, lc.halo > 0, lc.ravg, blocks, s, g);
  } else if (lc.wide) {
    launch_wide_group(lc.nontemporal, lc.halo > 0, lc.ravg, blocks, s, g);
  } else if (lc.f32) {
    if (lc.nontemporal) launch_group_h<kF32Cpl, float, true>(lc.halo > 0, lc.ravg, blocks, s, g);
    else launch_group_h<kF32Cpl, float, false>(lc.halo > 0, lc.ravg, blocks, s, g);
  } else {
    if (lc.nontemporal) launch_group_h<2, double, true>(lc.halo > 0, lc.ravg, blocks, s, g);
    else launch_group_h<2, double, false>(lc.halo > 0, lc.ravg, blocks, s, g);
  }
  return (int)hipGetLastError();
}

int launch_regrid_csr(const int32_t *row_ptr, const int32_t *col, const double *w,
                      const double *src, double *dst, int64_t n_dst, void *stream, bool f32, int64_t tpad) {
  if (n_dst <= 0) return 0;
  const int blocks = (int)((n_dst + 255) / 256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (f32)
    hipLaunchKernelGGL(regrid_csr_kernel<float>, dim3(blocks), dim3(256), 0, s, row_ptr, col,
                       reinterpret_cast<const float *>(w), reinterpret_cast<const float *>(src),
                       reinterpret_cast<float *>(dst), n_dst, tpad);
  else
    hipLaunchKernelGGL(regrid_csr_kernel<double>, dim3(blocks), dim3(256), 0, s, row_ptr, col, w, src, dst, n_dst, tpad);
  return (int)hipGetLastError();
}

int launch_atmos(const AtmosArgs &a, void *stream) {
  if (a.n_atmos <= 0 || a.nf <= 0) return 0;
  const int blocks = (int)((a.n_atmos + 255) / 256);
  const size_t lds = (size_t)a.nf * kAtmChunk * sizeof(double);
  if (a.f32)
    hipLaunchKernelGGL(atmos_kernel<float>, dim3(blocks), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(atmos_kernel<double>, dim3(blocks), dim3(256), lds, reinterpret_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

int launch_pack_records(const AtmosArgs &a, int64_t n, bool aligned16, bool nontemporal, void *rec, void *stream) {
  if (n <= 0 || a.nf <= 0) return 0;
  const int V = a.f32 ? 4 : 2;
  if (a.rec_p < a.nf || a.rec_p % V || a.nf > kMaxAtmosFields) return (int)hipErrorInvalidValue;
  const int64_t cb = 256 * V;
  const int blocks = (int)((n + cb - 1) / cb);
  const size_t lds = (size_t)a.nf * cb * (a.f32 ? 4 : 8);
  const int32_t flags = (aligned16 ? 1 : 0) | (nontemporal ? 2 : 0);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a.f32)
    hipLaunchKernelGGL(pack_records_kernel<float>, dim3(blocks), dim3(256), lds, s, a, n, flags,
                       reinterpret_cast<float *>(rec));
  else
    hipLaunchKernelGGL(pack_records_kernel<double>, dim3(blocks), dim3(256), lds, s, a, n, flags,
                       reinterpret_cast<double *>(rec));
  return (int)hipGetLastError();
}

int launch_atmos_finish(const AtmosArgs &a, int32_t n_boundaries, void *stream) {
  if (!a.shared) return 0;
  if (a.f32)
    hipLaunchKernelGGL(atmos_finish_kernel<float>, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       a, n_boundaries);
  else
    hipLaunchKernelGGL(atmos_finish_kernel<double>, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       a, n_boundaries);
  return (int)hipGetLastError();
}

int launch_atmos_finish_group(const AtmosArgs *as, const int32_t *nbs, int n, void *stream) {
  if (n < 1 || n > kMaxGroup) return (int)hipErrorInvalidValue;
  FinishGroup g{};
  g.n = n;
  for (int k = 0; k < n; ++k) {
    if (!as[k].shared || as[k].f32 != as[0].f32) return (int)hipErrorInvalidValue;
    g.a[k] = as[k];
    g.nb[k] = nbs[k];
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (as[0].f32)
    hipLaunchKernelGGL(atmos_finish_group_kernel<float>, dim3(n), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL(atmos_finish_group_kernel<double>, dim3(n), dim3(256), 0, s, g);
  return (int)hipGetLastError();
}

int launch_atmos_fixup(const AtmosFused &af, int64_t n, bool f32, void *stream, bool wide) {
  const int64_t kt = 64 * fused_cpl(f32, wide);
  const int64_t tiles = (n + kt - 1) / kt;
  if (tiles < 2) return 0;
  const int blocks = (int)(((tiles - 1) * kFusedFields + 255) / 256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (f32 && wide)
    hipLaunchKernelGGL((atmos_fixup_kernel<float, tile_cells<kWideCpl>()>), dim3(blocks), dim3(256), 0, s, af, tiles);
  else if (f32)
    hipLaunchKernelGGL((atmos_fixup_kernel<float, tile_cells<kF32Cpl>()>), dim3(blocks), dim3(256), 0, s, af, tiles);
  else
    hipLaunchKernelGGL((atmos_fixup_kernel<double, tile_cells<2>()>), dim3(blocks), dim3(256), 0, s, af, tiles);
  return (int)hipGetLastError();
}

// Atmosphere cells without exchange cells: the sequential SCRIP sum over no links is 0, and
// the fused launch, which stores one value per segment, has none for them.
// Atmosphere records -> the tile-blocked pool of plain arrays that the downloads read
// (FCX_OPT_ATM_RECORDS): a block takes 256 atmosphere cells (one layout tile holds them all),
// loads their contiguous records with 16-B loads into LDS and writes each field's 256 values.
__global__ __launch_bounds__(256) void atm_unpack_kernel(const double *__restrict__ rec, double *__restrict__ soa,
                                                         int64_t n_atmos, int nf, int64_t tpad) {
  constexpr int CB = 256;
  extern __shared__ unsigned char lds_raw[];
  double *lds = reinterpret_cast<double *>(lds_raw);  // [CB][nf]
  const int64_t c0 = (int64_t)blockIdx.x * CB;
  const int cn = (int)min((int64_t)CB, n_atmos - c0);
  const int ne = cn * nf;
  const double *src = rec + c0 * nf;  // 16-B aligned: c0 is even
  for (int e = 2 * (int)threadIdx.x; e < ne; e += 2 * CB) {
    if (e + 1 < ne) {
      const d2 v = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(src + e));
      lds[e] = v[0];
      lds[e + 1] = v[1];
    } else {
      lds[e] = src[e];
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= cn) return;
  double *dst = soa + tiled(c0, tpad) + t;
  for (int f = 0; f < nf; ++f) dst[(int64_t)f * kLayoutTile] = lds[t * nf + f];
}

int launch_atm_unpack(const double *rec, double *soa, int64_t n_atmos, int nf, int64_t tpad, void *stream) {
  if (n_atmos <= 0 || nf <= 0) return 0;
  const unsigned blocks = (unsigned)((n_atmos + 255) / 256);
  hipLaunchKernelGGL(atm_unpack_kernel, dim3(blocks), dim3(256), (size_t)256 * nf * sizeof(double),
                     reinterpret_cast<hipStream_t>(stream), rec, soa, n_atmos, nf, tpad);
  return (int)hipGetLastError();
}

template <class R>
__global__ __launch_bounds__(256) void atmos_zero_kernel(const AtmosFused af, const int32_t *cells, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t a = cells[i];
#pragma unroll
  for (int k = 0; k < kFusedFields; ++k)
    if (af.out[k]) reinterpret_cast<R *>(af.out[k])[atm_at(a, af.out_stride, af.out_tpad)] = R(0);
}

int launch_atmos_zero(const AtmosFused &af, const int32_t *cells, int64_t n, bool f32, void *stream) {
  if (n <= 0) return 0;
  const int blocks = (int)((n + 255) / 256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (f32)
    hipLaunchKernelGGL(atmos_zero_kernel<float>, dim3(blocks), dim3(256), 0, s, af, cells, n);
  else
    hipLaunchKernelGGL(atmos_zero_kernel<double>, dim3(blocks), dim3(256), 0, s, af, cells, n);
  return (int)hipGetLastError();
}

int launch_atmos_fixup_group(const AtmosFused *afs, const int64_t *n_cells, int n, bool f32, void *stream, bool wide) {
  if (n < 1 || n > kMaxGroup) return (int)hipErrorInvalidValue;
  const int64_t kt = 64 * fused_cpl(f32, wide);
  FixupGroup g{};
  g.n = n;
  for (int m = 0; m < n; ++m) {
    g.af[m] = afs[m];
    const int64_t tiles = (n_cells[m] + kt - 1) / kt;
    g.first[m + 1] = g.first[m] + std::max<int64_t>(tiles - 1, 0) * kFusedFields;
  }
  if (g.first[n] == 0) return 0;
  const int blocks = (int)((g.first[n] + 255) / 256);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (f32 && wide)
    hipLaunchKernelGGL((atmos_fixup_group_kernel<float, tile_cells<kWideCpl>()>), dim3(blocks), dim3(256), 0, s, g);
  else if (f32)
    hipLaunchKernelGGL((atmos_fixup_group_kernel<float, tile_cells<kF32Cpl>()>), dim3(blocks), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL((atmos_fixup_group_kernel<double, tile_cells<2>()>), dim3(blocks), dim3(256), 0, s, g);
  return (int)hipGetLastError();
}

int launch_fill(double *x, int64_t n, double value, bool f32, int64_t tpad, void *stream) {
  if (n <= 0) return 0;
  if (!x || reinterpret_cast<uintptr_t>(x) % 16 || tpad < 0) return (int)hipErrorInvalidValue;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (f32)
    hipLaunchKernelGGL(fill_kernel<float>, dim3(grid_for((n + 3) / 4)), dim3(256), 0, s, reinterpret_cast<float *>(x), n,
                       (float)value, tpad);
  else
    hipLaunchKernelGGL(fill_kernel<double>, dim3(grid_for((n + 1) / 2)), dim3(256), 0, s, x, n, value, tpad);
  return (int)hipGetLastError();
}

int launch_receive(const ReceiveArgs &a, void *stream) {
  if (a.n <= 0 || a.nf <= 0) return 0;
  if (a.nf > kMaxReceiveFields || a.tpad < 0) return (int)hipErrorInvalidValue;
  for (int f = 0; f < a.nf; ++f)
    if (!a.src[f] || !a.dst[f] || reinterpret_cast<uintptr_t>(a.dst[f]) % 16) return (int)hipErrorInvalidValue;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!a.idx) {
    if (!a.row_ptr || !a.col || !a.w) return (int)hipErrorInvalidValue;
    if (a.f32)
      hipLaunchKernelGGL(receive_csr_kernel<float>, dim3(grid_for(a.n)), dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL(receive_csr_kernel<double>, dim3(grid_for(a.n)), dim3(256), 0, s, a);
    return (int)hipGetLastError();
  }
  if (reinterpret_cast<uintptr_t>(a.idx) % 16) return (int)hipErrorInvalidValue;
  const int c = a.f32 ? 4 : 2;
  const dim3 grid(grid_for((a.n + c - 1) / c));
  if (a.f32 && a.w)
    hipLaunchKernelGGL((receive_inject_kernel<float, true>), grid, dim3(256), 0, s, a);
  else if (a.f32)
    hipLaunchKernelGGL((receive_inject_kernel<float, false>), grid, dim3(256), 0, s, a);
  else if (a.w)
    hipLaunchKernelGGL((receive_inject_kernel<double, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((receive_inject_kernel<double, false>), grid, dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

// ---- field ranges (fcx_field_ranges, fcx_atmos_ranges, FCX_OPT_CHECK_FINITE) ----
// One lane's running result.  min / max start at +Inf / -Inf, the identities of fmin / fmax, and
// a NaN never enters them (fmin / fmax return the other operand: v_min / v_max in IEEE mode), so
// "every cell was NaN" is told from the counts at the very end.  Exact and independent of order.
template <class S>
struct RangeAcc {
  S mn, mx;
  int64_t nn, ni, first;
};
constexpr int64_t kNoCell = INT64_MAX;
template <class S>
__device__ __forceinline__ void range_take(RangeAcc<S> &a, S x, int64_t j) {
  if constexpr (sizeof(S) == 8) {
    a.mn = __builtin_fmin(a.mn, x);
    a.mx = __builtin_fmax(a.mx, x);
  } else {
    a.mn = __builtin_fminf(a.mn, x);
    a.mx = __builtin_fmaxf(a.mx, x);
  }
  const bool nan = x != x;
  const bool inf = !nan && (x == S(INFINITY) || x == -S(INFINITY));
  a.nn += nan ? 1 : 0;
  a.ni += inf ? 1 : 0;
  if ((nan || inf) && j < a.first) a.first = j;
}
__device__ __forceinline__ void range_fold(fcx_field_range &r, const fcx_field_range &o) {
  r.min = __builtin_fmin(r.min, o.min);
  r.max = __builtin_fmax(r.max, o.max);
  r.n_nan += o.n_nan;
  r.n_inf += o.n_inf;
  r.first_bad = o.first_bad < r.first_bad ? o.first_bad : r.first_bad;
}
// across the 64 lanes (every lane ends with the wave's result)
__device__ __forceinline__ void range_wave(fcx_field_range &r) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    fcx_field_range o;
    o.min = __shfl_xor(r.min, m, 64);
    o.max = __shfl_xor(r.max, m, 64);
    o.n_nan = __shfl_xor((long long)r.n_nan, m, 64);
    o.n_inf = __shfl_xor((long long)r.n_inf, m, 64);
    o.first_bad = __shfl_xor((long long)r.first_bad, m, 64);
    range_fold(r, o);
  }
}

// Grid (blocks, fields): block x of field y takes the 4096-cell layout tiles x, x + blocks, ...
// of the field, so a tile's cells share one tile shift and a field's blocks are a row of the
// grid.  A 16-B lane holds C cells; a wave instruction reads 1 KiB, a block's trip 4 KiB, and
// the kTrips loads of a whole tile are issued before the first value is looked at.  Plain
// loads: the arrays were just written (or are about to be read) by the flux pass.  The partial
// last tile goes vector by vector, its partial last vector cell by cell, nothing at or past n.
// Record fields (stride > 1) and arrays that are not 16-B aligned are read value by value:
// correct, not fast.
template <class S>
__global__ __launch_bounds__(256) void field_range_kernel(const RangeArgs a) {
  constexpr int C = 16 / sizeof(S);
  constexpr int kTrips = (int)(kLayoutTile / (256 * C));
  static_assert(kTrips >= 1 && kTrips * 256 * C == kLayoutTile, "a block's trips cover one layout tile");
  using V = typename std::conditional<sizeof(S) == 8, d2, f4>::type;
  const RangeField &fd = a.f[blockIdx.y];
  const S *__restrict__ base = reinterpret_cast<const S *>(fd.p);
  const int64_t n = fd.n, tiles = (n + kLayoutTile - 1) >> kLayoutShift;
  RangeAcc<S> acc{S(INFINITY), -S(INFINITY), 0, 0, kNoCell};
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t j0 = t << kLayoutShift;
    const S *__restrict__ tp = base + (j0 + t * fd.tpad) * fd.stride;  // tiled(j0, tpad) * stride
    if (fd.vec && j0 + kLayoutTile <= n) {
      V v[kTrips];
#pragma unroll
      for (int k = 0; k < kTrips; ++k) v[k] = gptr(reinterpret_cast<const V *>(tp))[k * 256 + threadIdx.x];
#pragma unroll
      for (int k = 0; k < kTrips; ++k)
#pragma unroll
        for (int i = 0; i < C; ++i) range_take(acc, (S)v[k][i], j0 + (int64_t)(k * 256 + threadIdx.x) * C + i);
    } else if (fd.vec) {
      for (int k = 0; k < kTrips; ++k) {
        const int64_t u = (int64_t)(k * 256 + threadIdx.x) * C, j = j0 + u;
        if (j + C <= n) {
          const V x = *gptr(reinterpret_cast<const V *>(tp + u));
#pragma unroll
          for (int i = 0; i < C; ++i) range_take(acc, (S)x[i], j + i);
        } else {
          for (int i = 0; i < C; ++i)
            if (j + i < n) range_take(acc, gptr(tp)[u + i], j + i);
        }
      }
    } else {
      for (int64_t u = threadIdx.x; u < kLayoutTile && j0 + u < n; u += 256)
        range_take(acc, gptr(tp)[u * fd.stride], j0 + u);
    }
  }
  fcx_field_range r{(double)acc.mn, (double)acc.mx, acc.nn, acc.ni, acc.first};
  range_wave(r);
  __shared__ fcx_field_range wave_part[4];
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) range_fold(r, wave_part[w]);
    a.partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
  }
}

// One wave per field folds the field's `blocks` partials and writes the result: NaN for min and
// max when no cell was a number (every cell NaN, or n = 0), -1 for first_bad when none was bad.
__global__ __launch_bounds__(64) void field_range_finish_kernel(const RangeArgs a, int32_t blocks) {
  const fcx_field_range *__restrict__ p = a.partial + (int64_t)blockIdx.x * blocks;
  fcx_field_range r{(double)INFINITY, -(double)INFINITY, 0, 0, kNoCell};
  for (int b = threadIdx.x; b < blocks; b += 64) range_fold(r, p[b]);
  range_wave(r);
  if (threadIdx.x == 0) {
    if (a.f[blockIdx.x].n - r.n_nan <= 0) r.min = r.max = (double)NAN;
    if (r.first_bad == kNoCell) r.first_bad = -1;
    a.out[blockIdx.x] = r;
  }
}

// Enough blocks to fill the device (2048 of 256 threads: 8 per CU), shared by the fields of the
// launch so that the partials stay within kRangePartials; never more than the longest field's tiles
int launch_field_ranges(RangeArgs a, void *stream) {
  if (a.nf <= 0) return 0;
  if (a.nf > kMaxRangeFields || !a.partial || !a.out) return (int)hipErrorInvalidValue;
  const size_t es = a.f32 ? 4 : 8;
  int64_t tiles = 1;
  for (int f = 0; f < a.nf; ++f) {
    RangeField &fd = a.f[f];
    if (fd.n < 0 || fd.tpad < 0 || fd.stride < 1 || (fd.n > 0 && !fd.p) || reinterpret_cast<uintptr_t>(fd.p) % es)
      return (int)hipErrorInvalidValue;
    fd.vec = fd.stride == 1 && reinterpret_cast<uintptr_t>(fd.p) % 16 == 0 && (fd.tpad * es) % 16 == 0;
    tiles = std::max(tiles, (fd.n + kLayoutTile - 1) >> kLayoutShift);
  }
  const int blocks = (int)std::min<int64_t>(tiles, kRangePartials / a.nf);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a.f32)
    hipLaunchKernelGGL(field_range_kernel<float>, dim3(blocks, a.nf), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(field_range_kernel<double>, dim3(blocks, a.nf), dim3(256), 0, s, a);
  if (hipError_t r = hipGetLastError()) return (int)r;
  hipLaunchKernelGGL(field_range_finish_kernel, dim3(a.nf), dim3(64), 0, s, a, (int32_t)blocks);
  return (int)hipGetLastError();
}

#elif FCX_KERNELS_WIDE_TU  // the launchers of the F32Wide instantiations

int launch_wide_fused(int variant, bool halo, bool ravg, bool nt, int blocks, hipStream_t s, const Params *dp,
                      const double *corr_m, const AtmosFused &af, int64_t lo, int64_t hi) {
  if (ravg && halo) return (int)hipErrorInvalidValue;
#define FCX_WIDE_ATM(VAR)                                                                            \
  if (ravg)  /* several types, the type-0 averages in registers */                                   \
    launch_atm<kWideCpl, F32Wide, VAR, 0, true>(nt, blocks, s, dp, corr_m, af, lo, hi);              \
  else if (halo)                                                                                     \
    launch_atm<kWideCpl, F32Wide, VAR, 1, false, false, true>(nt, blocks, s, dp, corr_m, af, lo, hi); \
  else                                                                                               \
    launch_atm<kWideCpl, F32Wide, VAR, 1, false>(nt, blocks, s, dp, corr_m, af, lo, hi);
  switch (variant) {
    case 1: FCX_WIDE_ATM(1) break;
    case 2: FCX_WIDE_ATM(2) break;
    case 3: FCX_WIDE_ATM(3) break;
    default: return (int)hipErrorInvalidValue;
  }
#undef FCX_WIDE_ATM
  return 0;
}

void launch_wide_cells(int c, const Params *hp, const LaunchConfig &lc, int blocks, hipStream_t s, const Params *dp,
                       const double *corr_m, int64_t lo, int64_t hi) {
  if (c == 4)
    launch_r<4, F32Wide>(hp, lc, blocks, s, dp, corr_m, lo, hi);
  else
    launch_r<1, F32Wide>(hp, lc, blocks, s, dp, corr_m, lo, hi);
}

void launch_wide_group(bool nt, bool halo, bool ravg, int blocks, hipStream_t s, const GroupArgs &g) {
  if (nt)
    launch_group_h<kWideCpl, F32Wide, true>(halo, ravg, blocks, s, g);
  else
    launch_group_h<kWideCpl, F32Wide, false>(halo, ravg, blocks, s, g);
}

#else  // FCX_KERNELS_CR_TU: the launchers of the F64Cr instantiations

int launch_cr_fused(int variant, const Params *hp, const LaunchConfig &lc, int blocks, hipStream_t s, const Params *dp,
                    const double *corr_m, const AtmosFused &af, int64_t lo, int64_t hi) {
  switch (variant) {
    case 1: return launch_atm_f64<1, F64Cr>(hp, lc, blocks, s, dp, corr_m, af, lo, hi);
    case 2: return launch_atm_f64<2, F64Cr>(hp, lc, blocks, s, dp, corr_m, af, lo, hi);
    case 3: return launch_atm_f64<3, F64Cr>(hp, lc, blocks, s, dp, corr_m, af, lo, hi);
    default: return (int)hipErrorInvalidValue;
  }
}

void launch_cr_cells(int c, const Params *hp, const LaunchConfig &lc, int blocks, hipStream_t s, const Params *dp,
                     const double *corr_m, int64_t lo, int64_t hi) {
  if (c == 2)
    launch_r<2, F64Cr>(hp, lc, blocks, s, dp, corr_m, lo, hi);
  else
    launch_r<1, F64Cr>(hp, lc, blocks, s, dp, corr_m, lo, hi);
}

void launch_cr_rec(int variant, bool nt, int blocks, hipStream_t s, const Params *dp, const double *corr_m, int64_t lo,
                   int64_t hi) {
  switch (variant) {
    case 1: launch_rec<1, F64Cr>(nt, blocks, s, dp, corr_m, lo, hi); break;
    case 2: launch_rec<2, F64Cr>(nt, blocks, s, dp, corr_m, lo, hi); break;
    default: launch_rec<3, F64Cr>(nt, blocks, s, dp, corr_m, lo, hi); break;
  }
}

void launch_cr_group(bool nt, bool halo, bool ravg, int blocks, hipStream_t s, const GroupArgs &g) {
  if (nt)
    launch_group_h<2, F64Cr, true>(halo, ravg, blocks, s, g);
  else
    launch_group_h<2, F64Cr, false>(halo, ravg, blocks, s, g);
}
#endif

}  // namespace fcx
