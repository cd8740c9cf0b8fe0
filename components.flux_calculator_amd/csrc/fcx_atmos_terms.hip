// fcx_atmos_terms.hip -- FCX_OPT_ATMOS_INVARIANT: the terms of the atmosphere cells a rank shares
// with its neighbours.  A translation unit of its own: nothing here is shared with the flux
// kernels of fcx_kernels.hip but the addressing rules of fcx_internal.h.
//
// An atmosphere value is out[a] = sum_x w[x] * field[x], summed in increasing x from 0.0
// (fcx.h).  Where the exchange cells of one atmosphere cell lie on several ranks, partial sums
// added by the all-reduce are another association of the same terms, and the last bits move
// with the decomposition.  With the option on the ranks exchange the TERMS instead: every rank
// stores fl(w[x] * field[x]) of its own cells of the shared atmosphere cell at the cell's link
// position, the positions of the other ranks stay +0.0, and the one fp64 sum all-reduce the
// step already has carries each term exactly (x + 0 + ... + 0 = x; a -0.0 term arrives as
// +0.0).  The ordered finish (atmos_finish_kernel) then adds the K positions in order on every
// rank: the sequential sum of a one-rank engine, bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include "fcx_internal.h"

#pragma clang fp contract(off)

namespace fcx {

namespace {

struct TermsGroup {
  int32_t n;
  int32_t pad;
  AtmosArgs a[kMaxGroup];
};

// grid (blocks, 2, members): blockIdx.z is the engine, blockIdx.y the side (0: the first local
// atmosphere cell and boundary `left`, 1: the last one and `right`), the x blocks stride over
// (field, position) with the position fastest, so consecutive lanes read consecutive exchange
// cells.  The map is sorted (the engine refuses the option otherwise): link k is exchange cell k.
// The product is the fix-up's own operation (fixup_one): one IEEE multiply, fp32 fields widened.
// Nothing is added here, so every store is a plain vector store of one double.
template <class R>
__global__ __launch_bounds__(256) void atmos_terms_kernel(const TermsGroup g) {
  const AtmosArgs &a = g.a[blockIdx.z];
  const int side = (int)blockIdx.y;
  const int32_t K = a.terms_k;
  if (K <= 0 || a.n_atmos <= 0 || !a.shared) return;
  const int32_t slot = side ? a.right : a.left;
  if (slot < 0) return;
  // one local atmosphere cell shared on both sides (left == right): the left side stores it
  if (side && a.n_atmos == 1 && a.left >= 0) return;
  const int64_t c = side ? a.n_atmos - 1 : 0;
  // the cell's position on this rank: the last cell, when it is not also the first, begins here
  const int32_t pos0 = (c == 0 && a.left >= 0) ? a.left_pos : 0;
  const int32_t k0 = a.row_ptr[c], cnt = a.row_ptr[c + 1] - k0;
  double *row = a.shared + (int64_t)slot * a.stride + a.term0;
  const int64_t items = (int64_t)cnt * a.nf;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(i / cnt);
    const int32_t p = (int32_t)(i - (int64_t)f * cnt);
    if (pos0 + p >= K) continue;  // (the engine has checked left_pos + cells <= K at commit)
    const int32_t x = k0 + p;
    const R *xf = reinterpret_cast<const R *>(a.x[f]);
    row[(int64_t)a.scol[f] * K + pos0 + p] = a.w[x] * (double)xf[tiled(x, a.tpad)];
  }
}

}  // namespace

int launch_atmos_terms(const AtmosArgs *as, int n, int64_t max_items, void *stream) {
  if (n < 1 || n > kMaxGroup) return (int)hipErrorInvalidValue;
  TermsGroup g{};
  g.n = n;
  for (int k = 0; k < n; ++k) {
    if (as[k].f32 != as[0].f32 || as[k].col || as[k].nf > kMaxAtmosFields || as[k].terms_k > kMaxAtmosTerms ||
        (as[k].terms_k > 0 && as[k].stride < as[k].term0 * (1 + as[k].terms_k)))
      return (int)hipErrorInvalidValue;
    g.a[k] = as[k];
  }
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>((max_items + 255) / 256, 1), 16);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (as[0].f32)
    hipLaunchKernelGGL(atmos_terms_kernel<float>, dim3(blocks, 2, n), dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL(atmos_terms_kernel<double>, dim3(blocks, 2, n), dim3(256), 0, s, g);
  return (int)hipGetLastError();
}

}  // namespace fcx
