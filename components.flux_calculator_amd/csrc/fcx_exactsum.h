// fcx_exactsum.h -- the exact sum of doubles behind fcx_exact_sum (include/fcx.h): a fixed-point
// long accumulator.  Written once: compiled by the host compiler for the fcx_sum_* entry points
// and by the device compiler for the integral kernels (fcx_integrals.hip), as fcx_crmath.h is.
//
// value = sum_k limb[k] * 2^(32 k - 1088).  A finite double +-m * 2^q (m < 2^53, q >= -1074) sits
// at bit p = q + 1088 >= 14: its three 32-bit digits, those of m << (p & 31) < 2^84, go to limbs
// p >> 5 .. (p >> 5) + 2, added for a positive term and subtracted for a negative one.  DBL_MAX
// (p = 2059) touches limbs 64 and 65, the smallest denormal is limb[0] = 1 << 14; limb 67 only
// ever holds carries.  Every operation is an integer addition, so partial sums add
// associatively and the result is a pure function of the terms.
//
// INVARIANT: no limb reaches 2^62 in magnitude, anywhere.  One term moves a limb by less than
// 2^32, a canonical limb (below) is below 2^32 (limb 67: far smaller, the value is below
// 2^31 * 2^1024 * ranks), so carries are propagated (exsum_normalise)
//   * on the host after at most kExsumHostRun = 2^29 terms (2^29 * 2^32 + 2^32 < 2^62);
//   * on the device never inside a lane or a block: a block of the streaming launch takes at most
//     ceil(tiles / blocks) <= 2^31 / 4096 / 128 + 1 layout tiles of 4096 cells (the launcher
//     keeps at least min(tiles, 128) blocks per field), so a lane adds at most 2^16 + 16 terms
//     (< 2^49 per limb) and a block at most 2^24 + 4096 (< 2^57); but 2048 such partials could
//     reach 2^68, so every block normalises its partial before it stores it, and the finishing
//     launch adds at most 2048 canonical partials (< 2^43) before it normalises once more;
//   * in fcx_sum_merge on `other` alone first: a raw sum of 2^30 canonical sums has limbs up to
//     2^30 * (2^32 - 1) = 2^62 - 2^30, and the carry that arrives from the limb below is
//     below 2^30, so the invariant holds during that pass; the sum of two canonical sums
//     (< 2^33) is then normalised again.
//
// Canonical form: limbs 0..66 in [0, 2^32), limb 67 signed; a negative value is the two's
// complement over the 68 limbs (limb 67 < 0).  One value, one representation.
#pragma once
#include <cstdint>
#include "../../include/fcx.h"

#if defined(__HIPCC__)
#define FCX_XS_HD __host__ __device__ __forceinline__
#else
#define FCX_XS_HD inline
#endif

namespace fcx {

constexpr int kExsumLimbs = FCX_SUM_LIMBS;
constexpr int64_t kExsumHostRun = int64_t(1) << 29;
static_assert(kExsumLimbs == 68 && sizeof(fcx_exact_sum) == 576, "fcx_exact_sum: 68 limbs and four counts");

// what a term is: 0 a finite number (zeros included), 1 a NaN, 2 +Inf, 3 -Inf
FCX_XS_HD int exsum_class(uint64_t bits) {
  if (((bits >> 52) & 0x7ff) != 0x7ff) return 0;
  if (bits & ((uint64_t(1) << 52) - 1)) return 1;
  return (bits >> 63) ? 3 : 2;
}

// the digits of a finite double: limb index of the lowest (0 for a zero, whose digits are 0)
// and the three digits, each below 2^32; the sign is bit 63 of `bits`
struct ExsumDigits {
  int32_t limb;
  uint32_t d0, d1, d2;
};
FCX_XS_HD ExsumDigits exsum_digits(uint64_t bits) {
  const uint32_t e = (uint32_t)(bits >> 52) & 0x7ff;
  const uint64_t frac = bits & ((uint64_t(1) << 52) - 1);
  const uint64_t m = e ? (frac | (uint64_t(1) << 52)) : frac;
  const uint32_t p = (e ? e : 1u) + 13u;  // q + 1088, q = max(e, 1) - 1075
  const uint32_t s = p & 31u;
  const uint64_t lo = m << s;
  const uint64_t hi = (m >> 32) >> (32u - s);  // m >> (64 - s); s = 0 shifts the 21 bits out
  return ExsumDigits{(int32_t)(p >> 5), (uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi};
}

// carries from limb 0 upwards: limbs 0..66 into [0, 2^32), the rest into limb 67
FCX_XS_HD void exsum_normalise(int64_t *limb) {
  int64_t carry = 0;
  for (int k = 0; k < kExsumLimbs - 1; ++k) {
    const int64_t v = limb[k] + carry;
    limb[k] = v & 0xffffffffLL;
    carry = v >> 32;  // arithmetic: floor
  }
  limb[kExsumLimbs - 1] += carry;
}

// one finite term into unnormalised limbs
FCX_XS_HD void exsum_add_finite(int64_t *limb, uint64_t bits) {
  const ExsumDigits d = exsum_digits(bits);
  if (bits >> 63) {
    limb[d.limb] -= d.d0, limb[d.limb + 1] -= d.d1, limb[d.limb + 2] -= d.d2;
  } else {
    limb[d.limb] += d.d0, limb[d.limb + 1] += d.d1, limb[d.limb + 2] += d.d2;
  }
}

// Host only.  The canonical limbs rounded once, to nearest, ties to even; +-Inf beyond DBL_MAX; +0.0 for 0.
inline double exsum_round(const int64_t *limb) {
  // magnitude as 70 digits of 32 bits (limb 67 may be wider than 32 bits after merges)
  uint32_t d[kExsumLimbs + 2];
  const bool neg = limb[kExsumLimbs - 1] < 0;
  uint64_t top;
  if (neg) {
    uint64_t carry = 1;
    for (int k = 0; k < kExsumLimbs - 1; ++k) {
      const uint64_t t = (0xffffffffull - (uint64_t)limb[k]) + carry;
      d[k] = (uint32_t)t;
      carry = t >> 32;
    }
    top = ~(uint64_t)limb[kExsumLimbs - 1] + carry;
  } else {
    for (int k = 0; k < kExsumLimbs - 1; ++k) d[k] = (uint32_t)limb[k];
    top = (uint64_t)limb[kExsumLimbs - 1];
  }
  d[kExsumLimbs - 1] = (uint32_t)top;
  d[kExsumLimbs] = (uint32_t)(top >> 32);
  d[kExsumLimbs + 1] = 0;
  int hi = kExsumLimbs;
  while (hi >= 0 && !d[hi]) --hi;
  if (hi < 0) return 0.0;
  int P = 32 * hi + 31;
  while (!((d[hi] >> (P & 31)) & 1u)) --P;  // the leading bit, of weight 2^(P - 1088)
  const double inf = __builtin_inf();
  if (P - 1088 > 1023) return neg ? -inf : inf;
  auto bit = [&](int i) -> uint32_t { return i < 0 ? 0u : (d[i >> 5] >> (i & 31)) & 1u; };
  const int L = P - 52 > 14 ? P - 52 : 14;  // the last bit a double keeps (2^-1074 is bit 14)
  uint64_t M = 0;
  for (int i = P; i >= L; --i) M = (M << 1) | bit(i);
  bool sticky = false;
  for (int i = L - 2; i >= 0 && !sticky; --i) sticky = bit(i);
  if (bit(L - 1) && (sticky || (M & 1))) ++M;
  const double v = __builtin_ldexp((double)M, L - 1088);  // M <= 2^53: exact, or Inf past DBL_MAX
  return neg ? -v : v;
}

}  // namespace fcx
