// fcx_crmath.h -- correctly rounded exp and Exner power for the fp64 engine (FCX_OPT_CR_MATH).
//
//   cr_exp(x)            the double nearest exp(x), ties to even
//   cr_pow_exner(x, y)   the double nearest x**y
//
// "Correctly rounded" is a definition that no library release can move: the result is a
// function of the argument's bits alone.  Inside the stated domains the functions use only
// + - * /, explicit __builtin_fma (an explicit fma is an operation, not a contraction: the
// build's -ffp-contract=off stays), comparisons, selects and integer / bit operations, all
// of them IEEE-754 operations with one defined result.  The host build (plain g++) and the
// device build (hipcc, gfx950) therefore return the same bits, and a CPU program can check
// what the GPU computes (tests/cpp/cr_math_check.cpp).
//
// DOMAINS
//   cr_exp:        2^-30 <= |x| <= 690
//   cr_pow_exner:  0.5 <= x <= 2, x != 1, 1/16 <= y <= 1        (so |y log x| <= ln 2)
// Outside them a call returns what the default build computes at that site, exp(x) and
// exp(y * log(x)): NaN, Inf, zero, negative, subnormal, overflowing and underflowing
// arguments behave as in the default build by construction.  (Below 2^-30 exp(x) lies
// within 2^-31 ulp of 1 +- |x| and midpoints of the form 1 - 2^-54 are approached to 2^-109:
// no fixed-precision evaluation decides those, and no flux site forms such an argument
// unless TSUR equals the formula's reference temperature to 1e-8 K.)
//
// METHOD: one accurate phase for every lane, in double-double arithmetic.
// A double-double (dd) is an unevaluated sum h + l of two doubles with |l| <= ulp(h)/2.
// u = 2^-53.  The building blocks and their relative error bounds (Joldes, Muller, Popescu,
// "Tight and rigorous error bounds for basic building blocks of double-word arithmetic",
// ACM TOMS 44(2), 2017; Dekker 1971 and Knuth for the error-free transformations):
//   two_sum, fast_two_sum (|a| >= |b| or a = 0), two_prod (fma)   exact
//   dd_mul    dd * dd      (their Alg. 11)                         <= 5 u^2
//   dd_mul_d  dd * double  (their Alg. 9)                          <= 2 u^2  (3 u^2 used)
//   dd_add    dd + dd with |a.h| >= |b.h| and |a.h + b.h| >= |a.h| / 2 (every use below adds a
//             term at most half the size, of either sign), or a = 0 (then b is returned):
//             s + e = a.h + b.h exactly; w = a.l + b.l and e + w round once each, |w| <=
//             2 u |a.h|, |e| <= u |s|: error <= u (2 u |a.h|) + u (u |s| + 2 u |a.h|) <=
//             4 u^2 |a.h| + u^2 |s| <= 9 u^2 |s|.  Where |b.h| <= |a.h| / 8 (every use but the
//             last of log_dd): |s| >= 7/8 |a.h| and |w| <= 1.2 u |a.h|:  <= 4 u^2 of the sum;
//             the bounds below use 7 u^2 for it                     <= 7 u^2  (9 u^2 in log_dd's last)
//   dd_div_d  double / dd: q1 = RN(n / d.h); n - q1 d.h is exact (remainder of a correctly
//             rounded quotient, one fma); q2 = RN((that - q1 d.l) / d.h) carries three
//             roundings and the replacement of d by d.h, each <= u |q2|, |q2| <= 2 u |q1|
//                                                                  <= 5 u^2
//
// exp_dd(xh + xl), |xh| <= 690, |xl| <= 2^-53 (0 for cr_exp):
//   1. k = RN(xh * RN(N / ln2)) by the 1.5 * 2^52 shift, N = 16: |k| <= 15929 < 2^15.
//      ln2/N = Lhi + Lmid + Llo with Lhi of 38 bits: k Lhi is exact, and xh - k Lhi is exact
//      (k = 0: nothing is subtracted; otherwise the operands are within a factor 2: Sterbenz).
//      k Lmid is taken exactly (two_prod); the tail xl - lo(k Lmid) - k Llo + (two_sum error) is
//      summed in double: its terms are below 2^-52 for a dd argument (below 2^-80 for cr_exp),
//      three roundings, <= 2^-103.4 absolute (2^-131); |Lhi + Lmid + Llo - ln2/N| <= 2^-150, times
//      k: 2^-135.  So r = rh + rl = x - k ln2/N to 6 u^2 absolute (cr_exp: 2^-130), |r| <= 0.02167
//      = ln2/32 (1 + 2^-38).
//   2. expm1(r) = r + r^2 (1/2 + r (1/6 + ... + r^11/13!)).  The truncation is below
//      r^14/14! (1 + r) <= 2^-113.7 absolute, 2^-108 of expm1(r).  The terms 1/7! .. 1/13! run
//      as a double Horner chain q(rh): relative error 2^-51, weight r^7/7! / r <= 2^-45 of the
//      sum: 2^-96 of expm1(r), which is 2^-101.5 of the result (|expm1 r| <= 0.022).  1/6! .. 1/2!
//      are dd constants, each step P_k = c_k + r P_(k+1) one dd_mul and one dd_add (|c_k| >=
//      8 |r P_(k+1)|): <= 12 u^2 per step, relative to P_k; the error of step k+1 reaches P_k
//      scaled by |r| < 2^-5, so every P_k holds <= 13 u^2.  r^2: 15 u^2; r^2 P_2: <= 33 u^2 of a
//      term <= 0.011 |r|; the sum with r: 7 u^2.  expm1(r) carries <= 8 u^2 + 2^-101.5/0.022...
//      stated against the RESULT: (8 u^2 + 2^-96) * 0.022 <= 0.2 u^2 + 2^-101.5.
//   3. exp(x) = 2^e T_j (1 + expm1 r), k = 16 e + j.  T_j = 2^(j/16) is a dd constant (0.5 u^2),
//      T_j * expm1(r): 5 u^2 of a term <= 0.022; T_j + that: 7 u^2.  The 16 table values are
//      chosen by a tree of selects on the bits of j -- literals in the instruction stream, no
//      memory access, so no vector-memory wait enters the kernels' store phase.
//      2^e is exact (the result is normal: 2^-996 < exp(x) < 2^996).
//   Total for cr_exp: 0.5 + 0.2 + 0.2 + 7 u^2 + 2^-101.5 + 2^-130 <= 8 u^2 + 2^-101.5 < 2^-100.9.
//   With a dd argument: + 6 u^2 from the reduction                                < 2^-100.5.
//
// log_dd(x), 0.5 <= x <= 2:
//   x = 2^e m exactly with e in {-1, 0, 1} and m in [sqrt(1/2) (1 - u), sqrt(2) (1 + u)].
//   s = (m - 1) / (m + 1): m - 1 is exact (Sterbenz), m + 1 an exact dd (two_sum); dd_div_d:
//   5 u^2.  |s| <= 0.17158 = 2^-2.54.
//   log m = 2 s (1 + s^2 (1/3 + s^2/5 + ... + s^38/41)).  Truncation: s^42/43 < 2^-112 of log m.
//   1/23 .. 1/41 run as a double Horner chain in hi(s^2): relative 2^-51 on a term of weight
//   s^22/23 <= 2^-60.4: 2^-111.  1/21 .. 1/3 are dd constants, each step <= 12 u^2 relative to
//   P_k, the previous step's error scaled by s^2 <= 0.0295: every P_k holds <= 13 u^2.
//   s^2: 15 u^2.  s^2 P_1: <= 33 u^2 of a term <= 0.0099; s * that: <= 43 u^2 of a term <=
//   0.0099 |s|: 0.43 u^2; the sum with s: 7 u^2.  log m: 5 + 0.43 + 7 u^2 + 2^-111 <= 13 u^2.
//   log x = e ln2 + log m: ln2 as a dd (0.5 u^2), e ln2 exact, |log m| <= |ln2| / 2 (1 + 2u);
//   absolute error <= 0.6932 (0.5 + 3.5) u^2 + 0.3466 * 13 u^2 <= 7.3 u^2 on |log x| >= 0.3465
//   when e != 0: <= 22 u^2 relative; with e = 0 the 13 u^2 of log m.  (The add is skipped for
//   e = 0 by its own rule a = 0: it then returns log m unchanged.)
//
// cr_pow_exner: a = y * log x by dd_mul_d: <= 25 u^2 relative, |a| <= 0.6932 (y <= 1), so
//   <= 17.4 u^2 absolute = relative in exp(a); exp_dd with a dd argument adds 2^-100.5:
//   total <= 17.4 u^2 + 2^-100.5 < 2^-100.  The required bound is 2^-95 (2048 u^2): the exact
//   value would have to lie within 2^-47 ulp of a rounding midpoint for the result to be
//   misrounded, an expected 2 * 2.47e9 * 2^-47 = 3.5e-5 cells of a full-grid report.
//
// Why one phase: a Ziv fast phase (a quarter of the operations, with the accurate phase taken
// by about one lane in 1e5, so by one wave in 1,600) would make the sites several times
// cheaper in time.  It would not make the kernels smaller: the accurate phase stays inlined as
// the fallback, so the flux kernels hold their registers for the worst path either way, and
// they would run at the same two waves per SIMD.  It has not been built or measured; the cost
// figures of DESIGN.md 3 are those of this single phase, and a fast phase in front of it is
// the next step.  The accurate phase below is what that fallback would be, and it is exported
// as such (cr_exp_accurate / cr_pow_accurate) so that the tests call it directly.
#pragma once

#include <cmath>
#include <cstdint>

#include "fcx_crmath_tables.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FCX_CR_HD __host__ __device__ __forceinline__
#else
#define FCX_CR_HD inline
#endif

namespace fcx {
namespace cr {

struct dd {
  double h, l;
};

FCX_CR_HD dd two_sum(double a, double b) {
  const double s = a + b;
  const double bb = s - a;
  return dd{s, (a - (s - bb)) + (b - bb)};
}
// |a| >= |b|, or a = 0
FCX_CR_HD dd fast_two_sum(double a, double b) {
  const double s = a + b;
  return dd{s, b - (s - a)};
}
FCX_CR_HD dd two_prod(double a, double b) {
  const double p = a * b;
  return dd{p, __builtin_fma(a, b, -p)};
}
FCX_CR_HD dd dd_mul(dd a, dd b) {
  const dd p = two_prod(a.h, b.h);
  const double t = __builtin_fma(a.l, b.h, a.h * b.l);
  return fast_two_sum(p.h, p.l + t);
}
FCX_CR_HD dd dd_mul_d(dd a, double b) {
  const dd p = two_prod(a.h, b);
  return fast_two_sum(p.h, __builtin_fma(a.l, b, p.l));
}
// |a.h| >= 2 |b.h|, or a = 0
FCX_CR_HD dd dd_add(dd a, dd b) {
  const dd s = fast_two_sum(a.h, b.h);
  return fast_two_sum(s.h, s.l + (a.l + b.l));
}
FCX_CR_HD dd dd_div_d(double n, dd d) {
  const double q1 = n / d.h;
  const double rem = __builtin_fma(-q1, d.h, n);  // exact
  const double q2 = (rem - q1 * d.l) / d.h;
  return fast_two_sum(q1, q2);
}

FCX_CR_HD double bits_to_double(uint64_t b) { return __builtin_bit_cast(double, b); }
FCX_CR_HD uint64_t double_to_bits(double x) { return __builtin_bit_cast(uint64_t, x); }

// entry j of a 16-entry table of literals, by selects on the bits of j
#define FCX_CR_SEL2(b, a0, a1) ((b) ? (a1) : (a0))
#define FCX_CR_SEL4(b0, b1, a0, a1, a2, a3) FCX_CR_SEL2(b1, FCX_CR_SEL2(b0, a0, a1), FCX_CR_SEL2(b0, a2, a3))
#define FCX_CR_SEL16(W)                                                                                        \
  FCX_CR_SEL4(b2, b3, FCX_CR_SEL4(b0, b1, FCX_CRT_T0_##W, FCX_CRT_T1_##W, FCX_CRT_T2_##W, FCX_CRT_T3_##W),       \
              FCX_CR_SEL4(b0, b1, FCX_CRT_T4_##W, FCX_CRT_T5_##W, FCX_CRT_T6_##W, FCX_CRT_T7_##W),               \
              FCX_CR_SEL4(b0, b1, FCX_CRT_T8_##W, FCX_CRT_T9_##W, FCX_CRT_T10_##W, FCX_CRT_T11_##W),             \
              FCX_CR_SEL4(b0, b1, FCX_CRT_T12_##W, FCX_CRT_T13_##W, FCX_CRT_T14_##W, FCX_CRT_T15_##W))

// exp(xh + xl) as a dd, relative error < 2^-100.5; |xh| <= 690, |xl| <= 2^-53 (header comment)
FCX_CR_HD dd exp_dd(double xh, double xl) {
  using namespace crt;
  static_assert(kExpN == 16, "the select tree and the shifts below are written for N = 16");
  // 1. reduction
  const double shift = 0x1.8p52;
  const double t = xh * kInvL + shift;
  const double kd = t - shift;
  const int32_t k = (int32_t)(uint32_t)double_to_bits(t);
  const double a = xh - kd * kLhi;  // both exact
  const dd pm = two_prod(kd, kLmid);
  const dd s = two_sum(a, -pm.h);
  const double tail = ((xl - pm.l) - kd * kLlo) + s.l;
  const dd r = two_sum(s.h, tail);
  // 2. expm1(r)
  double q = kE13;
  q = __builtin_fma(q, r.h, kE12);
  q = __builtin_fma(q, r.h, kE11);
  q = __builtin_fma(q, r.h, kE10);
  q = __builtin_fma(q, r.h, kE9);
  q = __builtin_fma(q, r.h, kE8);
  q = __builtin_fma(q, r.h, kE7);
  dd p = dd_add(dd{kE6h, kE6l}, dd_mul_d(r, q));
  p = dd_add(dd{kE5h, kE5l}, dd_mul(r, p));
  p = dd_add(dd{kE4h, kE4l}, dd_mul(r, p));
  p = dd_add(dd{kE3h, kE3l}, dd_mul(r, p));
  p = dd_add(dd{kE2h, kE2l}, dd_mul(r, p));
  const dd em1 = dd_add(r, dd_mul(dd_mul(r, r), p));
  // 3. 2^e T_j (1 + expm1 r)
  const bool b0 = k & 1, b1 = k & 2, b2 = k & 4, b3 = k & 8;
  const dd T = dd{FCX_CR_SEL16(HI), FCX_CR_SEL16(LO)};
  const dd y = dd_add(T, dd_mul(T, em1));
  const double scale = bits_to_double((uint64_t)(int64_t)((k >> 4) + 1023) << 52);
  return dd{y.h * scale, y.l * scale};
}

// log(x) as a dd, relative error <= 22 u^2; 0.5 <= x <= 2 (header comment)
FCX_CR_HD dd log_dd(double x) {
  using namespace crt;
  const bool up = x > kSqrt2, dn = x < kSqrtHalf;
  const double m = up ? x * 0.5 : dn ? x * 2.0 : x;
  const double e = up ? 1.0 : dn ? -1.0 : 0.0;
  const dd s = dd_div_d(m - 1.0, two_sum(m, 1.0));
  const dd z = dd_mul(s, s);
  double q = kA20;
  q = __builtin_fma(q, z.h, kA19);
  q = __builtin_fma(q, z.h, kA18);
  q = __builtin_fma(q, z.h, kA17);
  q = __builtin_fma(q, z.h, kA16);
  q = __builtin_fma(q, z.h, kA15);
  q = __builtin_fma(q, z.h, kA14);
  q = __builtin_fma(q, z.h, kA13);
  q = __builtin_fma(q, z.h, kA12);
  q = __builtin_fma(q, z.h, kA11);
  dd p = dd_add(dd{kA10h, kA10l}, dd_mul_d(z, q));
  p = dd_add(dd{kA9h, kA9l}, dd_mul(z, p));
  p = dd_add(dd{kA8h, kA8l}, dd_mul(z, p));
  p = dd_add(dd{kA7h, kA7l}, dd_mul(z, p));
  p = dd_add(dd{kA6h, kA6l}, dd_mul(z, p));
  p = dd_add(dd{kA5h, kA5l}, dd_mul(z, p));
  p = dd_add(dd{kA4h, kA4l}, dd_mul(z, p));
  p = dd_add(dd{kA3h, kA3l}, dd_mul(z, p));
  p = dd_add(dd{kA2h, kA2l}, dd_mul(z, p));
  p = dd_add(dd{kA1h, kA1l}, dd_mul(z, p));
  const dd half = dd_add(s, dd_mul(s, dd_mul(z, p)));  // log(m) / 2
  return dd_add(dd{e * kLn2h, e * kLn2l}, dd{2.0 * half.h, 2.0 * half.l});
}

FCX_CR_HD bool exp_in_domain(double x) {
  const double ax = __builtin_fabs(x);
  return ax >= 0x1p-30 && ax <= 690.0;  // false for NaN
}
FCX_CR_HD bool pow_in_domain(double x, double y) {
  return x >= 0.5 && x <= 2.0 && x != 1.0 && y >= 0.0625 && y <= 1.0;  // false for NaN
}

// The accurate phase itself: the dd value whose head is the result.  Arguments inside the domain.
FCX_CR_HD dd cr_exp_accurate(double x) { return exp_dd(x, 0.0); }
FCX_CR_HD dd cr_pow_accurate(double x, double y) {
  const dd a = dd_mul_d(log_dd(x), y);
  return exp_dd(a.h, a.l);
}

}  // namespace cr

// The double nearest exp(x); outside 2^-30 <= |x| <= 690 the default build's exp(x).
FCX_CR_HD double cr_exp(double x) {
  if (!cr::exp_in_domain(x)) return exp(x);
  return cr::cr_exp_accurate(x).h;
}

// The double nearest x**y; outside 0.5 <= x <= 2, x != 1, 1/16 <= y <= 1 the default build's
// exp(y * log(x)).
FCX_CR_HD double cr_pow_exner(double x, double y) {
  if (!cr::pow_in_domain(x, y)) return exp(y * log(x));
  return cr::cr_pow_accurate(x, y).h;
}

}  // namespace fcx
