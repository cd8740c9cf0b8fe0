// f32_physics_check -- the host build of csrc/fcx_physics.h at R = float over a table of cells
// (tests/test_f32_expect.py).  Plain C++: with __HIP_PLATFORM_AMD__ the HIP host headers make
// __device__ empty, and at R = float every operation of the header but the three transcendental
// sites is one IEEE single operation (-ffp-contract=off), so what this program writes is what
// the numpy float32 restatement tests/f32_expect.py must return, bit for bit.
//
// The sites: the header calls exp / log unqualified from inside namespace fcx.  Declared HERE,
// inside that namespace and before the include, fcx::exp(float) / fcx::log(float) hide the global
// ones for those calls (unqualified lookup stops at the innermost namespace that has the name,
// and a float argument brings in nothing through its type).  They are the double function rounded
// to float once -- the same function the test hands to the restatement -- so every formula
// downstream of a site is bit-comparable too, whatever this host's expf / logf round like.  The
// double overloads keep fcx_crmath.h's own calls what they were.
//
// fmax and sqrt get the same treatment for another reason: the device compiler's headers declare
// float fmax(float, float) and float sqrt(float) in the global namespace, a plain host compiler's
// <math.h> only the double ones there -- the header's fmax(vel, R(kUmin)) would return a double
// and a * fmax(..) * ps be formed in double and rounded once, which is not what the device does.
// Here they are fmaxf and sqrtf, single operations as on the device.
//
//   f32_physics_check IN OUT
// IN: n rows of kIn floats (the columns below); OUT: n rows of kOut floats.
#include <cmath>
#include <cstdio>
#include <vector>

namespace fcx {
inline float exp(float x) { return (float)::exp((double)x); }
inline float log(float x) { return (float)::log((double)x); }
inline double exp(double x) { return ::exp(x); }
inline double log(double x) { return ::log(x); }
inline float fmax(float a, float b) { return ::fmaxf(a, b); }
inline double fmax(double a, double b) { return ::fmax(a, b); }
inline float sqrt(float x) { return ::sqrtf(x); }
inline double sqrt(double x) { return ::sqrt(x); }
}  // namespace fcx

#include "fcx_physics.h"

enum In { FICE, PS, PA, TS, TA, QA, QS, U, V, A, BIAS, F1, F2, kIn };
enum Out {
  QSUR, VEL, MEVA_CCLM, MEVA_RCO, HSEN_CCLM, HSEN_RCO, MOM_CCLM_RATE, MOM_RCO_RATE, RBBR, T_TILDE,
  RATE_NUM, TA_EXNER, POW_EXNER, MOM_NUM, MOM_CCLM_RATE_NUM, MEVA_CCLM_NUM, HSEN_CCLM_NUM, SITE_EXP,
  UMOM_CCLM, VMOM_RCO, HLAT_WATER, HLAT_ICE, MEVA_BIAS, AVERAGE, kOut
};

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<float> in;
  float buf[1024];
  size_t got;
  while ((got = std::fread(buf, sizeof(float), 1024, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  if (in.size() % kIn) return 4;
  const size_t n = in.size() / kIn;
  std::vector<float> out((size_t)kOut * n);
  using namespace fcx;
  for (size_t i = 0; i < n; ++i) {
    const float *x = &in[i * kIn];
    float *o = &out[i * kOut];
    const float vel = wind<float>(x[U], x[V]);
    o[QSUR] = qsur_cclm<float>(x[FICE], x[PS], x[TS]);
    o[VEL] = vel;
    o[MEVA_CCLM] = meva_cclm<float>(x[A], x[PS], x[QA], x[QS], x[TA], vel);  // P2: TATM in the T_s slot
    o[MEVA_RCO] = meva_rco<float>(x[QA], x[TS], vel);
    o[HSEN_CCLM] = hsen_cclm<float>(x[A], x[PA], x[PS], x[QA], x[TA], x[TS], vel);  // P3: QATM in the q_s slot
    o[HSEN_RCO] = hsen_rco<float>(x[TA], x[TS], vel);
    o[MOM_CCLM_RATE] = mom_cclm_rate<float>(x[A], x[PS], x[QS], x[TS], vel);
    o[MOM_RCO_RATE] = mom_rco_rate<float>(vel);
    o[RBBR] = rbbr_stbo<float>(x[TS]);
    o[T_TILDE] = t_tilde<float>(x[TS], x[QS]);
    o[RATE_NUM] = rate_num<float>(x[A], vel, x[PS]);
    o[TA_EXNER] = ta_exner<float>(x[TA], x[PS], x[PA]);
    o[POW_EXNER] = pow_exner<float>(x[PS] / x[PA], float(kRd / kCp));
    o[MOM_NUM] = mom_num<float>(x[A], vel, x[PS]);
    o[MOM_CCLM_RATE_NUM] = mom_cclm_rate_num<float>(o[MOM_NUM], x[QS], x[TS]);
    o[MEVA_CCLM_NUM] = meva_cclm_num<float>(o[RATE_NUM], x[QA], x[QS], x[TA]);
    o[HSEN_CCLM_NUM] = hsen_cclm_num<float>(o[RATE_NUM], x[QA], x[TS], o[TA_EXNER]);
    o[SITE_EXP] = site_exp<false, float>(x[QS]);
    // the glue of fcx_kernels.hip momentum<> / process<> on these values
    o[UMOM_CCLM] = -(o[MOM_CCLM_RATE] * x[U]);
    o[VMOM_RCO] = -(o[MOM_RCO_RATE] * x[V]);
    o[HLAT_WATER] = o[MEVA_RCO] * float(kLv);
    o[HLAT_ICE] = o[MEVA_RCO] * float(kLs);
    o[MEVA_BIAS] = o[MEVA_CCLM] + x[BIAS];
    float acc = 0.0f;
    acc = acc + o[MEVA_CCLM] * x[F1];
    acc = acc + o[MEVA_RCO] * x[F2];
    o[AVERAGE] = acc;
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  const bool ok = std::fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
  std::fclose(f);
  if (!ok) return 6;
  std::printf("F32_PHYSICS_CHECK_OK %zu\n", n);
  return 0;
}
