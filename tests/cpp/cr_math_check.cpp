// cr_math_check -- the host build of csrc/fcx_crmath.h over a file of arguments
// (tests/test_cr_math.py).  Plain C++: the header compiles without HIP, and inside its domains
// it uses IEEE operations only, so what this program prints is what the device computes.
//
//   cr_math_check exp IN OUT   IN: n doubles x
//   cr_math_check pow IN OUT   IN: n pairs (x, y)
// OUT: four doubles per case: the public function (cr_exp / cr_pow_exner), the head of the
// accurate phase called directly (NaN outside the domain, where it is not defined), 1.0 or
// 0.0 for "inside the domain", and the default build's function here (exp / exp(y * log x)).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "fcx_crmath.h"

int main(int argc, char **argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s exp|pow IN OUT\n", argv[0]);
    return 2;
  }
  const bool is_pow = std::strcmp(argv[1], "pow") == 0;
  if (!is_pow && std::strcmp(argv[1], "exp") != 0) return 2;
  std::FILE *f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[1024];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 1024, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  const size_t per = is_pow ? 2 : 1;
  if (in.size() % per) return 4;
  const size_t n = in.size() / per;
  std::vector<double> out(4 * n);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t i = 0; i < n; ++i) {
    if (is_pow) {
      const double x = in[2 * i], y = in[2 * i + 1];
      const bool dom = fcx::cr::pow_in_domain(x, y);
      out[4 * i + 0] = fcx::cr_pow_exner(x, y);
      out[4 * i + 1] = dom ? fcx::cr::cr_pow_accurate(x, y).h : nan;
      out[4 * i + 2] = dom ? 1.0 : 0.0;
      out[4 * i + 3] = std::exp(y * std::log(x));
    } else {
      const double x = in[i];
      const bool dom = fcx::cr::exp_in_domain(x);
      out[4 * i + 0] = fcx::cr_exp(x);
      out[4 * i + 1] = dom ? fcx::cr::cr_exp_accurate(x).h : nan;
      out[4 * i + 2] = dom ? 1.0 : 0.0;
      out[4 * i + 3] = std::exp(x);
    }
  }
  f = std::fopen(argv[3], "wb");
  if (!f) return 5;
  const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  std::fclose(f);
  if (!ok) return 6;
  std::printf("CR_MATH_CHECK_OK %zu\n", n);
  return 0;
}
