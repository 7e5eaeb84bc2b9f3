// div_by_int_rn (attpc_engine_amd/csrc/div_rn.hpp) against the host's IEEE division: the operands peaks.hip meets
// (h - y[i] over a sample difference, windows_edge - centroid over the edge span), random normal operands over 80
// binades with divisors up to 2^31 - 1 of either sign, exact quotients, and zero / subnormal / infinity / NaN.
// Prints "n=<operands> bad=<mismatches>" and returns bad != 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "div_rn.hpp"

static bool same(double a, double b) {
  if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
  return std::memcmp(&a, &b, sizeof a) == 0;
}

int main() {
  std::mt19937_64 g(1);
  long bad = 0, n = 0;
  auto check = [&](double a, int32_t d, double want) {
    const double q = attpc::div_by_int_rn(a, d);
    ++n;
    if (!same(q, want)) {
      if (bad < 10) std::printf("a=%a d=%d got %a want %a\n", a, d, q, want);
      ++bad;
    }
  };
  for (long it = 0; it < 4000000; ++it) {
    int32_t d;
    double a;
    switch (it % 4) {
      case 0:  // width: a in [0, d), d a sample difference
        d = (int32_t)(g() % 8190) + 1;
        a = std::fmod((double)(g() % 4095) + (double)(g() >> 11) * 0x1p-53, (double)d);
        break;
      case 1: {  // any normal operand, any divisor
        d = (int32_t)(g() % 2147483647u) + 1;
        if (g() & 1) d = -d;
        uint64_t b = g();
        b = (b & 0x800fffffffffffffull) | ((uint64_t)(1023 - 40 + g() % 80) << 52);
        std::memcpy(&a, &b, sizeof a);
        break;
      }
      case 2:  // z: windows_edge - centroid over the span of the edges
        d = (int32_t)(g() % 600) + 1;
        a = 512.0 - ((double)(g() % 512) + (double)(g() >> 11) * 0x1p-53);
        break;
      default:  // quotients that are exact or exactly half way
        d = (int32_t)(g() % 8190) + 1;
        a = (double)(int64_t)(g() % (uint64_t)(d * 4ll + 1)) * 0.25;
    }
    check(a, d, a / (double)d);
  }
  check(0.0, 7, 0.0);
  check(-0.0, 7, -0.0);
  check(0.0, -7, -0.0);
  check(4.9e-324, 3, 0.0);   // a subnormal operand counts as zero (stated in the header)
  check(-1.0e-310, 3, -0.0);
  check(INFINITY, 5, INFINITY);
  check(INFINITY, -5, -INFINITY);
  check(-INFINITY, 5, -INFINITY);
  check(NAN, 5, NAN);
  std::printf("n=%ld bad=%ld\n", n, bad);
  return bad != 0;
}
