// The closed form of the clipped integral (attpc_engine_amd/csrc/spyral_integral.hpp: the tables built from a response
// and 4095 k + q tail[k]) against the sum of the 512 products response[i] * q, each formed and clipped at 4095 in double
// as the reference's loop forms them, added in long double (64-bit mantissa: the sum of 512 terms is good to 3e-17).
//   spyral_integral_check <file of n x 512 doubles>     (the responses tests/test_spyral_cpu.py writes)
// Charges: 100 per decade over 1e0 ... 1e16, and for every sample r > 0 the charges either side of r q == 4095: the
// quotient 4095 / r, its two neighbours in double and the whole numbers below and above it (crossings up to 1e300).
// Prints "response <i>: n=<charges> worst=<relative error> at q=<charge> k=<clipped samples>" per response and
// returns 1 if any worst error is above 1e-12.  (A response with negative lobes has a clipped sum that changes sign
// at some charge; the relative error of any double formula grows towards that charge, and the figure printed is that
// of the nearest charge of the grid.)
#include <cmath>
#include <cstdio>
#include <vector>

#include "spyral_integral.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return std::fprintf(stderr, "usage: %s <responses.f64>\n", argv[0]), 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  std::vector<double> all;
  double buf[attpc::SPYRAL_SAMPLES];
  while (std::fread(buf, sizeof(double), attpc::SPYRAL_SAMPLES, f) == (size_t)attpc::SPYRAL_SAMPLES) all.insert(all.end(), buf, buf + attpc::SPYRAL_SAMPLES);
  std::fclose(f);
  const int n_resp = (int)(all.size() / attpc::SPYRAL_SAMPLES);
  if (n_resp == 0) return std::fprintf(stderr, "no response in %s\n", argv[1]), 2;
  static_assert(sizeof(long double) > sizeof(double), "the yardstick needs an extended long double");
  bool bad = false;
  for (int ri = 0; ri < n_resp; ++ri) {
    const double* r = all.data() + (size_t)ri * attpc::SPYRAL_SAMPLES;
    double sorted[attpc::SPYRAL_SAMPLES], tail[attpc::SPYRAL_SAMPLES + 1];
    attpc::spyral_integral_tables(r, sorted, tail);
    std::vector<double> charges;
    for (int i = 0; i <= 1600; ++i) charges.push_back(std::pow(10.0, (double)i / 100.0));
    for (int i = 0; i < attpc::SPYRAL_SAMPLES; ++i) {
      if (!(r[i] > 0.0)) continue;
      const double qc = attpc::SPYRAL_ADC_MAX / r[i];
      if (!(qc < 1e300)) continue;
      for (double q : {qc, std::nextafter(qc, 0.0), std::nextafter(qc, INFINITY), std::floor(qc), std::floor(qc) + 1.0}) charges.push_back(q);
    }
    double worst = 0.0, worst_q = 0.0;
    int worst_k = 0;
    for (double q : charges) {
      long double want = 0.0L;
      int k = 0;
      for (int i = 0; i < attpc::SPYRAL_SAMPLES; ++i) {
        double v = r[i] * q;
        if (v > attpc::SPYRAL_ADC_MAX) v = attpc::SPYRAL_ADC_MAX, ++k;
        want += (long double)v;
      }
      const double got = attpc::spyral_clipped_integral(sorted, tail, q);
      if (attpc::spyral_clipped_count(sorted, q) != k) {
        std::printf("response %d: q=%.17g clips %d samples, the search says %d\n", ri, q, k, attpc::spyral_clipped_count(sorted, q));
        bad = true;
      }
      const long double diff = std::fabs((long double)got - want);
      const double err = want != 0.0L ? (double)(diff / std::fabs(want)) : (got == 0.0 ? 0.0 : INFINITY);
      if (err > worst) worst = err, worst_q = q, worst_k = k;
    }
    std::printf("response %d: n=%zu worst=%.3e at q=%.17g k=%d\n", ri, charges.size(), worst, worst_q, worst_k);
    if (!(worst <= 1e-12)) bad = true;
  }
  return bad ? 1 : 0;
}
