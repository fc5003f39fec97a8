// Sanitizer sweep of the feature extractor's host coefficient tables (stable-diffusion_amd/csrc/fe_coeffs.cpp), CPU only:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Istable-diffusion_amd/csrc \
//       tools/fe_coeffs_sanitize.cpp stable-diffusion_amd/csrc/fe_coeffs.cpp -o /tmp/fe_coeffs_sanitize && /tmp/fe_coeffs_sanitize [max]
//
// Every (in, out) in 1 .. max (default 1024) fills exactly-sized heap tables, so a write past either table is an AddressSanitizer report and
// an out-of-range double -> int conversion an UndefinedBehaviorSanitizer one.  The invariants the kernels rely on are checked as well.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fe_coeffs.h"

int main(int argc, char** argv) {
  const int max = argc > 1 ? atoi(argv[1]) : 1024;
  long long tables = 0, bad = 0;
  for (int in = 1; in <= max; ++in) {
    for (int out = 1; out <= max; ++out) {
      const int ks = sdmi::fe_ksize(in, out);
      std::vector<int32_t> bounds((size_t)out * 2), kk((size_t)out * ks);
      if (ks < 5 || sdmi::fe_coeffs(in, out, bounds.data(), kk.data()) != 0) { ++bad; continue; }
      int prev_min = 0, prev_end = 0;
      for (int xx = 0; xx < out; ++xx) {
        const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
        int bmin, bmax;
        sdmi::fe_bounds(in, out, xx, &bmin, &bmax);
        long long sum = 0;
        for (int x = 0; x < ks; ++x) sum += kk[(size_t)xx * ks + x];
        // inside the source, inside the table row, monotonic (the crop window's rows are one contiguous range), weights sum to one
        const bool ok = xmin >= 0 && xmax >= 1 && xmax <= ks && xmin + xmax <= in && bmin == xmin && bmax == xmax && xmin >= prev_min &&
                        xmin + xmax >= prev_end && llabs(sum - (1 << sdmi::FE_PRECISION_BITS)) <= ks;
        if (!ok) {
          if (bad < 10) fprintf(stderr, "in %d out %d xx %d: xmin %d xmax %d ksize %d sum %lld\n", in, out, xx, xmin, xmax, ks, sum);
          ++bad;
        }
        prev_min = xmin; prev_end = xmin + xmax;
      }
      ++tables;
    }
  }
  printf("fe_coeffs sweep 1..%d: %lld tables, %lld violations\n", max, tables, bad);
  return bad ? 1 : 0;
}
