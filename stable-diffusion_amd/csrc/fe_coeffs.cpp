// The coefficient tables of PIL's Image.resize(..., BICUBIC) on 8-bit images (Pillow's Resample.c: precompute_coeffs, bicubic_filter,
// normalize_coeffs_8bpc), which the safety checker's feature extractor runs on every image (scripts/txt2img.py:26-29, 88-90).
// Everything is `double` in Pillow's own evaluation order; this file is built with -ffp-contract=off, and the pragma below says the same
// to a compiler that is not given the flag, so no product is fused into a sum and the integers equal Pillow's bit for bit.
#include "fe_coeffs.h"

#include <math.h>

#include <vector>

#pragma STDC FP_CONTRACT OFF

namespace sdmi {
namespace {

constexpr double FE_BICUBIC_SUPPORT = 2.0;

double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

struct Axis {
  double scale, filterscale, support, ss;
  int ksize;
  Axis(int in, int out) {
    filterscale = scale = (double)in / out;
    if (filterscale < 1.0) filterscale = 1.0;
    support = FE_BICUBIC_SUPPORT * filterscale;
    ksize = (int)ceil(support) * 2 + 1;
    ss = 1.0 / filterscale;
  }
  double center(int xx) const { return (xx + 0.5) * scale; }
  void bounds(int in, double c, int* xmin, int* xmax) const {
    int lo = (int)(c - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(c + support + 0.5);
    if (hi > in) hi = in;
    *xmin = lo;
    *xmax = hi - lo;
  }
};

}  // namespace

int fe_ksize(int in, int out) {
  if (in < 1 || out < 1) return -1;
  return Axis(in, out).ksize;
}

void fe_bounds(int in, int out, int xx, int* xmin, int* xmax) {
  const Axis ax(in, out);
  ax.bounds(in, ax.center(xx), xmin, xmax);
}

int fe_coeffs(int in, int out, int32_t* bounds, int32_t* kk) {
  if (in < 1 || out < 1 || !bounds || !kk) return -1;
  const Axis ax(in, out);
  std::vector<double> w((size_t)ax.ksize);
  for (int xx = 0; xx < out; ++xx) {
    const double center = ax.center(xx);
    int xmin, xmax;
    ax.bounds(in, center, &xmin, &xmax);
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      w[x] = bicubic_filter((x + xmin - center + 0.5) * ax.ss);
      ww += w[x];
    }
    int32_t* k = kk + (size_t)xx * ax.ksize;
    for (int x = 0; x < xmax; ++x) {
      if (ww != 0.0) w[x] /= ww;
      k[x] = w[x] < 0 ? (int32_t)(-0.5 + w[x] * (1 << FE_PRECISION_BITS)) : (int32_t)(0.5 + w[x] * (1 << FE_PRECISION_BITS));
    }
    for (int x = xmax; x < ax.ksize; ++x) k[x] = 0;
    bounds[xx * 2 + 0] = xmin;
    bounds[xx * 2 + 1] = xmax;
  }
  return 0;
}

void fe_output_size(int H, int W, int size, int* rh, int* rw) {
  // int(size * long / short): the quotient of two exact integers, truncated -- the integer division gives the same number
  const int shortest = H < W ? H : W, longest = H < W ? W : H;
  const int other = (int)((int64_t)size * longest / shortest);
  *rh = H <= W ? size : other;
  *rw = H <= W ? other : size;
}

}  // namespace sdmi
