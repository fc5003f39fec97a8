// Pillow's 8-bit bicubic resampling tables, on the host (fe_coeffs.cpp).  No HIP: this header and its translation unit compile with any
// C++ compiler, so the table code can be run under the host sanitizers on its own.
#pragma once
#include <stdint.h>

namespace sdmi {

constexpr int FE_PRECISION_BITS = 32 - 8 - 2;      // fraction bits of the fixed-point coefficients (Pillow's PRECISION_BITS)

// taps per output index of the axis in -> out (in, out >= 1)
int fe_ksize(int in, int out);
// first source index and tap count of output index xx (0 <= xx < out): reads stay inside [xmin, xmin + xmax), a subset of [0, in)
void fe_bounds(int in, int out, int xx, int* xmin, int* xmax);
// bounds [out][2] = {xmin, xmax}, kk [out][fe_ksize(in, out)] fixed-point coefficients (entries x >= xmax are 0).  0 ok, -1 bad sizes / null
int fe_coeffs(int in, int out, int32_t* bounds, int32_t* kk);
// CLIPFeatureExtractor.resize with an int size: the shortest side becomes `size`, the other int(size * long / short)
void fe_output_size(int H, int W, int size, int* rh, int* rw);

}  // namespace sdmi
