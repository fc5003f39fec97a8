// SpatialRescaler of the semantic-synthesis model (rescale.hip)
#pragma once
#include <hip/hip_runtime.h>

namespace sdmi {

// n in 0 .. 2 bilinear halvings of x fp32 NCHW [B][Cin][H][W], then the 1x1 channel map w [Cout][Cin] (+ bias), Cout <= 8
// -> out [B][Cout][H >> n][W >> n]; w null: out [B][Cin][H >> n][W >> n]
int launch_spatial_rescale(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int H, int W, int n, int Cout,
                           hipStream_t s);
// ... of one_hot(labels), labels int32 [B][H][W], bit for bit, without building it
int launch_spatial_rescale_labels(const int* labels, const float* w, const float* bias, float* out, int B, int Cin, int H, int W, int n,
                                  int Cout, hipStream_t s);

}  // namespace sdmi
