// The safety checker's image preprocessing (feature_extractor.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdmi {

enum FeSource { FE_U8_NHWC = 0, FE_F32_NHWC = 1, FE_F32_NCHW = 2, FE_F32_NCHW_RAW = 3 };     // SDMI_FE_SRC_* of include/sdmi.h

struct FeParams {
  const void* src = nullptr; int kind = FE_U8_NHWC;   // one batch of equal-sized images [B][H][W][3] or [B][3][H][W]
  int B = 0, H = 0, W = 0;
  int size = 0, crop = 0;                             // shortest side after the resize, side of the centre crop
  // device tables of fe_coeffs (fe_coeffs.h): W -> resized width, H -> resized height; unused (may be null) for an axis that keeps its size
  const int32_t* hb = nullptr; const int32_t* hk = nullptr; int h_ksize = 0;
  const int32_t* vb = nullptr; const int32_t* vk = nullptr; int v_ksize = 0;
  float mean[3] = {0.f, 0.f, 0.f}, std[3] = {1.f, 1.f, 1.f};
  void* ws = nullptr; int64_t ws_bytes = 0;           // the horizontal pass's uint8 rows (fe_workspace_bytes)
  float* pixel_values = nullptr;                      // [B][3][crop][crop]
  unsigned char* out_u8 = nullptr;                    // optional [B][crop][crop][3]: the resized and cropped image
};
int64_t fe_workspace_bytes(int B, int H, int W, int size, int crop);      // -1: refused (the error names why)
int launch_feature_extract(const FeParams& p, hipStream_t s);

}  // namespace sdmi
