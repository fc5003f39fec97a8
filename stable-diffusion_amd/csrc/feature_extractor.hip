// The safety checker's feature extractor (scripts/txt2img.py:26-29, 88-90: AutoFeatureExtractor -> CLIPFeatureExtractor) on the device:
// numpy_to_pil's uint8 conversion, PIL's 8-bit bicubic resize of the shortest side to `size`, the centre crop, / 255 and CLIP's mean / std.
//
// Arithmetic, bit for bit PIL's (Pillow Resample.c, ImagingResampleHorizontal_8bpc / Vertical_8bpc):
//   * image -> uint8 (float sources): rint(x * 255) in fp32, round half to even, clamped to 0 .. 255 (numpy_to_pil's
//     (x * 255).round().astype(uint8)); the raw decoder kind applies clamp((x + 1) / 2, 0, 1) first, in txt2img.py:314's fp32 op order
//   * a pass: acc = 1 << 21; acc += pixel[xmin + x] * k[x], x = 0 .. xmax - 1, in int32; out = clamp(acc >> 22, 0, 255).  The horizontal pass
//     runs first and stores uint8, the vertical pass reads that uint8.  An axis whose size does not change has no pass.
//   * (float(u8) / 255 - mean[c]) / std[c] in fp32: three correctly rounded operations, no contraction (built with -ffp-contract=off)
// The integer sums are exact (|acc| < 255 * 1.4 * 2^22 < 2^31), so their order is free.
//
// Launches: at most two.  fe_horizontal_kernel computes only the crop window's columns, and only the source rows the vertical pass of the
// crop window reads, into a uint8 workspace [B][rows][crop][3]; fe_vertical_kernel does the vertical pass, the crop and the float stage.
// An image whose shortest side already is `size` is not resized (neither axis changes): the second kernel alone crops the source, converting
// in its load, and normalises.
//   * horizontal: a lane owns an output column, so its coefficients are the same for every row: the block's 64 columns' table rows are
//     staged in LDS once (row pitch ksize is odd: the lanes' reads fall on distinct banks) and reused down 16 rows
//   * vertical: a block owns one output row, so ymin, the tap count and every coefficient are uniform: they come through scalar loads
// Table entries are clamped to the buffer they index before use, so a table that does not belong to the sizes cannot make a lane read outside
// the source or the workspace (with fe_coeffs' tables the clamps change nothing).
#include "common.h"
#include "fe_coeffs.h"
#include "feature_extractor.h"
#include "prof.h"

namespace sdmi {
namespace {

#pragma clang fp contract(off)

constexpr int FE_TW = 64;        // output columns per horizontal block (one per lane)
constexpr int FE_TR = 16;        // source rows per horizontal block (4 waves x 4 rows)
constexpr int FE_MAX_KSIZE = 255;   // FE_TW * ksize * 4 bytes of LDS <= 64 KB: a 63-fold reduction

struct FeNorm { float mean[3], std[3]; };

__device__ __forceinline__ int fe_to_u8(float x) {
  const float v = rintf(x * 255.0f);
  return (int)fminf(fmaxf(v, 0.0f), 255.0f);
}

// channel c of pixel (y, x) of image b as PIL's uint8; H, W: the buffer's rows and columns per image
template <int KIND>
__device__ __forceinline__ int fe_px(const void* __restrict__ src, int64_t b, int y, int x, int c, int H, int W) {
  if constexpr (KIND == FE_U8_NHWC) {
    return ((const unsigned char*)src)[((b * H + y) * W + x) * 3 + c];
  } else {
    const float* f = (const float*)src;
    float v = KIND == FE_F32_NHWC ? f[((b * H + y) * W + x) * 3 + c] : f[((b * 3 + c) * H + y) * W + x];
    if constexpr (KIND == FE_F32_NCHW_RAW) {
      v = (v + 1.0f) / 2.0f;                         // txt2img.py:314
      v = fminf(fmaxf(v, 0.0f), 1.0f);
    }
    return fe_to_u8(v);
  }
}

__device__ __forceinline__ int fe_clip8(int acc) { return min(max(acc >> FE_PRECISION_BITS, 0), 255); }

// tmp [B][nrows][cw][3] uint8 <- horizontal pass of source rows y0 .. y0 + nrows, resized columns left .. left + cw
template <int KIND>
__global__ void __launch_bounds__(256) fe_horizontal_kernel(const void* __restrict__ src, const int* __restrict__ hb,
                                                            const int* __restrict__ hk, int ks, unsigned char* __restrict__ tmp, int H, int W,
                                                            int left, int cw, int y0, int nrows) {
  extern __shared__ int s_fe[];                      // [2 * FE_TW] bounds, then [FE_TW][ks] coefficients
  int* s_k = s_fe + 2 * FE_TW;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int ox0 = blockIdx.x * FE_TW;
  const int ncol = min(FE_TW, cw - ox0);
  for (int i = threadIdx.x; i < 2 * ncol; i += 256) s_fe[i] = hb[(size_t)(left + ox0) * 2 + i];
  for (int i = threadIdx.x; i < ncol * ks; i += 256) s_k[i] = hk[(size_t)(left + ox0) * ks + i];
  __syncthreads();
  if (tx >= ncol) return;
  const int xmin = min(max(s_fe[2 * tx], 0), W - 1);
  const int n = min(s_fe[2 * tx + 1], min(ks, W - xmin));
  const int* k = s_k + tx * ks;
  const int64_t b = blockIdx.z;
  const int r_end = min(nrows, ((int)blockIdx.y + 1) * FE_TR);
  for (int r = blockIdx.y * FE_TR + ty; r < r_end; r += 4) {
    const int y = y0 + r;
    int a0 = 1 << (FE_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int x = 0; x < n; ++x) {
      const int kx = k[x];
      a0 += fe_px<KIND>(src, b, y, xmin + x, 0, H, W) * kx;
      a1 += fe_px<KIND>(src, b, y, xmin + x, 1, H, W) * kx;
      a2 += fe_px<KIND>(src, b, y, xmin + x, 2, H, W) * kx;
    }
    unsigned char* o = tmp + ((b * nrows + r) * cw + ox0 + tx) * 3;
    o[0] = (unsigned char)fe_clip8(a0);
    o[1] = (unsigned char)fe_clip8(a1);
    o[2] = (unsigned char)fe_clip8(a2);
  }
}

// pixel_values [B][3][crop][crop] (and out_u8 [B][crop][crop][3]) <- vertical pass of `in` for resized rows top .. top + crop, columns
// in_x0 .. in_x0 + crop of the buffer.  `in`: inH rows x inW columns per image, its row 0 = row in_y0 of the horizontally resized image.
// vk null: no vertical pass (the resized row IS the buffer row).
template <int KIND>
__global__ void __launch_bounds__(256) fe_vertical_kernel(const void* __restrict__ in, int inH, int inW, int in_y0, int in_x0,
                                                          const int* __restrict__ vb, const int* __restrict__ vk, int ks, int top, int crop,
                                                          FeNorm nm, float* __restrict__ pv, unsigned char* __restrict__ out_u8) {
  const int ox = blockIdx.x * 256 + threadIdx.x;
  const int oy = blockIdx.y;                         // uniform: the table reads below are scalar loads
  const int64_t b = blockIdx.z;
  if (ox >= crop) return;
  int u[3];
  if (vk) {
    const int ymin = min(max(vb[2 * (top + oy)], in_y0), in_y0 + inH - 1);
    const int n = min(vb[2 * (top + oy) + 1], min(ks, in_y0 + inH - ymin));
    const int* k = vk + (size_t)(top + oy) * ks;
    int a0 = 1 << (FE_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < n; ++t) {
      const int kt = k[t];
      a0 += fe_px<KIND>(in, b, ymin - in_y0 + t, in_x0 + ox, 0, inH, inW) * kt;
      a1 += fe_px<KIND>(in, b, ymin - in_y0 + t, in_x0 + ox, 1, inH, inW) * kt;
      a2 += fe_px<KIND>(in, b, ymin - in_y0 + t, in_x0 + ox, 2, inH, inW) * kt;
    }
    u[0] = fe_clip8(a0); u[1] = fe_clip8(a1); u[2] = fe_clip8(a2);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = fe_px<KIND>(in, b, top + oy - in_y0, in_x0 + ox, c, inH, inW);
  }
  const int64_t pix = (int64_t)oy * crop + ox, plane = (int64_t)crop * crop;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float f = (float)u[c] / 255.0f;
    pv[(b * 3 + c) * plane + pix] = (f - nm.mean[c]) / nm.std[c];
  }
  if (out_u8) {
    unsigned char* o = out_u8 + (b * plane + pix) * 3;
    o[0] = (unsigned char)u[0]; o[1] = (unsigned char)u[1]; o[2] = (unsigned char)u[2];
  }
}

// what the launcher derives from the sizes; every refusal names what it refuses
struct FeGeom {
  int rh, rw, top, left;       // resized size, crop origin
  bool resized;
  int y0, nrows;               // rows of the horizontally resized image the vertical pass of the crop window reads
};

int fe_geometry(int B, int H, int W, int size, int crop, FeGeom* g) {
  SDMI_CHECK(B >= 1 && H >= 1 && W >= 1 && size >= 1 && crop >= 1,
             "feature_extract: sizes below 1 (B, H, W, size and crop_size must all be at least 1)");
  SDMI_CHECK(crop <= size, "feature_extract: crop_size > size is not built (the processor would pad the image)");
  SDMI_CHECK((int64_t)size * std::max(H, W) / std::min(H, W) <= (1 << 20) && H <= (1 << 20) && W <= (1 << 20),
             "feature_extract: image sides up to 2^20");
  fe_output_size(H, W, size, &g->rh, &g->rw);
  g->top = (g->rh - crop) / 2;
  g->left = (g->rw - crop) / 2;
  // the shortest side goes to `size` and the other follows it: both axes change, or (size == the shortest side) neither does
  g->resized = g->rw != W || g->rh != H;
  if (g->resized) {
    SDMI_CHECK(g->rw != W && g->rh != H, "feature_extract: one axis alone changes size");
    int lo, n, hi_min, hi_n;
    fe_bounds(H, g->rh, g->top, &lo, &n);
    fe_bounds(H, g->rh, g->top + crop - 1, &hi_min, &hi_n);
    g->y0 = lo;
    g->nrows = hi_min + hi_n - lo;
  } else {
    g->y0 = g->top;
    g->nrows = crop;
  }
  return 0;
}

}  // namespace

int64_t fe_workspace_bytes(int B, int H, int W, int size, int crop) {
  FeGeom g;
  if (fe_geometry(B, H, W, size, crop, &g)) return -1;
  return g.resized ? (int64_t)B * g.nrows * crop * 3 : 0;
}

#define FE_DISPATCH(KERNEL, KIND_, ...)                                                       \
  do {                                                                                        \
    if ((KIND_) == FE_U8_NHWC) SDMI_LAUNCH((KERNEL<FE_U8_NHWC>), __VA_ARGS__);                \
    else if ((KIND_) == FE_F32_NHWC) SDMI_LAUNCH((KERNEL<FE_F32_NHWC>), __VA_ARGS__);         \
    else if ((KIND_) == FE_F32_NCHW) SDMI_LAUNCH((KERNEL<FE_F32_NCHW>), __VA_ARGS__);         \
    else SDMI_LAUNCH((KERNEL<FE_F32_NCHW_RAW>), __VA_ARGS__);                                 \
  } while (0)

int launch_feature_extract(const FeParams& p, hipStream_t s) {
  FeGeom g;
  if (int r = fe_geometry(p.B, p.H, p.W, p.size, p.crop, &g)) return r;
  SDMI_CHECK(p.kind >= FE_U8_NHWC && p.kind <= FE_F32_NCHW_RAW, "feature_extract: unknown source kind (SDMI_FE_SRC_*)");
  SDMI_CHECK(p.src && p.pixel_values, "feature_extract: null source or pixel_values");
  SDMI_CHECK(p.B <= 65535, "feature_extract: at most 65535 images per call");
  if (g.resized) {
    SDMI_CHECK(p.hb && p.hk && p.vb && p.vk, "feature_extract: the image is resized, the horizontal and vertical tables are needed");
    SDMI_CHECK(p.h_ksize == fe_ksize(p.W, g.rw), "feature_extract: the horizontal tables' ksize does not match W -> resized width (" +
                                                     std::to_string(p.h_ksize) + " given, " + std::to_string(fe_ksize(p.W, g.rw)) + " expected)");
    SDMI_CHECK(p.v_ksize == fe_ksize(p.H, g.rh), "feature_extract: the vertical tables' ksize does not match H -> resized height (" +
                                                     std::to_string(p.v_ksize) + " given, " + std::to_string(fe_ksize(p.H, g.rh)) + " expected)");
    SDMI_CHECK(p.h_ksize <= FE_MAX_KSIZE, "feature_extract: horizontal ksize above 255 (a reduction of more than 63x)");
    SDMI_CHECK(p.ws && p.ws_bytes >= (int64_t)p.B * g.nrows * p.crop * 3, "feature_extract: workspace too small (sdmi_fe_workspace_bytes)");
  }
  const double src_bytes = (double)p.B * p.H * p.W * 3.0 * (p.kind == FE_U8_NHWC ? 1.0 : 4.0);
  ProfScope ps("feature_extract", 0.0, src_bytes + (double)p.B * p.crop * p.crop * 12.0, s);
  FeNorm nm;
  for (int c = 0; c < 3; ++c) { nm.mean[c] = p.mean[c]; nm.std[c] = p.std[c]; }
  const dim3 vgrid((unsigned)cdiv(p.crop, 256), (unsigned)p.crop, (unsigned)p.B);
  SDMI_CHECK(p.crop <= 65535 && cdiv(g.nrows, FE_TR) <= 65535, "feature_extract: crop window too tall for one launch");
  if (g.resized) {
    unsigned char* tmp = (unsigned char*)p.ws;
    const dim3 hgrid((unsigned)cdiv(p.crop, FE_TW), (unsigned)cdiv(g.nrows, FE_TR), (unsigned)p.B);
    const size_t lds = (size_t)(2 * FE_TW + FE_TW * p.h_ksize) * sizeof(int);
    FE_DISPATCH(fe_horizontal_kernel, p.kind, hgrid, dim3(256), lds, s, p.src, p.hb, p.hk, p.h_ksize, tmp, p.H, p.W, g.left, p.crop, g.y0,
                g.nrows);
    SDMI_HIP_OK(hipGetLastError());
    SDMI_LAUNCH((fe_vertical_kernel<FE_U8_NHWC>), vgrid, dim3(256), 0, s, (const void*)tmp, g.nrows, p.crop, g.y0, 0, p.vb, p.vk, p.v_ksize, g.top,
                p.crop, nm, p.pixel_values, p.out_u8);
  } else {           // nothing to resize: crop and normalise the source itself
    FE_DISPATCH(fe_vertical_kernel, p.kind, vgrid, dim3(256), 0, s, p.src, p.H, p.W, 0, g.left, (const int*)nullptr, (const int*)nullptr, 0,
                g.top, p.crop, nm, p.pixel_values, p.out_u8);
  }
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace sdmi
