// Kernels of the latent-inpainting model (models/ldm/inpainting_big/config.yaml):
//   * resample2_kernel: 2x2 average pool / nearest x2 of an fp32 NHWC activation -- the h_upd / x_upd of a ResBlock with
//     resblock_updown (openaimodel.py:208-216,253-259: Downsample / Upsample with use_conv=False, i.e. F.avg_pool2d(x, 2) /
//     F.interpolate(x, scale_factor=2, mode="nearest")), writing fp32 and / or the fp16 (hi | lo) operand of the next conv
//   * the codebook quantizer of VQModelInterface.decode (autoencoder.py:274-283, taming's VectorQuantizer2 in its legacy
//     form): nearest code by d = sum(z^2) + sum(e^2) - 2 z.e, first index on ties, z_q = z + (e[idx] - z) in fp32.
#include "prof.h"
#include "split16.h"

namespace sdmi {
namespace {

// (the reference evaluates these expressions one rounded op at a time, in fp32: no contraction into FMAs)
#pragma clang fp contract(off)

__device__ __forceinline__ void put4(float* o32, f16* hi, f16* lo, size_t i, float4 v) {
  if (o32) *(float4*)(o32 + i) = v;
  if (hi) {
    const float a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f16 h = (f16)a[j];
      hi[i + j] = h;
      if (lo) lo[i + j] = (f16)(a[j] - (float)h);
    }
  }
}

// one thread per (output pixel, 4 channels); dir > 0: 2x2 average (H, W even), dir < 0: nearest x2
__global__ void __launch_bounds__(256) resample2_kernel(const float* __restrict__ x, float* __restrict__ o32, f16* __restrict__ hi,
                                                        f16* __restrict__ lo, int H, int W, int C, int Ho, int Wo, int dir, int64_t n4) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const int C4 = C >> 2;
  const int c = (int)(i % C4) * 4;
  const int64_t m = i / C4;                        // output pixel (b, yo, xo)
  const int xo = (int)(m % Wo);
  const int64_t r = m / Wo;
  const int yo = (int)(r % Ho);
  const int64_t b = r / Ho;
  float4 v;
  if (dir > 0) {
    const float* p = x + (((size_t)b * H + 2 * yo) * W + 2 * xo) * C + c;
    const float4 a = *(const float4*)p, bb = *(const float4*)(p + C);
    const float4 cc = *(const float4*)(p + (size_t)W * C), d = *(const float4*)(p + (size_t)W * C + C);
    // F.avg_pool2d: the four taps summed row by row, then divided by the window size
    v.x = (((a.x + bb.x) + cc.x) + d.x) / 4.0f;
    v.y = (((a.y + bb.y) + cc.y) + d.y) / 4.0f;
    v.z = (((a.z + bb.z) + cc.z) + d.z) / 4.0f;
    v.w = (((a.w + bb.w) + cc.w) + d.w) / 4.0f;
  } else {
    v = *(const float4*)(x + (((size_t)b * H + (yo >> 1)) * W + (xo >> 1)) * C + c);
  }
  put4(o32, hi, lo, (size_t)m * C + c, v);
}

__global__ void __launch_bounds__(256) vq_norms_kernel(const float* __restrict__ e, float* __restrict__ se, int n, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int c = 0; c < D; ++c) { const float v = e[(size_t)i * D + c]; s = s + v * v; }
  se[i] = s;
}

// 64 latent pixels per workgroup (lane = pixel), four waves; the codebook streams through LDS in tiles of VQ_TILE codes and
// wave w scans the w-th quarter of every tile.  Each wave keeps the first minimum of its codes; the four are merged by
// (distance, index), so the result is the first minimum over the whole table whatever the split.
constexpr int VQ_TILE = 512, VQ_MAXD = 8;

template <int D>
__global__ void __launch_bounds__(256) vq_quantize_kernel(const float* __restrict__ z, float z_scale, const float* __restrict__ e,
                                                          const float* __restrict__ se, int n_embed, float* __restrict__ zq,
                                                          int* __restrict__ idx_out, int HW, int64_t npix) {
  __shared__ float s_e[VQ_TILE * D];
  __shared__ float s_n[VQ_TILE];
  __shared__ float s_best[4][64];
  __shared__ int s_idx[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = (int64_t)blockIdx.x * 64 + lane;
  const bool live = p < npix;
  const int64_t b = live ? p / HW : 0;
  const int hw = live ? (int)(p - b * HW) : 0;
  float zv[D];
  float sz = 0.f;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    zv[c] = live ? z[((size_t)b * D + c) * HW + hw] * z_scale : 0.f;
    sz = sz + zv[c] * zv[c];
  }
  float best = INFINITY;
  int bi = 0x7fffffff;
  constexpr int Q = VQ_TILE / 4;
  for (int n0 = 0; n0 < n_embed; n0 += VQ_TILE) {
    const int nt = min(VQ_TILE, n_embed - n0);
    __syncthreads();
    for (int i = threadIdx.x; i < nt * D; i += 256) s_e[i] = e[(size_t)n0 * D + i];
    for (int i = threadIdx.x; i < nt; i += 256) s_n[i] = se[n0 + i];
    __syncthreads();
    const int j1 = min(nt, (wave + 1) * Q);
    for (int j = wave * Q; j < j1; ++j) {
      float dot = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) dot = dot + zv[c] * s_e[j * D + c];
      const float d = (sz + s_n[j]) - 2.0f * dot;
      if (d < best) { best = d; bi = n0 + j; }
    }
  }
  s_best[wave][lane] = best;
  s_idx[wave][lane] = bi;
  __syncthreads();
  if (wave != 0 || !live) return;
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const float d = s_best[w][lane];
    const int k = s_idx[w][lane];
    if (d < best || (d == best && k < bi)) { best = d; bi = k; }
  }
  if (bi >= n_embed) bi = 0;        // (every distance NaN: torch.argmin would not pick a valid row either; keep the store in bounds)
  if (idx_out) idx_out[p] = bi;
  if (zq) {
#pragma unroll
    for (int c = 0; c < D; ++c) zq[((size_t)b * D + c) * HW + hw] = zv[c] + (e[(size_t)bi * D + c] - zv[c]);
  }
}

template <int D>
int launch_vq_d(const float* z, float z_scale, const float* e, const float* se, int n_embed, float* zq, int* idx, int B, int HW,
                hipStream_t s) {
  const int64_t npix = (int64_t)B * HW;
  SDMI_LAUNCH(vq_quantize_kernel<D>, dim3((unsigned)((npix + 63) / 64)), dim3(256), 0, s, z, z_scale, e, se, n_embed, zq, idx, HW, npix);
  return 0;
}

}  // namespace

int launch_resample2(const float* x, float* o32, f16* hi, f16* lo, int B, int H, int W, int C, int dir, hipStream_t s) {
  SDMI_CHECK(x && (o32 || hi) && (!lo || hi) && B >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && (dir == 1 || dir == -1),
             "resample2: bad arguments");
  SDMI_CHECK(dir < 0 || (H % 2 == 0 && W % 2 == 0), "resample2: the 2x2 average pool needs even H and W");
  SDMI_CHECK((((uintptr_t)x | (uintptr_t)o32) & 15) == 0, "resample2: fp32 buffers must be 16-byte aligned");
  const int Ho = dir > 0 ? H / 2 : 2 * H, Wo = dir > 0 ? W / 2 : 2 * W;
  const int64_t n4 = (int64_t)B * Ho * Wo * (C / 4);
  ProfScope ps(dir > 0 ? "avgpool2" : "nearest2", 0.0, (double)B * (H * W + Ho * Wo) * C * 4.0, s);
  SDMI_LAUNCH(resample2_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, x, o32, hi, lo, H, W, C, Ho, Wo, dir, n4);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_vq_norms(const float* e, float* se, int n_embed, int D, hipStream_t s) {
  SDMI_CHECK(e && se && n_embed >= 1 && D >= 1 && D <= VQ_MAXD, "codebook norms: bad arguments");
  SDMI_LAUNCH(vq_norms_kernel, dim3((unsigned)((n_embed + 255) / 256)), dim3(256), 0, s, e, se, n_embed, D);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_vq_quantize(const float* z, float z_scale, const float* e, const float* se, int n_embed, int D, float* zq, int* idx, int B,
                       int HW, hipStream_t s) {
  SDMI_CHECK(z && e && se && (zq || idx) && n_embed >= 1 && B >= 1 && HW >= 1, "quantize: bad arguments");
  ProfScope ps("vq_quantize", 6.0 * B * (double)HW * n_embed * D, (double)B * HW * D * 8.0 + (double)n_embed * (D + 1) * 4.0, s);
  int r;
  switch (D) {
    case 1: r = launch_vq_d<1>(z, z_scale, e, se, n_embed, zq, idx, B, HW, s); break;
    case 2: r = launch_vq_d<2>(z, z_scale, e, se, n_embed, zq, idx, B, HW, s); break;
    case 3: r = launch_vq_d<3>(z, z_scale, e, se, n_embed, zq, idx, B, HW, s); break;
    case 4: r = launch_vq_d<4>(z, z_scale, e, se, n_embed, zq, idx, B, HW, s); break;
    case 8: r = launch_vq_d<8>(z, z_scale, e, se, n_embed, zq, idx, B, HW, s); break;
    default: return fail("quantize: embed_dim " + std::to_string(D) + " not instantiated (1, 2, 3, 4, 8)");
  }
  if (r) return r;
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace sdmi
