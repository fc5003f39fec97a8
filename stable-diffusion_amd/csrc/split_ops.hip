// Producers of split-fp16 operands for the full-precision UNet mode (split16.h): each reads an fp32 GEMM output and writes the
// pair hi = fp16(v), lo = fp16(v - float(hi)).  The default mode keeps its fused epilogues (igemm EPI_HEADS / EPI_GEGLU, the
// LayerNorm post-op) and never launches these.
#include <math.h>

#include "prof.h"
#include "split16.h"

namespace sdmi {
namespace {

__device__ __forceinline__ void store_split(f16* hi, f16* lo, size_t i, float v) {
  const f16 h = (f16)v;
  hi[i] = h;
  lo[i] = (f16)(v - (float)h);
}

// kind 0 (row layout): one thread per source element, reads coalesced, writes in runs of dh
__global__ void split_heads_rows_kernel(const float* __restrict__ src, int ld, int col0, f16* __restrict__ dst, f16* __restrict__ dst_lo,
                                        int ntok, int heads, int dh, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int C = heads * dh;
  const int64_t m = i / C;
  const int c = (int)(i - m * C);
  const int b = (int)(m / ntok), tok = (int)(m - (int64_t)b * ntok);
  const int head = c / dh, dd = c - head * dh;
  store_split(dst, dst_lo, (((size_t)b * heads + head) * ntok + tok) * dh + dd, src[(size_t)m * ld + col0 + c]);
}

// kind 1 (transposed, v^T): 32 tokens x 32 channels per workgroup through LDS; pad tokens are written as zero
__global__ void __launch_bounds__(256) split_heads_t_kernel(const float* __restrict__ src, int ld, int col0, f16* __restrict__ dst,
                                                            f16* __restrict__ dst_lo, int ntok, int ntok_pad, int heads, int dh) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;        // 32 x 8
  const int tok0 = blockIdx.x * 32, c0 = blockIdx.y * 32, b = blockIdx.z;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int tok = tok0 + ty + 8 * i;
    tile[ty + 8 * i][tx] = tok < ntok ? src[((size_t)b * ntok + tok) * ld + col0 + c0 + tx] : 0.f;
  }
  __syncthreads();
  const int tok = tok0 + tx;
  if (tok >= ntok_pad) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i;
    const int head = c / dh, dd = c - head * dh;
    store_split(dst, dst_lo, (((size_t)b * heads + head) * dh + dd) * ntok_pad + tok, tile[tx][ty + 8 * i]);
  }
}

// value * gelu(gate), gelu(g) = g / 2 (1 + erf(g / sqrt 2)) (torch.nn.functional.gelu, approximate='none'), evaluated as
// g / 2 erfc(-g / sqrt 2): the same function without the cancellation of 1 + erf for negative gates
__global__ void geglu_split_kernel(const float* __restrict__ src, int F, f16* __restrict__ out, f16* __restrict__ out_lo, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t m = i / F;
  const int f = (int)(i - m * F);
  const float v = src[(size_t)m * 2 * F + f], g = src[(size_t)m * 2 * F + F + f];
  store_split(out, out_lo, (size_t)i, v * (0.5f * g * erfcf(-g * 0.70710678118654752f)));
}

// one wave per row: mean, then the centred sum of squares (two passes over the row, fp32)
__global__ void __launch_bounds__(256) layernorm_split_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, f16* __restrict__ out, f16* __restrict__ out_lo,
                                                              int M, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float* r = x + (size_t)m * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += r[c];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / (float)C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) { const float d = r[c] - mean; q += d * d; }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = 1.0f / sqrtf(q / (float)C + eps);
  for (int c = lane; c < C; c += 64) store_split(out, out_lo, (size_t)m * C + c, (r[c] - mean) * rstd * gamma[c] + beta[c]);
}

}  // namespace

int launch_split_heads(const float* src, int ld, int col0, f16* dst, f16* dst_lo, int kind, int B, int ntok, int ntok_pad, int heads,
                       int dh, hipStream_t stream) {
  const int C = heads * dh;
  SDMI_CHECK(src && dst && dst_lo && B >= 1 && ntok >= 1 && heads >= 1 && dh >= 1 && col0 >= 0 && col0 + C <= ld, "split heads: bad arguments");
  if (kind == 0) {
    const int64_t n = (int64_t)B * ntok * C;
    ProfScope ps("split_heads", 0.0, (double)n * 8.0, stream);
    SDMI_LAUNCH(split_heads_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, ld, col0, dst, dst_lo, ntok, heads, dh, n);
  } else {
    SDMI_CHECK(kind == 1 && C % 32 == 0 && ntok_pad >= ntok && B <= 65535, "split heads (transposed): needs heads * dh % 32 == 0");
    ProfScope ps("split_heads_t", 0.0, (double)B * C * ((double)ntok * 4.0 + (double)ntok_pad * 4.0), stream);
    SDMI_LAUNCH(split_heads_t_kernel, dim3((unsigned)((ntok_pad + 31) / 32), (unsigned)(C / 32), (unsigned)B), dim3(256), 0, stream, src, ld,
                col0, dst, dst_lo, ntok, ntok_pad, heads, dh);
  }
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_geglu_split(const float* src, int M, int F, f16* out, f16* out_lo, hipStream_t stream) {
  SDMI_CHECK(src && out && out_lo && M >= 1 && F >= 1, "GEGLU split: bad arguments");
  const int64_t n = (int64_t)M * F;
  ProfScope ps("geglu_split", 0.0, (double)n * 12.0, stream);
  SDMI_LAUNCH(geglu_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, F, out, out_lo, n);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_layernorm_split(const float* x, const float* gamma, const float* beta, f16* out, f16* out_lo, int M, int C, float eps,
                           hipStream_t stream) {
  SDMI_CHECK(x && gamma && beta && out && out_lo && M >= 1 && C >= 1, "LayerNorm split: bad arguments");
  ProfScope ps("layernorm_split", 0.0, (double)M * C * 8.0, stream);
  SDMI_LAUNCH(layernorm_split_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, x, gamma, beta, out, out_lo, M, C, eps);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace sdmi
