// The pooled, projected head of OpenAI CLIP's encode_text (clip/model.py: x[arange(B), text.argmax(-1)] @ text_projection) behind the text
// tower of clip.cpp, as FrozenCLIPTextEmbedder uses it (ldm/modules/encoders/modules.py:165-194): two launches after the tower.
//   clip_pool_project_kernel: workgroup (sample, 32 outputs).  pos = the FIRST maximum of ids[b, :] (no fixed eos id); the row hidden[b, pos, :] of the
//   final-LayerNorm output goes to LDS as the GEMM operand of the handle's precision -- mixed: rounded to fp16 once, as the tower's GEMMs
//   round their operands; full: the split-fp16 pair hi = fp16(x), lo = fp16(x - hi) -- and meets the rows of text_projection.weight [E][W]
//   (fp16 rows, or the split-fp16 rows [hi | hi | lo]) with fp32 accumulation: mixed a * w; full a_hi w_hi + a_lo w_hi + a_hi w_lo, the
//   three products of every split-fp16 GEMM.  clip_l2norm_kernel (normalize): z / ||z||_2 in place, one workgroup per sample.
// No atomics; every sum has one fixed order (lane partials over ascending columns, then the lane masks 32 .. 1, then the waves in order).
#include <limits.h>
#include <math.h>

#include "common.h"
#include "prof.h"

namespace sdmi {
namespace {

constexpr int TP_MAXW = 2560, TP_MAXE = 4096, TP_MAXL = 1024;
constexpr int TP_EB = 32;             // outputs per workgroup

__device__ __forceinline__ float tp_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

template <bool FULL>
__global__ void __launch_bounds__(256) clip_pool_project_kernel(const int64_t* __restrict__ ids, const float* __restrict__ hidden,
                                                                const f16* __restrict__ w, float* __restrict__ out, int L, int W, int E) {
  __shared__ float s_hi[TP_MAXW];
  __shared__ float s_lo[FULL ? TP_MAXW : 1];
  __shared__ long long s_best[256];
  __shared__ int s_bpos[256];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the first maximum of ids[b, :]
  long long best = LLONG_MIN;
  int bpos = 0x7fffffff;
  for (int t = tid; t < L; t += 256) {
    const long long v = ids[(int64_t)b * L + t];
    if (v > best) { best = v; bpos = t; }          // (ascending t: the first maximum of this thread's positions)
  }
  s_best[tid] = best; s_bpos[tid] = bpos;
  __syncthreads();
  for (int n = 128; n >= 1; n >>= 1) {
    if (tid < n) {
      const long long ov = s_best[tid + n];
      const int op = s_bpos[tid + n];
      if (ov > s_best[tid] || (ov == s_best[tid] && op < s_bpos[tid])) { s_best[tid] = ov; s_bpos[tid] = op; }
    }
    __syncthreads();
  }
  const int pos = s_bpos[0];
  const float* h = hidden + ((int64_t)b * L + pos) * W;
  for (int c = tid; c < W; c += 256) {
    const float x = h[c];
    const f16 hi = (f16)x;
    s_hi[c] = (float)hi;
    if (FULL) s_lo[c] = (float)(f16)(x - (float)hi);
  }
  __syncthreads();

  const int ldw = FULL ? 3 * W : W;
  const int e_lo = blockIdx.y * TP_EB, e_hi = e_lo + TP_EB < E ? e_lo + TP_EB : E;
  for (int e = e_lo + wave; e < e_hi; e += 4) {
    const f16* wr = w + (int64_t)e * ldw;
    float acc = 0.f;
    for (int c = lane * 8; c < W; c += 512) {       // W % 8 == 0: one 16-byte load per operand
      const f16x8 wh = *(const f16x8*)(wr + c);
      if (FULL) {
        const f16x8 wl = *(const f16x8*)(wr + 2 * W + c);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          acc = fmaf(s_hi[c + i], (float)wh[i], acc);
          acc = fmaf(s_lo[c + i], (float)wh[i], acc);
          acc = fmaf(s_hi[c + i], (float)wl[i], acc);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = fmaf(s_hi[c + i], (float)wh[i], acc);
      }
    }
    acc = tp_wave_sum(acc);
    if (lane == 0) out[(int64_t)b * E + e] = acc;
  }
}

// out[b][:] /= ||out[b][:]||_2, one workgroup per sample
__global__ void __launch_bounds__(256) clip_l2norm_kernel(float* __restrict__ out, int E) {
  __shared__ float s_part[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* z = out + (int64_t)blockIdx.x * E;
  float ss = 0.f;
  for (int e = tid; e < E; e += 256) ss = fmaf(z[e], z[e], ss);
  ss = tp_wave_sum(ss);
  if (lane == 0) s_part[wave] = ss;
  __syncthreads();
  const float inv = 1.0f / sqrtf(((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]);
  for (int e = tid; e < E; e += 256) z[e] = z[e] * inv;
}

}  // namespace

int launch_clip_pool_project(const int64_t* ids, const float* hidden, const f16* w, bool full, float* out, int B, int L, int W, int E,
                             int normalize, hipStream_t s) {
  SDMI_CHECK(ids && hidden && w && out, "clip_pool_project: null operand");
  SDMI_CHECK(B >= 1 && B <= 65535 && L >= 1 && L <= TP_MAXL, "clip_pool_project: 1 <= B <= 65535, 1 <= L <= 1024");
  SDMI_CHECK(W >= 8 && W % 8 == 0 && W <= TP_MAXW && E >= 1 && E <= TP_MAXE, "clip_pool_project: W % 8 == 0, W <= 2560, E <= 4096");
  SDMI_CHECK(((uintptr_t)w & 15) == 0, "clip_pool_project: the projection weight must be 16-byte aligned");
  ProfScope ps("clip_pool_project", 2.0 * B * W * E * (full ? 3 : 1), (double)E * W * (full ? 6.0 : 2.0), s);
  const dim3 grid(B, (E + TP_EB - 1) / TP_EB);
  if (full) SDMI_LAUNCH(clip_pool_project_kernel<true>, grid, dim3(256), 0, s, ids, hidden, w, out, L, W, E);
  else SDMI_LAUNCH(clip_pool_project_kernel<false>, grid, dim3(256), 0, s, ids, hidden, w, out, L, W, E);
  if (normalize) SDMI_LAUNCH(clip_l2norm_kernel, dim3(B), dim3(256), 0, s, out, E);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace sdmi
