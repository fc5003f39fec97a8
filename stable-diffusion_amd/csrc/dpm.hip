// The rest of DPM-Solver (ldm/models/diffusion/dpm_solver/dpm_solver.py) beyond the one fused 2M step of sampler.hip: the model value
// with either prediction type and dynamic thresholding, every singlestep / multistep update form as one launch, the thresholding
// scale as a selection (no sort), and the adaptive solver's error norm.  fp32; this file is compiled with -ffp-contract=off and every
// product, sum and quotient below rounds on its own in the reference's order, so an elementwise result equals the reference's torch
// expression bit for bit.  Scalars (sigma_t / sigma_s, alpha_t * phi_1, r2 / r1 * ..., 1 / r0, ...) come from the host, which evaluates
// them with the reference's own torch ops (samplers.py); a subtraction of c * v arrives as the addition of (-c) * v, which is exact.
#include "common.h"
#include "prof.h"
#include "step_math.h"
#include <math.h>

#pragma clang fp contract(off)

namespace sdmi {
namespace {

// Model value (dpm_solver.py:340-346, :386-408): e = classifier-free combine of the raw model output;
//   predict_x0 == 0: out = e                                       noise_prediction_fn
//   predict_x0 != 0: x0 = (x - sigma_s * e) / alpha_s              data_prediction_fn (:393)
//   with s != NULL:  x0 = clamp(x0, -s[b], s[b]) / s[b]            dynamic thresholding (:397-398); s is per sample, on the device
__global__ void __launch_bounds__(256) dpm_model_value_kernel(DpmModelValueParams p) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const float e = p.cfg ? cfg_combine(p.eps_model[i], p.eps_model[p.n + i], p.scale) : p.eps_model[i];
  if (!p.predict_x0) { p.out[i] = e; return; }
  float x0 = dpm_data_prediction(p.x[i], e, p.sigma_s, p.alpha_s);
  if (p.s) {
    const float sv = p.s[i / p.row];
    const float lo = -sv;
    x0 = x0 < lo ? lo : x0;                          // torch.clamp(x0, -s, s): a NaN x0 stays NaN (both compares are false)
    x0 = x0 > sv ? sv : x0;
    x0 = x0 / sv;                                    // (a NaN s gives NaN here, as the reference's division does)
  }
  p.out[i] = x0;
}

// One launch per update of the reference.  x: the state at time s; m0, m1, m2: model values; c[]: host scalars.
//   form 0  LIN    out = c0 x + c1 m0
//                  dpm_solver_first_update (:530-533, :542-545); x_s1 of the singlestep second / third update (:588-591, :611-614, :682-685, :721-724)
//   form 1  DIFF   out = (c0 x + c1 m0) + c2 (c3 (m1 - m2))
//                  singlestep second update, both solver types (:594-604, :617-627): m1 = model_s1, m2 = m0 = model_s, c3 = 1
//                  x_s2 of the singlestep third update (:687-691, :726-730): the same, c2 = +-(r2 / r1 * ...)
//                  singlestep third update, 'dpm_solver' (:694-698, :733-737): m1 = model_s2, m2 = m0 = model_s, c3 = 1
//                  multistep second update, both solver types (:783-809): m1 = m0 = model_prev_0, m2 = model_prev_1, c3 = 1 / r0 (D1_0)
//                  (1.0f * v is v exactly, so the forms without an inner scalar pass c3 = 1)
//   form 2  SS3T   singlestep third update, 'taylor' (:700-709, :739-748): m0, m1, m2 = model_s, model_s1, model_s2
//                  D1_0 = c4 (m1 - m0); D1_1 = c5 (m2 - m0); D1 = (c6 D1_0 - c7 D1_1) / c8; D2 = (2 (D1_1 - D1_0)) / c8
//                  out = ((c0 x + c1 m0) + c2 D1) + c3 D2          c4 = 1 / r1, c5 = 1 / r2, c6 = r2, c7 = r1, c8 = r2 - r1
//   form 3  MS3    multistep third update (:835-856): m0, m1, m2 = model_prev_0, _1, _2
//                  D1_0 = c4 (m0 - m1); D1_1 = c5 (m1 - m2); dd = D1_0 - D1_1; D1 = D1_0 + c6 dd; D2 = c7 dd
//                  out = ((c0 x + c1 m0) + c2 D1) + c3 D2          c4 = 1 / r0, c5 = 1 / r1, c6 = r0 / (r0 + r1), c7 = 1 / (r0 + r1)
__global__ void __launch_bounds__(256) dpm_update_kernel(DpmUpdateParams p) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const float m1 = p.form != 0 ? p.m1[i] : 0.f;
  const float m2 = p.form != 0 ? p.m2[i] : 0.f;
  p.out[i] = dpm_update_of(p.form, p.c, p.x[i], p.m0[i], m1, m2);
}

// Dynamic-thresholding scale (:395-397): s[b] = max(quantile_0.995(|x0[b]|), max_val).  The two order statistics k_lo <= k_hi the
// quantile interpolates between are found by a radix select on the bit pattern of |x0| (for non-negative floats the unsigned order of
// the bits is the order of the values): four passes of 8 bits, each an LDS histogram of the elements that still match the prefix,
// then one pass for the next larger value.  One workgroup per sample; integer LDS atomics only, so the result depends on neither the
// launch geometry nor the run.  The row is never sorted and nothing returns to the host.  A NaN in the row gives a NaN s (torch.quantile).
constexpr int kSelThreads = 1024;
__global__ void __launch_bounds__(kSelThreads) dpm_threshold_scale_kernel(const float* x0, int64_t row, unsigned k_lo, unsigned k_hi,
                                                                          float w, float max_val, float* s_out, float* stats_out) {
#pragma clang fp contract(off)
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_k, sh_nan, sh_count_le, sh_min_above;
  const unsigned* r = reinterpret_cast<const unsigned*>(x0) + (int64_t)blockIdx.x * row;
  const int tid = threadIdx.x;
  if (tid == 0) { sh_prefix = 0u; sh_k = k_lo; sh_nan = 0u; sh_count_le = 0u; sh_min_above = 0xffffffffu; }
  unsigned mask = 0u;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    const unsigned prefix = sh_prefix;
    for (int64_t i = tid; i < row; i += kSelThreads) {
      const unsigned bits = r[i] & 0x7fffffffu;
      if (shift == 24 && bits > 0x7f800000u) atomicOr(&sh_nan, 1u);
      if ((bits & mask) == prefix) atomicAdd(&hist[(bits >> shift) & 0xffu], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned k = sh_k, acc = 0u;
      int bin = 255;
      for (int b = 0; b < 256; ++b) {
        const unsigned h = hist[b];
        if (k < acc + h) { bin = b; break; }
        acc += h;
      }
      sh_k = k - acc;
      sh_prefix = prefix | ((unsigned)bin << shift);
    }
    mask |= 0xffu << shift;
    __syncthreads();
  }
  const unsigned v_lo = sh_prefix;
  unsigned cnt = 0u, mn = 0xffffffffu;
  for (int64_t i = tid; i < row; i += kSelThreads) {
    const unsigned bits = r[i] & 0x7fffffffu;
    if (bits <= v_lo) ++cnt;
    else mn = bits < mn ? bits : mn;
  }
  atomicAdd(&sh_count_le, cnt);
  atomicMin(&sh_min_above, mn);
  __syncthreads();
  if (tid == 0) {
    const unsigned v_hi = (k_hi < sh_count_le) ? v_lo : sh_min_above;     // (k_hi <= row - 1, so a value above exists when it is needed)
    const float lo = __uint_as_float(v_lo), hi = __uint_as_float(v_hi);
    // torch.quantile's lerp (ATen lerp: the small-weight form below 0.5, else from the upper end)
    const float diff = hi - lo;
    float q;
    if (w < 0.5f) { const float t = w * diff; q = lo + t; }
    else { const float om = 1.f - w; const float t = diff * om; q = hi - t; }
    float s = q > max_val ? q : max_val;             // torch.maximum(s, max_val)
    if (sh_nan) { s = __uint_as_float(0x7fc00000u); }
    s_out[blockIdx.x] = s;
    if (stats_out) { stats_out[2 * blockIdx.x] = lo; stats_out[2 * blockIdx.x + 1] = hi; }
  }
}

// Adaptive error (:952-954): E = max_b sqrt(mean(((x_higher - x_lower) / max(atol, rtol max(|x_lower|, |x_prev|)))^2)).
// Summation tree, a function of the row length n alone: a row is cut into chunks of 1024; in a chunk thread t adds its elements
// t, t + 256, t + 512, t + 768 in that order, the 256 thread sums are added pairwise (8 levels); the finish adds the chunk sums of a
// row -- thread t takes chunks t, t + 256, ... in order -- and the 256 thread sums pairwise again.  No atomics.
constexpr int kErrChunk = 1024;
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

__device__ __forceinline__ float block_tree_sum(float v, float* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sh[tid] = sh[tid] + sh[tid + s];
    __syncthreads();
  }
  const float r = sh[0];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(256) dpm_error_partial_kernel(const float* xh, const float* xl, const float* xp, float atol, float rtol,
                                                                int64_t row, int nchunk, float* part) {
#pragma clang fp contract(off)
  __shared__ float sh[256];
  const int b = blockIdx.y, c = blockIdx.x;
  const int64_t base = (int64_t)b * row;
  float acc = 0.f;
  for (int j = 0; j < kErrChunk / 256; ++j) {
    const int64_t k = (int64_t)c * kErrChunk + j * 256 + threadIdx.x;
    if (k < row) {
      const float l = xl[base + k];
      const float m = nan_max(fabsf(l), fabsf(xp[base + k]));
      const float rm = rtol * m;
      const float delta = nan_max(atol, rm);
      const float d = xh[base + k] - l;
      const float v = d / delta;
      const float sq = v * v;
      acc = acc + sq;
    }
  }
  const float s = block_tree_sum(acc, sh);
  if (threadIdx.x == 0) part[(int64_t)b * nchunk + c] = s;
}

__global__ void __launch_bounds__(256) dpm_error_finish_kernel(const float* part, int nchunk, int B, float nf, float* E) {
#pragma clang fp contract(off)
  __shared__ float sh[256];
  float emax = 0.f;
  for (int b = 0; b < B; ++b) {
    float acc = 0.f;
    for (int c = threadIdx.x; c < nchunk; c += 256) acc = acc + part[(int64_t)b * nchunk + c];
    const float s = block_tree_sum(acc, sh);
    const float mean = s / nf;
    const float e = sqrtf(mean);
    emax = b == 0 ? e : nan_max(emax, e);            // tensor.max() hands a NaN on
  }
  if (threadIdx.x == 0) E[0] = emax;
}

}  // namespace

int launch_dpm_model_value(const DpmModelValueParams& p, hipStream_t s) {
  SDMI_CHECK(p.n > 0 && p.eps_model && p.out, "dpm_model_value: missing pointer");
  SDMI_CHECK(!p.predict_x0 || p.x, "dpm_model_value: the data prediction needs x");
  SDMI_CHECK(!p.s || (p.predict_x0 && p.row > 0 && p.n % p.row == 0), "dpm_model_value: thresholding needs predict_x0 and n = B * row");
  ProfScope ps("dpm_model_value", 0.0, (double)p.n * 4.0 * (p.cfg ? 4.0 : 3.0), s);
  SDMI_LAUNCH(dpm_model_value_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_dpm_update(const DpmUpdateParams& p, hipStream_t s) {
  SDMI_CHECK(p.n > 0 && p.x && p.m0 && p.out, "dpm_update: missing pointer");
  SDMI_CHECK(p.form >= 0 && p.form <= 3, "dpm_update: form");
  SDMI_CHECK(p.form == 0 || (p.m1 && p.m2), "dpm_update: forms 1-3 take three model values");
  ProfScope ps("dpm_update", 0.0, (double)p.n * 4.0 * (p.form == 0 ? 3.0 : 5.0), s);
  SDMI_LAUNCH(dpm_update_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_dpm_threshold_scale(const float* x0, int B, int64_t row, float max_val, float* s_out, float* stats_out, hipStream_t s) {
  SDMI_CHECK(x0 && s_out && B > 0 && B <= 65535 && row > 0, "dpm_threshold_scale: bad arguments");
  SDMI_CHECK(row <= ((int64_t)1 << 24), "dpm_threshold_scale: rows above 2^24 elements (torch.quantile's fp32 rank is not exact there)");
  // torch.quantile: rank = q * (n - 1) as an fp32 product of the fp32 q, below = floor, above = ceil, weight = rank - below
  const float rank = 0.995f * (float)(row - 1);
  const float below = floorf(rank), above = ceilf(rank);
  const float w = rank - below;
  ProfScope ps("dpm_threshold_scale", 0.0, (double)B * row * 4.0 * 5.0, s);
  SDMI_LAUNCH(dpm_threshold_scale_kernel, dim3((unsigned)B), dim3(kSelThreads), 0, s, x0, row, (unsigned)below, (unsigned)above, w, max_val,
              s_out, stats_out);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int64_t dpm_error_ws_floats(int B, int64_t row) { return (int64_t)B * ((row + kErrChunk - 1) / kErrChunk); }

int launch_dpm_adaptive_error(const float* x_higher, const float* x_lower, const float* x_prev, float atol, float rtol, int B, int64_t row,
                              float* ws, int64_t ws_floats, float* E, hipStream_t s) {
  SDMI_CHECK(x_higher && x_lower && x_prev && ws && E && B > 0 && B <= 65535 && row > 0, "dpm_adaptive_error: bad arguments");
  SDMI_CHECK(row <= ((int64_t)1 << 24), "dpm_adaptive_error: rows above 2^24 elements");
  const int64_t nchunk = (row + kErrChunk - 1) / kErrChunk;
  SDMI_CHECK(ws_floats >= (int64_t)B * nchunk, "dpm_adaptive_error: workspace too small");
  ProfScope ps("dpm_adaptive_error", 0.0, (double)B * row * 4.0 * 3.0, s);
  SDMI_LAUNCH(dpm_error_partial_kernel, dim3((unsigned)nchunk, (unsigned)B), dim3(256), 0, s, x_higher, x_lower, x_prev, atol, rtol, row,
              (int)nchunk, ws);
  SDMI_HIP_OK(hipGetLastError());
  SDMI_LAUNCH(dpm_error_finish_kernel, dim3(1), dim3(256), 0, s, ws, (int)nchunk, B, (float)row, E);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace sdmi
