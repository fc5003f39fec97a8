// Fused classifier-free-guidance combine + PLMS / DDIM latent update (fp32, one launch per sampler step).
// Replaces ~15 elementwise launches + 4 torch.full per step of the reference
// (ldm/models/diffusion/plms.py:178-236, ddim.py:165-204).
// Every operation is an individually rounded fp32 op in the reference's evaluation order (no FMA contraction),
// so with the same eps input the result is bit-identical to the reference's torch expression.
// Also here: the ancestral DDPM step of LatentDiffusion.p_sample (ddpm.py:1047-1107) with the loop's mask blend, one launch as well, and
// the PLMS / DDIM step split at pred_x0 for quantize_x0.
#include "common.h"
#include "prof.h"
#include "sampler_rows.h"
#include "step_math.h"
#include <math.h>

// every product / sum below must round on its own, exactly like the reference's separate torch ops
#pragma clang fp contract(off)

namespace sdmi {
namespace {

// plms.py:201-213, ddim.py:189-199: a_t.sqrt(), a_prev.sqrt(), (1 - a_prev - sigma_t**2).sqrt() -- fp32 tensor ops there, the host's
// fp32 ops here; the one place every launcher of the step takes them from
struct StepScalars { float sqrt_at, sqrt_aprev, dir_coef; };
inline StepScalars step_scalars(float a_t, float a_prev, float sigma) {
  return {sqrtf(a_t), sqrtf(a_prev), sqrtf((1.0f - a_prev) - sigma * sigma)};
}

// The arithmetic of one element, shared by every kernel of the step (the whole launch, its two halves, the per-slot launch): each helper
// is one expression of the reference, op by op (cfg_combine: step_math.h).
__device__ __forceinline__ float multistep_eps(int mode, float e_t, float o0, float o1, float o2) {
#pragma clang fp contract(off)
  switch (mode) {
    case 1: { const float a = 3.f * e_t; const float b = a - o0; return b / 2.f; }
    case 2: {
      const float a = 23.f * e_t, b = 16.f * o0, c = 5.f * o1;
      const float ab = a - b; const float abc = ab + c; return abc / 12.f;
    }
    case 3: {
      const float a = 55.f * e_t, b = 59.f * o0, c = 37.f * o1, d = 9.f * o2;
      const float ab = a - b; const float abc = ab + c; const float abcd = abc - d; return abcd / 24.f;
    }
    case 4: { const float a = o0 + e_t; return a / 2.f; }
    default: return e_t;
  }
}

__device__ __forceinline__ float pred_x0_of(float x, float ep, float sqrt_1m_at, float sqrt_at) {
#pragma clang fp contract(off)
  const float t1 = sqrt_1m_at * ep;
  const float t2 = x - t1;
  return t2 / sqrt_at;
}

// nz: sigma * noise, or 0 without noise
__device__ __forceinline__ float x_prev_of(float pred, float ep, float sqrt_aprev, float dir_coef, float nz) {
#pragma clang fp contract(off)
  const float t3 = sqrt_aprev * pred;
  const float t4 = dir_coef * ep;
  const float xp = t3 + t4;
  return xp + nz;
}

__global__ void __launch_bounds__(256) sampler_step_kernel(SamplerStepParams p, float sqrt_at, float sqrt_aprev,
                                                           float dir_coef) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const float e_t = p.cfg ? cfg_combine(p.eps_model[i], p.eps_model[p.n + i], p.scale) : p.eps_model[i];
  if (p.e_t_out) p.e_t_out[i] = e_t;
  const float o0 = p.mode != 0 ? p.old0[i] : 0.f;
  const float o1 = p.mode == 2 || p.mode == 3 ? p.old1[i] : 0.f;
  const float o2 = p.mode == 3 ? p.old2[i] : 0.f;
  const float ep = multistep_eps(p.mode, e_t, o0, o1, o2);
  if (p.ep_out) p.ep_out[i] = ep;
  const float pred = pred_x0_of(p.x[i], ep, p.sqrt_1m_at, sqrt_at);
  if (p.pred_x0) p.pred_x0[i] = pred;
  if (!p.x_prev) return;                             // first half of the split step: a quantizer runs on pred_x0 next
  const float nz = p.noise ? p.sigma * p.noise[i] : 0.f;
  p.x_prev[i] = x_prev_of(pred, ep, sqrt_aprev, dir_coef, nz);
}

// Second half of the split PLMS / DDIM step (quantize_x0: ddim.py:195-204, plms.py:207-216): from a given pred_x0 -- the codebook rows
// first_stage_model.quantize put in its place -- and the combined eps e' of the first half,
//   x_prev = sqrt(a_prev) * pred_x0 + sqrt(1 - a_prev - sigma^2) * e' + sigma * noise
// the same ops in the same order as the tail of sampler_step_kernel.
__global__ void __launch_bounds__(256) sampler_step_from_x0_kernel(const float* pred_x0, const float* ep, float sqrt_aprev, float dir_coef,
                                                                   float sigma, const float* noise, float* x_prev, int64_t n) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float nz = noise ? sigma * noise[i] : 0.f;
  x_prev[i] = x_prev_of(pred_x0[i], ep[i], sqrt_aprev, dir_coef, nz);
}

// The PLMS / DDIM step of sampler_step_kernel for up to SDMI_SAMPLER_MAX_SLOTS independent latents in one launch: rows of one UNet call
// that stand at different steps of different schedules (sdmi_sampler_step_rows).  blockIdx.y selects the slot, so every field of its
// descriptor is wave-uniform and comes out of the kernel arguments with scalar loads; there is no device-side table.  A slot whose
// pointers are all 16-byte aligned, with n % 4 == 0, moves four elements per lane (`vec`, decided on the host), any other one.
// At 16 K floats per slot this is launch- and latency-bound: no LDS, no atomics, nothing staged.
struct RowSlot {
  sdmi_sampler_slot d;
  float sqrt_at, sqrt_aprev, dir_coef;               // step_scalars() of the slot's table entries
  int vec;
};
struct RowsParams {
  RowSlot slot[SDMI_SAMPLER_MAX_SLOTS];
  int64_t n;
};

template <int V> __device__ __forceinline__ void load_elems(const float* p, int64_t i, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = p[i];
  }
}

template <int V> __device__ __forceinline__ void store_elems(float* p, int64_t i, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  else p[i] = v[0];
}

// elements [i, i + V) of one slot; every input is read before the first output is written, so x_state_out may be x
// (D: sdmi_sampler_slot, or the descriptor of sdmi_sampler_plan_rows, whose kind 0 has the same fields)
template <int V, class D> __device__ __forceinline__ void rows_elems(const D& d, float sqrt_at, float sqrt_aprev, float dir_coef, int64_t i) {
#pragma clang fp contract(off)
  float e_t[V], x[V], o0[V] = {}, o1[V] = {}, o2[V] = {}, nz[V] = {};
  load_elems<V>(d.eps_u, i, e_t);
  if (d.cfg) {
    float ec[V];
    load_elems<V>(d.eps_c, i, ec);
#pragma unroll
    for (int k = 0; k < V; ++k) e_t[k] = cfg_combine(e_t[k], ec[k], d.scale);
  }
  if (d.mode != 0) load_elems<V>(d.old0, i, o0);
  if (d.mode == 2 || d.mode == 3) load_elems<V>(d.old1, i, o1);
  if (d.mode == 3) load_elems<V>(d.old2, i, o2);
  load_elems<V>(d.x, i, x);
  const bool want_x_prev = d.x_state_out || d.unet_dst0 || d.unet_dst1;
  if (want_x_prev && d.noise) {
    load_elems<V>(d.noise, i, nz);
#pragma unroll
    for (int k = 0; k < V; ++k) nz[k] = d.sigma * nz[k];
  }
  float pred[V], xp[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float ep = multistep_eps(d.mode, e_t[k], o0[k], o1[k], o2[k]);
    pred[k] = pred_x0_of(x[k], ep, d.sqrt_1m_at, sqrt_at);
    xp[k] = x_prev_of(pred[k], ep, sqrt_aprev, dir_coef, nz[k]);
  }
  if (d.e_t_out) store_elems<V>(d.e_t_out, i, e_t);
  if (d.pred_x0) store_elems<V>(d.pred_x0, i, pred);
  if (d.x_state_out) store_elems<V>(d.x_state_out, i, xp);
  if (d.unet_dst0) store_elems<V>(d.unet_dst0, i, xp);      // the slot's row(s) of the next UNet call's input
  if (d.unet_dst1) store_elems<V>(d.unet_dst1, i, xp);
}

__global__ void __launch_bounds__(256) sampler_step_rows_kernel(RowsParams p) {
  const RowSlot& r = p.slot[blockIdx.y];
  const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane == 0) {                                   // the slot's timestep in the next call's timestep tensor: one lane, plain stores
    if (r.d.t_dst0) *r.d.t_dst0 = r.d.t_next;
    if (r.d.t_dst1) *r.d.t_dst1 = r.d.t_next;
  }
  if (r.vec) {
    if (lane * 4 < p.n) rows_elems<4>(r.d, r.sqrt_at, r.sqrt_aprev, r.dir_coef, lane * 4);
  } else {
    if (lane < p.n) rows_elems<1>(r.d, r.sqrt_at, r.sqrt_aprev, r.dir_coef, lane);
  }
}

// The same launch shape for slots of two kinds (sdmi_sampler_plan_rows): kind 0 is the step above, field for field; kind 1 is one model
// evaluation of a DPM-Solver plan with the update that follows it -- the model value of dpm_model_value_kernel, then one form of
// dpm_update_kernel whose operands named in m_self are that value, taken from registers.  Both kinds hand the next call its timestep as
// fp32, so PLMS / DDIM and DPM-Solver rows share one call.  The arithmetic is the helpers' the lone kernels call: nothing is restated.
struct PlanSlot {
  sdmi_sampler_plan_slot d;
  float sqrt_at, sqrt_aprev, dir_coef;               // kind 0: step_scalars() of the slot's table entries
  int vec;
};
struct PlanParams {
  PlanSlot slot[SDMI_SAMPLER_MAX_SLOTS];
  int64_t n;
};
static_assert(sizeof(PlanParams) <= 4096, "sampler_plan_rows: the descriptors travel in the kernel arguments (HIP's limit is 4096 bytes)");

// elements [i, i + V) of a kind 1 slot; every input is read before the first output is written, so x_state_out may be x_base or x
template <int V> __device__ __forceinline__ void plan_dpm_elems(const sdmi_sampler_plan_slot& d, int64_t i) {
#pragma clang fp contract(off)
  float m[V], xb[V] = {}, m0[V] = {}, m1[V] = {}, m2[V] = {};
  load_elems<V>(d.eps_u, i, m);
  if (d.cfg) {
    float ec[V];
    load_elems<V>(d.eps_c, i, ec);
#pragma unroll
    for (int k = 0; k < V; ++k) m[k] = cfg_combine(m[k], ec[k], d.scale);
  }
  if (d.data_prediction) {
    float x[V];
    load_elems<V>(d.x, i, x);
#pragma unroll
    for (int k = 0; k < V; ++k) m[k] = dpm_data_prediction(x[k], m[k], d.sigma_t, d.alpha_t);
  }
  if (d.form >= 0) {
    load_elems<V>(d.x_base, i, xb);
    if (!(d.m_self & 1)) load_elems<V>(d.m0, i, m0);
    if (d.form != 0) {
      if (!(d.m_self & 2)) load_elems<V>(d.m1, i, m1);
      if (!(d.m_self & 4)) load_elems<V>(d.m2, i, m2);
    }
  }
  float out[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float a0 = (d.m_self & 1) ? m[k] : m0[k];
    const float a1 = (d.m_self & 2) ? m[k] : m1[k];
    const float a2 = (d.m_self & 4) ? m[k] : m2[k];
    out[k] = d.form >= 0 ? dpm_update_of(d.form, d.c9, xb[k], a0, a1, a2) : m[k];     // no update: the slot's result is the model value
  }
  if (d.m_out) store_elems<V>(d.m_out, i, m);
  if (d.x_state_out) store_elems<V>(d.x_state_out, i, out);
  if (d.unet_dst0) store_elems<V>(d.unet_dst0, i, out);     // the slot's row(s) of the next UNet call's input
  if (d.unet_dst1) store_elems<V>(d.unet_dst1, i, out);
}

template <int V> __device__ __forceinline__ void plan_elems(const PlanSlot& r, int64_t i) {
  if (r.d.kind == 0) rows_elems<V>(r.d, r.sqrt_at, r.sqrt_aprev, r.dir_coef, i);
  else plan_dpm_elems<V>(r.d, i);
}

__global__ void __launch_bounds__(256) sampler_plan_rows_kernel(PlanParams p) {
  const PlanSlot& r = p.slot[blockIdx.y];
  const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane == 0) {                                   // the slot's timestep in the next call's fp32 timestep tensor: one lane, plain stores
    if (r.d.tf_dst0) *r.d.tf_dst0 = r.d.t_next;
    if (r.d.tf_dst1) *r.d.tf_dst1 = r.d.t_next;
  }
  if (r.vec) {
    if (lane * 4 < p.n) plan_elems<4>(r, lane * 4);
  } else {
    if (lane < p.n) plan_elems<1>(r, lane);
  }
}

// Ancestral DDPM step: LatentDiffusion.p_mean_variance + p_sample (ldm/models/diffusion/ddpm.py:1047-1107) and the loop's mask blend
// (:1203-1205), every product and sum rounded on its own in the reference's order:
//   x0     = c_recip * x - c_recipm1 * eps                  predict_start_from_noise (:216-220)
//   x0     = clamp(x0, -1, 1)                               clip_denoised (:1066-1067); a NaN stays NaN, as torch.clamp leaves it
//   mean   = coef1 * x0 + coef2 * x                         q_posterior (:222-229)
//   x_prev = mean + s * noise                               s = nonzero_mask * exp(0.5 * posterior_log_variance_clipped[t]) (:1100-1107)
//   q      = sa * x0_orig + s1ma * q_noise                  q_sample (:274-277)
//   x_prev = q * mask + (1 - mask) * x_prev                 (:1204-1205)
// eps == nullptr: x0 is read from x0_in (after the quantizer; no clamp).  x_prev == nullptr: stops after x0_out.
__global__ void __launch_bounds__(256) ddpm_step_kernel(DdpmStepParams p) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const float x = p.x[i];
  float x0;
  if (p.eps) {
    const float a = p.c_recip * x;
    const float b = p.c_recipm1 * p.eps[i];
    x0 = a - b;
    if (p.clip) x0 = x0 < -1.f ? -1.f : (x0 > 1.f ? 1.f : x0);      // (both compares are false on a NaN)
  } else {
    x0 = p.x0_in[i];
  }
  if (p.x0_out) p.x0_out[i] = x0;
  if (!p.x_prev) return;
  const float m1 = p.coef1 * x0;
  const float m2 = p.coef2 * x;
  const float mean = m1 + m2;
  const float nz = p.s * p.noise[i];
  float xp = mean + nz;
  if (p.mask) {
    const float q1 = p.sa * p.x0_orig[i];
    const float q2 = p.s1ma * p.q_noise[i];
    const float q = q1 + q2;
    const float m = p.mask[i];
    const float qm = q * m;
    const float om = 1.f - m;
    const float keep = om * xp;
    xp = qm + keep;
  }
  p.x_prev[i] = xp;
}

// DPM-Solver++ (multistep, data prediction) -- ldm/models/diffusion/dpm_solver/dpm_solver.py:
//   model value  m0 = (x - sigma_s * e) / alpha_s,  e = classifier-free combine           (:321-346, :386-399)
//   order 1      x_t = cx * x - a * m0                                                     (:519-530; a = alpha_t * expm1(-h))
//   order 2      x_t = cx * x - a * m0 - (0.5 * a) * (inv_r0 * (m0 - m1))                  (:776-790; a = alpha_t * (exp(-h) - 1))
// evaluated op by op in the reference's fp32 order (no contraction).
__global__ void __launch_bounds__(256) dpm_step_kernel(DpmStepParams p) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  float e;
  if (p.cfg) {
    const float eu = p.eps_model[i], ec = p.eps_model[p.n + i];
    const float d = ec - eu;
    const float sd = p.scale * d;
    e = eu + sd;
  } else {
    e = p.eps_model[i];
  }
  const float x = p.x[i];
  const float se = p.sigma_s * e;
  const float num = x - se;
  const float m0 = num / p.alpha_s;
  if (p.m_out) p.m_out[i] = m0;
  if (!p.x_next) return;
  const float t1 = p.cx * x;
  const float t2 = p.a * m0;
  float xt = t1 - t2;
  if (p.order == 2) {
    const float dm = m0 - p.m_prev[i];
    const float D1 = p.inv_r0 * dm;
    const float ha = 0.5f * p.a;
    const float t3 = ha * D1;
    xt = xt - t3;
  }
  p.x_next[i] = xt;
}

// Host post-processing of scripts/txt2img.py:313-324 as one pass on the device: decode_first_stage output (fp32 NCHW,
// nominally [-1, 1]) -> clamp((x + 1) / 2, 0, 1) -> NHWC -> 255 * x -> astype(uint8) (truncation, as numpy does).
// Each step is the reference's own fp32 operation in its order (this file is compiled with -ffp-contract=off), so the
// bytes equal the reference's exactly; 4x fewer bytes cross PCIe than with the fp32 image.
__global__ void __launch_bounds__(256) image_u8_kernel(const float* img, unsigned char* out, int B, int C, int H, int W) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;        // (b, y, x)
  const int64_t HW = (int64_t)H * W;
  if (idx >= (int64_t)B * HW) return;
  const int64_t b = idx / HW, pix = idx - b * HW;
  for (int c = 0; c < C; ++c) {
    float v = img[(b * C + c) * HW + pix];
    v = (v + 1.0f) / 2.0f;                          // txt2img.py:314
    v = fminf(fmaxf(v, 0.0f), 1.0f);                // torch.clamp(min=0, max=1) (a NaN stays NaN -> 0 below, as numpy's cast)
    v = 255.0f * v;                                 // txt2img.py:323
    out[idx * C + c] = (unsigned char)(int)v;       // astype(np.uint8): toward zero
  }
}

}  // namespace

int launch_image_u8(const float* img_nchw, unsigned char* out_nhwc, int B, int C, int H, int W, hipStream_t s) {
  SDMI_CHECK(img_nchw && out_nhwc && B > 0 && C > 0 && H > 0 && W > 0, "image_u8: bad arguments");
  const int64_t n = (int64_t)B * H * W;
  SDMI_LAUNCH(image_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, img_nchw, out_nhwc, B, C, H, W);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_dpm_step(const DpmStepParams& p, hipStream_t s) {
  SDMI_CHECK(p.n > 0 && p.eps_model && p.x && (p.m_out || p.x_next), "dpm_step: missing pointer");
  SDMI_CHECK(p.order == 1 || (p.order == 2 && p.m_prev), "dpm_step: order 1, or 2 with the previous model value");
  ProfScope ps("dpm_step", 0.0, (double)p.n * 4.0 * 6.0, s);
  SDMI_LAUNCH(dpm_step_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_ddpm_step(const DdpmStepParams& p, hipStream_t s) {
  SDMI_CHECK(p.n > 0 && p.x && (p.x0_out || p.x_prev), "ddpm_step: missing pointer");
  SDMI_CHECK((p.eps != nullptr) != (p.x0_in != nullptr), "ddpm_step: pass exactly one of eps / x0_in");
  SDMI_CHECK(!p.x_prev || p.noise, "ddpm_step: noise missing (the reference draws it at t = 0 too)");
  SDMI_CHECK(!p.mask || (p.x_prev && p.x0_orig && p.q_noise), "ddpm_step: the blend needs x_prev, x0_orig and q_noise");
  ProfScope ps("ddpm_step", 0.0, (double)p.n * 4.0 * (p.mask ? 7.0 : 4.0), s);
  SDMI_LAUNCH(ddpm_step_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_sampler_step_from_x0(const float* pred_x0, const float* ep, float a_prev, float sigma, const float* noise, float* x_prev,
                                int64_t n, hipStream_t s) {
  SDMI_CHECK(n > 0 && pred_x0 && ep && x_prev, "sampler_step_from_x0: missing pointer");
  const StepScalars c = step_scalars(1.0f, a_prev, sigma);                   // (a_t belongs to the first half)
  ProfScope ps("sampler_step_from_x0", 0.0, (double)n * 4.0 * 4.0, s);
  SDMI_LAUNCH(sampler_step_from_x0_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pred_x0, ep, c.sqrt_aprev, c.dir_coef, sigma,
              noise, x_prev, n);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_sampler_step(const SamplerStepParams& p, hipStream_t s) {
  SDMI_CHECK(p.n > 0 && p.eps_model && p.x && (p.x_prev || (p.pred_x0 && p.ep_out)), "sampler_step: missing pointer");
  SDMI_CHECK(p.mode >= 0 && p.mode <= 4, "sampler_step: mode");
  SDMI_CHECK(p.mode == 0 || p.old0, "sampler_step: history missing");
  SDMI_CHECK(p.mode != 2 && p.mode != 3 || p.old1, "sampler_step: history missing");
  SDMI_CHECK(p.mode != 3 || p.old2, "sampler_step: history missing");
  const StepScalars c = step_scalars(p.a_t, p.a_prev, p.sigma);
  ProfScope ps("sampler_step", 0.0, (double)p.n * 4.0 * 6.0, s);
  SDMI_LAUNCH(sampler_step_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p, c.sqrt_at, c.sqrt_aprev,
                     c.dir_coef);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_sampler_step_rows(const sdmi_sampler_slot* slots, int n_slots, int64_t n, hipStream_t s) {
  SDMI_CHECK(slots && n_slots >= 1, "sampler_step_rows: no slots");
  SDMI_CHECK(n_slots <= SDMI_SAMPLER_MAX_SLOTS, "sampler_step_rows: more than SDMI_SAMPLER_MAX_SLOTS (8) slots");
  SDMI_CHECK(n > 0 && n <= (int64_t)0x7fffffff * 256, "sampler_step_rows: n");
  RowsParams p = RowsParams();
  p.n = n;
  bool all_vec = true;
  for (int k = 0; k < n_slots; ++k) {
    const sdmi_sampler_slot& d = slots[k];
    const std::string at = " (slot " + std::to_string(k) + ")";
    SDMI_CHECK(d.eps_u && d.x && (!d.cfg || d.eps_c), "sampler_step_rows: missing pointer" + at);
    SDMI_CHECK(d.e_t_out || d.x_state_out || d.pred_x0 || d.unet_dst0 || d.unet_dst1, "sampler_step_rows: missing pointer: no output" + at);
    SDMI_CHECK(d.mode >= 0 && d.mode <= 4, "sampler_step_rows: mode" + at);
    SDMI_CHECK(d.mode == 0 || d.old0, "sampler_step_rows: history missing" + at);
    SDMI_CHECK(d.mode != 2 && d.mode != 3 || d.old1, "sampler_step_rows: history missing" + at);
    SDMI_CHECK(d.mode != 3 || d.old2, "sampler_step_rows: history missing" + at);
    RowSlot& r = p.slot[k];
    r.d = d;
    r.d.reserved = 0;
    if (!d.cfg) r.d.eps_c = nullptr;                 // (eps_u alone is read)
    const StepScalars c = step_scalars(d.a_t, d.a_prev, d.sigma);
    r.sqrt_at = c.sqrt_at; r.sqrt_aprev = c.sqrt_aprev; r.dir_coef = c.dir_coef;
    const void* ptrs[] = {r.d.eps_u, r.d.eps_c, d.x, d.old0, d.old1, d.old2, d.noise, d.e_t_out, d.x_state_out, d.pred_x0, d.unet_dst0,
                          d.unet_dst1};
    uintptr_t bits = (uintptr_t)(n % 4);
    for (const void* q : ptrs) bits |= (uintptr_t)q & 15;    // (a null pointer is aligned)
    r.vec = bits == 0;
    all_vec = all_vec && r.vec;
  }
  const int64_t lanes = all_vec ? n / 4 : n;         // one grid for all slots: a 16-byte slot's surplus blocks return at once
  ProfScope ps("sampler_step_rows", 0.0, (double)n * 4.0 * 7.0 * n_slots, s);
  SDMI_LAUNCH(sampler_step_rows_kernel, dim3((unsigned)((lanes + 255) / 256), (unsigned)n_slots), dim3(256), 0, s, p);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_sampler_plan_rows(const sdmi_sampler_plan_slot* slots, int n_slots, int64_t n, hipStream_t s) {
  SDMI_CHECK(slots && n_slots >= 1, "sampler_plan_rows: no slots");
  SDMI_CHECK(n_slots <= SDMI_SAMPLER_MAX_SLOTS, "sampler_plan_rows: more than SDMI_SAMPLER_MAX_SLOTS (8) slots");
  SDMI_CHECK(n > 0 && n <= (int64_t)0x7fffffff * 256, "sampler_plan_rows: n");
  PlanParams p = PlanParams();
  p.n = n;
  bool all_vec = true;
  for (int k = 0; k < n_slots; ++k) {
    const sdmi_sampler_plan_slot& d = slots[k];
    const std::string at = " (slot " + std::to_string(k) + ")";
    PlanSlot& r = p.slot[k];
    r.d = d;
    r.d.reserved = 0;
    sdmi_sampler_plan_slot& q = r.d;                 // what the kernel reads: the pointers the slot's kind and form do not read are cleared
    SDMI_CHECK(d.kind == 0 || d.kind == 1, "sampler_plan_rows: kind" + at);
    SDMI_CHECK(d.eps_u && (!d.cfg || d.eps_c), "sampler_plan_rows: missing pointer" + at);
    if (!d.cfg) q.eps_c = nullptr;                   // (eps_u alone is read)
    if (d.kind == 0) {
      SDMI_CHECK(d.x, "sampler_plan_rows: missing pointer" + at);
      SDMI_CHECK(d.e_t_out || d.x_state_out || d.pred_x0 || d.unet_dst0 || d.unet_dst1, "sampler_plan_rows: missing pointer: no output" + at);
      SDMI_CHECK(d.mode >= 0 && d.mode <= 4, "sampler_plan_rows: mode" + at);
      SDMI_CHECK(d.mode == 0 || d.old0, "sampler_plan_rows: history missing" + at);
      SDMI_CHECK(d.mode != 2 && d.mode != 3 || d.old1, "sampler_plan_rows: history missing" + at);
      SDMI_CHECK(d.mode != 3 || d.old2, "sampler_plan_rows: history missing" + at);
      const StepScalars c = step_scalars(d.a_t, d.a_prev, d.sigma);
      r.sqrt_at = c.sqrt_at; r.sqrt_aprev = c.sqrt_aprev; r.dir_coef = c.dir_coef;
      q.x_base = q.m0 = q.m1 = q.m2 = nullptr; q.m_out = nullptr;
      q.form = -1; q.m_self = 0; q.data_prediction = 0;
    } else {
      SDMI_CHECK(d.form >= -1 && d.form <= 3, "sampler_plan_rows: form" + at);
      SDMI_CHECK(!d.data_prediction || d.x, "sampler_plan_rows: missing pointer: the data prediction needs x" + at);
      const int reads = d.form < 0 ? 0 : (d.form == 0 ? 1 : 7);       // the operands of m0..m2 the form reads, as a mask
      SDMI_CHECK(d.m_self >= 0 && (d.m_self & ~reads) == 0, "sampler_plan_rows: m_self names an operand the form does not read" + at);
      SDMI_CHECK(d.form < 0 || d.x_base, "sampler_plan_rows: missing pointer: x_base" + at);
      const float* const ms[3] = {d.m0, d.m1, d.m2};
      for (int j = 0; j < 3; ++j)
        SDMI_CHECK(!((reads & ~d.m_self) >> j & 1) || ms[j], "sampler_plan_rows: missing pointer: a model value of the update" + at);
      SDMI_CHECK(d.m_out || d.x_state_out || d.unet_dst0 || d.unet_dst1, "sampler_plan_rows: missing pointer: no output" + at);
      if (!d.data_prediction) q.x = nullptr;
      if (d.form < 0) q.x_base = nullptr;
      if (!((reads & ~d.m_self) & 1)) q.m0 = nullptr;
      if (!((reads & ~d.m_self) & 2)) q.m1 = nullptr;
      if (!((reads & ~d.m_self) & 4)) q.m2 = nullptr;
      q.old0 = q.old1 = q.old2 = q.noise = nullptr; q.e_t_out = q.pred_x0 = nullptr;
      q.mode = 0;
    }
    const void* ptrs[] = {q.eps_u, q.eps_c, q.x, q.old0, q.old1, q.old2, q.noise, q.x_base, q.m0, q.m1, q.m2, q.e_t_out, q.pred_x0, q.m_out,
                          q.x_state_out, q.unet_dst0, q.unet_dst1};
    uintptr_t bits = (uintptr_t)(n % 4);
    for (const void* v : ptrs) bits |= (uintptr_t)v & 15;    // (a null pointer is aligned)
    r.vec = bits == 0;
    all_vec = all_vec && r.vec;
  }
  const int64_t lanes = all_vec ? n / 4 : n;         // one grid for all slots: a 16-byte slot's surplus blocks return at once
  ProfScope ps("sampler_plan_rows", 0.0, (double)n * 4.0 * 7.0 * n_slots, s);
  SDMI_LAUNCH(sampler_plan_rows_kernel, dim3((unsigned)((lanes + 255) / 256), (unsigned)n_slots), dim3(256), 0, s, p);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace sdmi
