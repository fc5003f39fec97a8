// Fused classifier-free-guidance combine + PLMS / DDIM latent update (fp32, one launch per sampler step).
// Replaces ~15 elementwise launches + 4 torch.full per step of the reference
// (ldm/models/diffusion/plms.py:178-236, ddim.py:165-204).
// Every operation is an individually rounded fp32 op in the reference's evaluation order (no FMA contraction),
// so with the same eps input the result is bit-identical to the reference's torch expression.
// Also here: the ancestral DDPM step of LatentDiffusion.p_sample (ddpm.py:1047-1107) with the loop's mask blend, one launch as well, and
// the PLMS / DDIM step split at pred_x0 for quantize_x0.
#include "common.h"
#include "prof.h"
#include <math.h>

// every product / sum below must round on its own, exactly like the reference's separate torch ops
#pragma clang fp contract(off)

namespace sdmi {
namespace {

__global__ void __launch_bounds__(256) sampler_step_kernel(SamplerStepParams p, float sqrt_at, float sqrt_aprev,
                                                           float dir_coef) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  float e_t;
  if (p.cfg) {
    const float eu = p.eps_model[i], ec = p.eps_model[p.n + i];
    const float d = ec - eu;
    const float sd = p.scale * d;
    e_t = eu + sd;                                   // e_u + s * (e_c - e_u)
  } else {
    e_t = p.eps_model[i];
  }
  if (p.e_t_out) p.e_t_out[i] = e_t;
  float ep;
  switch (p.mode) {
    case 1: { const float a = 3.f * e_t; const float b = a - p.old0[i]; ep = b / 2.f; break; }
    case 2: {
      const float a = 23.f * e_t, b = 16.f * p.old0[i], c = 5.f * p.old1[i];
      const float ab = a - b; const float abc = ab + c; ep = abc / 12.f; break;
    }
    case 3: {
      const float a = 55.f * e_t, b = 59.f * p.old0[i], c = 37.f * p.old1[i], d = 9.f * p.old2[i];
      const float ab = a - b; const float abc = ab + c; const float abcd = abc - d; ep = abcd / 24.f; break;
    }
    case 4: { const float a = p.old0[i] + e_t; ep = a / 2.f; break; }
    default: ep = e_t; break;
  }
  if (p.ep_out) p.ep_out[i] = ep;
  const float x = p.x[i];
  const float t1 = p.sqrt_1m_at * ep;
  const float t2 = x - t1;
  const float pred = t2 / sqrt_at;
  if (p.pred_x0) p.pred_x0[i] = pred;
  if (!p.x_prev) return;                             // first half of the split step: a quantizer runs on pred_x0 next
  const float t3 = sqrt_aprev * pred;
  const float t4 = dir_coef * ep;
  float xp = t3 + t4;
  const float nz = p.noise ? p.sigma * p.noise[i] : 0.f;
  xp = xp + nz;
  p.x_prev[i] = xp;
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
  const float t3 = sqrt_aprev * pred_x0[i];
  const float t4 = dir_coef * ep[i];
  float xp = t3 + t4;
  const float nz = noise ? sigma * noise[i] : 0.f;
  xp = xp + nz;
  x_prev[i] = xp;
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
  const float sqrt_aprev = sqrtf(a_prev);                                    // (as launch_sampler_step)
  const float dir_coef = sqrtf((1.0f - a_prev) - sigma * sigma);
  ProfScope ps("sampler_step_from_x0", 0.0, (double)n * 4.0 * 4.0, s);
  SDMI_LAUNCH(sampler_step_from_x0_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pred_x0, ep, sqrt_aprev, dir_coef, sigma,
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
  // plms.py:201-213: a_t.sqrt(), a_prev.sqrt(), (1 - a_prev - sigma_t**2).sqrt()  -- fp32 tensor ops
  const float sqrt_at = sqrtf(p.a_t);
  const float sqrt_aprev = sqrtf(p.a_prev);
  const float dir_coef = sqrtf((1.0f - p.a_prev) - p.sigma * p.sigma);
  ProfScope ps("sampler_step", 0.0, (double)p.n * 4.0 * 6.0, s);
  SDMI_LAUNCH(sampler_step_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p, sqrt_at, sqrt_aprev,
                     dir_coef);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace sdmi
