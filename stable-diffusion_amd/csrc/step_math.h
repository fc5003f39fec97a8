// The per-element arithmetic that more than one sampler kernel evaluates (sampler.hip, dpm.hip): the classifier-free combine, DPM-Solver's
// model value and its four update forms.  Each helper is one expression of the reference, every product, sum and quotient rounded on its
// own in the reference's order (no contraction), so a kernel that calls it writes the bits of every other kernel that does.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace sdmi {

__device__ __forceinline__ float cfg_combine(float eu, float ec, float scale) {
#pragma clang fp contract(off)
  const float d = ec - eu;
  const float sd = scale * d;
  return eu + sd;                                    // e_u + s * (e_c - e_u)
}

// data_prediction_fn (dpm_solver.py:393): x0 = (x - sigma_t * e) / alpha_t
__device__ __forceinline__ float dpm_data_prediction(float x, float e, float sigma_t, float alpha_t) {
#pragma clang fp contract(off)
  const float se = sigma_t * e;
  const float num = x - se;
  return num / alpha_t;
}

// The update forms of sdmi_dpm_update (dpm.hip's table; include/sdmi.h): c points at the nine host scalars.  Form 0 reads x and m0 alone.
__device__ __forceinline__ float dpm_update_of(int form, const float* c, float x, float m0, float m1, float m2) {
#pragma clang fp contract(off)
  const float t0 = c[0] * x;
  const float t1 = c[1] * m0;
  float xt = t0 + t1;
  if (form == 1) {
    const float d = m1 - m2;
    const float D = c[3] * d;
    const float t2 = c[2] * D;
    xt = xt + t2;
  } else if (form == 2) {
    const float a = m1 - m0, b = m2 - m0;
    const float d10 = c[4] * a, d11 = c[5] * b;
    const float u = c[6] * d10, v = c[7] * d11;
    const float uv = u - v;
    const float D1 = uv / c[8];
    const float w = d11 - d10;
    const float w2 = 2.f * w;
    const float D2 = w2 / c[8];
    const float t2 = c[2] * D1, t3 = c[3] * D2;
    xt = xt + t2;
    xt = xt + t3;
  } else if (form == 3) {
    const float a = m0 - m1, b = m1 - m2;
    const float d10 = c[4] * a, d11 = c[5] * b;
    const float dd = d10 - d11;
    const float q = c[6] * dd;
    const float D1 = d10 + q;
    const float D2 = c[7] * dd;
    const float t2 = c[2] * D1, t3 = c[3] * D2;
    xt = xt + t2;
    xt = xt + t3;
  }
  return xt;
}

}  // namespace sdmi
