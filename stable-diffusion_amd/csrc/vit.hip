// Streaming kernels around the CLIP vision tower (clip.cpp: ClipVision), i.e. transformers' CLIPVisionModelWithProjection as the safety
// checker of scripts/txt2img.py:check_safety and FrozenClipImageEmbedder (ldm/modules/encoders/modules.py:197-228) run it:
//   * vit_patchify_kernel:   the im2col of the stride-p, p x p patch-embedding convolution, fp32 NCHW -> fp16 rows [B P^2][Kp].  Column
//     k = (c * p + ky) * p + kx is the flattening of the conv weight's [3][p][p] tail, so the packed weight is the weight's own rows
//     (W_ROWS16_PAD64); columns K .. Kp - 1 (K = 3 p^2 = 588 -> Kp = 640, the next multiple of the 64-wide k-tile) are written as zeros.
//   * vit_embed_kernel:      the fp32 token matrix [B][1 + P^2][C]: row 0 = class_embedding + position_embedding[0], row 1 + i = patch row i
//     + position_embedding[1 + i] (one fp32 add per element, the reference's).
//   * vit_preprocess_kernel: FrozenClipImageEmbedder.preprocess -- bicubic resize (align_corners=True, A = -0.75, clamped border taps, no
//     antialiasing), (x + 1) / 2, (x - mean) / std.
//   * safety_head_kernel:    StableDiffusionSafetyChecker's concept head, one workgroup per image.
// No atomics, no cross-workgroup communication; every sum has one fixed order.
#include "common.h"
#include "prof.h"

namespace sdmi {
namespace {

// (the reference rounds every product and sum of these expressions: no contraction into FMAs)
#pragma clang fp contract(off)

// one thread per 8 consecutive columns of one output row (Kp % 8 == 0: one 16-byte store); n = B * P * P * (Kp / 8)
__global__ void __launch_bounds__(256) vit_patchify_kernel(const float* __restrict__ px, f16* __restrict__ out, int S, int p, int P, int K,
                                                           int Kp, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int kq = Kp / 8;
  const int k0 = (int)(i % kq) * 8;
  const int64_t row = i / kq;                       // (b * P + py) * P + pxi
  const int pxi = (int)(row % P);
  const int py = (int)((row / P) % P);
  const int64_t b = row / ((int64_t)P * P);
  const int pp = p * p;
  f16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    float t = 0.f;
    if (k < K) {
      const int c = k / pp, r = k - c * pp;
      const int ky = r / p, kx = r - ky * p;
      t = px[((b * 3 + c) * S + (py * p + ky)) * (int64_t)S + (pxi * p + kx)];
    }
    v[e] = (f16)t;
  }
  *(f16x8*)(out + row * Kp + k0) = v;
}

// one thread per 4 consecutive channels of one token row; n = B * T * (C / 4)
__global__ void __launch_bounds__(256) vit_embed_kernel(const float* __restrict__ patch, const float* __restrict__ cls,
                                                        const float* __restrict__ pos, float* __restrict__ out, int T, int C, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int cq = C / 4;
  const int c = (int)(i % cq) * 4;
  const int64_t r = i / cq;                         // b * T + t
  const int t = (int)(r % T);
  const int64_t b = r / T;
  const f32x4 a = t == 0 ? *(const f32x4*)(cls + c) : *(const f32x4*)(patch + (b * (T - 1) + (t - 1)) * C + c);
  const f32x4 q = *(const f32x4*)(pos + (int64_t)t * C + c);
  *(f32x4*)(out + r * C + c) = f32x4{a[0] + q[0], a[1] + q[1], a[2] + q[2], a[3] + q[3]};
}

// cubic-convolution weights of the four taps around a sample at fractional offset t (A = -0.75)
__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
  w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  w[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
  w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
  w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

// one thread per V consecutive output pixels of a row (V == 4: S % 4 == 0 and an aligned output, one 16-byte store); n = B * 3 * S * (S / V)
template <int V>
__global__ void __launch_bounds__(256) vit_preprocess_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int S,
                                                             float sy, float sx, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int sv = S / V;
  const int ox0 = (int)(i % sv) * V;
  int64_t r = i / sv;
  const int oy = (int)(r % S);
  r /= S;                                           // b * 3 + c
  const int c = (int)(r % 3);
  const float mean = c == 0 ? 0.48145466f : (c == 1 ? 0.4578275f : 0.40821073f);
  const float sd = c == 0 ? 0.26862954f : (c == 1 ? 0.26130258f : 0.27577711f);
  const float* src = x + r * (int64_t)H * W;
  const float fy = sy * (float)oy;
  const float fy0 = floorf(fy);
  const int iy = (int)fy0;
  float wy[4];
  cubic_weights(fy - fy0, wy);
  float res[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const float fx = sx * (float)(ox0 + j);
    const float fx0 = floorf(fx);
    const int ix = (int)fx0;
    float wx[4];
    cubic_weights(fx - fx0, wx);
    int xi[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) xi[a] = min(max(ix - 1 + a, 0), W - 1);
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float* rowp = src + (int64_t)min(max(iy - 1 + a, 0), H - 1) * W;
      const float rv = ((rowp[xi[0]] * wx[0] + rowp[xi[1]] * wx[1]) + rowp[xi[2]] * wx[2]) + rowp[xi[3]] * wx[3];
      acc = acc + rv * wy[a];
    }
    res[j] = ((acc + 1.f) / 2.f - mean) / sd;
  }
  float* dst = out + (r * S + oy) * (int64_t)S + ox0;
  if constexpr (V == 4) *(f32x4*)dst = f32x4{res[0], res[1], res[2], res[3]};
  else dst[0] = res[0];
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

constexpr int SH_MAXN = 64;          // concepts / special-care concepts per launch
constexpr int SH_MAXE = 8192;        // embedding width (LDS: 4 (E + 132) bytes)

// One workgroup of 4 waves per image.  cos(a, b) = sum_e (a_e / max(|a|, 1e-12)) (b_e / max(|b|, 1e-12)): both vectors are normalised element by
// element first (torch.nn.functional.normalize), then multiplied.  A wave owns a concept: lanes stride over E in quads, one butterfly.
// Thread 0 then walks the special-care concepts and the concepts in index order with the running adjustment.
__global__ void __launch_bounds__(256) safety_head_kernel(const float* __restrict__ img, const float* __restrict__ concepts,
                                                          const float* __restrict__ special, const float* __restrict__ concept_thr,
                                                          const float* __restrict__ special_thr, int* __restrict__ has_nsfw,
                                                          float* __restrict__ concept_scores, float* __restrict__ special_scores, int Nc,
                                                          int Ns, int E) {
  // all LDS in the dynamic region (no static array in front of it: its base stays 16-byte aligned for the 16-byte reads of s_img)
  extern __shared__ __attribute__((aligned(16))) float s_img[];      // [E] the normalised image vector
  float* s_cos = s_img + E;                         // [2 SH_MAXN]: [0, Ns) special-care, [SH_MAXN, SH_MAXN + Nc) concepts
  float* s_red = s_cos + 2 * SH_MAXN;               // [4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const float* ib = img + (int64_t)b * E;
  float ss = 0.f;
  for (int e = tid * 4; e < E; e += 1024) {
    const f32x4 v = *(const f32x4*)(ib + e);
    ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  ss = wave_sum(ss);
  if (lane == 0) s_red[wave] = ss;
  __syncthreads();
  const float inorm = fmaxf(sqrtf((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])), 1e-12f);
  for (int e = tid * 4; e < E; e += 1024) {
    const f32x4 v = *(const f32x4*)(ib + e);
    *(f32x4*)(s_img + e) = f32x4{v[0] / inorm, v[1] / inorm, v[2] / inorm, v[3] / inorm};
  }
  __syncthreads();
  for (int j = wave; j < Ns + Nc; j += 4) {
    const float* cv = j < Ns ? special + (int64_t)j * E : concepts + (int64_t)(j - Ns) * E;
    float cs = 0.f;
    for (int e = lane * 4; e < E; e += 256) {
      const f32x4 v = *(const f32x4*)(cv + e);
      cs += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    const float cnorm = fmaxf(sqrtf(wave_sum(cs)), 1e-12f);
    float dot = 0.f;
    for (int e = lane * 4; e < E; e += 256) {
      const f32x4 v = *(const f32x4*)(cv + e);
      const f32x4 q = *(const f32x4*)(s_img + e);
      dot += ((v[0] / cnorm) * q[0] + (v[1] / cnorm) * q[1]) + ((v[2] / cnorm) * q[2] + (v[3] / cnorm) * q[3]);
    }
    dot = wave_sum(dot);
    if (lane == 0) s_cos[j < Ns ? j : SH_MAXN + (j - Ns)] = dot;
  }
  __syncthreads();
  if (tid == 0) {
    float adjustment = 0.f;
    for (int j = 0; j < Ns; ++j) {
      const float s = rintf(((s_cos[j] - special_thr[j]) + adjustment) * 1000.f) / 1000.f;       // three decimals, half to even
      special_scores[(int64_t)b * Ns + j] = s;
      if (s > 0.f) adjustment = 0.01f;
    }
    int bad = 0;
    for (int j = 0; j < Nc; ++j) {
      const float s = rintf(((s_cos[SH_MAXN + j] - concept_thr[j]) + adjustment) * 1000.f) / 1000.f;
      concept_scores[(int64_t)b * Nc + j] = s;
      if (s > 0.f) bad = 1;
    }
    has_nsfw[b] = bad;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int vit_kpad(int patch_size) { return (int)round_up((int64_t)3 * patch_size * patch_size, 64); }

int launch_vit_patchify(const float* px, f16* out, int B, int S, int p, hipStream_t s) {
  SDMI_CHECK(px && out && B >= 1 && p >= 1 && S >= p && S % p == 0 && S <= 4096 && p <= 64, "vit_patchify: image_size % patch_size != 0 (or bad arguments)");
  SDMI_CHECK(aligned16(out), "vit_patchify: the output rows must be 16-byte aligned");
  const int P = S / p, K = 3 * p * p, Kp = vit_kpad(p);
  const int64_t n = (int64_t)B * P * P * (Kp / 8);
  SDMI_CHECK((n + 255) / 256 <= 0x7fffffff, "vit_patchify: too many elements for one launch");
  ProfScope ps("vit_patchify", 0.0, (double)B * 3 * S * S * 4.0 + (double)B * P * P * Kp * 2.0, s);
  SDMI_LAUNCH(vit_patchify_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, px, out, S, p, P, K, Kp, n);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_vit_embed(const float* patch, const float* cls, const float* pos, float* out, int B, int T, int C, hipStream_t s) {
  SDMI_CHECK(patch && cls && pos && out && B >= 1 && T >= 2 && C >= 4 && C % 4 == 0, "vit_embed: C % 4 (or bad arguments)");
  SDMI_CHECK(aligned16(patch) && aligned16(cls) && aligned16(pos) && aligned16(out), "vit_embed: operands must be 16-byte aligned");
  const int64_t n = (int64_t)B * T * (C / 4);
  SDMI_CHECK((n + 255) / 256 <= 0x7fffffff, "vit_embed: too many elements for one launch");
  ProfScope ps("vit_embed", 0.0, (double)B * T * C * 12.0, s);
  SDMI_LAUNCH(vit_embed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, patch, cls, pos, out, T, C, n);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_vit_preprocess(const float* x, float* out, int B, int H, int W, int S, hipStream_t s) {
  SDMI_CHECK(x && out && B >= 1 && H >= 1 && W >= 1 && S >= 1 && H <= 16384 && W <= 16384 && S <= 16384, "vit_preprocess: bad arguments");
  // align_corners=True: source coordinate = destination index * (in - 1) / (out - 1), the scale taken in fp32 as the reference takes it
  const float sy = S > 1 ? (float)(H - 1) / (float)(S - 1) : 0.f, sx = S > 1 ? (float)(W - 1) / (float)(S - 1) : 0.f;
  const bool v4 = S % 4 == 0 && aligned16(out);
  const int64_t n = (int64_t)B * 3 * S * (S / (v4 ? 4 : 1));
  SDMI_CHECK((n + 255) / 256 <= 0x7fffffff, "vit_preprocess: too many elements for one launch");
  ProfScope ps("vit_preprocess", 40.0 * B * 3 * S * (double)S, (double)B * 3 * ((double)H * W + (double)S * S) * 4.0, s);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (v4) SDMI_LAUNCH(vit_preprocess_kernel<4>, grid, dim3(256), 0, s, x, out, H, W, S, sy, sx, n);
  else SDMI_LAUNCH(vit_preprocess_kernel<1>, grid, dim3(256), 0, s, x, out, H, W, S, sy, sx, n);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_safety_head(const float* image_embeds, const float* concept_embeds, const float* special_care_embeds, const float* concept_thr,
                       const float* special_thr, int* has_nsfw, float* concept_scores, float* special_scores, int B, int Nc, int Ns, int E,
                       hipStream_t s) {
  SDMI_CHECK(image_embeds && concept_embeds && concept_thr && has_nsfw && concept_scores && B >= 1 && B <= 65535, "safety_head: bad arguments");
  SDMI_CHECK(Nc >= 1 && Nc <= SH_MAXN && Ns >= 0 && Ns <= SH_MAXN, "safety_head: 1 <= Nc <= 64 concepts, 0 <= Ns <= 64 special-care concepts");
  SDMI_CHECK(Ns == 0 || (special_care_embeds && special_thr && special_scores), "safety_head: special-care operands missing");
  SDMI_CHECK(E >= 4 && E % 4 == 0 && E <= SH_MAXE, "safety_head: the embedding width E must be a multiple of 4 (<= 8192)");
  SDMI_CHECK(aligned16(image_embeds) && aligned16(concept_embeds) && (Ns == 0 || aligned16(special_care_embeds)),
             "safety_head: the embedding matrices must be 16-byte aligned");
  ProfScope ps("safety_head", 4.0 * B * (double)(Nc + Ns) * E, ((double)B * (1 + Nc + Ns)) * E * 4.0, s);
  SDMI_LAUNCH(safety_head_kernel, dim3(B), dim3(256), (size_t)(E + 2 * SH_MAXN + 4) * sizeof(float), s, image_embeds, concept_embeds, special_care_embeds,
              concept_thr, special_thr, has_nsfw, concept_scores, special_scores, Nc, Ns, E);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace sdmi
