// extern "C" surface of libsdmi (include/sdmi.h).  Thin: argument checks, struct translation, error capture.
#include <string.h>

#include <new>

#include "prof.h"
#include "split16.h"
#include "unet.h"
#include "vae.h"
#include "clip.h"
#include "knn.h"
#include "rescale.h"
#include "fe_coeffs.h"
#include "feature_extractor.h"
#include "sampler_rows.h"

namespace sdmi {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int fail(const std::string& msg) { g_err = msg; return -1; }
}  // namespace sdmi

struct sdmi_unet { sdmi::UNet impl; };
struct sdmi_vae { sdmi::Vae impl; };
struct sdmi_clip { sdmi::ClipText impl; };
struct sdmi_bert { sdmi::BertText impl; };
struct sdmi_vit { sdmi::ClipVision impl; };
struct sdmi_knn { sdmi::Knn impl; };

using namespace sdmi;

static int weight_info(const WeightStore& w, int idx, char* key_buf, int key_buf_len, int64_t* shape4, int* ndim) {
  SDMI_CHECK(key_buf && shape4 && ndim, "null argument");
  SDMI_CHECK(idx >= 0 && idx < (int)w.slots().size(), "weight index out of range");
  const WeightSlot& s = w.slots()[idx];
  SDMI_CHECK((int)s.key.size() + 1 <= key_buf_len, "key buffer too small");
  memcpy(key_buf, s.key.c_str(), s.key.size() + 1);
  *ndim = (int)s.shape.size();
  for (int i = 0; i < 4; ++i) shape4[i] = i < *ndim ? s.shape[i] : 1;
  return 0;
}

static void* g_zero_page[16] = {nullptr};
static int zero_page(const f16** out) {
  int dev = 0;
  SDMI_HIP_OK(hipGetDevice(&dev));
  SDMI_CHECK(dev >= 0 && dev < 16, "device index");
  if (!g_zero_page[dev]) {
    SDMI_HIP_OK(hipMalloc(&g_zero_page[dev], 4096));
    SDMI_HIP_OK(hipMemset(g_zero_page[dev], 0, 4096));
  }
  *out = (const f16*)g_zero_page[dev];
  return 0;
}

extern "C" {

const char* sdmi_last_error(void) { return g_err.c_str(); }
int sdmi_abi_version(void) { return SDMI_ABI_VERSION; }
int sdmi_has_experiments(void) { return 0; }      // (see include/sdmi.h)

int sdmi_unet_create(const sdmi_unet_cfg* cfg, sdmi_unet** out) { return sdmi_unet_create_with_precision(cfg, SDMI_PRECISION_MIXED, out); }
int sdmi_unet_create_with_precision(const sdmi_unet_cfg* cfg, int precision, sdmi_unet** out) {
  SDMI_CHECK(cfg && out, "null argument");
  SDMI_CHECK(precision == SDMI_PRECISION_MIXED || precision == SDMI_PRECISION_FULL,
             "precision must be SDMI_PRECISION_MIXED (0) or SDMI_PRECISION_FULL (1), got " + std::to_string(precision));
  sdmi_unet* h = new (std::nothrow) sdmi_unet();
  SDMI_CHECK(h != nullptr, "out of host memory");
  if (h->impl.build(*cfg, precision)) { delete h; return -1; }
  *out = h;
  return 0;
}
int sdmi_unet_create_ext(const sdmi_unet_cfg* cfg, const sdmi_unet_ext* ext, int precision, sdmi_unet** out) {
  return sdmi_unet_create_flags(cfg, ext, 0u, precision, out);
}
int sdmi_unet_create_flags(const sdmi_unet_cfg* cfg, const sdmi_unet_ext* ext, unsigned flags, int precision, sdmi_unet** out) {
  SDMI_CHECK(cfg && out, "null argument");
  SDMI_CHECK(precision == SDMI_PRECISION_MIXED || precision == SDMI_PRECISION_FULL,
             "precision must be SDMI_PRECISION_MIXED (0) or SDMI_PRECISION_FULL (1), got " + std::to_string(precision));
  sdmi_unet* h = new (std::nothrow) sdmi_unet();
  SDMI_CHECK(h != nullptr, "out of host memory");
  if (h->impl.build(*cfg, precision, ext, flags)) { delete h; return -1; }
  *out = h;
  return 0;
}
int sdmi_unet_precision(const sdmi_unet* h) {
  if (!h) { fail("null handle"); return -1; }
  return h->impl.precision_;
}
int sdmi_unet_destroy(sdmi_unet* h) { delete h; return 0; }
int sdmi_unet_num_weights(const sdmi_unet* h) { return h ? (int)h->impl.weights().slots().size() : fail("null handle"); }
int sdmi_unet_weight_info(const sdmi_unet* h, int idx, char* key_buf, int key_buf_len, int64_t* shape4, int* ndim) {
  SDMI_CHECK(h, "null argument");
  return weight_info(h->impl.weights(), idx, key_buf, key_buf_len, shape4, ndim);
}
int sdmi_unet_set_weight(sdmi_unet* h, const char* key, const float* ptr, const int64_t* shape, int ndim, void* stream) {
  SDMI_CHECK(h && key && ptr && shape, "null argument");
  return h->impl.set_weight(key, ptr, shape, ndim, (hipStream_t)stream);
}
int sdmi_unet_finalize(sdmi_unet* h) { SDMI_CHECK(h, "null handle"); return h->impl.finalize(); }

int64_t sdmi_unet_packed_bytes(sdmi_unet* h) {
  if (!h) { fail("null handle"); return 0; }
  int64_t total = 0;
  h->impl.packed_layout(nullptr, &total);
  return total;
}
int sdmi_unet_export_packed(sdmi_unet* h, void* host_buf, int64_t bytes, void* stream) {
  SDMI_CHECK(h && host_buf, "null argument");
  return h->impl.export_packed(host_buf, bytes, (hipStream_t)stream);
}
int sdmi_unet_import_packed(sdmi_unet* h, const void* host_buf, int64_t bytes, void* stream) {
  SDMI_CHECK(h && host_buf, "null argument");
  return h->impl.import_packed(host_buf, bytes, (hipStream_t)stream);
}

int64_t sdmi_unet_workspace_bytes(sdmi_unet* h, int B, int H, int W, int Lctx) {
  if (!h) { fail("null handle"); return 0; }
  int64_t need = 0;
  if (h->impl.run(nullptr, nullptr, nullptr, nullptr, nullptr, B, H, W, Lctx, nullptr, 0, nullptr, true, false, &need)) return 0;
  return need;
}
int sdmi_unet_cache_context(sdmi_unet* h, const float* ctx, int B, int Lctx, void* workspace, int64_t workspace_bytes,
                            void* stream) {
  SDMI_CHECK(h && ctx, "null argument");
  const int down = 1 << (h->impl.cfg_.n_levels - 1);
  return h->impl.run(nullptr, nullptr, nullptr, ctx, nullptr, B, down, down, Lctx, workspace, workspace_bytes,
                     (hipStream_t)stream, false, true, nullptr);
}
int sdmi_unet_reserve_context(sdmi_unet* h, int B, int Lctx) {
  SDMI_CHECK(h, "null argument");
  SDMI_CHECK(B >= 1 && B <= 8 && Lctx >= 1, "bad context shape");
  return h->impl.reserve_ctx_cache(B, Lctx);
}
int sdmi_unet_cache_timesteps(sdmi_unet* h, const int64_t* t_host, int n, void* stream) {
  SDMI_CHECK(h, "null argument");
  return h->impl.cache_timesteps(t_host, n, (hipStream_t)stream);
}
int sdmi_unet_hint_timestep(sdmi_unet* h, int64_t t) {
  SDMI_CHECK(h, "null argument");
  return h->impl.hint_timestep(t);
}
int sdmi_unet_tape_stats(sdmi_unet* h, int64_t* replayed, int64_t* recorded) {
  SDMI_CHECK(h, "null argument");
  if (replayed) *replayed = (int64_t)h->impl.tape_hits_;
  if (recorded) *recorded = (int64_t)h->impl.tape_records_;
  return 0;
}
int sdmi_unet_forward(sdmi_unet* h, const float* x, const int64_t* t_i64, const float* t_f32, const float* ctx,
                      float* eps_out, int B, int H, int W, int Lctx, void* workspace, int64_t workspace_bytes, void* stream) {
  SDMI_CHECK(h && x && eps_out, "null argument");
  SDMI_CHECK((t_i64 != nullptr) != (t_f32 != nullptr), "pass exactly one of t_i64 / t_f32");
  return h->impl.run(x, t_i64, t_f32, ctx, eps_out, B, H, W, Lctx, workspace, workspace_bytes, (hipStream_t)stream, false,
                     false, nullptr);
}

int sdmi_sampler_step(const float* eps_model, int cfg, float scale, const float* x, int mode, const float* old0,
                      const float* old1, const float* old2, float a_t, float a_prev, float sigma, float sqrt_1m_at,
                      const float* noise, float* e_t_out, float* x_prev, float* pred_x0, int64_t n, void* stream) {
  SamplerStepParams p = SamplerStepParams();
  p.eps_model = eps_model; p.cfg = cfg; p.scale = scale; p.x = x; p.mode = mode;
  p.old0 = old0; p.old1 = old1; p.old2 = old2;
  p.a_t = a_t; p.a_prev = a_prev; p.sigma = sigma; p.sqrt_1m_at = sqrt_1m_at;
  p.noise = noise; p.e_t_out = e_t_out; p.x_prev = x_prev; p.pred_x0 = pred_x0; p.n = n;
  SDMI_CHECK(x_prev, "sampler_step: missing pointer");
  return launch_sampler_step(p, (hipStream_t)stream);
}

int sdmi_sampler_step_x0(const float* eps_model, int cfg, float scale, const float* x, int mode, const float* old0, const float* old1,
                         const float* old2, float a_t, float sqrt_1m_at, float* e_t_out, float* ep_out, float* pred_x0, int64_t n,
                         void* stream) {
  SamplerStepParams p = SamplerStepParams();
  p.eps_model = eps_model; p.cfg = cfg; p.scale = scale; p.x = x; p.mode = mode;
  p.old0 = old0; p.old1 = old1; p.old2 = old2;
  p.a_t = a_t; p.sqrt_1m_at = sqrt_1m_at;
  p.e_t_out = e_t_out; p.ep_out = ep_out; p.pred_x0 = pred_x0; p.n = n;
  return launch_sampler_step(p, (hipStream_t)stream);
}

int sdmi_sampler_step_from_x0(const float* pred_x0, const float* ep, float a_prev, float sigma, const float* noise, float* x_prev,
                              int64_t n, void* stream) {
  return launch_sampler_step_from_x0(pred_x0, ep, a_prev, sigma, noise, x_prev, n, (hipStream_t)stream);
}

int sdmi_sampler_step_rows(const sdmi_sampler_slot* slots, int n_slots, int64_t n, void* stream) {
  return launch_sampler_step_rows(slots, n_slots, n, (hipStream_t)stream);
}

int sdmi_sampler_plan_rows(const sdmi_sampler_plan_slot* slots, int n_slots, int64_t n, void* stream) {
  return launch_sampler_plan_rows(slots, n_slots, n, (hipStream_t)stream);
}

int sdmi_ddpm_step(const float* eps, const float* x0_in, const float* x, float c_recip, float c_recipm1, int clip, float coef1,
                   float coef2, float s, const float* noise, const float* mask, const float* x0_orig, const float* q_noise, float sa,
                   float s1ma, float* x0_out, float* x_prev, int64_t n, void* stream) {
  DdpmStepParams p = DdpmStepParams();
  p.eps = eps; p.x0_in = x0_in; p.x = x; p.c_recip = c_recip; p.c_recipm1 = c_recipm1; p.clip = clip;
  p.coef1 = coef1; p.coef2 = coef2; p.s = s; p.noise = noise;
  p.mask = mask; p.x0_orig = x0_orig; p.q_noise = q_noise; p.sa = sa; p.s1ma = s1ma;
  p.x0_out = x0_out; p.x_prev = x_prev; p.n = n;
  return launch_ddpm_step(p, (hipStream_t)stream);
}


int sdmi_dpm_solver_step(const float* eps_model, int cfg, float scale, const float* x, const float* m_prev, float alpha_s,
                         float sigma_s, float cx, float a, float inv_r0, int order, float* m_out, float* x_next, int64_t n,
                         void* stream) {
  DpmStepParams p = DpmStepParams();
  p.eps_model = eps_model; p.cfg = cfg; p.scale = scale; p.x = x; p.m_prev = m_prev; p.alpha_s = alpha_s; p.sigma_s = sigma_s;
  p.cx = cx; p.a = a; p.inv_r0 = inv_r0; p.order = order; p.m_out = m_out; p.x_next = x_next; p.n = n;
  return launch_dpm_step(p, (hipStream_t)stream);
}

int sdmi_dpm_model_value(const float* eps_model, int cfg, float scale, const float* x, int predict_x0, float alpha_s, float sigma_s,
                         const float* s, int64_t row, float* out, int64_t n, void* stream) {
  DpmModelValueParams p = DpmModelValueParams();
  p.eps_model = eps_model; p.cfg = cfg; p.scale = scale; p.x = x; p.predict_x0 = predict_x0; p.alpha_s = alpha_s; p.sigma_s = sigma_s;
  p.s = s; p.row = row; p.out = out; p.n = n;
  return launch_dpm_model_value(p, (hipStream_t)stream);
}

int sdmi_dpm_update(int form, const float* x, const float* m0, const float* m1, const float* m2, const float* c9, float* out, int64_t n,
                    void* stream) {
  SDMI_CHECK(c9, "dpm_update: null coefficients");
  DpmUpdateParams p = DpmUpdateParams();
  p.form = form; p.x = x; p.m0 = m0; p.m1 = m1; p.m2 = m2; p.out = out; p.n = n;
  for (int i = 0; i < 9; ++i) p.c[i] = c9[i];
  return launch_dpm_update(p, (hipStream_t)stream);
}

int sdmi_dpm_threshold_scale(const float* x0, int B, int64_t row, float max_val, float* s_out, float* stats_out, void* stream) {
  return launch_dpm_threshold_scale(x0, B, row, max_val, s_out, stats_out, (hipStream_t)stream);
}

int64_t sdmi_dpm_adaptive_error_ws_floats(int B, int64_t row) { return B > 0 && row > 0 ? dpm_error_ws_floats(B, row) : -1; }

int sdmi_dpm_adaptive_error(const float* x_higher, const float* x_lower, const float* x_prev, float atol, float rtol, int B, int64_t row,
                            float* ws, int64_t ws_floats, float* E, void* stream) {
  return launch_dpm_adaptive_error(x_higher, x_lower, x_prev, atol, rtol, B, row, ws, ws_floats, E, (hipStream_t)stream);
}

// ---- first stage --------------------------------------------------------------------------------------
int sdmi_vae_create(const sdmi_vae_cfg* cfg, int parts, sdmi_vae** out) {
  return sdmi_vae_create_precision(cfg, nullptr, parts, SDMI_PRECISION_MIXED, out);
}
int sdmi_vae_create_ext(const sdmi_vae_cfg* cfg, const sdmi_vae_ext* ext, int parts, sdmi_vae** out) {
  return sdmi_vae_create_precision(cfg, ext, parts, SDMI_PRECISION_MIXED, out);
}
int sdmi_vae_create_precision(const sdmi_vae_cfg* cfg, const sdmi_vae_ext* ext, int parts, int precision, sdmi_vae** out) {
  return sdmi_vae_create_attn(cfg, ext, parts, precision, 0u, out);
}
int sdmi_vae_create_attn(const sdmi_vae_cfg* cfg, const sdmi_vae_ext* ext, int parts, int precision, uint32_t attn_level_mask,
                         sdmi_vae** out) {
  SDMI_CHECK(cfg && out, "null argument");
  SDMI_CHECK(precision == SDMI_PRECISION_MIXED || precision == SDMI_PRECISION_FULL,
             "precision must be SDMI_PRECISION_MIXED (0) or SDMI_PRECISION_FULL (1), got " + std::to_string(precision));
  sdmi_vae* h = new (std::nothrow) sdmi_vae();
  SDMI_CHECK(h != nullptr, "out of host memory");
  if (h->impl.build(*cfg, parts, ext, precision, attn_level_mask)) { delete h; return -1; }
  *out = h;
  return 0;
}
int sdmi_vae_precision(const sdmi_vae* h) {
  if (!h) { fail("null handle"); return -1; }
  return h->impl.precision_;
}
int sdmi_vae_destroy(sdmi_vae* h) { delete h; return 0; }
int sdmi_vae_num_weights(const sdmi_vae* h) { return h ? (int)h->impl.weights().slots().size() : fail("null handle"); }
int sdmi_vae_weight_info(const sdmi_vae* h, int idx, char* key_buf, int key_buf_len, int64_t* shape4, int* ndim) {
  SDMI_CHECK(h, "null argument");
  return weight_info(h->impl.weights(), idx, key_buf, key_buf_len, shape4, ndim);
}
int sdmi_vae_set_weight(sdmi_vae* h, const char* key, const float* ptr, const int64_t* shape, int ndim, void* stream) {
  SDMI_CHECK(h && key && ptr && shape, "null argument");
  return h->impl.set_weight(key, ptr, shape, ndim, (hipStream_t)stream);
}
int sdmi_vae_finalize(sdmi_vae* h) { SDMI_CHECK(h, "null handle"); return h->impl.finalize(); }
int64_t sdmi_vae_decode_workspace_bytes(sdmi_vae* h, int B, int H, int W) {
  if (!h) { fail("null handle"); return 0; }
  int64_t need = 0;
  if (h->impl.decode(nullptr, 1.f, nullptr, B, H, W, nullptr, 0, nullptr, true, &need)) return 0;
  return need;
}
int sdmi_vae_decode(sdmi_vae* h, const float* z, float z_scale, float* img, int B, int H, int W, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  SDMI_CHECK(h && z && img, "null argument");
  return h->impl.decode(z, z_scale, img, B, H, W, workspace, workspace_bytes, (hipStream_t)stream, false, nullptr);
}
int sdmi_vae_decode_vq(sdmi_vae* h, const float* z, float z_scale, int quantize, float* img, int B, int H, int W, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  SDMI_CHECK(h && z && img, "null argument");
  return h->impl.decode(z, z_scale, img, B, H, W, workspace, workspace_bytes, (hipStream_t)stream, false, nullptr, quantize != 0);
}
int64_t sdmi_vae_encode_workspace_bytes(sdmi_vae* h, int B, int H, int W) {
  if (!h) { fail("null handle"); return 0; }
  int64_t need = 0;
  if (h->impl.encode(nullptr, nullptr, B, H, W, nullptr, 0, nullptr, true, &need)) return 0;
  return need;
}
int sdmi_vae_encode(sdmi_vae* h, const float* img, float* moments, int B, int H, int W, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  SDMI_CHECK(h && img && moments, "null argument");
  return h->impl.encode(img, moments, B, H, W, workspace, workspace_bytes, (hipStream_t)stream, false, nullptr);
}
int sdmi_k_pointwise_nchw(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int HW,
                          float in_scale, void* stream) {
  SDMI_CHECK(Cin <= 32, "pointwise conv: 1 <= Cin <= 32");       // (the limit this entry was published with; sdmi_k_pointwise_nchw128 is the wider one)
  return launch_pointwise_nchw(x, w, bias, out, B, Cin, Cout, HW, in_scale, (hipStream_t)stream);
}
int sdmi_k_pointwise_nchw128(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int HW,
                             float in_scale, void* stream) {
  return launch_pointwise_nchw(x, w, bias, out, B, Cin, Cout, HW, in_scale, (hipStream_t)stream);
}
int sdmi_k_softmax_rows(const float* S, void* P_f16, int rows, int cols, float scale, void* stream) {
  return launch_softmax_rows(S, (f16*)P_f16, rows, cols, cols, cols, scale, (hipStream_t)stream);
}


// ---- text encoder -------------------------------------------------------------------------------------
int sdmi_clip_create(const sdmi_clip_cfg* cfg, sdmi_clip** out) { return sdmi_clip_create_precision(cfg, SDMI_PRECISION_MIXED, out); }
int sdmi_clip_create_precision(const sdmi_clip_cfg* cfg, int precision, sdmi_clip** out) {
  SDMI_CHECK(cfg && out, "null argument");
  SDMI_CHECK(precision == SDMI_PRECISION_MIXED || precision == SDMI_PRECISION_FULL,
             "precision must be SDMI_PRECISION_MIXED (0) or SDMI_PRECISION_FULL (1), got " + std::to_string(precision));
  sdmi_clip* h = new (std::nothrow) sdmi_clip();
  SDMI_CHECK(h != nullptr, "out of host memory");
  if (h->impl.build(*cfg, precision)) { delete h; return -1; }
  *out = h;
  return 0;
}
int sdmi_clip_precision(const sdmi_clip* h) {
  if (!h) { fail("null handle"); return -1; }
  return h->impl.precision_;
}
int sdmi_clip_destroy(sdmi_clip* h) { delete h; return 0; }
int sdmi_clip_num_weights(const sdmi_clip* h) { return h ? (int)h->impl.weights().slots().size() : fail("null handle"); }
int sdmi_clip_weight_info(const sdmi_clip* h, int idx, char* key_buf, int key_buf_len, int64_t* shape4, int* ndim) {
  SDMI_CHECK(h, "null argument");
  return weight_info(h->impl.weights(), idx, key_buf, key_buf_len, shape4, ndim);
}
int sdmi_clip_set_weight(sdmi_clip* h, const char* key, const float* ptr, const int64_t* shape, int ndim, void* stream) {
  SDMI_CHECK(h && key && ptr && shape, "null argument");
  return h->impl.set_weight(key, ptr, shape, ndim, (hipStream_t)stream);
}
int sdmi_clip_finalize(sdmi_clip* h) { SDMI_CHECK(h, "null handle"); return h->impl.finalize(); }
int64_t sdmi_clip_workspace_bytes(sdmi_clip* h, int B, int L) {
  if (!h) { fail("null handle"); return 0; }
  int64_t need = 0;
  if (h->impl.forward(nullptr, nullptr, B, L, nullptr, 0, nullptr, true, &need)) return 0;
  return need;
}
int sdmi_clip_create_projection(const sdmi_clip_cfg* cfg, int projection_dim, int precision, sdmi_clip** out) {
  SDMI_CHECK(cfg && out, "null argument");
  SDMI_CHECK(precision == SDMI_PRECISION_MIXED || precision == SDMI_PRECISION_FULL,
             "precision must be SDMI_PRECISION_MIXED (0) or SDMI_PRECISION_FULL (1), got " + std::to_string(precision));
  SDMI_CHECK(projection_dim >= 1, "projection_dim must be positive, got " + std::to_string(projection_dim));
  sdmi_clip* h = new (std::nothrow) sdmi_clip();
  SDMI_CHECK(h != nullptr, "out of host memory");
  if (h->impl.build(*cfg, precision, projection_dim)) { delete h; return -1; }
  *out = h;
  return 0;
}
int sdmi_clip_projection_dim(const sdmi_clip* h) {
  if (!h) { fail("null handle"); return -1; }
  return h->impl.proj_dim_;
}
int64_t sdmi_clip_text_embeds_workspace_bytes(sdmi_clip* h, int B, int L) {
  if (!h) { fail("null handle"); return 0; }
  int64_t need = 0;
  if (h->impl.text_embeds(nullptr, nullptr, B, L, 0, nullptr, 0, nullptr, true, &need)) return 0;
  return need;
}
int sdmi_clip_text_embeds(sdmi_clip* h, const int64_t* ids, float* out, int B, int L, int normalize, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  SDMI_CHECK(h && ids && out, "null argument");
  return h->impl.text_embeds(ids, out, B, L, normalize, workspace, workspace_bytes, (hipStream_t)stream, false, nullptr);
}
int sdmi_clip_forward(sdmi_clip* h, const int64_t* ids, float* out, int B, int L, void* workspace, int64_t workspace_bytes,
                      void* stream) {
  SDMI_CHECK(h && ids && out, "null argument");
  return h->impl.forward(ids, out, B, L, workspace, workspace_bytes, (hipStream_t)stream, false, nullptr);
}

// ---- text encoder of the LAION-400M model ----------------------------------------------------------------------------
int sdmi_bert_create(const sdmi_bert_cfg* cfg, sdmi_bert** out) { return sdmi_bert_create_precision(cfg, SDMI_PRECISION_MIXED, out); }
int sdmi_bert_create_precision(const sdmi_bert_cfg* cfg, int precision, sdmi_bert** out) {
  SDMI_CHECK(cfg && out, "null argument");
  SDMI_CHECK(precision == SDMI_PRECISION_MIXED || precision == SDMI_PRECISION_FULL,
             "precision must be SDMI_PRECISION_MIXED (0) or SDMI_PRECISION_FULL (1), got " + std::to_string(precision));
  sdmi_bert* h = new (std::nothrow) sdmi_bert();
  SDMI_CHECK(h != nullptr, "out of host memory");
  if (h->impl.build(*cfg, precision)) { delete h; return -1; }
  *out = h;
  return 0;
}
int sdmi_bert_precision(const sdmi_bert* h) {
  if (!h) { fail("null handle"); return -1; }
  return h->impl.precision_;
}
int sdmi_bert_destroy(sdmi_bert* h) { delete h; return 0; }
int sdmi_bert_num_weights(const sdmi_bert* h) { return h ? (int)h->impl.weights().slots().size() : fail("null handle"); }
int sdmi_bert_weight_info(const sdmi_bert* h, int idx, char* key_buf, int key_buf_len, int64_t* shape4, int* ndim) {
  SDMI_CHECK(h, "null argument");
  return weight_info(h->impl.weights(), idx, key_buf, key_buf_len, shape4, ndim);
}
int sdmi_bert_set_weight(sdmi_bert* h, const char* key, const float* ptr, const int64_t* shape, int ndim, void* stream) {
  SDMI_CHECK(h && key && ptr && shape, "null argument");
  return h->impl.set_weight(key, ptr, shape, ndim, (hipStream_t)stream);
}
int sdmi_bert_finalize(sdmi_bert* h) { SDMI_CHECK(h, "null handle"); return h->impl.finalize(); }
int64_t sdmi_bert_workspace_bytes(sdmi_bert* h, int B, int L) {
  if (!h) { fail("null handle"); return 0; }
  int64_t need = 0;
  if (h->impl.forward(nullptr, nullptr, B, L, nullptr, 0, nullptr, true, &need)) return 0;
  return need;
}
int sdmi_bert_forward(sdmi_bert* h, const int64_t* ids, float* out, int B, int L, void* workspace, int64_t workspace_bytes,
                      void* stream) {
  SDMI_CHECK(h && ids && out, "null argument");
  return h->impl.forward(ids, out, B, L, workspace, workspace_bytes, (hipStream_t)stream, false, nullptr);
}

// ---- CLIP image encoder ------------------------------------------------------------------------------------------------
int sdmi_vit_create(const sdmi_vit_cfg* cfg, sdmi_vit** out) {
  SDMI_CHECK(cfg && out, "null argument");
  sdmi_vit* h = new (std::nothrow) sdmi_vit();
  SDMI_CHECK(h != nullptr, "out of host memory");
  if (h->impl.build(*cfg)) { delete h; return -1; }
  *out = h;
  return 0;
}
int sdmi_vit_destroy(sdmi_vit* h) { delete h; return 0; }
int sdmi_vit_num_weights(const sdmi_vit* h) { return h ? (int)h->impl.weights().slots().size() : fail("null handle"); }
int sdmi_vit_weight_info(const sdmi_vit* h, int idx, char* key_buf, int key_buf_len, int64_t* shape4, int* ndim) {
  SDMI_CHECK(h, "null argument");
  return weight_info(h->impl.weights(), idx, key_buf, key_buf_len, shape4, ndim);
}
int sdmi_vit_set_weight(sdmi_vit* h, const char* key, const float* ptr, const int64_t* shape, int ndim, void* stream) {
  SDMI_CHECK(h && key && ptr && shape, "null argument");
  return h->impl.set_weight(key, ptr, shape, ndim, (hipStream_t)stream);
}
int sdmi_vit_finalize(sdmi_vit* h) { SDMI_CHECK(h, "null handle"); return h->impl.finalize(); }
int64_t sdmi_vit_workspace_bytes(sdmi_vit* h, int B) {
  if (!h) { fail("null handle"); return 0; }
  int64_t need = 0;
  if (h->impl.forward(nullptr, nullptr, nullptr, nullptr, B, nullptr, 0, nullptr, true, &need)) return 0;
  return need;
}
int sdmi_vit_forward(sdmi_vit* h, const float* pixel_values, float* last_hidden_or_null, float* pooled_or_null, float* image_embeds, int B,
                     void* workspace, int64_t workspace_bytes, void* stream) {
  SDMI_CHECK(h && pixel_values && image_embeds, "null argument");
  return h->impl.forward(pixel_values, last_hidden_or_null, pooled_or_null, image_embeds, B, workspace, workspace_bytes, (hipStream_t)stream,
                         false, nullptr);
}
int sdmi_k_vit_kpad(int patch_size) {
  if (patch_size < 1 || patch_size > 64) { fail("patch_size outside 1..64"); return -1; }
  return vit_kpad(patch_size);
}
int sdmi_k_vit_patchify(const float* pixel_values, void* out_f16, int B, int S, int p, void* stream) {
  return launch_vit_patchify(pixel_values, (f16*)out_f16, B, S, p, (hipStream_t)stream);
}
int sdmi_k_vit_embed(const float* patch, const float* class_embedding, const float* position_embedding, float* out, int B, int T, int C,
                     void* stream) {
  return launch_vit_embed(patch, class_embedding, position_embedding, out, B, T, C, (hipStream_t)stream);
}
int sdmi_k_vit_preprocess(const float* x, float* out, int B, int H, int W, int S, void* stream) {
  return launch_vit_preprocess(x, out, B, H, W, S, (hipStream_t)stream);
}
int sdmi_k_safety_head(const float* image_embeds, const float* concept_embeds, const float* special_care_embeds,
                       const float* concept_thresholds, const float* special_care_thresholds, int32_t* has_nsfw, float* concept_scores,
                       float* special_care_scores, int B, int Nc, int Ns, int E, void* stream) {
  return launch_safety_head(image_embeds, concept_embeds, special_care_embeds, concept_thresholds, special_care_thresholds, (int*)has_nsfw,
                            concept_scores, special_care_scores, B, Nc, Ns, E, (hipStream_t)stream);
}
// ---- the safety checker's feature extractor ------------------------------------------------------------------------------
int sdmi_fe_ksize(int in, int out) {
  if (in < 1 || out < 1) { fail("fe_ksize: sizes below 1"); return -1; }
  return fe_ksize(in, out);
}
int sdmi_fe_coeffs(int in, int out, int32_t* bounds, int32_t* kk) {
  SDMI_CHECK(in >= 1 && out >= 1, "fe_coeffs: sizes below 1");
  SDMI_CHECK(bounds && kk, "fe_coeffs: null table");
  return fe_coeffs(in, out, bounds, kk);
}
int sdmi_fe_output_size(int H, int W, int size, int* rh, int* rw) {
  SDMI_CHECK(H >= 1 && W >= 1 && size >= 1 && rh && rw, "fe_output_size: sizes below 1, or a null output");
  SDMI_CHECK((int64_t)size * std::max(H, W) / std::min(H, W) <= 0x7fffffff, "fe_output_size: the resized side does not fit an int");
  fe_output_size(H, W, size, rh, rw);
  return 0;
}
int64_t sdmi_fe_workspace_bytes(int B, int H, int W, int size, int crop) { return fe_workspace_bytes(B, H, W, size, crop); }
int sdmi_k_clip_feature_extract(const void* src, int src_kind, int B, int C, int H, int W, int size, int crop, const int32_t* h_bounds,
                                const int32_t* h_kk, int h_ksize, const int32_t* v_bounds, const int32_t* v_kk, int v_ksize,
                                const float* mean3, const float* std3, void* workspace, int64_t workspace_bytes, float* pixel_values,
                                void* out_u8_or_null, void* stream) {
  SDMI_CHECK(C == 3, "feature_extract: a channel count other than 3 (RGB images only), got " + std::to_string(C));
  SDMI_CHECK(mean3 && std3, "feature_extract: null mean or std");
  FeParams p;
  p.src = src; p.kind = src_kind; p.B = B; p.H = H; p.W = W; p.size = size; p.crop = crop;
  p.hb = h_bounds; p.hk = h_kk; p.h_ksize = h_ksize; p.vb = v_bounds; p.vk = v_kk; p.v_ksize = v_ksize;
  for (int c = 0; c < 3; ++c) { p.mean[c] = mean3[c]; p.std[c] = std3[c]; }
  p.ws = workspace; p.ws_bytes = workspace_bytes; p.pixel_values = pixel_values; p.out_u8 = (unsigned char*)out_u8_or_null;
  return launch_feature_extract(p, (hipStream_t)stream);
}
// ---- exact k-NN search -----------------------------------------------------------------------------------------------
int sdmi_knn_create(int D, int64_t capacity_rows, sdmi_knn** out) {
  SDMI_CHECK(out, "null argument");
  sdmi_knn* h = new (std::nothrow) sdmi_knn();
  SDMI_CHECK(h != nullptr, "out of host memory");
  if (h->impl.build(D, capacity_rows)) { delete h; return -1; }
  *out = h;
  return 0;
}
int sdmi_knn_destroy(sdmi_knn* h) { delete h; return 0; }
int sdmi_knn_set_rows(sdmi_knn* h, int64_t first_row, int64_t n, const float* rows, void* stream) {
  SDMI_CHECK(h && rows, "null argument");
  return h->impl.set_rows(first_row, n, rows, (hipStream_t)stream);
}
int sdmi_knn_finalize(sdmi_knn* h, void* stream) { SDMI_CHECK(h, "null handle"); return h->impl.finalize((hipStream_t)stream); }
int64_t sdmi_knn_rows(const sdmi_knn* h) {
  if (!h) { fail("null handle"); return -1; }
  return h->impl.n_;
}
int sdmi_knn_dim(const sdmi_knn* h) { return h ? h->impl.D_ : fail("null handle"); }
int64_t sdmi_knn_workspace_bytes(sdmi_knn* h, int B, int k) {
  if (!h) { fail("null handle"); return 0; }
  if (knn_check_args(h->impl.n_, h->impl.D_, B, k)) return 0;
  return h->impl.workspace_bytes(B, k);
}
int sdmi_knn_search(sdmi_knn* h, const float* queries, int B, int k, int32_t* idx_out, float* score_out, float* nn_out_or_null,
                    void* workspace, int64_t workspace_bytes, void* stream) {
  SDMI_CHECK(h, "null handle");
  return h->impl.search(queries, B, k, (int*)idx_out, score_out, nn_out_or_null, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}
int sdmi_knn_condition(sdmi_knn* h, const float* c, int B, int k, float* c_out, int32_t* idx_out, float* score_out, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  SDMI_CHECK(h && c && c_out, "null argument");
  return h->impl.search(c, B, k, (int*)idx_out, score_out, c_out, c, workspace, workspace_bytes, (hipStream_t)stream);
}
int sdmi_k_knn_inv_norm(const float* db, int64_t N, int D, float* inv_norm, void* stream) {
  return launch_knn_inv_norm(db, N, D, inv_norm, (hipStream_t)stream);
}
int sdmi_k_knn_scan(const float* db, const float* inv_norm, int64_t N, int D, const float* queries, int B, int k, int64_t slab_rows,
                    float* cand_score, int32_t* cand_idx, void* stream) {
  return launch_knn_scan(db, inv_norm, N, D, queries, B, k, slab_rows, cand_score, (int*)cand_idx, (hipStream_t)stream);
}
int sdmi_k_knn_merge(const float* cand_score, const int32_t* cand_idx, int B, int n_lists, int k, int32_t* idx_out, float* score_out,
                     void* stream) {
  return launch_knn_merge(cand_score, (const int*)cand_idx, B, n_lists, k, (int*)idx_out, score_out, (hipStream_t)stream);
}
int sdmi_k_knn_stream_read(const float* p, int64_t n_floats, float* sink, void* stream) {
  return launch_knn_stream_read(p, n_floats, sink, (hipStream_t)stream);
}
int sdmi_k_knn_gather(const float* db, const float* inv_norm, int64_t N, int D, const int32_t* idx, int B, int k, const float* c0_or_null,
                      float* out, int64_t ldo, void* stream) {
  return launch_knn_gather(db, inv_norm, N, D, (const int*)idx, B, k, c0_or_null, out, ldo, (hipStream_t)stream);
}
int sdmi_k_vq_quantize(const float* z, float z_scale, const float* codebook, float* norms_ws, int n_embed, int D, float* zq, int32_t* idx,
                       int B, int HW, void* stream) {
  if (launch_vq_norms(codebook, norms_ws, n_embed, D, (hipStream_t)stream)) return -1;
  return launch_vq_quantize(z, z_scale, codebook, norms_ws, n_embed, D, zq, (int*)idx, B, HW, (hipStream_t)stream);
}
int sdmi_k_resample2(const float* x, float* out_f32, void* out_f16, void* out_lo, int B, int H, int W, int C, int dir, void* stream) {
  return launch_resample2(x, out_f32, (f16*)out_f16, (f16*)out_lo, B, H, W, C, dir, (hipStream_t)stream);
}
int sdmi_k_patch_unfold(const float* x, const float* c, float* out, int B, int Cx, int Cc, int H, int W, int kh, int kw, int sy, int sx,
                        int l0, int nl, void* stream) {
  return launch_patch_unfold(x, c, out, B, Cx, Cc, H, W, kh, kw, sy, sx, l0, nl, (hipStream_t)stream);
}
int sdmi_k_patch_fold(const float* o, const float* w, float* out, int B, int C, int H, int W, int kh, int kw, int sy, int sx, int uf, int df,
                      int norm_only, void* stream) {
  return launch_patch_fold(o, w, out, B, C, H, W, kh, kw, sy, sx, uf, df, norm_only, (hipStream_t)stream);
}
int sdmi_k_spatial_rescale(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int H, int W, int n_stages,
                           int Cout, void* stream) {
  return launch_spatial_rescale(x, w, bias, out, B, Cin, H, W, n_stages, Cout, (hipStream_t)stream);
}
int sdmi_k_spatial_rescale_labels(const int32_t* labels, const float* w, const float* bias, float* out, int B, int Cin, int H, int W,
                                  int n_stages, int Cout, void* stream) {
  return launch_spatial_rescale_labels((const int*)labels, w, bias, out, B, Cin, H, W, n_stages, Cout, (hipStream_t)stream);
}
int sdmi_k_gelu_erf(const float* x, void* out_f16, int64_t n, void* stream) {
  return launch_gelu_erf(x, (f16*)out_f16, n, (hipStream_t)stream);
}
int sdmi_k_quick_gelu(const float* x, void* out_f16, int64_t n, void* stream) {
  return launch_quick_gelu(x, (f16*)out_f16, n, (hipStream_t)stream);
}
int sdmi_k_quick_gelu_split(const float* x, void* out, void* out_lo, int64_t n, void* stream) {
  return launch_quick_gelu_split(x, (f16*)out, (f16*)out_lo, n, (hipStream_t)stream);
}
int sdmi_k_gelu_erf_split(const float* x, void* out, void* out_lo, int64_t n, void* stream) {
  return launch_gelu_erf_split(x, (f16*)out, (f16*)out_lo, n, (hipStream_t)stream);
}
int sdmi_k_attention_split16_causal(const void* q, const void* q_lo, const void* k, const void* k_lo, const void* vt, const void* vt_lo,
                                    void* out, void* out_lo, int BH, int heads, int n, int n_pad, int d, float scale, void* stream) {
  AttnSplitParams p = AttnSplitParams();
  p.q = (const f16*)q; p.q_lo = (const f16*)q_lo; p.k = (const f16*)k; p.k_lo = (const f16*)k_lo;
  p.vt = (const f16*)vt; p.vt_lo = (const f16*)vt_lo; p.out = (f16*)out; p.out_lo = (f16*)out_lo;
  p.BH = BH; p.heads = heads; p.nq = n; p.nkv = n; p.nkv_pad = n_pad; p.d = d; p.scale = scale; p.causal = 1;
  return launch_attention_split16(p, (hipStream_t)stream);
}
int sdmi_k_attention_causal(const void* q, const void* k, const void* vt, void* out, int BH, int heads, int n, int n_pad,
                            int d, float scale, void* stream) {
  AttnParams a = AttnParams();
  a.q = (const f16*)q; a.k = (const f16*)k; a.vt = (const f16*)vt; a.out = (f16*)out;
  a.BH = BH; a.heads = heads; a.nq = n; a.nkv = n; a.nkv_pad = n_pad; a.d = d; a.scale = scale; a.causal = 1;
  return launch_attention(a, (hipStream_t)stream);
}

// ---- kernel-level entry points ------------------------------------------------------------------------
static int igemm_params_of(const sdmi_igemm_desc* d, IGemmParams& p) {
  p.a0 = (const f16*)d->a0; p.a1 = (const f16*)d->a1; p.a2 = (const f16*)d->a2;
  p.c0 = d->c0; p.c1 = d->c1; p.c2 = d->c2; p.lda0 = d->lda0; p.lda1 = d->lda1; p.lda2 = d->lda2;
  p.B = d->B; p.Hin = d->Hin; p.Win = d->Win; p.Hout = d->Hout; p.Wout = d->Wout;
  p.ksize = d->ksize; p.stride = d->stride; p.up = d->up; p.pad = d->asym_pad ? 0 : 1;
  p.w = (const f16*)d->w; p.M = d->B * d->Hout * d->Wout; p.N = d->N; p.K = d->ksize * d->ksize * (d->c0 + d->c1 + d->c2);
  p.mode = d->mode; p.bias = d->bias; p.rowvec = d->rowvec; p.ld_rowvec = d->ld_rowvec;
  p.residual = d->residual; p.ldr = d->ldr; p.out_f32 = d->out_f32; p.out_f16 = (f16*)d->out_f16; p.ldo = d->ldo;
  for (int i = 0; i < 3; ++i) { p.seg_dst[i] = (f16*)d->seg_dst[i]; p.seg_kind[i] = d->seg_kind[i]; }
  p.heads = d->heads; p.dh = d->dh; p.ntok = d->ntok; p.ntok_pad = d->ntok_pad; p.segC = d->segC;
  p.splitk = d->splitk; p.splitk_ws = d->splitk_ws; p.splitk_ws_floats = d->splitk_ws_floats;
  p.splitk_cnt = d->splitk_cnt; p.splitk_cnt_ints = d->splitk_cnt_ints;
  p.gn_n = d->gn_n;
  for (int i = 0; i < 2; ++i) { p.gn_acc[i] = (long long*)d->gn_acc[i]; p.gn_cpg[i] = d->gn_cpg[i]; p.gn_cbase[i] = d->gn_cbase[i]; }
  if (d->split16) {                      // a0 = hi, a1 = lo (not a channel concat), w = packed [N][3K]
    p.split16 = 1; p.c1 = 0; p.K = d->c0; p.ldw = 3 * d->c0;
  }
  p.f16_scale = d->f16_scale; p.lnp_out = d->lnp_out;
  p.lnf_part = d->lnf_part; p.lnf_npart = d->lnf_npart; p.lnf_eps = d->lnf_eps; p.lnf_cs = d->lnf_cs; p.lnf_d = d->lnf_d;
  p.pgn_gamma = d->pgn_gamma; p.pgn_beta = d->pgn_beta; p.pgn_eps = d->pgn_eps; p.pgn_silu = d->pgn_silu;
  p.pgn_out = (f16*)d->pgn_out; p.pgn_keep_f32 = d->pgn_keep_f32; p.pgn_applied = d->pgn_applied;
  p.out_lo = (f16*)d->out_lo;
  return zero_page(&p.zero_page);
}
int sdmi_k_igemm(const sdmi_igemm_desc* d, void* stream) {
  SDMI_CHECK(d, "null descriptor");
  IGemmParams p = IGemmParams();
  if (igemm_params_of(d, p)) return -1;
  IGemmTune t; t.tile = d->tile; t.dma = d->dma;
  return launch_igemm(p, t, (hipStream_t)stream);
}
int sdmi_k_igemm_tail(const sdmi_igemm_desc* d, const void* t0, const void* t1, const void* t2, int tail_c, int tail_ld, const void* tail_w,
                      int tail_kt, void* stream) {
  SDMI_CHECK(d, "null descriptor");
  IGemmParams p = IGemmParams();
  if (igemm_params_of(d, p)) return -1;
  p.tail_a0 = (const f16*)t0; p.tail_a1 = (const f16*)t1; p.tail_a2 = (const f16*)t2;
  p.tail_c = tail_c; p.tail_ld = tail_ld; p.tail_w = (const f16*)tail_w; p.tail_kt = tail_kt;
  IGemmTune t; t.tile = d->tile; t.dma = d->dma;
  return launch_igemm(p, t, (hipStream_t)stream);
}
int sdmi_k_igemm_up_phase(const sdmi_igemm_desc* d, void* stream) {
  SDMI_CHECK(d, "null descriptor");
  IGemmParams p = IGemmParams();
  if (igemm_params_of(d, p)) return -1;
  SDMI_CHECK(p.ksize == 3 && p.up == 1 && p.stride == 1 && p.Hout == 2 * p.Hin && p.Wout == 2 * p.Win && p.c1 == 0 && p.c2 == 0 && !p.split16,
             "up_phase: the descriptor is the reference op, a 3x3 stride-1 conv of one nearest-x2 upsampled source (Hout = 2 Hin, Wout = 2 Win)");
  IGemmParams q = up_phase_of(p, p.w);
  q.splitk = d->splitk;
  IGemmTune t; t.tile = d->tile; t.dma = d->dma;
  return launch_igemm(q, t, (hipStream_t)stream);
}
int sdmi_k_up_phase_weights(const void* w_packed, void* dst, int N, int Cin, void* stream) {
  return launch_up_phase_weights((const f16*)w_packed, (f16*)dst, N, Cin, (hipStream_t)stream);
}
int sdmi_k_tail_split_range(int nkt, int nsplit, int split, int* begin, int* end) {
  SDMI_CHECK(begin && end && nkt >= 0 && nsplit >= 1 && split >= 0 && split < nsplit, "bad arguments");
  tail_split_range(nkt, nsplit, split, begin, end);
  return 0;
}
int sdmi_tune_lookup(int M, int N, int K, int ksize, int stride, int up, int mode, int splitk_req, int kt, int* tile, int* splitk) {
  SDMI_CHECK(tile && splitk, "null argument");
  return tune_lookup(M, N, K, ksize, stride, up, mode, splitk_req, kt, tile, splitk);
}
int sdmi_unet_skip_fold_plan(sdmi_unet* h, int B, int H, int W, int Lctx, int32_t* folded, int cap) {
  SDMI_CHECK(h && (folded || cap == 0), "null argument");
  int64_t need = 0;
  if (h->impl.run(nullptr, nullptr, nullptr, nullptr, nullptr, B, H, W, Lctx, nullptr, 0, nullptr, true, false, &need)) return -1;
  const std::vector<int>& plan = h->impl.skip_fold_plan_;
  for (int i = 0; i < (int)plan.size() && i < cap; ++i) folded[i] = plan[i];
  return (int)plan.size();
}
int sdmi_k_ff_tail(const sdmi_igemm_desc* proj_out, const void* ln_f16, const float* lnp, float ln_eps, const float* csd,
                   const void* wgg_f16, const void* wff2_f16, const float* bff2, const float* t, void* stream) {
  SDMI_CHECK(proj_out, "null descriptor");
  FfTailParams q = FfTailParams();
  if (igemm_params_of(proj_out, q.epi)) return -1;
  SDMI_CHECK(proj_out->split16 && proj_out->ksize == 1, "ff_tail: the proj_out descriptor is a split-fp16 1x1 (w = sdmi_k_pack_split3)");
  q.ln = (const f16*)ln_f16; q.lnp = lnp; q.ln_eps = ln_eps; q.csd = csd; q.wgg = (const f16*)wgg_f16; q.wff2 = (const f16*)wff2_f16;
  q.bff2 = bff2; q.t = t; q.wpo = (const f16*)proj_out->w;
  return launch_ff_tail(q, (hipStream_t)stream);
}
int sdmi_k_st_tail(const sdmi_igemm_desc* proj_out, const void* a_f16, const void* wo_f16, const float* bo, float* t, const float* ln_gamma,
                   float ln_eps, const float* csd, const void* wgg_f16, const void* wff2_f16, const float* bff2, void* stream) {
  SDMI_CHECK(proj_out && a_f16, "null argument");
  FfTailParams q = FfTailParams();
  if (igemm_params_of(proj_out, q.epi)) return -1;
  SDMI_CHECK(proj_out->split16 && proj_out->ksize == 1, "st_tail: the proj_out descriptor is a split-fp16 1x1 (w = sdmi_k_pack_split3)");
  q.a16 = (const f16*)a_f16; q.wo = (const f16*)wo_f16; q.bo = bo; q.ln_gamma = ln_gamma; q.ln_eps = ln_eps; q.csd = csd;
  q.wgg = (const f16*)wgg_f16; q.wff2 = (const f16*)wff2_f16; q.bff2 = bff2; q.t = t; q.wpo = (const f16*)proj_out->w;
  return launch_ff_tail(q, (hipStream_t)stream);
}
int sdmi_k_gn_conv3(const sdmi_igemm_desc* conv, const float* x0, const float* x1, int c0, int c1, float* gn_ws, int64_t gn_ws_floats,
                    const float* gn_gamma, const float* gn_beta, float gn_eps, void* stream) {
  SDMI_CHECK(conv && x0 && gn_ws && gn_gamma && gn_beta, "gn_conv3: null argument");
  GnConvParams q = GnConvParams();
  if (igemm_params_of(conv, q.epi)) return -1;
  const int B = q.epi.B;
  SDMI_CHECK(gn_ws_floats >= gn_acc_words(B) * 2, "groupnorm workspace too small");
  SDMI_HIP_OK(hipMemsetAsync(gn_ws, 0, gn_acc_words(B) * sizeof(long long), (hipStream_t)stream));
  GroupNormParams g = GroupNormParams();
  g.x0 = x0; g.c0 = c0; g.x1 = x1; g.c1 = c1; g.B = B; g.HW = q.epi.Hout * q.epi.Wout; g.gamma = gn_gamma; g.beta = gn_beta; g.eps = gn_eps;
  g.stats_only = 1; g.acc = (long long*)gn_ws;
  if (launch_groupnorm(g, (hipStream_t)stream)) return -1;
  q.x0 = x0; q.x1 = x1; q.c0 = c0; q.c1 = c1; q.gn_acc = (const long long*)gn_ws; q.gn_gamma = gn_gamma; q.gn_beta = gn_beta; q.gn_eps = gn_eps;
  q.w = (const f16*)conv->w;
  return launch_gn_conv3(q, (hipStream_t)stream);
}
int sdmi_k_st_head(const float* x, float* gn_ws, int64_t gn_ws_floats, const float* gn_gamma, const float* gn_beta, float gn_eps,
                   const void* w_in3, const float* b_in, float* t, const float* ln_gamma, float ln_eps, const void* wqkv_f16,
                   const float* lnf_cs, const float* lnf_d, void* q, void* k, void* vt, int B, int ntok, int ntok_pad, int heads, int dh,
                   int C, void* stream) {
  SDMI_CHECK(x && gn_ws && gn_gamma && gn_beta, "st_head: null argument");
  SDMI_CHECK(gn_ws_floats >= gn_acc_words(B) * 2, "groupnorm workspace too small");
  SDMI_HIP_OK(hipMemsetAsync(gn_ws, 0, gn_acc_words(B) * sizeof(long long), (hipStream_t)stream));
  GroupNormParams g = GroupNormParams();
  g.x0 = x; g.c0 = C; g.B = B; g.HW = ntok; g.gamma = gn_gamma; g.beta = gn_beta; g.eps = gn_eps; g.stats_only = 1; g.acc = (long long*)gn_ws;
  if (launch_groupnorm(g, (hipStream_t)stream)) return -1;
  StHeadParams p = StHeadParams();
  p.x = x; p.gn_acc = (const long long*)gn_ws; p.gn_gamma = gn_gamma; p.gn_beta = gn_beta; p.gn_eps = gn_eps;
  p.w_in = (const f16*)w_in3; p.b_in = b_in; p.t = t; p.ln_gamma = ln_gamma; p.ln_eps = ln_eps; p.wqkv = (const f16*)wqkv_f16;
  p.lnf_cs = lnf_cs; p.lnf_d = lnf_d; p.q = (f16*)q; p.k = (f16*)k; p.vt = (f16*)vt;
  p.M = B * ntok; p.B = B; p.ntok = ntok; p.ntok_pad = ntok_pad; p.heads = heads; p.dh = dh; p.C = C;
  return launch_st_head(p, (hipStream_t)stream);
}
int sdmi_k_st_mid(const void* a_f16, const void* wo_f16, const float* bo, float* t, const float* ln_gamma, float ln_eps, const void* wq_f16,
                  const float* lnf_cs, const float* lnf_d, void* q, int B, int ntok, int heads, int dh, int C, void* stream) {
  StHeadParams p = StHeadParams();
  p.a16 = (const f16*)a_f16; p.w_in = (const f16*)wo_f16; p.b_in = bo; p.t = t; p.ln_gamma = ln_gamma; p.ln_eps = ln_eps;
  p.wqkv = (const f16*)wq_f16; p.lnf_cs = lnf_cs; p.lnf_d = lnf_d; p.q = (f16*)q;
  p.M = B * ntok; p.B = B; p.ntok = ntok; p.ntok_pad = ntok; p.heads = heads; p.dh = dh; p.C = C;
  return launch_st_mid(p, (hipStream_t)stream);
}
int sdmi_k_st_mid_ctx(const void* a_f16, const void* wo_f16, const float* bo, float* t, const float* ln_gamma, float ln_eps, const void* wq_f16,
                      const float* lnf_cs, const float* lnf_d, const void* ctx_k, const void* ctx_vt, int nkv, int nkv_pad, float scale, void* ao_out,
                      int B, int ntok, int heads, int dh, int C, void* stream) {
  StHeadParams p = StHeadParams();
  p.a16 = (const f16*)a_f16; p.w_in = (const f16*)wo_f16; p.b_in = bo; p.t = t; p.ln_gamma = ln_gamma; p.ln_eps = ln_eps;
  p.wqkv = (const f16*)wq_f16; p.lnf_cs = lnf_cs; p.lnf_d = lnf_d;
  p.ctx_k = (const f16*)ctx_k; p.ctx_vt = (const f16*)ctx_vt; p.ctx_nkv = nkv; p.ctx_nkv_pad = nkv_pad; p.ctx_scale = scale; p.ao_out = (f16*)ao_out;
  SDMI_CHECK(ctx_k && ctx_vt && ao_out, "st_mid_ctx: null argument");
  p.M = B * ntok; p.B = B; p.ntok = ntok; p.ntok_pad = ntok; p.heads = heads; p.dh = dh; p.C = C;
  return launch_st_mid(p, (hipStream_t)stream);
}
int sdmi_k_ln_fold_prep(const void* w_f16, int N, int K, int ldw, const float* gamma, const float* beta, const float* bias,
                        float* cs, float* d, void* stream) {
  return launch_ln_fold_prep((const f16*)w_f16, N, K, ldw, gamma, beta, bias, cs, d, (hipStream_t)stream);
}
int sdmi_k_attention(const void* q, const void* k, const void* vt, void* out, int BH, int heads, int nq, int nkv,
                     int nkv_pad, int d, float scale, void* stream) {
  AttnParams a = AttnParams();
  a.q = (const f16*)q; a.k = (const f16*)k; a.vt = (const f16*)vt; a.out = (f16*)out;
  a.BH = BH; a.heads = heads; a.nq = nq; a.nkv = nkv; a.nkv_pad = nkv_pad; a.d = d; a.scale = scale;
  if (const char* e = getenv("SDMI_ATTN_NW")) a.nw = atoi(e);     // test / tuning knob
  return launch_attention(a, (hipStream_t)stream);
}
int sdmi_attn_small_takes(int d, int nq, int nkv, int causal, int knob) { return attn_small_takes(d, nq, nkv, causal, knob); }
int sdmi_k_attention_split16(const void* q, const void* q_lo, const void* k, const void* k_lo, const void* vt, const void* vt_lo, void* out,
                             void* out_lo, int BH, int heads, int nq, int nkv, int nkv_pad, int d, float scale, void* stream) {
  AttnSplitParams a = AttnSplitParams();
  a.q = (const f16*)q; a.q_lo = (const f16*)q_lo; a.k = (const f16*)k; a.k_lo = (const f16*)k_lo; a.vt = (const f16*)vt;
  a.vt_lo = (const f16*)vt_lo; a.out = (f16*)out; a.out_lo = (f16*)out_lo;
  a.BH = BH; a.heads = heads; a.nq = nq; a.nkv = nkv; a.nkv_pad = nkv_pad; a.d = d; a.scale = scale;
  return launch_attention_split16(a, (hipStream_t)stream);
}
int64_t sdmi_k_groupnorm_ws_floats(int B, int HW) { (void)HW; return gn_acc_words(B) * 2; }   // int64 words, counted in floats
int sdmi_k_groupnorm(const float* x0, const float* x1, int c0, int c1, int B, int HW, const float* gamma,
                     const float* beta, float eps, int silu, void* out_f16, float* out_f32, void* raw_f16, void* out_lo,
                     void* raw_lo, float* partial_ws, int64_t partial_floats, void* stream) {
  SDMI_CHECK(partial_floats >= gn_acc_words(B) * 2, "groupnorm workspace too small");
  // the workspace holds the fixed-point statistics accumulators; they must start at zero
  SDMI_HIP_OK(hipMemsetAsync(partial_ws, 0, gn_acc_words(B) * sizeof(long long), (hipStream_t)stream));
  GroupNormParams g = GroupNormParams();
  g.x0 = x0; g.x1 = x1; g.c0 = c0; g.c1 = c1; g.B = B; g.HW = HW; g.gamma = gamma; g.beta = beta; g.eps = eps;
  g.silu = silu; g.out_f16 = (f16*)out_f16; g.out_f32 = out_f32; g.raw_f16 = (f16*)raw_f16; g.out_lo = (f16*)out_lo; g.raw_lo = (f16*)raw_lo;
  g.acc = (long long*)partial_ws;
  return launch_groupnorm(g, (hipStream_t)stream);
}
int sdmi_k_groupnorm_film(const float* x0, const float* x1, int c0, int c1, int B, int HW, const float* gamma, const float* beta, float eps,
                          int silu, const float* film, int film_ld, void* out_f16, float* out_f32, void* raw_f16, void* out_lo, void* raw_lo,
                          float* partial_ws, int64_t partial_floats, void* stream) {
  SDMI_CHECK(partial_floats >= gn_acc_words(B) * 2, "groupnorm workspace too small");
  SDMI_HIP_OK(hipMemsetAsync(partial_ws, 0, gn_acc_words(B) * sizeof(long long), (hipStream_t)stream));
  GroupNormParams g = GroupNormParams();
  g.x0 = x0; g.x1 = x1; g.c0 = c0; g.c1 = c1; g.B = B; g.HW = HW; g.gamma = gamma; g.beta = beta; g.eps = eps;
  g.silu = silu; g.out_f16 = (f16*)out_f16; g.out_f32 = out_f32; g.raw_f16 = (f16*)raw_f16; g.out_lo = (f16*)out_lo; g.raw_lo = (f16*)raw_lo;
  g.film = film; g.film_ld = film_ld;
  g.acc = (long long*)partial_ws;
  return launch_groupnorm(g, (hipStream_t)stream);
}
int sdmi_k_layernorm(const float* x, const float* gamma, const float* beta, void* out_f16, int M, int C, float eps,
                     void* stream) {
  return launch_layernorm(x, gamma, beta, (f16*)out_f16, M, C, eps, (hipStream_t)stream);
}
int sdmi_k_cast_f16(const float* x, void* out_f16, void* out_lo, int64_t n, void* stream) {
  return launch_cast_f16(x, (f16*)out_f16, (f16*)out_lo, n, (hipStream_t)stream);
}
int sdmi_k_split_heads(const float* src, int ld, int col0, void* dst, void* dst_lo, int kind, int B, int ntok, int ntok_pad, int heads, int dh,
                       void* stream) {
  return launch_split_heads(src, ld, col0, (f16*)dst, (f16*)dst_lo, kind, B, ntok, ntok_pad, heads, dh, (hipStream_t)stream);
}
int sdmi_k_geglu_split(const float* src, int M, int F, void* out, void* out_lo, void* stream) {
  return launch_geglu_split(src, M, F, (f16*)out, (f16*)out_lo, (hipStream_t)stream);
}
int sdmi_k_layernorm_split(const float* x, const float* gamma, const float* beta, void* out, void* out_lo, int M, int C, float eps, void* stream) {
  return launch_layernorm_split(x, gamma, beta, (f16*)out, (f16*)out_lo, M, C, eps, (hipStream_t)stream);
}
int sdmi_k_timestep_embedding(const int64_t* t_i64, const float* t_f32, float* out, int B, int dim, void* stream) {
  return launch_timestep_embedding(t_i64, t_f32, out, B, dim, (hipStream_t)stream);
}
int sdmi_k_small_linear(const float* in, int ld_in, const float* w, const float* bias, float* out, int ld_out, int B,
                        int N, int K, int silu_in, void* stream) {
  return launch_small_linear(in, ld_in, w, bias, out, ld_out, B, N, K, silu_in, (hipStream_t)stream);
}
int sdmi_k_conv_in(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int H, int W, int Cout,
                   void* stream) {
  SDMI_CHECK(Cin <= 16, "conv_in: in_channels <= 16");           // (the limit this entry was published with; sdmi_k_conv_in64 is the wider one)
  return launch_conv_in(x, w, bias, out, B, Cin, H, W, Cout, (hipStream_t)stream);
}
int sdmi_k_conv_out(const float* h, const float* w, const float* bias, float* out, int B, int H, int W, int Cin, int Cout,
                    void* stream) {
  // (this entry keeps the contract it was published with, the UNet output heads': up to 16 outputs; sdmi_k_conv_out32 is the wider one)
  SDMI_CHECK(Cout <= 16, "conv_out: out_channels <= 16 on this entry (sdmi_k_conv_out32 takes up to 32)");
  return launch_conv_out(h, w, bias, out, B, H, W, Cin, Cout, (hipStream_t)stream);
}
int sdmi_k_conv_out32(const float* h, const float* w, const float* bias, float* out, int B, int H, int W, int Cin, int Cout,
                      void* stream) {
  SDMI_CHECK(Cout <= 32, "conv_out: out_channels <= 32, Cin % 4 == 0");     // (sdmi_k_conv_out128 takes up to 128)
  return launch_conv_out(h, w, bias, out, B, H, W, Cin, Cout, (hipStream_t)stream);
}
int sdmi_k_conv_in64(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int H, int W, int Cout,
                     void* stream) {
  return launch_conv_in(x, w, bias, out, B, Cin, H, W, Cout, (hipStream_t)stream);
}
int sdmi_k_conv_out128(const float* h, const float* w, const float* bias, float* out, int B, int H, int W, int Cin, int Cout,
                       void* stream) {
  return launch_conv_out(h, w, bias, out, B, H, W, Cin, Cout, (hipStream_t)stream);
}
int sdmi_k_pack_conv_weight(const float* w, void* dst, int O, int I, int KH, int KW, void* stream) {
  return launch_pack_conv_weight(w, (f16*)dst, O, I, KH, KW, (hipStream_t)stream);
}
int sdmi_k_pack_conv_weight_src(const float* w, void* dst, int O, int I, int KH, int KW, int c0, int c1, int c2, void* stream) {
  return launch_pack_conv_weight_src(w, (f16*)dst, O, I, KH, KW, c0, c1, c2, (hipStream_t)stream);
}
int sdmi_k_pack_conv_out(const float* w, float* dst, int O, int I, void* stream) {
  return launch_pack_conv_out(w, dst, O, I, (hipStream_t)stream);
}
int sdmi_k_pack_split3(const float* w, void* dst, int N, int K, void* stream) {
  return launch_pack_split3(w, (f16*)dst, N, K, (hipStream_t)stream);
}
int sdmi_k_pack_conv_split3(const float* w, void* dst, int O, int I, int KH, int KW, void* stream) {
  return launch_pack_conv_split3(w, (f16*)dst, O, I, KH, KW, (hipStream_t)stream);
}
int sdmi_k_pack_geglu(const float* w, const float* bias, void* wdst, float* bdst, int N, int K, void* stream) {
  return launch_pack_geglu(w, bias, (f16*)wdst, bdst, N, K, (hipStream_t)stream);
}
int sdmi_image_to_uint8(const float* img_nchw, void* out_nhwc_u8, int B, int C, int H, int W, void* stream) {
  return launch_image_u8(img_nchw, (unsigned char*)out_nhwc_u8, B, C, H, W, (hipStream_t)stream);
}
int sdmi_range_check(int enable) { return range_check_set(enable); }
int sdmi_range_report(char* buf, int buflen) {
  SDMI_CHECK(buf && buflen > 1, "null buffer");
  std::string js;
  if (range_report(&js)) return -1;
  SDMI_CHECK((int)js.size() + 1 <= buflen, "range report buffer too small");
  memcpy(buf, js.c_str(), js.size() + 1);
  return 0;
}
int sdmi_tune_begin(void) { return tune_begin(); }
int sdmi_tune_round(int r) { return tune_round(r); }
int sdmi_tune_end(const char* path, int* n_keys) { return tune_end(path, n_keys); }
int sdmi_tune_dump(char* buf, int buflen) {
  SDMI_CHECK(buf && buflen > 1, "null buffer");
  std::string txt;
  if (tune_dump(&txt)) return -1;
  SDMI_CHECK((int)txt.size() + 1 <= buflen, "tune dump buffer too small");
  memcpy(buf, txt.c_str(), txt.size() + 1);
  return 0;
}
int sdmi_profile_begin(void) { return prof_begin(); }
int sdmi_profile_end(char* buf, int buflen) {
  SDMI_CHECK(buf && buflen > 2, "null buffer");
  std::string js;
  if (prof_end(&js)) return -1;
  SDMI_CHECK((int)js.size() + 1 <= buflen, "profile buffer too small");
  memcpy(buf, js.c_str(), js.size() + 1);
  return 0;
}
int sdmi_k_prefetch_lines(const void* ptr, int64_t bytes, void* stream) {
  SDMI_CHECK(ptr != nullptr && bytes >= 0, "bad range");
  return launch_prefetch_lines(ptr, bytes, (hipStream_t)stream);
}
const void* sdmi_zero_page(void) {
  const f16* z = nullptr;
  if (zero_page(&z)) return nullptr;
  return z;
}

}  // extern "C"
