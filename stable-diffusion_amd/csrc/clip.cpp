// Text-encoder executor: the HF `CLIPTextModel` that `FrozenCLIPEmbedder.forward` runs
// (ldm/modules/encoders/modules.py:137-162; model code: transformers==4.19.2 (environment.yaml:25)
// models/clip/modeling_clip.py CLIPTextTransformer / CLIPEncoderLayer / CLIPAttention / CLIPMLP) -- SURVEY.md 8 f-2.
//   embeddings = token_embedding(ids) + position_embedding(0..L-1)
//   per layer:  x += out_proj(causal_softmax(q k^T d^-1/2) v),  q|k|v = Linear(LayerNorm1(x))     (biases everywhere)
//               x += fc2(quick_gelu(fc1(LayerNorm2(x))))
//   last_hidden_state = final_layer_norm(x)
// Same kernels as the UNet's transformer blocks: igemm (per-head scatter epilogue with bias, plain epilogue with the
// LayerNorm post-op), the flash-attention kernel with a causal mask, layernorm; the token stream is fp32.
// SDMI_PRECISION_FULL handles (both encoders) run TextEncBase::forward_full at the end of this file instead: split-fp16 operands on every MFMA.
// The CLIP vision tower (ClipVision, below) walks the same layers through TextEncBase::mixed_layers with the causal mask off.
#include "clip.h"

#include <math.h>

namespace sdmi {

int ClipText::build(const sdmi_clip_cfg& c, int precision, int projection_dim) {
  cfg_ = c;
  precision_ = precision;
  proj_dim_ = projection_dim;
  SDMI_CHECK(projection_dim >= 0 && projection_dim <= 4096, "projection_dim " + std::to_string(projection_dim) + " outside 0 .. 4096");
  SDMI_CHECK(c.hidden_size % 64 == 0 && c.intermediate_size % 64 == 0, "hidden / intermediate size must be multiples of 64");
  SDMI_CHECK(c.num_heads >= 1 && c.hidden_size % c.num_heads == 0, "hidden_size % num_heads");
  const int dh = c.hidden_size / c.num_heads;
  SDMI_CHECK(dh == 32 || dh == 40 || dh == 64 || dh == 80 || dh == 128 || dh == 160, "head dim must be one the attention kernel has");
  SDMI_CHECK(!full() || dh == 32 || dh == 64 || dh == 128, "full-precision CLIP text encoder: head dim " + std::to_string(dh) +
                                                               " has no causal split-fp16 attention kernel (32, 64, 128)");
  SDMI_CHECK(c.num_layers >= 1 && c.vocab_size >= 1 && c.max_positions >= 1 && c.hidden_size <= 2560, "bad text-model config");
  const int64_t C = c.hidden_size, I = c.intermediate_size;
  layers_.resize(c.num_layers);
  const std::string tm = "text_model.";
  store_.expect(tm + "embeddings.token_embedding.weight", {c.vocab_size, C}, W_F32, &tok_);
  store_.expect(tm + "embeddings.position_embedding.weight", {c.max_positions, C}, W_F32, &pos_);
  for (int i = 0; i < c.num_layers; ++i)   // NOTE: slots point into layers_, which must not reallocate from here on
    expect_layer(tm + "encoder.layers." + std::to_string(i) + ".", layers_[i], C, I);
  store_.expect(tm + "final_layer_norm.weight", {C}, W_F32, &fln_g_);
  store_.expect(tm + "final_layer_norm.bias", {C}, W_F32, &fln_b_);
  if (projection_dim > 0) store_.expect("text_projection.weight", {(int64_t)projection_dim, C}, lin_kind(), &wproj_);
  return 0;
}

int ClipText::text_embeds(const int64_t* ids, float* out, int B, int L, int normalize, void* workspace, int64_t ws_bytes, hipStream_t stream,
                          bool dry, int64_t* bytes_needed) {
  SDMI_CHECK(proj_dim_ > 0, "sdmi_clip_text_embeds: this handle was created without a text projection (sdmi_clip_create_projection)");
  int64_t need_fwd = 0;
  if (forward(nullptr, nullptr, B, L, nullptr, 0, nullptr, true, &need_fwd)) return -1;
  const int64_t hid_bytes = round_up((int64_t)B * L * cfg_.hidden_size * (int64_t)sizeof(float), 4096);
  if (bytes_needed) *bytes_needed = need_fwd + hid_bytes;
  if (dry) return 0;
  SDMI_CHECK(ids != nullptr && out != nullptr, "ids / out is NULL");
  SDMI_CHECK(workspace != nullptr && ws_bytes >= need_fwd + hid_bytes, "workspace too small: need " + std::to_string(need_fwd + hid_bytes) +
                                                                           " bytes, got " + std::to_string(ws_bytes));
  float* hidden = (float*)workspace;
  if (forward(ids, hidden, B, L, (char*)workspace + hid_bytes, ws_bytes - hid_bytes, stream, false, nullptr)) return -1;
  return launch_clip_pool_project(ids, hidden, wproj_, full(), out, B, L, cfg_.hidden_size, proj_dim_, normalize, stream);
}

void TextEncBase::expect_layer(const std::string& p, CLayer& L, int64_t C, int64_t I) {
  const char* names[3] = {"q_proj", "k_proj", "v_proj"};
  for (int j = 0; j < 3; ++j) {
    store_.expect(p + "self_attn." + names[j] + ".weight", {C, C}, lin_kind(), &L.wqkv, j * (int)C, 3 * (int)C);
    store_.expect(p + "self_attn." + names[j] + ".bias", {C}, W_F32_ROWS, &L.bqkv, j * (int)C, 3 * (int)C);
  }
  store_.expect(p + "self_attn.out_proj.weight", {C, C}, lin_kind(), &L.wo);
  store_.expect(p + "self_attn.out_proj.bias", {C}, W_F32, &L.bo);
  store_.expect(p + "layer_norm1.weight", {C}, W_F32, &L.ln[0]);
  store_.expect(p + "layer_norm1.bias", {C}, W_F32, &L.ln[1]);
  store_.expect(p + "mlp.fc1.weight", {I, C}, lin_kind(), &L.w1);
  store_.expect(p + "mlp.fc1.bias", {I}, W_F32, &L.b1);
  store_.expect(p + "mlp.fc2.weight", {C, I}, lin_kind(), &L.w2);
  store_.expect(p + "mlp.fc2.bias", {C}, W_F32, &L.b2);
  store_.expect(p + "layer_norm2.weight", {C}, W_F32, &L.ln[2]);
  store_.expect(p + "layer_norm2.bias", {C}, W_F32, &L.ln[3]);
}

void TextEncBase::mixed_layers(FwdBase& f, const std::vector<CLayer>& layers, const MixedBufs& b, int B, int L, int C, int I, int H, bool causal) {
  const int M = B * L, Lp = (int)round_up(L, 8), dh = C / H, n_layers = (int)layers.size();
  const float scale = 1.0f / sqrtf((float)dh);
  const bool d = f.dry;
  for (int i = 0; i < n_layers; ++i) {
    const CLayer& Ly = layers[i];
    {   // q | k | v = ln Wqkv^T + b, scattered per head (v transposed)
      IGemmParams p = f.dense(b.ln, M, C, Ly.wqkv, 3 * C, L);
      p.mode = EPI_HEADS; p.bias = Ly.bqkv; p.seg_dst[0] = b.q; p.seg_dst[1] = b.k; p.seg_dst[2] = b.vt;
      p.seg_kind[0] = 0; p.seg_kind[1] = 0; p.seg_kind[2] = 1;
      p.heads = H; p.dh = dh; p.ntok = L; p.ntok_pad = Lp; p.segC = C; p.splitk = 1;
      f.gemm(p);
    }
    if (!d && !f.rc) {
      AttnParams a = AttnParams();
      a.q = b.q; a.k = b.k; a.vt = b.vt; a.out = b.ao; a.BH = B * H; a.heads = H; a.nq = L; a.nkv = L; a.nkv_pad = Lp; a.d = dh;
      a.scale = scale; a.causal = causal ? 1 : 0;
      f.ok(launch_attention(a, f.s));
    }
    {   // x += ao Wo^T + bo ; ln = LayerNorm2(x)
      IGemmParams p = f.dense(b.ao, M, C, Ly.wo, C, L);
      p.bias = Ly.bo; p.residual = b.x; p.ldr = C; p.out_f32 = b.x; p.ldo = C;
      p.ln_gamma = Ly.ln[2]; p.ln_beta = Ly.ln[3]; p.ln_out = b.ln; p.ln_eps = 1e-5f;
      f.gemm(p);
    }
    {   // h1 = ln W1^T + b1 ; g = quick_gelu(h1)
      IGemmParams p = f.dense(b.ln, M, C, Ly.w1, I, L);
      p.bias = Ly.b1; p.out_f32 = b.h1; p.ldo = I;
      f.gemm(p);
      if (!d && !f.rc) f.ok(launch_quick_gelu(b.h1, b.g, (int64_t)M * I, f.s));
    }
    {   // x += g W2^T + b2 ; ln = LayerNorm1 of the next layer
      IGemmParams p = f.dense(b.g, M, I, Ly.w2, C, L);
      p.bias = Ly.b2; p.residual = b.x; p.ldr = C; p.out_f32 = b.x; p.ldo = C;
      if (i + 1 < n_layers) {
        p.ln_gamma = layers[i + 1].ln[0]; p.ln_beta = layers[i + 1].ln[1]; p.ln_out = b.ln; p.ln_eps = 1e-5f;
      }
      f.gemm(p);
    }
  }
}

int TextEncBase::set_weight(const char* key, const float* ptr, const int64_t* shape, int ndim, hipStream_t stream) {
  if (int rc = store_.set(key, ptr, shape, ndim, stream)) return rc;
  finalized_ = false;
  return 0;
}

int TextEncBase::finalize() {
  if (const WeightSlot* m = store_.missing()) return fail("weight not set: " + m->key);
  if (store_.zero_page()) return -1;
  finalized_ = true;
  return 0;
}

int ClipText::forward(const int64_t* ids, float* out, int B, int L, void* workspace, int64_t ws_bytes, hipStream_t stream,
                      bool dry, int64_t* bytes_needed) {
  SDMI_CHECK(dry || finalized_, "sdmi_clip_finalize() has not succeeded yet");
  SDMI_CHECK(B >= 1 && B <= 64 && L >= 1 && L <= cfg_.max_positions, "batch 1..64, 1 <= L <= max_positions");
  SDMI_CHECK(dry || (ids != nullptr && out != nullptr), "ids / out is NULL");
  if (full()) {
    TextFullDesc t;
    t.dim = t.inner = cfg_.hidden_size; t.ff = cfg_.intermediate_size; t.heads = cfg_.num_heads; t.dh = t.dim / t.heads;
    t.vocab = cfg_.vocab_size; t.causal = true; t.erf = false;
    t.tok = tok_; t.pos = pos_; t.fln_g = fln_g_; t.fln_b = fln_b_; t.slab_floats = (int64_t)4 << 20;
    for (const CLayer& Ly : layers_)
      t.layers.push_back({Ly.wqkv, Ly.bqkv, Ly.wo, Ly.bo, Ly.w1, Ly.b1, Ly.w2, Ly.b2, {Ly.ln[0], Ly.ln[1], Ly.ln[2], Ly.ln[3]}});
    return forward_full(t, ids, out, B, L, workspace, ws_bytes, stream, dry, bytes_needed);
  }
  const int C = cfg_.hidden_size, I = cfg_.intermediate_size, H = cfg_.num_heads;
  const int M = B * L, Lp = (int)round_up(L, 8);
  FwdBase f;
  f.s = stream; f.B = B; f.zero = store_.zero(); f.precise_1x1 = false;
  int64_t persist_bytes = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool d = pass == 0;
    if (pass == 1 && dry) break;
    f.dry = d; f.rc = 0;
    f.persist = Arena(); f.scratch = Arena();
    f.persist.dry = f.scratch.dry = d;
    if (!d) {
      SDMI_CHECK(persist_bytes <= ws_bytes, "workspace too small: need " + std::to_string(persist_bytes) + " bytes, got " +
                                                std::to_string(ws_bytes));
      SDMI_CHECK(workspace != nullptr, "workspace is NULL");
      f.persist.base = (char*)workspace; f.persist.cap = (size_t)persist_bytes;
    }
    if (f.begin_pass((int64_t)4 << 20, /*with_gn=*/false)) return -1;     // split-K slabs only: no GroupNorm in this model
    float* x = f.P<float>((size_t)M * C);
    f16* ln = f.P<f16>((size_t)M * C);
    f16* q = f.P<f16>((size_t)M * C);
    f16* k = f.P<f16>((size_t)M * C);
    f16* vt = f.P<f16>((size_t)B * C * Lp);
    f16* ao = f.P<f16>((size_t)M * C);
    float* h1 = f.P<float>((size_t)M * I);
    f16* g = f.P<f16>((size_t)M * I);
    if (!d) {
      if (launch_embed_tokens(ids, tok_, pos_, x, M, L, C, cfg_.vocab_size, stream)) return -1;
      if (launch_layernorm(x, layers_[0].ln[0], layers_[0].ln[1], ln, M, C, 1e-5f, stream)) return -1;
      if (Lp != L) SDMI_HIP_OK(hipMemsetAsync(vt, 0, (size_t)B * C * Lp * sizeof(f16), stream));   // pad keys of V^T stay zero
    }
    mixed_layers(f, layers_, MixedBufs{x, ln, q, k, vt, ao, h1, g}, B, L, C, I, H, /*causal=*/true);
    if (!d && !f.rc) f.ok(launch_layernorm(x, fln_g_, fln_b_, nullptr, M, C, 1e-5f, stream, out));
    if (f.rc) return f.rc;
    if (d) {
      persist_bytes = (int64_t)round_up((int64_t)f.persist.peak, 4096) + 4096;
      if (bytes_needed) *bytes_needed = persist_bytes;
    } else {
      SDMI_CHECK(!f.persist.overflow, "internal: arena overflow");
    }
  }
  return 0;
}

// ---- CLIP vision tower --------------------------------------------------------------------------------------------------------------
// CLIPVisionModelWithProjection (modeling_clip.py: CLIPVisionEmbeddings, CLIPVisionTransformer):
//   x = pre_layrnorm(cat(class_embedding, patch_embedding(pixel_values)) + position_embedding)      (patch_embedding: p x p conv, stride p, no bias)
//   x = the CLIPEncoderLayers of the text tower, without the causal mask                      -> last_hidden_state
//   pooled_output = post_layernorm(x[:, 0]);  image_embeds = visual_projection(pooled_output)       (no bias)
// The patch convolution is vit_patchify (im2col, fp16, K zero-padded to whole 64-wide k-tiles) and ONE dense GEMM of the family; both
// LayerNorms outside the layers feed fp32 consumers and write fp32.
int ClipVision::build(const sdmi_vit_cfg& c) {
  cfg_ = c;
  precision_ = SDMI_PRECISION_MIXED;
  SDMI_CHECK(c.hidden_size >= 64 && c.hidden_size % 64 == 0 && c.hidden_size <= 2560,
             "vision tower: hidden_size " + std::to_string(c.hidden_size) + " must be a multiple of 64 (<= 2560)");
  SDMI_CHECK(c.intermediate_size >= 64 && c.intermediate_size % 64 == 0,
             "vision tower: intermediate_size " + std::to_string(c.intermediate_size) + " must be a multiple of 64");
  SDMI_CHECK(c.num_heads >= 1 && c.hidden_size % c.num_heads == 0, "vision tower: hidden_size % num_heads");
  const int dh = c.hidden_size / c.num_heads;
  SDMI_CHECK(dh == 32 || dh == 40 || dh == 64 || dh == 80 || dh == 128 || dh == 160,
             "vision tower: head dim " + std::to_string(dh) + " is not one the attention kernel has (32, 40, 64, 80, 128, 160)");
  SDMI_CHECK(c.patch_size >= 1 && c.patch_size <= 64 && c.image_size >= c.patch_size && c.image_size % c.patch_size == 0,
             "vision tower: image_size % patch_size != 0 (image_size " + std::to_string(c.image_size) + ", patch_size " +
                 std::to_string(c.patch_size) + ")");
  SDMI_CHECK(tokens() <= 1024, "vision tower: " + std::to_string(tokens()) + " tokens, more than 1024 tokens are not supported");
  SDMI_CHECK(c.num_layers >= 1 && c.projection_dim >= 1, "bad vision-model config");
  const int64_t C = c.hidden_size, I = c.intermediate_size, p = c.patch_size;
  layers_.resize(c.num_layers);
  const std::string vm = "vision_model.";
  store_.expect(vm + "embeddings.class_embedding", {C}, W_F32, &cls_);
  store_.expect(vm + "embeddings.patch_embedding.weight", {C, 3, p, p}, W_ROWS16_PAD64, &wpatch_);
  store_.expect(vm + "embeddings.position_embedding.weight", {(int64_t)tokens(), C}, W_F32, &pos_);
  store_.expect(vm + "pre_layrnorm.weight", {C}, W_F32, &pre_g_);
  store_.expect(vm + "pre_layrnorm.bias", {C}, W_F32, &pre_b_);
  for (int i = 0; i < c.num_layers; ++i)   // NOTE: slots point into layers_, which must not reallocate from here on
    expect_layer(vm + "encoder.layers." + std::to_string(i) + ".", layers_[i], C, I);
  store_.expect(vm + "post_layernorm.weight", {C}, W_F32, &post_g_);
  store_.expect(vm + "post_layernorm.bias", {C}, W_F32, &post_b_);
  store_.expect("visual_projection.weight", {(int64_t)c.projection_dim, C}, W_F32, &wproj_);
  return 0;
}

int ClipVision::forward(const float* px, float* last_hidden, float* pooled, float* image_embeds, int B, void* workspace, int64_t ws_bytes,
                        hipStream_t stream, bool dry, int64_t* bytes_needed) {
  SDMI_CHECK(dry || finalized_, "sdmi_vit_finalize() has not succeeded yet");
  SDMI_CHECK(B >= 1 && B <= 64, "vision tower: batch " + std::to_string(B) + " outside 1..64 (B > 64 is not supported)");
  SDMI_CHECK(dry || (px != nullptr && image_embeds != nullptr), "pixel_values / image_embeds is NULL");
  const int C = cfg_.hidden_size, I = cfg_.intermediate_size, H = cfg_.num_heads, S = cfg_.image_size, ps = cfg_.patch_size;
  const int P2 = (S / ps) * (S / ps), T = 1 + P2, M = B * T, Tp = (int)round_up(T, 8), Kp = vit_kpad(ps), Pd = cfg_.projection_dim;
  FwdBase f;
  f.s = stream; f.B = B; f.zero = store_.zero(); f.precise_1x1 = false;
  int64_t persist_bytes = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool d = pass == 0;
    if (pass == 1 && dry) break;
    f.dry = d; f.rc = 0;
    f.persist = Arena(); f.scratch = Arena();
    f.persist.dry = f.scratch.dry = d;
    if (!d) {
      SDMI_CHECK(persist_bytes <= ws_bytes, "workspace too small: need " + std::to_string(persist_bytes) + " bytes, got " +
                                                std::to_string(ws_bytes));
      SDMI_CHECK(workspace != nullptr, "workspace is NULL");
      f.persist.base = (char*)workspace; f.persist.cap = (size_t)persist_bytes;
    }
    if (f.begin_pass((int64_t)4 << 20, /*with_gn=*/false)) return -1;     // split-K slabs only
    f16* cols = f.P<f16>((size_t)B * P2 * Kp);
    float* patch = f.P<float>((size_t)B * P2 * C);
    float* emb = f.P<float>((size_t)M * C);
    float* x = f.P<float>((size_t)M * C);
    f16* ln = f.P<f16>((size_t)M * C);
    f16* q = f.P<f16>((size_t)M * C);
    f16* k = f.P<f16>((size_t)M * C);
    f16* vt = f.P<f16>((size_t)B * C * Tp);
    f16* ao = f.P<f16>((size_t)M * C);
    float* h1 = f.P<float>((size_t)M * I);
    f16* g = f.P<f16>((size_t)M * I);
    float* cls = f.P<float>((size_t)B * C);
    float* pooled_ws = f.P<float>((size_t)B * C);
    auto launch = [&](auto&& fn) { if (!d && !f.rc) f.ok(fn()); };
    launch([&] { return launch_vit_patchify(px, cols, B, S, ps, stream); });
    {   // the patch embedding: [B P^2][Kp] x [C][Kp]^T, no bias
      IGemmParams p = f.dense(cols, B * P2, Kp, wpatch_, C, P2);
      p.out_f32 = patch; p.ldo = C;
      f.gemm(p);
    }
    launch([&] { return launch_vit_embed(patch, cls_, pos_, emb, B, T, C, stream); });
    launch([&] { return launch_layernorm(emb, pre_g_, pre_b_, nullptr, M, C, 1e-5f, stream, x); });                  // pre_layrnorm, fp32
    launch([&] { return launch_layernorm(x, layers_[0].ln[0], layers_[0].ln[1], ln, M, C, 1e-5f, stream); });
    if (!d && !f.rc && Tp != T) SDMI_HIP_OK(hipMemsetAsync(vt, 0, (size_t)B * C * Tp * sizeof(f16), stream));        // pad keys of V^T stay zero
    mixed_layers(f, layers_, MixedBufs{x, ln, q, k, vt, ao, h1, g}, B, T, C, I, H, /*causal=*/false);
    if (!d && !f.rc) {
      if (last_hidden) SDMI_HIP_OK(hipMemcpyAsync(last_hidden, x, (size_t)M * C * sizeof(float), hipMemcpyDeviceToDevice, stream));
      // post_layernorm reads row 0 of every sample only
      SDMI_HIP_OK(hipMemcpy2DAsync(cls, (size_t)C * sizeof(float), x, (size_t)T * C * sizeof(float), (size_t)C * sizeof(float), (size_t)B,
                                   hipMemcpyDeviceToDevice, stream));
    }
    float* po = pooled ? pooled : pooled_ws;
    launch([&] { return launch_layernorm(cls, post_g_, post_b_, nullptr, B, C, 1e-5f, stream, po); });
    for (int b0 = 0; b0 < B; b0 += 8)       // visual_projection through the fp32 small-batch linear (8 rows per launch)
      launch([&] { return launch_small_linear(po + (size_t)b0 * C, C, wproj_, nullptr, image_embeds + (size_t)b0 * Pd, Pd, std::min(8, B - b0), Pd, C, 0, stream); });
    if (f.rc) return f.rc;
    if (d) {
      persist_bytes = (int64_t)round_up((int64_t)f.persist.peak, 4096) + 4096;
      if (bytes_needed) *bytes_needed = persist_bytes;
    } else {
      SDMI_CHECK(!f.persist.overflow, "internal: arena overflow");
    }
  }
  return 0;
}

int TextEncBase::forward_full(const TextFullDesc& t, const int64_t* ids, float* out, int B, int L, void* workspace, int64_t ws_bytes,
                              hipStream_t stream, bool dry, int64_t* bytes_needed) {
  const int D = t.dim, I = t.inner, F = t.ff, H = t.heads, dh = t.dh;
  const int M = B * L, Lp = (int)round_up(L, 8);
  const float scale = 1.0f / sqrtf((float)dh);
  FwdBase f;
  f.s = stream; f.B = B; f.zero = store_.zero(); f.precise_1x1 = true;
  int64_t persist_bytes = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool d = pass == 0;
    if (pass == 1 && dry) break;
    f.dry = d; f.rc = 0;
    f.persist = Arena(); f.scratch = Arena();
    f.persist.dry = f.scratch.dry = d;
    if (!d) {
      SDMI_CHECK(persist_bytes <= ws_bytes, "workspace too small: need " + std::to_string(persist_bytes) + " bytes, got " +
                                                std::to_string(ws_bytes));
      SDMI_CHECK(workspace != nullptr, "workspace is NULL");
      f.persist.base = (char*)workspace; f.persist.cap = (size_t)persist_bytes;
    }
    if (f.begin_pass(t.slab_floats, /*with_gn=*/false)) return -1;
    float* x = f.P<float>((size_t)M * D);                                         // the token stream
    const size_t na = (size_t)M * (D > I ? D : I), ny = (size_t)M * (3 * I > F ? 3 * I : F);
    f16* a = f.P<f16>(na); f16* a_lo = f.P<f16>(na);                              // the operand of the next linear: LayerNorm / attention output
    float* y = f.P<float>(ny);                                                    // q | k | v, then fc1 (fp32)
    f16* q = f.P<f16>((size_t)M * I); f16* q_lo = f.P<f16>((size_t)M * I);
    f16* k = f.P<f16>((size_t)M * I); f16* k_lo = f.P<f16>((size_t)M * I);
    f16* vt = f.P<f16>((size_t)B * I * Lp); f16* vt_lo = f.P<f16>((size_t)B * I * Lp);
    f16* g = f.P<f16>((size_t)M * F); f16* g_lo = f.P<f16>((size_t)M * F);
    auto linear = [&](const f16* hi, const f16* lo, int K, const f16* w, int n_out, const float* bias, float* dst, bool residual) {
      IGemmParams p = f.dense1x1(hi, lo, M, K, w, n_out, L, true);
      p.bias = bias; p.out_f32 = dst; p.ldo = n_out;
      if (residual) { p.residual = dst; p.ldr = n_out; }       // x = f(x) + x, in place
      f.gemm(p);
    };
    auto launch = [&](auto&& fn) { if (!d && !f.rc) f.ok(fn()); };
    launch([&] { return launch_embed_tokens(ids, t.tok, t.pos, x, M, L, D, t.vocab, stream); });
    for (const TextFullLayer& Ly : t.layers) {
      launch([&] { return launch_layernorm_split(x, Ly.ln[0], Ly.ln[1], a, a_lo, M, D, 1e-5f, stream); });
      linear(a, a_lo, D, Ly.wqkv, 3 * I, Ly.bqkv, y, false);
      launch([&] { return launch_split_heads(y, 3 * I, 0, q, q_lo, 0, B, L, Lp, H, dh, stream); });
      launch([&] { return launch_split_heads(y, 3 * I, I, k, k_lo, 0, B, L, Lp, H, dh, stream); });
      launch([&] { return launch_split_heads(y, 3 * I, 2 * I, vt, vt_lo, 1, B, L, Lp, H, dh, stream); });   // (pad keys written as zero)
      launch([&] {
        AttnSplitParams p = AttnSplitParams();
        p.q = q; p.q_lo = q_lo; p.k = k; p.k_lo = k_lo; p.vt = vt; p.vt_lo = vt_lo; p.out = a; p.out_lo = a_lo;
        p.BH = B * H; p.heads = H; p.nq = L; p.nkv = L; p.nkv_pad = Lp; p.d = dh; p.scale = scale; p.causal = t.causal ? 1 : 0;
        return launch_attention_split16(p, stream);
      });
      linear(a, a_lo, I, Ly.wo, D, Ly.bo, x, true);
      launch([&] { return launch_layernorm_split(x, Ly.ln[2], Ly.ln[3], a, a_lo, M, D, 1e-5f, stream); });
      linear(a, a_lo, D, Ly.w1, F, Ly.b1, y, false);
      launch([&] {
        return t.erf ? launch_gelu_erf_split(y, g, g_lo, (int64_t)M * F, stream) : launch_quick_gelu_split(y, g, g_lo, (int64_t)M * F, stream);
      });
      linear(g, g_lo, F, Ly.w2, D, Ly.b2, x, true);
    }
    launch([&] { return launch_layernorm(x, t.fln_g, t.fln_b, nullptr, M, D, 1e-5f, stream, out); });
    if (f.rc) return f.rc;
    if (d) {
      persist_bytes = (int64_t)round_up((int64_t)f.persist.peak, 4096) + 4096;
      if (bytes_needed) *bytes_needed = persist_bytes;
    } else {
      SDMI_CHECK(!f.persist.overflow, "internal: arena overflow");
    }
  }
  return 0;
}

}  // namespace sdmi
