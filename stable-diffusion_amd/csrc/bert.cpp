// Text-encoder executor of the LAION-400M model: BERTEmbedder's transformer (ldm/modules/encoders/modules.py:80-103),
// x_transformer.TransformerWrapper(num_tokens, max_seq_len, attn_layers=Encoder(dim, depth)) with return_embeddings=True
// and every other setting at its default (ldm/modules/x_transformer.py):
//   x = token_emb(ids) + pos_emb.emb(0..L-1)                                                    (:609-610; dropout = id)
//   per layer (pre-norm, plain residual, :506-531):
//     x += to_out(softmax(q k^T dim_head^-1/2) v),  q|k|v = Linear(LN(x)) without bias         (:240-266, :296-367)
//     x += net.2(gelu_erf(net.0.0(LN(x))))                                                     (:194-212)
//   out = norm(x)                                                                              (:624; to_logits unused)
// No causal mask and no padding mask: every token attends to all L.  Same kernels as CLIP (clip.cpp): igemm with the per-head
// scatter epilogue for q|k|v, the plain epilogue with bias + residual + next-LayerNorm post-op for to_out and net.2, the
// flash-attention kernel, layernorm; the exact-erf GELU kernel for the feed-forward.
// A SDMI_PRECISION_FULL handle runs the shared split-fp16 walk instead (TextEncBase::forward_full, clip.cpp).
#include <algorithm>

#include "clip.h"

#include <math.h>

namespace sdmi {

int BertText::build(const sdmi_bert_cfg& c, int precision) {
  cfg_ = c;
  precision_ = precision;
  SDMI_CHECK(c.dim >= 64 && c.dim % 64 == 0 && c.dim <= 2560, "dim must be a multiple of 64 (64..2560)");
  SDMI_CHECK(c.ff_inner >= 64 && c.ff_inner % 64 == 0, "ff_inner must be a multiple of 64");
  const int dh = c.dim_head;
  SDMI_CHECK(dh == 32 || dh == 40 || dh == 64 || dh == 80 || dh == 128 || dh == 160,
             "dim_head must be one the attention kernel has (32, 40, 64, 80, 128, 160)");
  // (the full-precision mode refuses nothing more: the non-causal split-fp16 attention has every head dim of this set)
  SDMI_CHECK(c.heads >= 1 && (c.heads * dh) % 64 == 0, "heads * dim_head must be a multiple of 64");
  SDMI_CHECK(c.depth >= 1 && c.vocab_size >= 1 && c.max_seq_len >= 1, "bad BERT config (depth, vocab_size, max_seq_len >= 1)");
  const int64_t D = c.dim, F = c.ff_inner, I = (int64_t)c.heads * dh;
  layers_.resize(c.depth);
  store_.expect("token_emb.weight", {c.vocab_size, D}, W_F32, &tok_);
  store_.expect("pos_emb.emb.weight", {c.max_seq_len, D}, W_F32, &pos_);
  for (int i = 0; i < c.depth; ++i) {   // NOTE: slots point into layers_, which must not reallocate from here on
    BLayer& Ly = layers_[i];
    const std::string a = "attn_layers.layers." + std::to_string(2 * i) + ".";
    const std::string f = "attn_layers.layers." + std::to_string(2 * i + 1) + ".";
    store_.expect(a + "0.weight", {D}, W_F32, &Ly.ln[0]);
    store_.expect(a + "0.bias", {D}, W_F32, &Ly.ln[1]);
    const char* names[3] = {"to_q", "to_k", "to_v"};
    for (int j = 0; j < 3; ++j) store_.expect(a + "1." + names[j] + ".weight", {I, D}, lin_kind(), &Ly.wqkv, j * (int)I, 3 * (int)I);
    store_.expect(a + "1.to_out.weight", {D, I}, lin_kind(), &Ly.wo);
    store_.expect(a + "1.to_out.bias", {D}, W_F32, &Ly.bo);
    store_.expect(f + "0.weight", {D}, W_F32, &Ly.ln[2]);
    store_.expect(f + "0.bias", {D}, W_F32, &Ly.ln[3]);
    store_.expect(f + "1.net.0.0.weight", {F, D}, lin_kind(), &Ly.w1);
    store_.expect(f + "1.net.0.0.bias", {F}, W_F32, &Ly.b1);
    store_.expect(f + "1.net.2.weight", {D, F}, lin_kind(), &Ly.w2);
    store_.expect(f + "1.net.2.bias", {D}, W_F32, &Ly.b2);
  }
  store_.expect("norm.weight", {D}, W_F32, &fln_g_);
  store_.expect("norm.bias", {D}, W_F32, &fln_b_);
  store_.expect("to_logits.weight", {c.vocab_size, D}, W_DROP, nullptr);
  store_.expect("to_logits.bias", {c.vocab_size}, W_DROP, nullptr);
  return 0;
}

int BertText::forward(const int64_t* ids, float* out, int B, int L, void* workspace, int64_t ws_bytes, hipStream_t stream,
                      bool dry, int64_t* bytes_needed) {
  SDMI_CHECK(dry || finalized_, "sdmi_bert_finalize() has not succeeded yet");
  SDMI_CHECK(B >= 1 && B <= 64, "batch must be 1..64");
  SDMI_CHECK(L >= 1 && L <= cfg_.max_seq_len, "sequence length must be 1..max_seq_len (" + std::to_string(cfg_.max_seq_len) + ")");
  SDMI_CHECK(dry || (ids != nullptr && out != nullptr), "ids / out is NULL");
  const int D = cfg_.dim, F = cfg_.ff_inner, H = cfg_.heads, dh = cfg_.dim_head, I = H * dh;
  const int M = B * L, Lp = (int)round_up(L, 8);
  const float scale = 1.0f / sqrtf((float)dh);
  // split-K slabs: the auto split of the to_out / net.2 GEMMs at the LAION shape (N = 1280, K = 5120, M = 2 x 77) takes 8
  // splits of 64 x 64 tiles = 2M floats; room for 16 splits of the widest N at up to 256 rows, 4M floats at least (CLIP's size)
  const int64_t slab_floats = std::max<int64_t>((int64_t)4 << 20, (int64_t)16 * 256 * std::max(D, 3 * I));
  if (full()) {
    TextFullDesc t;
    t.dim = D; t.inner = I; t.ff = F; t.heads = H; t.dh = dh; t.vocab = cfg_.vocab_size; t.causal = false; t.erf = true;
    t.tok = tok_; t.pos = pos_; t.fln_g = fln_g_; t.fln_b = fln_b_; t.slab_floats = slab_floats;
    for (const BLayer& Ly : layers_)
      t.layers.push_back({Ly.wqkv, nullptr, Ly.wo, Ly.bo, Ly.w1, Ly.b1, Ly.w2, Ly.b2, {Ly.ln[0], Ly.ln[1], Ly.ln[2], Ly.ln[3]}});
    return forward_full(t, ids, out, B, L, workspace, ws_bytes, stream, dry, bytes_needed);
  }
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
    if (f.begin_pass(slab_floats, /*with_gn=*/false)) return -1;
    float* x = f.P<float>((size_t)M * D);
    f16* ln = f.P<f16>((size_t)M * D);
    f16* q = f.P<f16>((size_t)M * I);
    f16* k = f.P<f16>((size_t)M * I);
    f16* vt = f.P<f16>((size_t)B * I * Lp);
    f16* ao = f.P<f16>((size_t)M * I);
    float* h1 = f.P<float>((size_t)M * F);
    f16* g = f.P<f16>((size_t)M * F);
    if (!d) {
      if (launch_embed_tokens(ids, tok_, pos_, x, M, L, D, cfg_.vocab_size, stream)) return -1;
      if (launch_layernorm(x, layers_[0].ln[0], layers_[0].ln[1], ln, M, D, 1e-5f, stream)) return -1;
      if (Lp != L) SDMI_HIP_OK(hipMemsetAsync(vt, 0, (size_t)B * I * Lp * sizeof(f16), stream));   // pad keys of V^T stay zero
    }
    for (int i = 0; i < cfg_.depth; ++i) {
      BLayer& Ly = layers_[i];
      {   // q | k | v = ln Wqkv^T, scattered per head (v transposed)
        IGemmParams p = f.dense(ln, M, D, Ly.wqkv, 3 * I, L);
        p.mode = EPI_HEADS; p.bias = nullptr; p.seg_dst[0] = q; p.seg_dst[1] = k; p.seg_dst[2] = vt;
        p.seg_kind[0] = 0; p.seg_kind[1] = 0; p.seg_kind[2] = 1;
        p.heads = H; p.dh = dh; p.ntok = L; p.ntok_pad = Lp; p.segC = I; p.splitk = 1;
        f.gemm(p);
      }
      if (!d && !f.rc) {
        AttnParams a = AttnParams();
        a.q = q; a.k = k; a.vt = vt; a.out = ao; a.BH = B * H; a.heads = H; a.nq = L; a.nkv = L; a.nkv_pad = Lp; a.d = dh;
        a.scale = scale; a.causal = 0;
        f.ok(launch_attention(a, stream));
      }
      {   // x += ao Wo^T + bo ; ln = LayerNorm of the feed-forward
        IGemmParams p = f.dense(ao, M, I, Ly.wo, D, L);
        p.bias = Ly.bo; p.residual = x; p.ldr = D; p.out_f32 = x; p.ldo = D;
        p.ln_gamma = Ly.ln[2]; p.ln_beta = Ly.ln[3]; p.ln_out = ln; p.ln_eps = 1e-5f;
        f.gemm(p);
      }
      {   // h1 = ln W1^T + b1 ; g = gelu(h1)
        IGemmParams p = f.dense(ln, M, D, Ly.w1, F, L);
        p.bias = Ly.b1; p.out_f32 = h1; p.ldo = F;
        f.gemm(p);
        if (!d && !f.rc) f.ok(launch_gelu_erf(h1, g, (int64_t)M * F, stream));
      }
      {   // x += g W2^T + b2 ; ln = LayerNorm of the next layer's attention
        IGemmParams p = f.dense(g, M, F, Ly.w2, D, L);
        p.bias = Ly.b2; p.residual = x; p.ldr = D; p.out_f32 = x; p.ldo = D;
        if (i + 1 < cfg_.depth) {
          p.ln_gamma = layers_[i + 1].ln[0]; p.ln_beta = layers_[i + 1].ln[1]; p.ln_out = ln; p.ln_eps = 1e-5f;
        }
        f.gemm(p);
      }
    }
    if (!d && !f.rc) f.ok(launch_layernorm(x, fln_g_, fln_b_, nullptr, M, D, 1e-5f, stream, out));
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
