// First-stage executor: AutoencoderKL.decode / .encode (ldm/models/autoencoder.py:324-333) as a static launch
// sequence over the same gfx950 kernels the UNet uses.
//   Decoder.forward   ldm/modules/diffusionmodules/model.py:528-568   (ctor :462-526)
//   Encoder.forward   model.py:427-460                                 (ctor :368-425)
//   ResnetBlock       model.py:119-141 (temb is None for the first stage)
//   AttnBlock         model.py:172-202 (one head, d = C)
//   Upsample / Downsample  model.py:41-79 (nearest x2 + conv3x3 / zero pad (0,1,0,1) + conv3x3 stride 2)
//
// Data layout: the activation stream is fp32 NHWC [B*H*W][C]; GroupNorm(32, eps 1e-6)+SiLU writes the fp16 A operand of
// the following implicit-GEMM conv; nin_shortcut (1x1 on the raw stream) runs as a 3-pass split-fp16 GEMM; the first
// (z -> 512) and last (128 -> 3) convs and the two 1x1 "quant" convs are fp32.  Attention over N = H*W tokens with
// d = C = 512 is three GEMMs (q k^T, softmax rows, P v) on the igemm kernel, in query chunks so S stays cache-sized.
// A handle created with attention at resolution levels (sdmi_vae_create_attn, attn_level_mask != 0: KL-f16 of the retrieval-augmented model,
// AttnBlocks after every ResBlock of the 16 x 16 level) runs every attention block, level and mid, as one flash launch instead
// (VFwd::attn_block_flash): no S / P buffers, any token count.  A handle without level attention takes that form only at token counts the
// GEMM form refuses (H W % 64 != 0).  On a mixed handle of six or more levels (KL-f32) the decoder's mid block and its levels >= 4 run with
// split-fp16 operands, as every layer of a SDMI_PRECISION_FULL handle does (VLayer::split, set in Vae::build).
//
// A handle created with SDMI_PRECISION_FULL (sdmi_vae_create_precision) runs the same layers with every MFMA operand as a split-fp16
// pair, as the UNet's full-precision mode does (unet.cpp: Fwd::res_block / resample / attn_block_full): GroupNorm writes hi | lo, the
// 3x3 convs are 3-pass split convs against weights packed [w_hi | w_hi | w_lo], q / k / v / proj_out are split GEMMs into fp32 and the
// attention is one split-fp16 flash launch (attn_split16.hip up to d = 160, attn_wide_split16.hip for 192 .. 1024): no S / P buffer, no
// query chunks.  The fp32 ends (conv_in, conv_out, the quant convs, the codebook quantizer) are the same launches in both modes.
#include "vae.h"

#include "split16.h"

#include <math.h>
#include <stdlib.h>

#include <algorithm>

namespace sdmi {

// head dims launch_attention instantiates (attn.hip / attn_wide.hip) among the widths a first stage can have (ch % 64 == 0 does not hold for
// the narrow ones, which are listed for the message's sake) ...
static bool mixed_attn_width(int d) { return d == 32 || d == 40 || d == 64 || d == 80 || d == 96 || d == 128 || d == 160 || (d > 160 && d <= 1024 && d % 64 == 0); }
// ... and launch_attention_split16's (attn_split16.hip / attn_wide_split16.hip)
static bool full_attn_width(int d) { return d == 64 || d == 128 || (d > 160 && d <= 1024 && d % 64 == 0); }

int Vae::build(const sdmi_vae_cfg& c, int parts, const sdmi_vae_ext* ext, int precision, uint32_t attn_level_mask) {
  cfg_ = c; parts_ = parts; precision_ = precision; attn_level_mask_ = attn_level_mask;
  if (ext) ext_ = *ext;
  SDMI_CHECK((ext_.double_z == 0 || ext_.double_z == 1) && (ext_.mid_attn == 0 || ext_.mid_attn == 1) && ext_.n_embed >= 0,
             "first-stage extension: double_z and mid_attn are 0 or 1, n_embed >= 0");
  SDMI_CHECK(ext_.n_embed == 0 || (c.embed_dim == 1 || c.embed_dim == 2 || c.embed_dim == 3 || c.embed_dim == 4 || c.embed_dim == 8),
             "codebook quantizer: embed_dim must be 1, 2, 3, 4 or 8");
  SDMI_CHECK(parts >= 1 && parts <= 3, "parts: 1 decoder, 2 encoder, 3 both");
  SDMI_CHECK(c.n_levels >= 1 && c.n_levels <= 8 && c.num_res_blocks >= 1, "bad level / res block count");
  SDMI_CHECK(c.ch % 64 == 0, "ch must be a multiple of 64 on this path");
  // (the latent widths the fp32 ends take: decoder.conv_in reads up to 64 channels (launch_conv_in), encoder.conv_out writes up to 128 with
  // double_z (launch_conv_out), the quant convs read up to 128 (launch_pointwise_nchw))
  auto latent_width = [](int v) { return (v >= 1 && v <= 16) || v == 32 || v == 64; };
  SDMI_CHECK(c.in_channels >= 1 && c.in_channels <= 16 && latent_width(c.z_channels) && latent_width(c.embed_dim) && c.out_ch >= 1 &&
                 c.out_ch <= 8,
             "in_channels <= 16, z_channels <= 16 (or 32 / 64), embed_dim <= 16 (or 32 / 64), out_ch <= 8 on this path");
  const int n = c.n_levels;
  SDMI_CHECK((attn_level_mask >> n) == 0, "attn_level_mask " + std::to_string(attn_level_mask) + " names a level past the last one (" +
             std::to_string(n) + " levels)");
  if (full() && ext_.mid_attn) {       // the mid-block attention is single-headed at d = the mid width
    const int d = c.ch * c.ch_mult[n - 1];
    SDMI_CHECK(full_attn_width(d), "full-precision first stage: mid-block attention width " + std::to_string(d) +
               " has no split-fp16 attention kernel (64, 128, and 192 .. 1024 in steps of 64)");
  }
  // a handle with level attention runs every mixed-precision attention block, the mid block's too, as one flash launch at d = its width
  // (a handle without keeps the GEMM / softmax / GEMM form, which takes any width)
  if (!full() && attn_level_mask && ext_.mid_attn) {
    const int d = c.ch * c.ch_mult[n - 1];
    SDMI_CHECK(mixed_attn_width(d), "first stage with level attention: mid-block attention width " + std::to_string(d) +
               " has no attention kernel (32 / 40 / 64 / 80 / 96 / 128 / 160, and 192 .. 1024 in steps of 64)");
  }
  for (int lvl = 0; lvl < n; ++lvl) {
    if (!((attn_level_mask >> lvl) & 1)) continue;
    const int d = c.ch * c.ch_mult[lvl];
    if (full())
      SDMI_CHECK(full_attn_width(d), "full-precision first stage: level " + std::to_string(lvl) + " attention width " + std::to_string(d) +
                 " has no split-fp16 attention kernel (64, 128, and 192 .. 1024 in steps of 64)");
    else
      SDMI_CHECK(mixed_attn_width(d), "first stage: level " + std::to_string(lvl) + " attention width " + std::to_string(d) +
                 " has no attention kernel (32 / 40 / 64 / 80 / 96 / 128 / 160, and 192 .. 1024 in steps of 64)");
  }
  auto level_attn = [&](int lvl) { return ((attn_level_mask >> lvl) & 1) != 0; };
  auto res = [&](const std::string& p, int ci, int co) { VLayer L; L.kind = V_RES; L.prefix = p; L.cin = ci; L.cout = co; return L; };
  auto one = [&](VKind k, const std::string& p, int ch) { VLayer L; L.kind = k; L.prefix = p; L.cin = ch; L.cout = ch; return L; };

  if (parts & 1) {
    int bi = c.ch * c.ch_mult[n - 1];
    dec_.push_back(res("decoder.mid.block_1", bi, bi));
    if (ext_.mid_attn) dec_.push_back(one(V_ATTN, "decoder.mid.attn_1", bi));
    dec_.push_back(res("decoder.mid.block_2", bi, bi));
    for (int lvl = n - 1; lvl >= 0; --lvl) {
      const int bo = c.ch * c.ch_mult[lvl];
      for (int i = 0; i <= c.num_res_blocks; ++i) {
        dec_.push_back(res("decoder.up." + std::to_string(lvl) + ".block." + std::to_string(i), bi, bo));
        bi = bo;
        if (level_attn(lvl)) dec_.push_back(one(V_ATTN, "decoder.up." + std::to_string(lvl) + ".attn." + std::to_string(i), bi));   // model.py:553-555
      }
      if (lvl != 0) dec_.push_back(one(V_UP, "decoder.up." + std::to_string(lvl) + ".upsample", bi));
    }
    dec_c_end_ = bi;
    // Mixed precision on a stage of six levels or more (KL-f32): the decoder's mid block and its levels at 1 / 16 of the image resolution and
    // below run with split-fp16 operands, as a full-precision handle runs every layer.  A pixel of those maps reaches 16 x 16 .. 32 x 32
    // image pixels, so an fp16 operand rounding there is a coherent error over a whole patch: with the reference's own arithmetic those
    // layers carry 1.0e-3 of the decode's 1.3e-3 rms error at fp16 operands (profiles/first_stages_parity.txt), for about 8 % of its MACs.
    // Stages of up to five levels -- every handle that built before KL-f32 -- keep the allocation they had.
    if (!full() && n >= 6) {
      for (auto& L : dec_) {
        const bool mid = L.prefix.compare(0, 12, "decoder.mid.") == 0;
        int lvl = -1;
        if (!mid) lvl = atoi(L.prefix.c_str() + 11);            // "decoder.up.<lvl>."
        L.split = mid || lvl >= 4;
        if (L.split && L.kind == V_ATTN)
          SDMI_CHECK(full_attn_width(L.cin), "first stage: " + L.prefix + " runs with split-fp16 operands and its width " + std::to_string(L.cin) +
                     " has no split-fp16 attention kernel (64, 128, and 192 .. 1024 in steps of 64)");
      }
    }
  }
  if (parts & 2) {
    int bi = c.ch;
    for (int lvl = 0; lvl < n; ++lvl) {
      const int bo = c.ch * c.ch_mult[lvl];
      for (int i = 0; i < c.num_res_blocks; ++i) {
        enc_.push_back(res("encoder.down." + std::to_string(lvl) + ".block." + std::to_string(i), bi, bo));
        bi = bo;
        if (level_attn(lvl)) enc_.push_back(one(V_ATTN, "encoder.down." + std::to_string(lvl) + ".attn." + std::to_string(i), bi));   // model.py:442-444
      }
      if (lvl != n - 1) enc_.push_back(one(V_DOWN, "encoder.down." + std::to_string(lvl) + ".downsample", bi));
    }
    enc_.push_back(res("encoder.mid.block_1", bi, bi));
    if (ext_.mid_attn) enc_.push_back(one(V_ATTN, "encoder.mid.attn_1", bi));
    enc_.push_back(res("encoder.mid.block_2", bi, bi));
    enc_c_end_ = bi;
  }

  // ---- expected state_dict entries (AutoencoderKL.state_dict() minus loss.*) -------------------------------------------
  auto visit = [&](VLayer& L) {
    const std::string& p = L.prefix;
    const int64_t ci = L.cin, co = L.cout;
    if (full()) L.split = true;
    const WKind conv_kind = L.split ? W_CONV_SPLIT3 : W_CONV;
    const WKind lin_kind = L.split ? W_SPLIT3 : W_ROWS16;
    switch (L.kind) {
      case V_RES:
        store_.expect(p + ".norm1.weight", {ci}, W_F32, &L.f32[0]);
        store_.expect(p + ".norm1.bias", {ci}, W_F32, &L.f32[1]);
        store_.expect(p + ".conv1.weight", {co, ci, 3, 3}, conv_kind, &L.w16[0]);
        store_.expect(p + ".conv1.bias", {co}, W_F32, &L.f32[2]);
        store_.expect(p + ".norm2.weight", {co}, W_F32, &L.f32[3]);
        store_.expect(p + ".norm2.bias", {co}, W_F32, &L.f32[4]);
        store_.expect(p + ".conv2.weight", {co, co, 3, 3}, conv_kind, &L.w16[1]);
        store_.expect(p + ".conv2.bias", {co}, W_F32, &L.f32[5]);
        if (ci != co) {
          store_.expect(p + ".nin_shortcut.weight", {co, ci, 1, 1}, (precise_1x1_ || L.split) ? W_SPLIT3 : W_ROWS16, &L.w16[2]);
          store_.expect(p + ".nin_shortcut.bias", {co}, W_F32, &L.f32[6]);
        }
        break;
      case V_ATTN: {
        store_.expect(p + ".norm.weight", {ci}, W_F32, &L.f32[0]);
        store_.expect(p + ".norm.bias", {ci}, W_F32, &L.f32[1]);
        const char* names[4] = {"q", "k", "v", "proj_out"};
        for (int i = 0; i < 4; ++i) {
          store_.expect(p + "." + names[i] + ".weight", {ci, ci, 1, 1}, lin_kind, &L.w16[i]);
          store_.expect(p + "." + names[i] + ".bias", {ci}, W_F32, &L.f32[2 + i]);
        }
        break;
      }
      case V_UP:
      case V_DOWN:
        store_.expect(p + ".conv.weight", {co, ci, 3, 3}, conv_kind, &L.w16[0]);
        store_.expect(p + ".conv.bias", {co}, W_F32, &L.f32[0]);
        break;
    }
  };
  // NOTE: slots hold pointers into the VLayer objects: dec_ / enc_ must not reallocate after this point.
  if (parts & 2) {
    store_.expect("encoder.conv_in.weight", {c.ch, c.in_channels, 3, 3}, W_F32, &eci_w_);
    store_.expect("encoder.conv_in.bias", {c.ch}, W_F32, &eci_b_);
    for (auto& L : enc_) visit(L);
    store_.expect("encoder.norm_out.weight", {enc_c_end_}, W_F32, &eno_g_);
    store_.expect("encoder.norm_out.bias", {enc_c_end_}, W_F32, &eno_b_);
    store_.expect("encoder.conv_out.weight", {enc_zc(), enc_c_end_, 3, 3}, W_CONV_OUT, &eco_w_);
    store_.expect("encoder.conv_out.bias", {enc_zc()}, W_F32, &eco_b_);
    store_.expect("quant_conv.weight", {enc_ed(), enc_zc(), 1, 1}, W_F32, &q_w_);
    store_.expect("quant_conv.bias", {enc_ed()}, W_F32, &q_b_);
  }
  if (parts & 1) {
    if (ext_.n_embed > 0) store_.expect("quantize.embedding.weight", {ext_.n_embed, c.embed_dim}, W_F32, &cb_);
    store_.expect("post_quant_conv.weight", {c.z_channels, c.embed_dim, 1, 1}, W_F32, &pq_w_);
    store_.expect("post_quant_conv.bias", {c.z_channels}, W_F32, &pq_b_);
    store_.expect("decoder.conv_in.weight", {c.ch * c.ch_mult[n - 1], c.z_channels, 3, 3}, W_F32, &dci_w_);
    store_.expect("decoder.conv_in.bias", {c.ch * c.ch_mult[n - 1]}, W_F32, &dci_b_);
    for (auto& L : dec_) visit(L);
    store_.expect("decoder.norm_out.weight", {dec_c_end_}, W_F32, &dno_g_);
    store_.expect("decoder.norm_out.bias", {dec_c_end_}, W_F32, &dno_b_);
    store_.expect("decoder.conv_out.weight", {c.out_ch, dec_c_end_, 3, 3}, W_CONV_OUT, &dco_w_);
    store_.expect("decoder.conv_out.bias", {c.out_ch}, W_F32, &dco_b_);
  }
  return 0;
}

int Vae::set_weight(const char* key, const float* ptr, const int64_t* shape, int ndim, hipStream_t stream) {
  if (int rc = store_.set(key, ptr, shape, ndim, stream)) return rc;
  finalized_ = false;
  return 0;
}

int Vae::finalize() {
  if (const WeightSlot* m = store_.missing()) return fail("weight not set: " + m->key);
  if (store_.zero_page()) return -1;
  if (cb_) {          // sum e^2 of every code, once per set of weights (the quantizer's distance expression)
    if (store_.alloc((void**)&cb_norm_, (size_t)ext_.n_embed * sizeof(float))) return -1;
    SDMI_HIP_OK(hipDeviceSynchronize());         // (set_weight copied the codebook on the caller's stream)
    if (launch_vq_norms(cb_, cb_norm_, ext_.n_embed, cfg_.embed_dim, nullptr)) return -1;
    SDMI_HIP_OK(hipDeviceSynchronize());
  }
  // weights of the four 2x2 phase convs of every Upsample conv that may run as them (resample(); derived from the packed fp16 weights: not part
  // of the blob, re-derived whenever the weights were set again).  Mixed precision only: the full mode's weights are split-fp16.
  if (!full()) {
    SDMI_HIP_OK(hipDeviceSynchronize());           // (set_weight packed on the caller's stream)
    for (auto& L : dec_) {
      if (L.kind != V_UP || L.cin % 64 != 0 || L.split) continue;     // (a split layer's weights are packed [w_hi | w_hi | w_lo])
      if (store_.alloc((void**)&L.w_up_phase, (size_t)16 * L.cout * L.cin * sizeof(f16))) return -1;
      if (launch_up_phase_weights(L.w16[0], L.w_up_phase, L.cout, L.cin, nullptr)) return -1;
    }
    SDMI_HIP_OK(hipDeviceSynchronize());
  }
  finalized_ = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------
struct VFwd : FwdBase {
  static constexpr float EPS = 1e-6f;        // Normalize(): GroupNorm(32, eps=1e-6)   model.py:37-38
  bool full = false;                         // the running layer takes split-fp16 operands (VLayer::split; run_layer sets it)
  bool flash = false;                        // the handle has level attention (Vae::attn_level_mask_ != 0): attn_block_flash, not attn_block

  // SDMI_PRECISION_FULL: the 3x3 convs take split-fp16 operands (FwdBase::split3 against weights packed W_CONV_SPLIT3; the `_lo` buffers
  // below are null in the mixed mode), and no GEMM is split along K: every output element is then summed over K in one fixed order
  // whatever M is, so a sample's result does not depend on the batch it is decoded in (the split is otherwise chosen from the number
  // of workgroups)
  void gemm(IGemmParams& p) { if (full) p.splitk = 1; FwdBase::gemm(p); }

  // AttnBlock with one head of d = C: q, k, v (bias inside its GEMM) as split GEMMs into fp32, scattered to q / k / V^T hi | lo, one
  // split-fp16 flash attention launch, proj_out as a split GEMM with the residual
  Act attn_block_full(VLayer& L, const Act& x) {
    const int H = x.H, W = x.W, N = H * W, M = B * N, C = L.cin;
    const int Np = (int)round_up(N, 8);
    const size_t mark = scratch.off;
    f16* a = S<f16>((size_t)M * C); f16* a_lo = S<f16>((size_t)M * C);          // GroupNorm output, then the attention output
    float* y = S<float>((size_t)M * C);
    f16* qkv[3]; f16* qkv_lo[3];
    for (int i = 0; i < 3; ++i) {
      const size_t n = i == 2 ? (size_t)B * C * Np : (size_t)M * C;
      qkv[i] = S<f16>(n); qkv_lo[i] = S<f16>(n);
    }
    groupnorm(x, nullptr, L.f32[0], L.f32[1], EPS, 0, a, nullptr, nullptr, a_lo, nullptr);
    for (int i = 0; i < 3; ++i) {
      IGemmParams p = dense1x1(a, a_lo, M, C, L.w16[i], C, N, true);
      p.bias = L.f32[2 + i]; p.out_f32 = y; p.ldo = C;
      gemm(p);
      if (!dry && !rc) ok(launch_split_heads(y, C, 0, qkv[i], qkv_lo[i], i == 2 ? 1 : 0, B, N, Np, 1, C, s));
    }
    AttnSplitParams ap = AttnSplitParams();
    ap.q = qkv[0]; ap.q_lo = qkv_lo[0]; ap.k = qkv[1]; ap.k_lo = qkv_lo[1]; ap.vt = qkv[2]; ap.vt_lo = qkv_lo[2]; ap.out = a; ap.out_lo = a_lo;
    ap.BH = B; ap.heads = 1; ap.nq = N; ap.nkv = N; ap.nkv_pad = Np; ap.d = C; ap.scale = 1.0f / sqrtf((float)C);
    if (!dry && !rc) ok(launch_attention_split16(ap, s));
    Act out; out.p = P<float>((size_t)M * C); out.C = C; out.H = H; out.W = W;
    {
      IGemmParams p = dense1x1(a, a_lo, M, C, L.w16[3], C, N, true);
      p.bias = L.f32[5]; p.residual = x.p; p.ldr = C; p.out_f32 = out.p; p.ldo = C;
      gemm(p);
    }
    scratch.off = mark;
    return out;
  }

  Act res_block(VLayer& L, const Act& x) {   // model.py:119-141
    const int H = x.H, W = x.W, M = B * H * W, Cin = L.cin, Cout = L.cout;
    if (x.C != Cin) ok(fail("res block channel mismatch at " + L.prefix));
    const size_t mark = scratch.off;
    const bool nin = Cin != Cout;
    const bool p1 = precise_1x1 || full;       // nin_shortcut as a split-fp16 GEMM
    f16* a = S<f16>((size_t)M * Cin);
    f16* a_lo = full ? S<f16>((size_t)M * Cin) : nullptr;
    f16* raw = nin ? S<f16>((size_t)M * Cin) : nullptr;
    f16* raw_lo = (nin && p1) ? S<f16>((size_t)M * Cin) : nullptr;
    float* h = S<float>((size_t)M * Cout);
    Act out; out.p = P<float>((size_t)M * Cout); out.C = Cout; out.H = H; out.W = W;
    groupnorm(x, nullptr, L.f32[0], L.f32[1], EPS, 1, a, nullptr, raw, a_lo, raw_lo);
    {
      IGemmParams p = conv3(a, Cin, H, W, H, W, 1, 0, L.w16[0], Cout);
      if (full) split3(p, a, a_lo, Cin);
      p.bias = L.f32[2]; p.out_f32 = h; p.ldo = Cout;
      gemm(p);
    }
    const float* residual = x.p;
    if (nin) {
      IGemmParams p = dense1x1(raw, raw_lo, M, Cin, L.w16[2], Cout, H * W, p1);
      p.bias = L.f32[6]; p.out_f32 = out.p; p.ldo = Cout;
      gemm(p);
      residual = out.p;
    }
    Act hact; hact.p = h; hact.C = Cout; hact.H = H; hact.W = W;
    f16* a2 = S<f16>((size_t)M * Cout);
    f16* a2_lo = full ? S<f16>((size_t)M * Cout) : nullptr;
    groupnorm(hact, nullptr, L.f32[3], L.f32[4], EPS, 1, a2, nullptr, nullptr, a2_lo, nullptr);
    {
      IGemmParams p = conv3(a2, Cout, H, W, H, W, 1, 0, L.w16[1], Cout);
      if (full) split3(p, a2, a2_lo, Cout);
      p.bias = L.f32[5]; p.residual = residual; p.ldr = Cout; p.out_f32 = out.p; p.ldo = Cout;
      gemm(p);
    }
    scratch.off = mark;
    return out;
  }

  Act attn_block(VLayer& L, const Act& x) {  // model.py:172-202
    const int H = x.H, W = x.W, N = H * W, M = B * N, C = L.cin;
    if (N % 64) ok(fail("first-stage attention needs H*W % 64 == 0 (latent sides multiples of 8)"));
    const float scale = 1.0f / sqrtf((float)C);
    const size_t mark = scratch.off;
    f16* xn = S<f16>((size_t)M * C);
    groupnorm(x, nullptr, L.f32[0], L.f32[1], EPS, 0, xn, nullptr, nullptr);
    f16* q = S<f16>((size_t)M * C);
    f16* k = S<f16>((size_t)M * C);
    f16* vt = S<f16>((size_t)M * C);      // per image [C][N]
    f16* ao = S<f16>((size_t)M * C);
    for (int i = 0; i < 2; ++i) {         // q = xn Wq^T + bq,  k = xn Wk^T + bk
      IGemmParams p = dense(xn, M, C, L.w16[i], C, N);
      p.bias = L.f32[2 + i]; p.out_f16 = i ? k : q; p.ldo = C; p.splitk = 1;
      gemm(p);
    }
    const int QC = std::min(N, 2048);     // query rows per chunk: S (fp32) + P (fp16) <= 48 MB at N = 4096
    float* Sm = S<float>((size_t)QC * N);
    f16* Pm = S<f16>((size_t)QC * N);
    for (int b = 0; b < B; ++b) {
      {   // v^T [C][N] = Wv [C][C] x xn_b[N][C]^T  (the bias is added after P v: softmax rows sum to 1)
        IGemmParams p = dense(L.w16[2], C, C, xn + (size_t)b * N * C, N, C);
        p.out_f16 = vt + (size_t)b * N * C; p.ldo = N; p.splitk = 1;
        gemm(p);
      }
      for (int r0 = 0; r0 < N; r0 += QC) {
        const int rows = std::min(QC, N - r0);
        {
          IGemmParams p = dense(q + ((size_t)b * N + r0) * C, rows, C, k + (size_t)b * N * C, N, rows);
          p.out_f32 = Sm; p.ldo = N; p.splitk = 1;
          gemm(p);
        }
        if (!dry && !rc) ok(launch_softmax_rows(Sm, Pm, rows, N, N, N, scale, s));
        {
          IGemmParams p = dense(Pm, rows, N, vt + (size_t)b * N * C, C, rows);
          p.bias = L.f32[4]; p.out_f16 = ao + ((size_t)b * N + r0) * C; p.ldo = C; p.splitk = 1;
          gemm(p);
        }
      }
    }
    Act out; out.p = P<float>((size_t)M * C); out.C = C; out.H = H; out.W = W;
    {
      IGemmParams p = dense(ao, M, C, L.w16[3], C, N);
      p.bias = L.f32[5]; p.residual = x.p; p.ldr = C; p.out_f32 = out.p; p.ldo = C;
      gemm(p);
    }
    scratch.off = mark;
    return out;
  }

  // AttnBlock on a handle with level attention (Vae::attn_level_mask_ != 0), mixed precision, level and mid block alike: GroupNorm, the
  // q / k / v GEMMs scattering their fp16 outputs straight into the flash kernels' layouts (EPI_HEADS with one head of d = C: q, k as
  // [B][N][C], v as V^T [B][C][Np]), ONE flash launch (attn.hip up to d = 160, attn_wide.hip for 192 .. 1024: d = 512 on KL-f16),
  // proj_out with the residual.  No S / P buffers (attn_block's are QC x N: 2304 x 2304 at the native 48 x 48 latent, per image and block)
  // and no N % 64 rule: the flash kernels mask the keys past nkv, so any H x W runs.
  // The v bias is added INSIDE the v GEMM (its epilogue, before the fp16 rounding of V^T), where attn_block adds it after P V; the pad
  // columns N .. Np - 1 of V^T are zeroed first, as the kernels' contract asks (AttnParams::vt).
  Act attn_block_flash(VLayer& L, const Act& x) {
    const int H = x.H, W = x.W, N = H * W, M = B * N, C = L.cin;
    const int Np = (int)round_up(N, 8);
    const size_t mark = scratch.off;
    f16* xn = S<f16>((size_t)M * C);
    groupnorm(x, nullptr, L.f32[0], L.f32[1], EPS, 0, xn, nullptr, nullptr);
    f16* qkv[3] = {S<f16>((size_t)M * C), S<f16>((size_t)M * C), S<f16>((size_t)B * C * Np)};
    f16* ao = S<f16>((size_t)M * C);
    if (!dry && !rc && Np != N) {
      hipError_t e = memset_async(qkv[2], 0, (size_t)B * C * Np * sizeof(f16), s);
      if (e != hipSuccess) ok(fail(std::string("hipMemsetAsync: ") + hipGetErrorString(e)));
    }
    for (int i = 0; i < 3; ++i) {
      IGemmParams p = dense(xn, M, C, L.w16[i], C, N);
      p.mode = EPI_HEADS; p.bias = L.f32[2 + i]; p.seg_dst[0] = qkv[i]; p.seg_kind[0] = i == 2 ? 1 : 0;
      p.heads = 1; p.dh = C; p.ntok = N; p.ntok_pad = Np; p.segC = C; p.splitk = 1;
      gemm(p);
    }
    AttnParams a = AttnParams();
    a.q = qkv[0]; a.k = qkv[1]; a.vt = qkv[2]; a.out = ao; a.BH = B; a.heads = 1; a.nq = N; a.nkv = N; a.nkv_pad = Np; a.d = C;
    a.scale = 1.0f / sqrtf((float)C);
    if (!dry && !rc) ok(launch_attention(a, s));
    Act out; out.p = P<float>((size_t)M * C); out.C = C; out.H = H; out.W = W;
    {
      IGemmParams p = dense(ao, M, C, L.w16[3], C, N);
      p.bias = L.f32[5]; p.residual = x.p; p.ldr = C; p.out_f32 = out.p; p.ldo = C;
      gemm(p);
    }
    scratch.off = mark;
    return out;
  }

  Act resample(VLayer& L, const Act& x, bool up) {   // model.py:41-79
    const int Hin = x.H, Win = x.W, C = x.C;
    if (!up && ((Hin | Win) & 1)) ok(fail("first-stage Downsample needs even H and W"));
    const int Hout = up ? 2 * Hin : Hin / 2, Wout = up ? 2 * Win : Win / 2;
    const size_t mark = scratch.off;
    const int64_t n = (int64_t)B * Hin * Win * C;
    f16* x16 = S<f16>((size_t)n);
    f16* x16_lo = full ? S<f16>((size_t)n) : nullptr;
    if (!dry && !rc) ok(launch_cast_f16(x.p, x16, x16_lo, n, s));
    Act out; out.p = P<float>((size_t)B * Hout * Wout * C); out.C = C; out.H = Hout; out.W = Wout;
    IGemmParams p = conv3(x16, C, Hin, Win, Hout, Wout, up ? 1 : 2, up ? 1 : 0, L.w16[0], C);
    if (full) split3(p, x16, x16_lo, C);
    if (!up) p.pad = 0;                   // F.pad(x, (0,1,0,1)) + conv(stride 2, padding 0)
    p.bias = L.f32[0]; p.out_f32 = out.p; p.ldo = C;
    // nearest x2 + 3x3 as the four 2x2 phase convs of one launch (igemm KIND_2X2: 4 / 9 of the MACs) where the tuning table says that wins
    if (up && !full && L.w_up_phase && igemm_plans_up_phase(p)) p = up_phase_of(p, L.w_up_phase);
    gemm(p);
    scratch.off = mark;
    return out;
  }

  Act run_layer(VLayer& L, const Act& x) {
    full = L.split;                            // (every layer of a full-precision handle; the layers Vae::build names on a mixed one)
    switch (L.kind) {
      case V_RES: return res_block(L, x);
      case V_ATTN:
        if (full) return attn_block_full(L, x);
        // a handle without level attention keeps the GEMM / softmax / GEMM form wherever it runs (H W % 64 == 0: the launches it always
        // made); a token count it refuses (KL-f4 / VQ-f4 at a 6 x 10 latent: 60 tokens) takes the flash form where the width has a kernel
        if (flash || ((x.H * x.W) % 64 != 0 && mixed_attn_width(L.cin))) return attn_block_flash(L, x);
        return attn_block(L, x);
      case V_UP: return resample(L, x, true);
      case V_DOWN: return resample(L, x, false);
    }
    return x;
  }
};

// two passes over one executor: the first (dry) sizes the persist / scratch arenas, the second launches
template <class Body>
static int run_two_pass(VFwd& f, bool dry, void* workspace, int64_t ws_bytes, int64_t* bytes_needed, Body body) {
  int64_t persist_bytes = 0, scratch_bytes = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool d = pass == 0;
    if (pass == 1 && dry) break;
    f.dry = d; f.rc = 0;
    f.persist = Arena(); f.scratch = Arena();
    f.persist.dry = f.scratch.dry = d;
    if (!d) {
      SDMI_CHECK(persist_bytes + scratch_bytes <= ws_bytes, "workspace too small: need " +
                 std::to_string(persist_bytes + scratch_bytes) + " bytes, got " + std::to_string(ws_bytes));
      SDMI_CHECK(workspace != nullptr, "workspace is NULL");
      f.persist.base = (char*)workspace; f.persist.cap = (size_t)persist_bytes;
      f.scratch.base = (char*)workspace + persist_bytes; f.scratch.cap = (size_t)scratch_bytes;
    }
    if (f.begin_pass((int64_t)8 << 20)) return -1;
    if (body(f)) return -1;
    if (f.rc) return f.rc;
    if (d) {
      persist_bytes = (int64_t)round_up((int64_t)f.persist.peak, 4096) + 4096;
      scratch_bytes = (int64_t)round_up((int64_t)f.scratch.peak, 4096) + 4096;
      if (bytes_needed) *bytes_needed = persist_bytes + scratch_bytes;
    } else {
      SDMI_CHECK(!f.persist.overflow && !f.scratch.overflow, "internal: arena overflow");
    }
  }
  return 0;
}

int Vae::decode(const float* z, float z_scale, float* img, int B, int H, int W, void* workspace, int64_t ws_bytes,
                hipStream_t stream, bool dry, int64_t* bytes_needed, bool quantize) {
  SDMI_CHECK(parts_ & 1, "this handle was created without the decoder");
  SDMI_CHECK(!quantize || ext_.n_embed > 0, "this first stage has no codebook (n_embed = 0): nothing to quantize");
  SDMI_CHECK(dry || finalized_, "sdmi_vae_finalize() has not succeeded yet");
  SDMI_CHECK(B >= 1 && B <= 8, "batch must be 1..8 per call");
  SDMI_CHECK(H >= 1 && W >= 1, "bad shape");
  SDMI_CHECK(dry || (z != nullptr && img != nullptr), "z / img is NULL");
  VFwd f;
  f.s = stream; f.B = B; f.zero = store_.zero(); f.precise_1x1 = precise_1x1_; f.full = full(); f.flash = attn_level_mask_ != 0;
  const int n = cfg_.n_levels, c_in = cfg_.ch * cfg_.ch_mult[n - 1];
  return run_two_pass(f, dry, workspace, ws_bytes, bytes_needed, [&](VFwd& f) -> int {
    const bool d = f.dry;
    float* zq = f.P<float>((size_t)B * cfg_.z_channels * H * W);
    // (VQ: quantize(z_scale * z) first -- the workspace always has room for it, so its size does not depend on the flag)
    float* zc = ext_.n_embed > 0 ? f.P<float>((size_t)B * cfg_.embed_dim * H * W) : nullptr;
    if (!d && quantize) {
      if (launch_vq_quantize(z, z_scale, cb_, cb_norm_, ext_.n_embed, cfg_.embed_dim, zc, nullptr, B, H * W, stream)) return -1;
      if (launch_pointwise_nchw(zc, pq_w_, pq_b_, zq, B, cfg_.embed_dim, cfg_.z_channels, H * W, 1.0f, stream)) return -1;
    } else if (!d && launch_pointwise_nchw(z, pq_w_, pq_b_, zq, B, cfg_.embed_dim, cfg_.z_channels, H * W, z_scale, stream)) return -1;
    Act x; x.p = f.P<float>((size_t)B * H * W * c_in); x.C = c_in; x.H = H; x.W = W;
    if (!d && launch_conv_in(zq, dci_w_, dci_b_, x.p, B, cfg_.z_channels, H, W, c_in, stream)) return -1;
    for (auto& L : dec_) x = f.run_layer(L, x);
    if (f.rc) return f.rc;
    float* hn = f.S<float>((size_t)B * x.H * x.W * x.C);
    f.groupnorm(x, nullptr, dno_g_, dno_b_, VFwd::EPS, 1, nullptr, hn, nullptr);
    if (!d && !f.rc && launch_conv_out(hn, dco_w_, dco_b_, img, B, x.H, x.W, x.C, cfg_.out_ch, stream)) return -1;
    return f.rc;
  });
}

int Vae::encode(const float* img, float* moments, int B, int H, int W, void* workspace, int64_t ws_bytes,
                hipStream_t stream, bool dry, int64_t* bytes_needed) {
  SDMI_CHECK(parts_ & 2, "this handle was created without the encoder");
  SDMI_CHECK(dry || finalized_, "sdmi_vae_finalize() has not succeeded yet");
  SDMI_CHECK(B >= 1 && B <= 8, "batch must be 1..8 per call");
  const int fct = factor();
  SDMI_CHECK(H >= fct && W >= fct && H % fct == 0 && W % fct == 0, "H and W must be multiples of 2^(levels-1)");
  SDMI_CHECK(dry || (img != nullptr && moments != nullptr), "img / moments is NULL");
  VFwd f;
  f.s = stream; f.B = B; f.zero = store_.zero(); f.precise_1x1 = precise_1x1_; f.full = full(); f.flash = attn_level_mask_ != 0;
  return run_two_pass(f, dry, workspace, ws_bytes, bytes_needed, [&](VFwd& f) -> int {
    const bool d = f.dry;
    Act x; x.p = f.P<float>((size_t)B * H * W * cfg_.ch); x.C = cfg_.ch; x.H = H; x.W = W;
    if (!d && launch_conv_in(img, eci_w_, eci_b_, x.p, B, cfg_.in_channels, H, W, cfg_.ch, stream)) return -1;
    for (auto& L : enc_) x = f.run_layer(L, x);
    if (f.rc) return f.rc;
    float* hn = f.S<float>((size_t)B * x.H * x.W * x.C);
    f.groupnorm(x, nullptr, eno_g_, eno_b_, VFwd::EPS, 1, nullptr, hn, nullptr);
    const int zc2 = enc_zc();
    float* mo = f.S<float>((size_t)B * zc2 * x.H * x.W);
    if (!d && !f.rc && launch_conv_out(hn, eco_w_, eco_b_, mo, B, x.H, x.W, x.C, zc2, stream)) return -1;
    if (!d && !f.rc && launch_pointwise_nchw(mo, q_w_, q_b_, moments, B, zc2, enc_ed(), x.H * x.W, 1.0f, stream))
      return -1;
    return f.rc;
  });
}

}  // namespace sdmi
