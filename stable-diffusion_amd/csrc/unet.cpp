// UNet executor: the static launch graph of UNetModel.forward
// (ldm/modules/diffusionmodules/openaimodel.py:710-742) over the gfx950 kernels of this library.
//
// Data layout in HBM (per forward call, B = CFG batch):
//   * residual stream and skip stack: fp32 NHWC [B*H*W][C] (rounded nowhere; see DESIGN.md "precision")
//   * MFMA A operands (normalised activations, q/k/v^T, GEGLU output): fp16, written once by the producing
//     kernel and read once by the consuming GEMM
//   * weights: fp16 [N][K] (K = ky,kx,cin), packed once at load; norm/bias/time-embedding parameters fp32
//   * workspace = [persist | scratch]: every layer output lives in `persist` until the call ends (skip stack),
//     `scratch` is rewound after each layer so temporaries stay in the 256 MB Infinity Cache.
#include "unet.h"

extern "C" char** environ;       // (the launch tapes hash the SDMI_* knobs)
#include "prof.h"
#include "split16.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

namespace sdmi {

// ------------------------------------------------------------------------------------------------------
// construction: mirror of UNetModel.__init__ (openaimodel.py:443-692) for the SD-v1 family
// ------------------------------------------------------------------------------------------------------
static bool in_list(const int* v, int n, int x) {
  for (int i = 0; i < n; ++i)
    if (v[i] == x) return true;
  return false;
}

thread_local Tape* g_tape_rec = nullptr;

namespace {
// FNV-1a over every SDMI_* entry of the environment: the knobs the library reads per call / per launch are part of a tape's identity
// (the tests flip them between two forwards of one shape)
uint64_t sdmi_env_hash() {
  uint64_t h = 1469598103934665603ull;
  for (char** e = environ; e && *e; ++e) {
    if (strncmp(*e, "SDMI_", 5) != 0) continue;
    for (const char* c = *e; *c; ++c) { h ^= (unsigned char)*c; h *= 1099511628211ull; }
    h ^= 0xff; h *= 1099511628211ull;
  }
  return h;
}
struct TapeRecGuard {         // recording ends with the scope, whatever path leaves it
  explicit TapeRecGuard(Tape* t) { g_tape_rec = t; }
  ~TapeRecGuard() { g_tape_rec = nullptr; }
};
}  // namespace

int UNet::build(const sdmi_unet_cfg& c, int precision, const sdmi_unet_ext* ext, unsigned flags) {
  cfg_ = c;
  precision_ = precision;
  if (ext) ext_ = *ext;
  SDMI_CHECK((flags & ~((unsigned)SDMI_UNET_SCALE_SHIFT_NORM | (unsigned)SDMI_UNET_NUM_HEAD_CHANNELS_MASK)) == 0, "unknown UNet creation flag");
  scale_shift_ = (flags & SDMI_UNET_SCALE_SHIFT_NORM) != 0;
  // num_head_channels (openaimodel.py:532-535,561-563: heads = ch // num_head_channels per AttentionBlock) rides in the flag word
  num_head_channels_ = (int)((flags & SDMI_UNET_NUM_HEAD_CHANNELS_MASK) >> SDMI_UNET_NUM_HEAD_CHANNELS_SHIFT);
  // (the family this executor path is validated for: the unconditional LDMs -- AttentionBlocks and resampling ResBlocks)
  SDMI_CHECK(!scale_shift_ || (ext_.attention_block == 1 && ext_.resblock_updown == 1),
             "SDMI_UNET_SCALE_SHIFT_NORM needs attention_block = 1 and resblock_updown = 1");
  SDMI_CHECK(ext_.attention_block == 0 || ext_.attention_block == 1, "attention_block must be 0 (SpatialTransformer) or 1 (AttentionBlock)");
  SDMI_CHECK(ext_.resblock_updown == 0 || ext_.resblock_updown == 1, "resblock_updown must be 0 or 1");
  SDMI_CHECK(c.n_levels >= 1 && c.n_levels <= 8 && c.n_attention_resolutions >= 0 && c.n_attention_resolutions <= 8,
             "bad level / attention_resolutions count");
  // (with attention_block = 0 the SpatialTransformers take heads = ch / num_head_channels, dim_head = num_head_channels: openaimodel.py:542-549,
  // the retrieval-augmented and layout-to-image UNets), at the one head dim that family is tested at
  SDMI_CHECK(num_head_channels_ == 0 || ext_.attention_block == 1 || num_head_channels_ == 32,
             "num_head_channels " + std::to_string(num_head_channels_) + " on a SpatialTransformer handle (attention_block = 0): only 32 is admitted "
             "(the head dim this family is tested at)");
  SDMI_CHECK(num_head_channels_ == 0 || ext_.attention_block == 1 || c.num_heads < 1,
             "num_head_channels together with num_heads on a SpatialTransformer handle: one of the two (pass num_heads = -1 with num_head_channels)");
  // AttentionBlock UNets: every GEMM source is a multiple of 32 channels (a source of 32 (mod 64) ends in a half k-tile, igemm_kernel.h);
  // the SpatialTransformer's row-strip chains and LayerNorm fold keep whole 64-channel chunks
  if (ext_.attention_block == 1) SDMI_CHECK(c.model_channels > 0 && c.model_channels % 32 == 0, "model_channels must be a multiple of 32 on this path");
  else SDMI_CHECK(c.model_channels % 64 == 0, "model_channels must be a multiple of 64 on this path (SpatialTransformer family)");
  if (has_ctx()) SDMI_CHECK(c.context_dim % 64 == 0, "context_dim must be a multiple of 64 on this path");
  else SDMI_CHECK(c.context_dim == 0, "a UNet of AttentionBlocks has no cross-attention: context_dim must be 0");
  SDMI_CHECK((c.num_heads >= 1 || num_head_channels_ > 0) && c.transformer_depth >= 1, "num_heads / transformer_depth");
  const int mc = c.model_channels;
  te_ = 4 * mc;
  if (const char* e = getenv("SDMI_FUSE_GN_STATS")) fuse_gn_stats_ = atoi(e) != 0;
  if (const char* e = getenv("SDMI_LN_FOLD")) ln_fold_ = atoi(e) != 0;
  if (const char* e = getenv("SDMI_LN_FOLD_MIN_ROWS")) ln_fold_min_rows_ = atoi(e);

  int cur_ds = 1;               // downsample factor of the layer being added (ds below; the middle block sits at the deepest one)
  auto add_res = [&](const std::string& p, int cin, int cout) {
    Layer L; L.kind = L_RES; L.prefix = p; L.cin = cin; L.cout = cout;
    L.emb_off = emb_total_; emb_total_ += scale_shift_ ? 2 * cout : cout;      // (scale-shift: [scale | shift], th.chunk(emb_out, 2, dim=1))
    L.p1x1 = full() || (precise_1x1_ && cur_ds < precise_1x1_max_ds_);
    L.precise3 = full();        // (every ResBlock's channel counts are multiples of 32: the split-fp16 3x3 conv takes them)
    return L;
  };
  auto add_attn = [&](const std::string& p, int ch) {
    Layer L; L.kind = has_ctx() ? L_ATTN : L_ATTN_LEGACY; L.prefix = p; L.cin = ch; L.cout = ch;
    if (num_head_channels_ > 0) { L.heads = ch / num_head_channels_; L.dh = num_head_channels_; }
    else { L.heads = c.num_heads; L.dh = ch / c.num_heads; }
    L.attn_index = n_attn_++;
    L.p1x1 = full() || (precise_1x1_ && cur_ds < precise_1x1_max_ds_);
    return L;
  };
  auto add_updown = [&](const std::string& p, int ch, int dir) {     // resblock_updown: ResBlock(ch, down=True / up=True)
    Layer L = add_res(p, ch, ch);
    L.updown = dir;
    return L;
  };

  {
    Layer L; L.kind = L_CONV_IN; L.prefix = "input_blocks.0.0"; L.cin = c.in_channels; L.cout = mc;
    input_blocks_.push_back({L});
  }
  std::vector<int> chans{mc};
  int ch = mc, ds = 1;
  for (int level = 0; level < c.n_levels; ++level) {
    const int mult = c.channel_mult[level];
    for (int r = 0; r < c.num_res_blocks; ++r) {
      const int n = (int)input_blocks_.size();
      std::vector<Layer> blk;
      cur_ds = ds;
      blk.push_back(add_res("input_blocks." + std::to_string(n) + ".0", ch, mult * mc));
      ch = mult * mc;
      if (in_list(c.attention_resolutions, c.n_attention_resolutions, ds))
        blk.push_back(add_attn("input_blocks." + std::to_string(n) + ".1", ch));
      input_blocks_.push_back(blk);
      chans.push_back(ch);
    }
    if (level != c.n_levels - 1) {
      const int n = (int)input_blocks_.size();
      Layer L; L.kind = L_DOWN; L.prefix = "input_blocks." + std::to_string(n) + ".0"; L.cin = ch; L.cout = ch;
      if (ext_.resblock_updown) { cur_ds = ds; L = add_updown(L.prefix, ch, 1); }
      input_blocks_.push_back({L});
      chans.push_back(ch);
      ds *= 2;
    }
  }
  cur_ds = ds;
  middle_.push_back(add_res("middle_block.0", ch, ch));
  middle_.push_back(add_attn("middle_block.1", ch));
  middle_.push_back(add_res("middle_block.2", ch, ch));
  for (int level = c.n_levels - 1; level >= 0; --level) {
    const int mult = c.channel_mult[level];
    for (int i = 0; i <= c.num_res_blocks; ++i) {
      const int ich = chans.back(); chans.pop_back();
      const int n = (int)output_blocks_.size();
      std::vector<Layer> blk;
      cur_ds = ds;
      blk.push_back(add_res("output_blocks." + std::to_string(n) + ".0", ch + ich, mc * mult));
      ch = mc * mult;
      if (in_list(c.attention_resolutions, c.n_attention_resolutions, ds))
        blk.push_back(add_attn("output_blocks." + std::to_string(n) + "." + std::to_string(blk.size()), ch));
      if (level && i == c.num_res_blocks) {
        Layer L; L.kind = L_UP; L.prefix = "output_blocks." + std::to_string(n) + "." + std::to_string(blk.size());
        L.cin = ch; L.cout = ch;
        if (ext_.resblock_updown) L = add_updown(L.prefix, ch, -1);
        blk.push_back(L);
        ds /= 2;
      }
      output_blocks_.push_back(blk);
    }
  }

  {                          // (the attention kernels are instantiated per head dim)
    if (for_each_layer([&](const Layer& L) -> int {
      // wide heads (num_heads = 1: d_head = C) run on attn_wide.hip; its split-fp16 form attn_wide_split16.hip exists, but this executor
      // does not dispatch to it
      if (L.kind == L_ATTN) {
        SDMI_CHECK(!(full() && L.dh > 160), L.prefix + ": attention head dim " + std::to_string(L.dh) +
                   " has no full-precision kernel (split-fp16 attention is instantiated up to head dim 160)");
        if (num_head_channels_ > 0)
          SDMI_CHECK(L.cin % num_head_channels_ == 0, L.prefix + ": " + std::to_string(L.cin) + " channels not divisible by num_head_channels " +
                     std::to_string(num_head_channels_));
        return 0;
      }
      if (L.kind != L_ATTN_LEGACY) return 0;
      if (num_head_channels_ > 0)
        SDMI_CHECK(L.cin % num_head_channels_ == 0, L.prefix + ": " + std::to_string(L.cin) + " channels not divisible by num_head_channels " +
                   std::to_string(num_head_channels_));
      else SDMI_CHECK(L.cin % c.num_heads == 0, L.prefix + ": channels not divisible by num_heads");
      SDMI_CHECK(L.dh == 24 || L.dh == 32 || L.dh == 40 || L.dh == 48 || L.dh == 64 || L.dh == 80 || L.dh == 96 || L.dh == 128 || L.dh == 160,
                 L.prefix + ": attention head dim " + std::to_string(L.dh) + " not instantiated (24/32/40/48/64/80/96/128/160)");
      return 0;
    })) return -1;
  }

  // the last ResBlock (output_blocks.<last>.0: its two 3x3 convs are the largest single contributors to the eps error)
  if (precise_last_res_ && !output_blocks_.empty() && output_blocks_.back()[0].kind == L_RES)
    output_blocks_.back()[0].precise3 = true;

  // ---- expected state_dict entries and where each one is packed to -------------------
  const int64_t TE = te_;
  store_.expect("time_embed.0.weight", {TE, mc}, W_F32, &te_w0_);
  store_.expect("time_embed.0.bias", {TE}, W_F32, &te_b0_);
  store_.expect("time_embed.2.weight", {TE, TE}, W_F32, &te_w2_);
  store_.expect("time_embed.2.bias", {TE}, W_F32, &te_b2_);
  for_each_layer([&](Layer& L) -> int {
    const std::string& p = L.prefix;
    const int64_t ci = L.cin, co = L.cout;
    switch (L.kind) {
      case L_CONV_IN:
        store_.expect(p + ".weight", {co, ci, 3, 3}, W_F32, &L.w32[0]);
        store_.expect(p + ".bias", {co}, W_F32, &L.f32[0]);
        break;
      case L_RES:
        store_.expect(p + ".in_layers.0.weight", {ci}, W_F32, &L.f32[0]);
        store_.expect(p + ".in_layers.0.bias", {ci}, W_F32, &L.f32[1]);
        store_.expect(p + ".in_layers.2.weight", {co, ci, 3, 3}, L.precise3 ? W_CONV_SPLIT3 : W_CONV, &L.w16[0]);
        store_.expect(p + ".in_layers.2.bias", {co}, W_F32, &L.f32[2]);
        store_.expect(p + ".emb_layers.1.weight", {scale_shift_ ? 2 * co : co, TE}, W_F32_ROWS, &emb_w_, L.emb_off, emb_total_);
        store_.expect(p + ".emb_layers.1.bias", {scale_shift_ ? 2 * co : co}, W_F32_ROWS, &emb_b_, L.emb_off, emb_total_);
        store_.expect(p + ".out_layers.0.weight", {co}, W_F32, &L.f32[3]);
        store_.expect(p + ".out_layers.0.bias", {co}, W_F32, &L.f32[4]);
        store_.expect(p + ".out_layers.3.weight", {co, co, 3, 3}, L.precise3 ? W_CONV_SPLIT3 : W_CONV, &L.w16[1]);
        store_.expect(p + ".out_layers.3.bias", {co}, W_F32, &L.f32[5]);
        if (ci != co) {
          store_.expect(p + ".skip_connection.weight", {co, ci, 1, 1}, L.p1x1 ? W_SPLIT3 : W_CONV, &L.w16[2]);
          store_.expect(p + ".skip_connection.bias", {co}, W_F32, &L.f32[6]);
        }
        break;
      case L_ATTN: {
        const int64_t C = ci, CD = cfg_.context_dim;
        store_.expect(p + ".norm.weight", {C}, W_F32, &L.f32[0]);
        store_.expect(p + ".norm.bias", {C}, W_F32, &L.f32[1]);
        store_.expect(p + ".proj_in.weight", {C, C, 1, 1}, L.p1x1 ? W_SPLIT3 : W_CONV, &L.w16[0]);
        store_.expect(p + ".proj_in.bias", {C}, W_F32, &L.f32[2]);
        store_.expect(p + ".proj_out.weight", {C, C, 1, 1}, L.p1x1 ? W_SPLIT3 : W_CONV, &L.w16[1]);
        store_.expect(p + ".proj_out.bias", {C}, W_F32, &L.f32[3]);
        L.tb.resize(cfg_.transformer_depth);
        for (int d = 0; d < cfg_.transformer_depth; ++d) {
          TBlock& T = L.tb[d];
          const std::string t = p + ".transformer_blocks." + std::to_string(d);
          // full mode: every linear split-fp16 ([rows][3 K] = [hi | hi | lo]), the GEGLU projection in the reference's column order
          const WKind lin = full() ? W_SPLIT3_ROWS : W_ROWS16;
          store_.expect(t + ".attn1.to_q.weight", {C, C}, lin, &T.wqkv, 0, 3 * (int)C);
          store_.expect(t + ".attn1.to_k.weight", {C, C}, lin, &T.wqkv, (int)C, 3 * (int)C);
          store_.expect(t + ".attn1.to_v.weight", {C, C}, lin, &T.wqkv, 2 * (int)C, 3 * (int)C);
          store_.expect(t + ".attn1.to_out.0.weight", {C, C}, lin, &T.wo1);
          store_.expect(t + ".attn1.to_out.0.bias", {C}, W_F32, &T.bo1);
          store_.expect(t + ".attn2.to_q.weight", {C, C}, lin, &T.wq2);
          // round 6: the context K / V projections as 3-pass split-fp16 (k_hi w_hi + k_lo w_hi + k_hi w_lo, one K-concatenated GEMM): the
          // context is the one operand of the call with channel outliers by construction (CLIP's last_hidden_state has channels at
          // |x| ~ 30) and its fp16 rounding was the error class that grew most (11x) on the outlier goldens (tools/precision_emul.py);
          // computed once per prompt and cached for all 51 calls, so the extra passes cost nothing per UNet call
          store_.expect(t + ".attn2.to_k.weight", {C, CD}, precise_kv_ ? W_SPLIT3_ROWS : W_ROWS16, &T.wkv2, 0, 2 * (int)C);
          store_.expect(t + ".attn2.to_v.weight", {C, CD}, precise_kv_ ? W_SPLIT3_ROWS : W_ROWS16, &T.wkv2, (int)C, 2 * (int)C);
          store_.expect(t + ".attn2.to_out.0.weight", {C, C}, lin, &T.wo2);
          store_.expect(t + ".attn2.to_out.0.bias", {C}, W_F32, &T.bo2);
          store_.expect(t + ".ff.net.0.proj.weight", {8 * C, C}, full() ? W_SPLIT3 : W_GEGLU_W, &T.wgg);
          store_.expect(t + ".ff.net.0.proj.bias", {8 * C}, full() ? W_F32 : W_GEGLU_B, &T.bgg);
          store_.expect(t + ".ff.net.2.weight", {C, 4 * C}, lin, &T.wff2);
          store_.expect(t + ".ff.net.2.bias", {C}, W_F32, &T.bff2);
          store_.expect(t + ".norm1.weight", {C}, W_F32, &T.ln[0]);
          store_.expect(t + ".norm1.bias", {C}, W_F32, &T.ln[1]);
          store_.expect(t + ".norm2.weight", {C}, W_F32, &T.ln[2]);
          store_.expect(t + ".norm2.bias", {C}, W_F32, &T.ln[3]);
          store_.expect(t + ".norm3.weight", {C}, W_F32, &T.ln[4]);
          store_.expect(t + ".norm3.bias", {C}, W_F32, &T.ln[5]);
        }
        break;
      }
      case L_ATTN_LEGACY: {      // AttentionBlock (openaimodel.py:302-312): conv1d weights [out][in][1]
        const int64_t C = ci;
        const bool pq = L.p1x1;              // qkv as split-fp16 (the GroupNorm writes hi | lo) where the 1x1 allocation says so
        store_.expect(p + ".norm.weight", {C}, W_F32, &L.f32[0]);
        store_.expect(p + ".norm.bias", {C}, W_F32, &L.f32[1]);
        WeightSlot& qkv = store_.expect(p + ".qkv.weight", {3 * C, C, 1}, W_QKV_LEGACY, &L.w16[0]);
        qkv.heads = L.heads; qkv.split = pq;
        store_.expect(p + ".qkv.bias", {3 * C}, W_QKV_LEGACY_B, &L.f32[2]).heads = L.heads;
        // proj_out reads the attention output: fp16 in the mixed mode, hi | lo in the full mode
        store_.expect(p + ".proj_out.weight", {C, C, 1}, full() ? W_SPLIT3 : W_ROWS16, &L.w16[1]);
        store_.expect(p + ".proj_out.bias", {C}, W_F32, &L.f32[3]);
        break;
      }
      case L_DOWN:
        store_.expect(p + ".op.weight", {co, ci, 3, 3}, full() ? W_CONV_SPLIT3 : W_CONV, &L.w16[0]);
        store_.expect(p + ".op.bias", {co}, W_F32, &L.f32[0]);
        break;
      case L_UP:
        store_.expect(p + ".conv.weight", {co, ci, 3, 3}, full() ? W_CONV_SPLIT3 : W_CONV, &L.w16[0]);
        store_.expect(p + ".conv.bias", {co}, W_F32, &L.f32[0]);
        break;
    }
    return 0;
  });       // NOTE: slots hold pointers into the Layer objects, so the containers must not reallocate after this point.
  store_.expect("out.0.weight", {mc}, W_F32, &out_gamma_);
  store_.expect("out.0.bias", {mc}, W_F32, &out_beta_);
  store_.expect("out.2.weight", {c.out_channels, mc, 3, 3}, W_CONV_OUT, &out_w_);
  store_.expect("out.2.bias", {c.out_channels}, W_F32, &out_b_);
  return 0;
}

UNet::~UNet() {
  if (emb_tab_) (void)hipFree(emb_tab_);
  if (emb_tab_tdev_) (void)hipFree(emb_tab_tdev_);
  for_each_layer([](Layer& L) -> int {      // cross-attention K / V^T caches (ensure_ctx_cache)
    for (auto& T : L.tb) {
      if (T.ck) (void)hipFree(T.ck);
      if (T.cvt) (void)hipFree(T.cvt);
      if (T.ck_lo) (void)hipFree(T.ck_lo);
      if (T.cvt_lo) (void)hipFree(T.cvt_lo);
    }
    return 0;
  });
}

int UNet::set_weight(const char* key, const float* ptr, const int64_t* shape, int ndim, hipStream_t stream) {
  if (int rc = store_.set(key, ptr, shape, ndim, stream)) return rc;
  ++weights_gen_;            // (recorded launch tapes point into the packed buffers / were planned for them)
  finalized_ = false;
  ctx_valid_ = false;      // cached cross-attention K/V were computed with the previous to_k / to_v weights
  drop_timestep_table();   // ... and the timestep table with the previous time_embed / emb_layers weights
  return 0;
}

int UNet::finalize() {
  if (const WeightSlot* m = store_.missing()) return fail("weight not set: " + m->key);
  if (store_.zero_page()) return -1;
  if (reserve_ctx_cache(8, 77)) return -1;       // default K/V capacity (a no-op once reserved)
  // column terms of the GEMMs that fold a LayerNorm of their input rows (derived from the packed weights: not part of the blob)
  {
    SDMI_HIP_OK(hipDeviceSynchronize());          // (the packing kernels ran on the caller's streams; finalize is off the hot path)
    if (for_each_layer([&](Layer& L) -> int {
      if (L.kind != L_ATTN || full()) return 0;        // (full mode: no LayerNorm fold, and its weights are split-fp16)
      const int C = L.cin;
      for (auto& T : L.tb) {
        const int n_[3] = {3 * C, C, 8 * C};
        const f16* w_[3] = {T.wqkv, T.wq2, T.wgg};
        const float* b_[3] = {nullptr, nullptr, T.bgg};
        for (int i = 0; i < 3; ++i) {
          if (store_.alloc((void**)&T.lnf[2 * i], (size_t)n_[i] * sizeof(float)) || store_.alloc((void**)&T.lnf[2 * i + 1], (size_t)n_[i] * sizeof(float)))
            return -1;
          if (launch_ln_fold_prep(w_[i], n_[i], C, C, T.ln[2 * i], T.ln[2 * i + 1], b_[i], T.lnf[2 * i], T.lnf[2 * i + 1], nullptr)) return -1;
        }
        if (ff_tail_supported(C, 32, 32)) {            // (geometry only: rows are checked per call)
          if (store_.alloc((void**)&T.lnf_csd, (size_t)16 * C * sizeof(float))) return -1;
          for (int h = 0; h < 4; ++h) {                 // (default stream, behind the prep kernels above)
            SDMI_HIP_OK(hipMemcpyAsync(T.lnf_csd + (size_t)h * 4 * C, T.lnf[4] + (size_t)h * 2 * C, (size_t)2 * C * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
            SDMI_HIP_OK(hipMemcpyAsync(T.lnf_csd + (size_t)h * 4 * C + 2 * C, T.lnf[5] + (size_t)h * 2 * C, (size_t)2 * C * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
          }
        }
      }
      return 0;
    })) return -1;
    // weights of the four 2x2 phase convs of every Upsample conv that may run as them (Fwd::resample; derived from the packed fp16 weights: not
    // part of the blob, re-derived whenever the weights were set again).  Mixed precision only: the full mode's weights are split-fp16.
    if (for_each_layer([&](Layer& L) -> int {
      if (L.kind != L_UP || full() || L.cin % 64 != 0) return 0;
      if (store_.alloc((void**)&L.w_up_phase, (size_t)16 * L.cout * L.cin * sizeof(f16))) return -1;
      return launch_up_phase_weights(L.w16[0], L.w_up_phase, L.cout, L.cin, nullptr);
    })) return -1;
    SDMI_HIP_OK(hipDeviceSynchronize());
    // bias of a conv2 that carries its block's skip convolution as a tail phase (Fwd::res_block): out_layers.3.bias + skip_connection.bias,
    // one fp32 sum per channel (derived from the set weights: not part of the blob)
    if (for_each_layer([&](Layer& L) -> int {
      if (L.kind != L_RES || L.updown || L.cin == L.cout || !L.f32[5] || !L.f32[6]) return 0;
      std::vector<float> b2((size_t)L.cout), bs((size_t)L.cout);
      SDMI_HIP_OK(hipMemcpy(b2.data(), L.f32[5], b2.size() * sizeof(float), hipMemcpyDeviceToHost));
      SDMI_HIP_OK(hipMemcpy(bs.data(), L.f32[6], bs.size() * sizeof(float), hipMemcpyDeviceToHost));
      for (size_t i = 0; i < b2.size(); ++i) b2[i] += bs[i];
      if (store_.alloc((void**)&L.bias_fold, b2.size() * sizeof(float))) return -1;
      SDMI_HIP_OK(hipMemcpy(L.bias_fold, b2.data(), b2.size() * sizeof(float), hipMemcpyHostToDevice));
      return 0;
    })) return -1;
  }
  ++weights_gen_;
  finalized_ = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------------
// packed-weight blob: the device buffers exactly as set_weight() leaves them, one after another
// in slot order, behind a header that pins the configuration -- loading it skips the fp32 checkpoint and the repack
// ------------------------------------------------------------------------------------------------------
namespace {
struct PackedHeader {
  char magic[8];               // "SDMIPK01"
  int32_t abi, precise_1x1, n_buffers, reserved;
  sdmi_unet_cfg cfg;
  int64_t total_bytes;
};
constexpr int64_t PK_ALIGN = 256;
constexpr int PK_NHC_SHIFT = 16;     // PackedHeader::reserved bits 16..27: num_head_channels of the handle that wrote the blob (the qkv rows are permuted per head)
constexpr int32_t PK_NHC_MASK = 0xfff << PK_NHC_SHIFT;
constexpr int32_t PK_FULL = 4;      // PackedHeader::reserved: written by a full-precision handle (its packed weights are split-fp16)
}  // namespace

int UNet::packed_layout(std::vector<std::pair<void**, size_t>>* bufs, int64_t* total) const {
  int64_t off = (int64_t)round_up((int64_t)sizeof(PackedHeader), PK_ALIGN);
  for (const auto& b : store_.buffers()) {
    if (bufs) bufs->push_back(b);
    off += (int64_t)round_up((int64_t)b.second, PK_ALIGN);
  }
  *total = off;
  return 0;
}

int UNet::export_packed(void* host_buf, int64_t bytes, hipStream_t stream) {
  SDMI_CHECK(finalized_, "export needs a finalized handle");
  std::vector<std::pair<void**, size_t>> bufs;
  int64_t total = 0;
  packed_layout(&bufs, &total);
  SDMI_CHECK(host_buf && bytes >= total, "packed buffer too small: need " + std::to_string(total) + " bytes");
  PackedHeader h{};
  memcpy(h.magic, "SDMIPK01", 8);
  h.abi = SDMI_ABI_VERSION; h.precise_1x1 = precise_1x1_ ? 1 : 0; h.n_buffers = (int32_t)bufs.size(); h.cfg = cfg_;
  h.reserved = (precise_kv_ ? 1 : 0) | (precise_last_res_ ? 2 : 0) | (precise_1x1_max_ds_ << 8);      // (ABI 17: the precision allocation)
  h.reserved |= (ext_.attention_block << 4) | (ext_.resblock_updown << 5) | ((scale_shift_ ? 1 : 0) << 6);   // (sdmi_unet_ext, creation flags: 0 for SD v1)
  h.reserved |= num_head_channels_ << PK_NHC_SHIFT;       // (0 = heads by num_heads)
  if (full()) h.reserved |= PK_FULL;
  h.total_bytes = total;
  memcpy(host_buf, &h, sizeof(h));
  int64_t off = (int64_t)round_up((int64_t)sizeof(PackedHeader), PK_ALIGN);
  for (auto& b : bufs) {
    SDMI_HIP_OK(hipMemcpyAsync((char*)host_buf + off, *b.first, b.second, hipMemcpyDeviceToHost, stream));
    off += (int64_t)round_up((int64_t)b.second, PK_ALIGN);
  }
  SDMI_HIP_OK(hipStreamSynchronize(stream));
  return 0;
}

int UNet::import_packed(const void* host_buf, int64_t bytes, hipStream_t stream) {
  SDMI_CHECK(host_buf && bytes >= (int64_t)sizeof(PackedHeader), "packed blob truncated");
  PackedHeader h;
  memcpy(&h, host_buf, sizeof(h));
  SDMI_CHECK(memcmp(h.magic, "SDMIPK01", 8) == 0, "not a libsdmi packed-weight blob");
  SDMI_CHECK(h.abi == SDMI_ABI_VERSION, "packed blob was written by a different ABI version: repack it");
  SDMI_CHECK(memcmp(&h.cfg, &cfg_, sizeof(cfg_)) == 0, "packed blob was written for a different UNet configuration");
  SDMI_CHECK(((h.reserved & PK_FULL) != 0) == full(), std::string("packed blob was written by a ") +
             ((h.reserved & PK_FULL) ? "full" : "mixed") + "-precision UNet handle and cannot be imported into a " + (full() ? "full" : "mixed") +
             "-precision one: repack it with a handle of this precision");
  SDMI_CHECK((h.precise_1x1 != 0) == precise_1x1_, "packed blob was written with a different precision allocation (split-fp16 1x1 convs)");
  SDMI_CHECK((h.reserved & (7 << 4)) == ((ext_.attention_block << 4) | (ext_.resblock_updown << 5) | ((scale_shift_ ? 1 : 0) << 6)),
             "packed blob was written for a different UNet family (attention_block / resblock_updown / scale-shift norm)");
  SDMI_CHECK(((h.reserved & PK_NHC_MASK) >> PK_NHC_SHIFT) == num_head_channels_,
             "packed blob was written for num_head_channels " + std::to_string((h.reserved & PK_NHC_MASK) >> PK_NHC_SHIFT) + ", this handle has " +
             std::to_string(num_head_channels_) + ": repack it");
  SDMI_CHECK((h.reserved & ~PK_FULL & ~(7 << 4) & ~PK_NHC_MASK) == ((precise_kv_ ? 1 : 0) | (precise_last_res_ ? 2 : 0) | (precise_1x1_max_ds_ << 8)),
             "packed blob was written with a different precision allocation (context K / V, last ResBlock, 1x1 conv levels)");
  std::vector<std::pair<void**, size_t>> bufs;
  int64_t total = 0;
  packed_layout(&bufs, &total);
  SDMI_CHECK(h.n_buffers == (int32_t)bufs.size() && h.total_bytes == total && bytes >= total, "packed blob truncated or inconsistent");
  int64_t off = (int64_t)round_up((int64_t)sizeof(PackedHeader), PK_ALIGN);
  for (auto& b : bufs) {
    if (store_.alloc(b.first, b.second)) return -1;
    SDMI_HIP_OK(hipMemcpyAsync(*b.first, (const char*)host_buf + off, b.second, hipMemcpyHostToDevice, stream));
    off += (int64_t)round_up((int64_t)b.second, PK_ALIGN);
  }
  SDMI_HIP_OK(hipStreamSynchronize(stream));
  store_.mark_all_set();
  ctx_valid_ = false;
  drop_timestep_table();
  return finalize();
}

// ------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------
struct Fwd : FwdBase {
  UNet* u; int Lctx;
  bool ln_fold_on = false;      // this call folds LayerNorms into their consuming GEMMs (UNet::ln_fold_; read per call: A/B knobs)
  bool ff_tail_on = false;      // ... and runs SpatialTransformer tails as row-strip chain launches (UNet::ff_tail_; SDMI_FF_TAIL, read per call)
  bool st_head_on = false;      // ... and SpatialTransformer heads (UNet::st_head_; SDMI_ST_HEAD, read per call)
  bool st_mid_on = false;       // ... and the out-projection of attn1 with attn2's to_q (SDMI_ST_MID)
  bool st_tail_on = false;      // ... and the out-projection of attn2 in front of the tail's chain launch (SDMI_ST_TAIL)
  bool st_mid_ctx_on = false;   // ... and the cross-attention inside the st_mid launch (SDMI_ST_MID_CTX)
  bool ctx1_on = false;         // a context of ONE token: the cross-attention output is V of the sample, copied from the cached V^T (SDMI_CTX1, read per call)
  // a ResBlock's skip_connection as the 1x1 tail phase of conv2's halo-staged launch (IGemmParams::tail_*; SDMI_SKIP_FOLD, read per call), on maps
  // up to skip_fold_max_w wide (SDMI_SKIP_FOLD_MAX_W); skip_fold_plan: one entry per ResBlock with a skip convolution, in execution order
  bool skip_fold_on = false; int skip_fold_max_w = 64;
  std::vector<int>* skip_fold_plan = nullptr;
  bool gn_conv_on = false;      // ResBlock GroupNorm + SiLU + conv3x3 as one launch where a workgroup can own all output columns (gnconv.hip; SDMI_GN_CONV)
  float* emb_all = nullptr;     // [B][emb_total] (emb_ld = emb_total), or one row of the timestep table shared by every sample (emb_ld = 0)
  int emb_ld = 0;
  bool emb_caller = false;      // emb_all is that table row: a caller pointer of a launch tape (Tape::R_EMB)
  const f16* ctx16 = nullptr;   // [B*L][context_dim], null when the cached K/V are used
  const f16* ctx16_lo = nullptr; // ... its split-fp16 low half fp16(ctx - fp16(ctx)) (precise K / V projections)

  Act res_block(Layer& L, const Act& x0, const Act* x1) {
    const int H = x0.H, W = x0.W, M = B * H * W;
    const int Cin = x0.C + (x1 ? x1->C : 0), Cout = L.cout;
    if (Cin != L.cin) { ok(fail("res block channel mismatch at " + L.prefix)); }
    if (Cin == Cout && x1) ok(fail("identity skip with a concatenated input at " + L.prefix));
    const size_t mark = scratch.off;
    f16* raw = (Cin != Cout) ? S<f16>((size_t)M * Cin) : nullptr;
    const bool p1 = L.p1x1;              // this layer's skip convolution as 3-pass split-fp16
    const bool p3 = L.precise3;          // ... and its two 3x3 convs (the last ResBlock): operands [hi | lo | hi] against packed [w_hi | w_hi | w_lo]
    f16* raw_lo = (Cin != Cout && p1) ? S<f16>((size_t)M * Cin) : nullptr;
    float* h = S<float>((size_t)M * Cout);
    Act out = make_act(P<float>((size_t)M * Cout), Cout, H, W, true);
    Act hact = make_act(h, Cout, H, W, true);
    f16* a2 = nullptr;
    int& gn2_applied = u->gn2_applied_;     // (its address rides in the recorded parameter bytes: the same on every call)
    gn2_applied = 0;
    // in_layers / out_layers as ONE launch each (gnconv.hip: 32 pixels x all 320 output channels per workgroup, the halo normalised once):
    // the 64 x 64 level of SD v1.  (in_layers only without a skip convolution: that one reads raw fp16 copies the GroupNorm launch writes.)
    // scale-shift ResBlock (openaimodel.py:267-271): conv1 adds no embedding row; out_layers' GroupNorm takes the layer's [scale | shift] row
    // in its apply launch (GroupNormParams::film) -- so neither the one-launch forms nor the split-K reduction that applies a GroupNorm
    const bool ss = u->scale_shift_;
    const float* const film = ss ? emb_all + L.emb_off : nullptr;
    const bool gc1 = gn_conv_on && !ss && !p3 && Cin == Cout && gn_conv3_supported(B, H, W, x0.C, x1 ? x1->C : 0, Cout);
    const bool gc2 = gn_conv_on && !ss && !p3 && gn_conv3_supported(B, H, W, Cout, 0, Cout);
    auto gn_conv = [&](const Act& a0, const Act* a1, const float* gamma, const float* beta, const f16* w, IGemmParams& e) {
      GnConvParams g = GnConvParams();
      g.gn_acc = groupnorm(a0, a1, gamma, beta, 1e-5f, 1, nullptr, nullptr, nullptr, nullptr, nullptr, /*stats_only=*/true);
      g.x0 = a0.p; g.c0 = a0.C; g.x1 = a1 ? a1->p : nullptr; g.c1 = a1 ? a1->C : 0;
      g.gn_gamma = gamma; g.gn_beta = beta; g.gn_eps = 1e-5f; g.w = w; g.epi = e;
      if (!dry && !rc) ok(launch_gn_conv3(g, s));
    };
    if (gc1) {
      IGemmParams p = conv3(nullptr, Cin, H, W, H, W, 1, 0, L.w16[0], Cout);
      p.bias = L.f32[2]; p.rowvec = emb_all + L.emb_off; p.ld_rowvec = emb_ld;
      p.out_f32 = h; p.ldo = Cout;
      attach_gn_targets(p, hact);
      TapeCaller tc(Tape::R_EMB, emb_caller ? p.rowvec : nullptr);
      gn_conv(x0, x1, L.f32[0], L.f32[1], L.w16[0], p);
    } else {
      f16* a = S<f16>((size_t)M * Cin);
      f16* a_lo = p3 ? S<f16>((size_t)M * Cin) : nullptr;
      groupnorm(x0, x1, L.f32[0], L.f32[1], 1e-5f, 1, a, nullptr, raw, a_lo, raw_lo);
      IGemmParams p = conv3(a, Cin, H, W, H, W, 1, 0, L.w16[0], Cout);
      if (p3) split3(p, a, a_lo, Cin);
      p.bias = L.f32[2];
      if (!ss) { p.rowvec = emb_all + L.emb_off; p.ld_rowvec = emb_ld; }
      p.out_f32 = h; p.ldo = Cout;
      attach_gn_targets(p, hact);          // statistics of out_layers' GroupNorm come out of this epilogue
      if (!gc2 && !p3 && !ss) {
        // ... or, where this conv ends up split along K (8x8, 16x16, the concat blocks of 32x32), GroupNorm + SiLU are applied by
        // its split-K reduction: a2 = the conv2 operand comes straight out of it (IGemmParams::pgn_*; gn2_applied says so)
        a2 = S<f16>((size_t)M * Cout);
        p.pgn_gamma = L.f32[3]; p.pgn_beta = L.f32[4]; p.pgn_eps = 1e-5f; p.pgn_silu = 1; p.pgn_out = a2; p.pgn_applied = &gn2_applied;
      }
      TapeCaller tc(Tape::R_EMB, emb_caller ? p.rowvec : nullptr);      // (null for a scale-shift block: declares nothing)
      gemm(p);
    }
    const float* residual = x0.p;
    // skip_connection (needs only the raw fp16 copies, written by GroupNorm 1).  out = conv2(...) + skip(x) is one sum per output element:
    // where conv2 runs on a halo-staged tile the skip conv is the 1x1 tail phase of that launch -- extra k-tiles of conv2's accumulators,
    // [raw | raw_lo | raw] against W_SPLIT3's [w_hi | w_hi | w_lo] or raw against W_CONV -- with the bias bias2 + bias_skip (L.bias_fold) and
    // no residual: no skip GEMM launch, no split-K reduce behind it, no fp32 [M][Cout] round trip.  Everything else takes the two launches:
    // full precision and the split-fp16 last block (their convs are no halo launches), scale-shift blocks and the opt-in gn_conv path
    // (not measured with a tail), and whatever conv2 shape the tuning table does not send to a halo tile.
    IGemmParams tailp = IGemmParams();      // conv2's tail fields when folding (tail_kt = 0: two launches)
    if (Cin != Cout) {
      bool fold = skip_fold_on && !u->full() && !p3 && !ss && !gc2 && !gn_conv_on && W <= skip_fold_max_w && Cin % 64 == 0 && (dry || L.bias_fold != nullptr);
      if (fold) {
        IGemmParams c2 = conv3(raw, Cout, H, W, H, W, 1, 0, L.w16[1], Cout);       // conv2's shape (its operand pointer is not looked at)
        c2.tail_a0 = raw; c2.tail_a1 = p1 ? raw_lo : nullptr; c2.tail_a2 = p1 ? raw : nullptr;
        c2.tail_c = Cin; c2.tail_ld = Cin; c2.tail_w = L.w16[2]; c2.tail_kt = p1 ? 3 * Cin : Cin;
        c2.out_f32 = out.p; c2.ldo = Cout;
        c2.splitk_ws = splitk_ws; c2.splitk_ws_floats = splitk_ws_floats;
        fold = igemm_plans_halo(c2);
        if (fold) tailp = c2;
      }
      if (skip_fold_plan && dry) skip_fold_plan->push_back(fold ? 1 : 0);      // (the dry pass in front of every forward decides the same)
      if (!fold) {
        IGemmParams p = dense1x1(raw, raw_lo, M, Cin, L.w16[2], Cout, H * W, p1);
        p.bias = L.f32[6]; p.out_f32 = out.p; p.ldo = Cout;
        gemm(p);
        residual = out.p;
      }
    }
    if (gc2) {
      IGemmParams p = conv3(nullptr, Cout, H, W, H, W, 1, 0, L.w16[1], Cout);
      p.bias = L.f32[5]; p.residual = residual; p.ldr = Cout; p.out_f32 = out.p; p.ldo = Cout;
      attach_gn_targets(p, out);
      attach_f16_copy(p, out);
      gn_conv(hact, nullptr, L.f32[3], L.f32[4], L.w16[1], p);
    } else {
      f16* a2_lo = nullptr;
      if (p3) { a2 = S<f16>((size_t)M * Cout); a2_lo = S<f16>((size_t)M * Cout); }
      if (ss && !a2) a2 = S<f16>((size_t)M * Cout);
      {
        // the row is a caller pointer of the launch tape whenever it comes from the timestep table: a replay at another timestep
        // must normalise with that step's row
        TapeCaller tc(Tape::R_EMB, emb_caller ? film : nullptr);
        groupnorm(hact, nullptr, L.f32[3], L.f32[4], 1e-5f, 1, a2, nullptr, nullptr, a2_lo, nullptr, false, gn2_applied != 0, film, emb_ld);
      }
      IGemmParams p = conv3(a2, Cout, H, W, H, W, 1, 0, L.w16[1], Cout);
      if (p3) split3(p, a2, a2_lo, Cout);
      p.bias = L.f32[5]; p.residual = residual; p.ldr = Cout; p.out_f32 = out.p; p.ldo = Cout;
      if (tailp.tail_kt) {                 // the skip convolution rides in this launch (see above)
        p.tail_a0 = tailp.tail_a0; p.tail_a1 = tailp.tail_a1; p.tail_a2 = tailp.tail_a2; p.tail_c = tailp.tail_c; p.tail_ld = tailp.tail_ld;
        p.tail_w = tailp.tail_w; p.tail_kt = tailp.tail_kt;
        p.bias = L.bias_fold; p.residual = nullptr; p.ldr = 0;
      }
      attach_gn_targets(p, out);           // ... and those of the GroupNorm(s) that read this block's output
      attach_f16_copy(p, out);             // ... and the fp16 copy a Downsample / Upsample behind this block wants
      gemm(p);
    }
    scratch.off = mark;
    return out;
  }

  // K / V^T of the cross-attention for one transformer block (depends on the context only)
  void context_kv(Layer& L, int d) {
    TBlock& T = L.tb[d];
    const int C = L.cin, Lp = (int)round_up(Lctx, 8);
    const int CD = u->cfg_.context_dim;
    IGemmParams p = dense(ctx16, B * Lctx, CD, T.wkv2, 2 * C, Lctx);
    if (ctx16_lo) split3(p, ctx16, ctx16_lo, CD);
    if (u->full()) {         // K | V in fp32, then hi / lo per head (the V^T pad keys are written as zeros)
      const size_t mark = scratch.off;
      float* kv = S<float>((size_t)B * Lctx * 2 * C);
      p.out_f32 = kv; p.ldo = 2 * C;
      gemm(p);
      if (!dry && !rc) ok(launch_split_heads(kv, 2 * C, 0, T.ck, T.ck_lo, 0, B, Lctx, Lp, L.heads, L.dh, s));
      if (!dry && !rc) ok(launch_split_heads(kv, 2 * C, C, T.cvt, T.cvt_lo, 1, B, Lctx, Lp, L.heads, L.dh, s));
      scratch.off = mark;
      return;
    }
    p.mode = EPI_HEADS; p.seg_dst[0] = T.ck; p.seg_dst[1] = T.cvt; p.seg_kind[0] = 0; p.seg_kind[1] = 1;
    p.heads = L.heads; p.dh = L.dh; p.ntok = Lctx; p.ntok_pad = Lp; p.segC = C; p.splitk = 1;
    if (!dry && !rc && Lp != Lctx) {
      hipError_t e = memset_async(T.cvt, 0, (size_t)B * C * Lp * sizeof(f16), s);
      if (e != hipSuccess) ok(fail(std::string("hipMemsetAsync: ") + hipGetErrorString(e)));
    }
    gemm(p);
  }

  // The SpatialTransformer of the full-precision mode (attention.py:196-257): every linear is a split-fp16 GEMM into fp32, the
  // producers of the next operand (GroupNorm-apply, LayerNorm, per-head scatter, GEGLU, the cast in front of proj_out) write hi | lo,
  // both attention products run on attn_split16.hip.  No chains, no folds.
  Act attn_block_full(Layer& L, const Act& x) {
    const int H = x.H, W = x.W, N = H * W, M = B * N, C = L.cin;
    const int Np = (int)round_up(N, 8), Lp = (int)round_up(Lctx, 8);
    const float scale = 1.0f / sqrtf((float)L.dh);
    const size_t mark = scratch.off;
    f16* a = S<f16>((size_t)M * C); f16* a_lo = S<f16>((size_t)M * C);          // the [M][C] operand of the next linear
    float* t = S<float>((size_t)M * C);                                          // the token stream
    float* y = S<float>((size_t)M * 8 * C);                                      // q | k | v, to_q, GEGLU projection (fp32)
    f16* q = S<f16>((size_t)M * C); f16* q_lo = S<f16>((size_t)M * C);
    f16* k = S<f16>((size_t)M * C); f16* k_lo = S<f16>((size_t)M * C);
    f16* vt = S<f16>((size_t)B * C * Np); f16* vt_lo = S<f16>((size_t)B * C * Np);
    f16* gg = S<f16>((size_t)M * 4 * C); f16* gg_lo = S<f16>((size_t)M * 4 * C);
    auto linear = [&](const f16* hi, const f16* lo, int K, const f16* w, int n_out, const float* bias, float* out, bool residual) {
      IGemmParams p = dense1x1(hi, lo, M, K, w, n_out, N, true);
      p.bias = bias; p.out_f32 = out; p.ldo = n_out;
      if (residual) { p.residual = out; p.ldr = n_out; }       // x = f(x) + x, in place
      gemm(p);
    };
    auto layernorm = [&](const float* gamma, const float* beta) {
      if (!dry && !rc) ok(launch_layernorm_split(t, gamma, beta, a, a_lo, M, C, 1e-5f, s));
    };
    auto heads = [&](const float* src, int ld, int col0, f16* dst, f16* dst_lo, int kind) {
      if (!dry && !rc) ok(launch_split_heads(src, ld, col0, dst, dst_lo, kind, B, N, Np, L.heads, L.dh, s));
    };
    auto attend = [&](const f16* kk, const f16* kk_lo, const f16* v, const f16* v_lo, int nkv, int nkv_pad) {
      AttnSplitParams p = AttnSplitParams();
      p.q = q; p.q_lo = q_lo; p.k = kk; p.k_lo = kk_lo; p.vt = v; p.vt_lo = v_lo; p.out = a; p.out_lo = a_lo;
      p.BH = B * L.heads; p.heads = L.heads; p.nq = N; p.nkv = nkv; p.nkv_pad = nkv_pad; p.d = L.dh; p.scale = scale;
      if (!dry && !rc) ok(launch_attention_split16(p, s));
    };
    groupnorm(x, nullptr, L.f32[0], L.f32[1], 1e-6f, 0, a, nullptr, nullptr, a_lo, nullptr);
    linear(a, a_lo, C, L.w16[0], C, L.f32[2], t, false);                          // proj_in
    for (auto& T : L.tb) {
      layernorm(T.ln[0], T.ln[1]);                                               // x = attn1(norm1(x)) + x
      linear(a, a_lo, C, T.wqkv, 3 * C, nullptr, y, false);
      heads(y, 3 * C, 0, q, q_lo, 0); heads(y, 3 * C, C, k, k_lo, 0); heads(y, 3 * C, 2 * C, vt, vt_lo, 1);
      attend(k, k_lo, vt, vt_lo, N, Np);
      linear(a, a_lo, C, T.wo1, C, T.bo1, t, true);
      layernorm(T.ln[2], T.ln[3]);                                               // x = attn2(norm2(x), context) + x
      if (ctx16) context_kv(L, (int)(&T - L.tb.data()));
      linear(a, a_lo, C, T.wq2, C, nullptr, y, false);
      heads(y, C, 0, q, q_lo, 0);
      attend(T.ck, T.ck_lo, T.cvt, T.cvt_lo, Lctx, Lp);
      linear(a, a_lo, C, T.wo2, C, T.bo2, t, true);
      layernorm(T.ln[4], T.ln[5]);                                               // x = ff(norm3(x)) + x
      linear(a, a_lo, C, T.wgg, 8 * C, T.bgg, y, false);
      if (!dry && !rc) ok(launch_geglu_split(y, M, 4 * C, gg, gg_lo, s));
      linear(gg, gg_lo, 4 * C, T.wff2, C, T.bff2, t, true);
    }
    if (!dry && !rc) ok(launch_cast_f16(t, a, a_lo, (int64_t)M * C, s));
    Act out = make_act(P<float>((size_t)M * C), C, H, W, true);
    {
      IGemmParams p = dense1x1(a, a_lo, M, C, L.w16[1], C, N, true);            // proj_out + x
      p.bias = L.f32[3]; p.residual = x.p; p.ldr = C; p.out_f32 = out.p; p.ldo = C;
      attach_gn_targets(p, out);
      gemm(p);
    }
    scratch.off = mark;
    return out;
  }

  Act attn_block(Layer& L, const Act& x) {
    if (u->full()) return attn_block_full(L, x);
    const int H = x.H, W = x.W, N = H * W, M = B * N, C = L.cin;
    const int Np = (int)round_up(N, 8), Lp = (int)round_up(Lctx, 8);
    const float scale = 1.0f / sqrtf((float)L.dh);
    const size_t mark = scratch.off;
    f16* xn = S<f16>((size_t)M * C);
    const bool p1 = L.p1x1;              // proj_in / proj_out of this SpatialTransformer as 3-pass split-fp16
    f16* xn_lo = p1 ? S<f16>((size_t)M * C) : nullptr;
    // proj_in(norm(x)), attention.py:254-255: the GroupNorm as its own launch (fp32 stream -> split-fp16 hi | lo operands) or inside
    // the chain launch below
    const bool fold_ln = ln_fold_on && C % 64 == 0 && C <= 1280 && N % 64 == 0 && M % 64 == 0 && M >= u->ln_fold_min_rows_;
    // the head of the SpatialTransformer (GroupNorm-apply -> proj_in -> q | k | v of the first transformer block) as one row-strip chain
    // launch (rowchain.hip st_head_kernel; UNet::st_head_): LayerNorm fold on, split-fp16 proj_in, C = 320
    const bool chain_head = st_head_on && fold_ln && p1 && L.tb[0].lnf[0] != nullptr &&
                            st_head_supported(C, M, N, Np, L.heads, L.dh) && dense1x1(nullptr, nullptr, M, C, L.w16[0], C, N, p1).split16;
    long long* gn_stats = nullptr;
    if (chain_head) gn_stats = groupnorm(x, nullptr, L.f32[0], L.f32[1], 1e-6f, 0, nullptr, nullptr, nullptr, nullptr, nullptr, /*stats_only=*/true);
    else groupnorm(x, nullptr, L.f32[0], L.f32[1], 1e-6f, 0, xn, nullptr, nullptr, xn_lo, nullptr);
    float* t = S<float>((size_t)M * C);
    f16* ln = S<f16>((size_t)M * C);
    f16* q = S<f16>((size_t)M * C);
    f16* k = S<f16>((size_t)M * C);
    f16* vt = S<f16>((size_t)B * C * Np);
    f16* ao = S<f16>((size_t)M * C);
    f16* gg = S<f16>((size_t)M * 4 * C);
    // Every LayerNorm of the block reads the token stream `t` right after the GEMM that produced it.  Two forms:
    //  * folded into the GEMM that READS it (IGemmParams::lnp_out / lnf_*): the producer stores ln = fp16(gamma * t) and the row
    //    statistics, the consumer corrects its accumulators -- no launch; taken where the producer is not split (many rows);
    //  * a post-op launch behind the producer (launch_igemm issues it after the GEMM / its split-K reduce): ln = LN(t).
    float* lnp = fold_ln ? S<float>((size_t)(C / 32) * M * 2) : nullptr;
    auto with_ln = [&](IGemmParams& p, const float* gamma, const float* beta) {
      if (fold_ln) { p.out_f16 = ln; p.f16_scale = gamma; p.lnp_out = lnp; p.splitk = 1; }
      else { p.ln_gamma = gamma; p.ln_beta = beta; p.ln_out = ln; p.ln_eps = 1e-5f; }
    };
    auto fold_in = [&](IGemmParams& p, const float* cs, const float* dn) {      // the GEMM that reads `ln`
      if (!fold_ln) return;
      p.lnf_part = lnp; p.lnf_npart = C / 32; p.lnf_eps = 1e-5f; p.lnf_cs = cs; p.lnf_d = dn; p.bias = nullptr;
    };
    if (chain_head) {
      TBlock& T = L.tb[0];
      StHeadParams h = StHeadParams();
      h.x = x.p; h.gn_acc = gn_stats; h.gn_gamma = L.f32[0]; h.gn_beta = L.f32[1]; h.gn_eps = 1e-6f;
      h.w_in = L.w16[0]; h.b_in = L.f32[2]; h.t = t; h.ln_gamma = T.ln[0]; h.ln_eps = 1e-5f;
      h.wqkv = T.wqkv; h.lnf_cs = T.lnf[0]; h.lnf_d = T.lnf[1]; h.q = q; h.k = k; h.vt = vt;
      h.M = M; h.B = B; h.ntok = N; h.ntok_pad = Np; h.heads = L.heads; h.dh = L.dh; h.C = C;
      if (!dry && !rc && Np != N) {
        hipError_t e = memset_async(vt, 0, (size_t)B * C * Np * sizeof(f16), s);
        if (e != hipSuccess) ok(fail(std::string("hipMemsetAsync: ") + hipGetErrorString(e)));
      }
      if (!dry && !rc) ok(launch_st_head(h, s));
    } else {
      IGemmParams p = dense1x1(xn, xn_lo, M, C, L.w16[0], C, N, p1);
      p.bias = L.f32[2]; p.out_f32 = t; p.ldo = C;
      with_ln(p, L.tb[0].ln[0], L.tb[0].ln[1]);                      // norm1 of the first block
      gemm(p);
    }
    const int depth = (int)L.tb.size();
    // the tail of the SpatialTransformer (GEGLU -> FF-out -> proj_out) as one row-strip chain launch: last (= only) transformer block,
    // LayerNorm fold on, split-fp16 proj_out, C = 320 (UNet::ff_tail_)
    const bool chain_ff = ff_tail_on && fold_ln && p1 && depth == 1 && L.tb[0].lnf_csd != nullptr && ff_tail_supported(C, M, N) &&
                          dense1x1(nullptr, nullptr, M, C, L.w16[1], C, N, p1).split16;
    const bool chain_tail = chain_ff && st_tail_on;      // ... with attn2's out-projection in front (ff_tail_kernel HEAD)
    for (int d = 0; d < depth; ++d) {
      TBlock& T = L.tb[d];
      // x = attn1(norm1(x)) + x                                   attention.py:212
      if (!(chain_head && d == 0)) {       // (the chain launch above has written q, k, v^T of the first block)
        IGemmParams p = dense(ln, M, C, T.wqkv, 3 * C, N);
        p.mode = EPI_HEADS; p.seg_dst[0] = q; p.seg_dst[1] = k; p.seg_dst[2] = vt;
        p.seg_kind[0] = 0; p.seg_kind[1] = 0; p.seg_kind[2] = 1;
        p.heads = L.heads; p.dh = L.dh; p.ntok = N; p.ntok_pad = Np; p.segC = C; p.splitk = 1;
        fold_in(p, T.lnf[0], T.lnf[1]);
        if (!dry && !rc && Np != N) {
          hipError_t e = memset_async(vt, 0, (size_t)B * C * Np * sizeof(f16), s);
          if (e != hipSuccess) ok(fail(std::string("hipMemsetAsync: ") + hipGetErrorString(e)));
        }
        gemm(p);
      }
      attention(q, k, vt, ao, L, N, N, Np, scale);
      // attn1's out-projection (+ x) and attn2's to_q over norm2 as one row-strip chain launch (rowchain.hip, st_head_kernel KIND 1)
      bool chain_ctx = false;
      const bool chain_mid = st_mid_on && fold_ln && T.lnf[2] != nullptr && st_head_supported(C, M, N, Np, L.heads, L.dh);
      if (chain_mid) {
        StHeadParams h = StHeadParams();
        h.a16 = ao; h.w_in = T.wo1; h.b_in = T.bo1; h.t = t; h.ln_gamma = T.ln[2]; h.ln_eps = 1e-5f;
        h.wqkv = T.wq2; h.lnf_cs = T.lnf[2]; h.lnf_d = T.lnf[3]; h.q = q;
        h.M = M; h.B = B; h.ntok = N; h.ntok_pad = Np; h.heads = L.heads; h.dh = L.dh; h.C = C;
        if (ctx16) context_kv(L, d);
        // ... and the cross-attention itself inside that launch (st_head_kernel CTX: q never leaves the CU)
        chain_ctx = st_mid_ctx_on && L.dh == 40 && Lctx <= 128;
        if (chain_ctx) { h.ctx_k = T.ck; h.ctx_vt = T.cvt; h.ctx_nkv = Lctx; h.ctx_nkv_pad = Lp; h.ctx_scale = scale; h.ao_out = ao; }
        if (!dry && !rc) ok(launch_st_mid(h, s));
      } else {
        IGemmParams p = dense(ao, M, C, T.wo1, C, N);
        p.bias = T.bo1; p.residual = t; p.ldr = C; p.out_f32 = t; p.ldo = C;
        with_ln(p, T.ln[2], T.ln[3]);                                // norm2
        gemm(p);
      }
      // x = attn2(norm2(x), context) + x                           attention.py:213
      if (ctx16 && !chain_mid) context_kv(L, d);
      if (chain_mid) {
        if (!chain_ctx) attention(q, T.ck, T.cvt, ao, L, N, Lctx, Lp, scale);       // (q = to_q(norm2(t)) came out of the chain launch)
      } else if (ctx1_on && Lctx == 1) {
        // one-token context: softmax over one key is 1, the attention output is V of the sample for every query, bit for bit -- written
        // straight from the cached V^T: no to_q GEMM, no attention launch.  Every other launch is the general path's, so eps is too.
        if (!dry && !rc) ok(launch_ctx1_broadcast(T.cvt, Lp, ao, B, N, C, s));
      } else {
        IGemmParams p = dense(ln, M, C, T.wq2, C, N);
        p.mode = EPI_HEADS; p.seg_dst[0] = q; p.seg_kind[0] = 0;
        p.heads = L.heads; p.dh = L.dh; p.ntok = N; p.ntok_pad = Np; p.segC = C; p.splitk = 1;
        fold_in(p, T.lnf[2], T.lnf[3]);
        gemm(p);
        attention(q, T.ck, T.cvt, ao, L, N, Lctx, Lp, scale);
      }
      if (!chain_tail) {                     // (else: inside the chain launch below)
        IGemmParams p = dense(ao, M, C, T.wo2, C, N);
        p.bias = T.bo2; p.residual = t; p.ldr = C; p.out_f32 = t; p.ldo = C;
        with_ln(p, T.ln[4], T.ln[5]);                                // norm3
        gemm(p);
      }
      // x = ff(norm3(x)) + x                                       attention.py:214
      if (chain_ff) break;                   // (depth 1: GEGLU, FF-out and proj_out are the chain launch below)
      {
        IGemmParams p = dense(ln, M, C, T.wgg, 8 * C, N);
        p.mode = EPI_GEGLU; p.bias = T.bgg; p.out_f16 = gg; p.ldo = 4 * C; p.splitk = 1;
        fold_in(p, T.lnf[4], T.lnf[5]);
        gemm(p);
      }
      {
        IGemmParams p = dense(gg, M, 4 * C, T.wff2, C, N);
        p.bias = T.bff2; p.residual = t; p.ldr = C; p.ldo = C;
        if (d + 1 < depth) {
          p.out_f32 = t;
          with_ln(p, L.tb[d + 1].ln[0], L.tb[d + 1].ln[1]);          // norm1 of the next block
        } else {
          // last block: only proj_out reads the result -- emit its split-fp16 operand (hi | lo) directly
          p.out_f16 = ln; p.out_lo = xn_lo;
        }
        gemm(p);
      }
    }
    Act out = make_act(P<float>((size_t)M * C), C, H, W, true);
    {
      IGemmParams p = dense1x1(ln, xn_lo, M, C, L.w16[1], C, N, p1);
      p.Hout = H * W;                       // (dense: rows per sample)
      p.bias = L.f32[3]; p.residual = x.p; p.ldr = C; p.out_f32 = out.p; p.ldo = C;
      attach_gn_targets(p, out);
      attach_f16_copy(p, out);
      if (chain_ff) {
        // out = x + proj_out(t + FF(norm3(t))): one row-strip chain launch (rowchain.hip); `ln` / `lnp` are what attn2's out-projection stored
        TBlock& T = L.tb[0];
        FfTailParams q = FfTailParams();
        q.ln = ln; q.lnp = lnp; q.ln_eps = 1e-5f; q.csd = T.lnf_csd; q.wgg = T.wgg; q.wff2 = T.wff2; q.bff2 = T.bff2; q.t = t; q.wpo = L.w16[1];
        if (chain_tail) { q.a16 = ao; q.wo = T.wo2; q.bo = T.bo2; q.ln_gamma = T.ln[4]; }     // t += ao Wo2^T + bo2 first (attention.py:213)
        q.epi = p;
        if (!dry && !rc) ok(launch_ff_tail(q, s));
      } else {
        gemm(p);
      }
    }
    scratch.off = mark;
    return out;
  }

  void attention(const f16* q, const f16* k, const f16* vt, f16* out, Layer& L, int nq, int nkv, int nkv_pad, float scale) {
    AttnParams a = AttnParams();
    a.q = q; a.k = k; a.vt = vt; a.out = out; a.BH = B * L.heads; a.heads = L.heads; a.nq = nq; a.nkv = nkv;
    a.nkv_pad = nkv_pad; a.d = L.dh; a.scale = scale;
    if (!dry && !rc) ok(launch_attention(a, s));
  }

  Act resample(Layer& L, const Act& x, bool up) {
    const int Hin = x.H, Win = x.W, C = x.C;
    const int Hout = up ? 2 * Hin : (Hin - 1) / 2 + 1, Wout = up ? 2 * Win : (Win - 1) / 2 + 1;
    const size_t mark = scratch.off;
    if (u->full()) {         // split-fp16 operand [hi | lo | hi] against the packed [w_hi | w_hi | w_lo] (W_CONV_SPLIT3)
      const int64_t n = (int64_t)B * Hin * Win * C;
      f16* hi = S<f16>((size_t)n); f16* lo = S<f16>((size_t)n);
      if (!dry && !rc) ok(launch_cast_f16(x.p, hi, lo, n, s));
      Act out = make_act(P<float>((size_t)B * Hout * Wout * C), L.cout, Hout, Wout, true);
      IGemmParams p = conv3(hi, C, Hin, Win, Hout, Wout, up ? 1 : 2, up ? 1 : 0, L.w16[0], L.cout);
      split3(p, hi, lo, C);
      p.bias = L.f32[0]; p.out_f32 = out.p; p.ldo = L.cout;
      attach_gn_targets(p, out);
      gemm(p);
      scratch.off = mark;
      return out;
    }
    // the fp16 operand: stored by the producing GEMM's epilogue when there is one (see FwdBase::attach_f16_copy), else cast here
    const f16* x16 = nullptr;
    if (dry) { if (!want_f16_copy(x)) (void)S<f16>((size_t)B * Hin * Win * C); }
    else {
      x16 = f16_copy(x);
      if (!x16) {
        f16* c = S<f16>((size_t)B * Hin * Win * C);
        if (!rc) ok(launch_cast_f16(x.p, c, nullptr, (int64_t)B * Hin * Win * C, s));
        x16 = c;
      }
    }
    Act out = make_act(P<float>((size_t)B * Hout * Wout * C), L.cout, Hout, Wout, true);
    IGemmParams p = conv3(x16, C, Hin, Win, Hout, Wout, up ? 1 : 2, up ? 1 : 0, L.w16[0], L.cout);
    p.bias = L.f32[0]; p.out_f32 = out.p; p.ldo = L.cout;
    attach_gn_targets(p, out);
    // nearest x2 + 3x3 as the four 2x2 phase convs of one launch (igemm KIND_2X2: 4 / 9 of the MACs) where the tuning table says that wins;
    // its statistics rows are the source pixels of a phase, so a sample must hold a multiple of 32 of those
    if (up && L.w_up_phase && (p.gn_n == 0 || (Hin * Win) % 32 == 0) && igemm_plans_up_phase(p)) p = up_phase_of(p, L.w_up_phase);
    gemm(p);
    scratch.off = mark;
    return out;
  }

  // ResBlock with resblock_updown (openaimodel.py:253-259): h = conv3(resample(SiLU(GN(x)))), skip = resample(x) (Identity: the
  // channel count does not change), resample = F.avg_pool2d(2) (dir 1) or nearest x2 (dir -1); the rest as in res_block
  Act res_block_updown(Layer& L, const Act& x) {
    const int dir = L.updown, H = x.H, W = x.W, C = L.cin;
    if (x.C != C || L.cout != C) ok(fail("resampling res block channel mismatch at " + L.prefix));
    if (dir > 0 && ((H | W) & 1)) ok(fail("resampling res block at " + L.prefix + ": the 2x2 average pool needs even H and W"));
    const int Ho = dir > 0 ? H / 2 : 2 * H, Wo = dir > 0 ? W / 2 : 2 * W, M = B * Ho * Wo;
    const bool p3 = L.precise3;
    const bool ss = u->scale_shift_;                                   // (as in res_block: the row modulates out_layers' GroupNorm)
    const float* const film = ss ? emb_all + L.emb_off : nullptr;
    const size_t mark = scratch.off;
    float* g = S<float>((size_t)B * H * W * C);                        // SiLU(GN(x)) at the input resolution (fp32)
    groupnorm(x, nullptr, L.f32[0], L.f32[1], 1e-5f, 1, nullptr, g, nullptr);
    f16* a = S<f16>((size_t)M * C);
    f16* a_lo = p3 ? S<f16>((size_t)M * C) : nullptr;
    float* xs = S<float>((size_t)M * C);                               // x_upd(x): the residual
    if (!dry && !rc) ok(launch_resample2(g, nullptr, a, a_lo, B, H, W, C, dir, s));
    if (!dry && !rc) ok(launch_resample2(x.p, xs, nullptr, nullptr, B, H, W, C, dir, s));
    float* h = S<float>((size_t)M * C);
    Act out = make_act(P<float>((size_t)M * C), C, Ho, Wo, true);
    Act hact = make_act(h, C, Ho, Wo, true);
    {
      IGemmParams p = conv3(a, C, Ho, Wo, Ho, Wo, 1, 0, L.w16[0], C);
      if (p3) split3(p, a, a_lo, C);
      p.bias = L.f32[2];
      if (!ss) { p.rowvec = emb_all + L.emb_off; p.ld_rowvec = emb_ld; }
      p.out_f32 = h; p.ldo = C;
      attach_gn_targets(p, hact);
      TapeCaller tc(Tape::R_EMB, emb_caller ? p.rowvec : nullptr);
      gemm(p);
    }
    {
      f16* a2 = S<f16>((size_t)M * C);
      f16* a2_lo = p3 ? S<f16>((size_t)M * C) : nullptr;
      {
        TapeCaller tc(Tape::R_EMB, emb_caller ? film : nullptr);
        groupnorm(hact, nullptr, L.f32[3], L.f32[4], 1e-5f, 1, a2, nullptr, nullptr, a2_lo, nullptr, false, false, film, emb_ld);
      }
      IGemmParams p = conv3(a2, C, Ho, Wo, Ho, Wo, 1, 0, L.w16[1], C);
      if (p3) split3(p, a2, a2_lo, C);
      p.bias = L.f32[5]; p.residual = xs; p.ldr = C; p.out_f32 = out.p; p.ldo = C;
      attach_gn_targets(p, out);
      gemm(p);
    }
    scratch.off = mark;
    return out;
  }

  // AttentionBlock._forward (openaimodel.py:318-323): x + proj_out(QKVAttentionLegacy(qkv(GroupNorm32(x)))) over all H * W pixels.
  // The qkv rows were permuted at pack time (W_QKV_LEGACY), so the fp32 GEMM output is [q | k | v] with heads contiguous; the
  // legacy scale 1/sqrt(sqrt(d)) on q and on k is the one scale 1/sqrt(d) on q k^T here.  Full mode: split-fp16 everywhere.
  Act attn_block_legacy(Layer& L, const Act& x) {
    const int H = x.H, W = x.W, N = H * W, M = B * N, C = L.cin;
    const int Np = (int)round_up(N, 8);
    const bool fm = u->full();
    const bool pq = L.p1x1;                 // qkv GEMM on split-fp16 operands (packed accordingly, see UNet::build)
    const size_t mark = scratch.off;
    f16* xn = S<f16>((size_t)M * C);
    f16* xn_lo = pq ? S<f16>((size_t)M * C) : nullptr;
    groupnorm(x, nullptr, L.f32[0], L.f32[1], 1e-5f, 0, xn, nullptr, nullptr, xn_lo, nullptr);
    float* qkv = S<float>((size_t)M * 3 * C);
    {
      IGemmParams p = dense1x1(xn, xn_lo, M, C, L.w16[0], 3 * C, N, pq);
      p.bias = L.f32[2]; p.out_f32 = qkv; p.ldo = 3 * C;
      gemm(p);
    }
    f16* q = S<f16>((size_t)M * C); f16* q_lo = S<f16>((size_t)M * C);
    f16* k = S<f16>((size_t)M * C); f16* k_lo = S<f16>((size_t)M * C);
    f16* vt = S<f16>((size_t)B * C * Np); f16* vt_lo = S<f16>((size_t)B * C * Np);
    if (!dry && !rc) ok(launch_split_heads(qkv, 3 * C, 0, q, q_lo, 0, B, N, Np, L.heads, L.dh, s));
    if (!dry && !rc) ok(launch_split_heads(qkv, 3 * C, C, k, k_lo, 0, B, N, Np, L.heads, L.dh, s));
    if (!dry && !rc) ok(launch_split_heads(qkv, 3 * C, 2 * C, vt, vt_lo, 1, B, N, Np, L.heads, L.dh, s));
    f16* ao = S<f16>((size_t)M * C);
    f16* ao_lo = fm ? S<f16>((size_t)M * C) : nullptr;
    const float scale = 1.0f / sqrtf((float)L.dh);
    if (fm) {
      AttnSplitParams a = AttnSplitParams();
      a.q = q; a.q_lo = q_lo; a.k = k; a.k_lo = k_lo; a.vt = vt; a.vt_lo = vt_lo; a.out = ao; a.out_lo = ao_lo;
      a.BH = B * L.heads; a.heads = L.heads; a.nq = N; a.nkv = N; a.nkv_pad = Np; a.d = L.dh; a.scale = scale;
      if (!dry && !rc) ok(launch_attention_split16(a, s));
    } else {
      attention(q, k, vt, ao, L, N, N, Np, scale);
    }
    Act out = make_act(P<float>((size_t)M * C), C, H, W, true);
    {
      IGemmParams p = dense1x1(ao, ao_lo, M, C, L.w16[1], C, N, fm);
      p.bias = L.f32[3]; p.residual = x.p; p.ldr = C; p.out_f32 = out.p; p.ldo = C;
      attach_gn_targets(p, out);
      attach_f16_copy(p, out);             // ... and the fp16 copy a Downsample / Upsample convolution behind this block wants (resblock_updown = 0)
      gemm(p);
    }
    scratch.off = mark;
    return out;
  }

  Act run_layer(Layer& L, const Act& x, const Act* skip) {
    switch (L.kind) {
      case L_RES: return L.updown ? res_block_updown(L, x) : res_block(L, x, skip);
      case L_ATTN: return attn_block(L, x);
      case L_ATTN_LEGACY: return attn_block_legacy(L, x);
      case L_DOWN: return resample(L, x, false);
      case L_UP: return resample(L, x, true);
      default: ok(fail("unexpected layer kind")); return x;
    }
  }
};

// Cross-attention K / V^T caches of every transformer block: capacity-sized device buffers owned by the handle.  They are
// allocated by finalize() for the default capacity (8 rows x 80 padded context tokens: SD v1's 77-token prompts at the largest
// batch one call takes) and grown only by reserve_ctx_cache() -- sdmi_unet_reserve_context / sdmi_unet_cache_context, both off
// the hot path.  sdmi_unet_forward never allocates: a context beyond the capacity is an error that names the remedy.
int UNet::reserve_ctx_cache(int B, int Lctx) {
  const int64_t need = (int64_t)B * round_up(Lctx, 8);          // (B * Lctx * C <= B * Lp * C: one capacity covers K and V^T)
  if (need <= ctx_cap_) return 0;
  ++ctx_gen_;                // (the K / V^T buffers move: recorded launch tapes are stale)
  if (for_each_layer([&](Layer& L) -> int {
    if (L.kind != L_ATTN) return 0;
    for (auto& T : L.tb) {
      if (T.ck) { (void)hipFree(T.ck); T.ck = nullptr; }
      if (T.cvt) { (void)hipFree(T.cvt); T.cvt = nullptr; }
      SDMI_HIP_OK(hipMalloc((void**)&T.ck, (size_t)need * L.cin * sizeof(f16)));
      SDMI_HIP_OK(hipMalloc((void**)&T.cvt, (size_t)need * L.cin * sizeof(f16)));
      if (full()) {            // (the low halves of the split-fp16 K / V^T)
        if (T.ck_lo) { (void)hipFree(T.ck_lo); T.ck_lo = nullptr; }
        if (T.cvt_lo) { (void)hipFree(T.cvt_lo); T.cvt_lo = nullptr; }
        SDMI_HIP_OK(hipMalloc((void**)&T.ck_lo, (size_t)need * L.cin * sizeof(f16)));
        SDMI_HIP_OK(hipMalloc((void**)&T.cvt_lo, (size_t)need * L.cin * sizeof(f16)));
      }
    }
    return 0;
  })) return -1;
  ctx_cap_ = need; ctx_B_ = 0; ctx_L_ = 0; ctx_valid_ = false;
  return 0;
}

// bind the cache to the shape of this call: no allocation; a different shape only invalidates the cached contents
int UNet::ensure_ctx_cache(int B, int Lctx, bool may_grow) {
  if (ctx_B_ == B && ctx_L_ == Lctx) return 0;
  const int64_t need = (int64_t)B * round_up(Lctx, 8);
  if (need > ctx_cap_) {
    if (may_grow) { if (reserve_ctx_cache(B, Lctx)) return -1; }
    else return fail("context of " + std::to_string(B) + " x " + std::to_string(Lctx) + " tokens exceeds the reserved K/V capacity (" +
                     std::to_string(ctx_cap_) + " padded rows): call sdmi_unet_reserve_context(h, B, Lctx) once, outside the sampling loop");
  }
  ctx_B_ = B; ctx_L_ = Lctx; ctx_valid_ = false;
  return 0;
}

int UNet::cache_timesteps(const int64_t* t_host, int n, hipStream_t stream) {
  SDMI_CHECK(finalized_, "sdmi_unet_finalize() has not succeeded yet");
  SDMI_CHECK(n >= 0 && n <= 4096 && (n == 0 || t_host != nullptr), "bad timestep list");
  drop_timestep_table();
  if (n == 0) return 0;
  const int mc = cfg_.model_channels;
  const size_t row = (size_t)emb_total_, tmp = (size_t)8 * (mc + 2 * (size_t)te_);
  const size_t need = (size_t)n * row + tmp;
  if (need > emb_tab_floats_) {              // (grow-only; called once per sampling run, not per UNet call)
    if (emb_tab_) (void)hipFree(emb_tab_);
    emb_tab_ = nullptr; emb_tab_floats_ = 0;
    SDMI_HIP_OK(hipMalloc((void**)&emb_tab_, need * sizeof(float)));
    emb_tab_floats_ = need;
  }
  if ((size_t)n > emb_tab_tcap_) {
    if (emb_tab_tdev_) (void)hipFree(emb_tab_tdev_);
    emb_tab_tdev_ = nullptr; emb_tab_tcap_ = 0;
    SDMI_HIP_OK(hipMalloc((void**)&emb_tab_tdev_, (size_t)n * sizeof(int64_t)));
    emb_tab_tcap_ = (size_t)n;
  }
  std::vector<int64_t> host(t_host, t_host + n);      // (the copy below reads a buffer this object owns, not the caller's)
  emb_tab_src_.swap(host);
  SDMI_HIP_OK(hipMemcpyAsync(emb_tab_tdev_, emb_tab_src_.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, stream));
  float* temb = emb_tab_ + (size_t)n * row;
  float* e1 = temb + (size_t)8 * mc;
  float* emb = e1 + (size_t)8 * te_;
  for (int i0 = 0; i0 < n; i0 += 8) {        // the same launches as a forward's timestep path, 8 timesteps as the batch rows
    const int nb = std::min(8, n - i0);
    int r = launch_timestep_embedding(emb_tab_tdev_ + i0, nullptr, temb, nb, mc, stream);
    if (!r) r = launch_small_linear(temb, mc, te_w0_, te_b0_, e1, te_, nb, te_, mc, 0, stream);
    if (!r) r = launch_small_linear(e1, te_, te_w2_, te_b2_, emb, te_, nb, te_, te_, 1, stream);
    if (!r) r = launch_small_linear(emb, te_, emb_w_, emb_b_, emb_tab_ + (size_t)i0 * row, emb_total_, nb, emb_total_, te_, 1, stream);
    if (r) return r;
  }
  emb_tab_t_ = emb_tab_src_;
  return 0;
}

int UNet::hint_timestep(int64_t t) {
  emb_hint_row_ = -1;
  for (size_t i = 0; i < emb_tab_t_.size(); ++i)
    if (emb_tab_t_[i] == t) { emb_hint_row_ = (int)i; break; }
  return 0;
}

int UNet::run(const float* x, const int64_t* t_i64, const float* t_f32, const float* ctx, float* eps_out, int B, int H,
              int W, int Lctx, void* workspace, int64_t ws_bytes, hipStream_t stream, bool dry, bool ctx_only,
              int64_t* bytes_needed) {
  SDMI_CHECK(dry || finalized_, "sdmi_unet_finalize() has not succeeded yet");
  SDMI_CHECK(B >= 1 && B <= 8, "batch (CFG rows) must be 1..8 per call");
  if (has_ctx()) SDMI_CHECK(H >= 1 && W >= 1 && Lctx >= 1, "bad shape");
  else SDMI_CHECK(H >= 1 && W >= 1 && Lctx == 0 && ctx == nullptr && !ctx_only,
                  "bad shape: this UNet has no cross-attention (AttentionBlocks): pass ctx = NULL and Lctx = 0");
  const int down = 1 << (cfg_.n_levels - 1);
  if (ext_.resblock_updown)
    SDMI_CHECK(H % down == 0 && W % down == 0, "latent H and W must be multiples of " + std::to_string(down) +
               " for resblock_updown (the down ResBlocks' avg_pool2d rounds down, the skip concat needs the sizes back)");
  SDMI_CHECK(H % down == 0 && W % down == 0, "H and W must be divisible by 2^(levels-1) (the UNet's skip concat requires it)");

  // The timestep hint is an announcement about THIS call only: consume it up front, so that a call that fails on any of the
  // early returns below (workspace too small, missing context, a launch error) cannot leave it behind for an unrelated
  // later forward, which would then silently take the table row of the old timestep.  (Sizing and context-only calls
  // do not touch the timestep path and leave the hint alone.)
  const int hint_row = emb_hint_row_;
  if (!dry && !ctx_only) emb_hint_row_ = -1;

  // ---- launch tape (tape.h): replay the recorded launch list of this (shape, workspace, mode, knobs), or record it below -------------
  // (both read per call: the tests flip them between two forwards)
  const char* e_rp = getenv("SDMI_REPLAY"); const char* e_rv = getenv("SDMI_REPLAY_VERIFY");
  const bool replay_on = !(e_rp && atoi(e_rp) == 0);
  const bool replay_verify = e_rv && atoi(e_rv) != 0;
  const bool hinted = t_i64 != nullptr && hint_row >= 0 && hint_row < (int)emb_tab_t_.size();
  // (a caller buffer inside the workspace is undefined input: such a call runs the executor, untaped)
  auto in_ws = [&](const void* p, size_t bytes) {
    return p && (uintptr_t)p < (uintptr_t)workspace + (uint64_t)ws_bytes && (uintptr_t)workspace < (uintptr_t)p + bytes;
  };
  const size_t img = (size_t)B * H * W * sizeof(float);
  const bool tape_ok = replay_on && !dry && !ctx_only && !prof_enabled() && !tune_collecting() && !range_check_enabled() &&
                       workspace != nullptr && (t_i64 || t_f32) && !in_ws(x, img * cfg_.in_channels) && !in_ws(eps_out, img * cfg_.out_channels) &&
                       !in_ws(t_i64 ? (const void*)t_i64 : t_f32, (size_t)B * (t_i64 ? 8 : 4)) &&
                       !in_ws(ctx, (size_t)B * Lctx * cfg_.context_dim * sizeof(float));
  TapeKey tkey;
  uintptr_t caller[Tape::R_COUNT] = {0, 0, 0, 0, 0};
  Tape* rec = nullptr;
  std::unique_ptr<Tape> verify_against;
  if (tape_ok) {
    tkey.B = B; tkey.H = H; tkey.W = W; tkey.Lctx = Lctx; tkey.mode = hinted ? 0 : (t_i64 ? 1 : 2);
    tkey.ws = workspace; tkey.ws_bytes = ws_bytes; tkey.have_ctx = ctx != nullptr;
    tkey.env = sdmi_env_hash() ^ (tune_generation() * 0x9e3779b97f4a7c15ull); tkey.weights_gen = weights_gen_; tkey.ctx_gen = ctx_gen_;
    auto low4 = [](const void* p, int shift) { return (unsigned)((uintptr_t)p & 15) << shift; };
    tkey.align = low4(x, 0) | low4(eps_out, 4) | low4(ctx, 8) | low4(t_i64 ? (const void*)t_i64 : t_f32, 12);
    caller[Tape::R_X] = (uintptr_t)x; caller[Tape::R_OUT] = (uintptr_t)eps_out;
    caller[Tape::R_T] = hinted ? 0 : (t_i64 ? (uintptr_t)t_i64 : (uintptr_t)t_f32);
    caller[Tape::R_CTX] = (uintptr_t)ctx;
    caller[Tape::R_EMB] = hinted ? (uintptr_t)(emb_tab_ + (size_t)hint_row * emb_total_) : 0;
    for (size_t i = 0; i < tapes_.size(); ++i) {
      if (!(tapes_[i].first == tkey)) continue;
      std::unique_ptr<Tape> hit = std::move(tapes_[i].second);
      tapes_.erase(tapes_.begin() + (long)i);
      SDMI_CHECK(finalized_, "sdmi_unet_finalize() has not succeeded yet");
      if (ensure_ctx_cache(B, Lctx, false)) return -1;
      if (!ctx && has_ctx()) SDMI_CHECK(ctx_valid_, "ctx == NULL but no cached context for this (B, Lctx); call sdmi_unet_cache_context first");
      hit->retarget(caller);
      if (replay_verify) { verify_against = std::move(hit); break; }      // run the executor and compare what it launches
      const int e = hit->replay(stream);
      const bool sets = hit->sets_ctx_valid;
      const int64_t need = hit->bytes_needed;
      tapes_.emplace_back(tkey, std::move(hit));
      if (e) return fail(std::string("launch tape replay: ") + hipGetErrorString((hipError_t)e));
      if (sets) ctx_valid_ = true;
      if (bytes_needed) *bytes_needed = need;
      ++tape_hits_;
      return 0;
    }
  }
  std::unique_ptr<Tape> fresh;
  if (tape_ok) {
    fresh.reset(new Tape());
    memcpy(fresh->caller, caller, sizeof(caller));
    rec = fresh.get();
  }

  Fwd f;
  f.u = this; f.s = stream; f.dry = dry; f.B = B; f.Lctx = Lctx; f.zero = store_.zero(); f.precise_1x1 = precise_1x1_;
  {
    // (both knobs are read per call -- the tests flip them between two forwards; the row statistics ride on the 16-byte epilogue)
    const char* e_fold = getenv("SDMI_LN_FOLD"); const char* e_vec = getenv("SDMI_EPI_VEC");
    f.ln_fold_on = (e_fold ? atoi(e_fold) != 0 : ln_fold_) && !(e_vec && atoi(e_vec) == 0);
    const char* e_ff = getenv("SDMI_FF_TAIL");
    f.ff_tail_on = e_ff ? atoi(e_ff) != 0 : ff_tail_;
    const char* e_sh = getenv("SDMI_ST_HEAD");
    f.st_head_on = e_sh ? atoi(e_sh) != 0 : st_head_;
    const char* e_sm = getenv("SDMI_ST_MID");
    f.st_mid_on = e_sm ? atoi(e_sm) != 0 : st_head_;
    const char* e_st = getenv("SDMI_ST_TAIL");
    f.st_tail_on = e_st ? atoi(e_st) != 0 : ff_tail_;
    const char* e_mc = getenv("SDMI_ST_MID_CTX");
    f.st_mid_ctx_on = e_mc ? atoi(e_mc) != 0 : st_head_;
    const char* e_c1 = getenv("SDMI_CTX1");               // (A/B knob, read per call: 0 = the general cross-attention path at one key)
    f.ctx1_on = !(e_c1 && atoi(e_c1) == 0);
    const char* e_gc = getenv("SDMI_GN_CONV");
    f.gn_conv_on = e_gc ? atoi(e_gc) != 0 : false;       // (opt-in: bit-identical, 36 us against 41 us with hot operands, +4 us per launch inside a UNet call -- profiles/gn_conv3_r05.txt)
    const char* e_sf = getenv("SDMI_SKIP_FOLD");          // (A/B knob, read per call: 0 = the skip convolutions as their own GEMM launches)
    f.skip_fold_on = e_sf ? atoi(e_sf) != 0 : skip_fold_;
    const char* e_sfw = getenv("SDMI_SKIP_FOLD_MAX_W");   // (... and the widest map whose ResBlocks fold)
    f.skip_fold_max_w = e_sfw ? atoi(e_sfw) : skip_fold_max_w_;
    skip_fold_plan_.clear();
    f.skip_fold_plan = &skip_fold_plan_;
    if (full()) {
      // every chain and fold rounds some operand to fp16 once: the full-precision mode runs the per-op path whatever the knobs say
      f.ln_fold_on = f.ff_tail_on = f.st_head_on = f.st_mid_on = f.st_tail_on = f.st_mid_ctx_on = f.gn_conv_on = false;
    }
  }
  // first pass (always dry) sizes the two arenas; the persist arena sits in front of the scratch arena
  int64_t persist_bytes = 0, scratch_bytes = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const bool d = (pass == 0) ? true : false;
    if (pass == 1 && dry) break;
    f.dry = d; f.rc = 0;
    f.n_acts = 0;
    TapeRecGuard tape_guard(d ? nullptr : rec);         // (the dry pass launches nothing)
    f.plan = fuse_gn_stats_ ? &gn_plan_ : nullptr;
    if (d) gn_plan_.clear();
    f.persist = Arena(); f.scratch = Arena();
    f.persist.dry = f.scratch.dry = d;
    if (!d) {
      SDMI_CHECK(persist_bytes + scratch_bytes <= ws_bytes, "workspace too small: need " +
                 std::to_string(persist_bytes + scratch_bytes) + " bytes, got " + std::to_string(ws_bytes));
      SDMI_CHECK(workspace != nullptr, "workspace is NULL");
      f.persist.base = (char*)workspace; f.persist.cap = (size_t)persist_bytes;
      f.scratch.base = (char*)workspace + persist_bytes; f.scratch.cap = (size_t)scratch_bytes;
      if (ensure_ctx_cache(B, Lctx, ctx_only)) return -1;
    }
    const int mc = cfg_.model_channels;
    if (f.begin_pass((int64_t)12 << 20)) return -1;    // 48 MB of fp32 split-K slabs (largest user: 8 x 512 x 1280)
    f16* ctx16 = f.P<f16>((size_t)B * Lctx * cfg_.context_dim);
    f16* ctx16_lo = precise_kv_ ? f.P<f16>((size_t)B * Lctx * cfg_.context_dim) : nullptr;
    const bool have_ctx = has_ctx() && ((ctx != nullptr) || d);
    if (!has_ctx()) {
      f.ctx16 = nullptr; f.ctx16_lo = nullptr;          // (no cross-attention: nothing reads a context)
    } else if (have_ctx) {
      if (!d) {
        TapeCaller tc(Tape::R_CTX, ctx);
        int r = launch_cast_f16(ctx, ctx16, ctx16_lo, (int64_t)B * Lctx * cfg_.context_dim, stream);
        if (r) return r;
      }
      f.ctx16 = ctx16; f.ctx16_lo = ctx16_lo;
    } else {
      SDMI_CHECK(ctx_valid_, "ctx == NULL but no cached context for this (B, Lctx); call sdmi_unet_cache_context first");
      f.ctx16 = nullptr; f.ctx16_lo = nullptr;
    }
    if (ctx_only) {
      for_each_layer([&](Layer& L) -> int {
        if (L.kind == L_ATTN) for (int dd = 0; dd < (int)L.tb.size(); ++dd) f.context_kv(L, dd);
        return 0;
      });
    } else {
      // ---- time embedding (util.py:151-171, openaimodel.py:506-511,723-724) and all emb_layers at once ----
      float* temb = f.P<float>((size_t)B * mc);
      float* e1 = f.P<float>((size_t)B * te_);
      float* emb = f.P<float>((size_t)B * te_);
      f.emb_all = f.P<float>((size_t)B * emb_total_);
      f.emb_ld = emb_total_;
      if (!d && t_i64 != nullptr && hint_row >= 0 && hint_row < (int)emb_tab_t_.size()) {
        // every row has the hinted timestep and its emb_layers outputs are in the table: one shared row, nothing to launch
        f.emb_all = emb_tab_ + (size_t)hint_row * emb_total_;
        f.emb_ld = 0;
        f.emb_caller = true;
      } else if (!d) {
        int r;
        {
          TapeCaller tc(Tape::R_T, t_i64 ? (const void*)t_i64 : t_f32);
          r = launch_timestep_embedding(t_i64, t_f32, temb, B, mc, stream);
        }
        if (!r) r = launch_small_linear(temb, mc, te_w0_, te_b0_, e1, te_, B, te_, mc, 0, stream);
        if (!r) r = launch_small_linear(e1, te_, te_w2_, te_b2_, emb, te_, B, te_, te_, 1, stream);
        if (!r) r = launch_small_linear(emb, te_, emb_w_, emb_b_, f.emb_all, emb_total_, B, emb_total_, te_, 1, stream);
        if (r) return r;
      }
      // ---- input blocks ----
      std::vector<Act> hs;
      Act h;
      {
        Layer& L = input_blocks_[0][0];
        // round 6: conv_in emits the GroupNorm statistics of its output itself (the two GroupNorms that read it -- input_blocks.1.0 and, through
        // the skip concat, the last output block -- ran the statistics kernel; rounds 1-5: "conv_in is not an igemm: no fused statistics")
        const char* e_cis = getenv("SDMI_CONV_IN_STATS");                 // (A/B knob, read per call; 0 = the statistics kernel as in rounds 1-5)
        h = f.make_act(f.P<float>((size_t)B * H * W * mc), mc, H, W, (H * W) % 16 == 0 && !(e_cis && atoi(e_cis) == 0));
        IGemmParams st = IGemmParams();                                   // (carrier of the statistics targets only)
        f.attach_gn_targets(st, h);
        if (!d) {
          SDMI_CHECK(cfg_.in_channels <= 16, "conv_in: in_channels <= 16");      // (the UNet's limit; the launcher's own is the first stages' 64)
          TapeCaller tc(Tape::R_X, x);
          int r = launch_conv_in(x, L.w32[0], L.f32[0], h.p, B, cfg_.in_channels, H, W, mc, stream, st.gn_n, st.gn_acc, st.gn_cpg, st.gn_cbase);
          if (r) return r;
        }
        hs.push_back(h);
      }
      for (size_t bi = 1; bi < input_blocks_.size(); ++bi) {
        for (auto& L : input_blocks_[bi]) h = f.run_layer(L, h, nullptr);
        hs.push_back(h);
      }
      for (auto& L : middle_) h = f.run_layer(L, h, nullptr);
      for (auto& blk : output_blocks_) {
        Act skip = hs.back(); hs.pop_back();
        SDMI_CHECK(skip.H == h.H && skip.W == h.W, "skip/h spatial mismatch");
        bool first = true;
        for (auto& L : blk) { h = f.run_layer(L, h, first ? &skip : nullptr); first = false; }
      }
      // ---- output head: GN -> SiLU -> conv3x3 (fp32) ----
      float* hn = f.S<float>((size_t)B * H * W * mc);
      f.groupnorm(h, nullptr, out_gamma_, out_beta_, 1e-5f, 1, nullptr, hn, nullptr);
      if (!d && !f.rc) {
        SDMI_CHECK(cfg_.out_channels <= 32, "conv_out: out_channels <= 32, Cin % 4 == 0");   // (the UNet's limit; the launcher's own is 128)
        TapeCaller tc(Tape::R_OUT, eps_out);
        int r = launch_conv_out(hn, out_w_, out_b_, eps_out, B, H, W, mc, cfg_.out_channels, stream);
        if (r) return r;
      }
    }
    if (f.rc) return f.rc;
    if (d) { persist_bytes = (int64_t)f.persist.peak + 256; scratch_bytes = (int64_t)f.scratch.peak + 256; }
    else {
      SDMI_CHECK(!f.persist.overflow && !f.scratch.overflow, "internal: arena overflow");
      if (have_ctx) ctx_valid_ = true;
    }
  }
  if (bytes_needed) *bytes_needed = persist_bytes + scratch_bytes;
  if (fresh) {
    // (a declaration that matched no argument word: internal error, the executor's result of this call stands but it is not taped)
    if (fresh->broken && !verify_against) {
      static bool noted = false;
      if (!noted) fprintf(stderr, "sdmi: internal: a declared caller pointer (TapeCaller) is in no launch argument; such calls run untaped\n");
      noted = true;
      return 0;
    }
    fresh->bytes_needed = persist_bytes + scratch_bytes;
    fresh->sets_ctx_valid = ctx != nullptr;
    if (verify_against) {
      const Tape& a = *verify_against; const Tape& b = *fresh;
      auto eq3 = [](const dim3& u, const dim3& v) { return u.x == v.x && u.y == v.y && u.z == v.z; };
      bool same = !b.broken && a.ops.size() == b.ops.size() && a.blob == b.blob && a.arg_off == b.arg_off && a.arg_size == b.arg_size &&
                  a.relocs.size() == b.relocs.size();
      for (size_t i = 0; same && i < a.relocs.size(); ++i)
        same = a.relocs[i].off == b.relocs[i].off && a.relocs[i].which == b.relocs[i].which && a.relocs[i].delta == b.relocs[i].delta;
      for (size_t i = 0; same && i < a.ops.size(); ++i) {
        const Tape::Op &p = a.ops[i], &q = b.ops[i];
        same = p.kind == q.kind && p.fn == q.fn && eq3(p.grid, q.grid) && eq3(p.block, q.block) && p.shmem == q.shmem &&
               p.first_arg == q.first_arg && p.nargs == q.nargs && p.ptr == q.ptr && p.value == q.value && p.bytes == q.bytes;
      }
      SDMI_CHECK(same, "SDMI_REPLAY_VERIFY: the retargeted launch tape differs from what the executor launches for this call");
      ++tape_hits_;
    } else {
      ++tape_records_;
    }
    if (tapes_.size() >= kMaxTapes) tapes_.erase(tapes_.begin());
    tapes_.emplace_back(tkey, std::move(fresh));
  }
  return 0;
}

}  // namespace sdmi
