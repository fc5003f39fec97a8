// First-stage (AutoencoderKL) executor state (see vae.cpp).
#pragma once
#include <string>
#include <vector>

#include "../../include/sdmi.h"
#include "common.h"
#include "unet.h"

namespace sdmi {

enum VKind { V_RES, V_ATTN, V_UP, V_DOWN };

struct VLayer {
  VKind kind = V_RES;
  std::string prefix;
  int cin = 0, cout = 0;
  // V_RES : w16 = {conv1, conv2, nin_shortcut(split3)}, f32 = {norm1.w, norm1.b, conv1.b, norm2.w, norm2.b, conv2.b, nin.b}
  // V_ATTN: w16 = {q, k, v, proj_out},                   f32 = {norm.w, norm.b, q.b, k.b, v.b, proj_out.b}
  // V_UP / V_DOWN: w16 = {conv},                         f32 = {conv.b}
  f16* w16[4] = {nullptr, nullptr, nullptr, nullptr};
  float* f32[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // every MFMA operand of the layer is a split-fp16 pair and its weights are packed for that: all layers of a SDMI_PRECISION_FULL handle,
  // and on a mixed handle the decoder layers Vae::build names (the mid block and the levels at 1 / 16 resolution and below of a six-level stage)
  bool split = false;
  f16* w_up_phase = nullptr;     // V_UP, mixed precision, cin % 64 == 0: [4][cout][4 cin] weights of the conv's four 2x2 phase convs (finalize())
};

class Vae {
 public:
  Vae() = default;
  Vae(const Vae&) = delete;
  Vae& operator=(const Vae&) = delete;

  // attn_level_mask: bit l set = an AttnBlock follows every ResBlock of level l, in the encoder (down.l.attn.i) and in the decoder
  // (up.l.attn.i): the reference's attn_resolutions, resolved to levels by the caller (sdmi_vae_create_attn)
  int build(const sdmi_vae_cfg& cfg, int parts, const sdmi_vae_ext* ext = nullptr, int precision = SDMI_PRECISION_MIXED,
            uint32_t attn_level_mask = 0);
  int set_weight(const char* key, const float* ptr, const int64_t* shape, int ndim, hipStream_t stream);
  int finalize();
  // z [B, embed_dim, H, W] fp32 NCHW -> img [B, out_ch, H*f, W*f] fp32 NCHW; z is multiplied by z_scale first
  // quantize: VQModelInterface.decode without force_not_quantize -- z_scale * z is replaced by its nearest codebook entry first
  int decode(const float* z, float z_scale, float* img, int B, int H, int W, void* workspace, int64_t ws_bytes,
             hipStream_t stream, bool dry, int64_t* bytes_needed, bool quantize = false);
  // img [B, in_channels, H, W] fp32 NCHW -> moments [B, 2*embed_dim, H/f, W/f] fp32 NCHW (double_z; else h [B, embed_dim, H/f, W/f])
  int encode(const float* img, float* moments, int B, int H, int W, void* workspace, int64_t ws_bytes, hipStream_t stream,
             bool dry, int64_t* bytes_needed);

  const WeightStore& weights() const { return store_; }
  int factor() const { return 1 << (cfg_.n_levels - 1); }

  sdmi_vae_cfg cfg_{};
  sdmi_vae_ext ext_{1, 1, 0};       // AutoencoderKL unless created with an extension (include/sdmi.h)
  int parts_ = 0;
  int enc_zc() const { return ext_.double_z ? 2 * cfg_.z_channels : cfg_.z_channels; }    // encoder.conv_out channels
  int enc_ed() const { return ext_.double_z ? 2 * cfg_.embed_dim : cfg_.embed_dim; }      // quant_conv output channels
  bool precise_1x1_ = true;
  // SDMI_PRECISION_FULL: every MFMA operand of the ResBlocks, the resampling convs and the mid-block attention is a split-fp16 pair
  // (vae.cpp: VFwd); fixed at creation, the weights are packed for it
  int precision_ = SDMI_PRECISION_MIXED;
  bool full() const { return precision_ == SDMI_PRECISION_FULL; }
  // levels with attention after every ResBlock; non-zero also moves every mixed-precision attention block of the handle, the mid block's
  // included, to the flash form (vae.cpp: VFwd::attn_block_flash).  0: the handle launches what it launched before the mask existed
  uint32_t attn_level_mask_ = 0;

 private:
  friend struct VFwd;
  std::vector<VLayer> dec_, enc_;
  WeightStore store_;           // (slots point into the VLayer objects and the members below)
  // decoder ends
  float *pq_w_ = nullptr, *pq_b_ = nullptr;                 // post_quant_conv
  float *dci_w_ = nullptr, *dci_b_ = nullptr;               // decoder.conv_in (raw OIHW fp32)
  float *dno_g_ = nullptr, *dno_b_ = nullptr, *dco_w_ = nullptr, *dco_b_ = nullptr;   // decoder.norm_out, conv_out (OHWI fp32)
  // encoder ends
  float *eci_w_ = nullptr, *eci_b_ = nullptr;
  float *eno_g_ = nullptr, *eno_b_ = nullptr, *eco_w_ = nullptr, *eco_b_ = nullptr;
  float *q_w_ = nullptr, *q_b_ = nullptr;                   // quant_conv
  float *cb_ = nullptr, *cb_norm_ = nullptr;                // codebook [n_embed][embed_dim] (quantize.embedding.weight), sum e^2 per row
  int dec_c_end_ = 0, enc_c_end_ = 0;                       // channels entering norm_out
  bool finalized_ = false;
};

}  // namespace sdmi
