// Text-encoder executor state: HF CLIPTextModel as wrapped by FrozenCLIPEmbedder (clip.cpp) and the LAION-400M model's
// BERTEmbedder transformer (bert.cpp); and the CLIP vision tower (ClipVision, clip.cpp) on the same weight store and layer walk.
#pragma once
#include <string>
#include <vector>

#include "../../include/sdmi.h"
#include "common.h"
#include "split16.h"
#include "unet.h"

namespace sdmi {

struct CLayer {   // CLIPEncoderLayer
  f16* wqkv = nullptr; float* bqkv = nullptr;     // [3C][C], [3C]   q_proj | k_proj | v_proj
  f16* wo = nullptr; float* bo = nullptr;
  f16* w1 = nullptr; float* b1 = nullptr;         // fc1 [I][C]
  f16* w2 = nullptr; float* b2 = nullptr;         // fc2 [C][I]
  float* ln[4] = {nullptr, nullptr, nullptr, nullptr};   // layer_norm1.{weight,bias}, layer_norm2.{weight,bias}
};

// One transformer layer as the full-precision walk sees it (both encoders): pre-norm attention and feed-forward, weights packed
// W_SPLIT3_ROWS ([rows][3K] = [hi | hi | lo])
struct TextFullLayer {
  const f16* wqkv; const float* bqkv;      // [3 inner][3 dim]; bias [3 inner] or null (BERT)
  const f16* wo; const float* bo;
  const f16* w1; const float* b1;
  const f16* w2; const float* b2;
  const float* ln[4];
};
struct TextFullDesc {
  int dim = 0, inner = 0, ff = 0, heads = 0, dh = 0, vocab = 0;
  bool causal = false, erf = false;        // CLIP: causal mask, quick_gelu; BERT: no mask, exact-erf GELU
  const float *tok = nullptr, *pos = nullptr, *fln_g = nullptr, *fln_b = nullptr;
  int64_t slab_floats = 0;                 // split-K slabs (the mixed walk's size)
  std::vector<TextFullLayer> layers;
};

// Host plumbing shared by the text encoders: the weight store, the all-set check and the full-precision layer walk.
class TextEncBase {
 public:
  int set_weight(const char* key, const float* ptr, const int64_t* shape, int ndim, hipStream_t stream);
  int finalize();
  const WeightStore& weights() const { return store_; }
  int precision_ = SDMI_PRECISION_MIXED;       // fixed at creation
  bool full() const { return precision_ == SDMI_PRECISION_FULL; }

 protected:
  // SDMI_PRECISION_FULL: every MFMA operand a split-fp16 pair, as attn_block_full (unet.cpp) runs the UNet's transformer blocks:
  // layernorm_split -> split-fp16 GEMM into fp32 -> split_heads x 3 -> attn_split16 (causal or not) -> out-projection with bias and
  // in-place residual -> layernorm_split -> fc1 -> activation producer (hi | lo) -> fc2 with bias and residual; the final LayerNorm
  // writes fp32.  No LayerNorm post-op and no per-head scatter epilogue: both round to fp16.
  int forward_full(const TextFullDesc& t, const int64_t* ids, float* out, int B, int L, void* workspace, int64_t ws_bytes,
                   hipStream_t stream, bool dry, int64_t* bytes_needed);
  // The mixed-precision walk over CLIPEncoderLayers (fp16 MFMA operands, fp32 residual stream x), shared by the text tower (causal) and the
  // vision tower (not causal).  On entry ln = fp16(LayerNorm1 of layer 0 (x)) and the pad keys of vt are zero; on exit x is the encoder output.
  struct MixedBufs { float* x; f16 *ln, *q, *k, *vt, *ao; float* h1; f16* g; };
  void mixed_layers(FwdBase& f, const std::vector<CLayer>& layers, const MixedBufs& b, int B, int L, int C, int I, int H, bool causal);
  void expect_layer(const std::string& prefix, CLayer& L, int64_t C, int64_t I);     // the 16 tensors of one CLIPEncoderLayer
  WKind lin_kind() const { return full() ? W_SPLIT3_ROWS : W_ROWS16; }
  WeightStore store_;           // (slots point into the layer objects of the derived class)
  bool finalized_ = false;
};

class ClipText : public TextEncBase {
 public:
  // projection_dim > 0 declares `text_projection.weight` [projection_dim][hidden] behind the tower's weights (CLIPTextModelWithProjection)
  int build(const sdmi_clip_cfg& cfg, int precision = SDMI_PRECISION_MIXED, int projection_dim = 0);
  // ids int64 [B][L] (device) -> last_hidden_state fp32 [B][L][hidden] (after final_layer_norm)
  int forward(const int64_t* ids, float* out, int B, int L, void* workspace, int64_t ws_bytes, hipStream_t stream, bool dry,
              int64_t* bytes_needed);
  // OpenAI CLIP's encode_text: the tower, then the row at the first maximum of ids[b, :] times text_projection^T, optionally L2-normalised
  // -> out fp32 [B][projection_dim].  The hidden state lives at the head of the workspace; two launches behind the tower (textpool.hip).
  int text_embeds(const int64_t* ids, float* out, int B, int L, int normalize, void* workspace, int64_t ws_bytes, hipStream_t stream, bool dry,
                  int64_t* bytes_needed);
  sdmi_clip_cfg cfg_{};
  int proj_dim_ = 0;

 private:
  std::vector<CLayer> layers_;
  float *tok_ = nullptr, *pos_ = nullptr, *fln_g_ = nullptr, *fln_b_ = nullptr;
  f16* wproj_ = nullptr;                // text_projection.weight: fp16 rows (mixed) or split-fp16 rows [hi | hi | lo] (full)
};

// hidden fp32 [B][L][W] (the final-LayerNorm output), w [E][W] fp16 or [E][3 W] split-fp16 -> out fp32 [B][E] (textpool.hip)
int launch_clip_pool_project(const int64_t* ids, const float* hidden, const f16* w, bool full, float* out, int B, int L, int W, int E,
                             int normalize, hipStream_t s);

// transformers' CLIPVisionModelWithProjection (models/clip/modeling_clip.py: CLIPVisionTransformer + visual_projection): the safety checker's
// tower and FrozenClipImageEmbedder's.  Mixed precision only.
class ClipVision : public TextEncBase {
 public:
  int build(const sdmi_vit_cfg& cfg);
  int tokens() const { const int P = cfg_.image_size / cfg_.patch_size; return 1 + P * P; }
  // pixel_values fp32 [B][3][S][S] (device) -> last_hidden_state [B][T][hidden] (the encoder output; optional), pooled_output [B][hidden]
  // (post_layernorm of row 0; optional), image_embeds [B][projection_dim]
  int forward(const float* px, float* last_hidden, float* pooled, float* image_embeds, int B, void* workspace, int64_t ws_bytes,
              hipStream_t stream, bool dry, int64_t* bytes_needed);
  sdmi_vit_cfg cfg_{};

 private:
  std::vector<CLayer> layers_;
  f16* wpatch_ = nullptr;               // [hidden][vit_kpad(patch)]
  float *cls_ = nullptr, *pos_ = nullptr, *pre_g_ = nullptr, *pre_b_ = nullptr, *post_g_ = nullptr, *post_b_ = nullptr, *wproj_ = nullptr;
};

struct BLayer {   // one ('a', 'f') pair of x_transformer.Encoder
  f16* wqkv = nullptr;                            // [3 inner][dim]   to_q | to_k | to_v (no bias)
  f16* wo = nullptr; float* bo = nullptr;         // to_out [dim][inner]
  f16* w1 = nullptr; float* b1 = nullptr;         // net.0.0 [ff_inner][dim]
  f16* w2 = nullptr; float* b2 = nullptr;         // net.2 [dim][ff_inner]
  float* ln[4] = {nullptr, nullptr, nullptr, nullptr};   // layers.{2i}.0.{weight,bias}, layers.{2i+1}.0.{weight,bias}
};

// BERTEmbedder's TransformerWrapper(return_embeddings=True) (see bert.cpp)
class BertText : public TextEncBase {
 public:
  int build(const sdmi_bert_cfg& cfg, int precision = SDMI_PRECISION_MIXED);
  // ids int64 [B][L] (device) -> embeddings fp32 [B][L][dim] (after the final LayerNorm)
  int forward(const int64_t* ids, float* out, int B, int L, void* workspace, int64_t ws_bytes, hipStream_t stream, bool dry,
              int64_t* bytes_needed);
  sdmi_bert_cfg cfg_{};

 private:
  std::vector<BLayer> layers_;
  float *tok_ = nullptr, *pos_ = nullptr, *fln_g_ = nullptr, *fln_b_ = nullptr;
};

}  // namespace sdmi
