// Text-encoder executor state: HF CLIPTextModel as wrapped by FrozenCLIPEmbedder (clip.cpp) and the LAION-400M model's
// BERTEmbedder transformer (bert.cpp).
#pragma once
#include <string>
#include <vector>

#include "../../include/sdmi.h"
#include "common.h"
#include "unet.h"

namespace sdmi {

struct CLayer {   // CLIPEncoderLayer
  f16* wqkv = nullptr; float* bqkv = nullptr;     // [3C][C], [3C]   q_proj | k_proj | v_proj
  f16* wo = nullptr; float* bo = nullptr;
  f16* w1 = nullptr; float* b1 = nullptr;         // fc1 [I][C]
  f16* w2 = nullptr; float* b2 = nullptr;         // fc2 [C][I]
  float* ln[4] = {nullptr, nullptr, nullptr, nullptr};   // layer_norm1.{weight,bias}, layer_norm2.{weight,bias}
};

// Host plumbing shared by the text encoders: the weight store and the all-set check.  No device code of its own.
class TextEncBase {
 public:
  int set_weight(const char* key, const float* ptr, const int64_t* shape, int ndim, hipStream_t stream);
  int finalize();
  const WeightStore& weights() const { return store_; }

 protected:
  WeightStore store_;           // (slots point into the layer objects of the derived class)
  bool finalized_ = false;
};

class ClipText : public TextEncBase {
 public:
  int build(const sdmi_clip_cfg& cfg);
  // ids int64 [B][L] (device) -> last_hidden_state fp32 [B][L][hidden] (after final_layer_norm)
  int forward(const int64_t* ids, float* out, int B, int L, void* workspace, int64_t ws_bytes, hipStream_t stream, bool dry,
              int64_t* bytes_needed);
  sdmi_clip_cfg cfg_{};

 private:
  std::vector<CLayer> layers_;
  float *tok_ = nullptr, *pos_ = nullptr, *fln_g_ = nullptr, *fln_b_ = nullptr;
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
  int build(const sdmi_bert_cfg& cfg);
  // ids int64 [B][L] (device) -> embeddings fp32 [B][L][dim] (after the final LayerNorm)
  int forward(const int64_t* ids, float* out, int B, int L, void* workspace, int64_t ws_bytes, hipStream_t stream, bool dry,
              int64_t* bytes_needed);
  sdmi_bert_cfg cfg_{};

 private:
  std::vector<BLayer> layers_;
  float *tok_ = nullptr, *pos_ = nullptr, *fln_g_ = nullptr, *fln_b_ = nullptr;
};

}  // namespace sdmi
