// Weight store shared by the UNet, first-stage and text-encoder handles: the table of expected state_dict entries (key -> shape,
// packing kind, device destination), staging of caller tensors, the packing launches and the device allocations they fill.
#pragma once
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "common.h"

namespace sdmi {

// host or device fp32 pointer -> device pointer (staged through a temporary device buffer when it is host memory)
struct DevStage {
  const float* dptr = nullptr; float* staged = nullptr;
  int acquire(const float* ptr, int64_t numel, hipStream_t stream);
  int release(hipStream_t stream);
};

// W_F32 / W_F32_ROWS    fp32 as it is / rows [row0, ..) of a concatenated fp32 matrix (the emb_layers, a q | k | v bias)
// W_CONV / W_CONV_OUT   conv weight OIHW -> fp16 [O][ky,kx,I] / the fp32 OHWI layout of the output convolution
// W_ROWS16              rows [row0, ..) of an fp16 [buf_rows][ld] matrix (a linear, a 1x1 conv, q | k | v concatenations)
// W_ROWS16_PAD64        an fp16 [rows][round_up(ld, 64)] matrix, the columns behind ld zero (the ViT patch embedding: K = 588 -> 640)
// W_SPLIT3 / W_SPLIT3_ROWS / W_CONV_SPLIT3   the split-fp16 forms [w_hi | w_hi | w_lo] of a matrix, of rows of one, of a conv weight
// W_GEGLU_W / W_GEGLU_B the GEGLU projection and its bias, rows interleaved (value32 | gate32)
// W_QKV_LEGACY / W_QKV_LEGACY_B   the AttentionBlock's conv1d qkv weight / bias, its head-interleaved rows (head, q | k | v, channel)
//                       permuted to the [q | k | v] head-major rows launch_split_heads reads
// W_DROP                accepted (shape-checked) and never uploaded -- a checkpoint tensor the forward does not use
enum WKind { W_F32, W_F32_ROWS, W_CONV, W_CONV_OUT, W_ROWS16, W_GEGLU_W, W_GEGLU_B, W_SPLIT3, W_SPLIT3_ROWS, W_CONV_SPLIT3, W_QKV_LEGACY,
             W_QKV_LEGACY_B, W_DROP, W_ROWS16_PAD64 };

struct WeightSlot {
  std::string key;
  std::vector<int64_t> shape;
  WKind kind = W_F32;
  void** dst = nullptr;
  int row0 = 0;          // first row of the destination buffer this tensor fills
  int ld = 0;            // elements of one row of the tensor (= of the destination; a split-fp16 row is 3 ld wide)
  int buf_rows = 0;      // rows of the whole destination buffer
  int heads = 0;         // W_QKV_LEGACY / W_QKV_LEGACY_B: heads of the row permutation
  bool split = false;    // W_QKV_LEGACY: packed split-fp16
  bool set = false;
};

class WeightStore {
 public:
  WeightStore() = default;
  ~WeightStore();
  WeightStore(const WeightStore&) = delete;
  WeightStore& operator=(const WeightStore&) = delete;

  // `dst`: address of the f16* / float* that receives the device buffer (null for W_DROP); it must stay where it is for the store's
  // lifetime.  buf_rows = 0: the tensor is the whole buffer.
  WeightSlot& expect(const std::string& key, std::vector<int64_t> shape, WKind kind, void* dst, int row0 = 0, int buf_rows = 0);
  int set(const char* key, const float* ptr, const int64_t* shape, int ndim, hipStream_t stream);
  static size_t bytes(const WeightSlot& s);          // of the device buffer the slot writes into (several slots may share one)
  const WeightSlot* missing() const;                 // the first slot that still waits for its tensor
  void mark_all_set() { for (auto& s : slots_) s.set = true; }
  int alloc(void** dst, size_t bytes);               // a device buffer this store frees; a no-op where *dst is set
  int zero_page();                                   // 4 KB of zeros for out-of-image conv taps (allocated once)
  const f16* zero() const { return zero_; }
  std::vector<std::pair<void**, size_t>> buffers() const;      // the distinct destinations in slot order, with their bytes
  const std::vector<WeightSlot>& slots() const { return slots_; }

 private:
  std::vector<WeightSlot> slots_;
  std::map<std::string, int> index_;
  std::vector<void*> owned_;
  f16* zero_ = nullptr;
};

}  // namespace sdmi
