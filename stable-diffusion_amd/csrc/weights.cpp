// Weight store of the model handles (weights.h): state_dict tensors -> packed device buffers.
#include "weights.h"

namespace sdmi {

int DevStage::acquire(const float* ptr, int64_t numel, hipStream_t stream) {
  dptr = ptr;
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, ptr);
  const bool on_device = (e == hipSuccess) && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged);
  if (e != hipSuccess) (void)hipGetLastError();
  if (!on_device) {
    SDMI_HIP_OK(hipMalloc((void**)&staged, numel * sizeof(float)));
    SDMI_HIP_OK(hipMemcpyAsync(staged, ptr, numel * sizeof(float), hipMemcpyHostToDevice, stream));
    dptr = staged;
  }
  return 0;
}
int DevStage::release(hipStream_t stream) {
  if (staged) {
    SDMI_HIP_OK(hipStreamSynchronize(stream));
    (void)hipFree(staged);
    staged = nullptr;
  }
  return 0;
}

WeightStore::~WeightStore() {
  for (void* p : owned_) (void)hipFree(p);
}

static size_t numel_of(const WeightSlot& s) {
  size_t n = 1;
  for (int64_t d : s.shape) n *= (size_t)d;
  return n;
}

WeightSlot& WeightStore::expect(const std::string& key, std::vector<int64_t> shape, WKind kind, void* dst, int row0, int buf_rows) {
  WeightSlot s;
  s.key = key; s.shape = std::move(shape); s.kind = kind; s.dst = (void**)dst; s.row0 = row0;
  s.ld = (int)(numel_of(s) / (size_t)s.shape[0]);
  s.buf_rows = buf_rows ? buf_rows : (int)s.shape[0];
  index_[key] = (int)slots_.size();
  slots_.push_back(std::move(s));
  return slots_.back();
}

size_t WeightStore::bytes(const WeightSlot& s) {
  const size_t numel = numel_of(s), rows = (size_t)s.buf_rows * s.ld;
  switch (s.kind) {
    case W_F32: case W_CONV_OUT: case W_GEGLU_B: case W_QKV_LEGACY_B: return numel * sizeof(float);
    case W_F32_ROWS: return rows * sizeof(float);
    case W_CONV: case W_GEGLU_W: return numel * sizeof(f16);
    case W_SPLIT3: case W_CONV_SPLIT3: return 3 * numel * sizeof(f16);
    case W_QKV_LEGACY: return numel * sizeof(f16) * (s.split ? 3 : 1);
    case W_ROWS16: return rows * sizeof(f16);
    case W_ROWS16_PAD64: return (size_t)s.buf_rows * (size_t)round_up(s.ld, 64) * sizeof(f16);
    case W_SPLIT3_ROWS: return 3 * rows * sizeof(f16);
    case W_DROP: return 0;
  }
  return 0;
}

int WeightStore::alloc(void** dst, size_t bytes) {
  if (*dst) return 0;
  SDMI_HIP_OK(hipMalloc(dst, bytes));
  owned_.push_back(*dst);
  return 0;
}

int WeightStore::zero_page() {
  if (zero_) return 0;
  if (alloc((void**)&zero_, 4096)) return -1;
  SDMI_HIP_OK(hipMemset(zero_, 0, 4096));
  return 0;
}

const WeightSlot* WeightStore::missing() const {
  for (const auto& s : slots_)
    if (!s.set && s.kind != W_DROP) return &s;
  return nullptr;
}

std::vector<std::pair<void**, size_t>> WeightStore::buffers() const {
  std::vector<std::pair<void**, size_t>> bufs;
  for (const auto& s : slots_) {
    if (s.kind == W_DROP) continue;
    bool seen = false;
    for (const auto& b : bufs) seen = seen || b.first == s.dst;
    if (!seen) bufs.push_back({s.dst, bytes(s)});
  }
  return bufs;
}

int WeightStore::set(const char* key, const float* ptr, const int64_t* shape, int ndim, hipStream_t stream) {
  auto it = index_.find(key);
  if (it == index_.end()) return fail(std::string("unexpected weight key: ") + key);
  WeightSlot& s = slots_[it->second];
  SDMI_CHECK((int)s.shape.size() == ndim, std::string("rank mismatch for ") + key);
  int64_t numel = 1;
  for (int i = 0; i < ndim; ++i) {
    SDMI_CHECK(shape[i] == s.shape[i], std::string("shape mismatch for ") + key);
    numel *= shape[i];
  }
  if (s.kind == W_DROP) {
    s.set = true;
    return 0;
  }
  DevStage st;
  if (st.acquire(ptr, numel, stream)) return -1;
  const float* dptr = st.dptr;
  int rc = alloc(s.dst, bytes(s));
  if (!rc) switch (s.kind) {
    case W_F32:
      SDMI_HIP_OK(hipMemcpyAsync(*s.dst, dptr, numel * sizeof(float), hipMemcpyDeviceToDevice, stream));
      break;
    case W_F32_ROWS:
      SDMI_HIP_OK(hipMemcpyAsync((float*)*s.dst + (size_t)s.row0 * s.ld, dptr, numel * sizeof(float), hipMemcpyDeviceToDevice, stream));
      break;
    case W_CONV:
      rc = launch_pack_conv_weight(dptr, (f16*)*s.dst, (int)shape[0], (int)shape[1], (int)shape[2], (int)shape[3], stream);
      break;
    case W_SPLIT3:
      rc = launch_pack_split3(dptr, (f16*)*s.dst, (int)shape[0], (int)shape[1], stream);
      break;
    case W_CONV_SPLIT3:
      rc = launch_pack_conv_split3(dptr, (f16*)*s.dst, (int)shape[0], (int)shape[1], (int)shape[2], (int)shape[3], stream);
      break;
    case W_SPLIT3_ROWS:
      rc = launch_pack_split3(dptr, (f16*)*s.dst + (size_t)s.row0 * 3 * s.ld, (int)shape[0], (int)shape[1], stream);
      break;
    case W_CONV_OUT:
      rc = launch_pack_conv_out(dptr, (float*)*s.dst, (int)shape[0], (int)shape[1], stream);
      break;
    case W_ROWS16:
      rc = launch_pack_rows(dptr, (f16*)*s.dst, (int)shape[0], (int)shape[1], s.row0, s.ld, stream);
      break;
    case W_ROWS16_PAD64:
      SDMI_HIP_OK(hipMemsetAsync(*s.dst, 0, bytes(s), stream));
      rc = launch_pack_rows(dptr, (f16*)*s.dst, (int)shape[0], s.ld, 0, (int)round_up(s.ld, 64), stream);
      break;
    case W_QKV_LEGACY:
    case W_QKV_LEGACY_B: {
      // QKVAttentionLegacy (openaimodel.py:361-366) reads the qkv rows as [head][q | k | v][channel]: reference row h * 3d + j * d + i
      // becomes packed row j * C + h * d + i, the [q | k | v] head-major order of the SpatialTransformer's fused projection
      const int R = (int)shape[0], K = s.ld, C = R / 3, d = C / s.heads;
      float* perm = nullptr;
      if (s.kind == W_QKV_LEGACY) SDMI_HIP_OK(hipMalloc((void**)&perm, (size_t)R * K * sizeof(float)));
      float* dst = s.kind == W_QKV_LEGACY ? perm : (float*)*s.dst;
      for (int h = 0; h < s.heads; ++h)
        for (int j = 0; j < 3; ++j)
          SDMI_HIP_OK(hipMemcpyAsync(dst + ((size_t)j * C + (size_t)h * d) * K, dptr + ((size_t)h * 3 * d + (size_t)j * d) * K,
                                     (size_t)d * K * sizeof(float), hipMemcpyDeviceToDevice, stream));
      if (s.kind == W_QKV_LEGACY)
        rc = s.split ? launch_pack_split3(perm, (f16*)*s.dst, R, K, stream) : launch_pack_rows(perm, (f16*)*s.dst, R, K, 0, K, stream);
      if (perm) {
        SDMI_HIP_OK(hipStreamSynchronize(stream));
        (void)hipFree(perm);
      }
      break;
    }
    case W_GEGLU_W:        // weight and bias arrive separately; the weight packer does not need the bias (and vice versa)
      rc = launch_pack_geglu(dptr, nullptr, (f16*)*s.dst, nullptr, (int)shape[0], (int)shape[1], stream);
      break;
    case W_GEGLU_B: {      // permute the bias with the same 32-row interleave: reuse the packer with K = 1 on a [N][1] "matrix"
      f16* tmp = nullptr;
      SDMI_HIP_OK(hipMalloc((void**)&tmp, numel * sizeof(f16)));
      rc = launch_pack_geglu(dptr, dptr, tmp, (float*)*s.dst, (int)shape[0], 1, stream);
      SDMI_HIP_OK(hipStreamSynchronize(stream));
      (void)hipFree(tmp);
      break;
    }
    case W_DROP:
      break;
  }
  if (st.release(stream)) return -1;
  if (rc) return rc;
  s.set = true;
  return 0;
}

}  // namespace sdmi
