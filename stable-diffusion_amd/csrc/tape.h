// Launch tape (round 6): the executor's host cost per UNet call was 11 us per launch, of which ~3.5 us is the HIP launch itself.
// The rest -- a dry pass that sizes the arenas and derives the fusion plan, tuning-table lookups, descriptor fills, environment reads -- produces
// the SAME launch list every time a (B, H, W, Lctx) shape comes back with the same workspace, weights and knobs.  So the list is recorded once
// (kernel pointer, grid, block, the filled parameter structs with their arena pointers, the memsets) and replayed as a flat loop of
// hipLaunchKernel; only the pointers that belong to the CALLER change between calls (x, eps_out, timesteps, context, the row of the timestep
// table).  The executor declares each of them where it hands it to a kernel (TapeCaller: caller range + exact pointer value); while such a scope
// is open, every 8-byte argument word equal to the declared value becomes a relocation {offset, range, value - range base}, and a replay writes
// new base + delta there.  Launches outside a scope are never patched, and the range comes from the declaration, not from the address: the
// caller's buffers may alias or overlap.
//
// Every kernel launch of the library goes through SDMI_LAUNCH (= hipLaunchKernelGGL + the recording hook), every stream memset of a forward
// through sdmi::memset_async.  Recording is thread-local and only active inside UNet::run.  The parameter structs are value-initialised
// (`T p = T();`: zero padding), so the recorded bytes are a function of the launch alone and SDMI_REPLAY_VERIFY compares them whole.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

namespace sdmi {

struct Tape {
  struct Op {
    int kind = 0;                       // 0 kernel launch, 1 memset
    const void* fn = nullptr; dim3 grid, block; unsigned shmem = 0; uint32_t first_arg = 0, nargs = 0;
    void* ptr = nullptr; int value = 0; size_t bytes = 0;
  };
  struct Reloc { uint32_t off; int which; int64_t delta; };   // the 8-byte word at blob[off] = caller range `which` + delta
  enum { R_X = 0, R_OUT, R_T, R_CTX, R_EMB, R_COUNT };
  struct Decl { int which; uint64_t value; bool matched; };     // an open TapeCaller scope
  std::vector<Op> ops;
  std::vector<unsigned char> blob;                    // the parameter bytes of every launch, each argument at its natural alignment
  std::vector<uint32_t> arg_off;                      // per argument: offset into blob
  std::vector<uint32_t> arg_size;
  std::vector<Reloc> relocs;
  uintptr_t caller[R_COUNT] = {0, 0, 0, 0, 0};        // while recording: the base of each caller range
  std::vector<Decl> open;                             // while recording: the declarations in scope
  bool broken = false;                                // a declaration matched no argument word: not a usable tape
  int64_t bytes_needed = 0;
  bool sets_ctx_valid = false;

  void push_arg(const void* src, size_t size, size_t align) {
    size_t off = (blob.size() + align - 1) / align * align;
    blob.resize(off + size);
    memcpy(blob.data() + off, src, size);
    arg_off.push_back((uint32_t)off); arg_size.push_back((uint32_t)size);
    if (open.empty()) return;
    for (uint32_t o = (uint32_t)off; o + 8 <= off + size; o += 8) {      // (off is 8-aligned: so are the pointers inside)
      uint64_t v;
      memcpy(&v, blob.data() + o, 8);
      for (size_t d = open.size(); d-- > 0;) {
        if (v != open[d].value) continue;
        relocs.push_back({o, open[d].which, (int64_t)(v - caller[open[d].which])});
        open[d].matched = true;
        break;
      }
    }
  }
  // point the blob at new caller ranges
  void retarget(const uintptr_t (&nb)[R_COUNT]) {
    for (const Reloc& rl : relocs) {
      const uint64_t v = nb[rl.which] + (uint64_t)rl.delta;
      memcpy(blob.data() + rl.off, &v, 8);
    }
  }
  int replay(hipStream_t s) {
    void* args[64];
    for (const Op& op : ops) {
      hipError_t e;
      if (op.kind == 1) {
        e = hipMemsetAsync(op.ptr, op.value, op.bytes, s);
      } else {
        for (uint32_t i = 0; i < op.nargs; ++i) args[i] = blob.data() + arg_off[op.first_arg + i];
        e = hipLaunchKernel(op.fn, op.grid, op.block, args, op.shmem, s);
      }
      if (e != hipSuccess) return (int)e;
    }
    return 0;
  }
};

extern thread_local Tape* g_tape_rec;        // non-null while UNet::run records

// Declares, for the launches enqueued inside its scope, that `value` is a pointer of caller range `which` (range base: Tape::caller).  A
// null value declares nothing (the pointer is not the caller's in this mode).  A declaration that matches no argument word breaks the tape.
struct TapeCaller {
  Tape* t;
  TapeCaller(int which, const void* value) : t(value ? g_tape_rec : nullptr) {
    if (t) t->open.push_back({which, (uint64_t)(uintptr_t)value, false});
  }
  ~TapeCaller() {
    if (!t) return;
    t->broken = t->broken || !t->open.back().matched;
    t->open.pop_back();
  }
  TapeCaller(const TapeCaller&) = delete;
  TapeCaller& operator=(const TapeCaller&) = delete;
};

template <typename... KArgs>
inline void tape_push_launch(Tape* t, const void* fn, dim3 g, dim3 b, size_t shm, const KArgs&... a) {
  Tape::Op op;
  op.kind = 0; op.fn = fn; op.grid = g; op.block = b; op.shmem = (unsigned)shm;
  op.first_arg = (uint32_t)t->arg_off.size(); op.nargs = (uint32_t)sizeof...(KArgs);
  (t->push_arg(&a, sizeof(KArgs), alignof(KArgs) < 8 ? 8 : alignof(KArgs)), ...);
  t->ops.push_back(op);
}

#if defined(__HIP__) || defined(__HIPCC__)
// hipLaunchKernelGGL + the recording hook.  The arguments are converted to the kernel's parameter types first, so the recorded bytes are
// exactly what the launch passes.
template <typename... KArgs, typename... Args>
inline void launch_rec(void (*kernel)(KArgs...), dim3 g, dim3 b, size_t shm, hipStream_t s, Args&&... a) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "kernel argument count");
  static_assert(sizeof...(KArgs) <= 64, "Tape::replay's argument array");
  if (g_tape_rec) {
    [&](const KArgs&... conv) { tape_push_launch<KArgs...>(g_tape_rec, (const void*)kernel, g, b, shm, conv...); }(static_cast<KArgs>(a)...);
  }
  hipLaunchKernelGGL(kernel, g, b, shm, s, static_cast<KArgs>(a)...);
}

#endif

inline hipError_t memset_async(void* ptr, int value, size_t bytes, hipStream_t s) {
  if (g_tape_rec) {
    Tape::Op op;
    op.kind = 1; op.ptr = ptr; op.value = value; op.bytes = bytes;
    g_tape_rec->ops.push_back(op);
  }
  return hipMemsetAsync(ptr, value, bytes, s);
}

}  // namespace sdmi

#define SDMI_LAUNCH(kernel, grid, block, shmem, stream, ...) ::sdmi::launch_rec(kernel, grid, block, shmem, stream, __VA_ARGS__)
