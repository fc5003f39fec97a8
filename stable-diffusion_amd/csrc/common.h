// Shared device/host helpers for the MI355X (gfx950) kernels of libsdmi.
// wave = 64 lanes, MFMA 32x32x16 f16 -> f32, LDS tiles read as ds_read_b128.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <string>

#include "tape.h"

typedef _Float16 f16;
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#ifdef __HIPCC__
// The GroupNorm(32) (+ SiLU) arithmetic of one element, shared by the stand-alone apply kernel (norm.hip) and the convolution that
// applies it while staging its input (conv3halo.hip): one expression, written operation by operation, so both produce the same bits.
__device__ __forceinline__ float gn_apply_elem(float v, float mean, float rstd, float gamma, float beta, int silu) {
  float t = __builtin_fmaf((v - mean) * rstd, gamma, beta);
  if (silu) t = t * __builtin_amdgcn_rcpf(1.0f + __expf(-t));
  return t;
}
// ... with the scale-shift ("FiLM") modulation of a use_scale_shift_norm ResBlock between the affine and the SiLU (openaimodel.py:267-271:
// out_norm(h) * (1 + scale) + shift, then SiLU): the same two expressions around one more fused multiply-add
__device__ __forceinline__ float gn_apply_film_elem(float v, float mean, float rstd, float gamma, float beta, float scale, float shift,
                                                    int silu) {
  float t = __builtin_fmaf((v - mean) * rstd, gamma, beta);
  t = __builtin_fmaf(t, 1.0f + scale, shift);
  if (silu) t = t * __builtin_amdgcn_rcpf(1.0f + __expf(-t));
  return t;
}
// GroupNorm statistics words (see GroupNormParams::acc): add one fp32 partial / read a folded total
__device__ __forceinline__ void gn_acc_add(unsigned long long* dst, float v) {
  const double d = (double)v;
  const double hi = rint(d);
  atomicAdd(dst, (unsigned long long)(long long)hi);
  atomicAdd(dst + 1, (unsigned long long)__double2ll_rn((d - hi) * 1099511627776.0));
}
__device__ __forceinline__ double gn_acc_value(long long hi, long long lo) {
  return (double)hi + (double)lo * (1.0 / 1099511627776.0);
}
// the two words gn_acc_add adds for one fp32 partial (same expressions: a kernel that sums its partials in registers instead of
// through the accumulator words arrives at the same integers)
__device__ __forceinline__ void gn_fixed_split(float v, long long* hi, long long* lo) {
  const double d = (double)v;
  const double h = rint(d);
  *hi = (long long)h;
  *lo = __double2ll_rn((d - h) * 1099511627776.0);
}
// {mean, rstd} of a group from its folded totals {sum, sum of squares} (integer + 2^-40 fraction words), n elements: ONE expression
// for every kernel that normalises (norm.hip's apply kernel, the split-K reduction that applies a GroupNorm) -- same bits
__device__ __forceinline__ void gn_mean_rstd(long long s, long long sl, long long ss, long long ssl, double n, float eps,
                                             float* mean, float* rstd) {
  const double m = gn_acc_value(s, sl) / n;
  double var = gn_acc_value(ss, ssl) / n - m * m;
  if (var < 0.0) var = 0.0;
  *mean = (float)m;
  *rstd = (float)(1.0 / sqrt(var + (double)eps));
}
#endif

namespace sdmi {

// thread-local error text surfaced through sdmi_last_error()
void set_error(const std::string& msg);
int fail(const std::string& msg);   // sets the error, returns -1

#define SDMI_HIP_OK(expr)                                                                    \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return ::sdmi::fail(std::string(#expr) + ": " + hipGetErrorString(_e));                \
  } while (0)

#define SDMI_CHECK(cond, msg)                                                                \
  do {                                                                                       \
    if (!(cond)) return ::sdmi::fail(std::string("check failed: ") + #cond + " -- " + (msg)); \
  } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// ----------------------------------------------------------------------------------------------
// Implicit-GEMM descriptor:  out[M,N] (+epilogue) = gatherA[M,K] * W[N,K]^T
//   A is fp16 NHWC activations (one or two channel-concatenated sources), gathered as a
//   1x1 or 3x3 (stride 1/2, optional nearest-x2 upsampled input) convolution; a Linear is ksize=1.
//   W is fp16 [N][K], K ordered (64-channel chunk, ky, kx, channel within chunk); for 1x1 / Linear simply [N][Cin]
//   -- packed once by small.hip.  Every source is a multiple of 32 channels; the chunks are per source, and the last chunk of a
//   source of 32 (mod 64) channels is 32 wide (launch_pack_conv_weight_src takes the source split).
// ----------------------------------------------------------------------------------------------
enum EpiMode { EPI_PLAIN = 0, EPI_GEGLU = 1, EPI_HEADS = 2 };

// Output stores of the big producers (GEMM epilogues, split-K reduce, GroupNorm-apply, LayerNorm, attention): nothing inside the
// producing kernel reads them back, the next kernel does.  -DSDMI_NT_STORES marks them non-temporal (experiment: does streaming
// them out shorten the write-back at the kernel boundary?  SDMI_CXXFLAGS=-DSDMI_NT_STORES SDMI_LIB_OUT=libsdmi_nt.so build.py).
#ifdef SDMI_NT_STORES
#define SDMI_ST(T, ptr, val) __builtin_nontemporal_store((T)(val), (T*)(ptr))
#else
#define SDMI_ST(T, ptr, val) (*(T*)(ptr) = (T)(val))
#endif
// Cache policy of the WEIGHT tiles' LDS-DMA loads in the GEMM kernels (igemm / conv3halo / gemm_split16): aux bits of
// raw_ptr_buffer_load_lds, 0 = default, 2 = nt (MI355X_MICROARCH.md "nt-weights": issued -> landed -18 % on a stream that one CU
// reads once, -6 % end to end where every CU re-reads the slices).  -DSDMI_W_AUX=2 is a build experiment (round 4).
#ifndef SDMI_W_AUX
#define SDMI_W_AUX 0
#endif
// Write-through output stores (round 4, default): the 16-byte fp32 output stores of the GEMM epilogues, the split-K reduce and
// GroupNorm-apply carry the sc1 bit, i.e. they are written THROUGH the XCD's L2 while the kernel runs instead of sitting dirty in
// it until the end-of-kernel write-back (MI355X_MICROARCH.md: a boundary costs + dirty bytes / 6 TB/s; `nt` is not write-through,
// sc1 is; a 16-byte sc1 store costs what a plain one does, narrower ones are one fabric write each).  Same values, same addresses:
// bit-identical.  Same-box A/B (profiles/wt_stores_r04.txt): -0.03 ms per UNet call (-0.5 %), first-stage decode unchanged;
// -DSDMI_WT_STORES=2 (the 8-byte fp16 stores as well) measured the same as 1, -DSDMI_WT_STORES=0 = plain stores.
// base = wave-uniform tensor base, off = element offset.  The buffer instruction takes a 32-bit byte offset checked against 2^31
// records: a lane whose byte offset does not fit (outputs beyond 2 GB: first-stage decodes at 768 x 768 with 4+ images, 1024 x 1024
// with 3+) takes the plain 64-bit store instead -- same value, same address; a store past 2^31 would otherwise be dropped by the range
// check and one past 2^32 would wrap onto an earlier sample.
#ifndef SDMI_WT_STORES
#define SDMI_WT_STORES 1
#endif
#if defined(__HIPCC__) && SDMI_WT_STORES >= 1
typedef unsigned sdmi_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned sdmi_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void sdmi_st_wt16(const void* base, size_t byte_off, f32x4 v) {
  if (__builtin_expect(byte_off < (size_t)0x80000000u - 16, 1)) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)0x80000000, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(sdmi_u32x4, v), r, (int)byte_off, 0, 16);
  } else {
    *(f32x4*)((char*)base + byte_off) = v;
  }
}
__device__ __forceinline__ void sdmi_st_wt8(const void* base, size_t byte_off, f16x4 v) {
  if (__builtin_expect(byte_off < (size_t)0x80000000u - 16, 1)) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)0x80000000, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(sdmi_u32x2, v), r, (int)byte_off, 0, 16);
  } else {
    *(f16x4*)((char*)base + byte_off) = v;
  }
}
#define SDMI_ST_F32X4(base, off, val) sdmi_st_wt16((base), (size_t)(off) * 4, (val))
#if SDMI_WT_STORES >= 2
#define SDMI_ST_F16X4(base, off, val) sdmi_st_wt8((base), (size_t)(off) * 2, (val))
#else
#define SDMI_ST_F16X4(base, off, val) SDMI_ST(f16x4, (base) + (off), (val))
#endif
#else
#define SDMI_ST_F32X4(base, off, val) SDMI_ST(f32x4, (base) + (off), (val))
#define SDMI_ST_F16X4(base, off, val) SDMI_ST(f16x4, (base) + (off), (val))
#endif

struct IGemmParams {
  const f16* a0 = nullptr; const f16* a1 = nullptr; const f16* a2 = nullptr;   // A sources, channel concat [a0 | a1 | a2]
  int c0 = 0, c1 = 0, c2 = 0;                          // channels taken from each source (Cin = c0 + c1 + c2)
  int lda0 = 0, lda1 = 0, lda2 = 0;                    // row pitch (elements) of each source
  int B = 1, Hin = 1, Win = 1;                         // source spatial dims (M = B*Hout*Wout)
  int Hout = 1, Wout = 1;
  int ksize = 1, stride = 1, up = 0;
  int pad = 1;                                         // 3x3 only: 1 = symmetric zero pad; 0 = pad right/bottom only (taps at +0..+2)
  const f16* w = nullptr;                              // [N][K]
  int M = 0, N = 0, K = 0;
  // K of the reference op when the descriptor executes more (the K-concatenated 3-pass split-fp16 1x1 convs: K = 3 * k_alg);
  // 0 = K.  Only the profiler's algorithmic FLOP count reads it.
  int k_alg = 0;
  // split-fp16 dense GEMM (gemm_split16.hip): a0 = high halves, a1 = low halves of the activation ([M][K], pitch lda0), w =
  // packed [N][ldw >= 3 K] = [hi | hi | lo]; out = a_hi w_hi^T + a_lo w_hi^T + a_hi w_lo^T.  K = the reference op's K.
  int split16 = 0;
  int ldw = 0;                                         // weight row pitch (elements) of the split-fp16 GEMM
  // epilogue
  int mode = EPI_PLAIN;
  const float* bias = nullptr;                         // [N]
  const float* rowvec = nullptr; int ld_rowvec = 0;    // per-batch vector [B][ld_rowvec] added to every row of batch b
  const float* residual = nullptr; int ldr = 0;        // fp32 [M][ldr]
  float* out_f32 = nullptr; f16* out_f16 = nullptr; int ldo = 0;   // either / both
  f16* out_lo = nullptr;                               // optional (plain mode): fp16(v - float(fp16(v))), the low half of a split-fp16 operand
  // optional (plain mode): LayerNorm of the finished output rows -> ln_out fp16 [M][N] (needs out_f32 with ldo == N);
  // launch_igemm issues the layernorm kernel after the GEMM (and its split-K reduce).  A reduce kernel with the
  // LayerNorm folded in (one wave per row) was measured and was no faster than the two launches.
  const float* ln_gamma = nullptr; const float* ln_beta = nullptr; f16* ln_out = nullptr; float ln_eps = 1e-5f;
  // ---- LayerNorm folded into the CONSUMING GEMM (attention.py:211-215: x + attn1(norm1(x)), ... -- no LayerNorm launch) --------
  //   sum_k LN(x)_k W_nk = rstd_m * ( sum_k (gamma_k x_k) W_nk  -  mean_m * cs_n ) + d_n,   cs_n = sum_k gamma_k W_nk,
  //                                                                                          d_n  = sum_k beta_k W_nk (+ bias_n)
  // Producer side (plain mode, the GEMM whose output rows x a LayerNorm reads): beside the fp32 stream it stores the operand
  // fp16(gamma_n * x) through out_f16 (f16_scale = gamma: one rounding, as the stand-alone kernel rounds LN(x) once) and the
  // {sum, sum of squares} of every row over each 32-column block of its tile: lnp_out[(n / 32) * M + m] (float2).  Needs the
  // 16-byte epilogue (full tiles inside one sample, N % BN == 0: the launcher picks such a tile) and no split-K.
  const float* f16_scale = nullptr;                    // [N] fp32, multiplies the out_f16 copy only
  float* lnp_out = nullptr;                            // [N / 32][M][2] fp32 row-statistics partials
  // Consumer side (any mode): a0 = that fp16(gamma * x) operand [M][K]; lnf_part = its row partials ([lnf_npart = K / 32][M][2]),
  // folded per row in the prologue (fp64) into {mean, rstd}; the epilogue turns every accumulator into
  // rstd_m * (acc - mean_m * lnf_cs[n]) + lnf_d[n] before its mode-specific part (bias must be NULL: it is inside lnf_d).
  const float* lnf_part = nullptr; int lnf_npart = 0; float lnf_eps = 1e-5f;
  const float* lnf_cs = nullptr; const float* lnf_d = nullptr;
  // EPI_HEADS: N = nseg * C, column n -> segment n / C, head (n % C) / dh, dd = n % dh
  //   seg_kind 0: row layout   dst[((b*heads + head) * ntok + tok) * dh + dd]
  //   seg_kind 1: transposed   dst[((b*heads + head) * dh + dd) * ntok_pad + tok]
  f16* seg_dst[3] = {nullptr, nullptr, nullptr};
  int seg_kind[3] = {0, 0, 0};
  int heads = 0, dh = 0, ntok = 0, ntok_pad = 0, segC = 0;
  // split-K (plain mode only): every split stores its partial tile into a private fp32 slab of splitk_ws
  // ([split][M][N]); a second kernel sums the slabs in a fixed order and applies the epilogue (deterministic).
  int splitk = 1;                                      // 1 none, 0 auto, >1 forced
  float* splitk_ws = nullptr; int64_t splitk_ws_floats = 0;
  // counters, zero before the first launch: the grid barrier of the GroupNorm-applying reduction (igemm.hip, COOP_BAR_INTS)
  // uses the tail.  (The fused reduction of the kernels' splitk_fused arm -- the last block of a tile to arrive sums the
  // splits -- lost its A/B, profiles/splitk_fused_r02.txt: no launcher enables it.)
  int* splitk_cnt = nullptr; int splitk_cnt_ints = 0;
  int nkt = 0;                                         // set by the launcher: k-tiles of the whole K (igemm_nkt: a source of 32 (mod 64) channels ends in a half tile)
#ifdef SDMI_IGEMM_TIMING
  long long* dbg_times = nullptr;                      // timing build only: 6 s_memtime slots per workgroup (5 used)
  int dbg_abl = 0;                                     // timing build only (SDMI_EPI_ABL): 1 no residual loads, 2 no GroupNorm statistics, 4 no output stores
#endif
  int splitk_fused = 0;                                // set by the launcher
  // set by the launcher (round 4): the unfused split-K slabs hold whole TILES in the MFMA register order -- slab float index
  // ((split * ntiles + tile) * BM * BN) + ((i * TN + j) * 4 + r4) * (NT * 4) + thread * 4 + e -- instead of [split][M][N]: a lane
  // stores its 4 consecutive accumulator rows of a column as ONE 16-byte write-through store (a wave writes 1 KB runs; the
  // row-major layout takes 4-byte stores, 128-byte runs), and splitk_reduce_tiled_kernel turns 4 x 4 blocks between 4 adjacent
  // lanes back into row-major quads.  slab_bm / bn / wm / wn: the tile geometry the reduction needs to decode it.
  int slab_tiled = 0, slab_bm = 0, slab_bn = 0, slab_wm = 0, slab_wn = 0;
  int slab_sh_qpt = 0, slab_sh_nt = 0, slab_sh_tn = 0, slab_sh_wn = 0;      // log2 of BM * BN / 4, threads, TN, WARPS_N
  int epi_vec = 0;                                     // set by the launcher: 16-byte epilogue (pointer / pitch alignment checked there)
  int tile_n_fastest = 0;                              // set by the launcher: tile numbering inside an XCD's range
  const f16* zero_page = nullptr;                      // >= 16 bytes of zeros (for out-of-image taps)
  // optional (plain mode): GroupNorm(32) statistics of the finished output for up to two consuming GroupNorms -- the
  // output's channels are channels [gn_cbase, gn_cbase + N) of that GroupNorm's (possibly concatenated) input with
  // gn_cpg channels per group; gn_acc = its accumulator region (GroupNormParams::acc).  Needs Hout*Wout % 32 == 0.
  int gn_n = 0;
  long long* gn_acc[2] = {nullptr, nullptr};
  int gn_cpg[2] = {0, 0}, gn_cbase[2] = {0, 0};
  unsigned long long gn_magic[2] = {0, 0};             // ceil(2^40 / gn_cpg), filled by the launcher
  // optional (plain mode, round 4): GroupNorm(32) (+ SiLU) of the finished OUTPUT applied by the split-K reduction itself --
  // ResBlock conv1 -> out_layers' GroupNorm + SiLU -> conv2 (openaimodel.py:225-231).  When this GEMM ends up split, the
  // geometry fits and SDMI_REDUCE_GN_XCD is on (splitk_reduce_tiled_kernel<true>: the reduction takes the statistics behind a
  // grid barrier and stores pgn_out = fp16(SiLU(GN(v))) -- the conv2 operand; no GroupNorm-apply launch, and the fp32 value v
  // is not stored unless pgn_keep_f32), *pgn_applied is set to 1; otherwise it is left alone and the caller runs its
  // GroupNorm-apply launch as before.
  const float* pgn_gamma = nullptr; const float* pgn_beta = nullptr; float pgn_eps = 1e-5f; int pgn_silu = 1;
  f16* pgn_out = nullptr;                              // [M][N] fp16
  int pgn_keep_f32 = 0;                                // also store out_f32 (someone besides that GroupNorm reads it)
  int* pgn_applied = nullptr;                          // host flag, written by the launcher
  // filled by the launcher: ceil(2^40 / (Hout*Wout)) and ceil(2^40 / Wout) for the kernel's division-free row split
  unsigned long long magic_hw = 0, magic_w = 0, magic_w2 = 0;   // (magic_w2: Wout + 2, halo-staged conv)
  int log2w = 0;
  // ---- unused: the GroupNorm-folding convolutions that read these fields were removed (they lost their A/B); the fields stay
  // so that the layout of this by-value kernel argument does not change.
  const float* xf0 = nullptr; const float* xf1 = nullptr;
  const long long* gn_in_acc = nullptr;
  const float* gn_in_gamma = nullptr; const float* gn_in_beta = nullptr; float gn_in_eps = 1e-5f; int gn_in_silu = 1;
  f16* raw_hi = nullptr; f16* raw_lo = nullptr;
  f16* gn_scratch = nullptr;
  unsigned long long magic_cpg_in = 0;                 // launcher: ceil(2^40 / ((c0 + c1) / 32))
  // halo-staged conv geometry (launcher): output rows per image in a tile, images per tile, log2(pixels per image part)
  int halo_thi = 0, halo_ipt = 1, log2_tpi = 30;
  unsigned long long magic_hpi = 0;
  // ---- 1x1 tail of a halo-staged conv (conv3halo.hip, TAIL instantiations): out += cat(tail_a0, tail_a1, tail_a2)[M][tail_kt] tail_w[N][tail_kt]^T
  // accumulated into the conv's own accumulators behind its chunk loop -- a ResBlock's skip_connection inside conv2's launch
  // (openaimodel.py:233-240,263-276: skip_connection(x) + h).  Every source is tail_c channels (a multiple of 64) of an fp16 [M][tail_ld] buffer
  // whose rows are the conv's output pixels; tail_kt = tail_c (single pass, W_CONV weights) or 3 tail_c ([hi | lo | hi] against W_SPLIT3's
  // [w_hi | w_hi | w_lo]).  tail_kt = 0: no tail.  The tail's k-tiles are dealt over the conv's splits in contiguous ranges (tail_split_range).
  const f16* tail_a0 = nullptr; const f16* tail_a1 = nullptr; const f16* tail_a2 = nullptr;
  int tail_c = 0, tail_ld = 0;
  const f16* tail_w = nullptr;
  int tail_kt = 0;
};
// k-tiles [begin, end) of a tail of nkt k-tiles that split `split` of nsplit runs: contiguous, every k-tile exactly once, empty ranges allowed
// (host and device: the kernel and the launcher's checks use this one expression)
__host__ __device__ static inline void tail_split_range(int nkt, int nsplit, int split, int* begin, int* end) {
  *begin = (int)(((long long)split * nkt) / nsplit);
  *end = (int)(((long long)(split + 1) * nkt) / nsplit);
}

constexpr int SDMI_NUM_TILES = 22;   // tile ids 0 .. 21 (14..17: halo-staged 3x3 conv), see kTiles in igemm.hip and include/sdmi.h
struct IGemmTune {        // runtime knobs (tests sweep them; the executor takes the tuning table's choice)
  int tile = -1;          // -1 auto (tuning table, then heuristic); else a tile id
  int dma = -1;           // -1 default, 0 register-staged loads, 1 global_load_lds
};

int launch_igemm(const IGemmParams& p, const IGemmTune& tune, hipStream_t stream);
// host only: will launch_igemm run this auto-configured 3x3 conv (with the tail fields it carries) on a halo-staged tile?  (igemm.hip)
bool igemm_plans_halo(const IGemmParams& p);
// host only: will the executor run this Upsample conv (`p` = its KIND_3X3_UP launch) as the four 2x2 phase convs of one ksize = 2 launch?  (igemm.hip)
bool igemm_plans_up_phase(const IGemmParams& p);
// ... and the IGemmParams of that launch: rows = the SOURCE pixels of one phase (Hout x Wout = Hin x Win, M = B Hin Win), K = 4 Cin, w = the
// derived [4][N][4 Cin] weights (launch_up_phase_weights); bias, outputs (4 M rows of pitch ldo) and statistics targets as they were
static inline IGemmParams up_phase_of(const IGemmParams& p, const f16* w_phase) {
  IGemmParams q = p;
  q.ksize = 2; q.Hout = p.Hin; q.Wout = p.Win; q.M = p.B * p.Hin * p.Win; q.K = 4 * p.c0; q.w = w_phase; q.splitk = 0;      // (splitk 0: the table's tile; the launcher runs it unsplit)
  return q;
}
// host only: the tuning table's (tile, split-K) of a key; kt = K of a 1x1 tail (tried first, then the plain conv's entry).  0 found, 1 no entry
int tune_lookup(int M, int N, int K, int ksize, int stride, int up, int mode, int splitk_req, int kt, int* tile, int* splitk);
// fp16 range guard (range.hip, debug): scan an fp16 activation buffer a launch just wrote; see SDMI_CHECK_RANGE
bool range_check_enabled();
uint64_t tune_generation();
bool tune_collecting();                 // a tuning collection is running (igemm.hip): launches must go through the executor
int range_check_set(int enable);
int range_scan(const char* what, const f16* p, int64_t n, hipStream_t stream);
int range_report(std::string* json);

// in-situ tuning (igemm.hip): begin a collection run, select the candidate index for the following launches, end it
// (folds the timings into the table and writes it to `path`, or next to libsdmi.so when NULL)
int tune_begin();
int tune_round(int r);
int tune_end(const char* path, int* n_keys);
int tune_dump(std::string* out);
// out = sum_s slab[s] + bias + rowvec[batch] + residual (fixed order); uses M, N, Hout*Wout, splitk_ws, out_f32/out_f16
int launch_splitk_reduce(const IGemmParams& p, int nsplit, hipStream_t stream);

// Row-strip chain (rowchain.hip): GEGLU -> FF-out -> proj_out of a SpatialTransformer as ONE launch (attention.py:58-64,214,258-261).
// A workgroup owns 32 token rows for the whole chain; the weights stream through one LDS-DMA ring.  `epi` is the descriptor of the
// proj_out GEMM (M, N = K = C, B, Hout * Wout = rows per sample, bias, residual = the SpatialTransformer's input, out_f32 / ldo,
// optional fp16 copy and GroupNorm-statistics targets); the operand pointers of that descriptor are not read.
struct FfTailParams {
  const f16* ln = nullptr;        // [M][C] fp16(gamma3 * t): the LayerNorm-folded GEGLU operand its producer stored (IGemmParams::f16_scale)
  const float* lnp = nullptr;     // [C / 32][M][2] row partials of t (IGemmParams::lnp_out)
  float ln_eps = 1e-5f;
  const float* csd = nullptr;     // LayerNorm-fold column terms of the packed GEGLU columns, per hidden chunk of C: [4][cs 2C | d 2C]
  const f16* wgg = nullptr;       // [8C][C] packed GEGLU weights (value32 | gate32 interleave)
  const f16* wff2 = nullptr;      // [C][4C]
  const float* bff2 = nullptr;    // [C]
  const float* t = nullptr;       // [M][C] fp32 token stream (residual of FF-out)
  const f16* wpo = nullptr;       // [C][3C] split-fp16 proj_out weights [hi | hi | lo]
  // the out-projection of attn2 in front (a16 != nullptr; `ln` / `lnp` are then unused, t is updated in place): t += a16 Wo^T + bo,
  // the GEGLU operand fp16(ln_gamma * t) and its row statistics stay on the CU                 attention.py:213, 191-192
  const f16* a16 = nullptr;       // [M][C] fp16: the cross-attention output rows
  const f16* wo = nullptr;        // [C][C] attn2.to_out weights
  const float* bo = nullptr;      // [C]
  const float* ln_gamma = nullptr;  // [C] norm3 weight
#ifdef SDMI_RC_TIMING
  long long* dbg = nullptr;       // timing build only: [workgroups][128] s_memtime stamps
#endif
  IGemmParams epi;
};
bool ff_tail_supported(int C, int M, int rows_per_sample);
int launch_ff_tail(const FfTailParams& p, hipStream_t stream);

// Row-strip chain kernel, the HEAD of a SpatialTransformer (rowchain.hip): GroupNorm-apply -> proj_in -> (norm1 folded) q | k | v
//   t = proj_in(norm(x)) + b;  q | k | v = norm1(t) Wqkv^T        ldm/modules/attention.py:254-256 (norm, proj_in), :212 + :170-176 (attn1's
// projections) as ONE launch instead of GroupNorm-apply, the split-fp16 proj_in GEMM and the q|k|v GEMM.  Same arithmetic in the same order as
// those launches (the outputs are the same bits).
struct StHeadParams {
  const f16* a16 = nullptr;        // (launch_st_mid only) [M][C] fp16: the self-attention output rows, operand of the out-projection
  const float* x = nullptr;        // [M][C] fp32: the SpatialTransformer's input (NHWC rows)
  const long long* gn_acc = nullptr;   // GroupNorm statistics accumulators of x (GroupNormParams::acc, complete before the launch)
  const float* gn_gamma = nullptr; const float* gn_beta = nullptr; float gn_eps = 1e-6f;
  const f16* w_in = nullptr;       // [C][3C] split-fp16 proj_in weights [hi | hi | lo]
  const float* b_in = nullptr;     // [C]
  float* t = nullptr;              // [M][C] fp32 out: the token stream
  const float* ln_gamma = nullptr; // norm1 weight: the q|k|v operand is fp16(gamma * t) (IGemmParams::f16_scale), beta lives in lnf_d
  float ln_eps = 1e-5f;
  const f16* wqkv = nullptr;       // [3C][C] attn1 to_q | to_k | to_v
  const float* lnf_cs = nullptr; const float* lnf_d = nullptr;   // [3C] LayerNorm-fold column terms (IGemmParams::lnf_cs / lnf_d)
  f16* q = nullptr; f16* k = nullptr;  // [B * heads][ntok][dh]
  f16* vt = nullptr;               // [B * heads][dh][ntok_pad]
  int M = 0, B = 0, ntok = 0, ntok_pad = 0, heads = 0, dh = 0, C = 0;
  // (launch_st_mid, optional) the cross-attention behind to_q inside the launch: cached context K [B * heads][nkv][dh] and V^T
  // [B * heads][dh][nkv_pad] (TBlock::ck / cvt), softmax scale, the attention output rows ao_out [M][C] fp16; `q` is then not written
  const f16* ctx_k = nullptr; const f16* ctx_vt = nullptr; int ctx_nkv = 0, ctx_nkv_pad = 0; float ctx_scale = 0.f; f16* ao_out = nullptr;
#ifdef SDMI_RC_TIMING
  long long* dbg = nullptr;
#endif
};
bool st_head_supported(int C, int M, int ntok, int ntok_pad, int heads, int dh);
int launch_st_head(const StHeadParams& p, hipStream_t stream);
// ... and the MIDDLE of a BasicTransformerBlock on the same kernel: t += a16 Wo^T + b_in in place (w_in = Wo [C][C] plain fp16), q = norm2(t) Wq^T
// (ln_gamma = norm2 weight, wqkv = Wq [C][C], lnf_cs / lnf_d [C]; k / vt / x / gn_* unused)     attention.py:212-213, 170, 191-192
int launch_st_mid(const StHeadParams& p, hipStream_t stream);

// ResBlock in_layers / out_layers as one launch (gnconv.hip): out = conv3x3(SiLU(GroupNorm32(cat(x0, x1)))) + bias (+ row vector, + residual)
//   openaimodel.py:201-204, 225-231; util.py:199-216.  A workgroup owns 32 pixels x ALL 320 output channels: the halo is normalised once.
struct GnConvParams {
  const float* x0 = nullptr; const float* x1 = nullptr; int c0 = 0, c1 = 0;      // fp32 NHWC sources (channel concat; c0 % 64 == 0)
  const long long* gn_acc = nullptr;        // GroupNorm statistics accumulators of cat(x0, x1) (GroupNormParams::acc, complete before the launch)
  const float* gn_gamma = nullptr; const float* gn_beta = nullptr; float gn_eps = 1e-5f;
  const f16* w = nullptr;                   // packed conv weights [320][9 Cin] (launch_pack_conv_weight)
#ifdef SDMI_RC_TIMING
  long long* dbg = nullptr;                 // timing build only: [workgroups][16] cycle stamps
#endif
  IGemmParams epi;                          // the convolution's descriptor (conv3(): B, H, W, N = 320, K = 9 Cin) with its epilogue fields
};
bool gn_conv3_supported(int B, int H, int W, int c0, int c1, int Cout);
int launch_gn_conv3(const GnConvParams& p, hipStream_t stream);

// Flash attention over per-head layouts produced by EPI_HEADS
struct AttnParams {
  const f16* q = nullptr;    // [BH][nq][d]
  const f16* k = nullptr;    // [BH][nkv][d]
  const f16* vt = nullptr;   // [BH][d][nkv_pad]   (nkv_pad = round_up(nkv, 8), pad tokens zero)
  f16* out = nullptr;        // [B][nq][heads*d]  (heads merged, '(b h) n d -> b n (h d)')
  int BH = 0, heads = 0, nq = 0, nkv = 0, nkv_pad = 0, d = 0;
  float scale = 1.f;
  int nw = 0;                // waves per workgroup (0 = auto): each wave owns 32 queries
  int causal = 0;            // 1: key j attends only to queries i >= j (CLIP text model); needs nq == nkv
  int prio = 0;              // 1: s_setprio 1 for the second-dispatched half of an 8-wave workgroup (measured no faster; no caller sets it)
  int pingpong = 0;          // unused (its ping-pong kernel lost its A/B and was removed); kept for the by-value layout
};
int launch_attention(const AttnParams& p, hipStream_t stream);
// head dims 192 .. 1024 in steps of 64, non-causal (attn_wide.hip); launch_attention dispatches to it by d
int launch_attention_wide(const AttnParams& p, hipStream_t stream);
// the one-pass kernel for at most 256 keys (attn_small.hip), nw = 1, 2 or 4 waves per workgroup; launch_attention routes to it by
// attn_small_takes (attn.hip: the routing table and the SDMI_ATTN_SMALL knob)
bool attn_small_supported(int d, int nq, int nkv, int causal);
int launch_attention_small(const AttnParams& p, int nw, hipStream_t stream);
int attn_small_takes(int d, int nq, int nkv, int causal, int knob);    // waves per workgroup, or 0 = the ring kernel

// GroupNorm(32) (+SiLU) over fp32 NHWC, channel-concat of two sources, fp16 or fp32 output
struct GroupNormParams {
  const float* x0 = nullptr; const float* x1 = nullptr; int c0 = 0, c1 = 0;
  int B = 0, HW = 0;
  const float* gamma = nullptr; const float* beta = nullptr; float eps = 1e-5f;
  int silu = 0;
  int stats_only = 0;          // 1: only fill the statistics accumulators (consumed by a launch that normalises its own input: gnconv.hip, rowchain.hip)
  int skip_stats = 0;          // 1: the accumulators were already filled by the producing GEMM epilogues (IGemmParams::gn_*)
  f16* out_f16 = nullptr;      // [B*HW][C] normalised (+SiLU)
  float* out_f32 = nullptr;    // same in fp32 (used by the output head)
  f16* raw_f16 = nullptr;      // optional: un-normalised fp16 copy of cat(x0,x1) (A operand of the 1x1 skip conv)
  f16* out_lo = nullptr;       // optional: fp16(y - float(fp16(y)))   -- low half of a split-fp16 operand
  f16* raw_lo = nullptr;       // optional: same for the raw copy
  // optional scale-shift rows of a use_scale_shift_norm ResBlock (openaimodel.py:267-271): row b = film + b * film_ld holds scale in its first
  // C floats and shift in the next C (th.chunk(emb_out, 2, dim=1)); y = SiLU((GN(x) gamma + beta) (1 + scale) + shift) then feeds out_f16 / out_lo /
  // out_f32 (the raw copies are unchanged).  film_ld = 0: one row shared by every sample (a timestep-table row).  16-byte aligned, film_ld % 4 == 0.
  const float* film = nullptr; int film_ld = 0;
  // fixed-point statistics accumulators of THIS GroupNorm call: [B][32 groups][GN_SLOTS][GN_STRIDE] int64 (GN_WORDS used), zero before
  // the launch.  Each of {sum, sumsq} is kept as an integer part and a 2^-40 fraction (two words), so the range is that
  // of an int64 and nothing can wrap.  Integer atomics are associative: the statistics are bit-reproducible without a
  // finalize pass or inter-block ordering; consumers fold the slots themselves (gn_fold in norm.hip).
  long long* acc = nullptr;
};
constexpr int GN_SLOTS = 8;
constexpr int GN_MAX_CALLS = 96;   // accumulator regions per UNet forward (SD v1 has 61 GroupNorms)
constexpr int GN_WORDS = 4;         // {sum int, sum frac * 2^40, sumsq int, sumsq frac * 2^40}
// words between two slot entries: every (sample, group, slot) entry owns a 128-byte line, so the atomic adds of one
// GroupNorm spread over 512+ lines / all memory channels instead of queueing on 128 (measured: the adds, not the
// arithmetic, were what the statistics cost)
constexpr int GN_STRIDE = 16;
static inline int64_t gn_acc_words(int B) { return (int64_t)B * 32 * GN_SLOTS * GN_STRIDE; }   // int64 words per GroupNorm call
int launch_groupnorm(const GroupNormParams& p, hipStream_t stream);

int launch_layernorm(const float* x, const float* gamma, const float* beta, f16* out, int M, int C, float eps,
                     hipStream_t stream, float* out_f32 = nullptr);     // out / out_f32: either or both
int launch_cast_f16(const float* x, f16* out, f16* out_lo, int64_t n, hipStream_t stream);

// fp32 "small" path
int launch_timestep_embedding(const int64_t* t_i64, const float* t_f32, float* out, int B, int dim, hipStream_t s);
int launch_small_linear(const float* in, int ld_in, const float* w, const float* bias, float* out, int ld_out,
                        int B, int N, int K, int silu_in, hipStream_t s);
// one-token context: ao[(b * ntok + tok) * C + c] = vt[(b * C + c) * ld_v] -- the cross-attention output of every query of sample b (small.hip)
int launch_ctx1_broadcast(const f16* vt, int ld_v, f16* ao, int B, int ntok, int C, hipStream_t s);
// the fp32 3x3 ends, each over its whole range: Cin <= 64 (above 16: a 36 KB patch, outputs split over blockIdx.y) resp. Cout <= 128 in
// slices of eight outputs (above 32 outputs: Cin <= 512).  The narrower limits that C entries were published with are checked in api.cpp.
// gn_*: GroupNorm statistics of the output for up to two consuming GroupNorms (accumulator regions, channels per group, channel offset of
// this tensor inside the GroupNorm's input: IGemmParams::gn_acc / gn_cpg / gn_cbase); needs Cin <= 16 and H * W % 16 == 0
int launch_conv_in(const float* x_nchw, const float* w, const float* bias, float* out_nhwc, int B, int Cin, int H,
                   int W, int Cout, hipStream_t s, int gn_n = 0, long long* const* gn_acc = nullptr, const int* gn_cpg = nullptr,
                   const int* gn_cbase = nullptr);
int launch_conv_out(const float* h_nhwc, const float* w_khwc, const float* bias, float* out_nchw, int B, int H, int W,
                    int Cin, int Cout, hipStream_t s);

// DPM-Solver++ multistep step (see sampler.hip)
struct DpmStepParams {
  const float* eps_model = nullptr;  // model output: rows [0,n) uncond, [n,2n) cond when cfg, else [0,n)
  int cfg = 0; float scale = 1.f;
  const float* x = nullptr;          // latent the model was evaluated at
  const float* m_prev = nullptr;     // previous data prediction (order 2)
  float alpha_s = 1.f, sigma_s = 0.f;      // marginal alpha / std at the evaluation time
  float cx = 1.f, a = 0.f, inv_r0 = 0.f;   // update coefficients
  int order = 1;
  float* m_out = nullptr;            // data prediction at this step (kept as history)
  float* x_next = nullptr;           // optional: the updated latent
  int64_t n = 0;
};
int launch_dpm_step(const DpmStepParams& p, hipStream_t s);

// the other DPM-Solver variants (see dpm.hip)
struct DpmModelValueParams {
  const float* eps_model = nullptr;  // as DpmStepParams
  int cfg = 0; float scale = 1.f;
  const float* x = nullptr;          // latent the model was evaluated at (predict_x0 only)
  int predict_x0 = 0;
  float alpha_s = 1.f, sigma_s = 0.f;
  const float* s = nullptr;          // optional per-sample thresholding scale [n / row], device memory
  int64_t row = 0;                   // elements per sample (with s)
  float* out = nullptr;
  int64_t n = 0;
};
int launch_dpm_model_value(const DpmModelValueParams& p, hipStream_t s);
struct DpmUpdateParams {
  int form = 0;                      // 0 LIN, 1 DIFF, 2 SS3T, 3 MS3 (dpm.hip)
  const float* x = nullptr;
  const float* m0 = nullptr; const float* m1 = nullptr; const float* m2 = nullptr;
  float c[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float* out = nullptr;
  int64_t n = 0;
};
int launch_dpm_update(const DpmUpdateParams& p, hipStream_t s);
int launch_dpm_threshold_scale(const float* x0, int B, int64_t row, float max_val, float* s_out, float* stats_out, hipStream_t s);
int64_t dpm_error_ws_floats(int B, int64_t row);
int launch_dpm_adaptive_error(const float* x_higher, const float* x_lower, const float* x_prev, float atol, float rtol, int B, int64_t row,
                              float* ws, int64_t ws_floats, float* E, hipStream_t s);

// text-encoder helpers: out[m][:] = tok_emb[ids[m]][:] + pos_emb[m % L][:] (fp32); out16 = fp16(x * sigmoid(1.702 x))
int launch_embed_tokens(const int64_t* ids, const float* tok_emb, const float* pos_emb, float* out, int M, int L, int C,
                        int vocab, hipStream_t s);
int launch_quick_gelu(const float* x, f16* out, int64_t n, hipStream_t s);
int launch_gelu_erf(const float* x, f16* out, int64_t n, hipStream_t s);
// ... the same activations as split-fp16 operand producers: out = fp16(y), the bits of the kernels above, out_lo = fp16(y_ref - out) with
// y_ref = y (quick_gelu) or the erfc form of the GELU (erf: out + out_lo is then the function itself, not gelu_erf's approximation of it)
int launch_quick_gelu_split(const float* x, f16* out, f16* out_lo, int64_t n, hipStream_t s);
int launch_gelu_erf_split(const float* x, f16* out, f16* out_lo, int64_t n, hipStream_t s);

// CLIP vision tower helpers (vit.hip)
int vit_kpad(int patch_size);           // columns of a patchify row: 3 p^2 rounded up to the 64-wide k-tile of the GEMM family
// pixel_values fp32 NCHW [B][3][S][S] -> fp16 [B (S / p)^2][vit_kpad(p)]: column (c, ky, kx) of patch (py, px); pad columns zero
int launch_vit_patchify(const float* px, f16* out, int B, int S, int p, hipStream_t s);
// out [B][T][C] fp32: row 0 = cls + pos[0], row 1 + i = patch[b (T - 1) + i] + pos[1 + i]
int launch_vit_embed(const float* patch, const float* cls, const float* pos, float* out, int B, int T, int C, hipStream_t s);
// [B][3][H][W] in [-1, 1] -> bicubic (align_corners, A = -0.75) [B][3][S][S], (x + 1) / 2, CLIP mean / std
int launch_vit_preprocess(const float* x, float* out, int B, int H, int W, int S, hipStream_t s);
// StableDiffusionSafetyChecker's head: cosines of image_embeds [B][E] with the special-care [Ns][E] and concept [Nc][E] vectors, the
// running adjustment, scores rounded to three decimals -> has_nsfw int32 [B], concept_scores [B][Nc], special_scores [B][Ns]
int launch_safety_head(const float* image_embeds, const float* concept_embeds, const float* special_care_embeds, const float* concept_thr,
                       const float* special_thr, int* has_nsfw, float* concept_scores, float* special_scores, int B, int Nc, int Ns, int E,
                       hipStream_t s);

// first-stage (VAE) helpers
// 1x1 conv, Cin <= 128 (up to 32: pointwise_nchw_kernel, the inputs in registers; beyond: pointwise_nchw_wide_kernel, Cout <= 1024)
int launch_pointwise_nchw(const float* x_nchw, const float* w, const float* bias, float* out_nchw, int B, int Cin, int Cout,
                          int HW, float in_scale, hipStream_t s);
int launch_softmax_rows(const float* S, f16* P, int rows, int cols, int lds, int ldp, float scale, hipStream_t s);

// latent-inpainting model (inpaint.hip)
// fp32 NHWC [B][H][W][C] -> dir 1: 2x2 average pool, dir -1: nearest x2; writes fp32 (o32) and / or fp16 hi (+ lo = fp16(v - hi))
int launch_resample2(const float* x, float* o32, f16* hi, f16* lo, int B, int H, int W, int C, int dir, hipStream_t s);
// codebook [n_embed][D] fp32 -> se[n] = sum_c e[n][c]^2
int launch_vq_norms(const float* e, float* se, int n_embed, int D, hipStream_t s);
// z fp32 NCHW [B][D][HW] (times z_scale) -> nearest code (first index on ties) idx [B * HW] and / or zq = z + (e[idx] - z), NCHW
int launch_vq_quantize(const float* z, float z_scale, const float* e, const float* se, int n_embed, int D, float* zq, int* idx, int B,
                       int HW, hipStream_t s);

// sliding windows of LatentDiffusion.split_input_params (patch.hip)
// rows (l, b), l in [l0, l0 + nl), of [nl * B][Cx + Cc][kh][kw] <- windows of x [B][Cx][H][W] and c [B][Cc][H][W] (c may be null with Cc = 0)
int launch_patch_unfold(const float* x, const float* c, float* out, int B, int Cx, int Cc, int H, int W, int kh, int kw, int sy, int sx,
                        int l0, int nl, hipStream_t s);
// out [B][C][H uf / df][W uf / df] = sum_l w[l] o[(l, b)] / sum_l w[l] over the covering windows (window and stride scaled by uf / df);
// norm_only: out [H uf / df][W uf / df] = sum_l w[l]
int launch_patch_fold(const float* o, const float* w, float* out, int B, int C, int H, int W, int kh, int kw, int sy, int sx, int uf, int df,
                      int norm_only, hipStream_t s);

// cache hint (small.hip): touch every 128-byte line of a device range
int launch_prefetch_lines(const void* ptr, int64_t bytes, hipStream_t s);

// weight packing (device pointers, fp32 reference layouts -> packed)
int launch_pack_conv_weight(const float* w_oihw, f16* dst, int O, int I, int KH, int KW, hipStream_t s);  // -> [O][KH][KW][I]
int launch_pack_rows(const float* w, f16* dst, int rows, int cols, int dst_row0, int dst_ld, hipStream_t s);
// column terms of a GEMM that folds LayerNorm(gamma, beta) of its input rows (IGemmParams::lnf_cs / lnf_d), from the PACKED fp16
// weights: cs[n] = sum_k gamma[k] w[n][k], d[n] = sum_k beta[k] w[n][k] (+ bias[n])
int launch_ln_fold_prep(const f16* w, int N, int K, int ldw, const float* gamma, const float* beta, const float* bias, float* cs,
                        float* d, hipStream_t s);
// split-fp16 weights for the 3-pass 1x1 convs: dst [N][3K] = [hi | hi | lo], lo = fp16(w - float(hi))
int launch_pack_split3(const float* w, f16* dst, int N, int K, hipStream_t s);
// ... for A sources that are multiples of 32 channels: K chunk-major PER SOURCE (c0 + c1 + c2 == I), the last chunk of a source of
// 32 (mod 64) channels 32 wide.  One kernel serves the three conv packers: launch_pack_conv_weight is the one-source case (c0 = I), and
// with every source a multiple of 64 the split does not change the bytes.  launch_pack_conv_split3: three sources of the same I channels,
// [hi | hi | lo].
int launch_pack_conv_weight_src(const float* w_oihw, f16* dst, int O, int I, int KH, int KW, int c0, int c1, int c2, hipStream_t s);
int launch_pack_conv_split3(const float* w, f16* dst, int O, int I, int KH, int KW, hipStream_t s);
// packed 3x3 weights [N][9 Cin] -> the weights [4][N][4 Cin] of the four 2x2 phase convs of conv3x3(nearest x2 (x)) (small.hip; Cin % 64 == 0)
int launch_up_phase_weights(const f16* wp, f16* dst, int N, int Cin, hipStream_t s);
int launch_pack_geglu(const float* w, const float* bias, f16* wdst, float* bdst, int N, int K, hipStream_t s);
int launch_pack_conv_out(const float* w_oihw, float* dst, int O, int I, hipStream_t s);   // -> [O][3][3][I] fp32

// sampler update (fp32): see sampler.hip
struct SamplerStepParams {
  const float* eps_model = nullptr;  // model output: rows [0,n) uncond, [n,2n) cond when cfg, else [0,n)
  int cfg = 0; float scale = 1.f;    // e_t = e_u + scale * (e_c - e_u)                      plms.py:182-186
  const float* x = nullptr;          // [B,4,H,W] current latent
  // multistep combination (plms.py:218-232), evaluated in the reference's fp32 operation order:
  //   0: e' = e_t                      (DDIM, ddim.py:189-204)
  //   1: e' = (3 e_t - o0) / 2         2: e' = (23 e_t - 16 o0 + 5 o1) / 12
  //   3: e' = (55 e_t - 59 o0 + 37 o1 - 9 o2) / 24
  //   4: e' = (o0 + e_t) / 2           (first PLMS step: o0 = e_t, e_t = e_t_next)
  int mode = 0;
  const float* old0 = nullptr; const float* old1 = nullptr; const float* old2 = nullptr;  // newest first
  float a_t = 1.f, a_prev = 1.f, sigma = 0.f, sqrt_1m_at = 0.f;                           // table entries
  const float* noise = nullptr;      // optional [B,4,H,W] (sigma > 0), already scaled by temperature
  float* e_t_out = nullptr;          // optional: combined (post-CFG) eps, kept for the history
  float* x_prev = nullptr; float* pred_x0 = nullptr;   // pred_x0 optional
  int64_t n = 0;                     // elements per output (B*4*H*W)
  // the step split at pred_x0 (quantize_x0): x_prev null -> stop after pred_x0, with the combined e' in ep_out for the second half
  float* ep_out = nullptr;
};
int launch_sampler_step(const SamplerStepParams& p, hipStream_t s);
// ... its second half: x_prev from a given pred_x0 and e' (a_prev, sigma: the table entries; noise optional as above)
int launch_sampler_step_from_x0(const float* pred_x0, const float* ep, float a_prev, float sigma, const float* noise, float* x_prev,
                                int64_t n, hipStream_t s);
// ancestral DDPM step (fp32): see sampler.hip
struct DdpmStepParams {
  const float* eps = nullptr;        // model output; null: x0 comes from x0_in (the second half, after the codebook quantizer)
  const float* x0_in = nullptr;
  const float* x = nullptr;          // current latent
  float c_recip = 1.f, c_recipm1 = 0.f;     // sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t]
  int clip = 0;                      // clip_denoised
  float coef1 = 0.f, coef2 = 1.f;    // posterior_mean_coef1[t], posterior_mean_coef2[t]
  float s = 0.f;                     // (t != 0) * exp(0.5 * posterior_log_variance_clipped[t])
  const float* noise = nullptr;      // already scaled by temperature
  const float* mask = nullptr;       // optional blend: all of mask (expanded to the latent's shape), x0_orig, q_noise
  const float* x0_orig = nullptr; const float* q_noise = nullptr;
  float sa = 1.f, s1ma = 0.f;        // sqrt_alphas_cumprod[t], sqrt_one_minus_alphas_cumprod[t]
  float* x0_out = nullptr;           // optional (return_x0)
  float* x_prev = nullptr;           // may be x; null: stop after x0_out (the first half)
  int64_t n = 0;
};
int launch_ddpm_step(const DdpmStepParams& p, hipStream_t s);
// decode output fp32 NCHW -> uint8 NHWC exactly as scripts/txt2img.py:313-324 does on the host (sampler.hip)
int launch_image_u8(const float* img_nchw, unsigned char* out_nhwc, int B, int C, int H, int W, hipStream_t s);

}  // namespace sdmi
