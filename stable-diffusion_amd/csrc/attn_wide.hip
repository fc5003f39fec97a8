// Fused softmax(Q K^T * scale) V for WIDE heads: 160 < d <= 1024, d % 64 == 0 (the class-conditional ImageNet UNet runs single-headed
// SpatialTransformers with d = C = 384 / 576 / 960; reference: CrossAttention.forward, ldm/modules/attention.py:170-193 with heads = 1).
// Same contract as attn.hip (AttnParams; launch_attention dispatches here by d): fp16 operands, fp32 scores / softmax / accumulation,
// one launch, S never leaves the registers.
//
// attn.hip keeps Q, a 32 x d fp32 accumulator and whole [64 keys][d] K / V^T tiles per wave / ring stage; none of that grows to d = 960
// (the accumulator alone would be 480 registers).  Here:
//   * a workgroup owns 32 * NW queries (one wave = 32 queries, as in attn.hip) AND a 64-row slice of the output's d: grid =
//     query tiles x d / 64 x BH.  The fp32 accumulator of a wave is 32 x 64 (32 registers) at every d, and the levels with few tokens
//     (64 tokens at d = 960: 2 x BH query slices) still spread over d / 64 times as many workgroups.  These shapes are latency bound with
//     few workgroups; the full-d Q K^T that every slice recomputes is the price (2 d / 16 MFMAs per 64 keys against 8 for P V);
//   * Q stays in registers for the whole kernel (d / 16 fragments = d / 4 registers: 240 at d = 960; at most four waves per workgroup,
//     so a wave may take the SIMD's whole 512-entry file);
//   * K streams through LDS in chunks of [64 keys][64 halves of d] (8 KB), followed per key tile by the slice's V^T chunk
//     [64 d rows][64 keys] (8 KB): ONE ring of NS chunk stages fed by LDS-DMA, NS - 1 chunks in flight, one barrier per chunk.  A
//     stage has the layout of attn.hip's LDS-DMA kernel (rows of 128 B, 16-byte chunks XOR-swizzled with (row >> 1) & 7 on the DMA
//     source side, the keys of a K chunk permuted so that the eight keys a lane owns in a P^T fragment are contiguous in the V^T row);
//   * the swapped products S^T = K Q^T and O^T = V^T P^T, the in-lane online softmax and the P^T fragments taken straight from the
//     accumulator registers are attn.hip's.  Every d-slice computes the same scores in the same order, hence the same P.
//   * keys past nkv: their scores are masked (P = 0 exactly) and, in that last tile, their V^T columns are replaced by zeros after
//     the LDS read, so whatever the pad columns nkv .. nkv_pad (or, past nkv_pad, the neighbouring row) hold never reaches an MFMA.
#include "common.h"
#include "prof.h"

namespace sdmi {
namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int KVT = 64;          // keys per tile
constexpr int WNS = 8;           // ring stages
constexpr int CHB = 8192;        // bytes of a stage: 64 rows x 128 B

template <int N>
__device__ __forceinline__ void wide_wait_dma() {     // counted s_waitcnt vmcnt(N): the immediate must be a literal
  static_assert(N == 0 || N == 12 || N == 24, "add the literal");
  if (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
}
// max / sum over the two 32-lane halves of the wave, in every lane (see attn.hip: v_permlane32_swap, not ds_bpermute)
__device__ __forceinline__ void wide_swap_halves(float& a, float& b) {      // a.hi <-> b.lo
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float wide_max_halves(float x) {
  float a = x, b = x;
  wide_swap_halves(a, b);
  return fmaxf(a, b);
}
__device__ __forceinline__ float wide_sum_halves(float x) {
  float a = x, b = x;
  wide_swap_halves(a, b);
  return a + b;
}

template <int D, int NW>
__global__ void __launch_bounds__(NW * 64) attn_wide_kernel(const AttnParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert(D % 64 == 0 && D > 160 && D <= 1024, "wide heads: 192 .. 1024 in steps of 64");
  static_assert(NW == 2 || NW == 4, "a wave needs more than 256 registers at the upper end: at most one wave per SIMD");
  constexpr int DKS = D / 16;          // k-steps of 16 over the head dim (QK^T)
  constexpr int NCH = D / 64;          // K chunks per key tile
  constexpr int CPT = NCH + 1;         // ring chunks per key tile: K chunks, then the slice's V^T chunk
  constexpr int PPW = 8 / NW;          // DMA pieces (8 rows x 128 B) per wave and chunk
  constexpr int INFL = PPW * (WNS - 2);

  __shared__ __attribute__((aligned(16))) unsigned char smem[WNS * CHB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lg = lane >> 5;
  const int bh = blockIdx.z, d0 = blockIdx.y * 64;
  const int q0 = blockIdx.x * (32 * NW) + wave * 32;
  const f16* Qg = p.q + (size_t)bh * p.nq * D;
  const __amdgpu_buffer_rsrc_t rsrc_k =
      __builtin_amdgcn_make_buffer_rsrc((void*)(p.k + (size_t)bh * p.nkv * D), 0, p.nkv * D * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsrc_v =
      __builtin_amdgcn_make_buffer_rsrc((void*)(p.vt + (size_t)bh * D * p.nkv_pad), 0, D * p.nkv_pad * 2, 0x00020000);

  // Q^T fragments (MFMA B operand): lane (q = l31, g = lg) holds Q[q][16*ks + 8*g .. +8]; zero beyond nq
  f16x8 qf[DKS];
#pragma unroll
  for (int ks = 0; ks < DKS; ++ks) {
    f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (q0 + l31 < p.nq) v = *(const f16x8*)(Qg + (size_t)(q0 + l31) * D + ks * 16 + lg * 8);
    qf[ks] = v;
  }

  // this wave's DMA pieces of a chunk: piece = wave + j * NW covers LDS rows piece * 8 .. + 8 (lane: row + lane / 8, 16-byte column lane % 8).
  // Per-lane byte offsets at key tile 0 (K: chunk 0); everything that moves goes into the per-lane offset as well, because the
  // buffer range check (rows / columns past the tensor read as zeros) does not see the scalar offset.
  unsigned koff[PPW], voff[PPW];
#pragma unroll
  for (int j = 0; j < PPW; ++j) {
    const int row = (wave + j * NW) * 8 + (lane >> 3), cp = lane & 7;
    const int gch = cp ^ ((row >> 1) & 7);
    const int key = (row & ~12) | ((row & 4) << 1) | ((row & 8) >> 1);      // LDS row `row` holds key perm(row) of the tile
    koff[j] = (unsigned)(key * (D * 2) + gch * 16);
    voff[j] = (unsigned)((d0 + row) * (p.nkv_pad * 2) + gch * 16);
  }
  // ic = chunk of the key tile this issue fetches: the stream runs WNS - 1 chunks ahead of the loop, which consumes CPT per
  // iteration, so ic is a constant at every call site.  Advances the stream: call once per chunk, in order.
  auto issue = [&](int stage, int ic) {
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      auto dst = (__attribute__((address_space(3))) void*)(smem + stage * CHB + (wave + j * NW) * 1024);
      if (ic < NCH) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_k, dst, 16, koff[j] + ic * 128, 0, 0, 0);
      } else {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_v, dst, 16, voff[j], 0, 0, 0);
        koff[j] += KVT * D * 2;                 // (chunks past the last tile: K offsets only grow -> out of range -> zeros; V^T reads stay
        voff[j] += KVT * 2;                     //  inside this (b, head)'s tensor or past its end; none of them is consumed)
      }
    }
  };

  f32x16 o[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  const float sc = p.scale * 1.4426950408889634f;   // scores are compared / exponentiated in log2 units

  const int nt = (p.nkv + KVT - 1) / KVT;
#pragma unroll
  for (int s2 = 0; s2 < WNS - 1; ++s2) issue(s2, s2 % CPT);
  wide_wait_dma<INFL>();
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  const int ksw = (l31 >> 1) & 7;
  int cur = 0, nxt = WNS - 1;
  auto advance = [&]() {
    wide_wait_dma<INFL>();                                             // this wave's pieces of the next chunk have landed
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");    // ... everybody's; and the current chunk is fully read
    cur = (cur + 1 == WNS) ? 0 : cur + 1;
    nxt = (nxt + 1 == WNS) ? 0 : nxt + 1;
  };
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  for (int t = 0; t < nt; ++t) {
    // ---- S^T = K Q^T (two 32-key blocks), one 64-half chunk of d per ring stage ----
    f32x16 s[KVT / 32];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      // the fragment reads first, the DMA issue of the chunk NS - 1 ahead under their latency (an LDS-DMA piece costs the wave ~100
      // issue cycles; the compiler keeps LDS reads behind an LDS-DMA write it cannot tell apart from them)
      const unsigned char* Kq = smem + cur * CHB;
      f16x8 a[KVT / 32][4];
#pragma unroll
      for (int kvb = 0; kvb < KVT / 32; ++kvb)
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) a[kvb][k4] = *(const f16x8*)(Kq + (kvb * 32 + l31) * 128 + (((k4 * 2 + lg) ^ ksw) << 4));
      issue(nxt, (WNS - 1 + c) % CPT);
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4)
#pragma unroll
        for (int kvb = 0; kvb < KVT / 32; ++kvb)
          s[kvb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kvb][k4], qf[c * 4 + k4], (c == 0 && k4 == 0) ? zero16 : s[kvb], 0, 0, 0);
      advance();
    }
    // ---- mask keys beyond nkv (last tile only: a real, wave-uniform branch) ----
    const int kv0 = t * KVT;
    const bool tail = kv0 + KVT > p.nkv;
    if (tail) {
      asm volatile("; masked tile" ::: "memory");
#pragma unroll
      for (int kvb = 0; kvb < KVT / 32; ++kvb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + kvb * 32 + (r & 3) + 4 * ((r >> 2) & 1) + 8 * lg + 16 * (r >> 3);   // (permuted rows)
          if (kv >= p.nkv) s[kvb][r] = -1e30f;
        }
    }
    // ---- online softmax (per query = per lane column; halves lg = 0/1 hold disjoint keys) ----
    float mx = -1e30f;
#pragma unroll
    for (int kvb = 0; kvb < KVT / 32; ++kvb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kvb][r]);
    mx = wide_max_halves(mx);
    const float m_new = fmaxf(m_run, mx * sc);
    if (__any(m_new > m_run)) {              // (else the factor is exactly 1 for every lane: skipping is bit-identical)
      asm volatile("; rescale" ::: "memory");
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
    }
    f32x2 psum2 = {0.f, 0.f};
    const f32x2 sc2 = {sc, sc}, nm2 = {-m_run, -m_run};
#pragma unroll
    for (int kvb = 0; kvb < KVT / 32; ++kvb)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const f32x2 sv = {s[kvb][r], s[kvb][r + 1]};
        const f32x2 e = __builtin_elementwise_fma(sv, sc2, nm2);
        const f32x2 pv = {__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1])};
        s[kvb][r] = pv[0];
        s[kvb][r + 1] = pv[1];
        psum2 += pv;
      }
    l_run += psum2[0] + psum2[1];

    // ---- O^T += V^T P^T for this workgroup's 64 rows of d ----
    const unsigned char* Vs = smem + cur * CHB;
    f16x8 vf[KVT / 32][2][2];
#pragma unroll
    for (int kvb = 0; kvb < KVT / 32; ++kvb)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int ch = 4 * kvb + 2 * s2 + lg;       // the 16-byte chunk with this lane's eight keys: kv0 + 8 * ch .. + 8
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          f16x8 a = *(const f16x8*)(Vs + (dt * 32 + l31) * 128 + ((ch ^ ksw) << 4));
          if (tail) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (kv0 + 8 * ch + e >= p.nkv) a[e] = (f16)0.f;
          }
          vf[kvb][s2][dt] = a;
        }
      }
    issue(nxt, (WNS - 1 + NCH) % CPT);
#pragma unroll
    for (int kvb = 0; kvb < KVT / 32; ++kvb) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        f16x8 pf;
#pragma unroll
        for (int e = 0; e < 8; ++e) pf[e] = (f16)s[kvb][8 * s2 + e];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[kvb][s2][dt], pf, o[dt], 0, 0, 0);
      }
    }
    advance();
  }
  wide_wait_dma<0>();            // the chunks issued past the last tile must have landed before the LDS is given back

  // ---- normalise and store: O[b][q][head*D + d0 + dd] ----
  const float inv = 1.0f / wide_sum_halves(l_run);
  const int q = q0 + l31;
  if (q < p.nq) {
    const int b = bh / p.heads, head = bh - b * p.heads;
    f16* orow = p.out + ((size_t)b * p.nq + q) * ((size_t)p.heads * D) + (size_t)head * D + d0;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int dd = dt * 32 + 8 * r4 + 4 * lg;
        f16x4 v = {(f16)(o[dt][r4 * 4 + 0] * inv), (f16)(o[dt][r4 * 4 + 1] * inv), (f16)(o[dt][r4 * 4 + 2] * inv),
                   (f16)(o[dt][r4 * 4 + 3] * inv)};
        SDMI_ST(f16x4, orow + dd, v);
      }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

template <int D>
int launch_wide_d(const AttnParams& p, hipStream_t stream) {
  // one wave = 32 queries.  Four waves share a K chunk where that still leaves more workgroups than half the chip has CUs; below,
  // two waves per workgroup: twice the workgroups, and every wave re-reads each K fragment from LDS (one ds_read_b128 per MFMA), so
  // two waves also halve what the CU's LDS has to deliver per MFMA interval.  (Eight waves, two per SIMD, at d = 384: 51.9 us against
  // 37.3 us at BH = 2, 62.7 against 64.9 at BH = 8 -- profiles/attn_wide.txt; not instantiated.)
  int nw = p.nw;
  if (nw != 2 && nw != 4) nw = (p.nq > 64 && (int64_t)cdiv(p.nq, 128) * (D / 64) * p.BH > 128) ? 4 : 2;
  dim3 grid(cdiv(p.nq, 32 * nw), D / 64, p.BH);
  static const std::string pname_long = std::string("attn_d") + std::to_string(D) + "_self";
  static const std::string pname_short = std::string("attn_d") + std::to_string(D) + "_ctx";
  ProfScope ps((p.nkv >= 256 ? pname_long : pname_short).c_str(), 4.0 * p.BH * (double)p.nq * p.nkv * D,
               2.0 * p.BH * D * (2.0 * p.nq + 2.0 * p.nkv), stream, (2.0 * (D / 64) + 2.0) * p.BH * (double)p.nq * p.nkv * D);
  if (nw == 4) SDMI_LAUNCH((attn_wide_kernel<D, 4>), grid, dim3(256), 0, stream, p);
  else SDMI_LAUNCH((attn_wide_kernel<D, 2>), grid, dim3(128), 0, stream, p);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace

int launch_attention_wide(const AttnParams& p, hipStream_t stream) {
  SDMI_CHECK(!p.causal, "wide-head attention has no causal mask");
  SDMI_CHECK(p.BH <= 65535, "wide-head attention: at most 65535 (batch x head) rows per launch");
  // 32-bit buffer offsets: the ring runs up to WNS chunks past the last key tile
  SDMI_CHECK(((int64_t)p.nkv + KVT * (WNS + 1)) * p.d * 2 < (int64_t)1 << 31 && ((int64_t)p.d * p.nkv_pad + KVT * (WNS + 1)) * 2 < (int64_t)1 << 31,
             "wide-head attention: K / V^T of one (batch, head) row must stay below 2 GB");
  switch (p.d) {
#define SDMI_WIDE(dd) case dd: return launch_wide_d<dd>(p, stream)
    SDMI_WIDE(192); SDMI_WIDE(256); SDMI_WIDE(320); SDMI_WIDE(384); SDMI_WIDE(448); SDMI_WIDE(512); SDMI_WIDE(576);
    SDMI_WIDE(640); SDMI_WIDE(704); SDMI_WIDE(768); SDMI_WIDE(832); SDMI_WIDE(896); SDMI_WIDE(960); SDMI_WIDE(1024);
#undef SDMI_WIDE
    default: return fail("attention head dim " + std::to_string(p.d) + " not instantiated (32/40/64/80/96/128/160, and 192 .. 1024 in steps of 64)");
  }
}

}  // namespace sdmi
