// Split-fp16 flash attention for WIDE heads: 160 < d <= 1024, d % 64 == 0 (the first stage's single-headed mid-block attention runs at
// d = ch * ch_mult[-1] = 512; reference: AttnBlock.forward, ldm/modules/diffusionmodules/model.py:172-202).  Same contract and the
// same arithmetic as attn_split16.hip (AttnSplitParams; launch_attention_split16 dispatches here by d):
//
//   S = q_hi k_hi^T + q_lo k_hi^T + q_hi k_lo^T          (v_mfma_f32_32x32x16_f16, fp32 accumulation)
//   P = exp((S - running max) * scale) in fp32 (see below), split into P_hi = fp16(P), P_lo = fp16(P - P_hi)
//   O += P_hi V_hi + P_lo V_hi + P_hi V_lo               (fp32), normalised by the fp32 row sum of P and stored as hi / lo
//
// attn_wide.hip keeps a wave's whole Q in registers (d / 4 of them); with hi and lo that is d / 2 = 512 at d = 1024, the whole
// file.  Here the four waves of a workgroup share 32 queries and split d instead:
//   * wave w holds Q hi / lo for its quarter of d (k-steps w * d / 64 .. + d / 64: d / 8 registers, 128 at d = 1024) and computes the
//     partial S^T of a 64-key tile over that quarter with the three products;
//   * the four partials go through LDS (8 KB each, two generations so that one barrier per key tile is enough) and every wave sums
//     them in the same order ((w0 + w1) + w2) + w3: all four hold the same scores bit for bit and run the same fp32 online softmax;
//   * wave w accumulates O^T for the 32-row tiles w, w + 4, w + 8 .. of the output's d (at most d / 8 accumulator registers;
//     where d / 32 is no multiple of 4, waves 0 and 1 own one tile more than waves 2 and 3);
//   * no K or V^T element is used by two waves of a workgroup, so the fragments are loaded from global memory (L2 serves the re-reads
//     of the other workgroups) straight into the MFMA operand layout, 16 bytes per K fragment and 2 x 8 bytes per V^T fragment.
// The fragment, key-order and P^T-from-accumulator mapping is attn_split16_kernel's.  Keys past nkv: their K rows are not loaded, their
// scores are masked (P = 0 exactly) and, in that last tile, their V^T elements (hi and lo) are replaced by zeros after the load, so
// the pad columns nkv .. nkv_pad may hold anything; nothing is read past nkv_pad.  Queries past nq are neither loaded nor stored.
// Every loop is bounded by the tile count, the summation order is fixed and there are no atomics: results repeat bit for bit.
// Like attn_split16.hip, no speed target is attached to this mode.
#include "prof.h"
#include "split16.h"

namespace sdmi {
namespace {

constexpr int WKVT = 64;         // keys per tile
constexpr int WNW = 4;           // waves per workgroup = parts of d

__device__ __forceinline__ f16 wlo_of(float v, f16 hi) { return (f16)(v - (float)hi); }   // the low half of a split-fp16 pair

template <int D>
__global__ void __launch_bounds__(WNW * 64) attn_wide_split16_kernel(const AttnSplitParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert(D % 64 == 0 && D > 160 && D <= 1024, "wide heads: 192 .. 1024 in steps of 64");
  constexpr int KSW = D / 64;                     // k-steps of 16 over this wave's quarter of d (Q K^T)
  constexpr int NDT = D / 32;                     // 32-row tiles of the output's d (P V)
  constexpr int DVT = (NDT + WNW - 1) / WNW;      // ... of which a wave owns at most this many
  constexpr int PART = 8 * 64 * 16;               // bytes of one wave's partial S^T: 2 x 16 fp32 per lane, [register quad][lane]

  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * WNW * PART];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lg = lane >> 5;
  const int bh = blockIdx.y;
  const int q0 = blockIdx.x * 32;
  const size_t qoff = (size_t)bh * p.nq * D, koff = (size_t)bh * p.nkv * D, voff = (size_t)bh * D * p.nkv_pad;
  const f16* const Kh = p.k + koff; const f16* const Kl = p.k_lo + koff;
  const f16* const Vh = p.vt + voff; const f16* const Vl = p.vt_lo + voff;
  const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const f16x4 zero4 = {0, 0, 0, 0};

  // Q^T fragments (MFMA B operand) of this wave's k-steps: lane (q = l31, g = lg) holds Q[q][16 * ks + 8 * g .. + 8]
  f16x8 qh[KSW], ql[KSW];
#pragma unroll
  for (int j = 0; j < KSW; ++j) {
    const int dcol = (wave * KSW + j) * 16 + lg * 8;
    f16x8 h = zero8, l = zero8;
    if (q0 + l31 < p.nq) {
      h = *(const f16x8*)(p.q + qoff + (size_t)(q0 + l31) * D + dcol);
      l = *(const f16x8*)(p.q_lo + qoff + (size_t)(q0 + l31) * D + dcol);
    }
    qh[j] = h; ql[j] = l;
  }

  f32x16 o[DVT];
#pragma unroll
  for (int j = 0; j < DVT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[j][r] = 0.f;
  // The running max is kept in score units and the exponent is formed as (s - m) * scale: the difference is exact (or as good as its
  // own size) before the scale rounds it, so a row's largest score gets P = exp2(0) = 1 exactly -- with one key the output is V's
  // hi + lo bit for bit -- and every key of any weight sees an exponent error proportional to its distance from the maximum.
  // (attn_split16.hip forms fma(s, scale, -m) against a max in scaled units, whose rounding is common to a row and cancels in the
  // normalisation, but leaves P of the maximum one ulp off 1.)
  float m_run = -1e30f, l_run = 0.f;
  const float sc = p.scale * 1.4426950408889634f;   // scores are exponentiated in log2 units

  const int nt = (p.nkv + WKVT - 1) / WKVT;
  for (int t = 0; t < nt; ++t) {
    const int kv0 = t * WKVT;
    const bool tail = kv0 + WKVT > p.nkv;
    // ---- partial S^T = K Q^T over this wave's quarter of d, two 32-key blocks, three products per fragment pair ----
    f32x16 s[WKVT / 32];
#pragma unroll
    for (int kvb = 0; kvb < WKVT / 32; ++kvb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kvb][r] = 0.f;
      const int key = kv0 + kvb * 32 + l31;
      const bool kin = key < p.nkv;
      const size_t kofs = (size_t)(kin ? key : 0) * D + (size_t)(wave * KSW * 16 + lg * 8);
#pragma unroll
      for (int j = 0; j < KSW; ++j) {
        f16x8 kh = zero8, kl = zero8;
        if (kin) {
          kh = *(const f16x8*)(Kh + kofs + j * 16);
          kl = *(const f16x8*)(Kl + kofs + j * 16);
        }
        s[kvb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[j], s[kvb], 0, 0, 0);
        s[kvb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[j], s[kvb], 0, 0, 0);
        s[kvb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[j], s[kvb], 0, 0, 0);
      }
    }
    // ---- sum the four partials in a fixed order: generation t & 1 of the exchange buffer (a wave that is still reading generation
    //      t - 1 is not disturbed; generation t - 2 was read by everybody before the barrier of tile t - 1) ----
    {
      unsigned char* const gen = smem + (t & 1) * (WNW * PART);
#pragma unroll
      for (int kvb = 0; kvb < WKVT / 32; ++kvb)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
          *(f32x4*)(gen + wave * PART + ((kvb * 4 + r4) * 64 + lane) * 16) =
              f32x4{s[kvb][r4 * 4], s[kvb][r4 * 4 + 1], s[kvb][r4 * 4 + 2], s[kvb][r4 * 4 + 3]};
      __syncthreads();
#pragma unroll
      for (int kvb = 0; kvb < WKVT / 32; ++kvb)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const unsigned char* src = gen + ((kvb * 4 + r4) * 64 + lane) * 16;
          const f32x4 p0 = *(const f32x4*)(src), p1 = *(const f32x4*)(src + PART);
          const f32x4 p2 = *(const f32x4*)(src + 2 * PART), p3 = *(const f32x4*)(src + 3 * PART);
          const f32x4 sum = ((p0 + p1) + p2) + p3;
#pragma unroll
          for (int e = 0; e < 4; ++e) s[kvb][r4 * 4 + e] = sum[e];
        }
    }
    // ---- mask keys beyond nkv (accumulator register r of lane half lg holds key (r & 3) + 8 (r >> 2) + 4 lg of its block) ----
    if (tail) {
#pragma unroll
      for (int kvb = 0; kvb < WKVT / 32; ++kvb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + kvb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lg;
          if (kv >= p.nkv) s[kvb][r] = -1e30f;
        }
    }
    // ---- online softmax in fp32 (per query = per lane column; the halves lg = 0 / 1 hold disjoint keys) ----
    float mx = -1e30f;
#pragma unroll
    for (int kvb = 0; kvb < WKVT / 32; ++kvb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kvb][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sc);
    m_run = m_new;
    l_run *= alpha;
#pragma unroll
    for (int j = 0; j < DVT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[j][r] *= alpha;
    float psum = 0.f;
#pragma unroll
    for (int kvb = 0; kvb < WKVT / 32; ++kvb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f((s[kvb][r] - m_run) * sc);
        s[kvb][r] = pv;
        psum += pv;
      }
    l_run += psum;

    // ---- O^T += V^T P^T for this wave's tiles of d, three products per fragment pair ----
#pragma unroll
    for (int kvb = 0; kvb < WKVT / 32; ++kvb) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        f16x8 ph, pl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          ph[e] = (f16)s[kvb][8 * s2 + e];
          pl[e] = wlo_of(s[kvb][8 * s2 + e], ph[e]);
        }
        // this lane's eight keys of the k-step: c0 .. c0 + 3 and c0 + 8 .. c0 + 11 (V^T columns; nkv_pad % 8 == 0, so a group of
        // four that starts below nkv_pad ends inside the row)
        const int c0 = kv0 + kvb * 32 + 16 * s2 + 4 * lg;
        const bool in0 = c0 < p.nkv_pad, in1 = c0 + 8 < p.nkv_pad;
#pragma unroll
        for (int j = 0; j < DVT; ++j) {
          const int dt = wave + j * WNW;
          if (dt < NDT) {                                  // (wave-uniform)
            const size_t vofs = (size_t)(dt * 32 + l31) * p.nkv_pad + c0;
            f16x4 h0 = zero4, h1 = zero4, l0 = zero4, l1 = zero4;
            if (in0) { h0 = *(const f16x4*)(Vh + vofs); l0 = *(const f16x4*)(Vl + vofs); }
            if (in1) { h1 = *(const f16x4*)(Vh + vofs + 8); l1 = *(const f16x4*)(Vl + vofs + 8); }
            if (tail) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                if (c0 + e >= p.nkv) { h0[e] = (f16)0.f; l0[e] = (f16)0.f; }
                if (c0 + 8 + e >= p.nkv) { h1[e] = (f16)0.f; l1[e] = (f16)0.f; }
              }
            }
            const f16x8 ah = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
            const f16x8 al = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
            o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, ph, o[j], 0, 0, 0);
            o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, pl, o[j], 0, 0, 0);
            o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ph, o[j], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- normalise and store hi / lo: O[b][q][head * D + dd] ----
  const float l_tot = l_run + __shfl_xor(l_run, 32);
  const int q = q0 + l31;
  if (q < p.nq) {
    const int b = bh / p.heads, head = bh - b * p.heads;
    const size_t row = ((size_t)b * p.nq + q) * ((size_t)p.heads * D) + (size_t)head * D;
#pragma unroll
    for (int j = 0; j < DVT; ++j) {
      const int dt = wave + j * WNW;
      if (dt < NDT) {
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int dd = dt * 32 + 8 * r4 + 4 * lg;
          f16x4 h, l;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float v = o[j][r4 * 4 + e] / l_tot;
            h[e] = (f16)v;
            l[e] = wlo_of(v, h[e]);
          }
          *(f16x4*)(p.out + row + dd) = h;
          *(f16x4*)(p.out_lo + row + dd) = l;
        }
      }
    }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

template <int D>
int launch_wide_split_d(const AttnSplitParams& p, hipStream_t stream) {
  dim3 grid((unsigned)((p.nq + 31) / 32), (unsigned)p.BH);
  SDMI_LAUNCH(attn_wide_split16_kernel<D>, grid, dim3(WNW * 64), 0, stream, p);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace

// called by launch_attention_split16 (attn_split16.hip), which has checked the operands and the shape
int launch_attention_wide_split16(const AttnSplitParams& p, hipStream_t stream) {
  switch (p.d) {
#define SDMI_WIDE_SPLIT(dd) case dd: return launch_wide_split_d<dd>(p, stream)
    SDMI_WIDE_SPLIT(192); SDMI_WIDE_SPLIT(256); SDMI_WIDE_SPLIT(320); SDMI_WIDE_SPLIT(384); SDMI_WIDE_SPLIT(448);
    SDMI_WIDE_SPLIT(512); SDMI_WIDE_SPLIT(576); SDMI_WIDE_SPLIT(640); SDMI_WIDE_SPLIT(704); SDMI_WIDE_SPLIT(768);
    SDMI_WIDE_SPLIT(832); SDMI_WIDE_SPLIT(896); SDMI_WIDE_SPLIT(960); SDMI_WIDE_SPLIT(1024);
#undef SDMI_WIDE_SPLIT
    default: return fail("split-fp16 wide-head attention: head dim " + std::to_string(p.d) + " has no instantiation (192 .. 1024 in steps of 64)");
  }
}

}  // namespace sdmi
