// Split-fp16 flash attention for the full-precision UNet mode (reference: CrossAttention.forward, ldm/modules/attention.py:170-193).
//
//   S = q_hi k_hi^T + q_lo k_hi^T + q_hi k_lo^T          (v_mfma_f32_32x32x16_f16, fp32 accumulation)
//   P = exp(S * scale - running max)  in fp32, split into P_hi = fp16(P), P_lo = fp16(P - P_hi)
//   O += P_hi V_hi + P_lo V_hi + P_hi V_lo               (fp32), normalised by the fp32 row sum of P and stored as hi / lo
//
// The operand layouts and fragment mapping are those of attn_kernel (attn.hip): one wave owns 32 queries, the swapped product
// S^T = K Q^T gives every lane one query column, and P^T is fed to the PV MFMA straight from the accumulator registers in the
// permuted key order that V^T fragments are read in.  Differences: every tile and fragment exists twice (hi, lo); the K / V^T tiles
// of 64 keys are staged in ONE LDS stage (d = 160: 2 x 43 KB), loaded and stored synchronously between two barriers -- several
// workgroups per CU (d <= 80) or the four waves of one (d = 160) hide the load latency; no speed target is attached to this mode.
#include "prof.h"
#include "split16.h"

namespace sdmi {
namespace {

constexpr int KVT = 64;

__device__ __forceinline__ f16 lo_of(float v, f16 hi) { return (f16)(v - (float)hi); }   // the low half of a split-fp16 pair

// CAUSAL (the text encoder of the full-precision mode, clip.cpp): nq == nkv, query i sees keys <= i.  The mask is applied to the scores
// beside the key-range mask; every wave, with queries or without, walks every key tile of the workgroup and takes part in both barriers
// (no tile is skipped: at the text lengths one workgroup holds all queries).  Key 0 is visible to every query, so the running maximum is
// finite from the first tile on and a masked score of -1e30 exponentiates to exactly 0.
template <int D, int NW, bool CAUSAL>
__global__ void __launch_bounds__(NW * 64) attn_split16_kernel(const AttnSplitParams p) {
  constexpr int DKS = (D + 15) / 16;   // k-steps of 16 over the head dim (QK^T)
  constexpr int DVT = (D + 31) / 32;   // 32-row tiles over the head dim (PV)
  constexpr int NT = NW * 64;
  constexpr int KSTRIDE = DKS * 32 + 16;          // bytes; odd multiple of 16 -> conflict-free ds_read_b128
  constexpr int VSTRIDE = KVT * 2 + 8;            // bytes; 34 dwords -> conflict-free ds_read_b64
  constexpr int KBYTES = KVT * KSTRIDE;
  constexpr int VBYTES = DVT * 32 * VSTRIDE;
  constexpr int KCH = KVT * DKS * 2;              // 16-B chunks in a K tile
  constexpr int VCH = DVT * 32 * (KVT / 8);       // 16-B chunks in a V^T tile
  static_assert(2 * (KBYTES + VBYTES) <= 160 * 1024, "LDS budget");

  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (KBYTES + VBYTES)];
  unsigned char* const Ks[2] = {smem, smem + KBYTES};                         // hi, lo
  unsigned char* const Vs[2] = {smem + 2 * KBYTES, smem + 2 * KBYTES + VBYTES};

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lg = lane >> 5;
  const int bh = blockIdx.y;
  const int q0 = blockIdx.x * (32 * NW) + wave * 32;
  const size_t qoff = (size_t)bh * p.nq * D, koff = (size_t)bh * p.nkv * D, voff = (size_t)bh * D * p.nkv_pad;
  const f16* const Kg[2] = {p.k + koff, p.k_lo + koff};
  const f16* const Vg[2] = {p.vt + voff, p.vt_lo + voff};

  // Q^T fragments (MFMA B operand): lane (q = l31, g = lg) holds Q[q][16 * ks + 8 * g .. + 8]
  f16x8 qh[DKS], ql[DKS];
#pragma unroll
  for (int ks = 0; ks < DKS; ++ks) {
    const int dcol = ks * 16 + lg * 8;
    f16x8 h = {0, 0, 0, 0, 0, 0, 0, 0}, l = h;
    if (q0 + l31 < p.nq && dcol < D) {
      h = *(const f16x8*)(p.q + qoff + (size_t)(q0 + l31) * D + dcol);
      l = *(const f16x8*)(p.q_lo + qoff + (size_t)(q0 + l31) * D + dcol);
    }
    qh[ks] = h; ql[ks] = l;
  }

  f32x16 o[DVT];
#pragma unroll
  for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  const float sc = p.scale * 1.4426950408889634f;   // scores are exponentiated in log2 units

  const int nt = (p.nkv + KVT - 1) / KVT;
  for (int t = 0; t < nt; ++t) {
    const int kv0 = t * KVT;
    // ---- stage the K and V^T tiles (hi and lo) of keys kv0 .. kv0 + 63; rows / columns past the tensors are zeros ----
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      for (int c = tid; c < KCH; c += NT) {
        const int row = c / (DKS * 2), col = c - row * (DKS * 2);
        f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (kv0 + row < p.nkv && col * 8 < D) v = *(const f16x8*)(Kg[h] + (size_t)(kv0 + row) * D + col * 8);
        *(f16x8*)(Ks[h] + row * KSTRIDE + col * 16) = v;
      }
      for (int c = tid; c < VCH; c += NT) {
        const int row = c / (KVT / 8), col = c - row * (KVT / 8);
        f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < D && kv0 + col * 8 < p.nkv_pad) v = *(const f16x8*)(Vg[h] + (size_t)row * p.nkv_pad + kv0 + col * 8);
        unsigned char* d = Vs[h] + row * VSTRIDE + col * 16;
        *(f16x4*)(d) = f16x4{v[0], v[1], v[2], v[3]};
        *(f16x4*)(d + 8) = f16x4{v[4], v[5], v[6], v[7]};
      }
    }
    __syncthreads();

    // ---- S^T = K Q^T over two 32-key blocks, three products per fragment pair ----
    f32x16 s[KVT / 32];
#pragma unroll
    for (int kvb = 0; kvb < KVT / 32; ++kvb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kvb][r] = 0.f;
      const int kofs = (kvb * 32 + l31) * KSTRIDE + lg * 16;
#pragma unroll
      for (int ks = 0; ks < DKS; ++ks) {
        const f16x8 kh = *(const f16x8*)(Ks[0] + kofs + ks * 32);
        const f16x8 kl = *(const f16x8*)(Ks[1] + kofs + ks * 32);
        s[kvb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[ks], s[kvb], 0, 0, 0);
        s[kvb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[ks], s[kvb], 0, 0, 0);
        s[kvb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ks], s[kvb], 0, 0, 0);
      }
    }
    // ---- mask keys beyond nkv (accumulator register r of lane half lg holds key (r & 3) + 8 (r >> 2) + 4 lg of its block) ----
    if (kv0 + KVT > p.nkv) {
#pragma unroll
      for (int kvb = 0; kvb < KVT / 32; ++kvb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + kvb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lg;
          if (kv >= p.nkv) s[kvb][r] = -1e30f;
        }
    }
    if (CAUSAL && kv0 + KVT - 1 > q0) {          // (wave-uniform: the tile reaches past the wave's first query)
#pragma unroll
      for (int kvb = 0; kvb < KVT / 32; ++kvb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv = kv0 + kvb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lg;
          if (kv > q0 + l31) s[kvb][r] = -1e30f;
        }
    }
    // ---- online softmax in fp32 (per query = per lane column; the halves lg = 0 / 1 hold disjoint keys) ----
    float mx = -1e30f;
#pragma unroll
    for (int kvb = 0; kvb < KVT / 32; ++kvb)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kvb][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx * sc);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    l_run *= alpha;
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
    float psum = 0.f;
#pragma unroll
    for (int kvb = 0; kvb < KVT / 32; ++kvb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __builtin_amdgcn_exp2f(fmaf(s[kvb][r], sc, -m_run));
        s[kvb][r] = pv;
        psum += pv;
      }
    l_run += psum;

    // ---- O^T += V^T P^T, three products per fragment pair ----
#pragma unroll
    for (int kvb = 0; kvb < KVT / 32; ++kvb) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        f16x8 ph, pl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          ph[e] = (f16)s[kvb][8 * s2 + e];
          pl[e] = lo_of(s[kvb][8 * s2 + e], ph[e]);
        }
        const int vofs = l31 * VSTRIDE + (kvb * 32 + 16 * s2 + 4 * lg) * 2;
#pragma unroll
        for (int dt = 0; dt < DVT; ++dt) {
          const unsigned char* vh = Vs[0] + vofs + dt * 32 * VSTRIDE;
          const unsigned char* vl = Vs[1] + vofs + dt * 32 * VSTRIDE;
          const f16x4 h0 = *(const f16x4*)(vh), h1 = *(const f16x4*)(vh + 16);
          const f16x4 l0 = *(const f16x4*)(vl), l1 = *(const f16x4*)(vl + 16);
          const f16x8 ah = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
          const f16x8 al = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, ph, o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, pl, o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, ph, o[dt], 0, 0, 0);
        }
      }
    }
    __syncthreads();          // (the next tile overwrites the stage)
  }

  // ---- normalise and store hi / lo: O[b][q][head * D + dd] ----
  const float l_tot = l_run + __shfl_xor(l_run, 32);
  const int q = q0 + l31;
  if (q < p.nq) {
    const int b = bh / p.heads, head = bh - b * p.heads;
    const size_t row = ((size_t)b * p.nq + q) * ((size_t)p.heads * D) + (size_t)head * D;
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int dd = dt * 32 + 8 * r4 + 4 * lg;
        if (dd < D) {
          f16x4 h, l;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float v = o[dt][r4 * 4 + e] / l_tot;
            h[e] = (f16)v;
            l[e] = lo_of(v, h[e]);
          }
          *(f16x4*)(p.out + row + dd) = h;
          *(f16x4*)(p.out_lo + row + dd) = l;
        }
      }
  }
}

template <int D, bool CAUSAL = false>
int launch_d(const AttnSplitParams& p, hipStream_t stream) {
  constexpr int NW = 4;
  dim3 grid((unsigned)((p.nq + 32 * NW - 1) / (32 * NW)), (unsigned)p.BH);
  SDMI_LAUNCH((attn_split16_kernel<D, NW, CAUSAL>), grid, dim3(NW * 64), 0, stream, p);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace

int launch_attention_split16(const AttnSplitParams& p, hipStream_t stream) {
  SDMI_CHECK(p.q && p.q_lo && p.k && p.k_lo && p.vt && p.vt_lo && p.out && p.out_lo, "split-fp16 attention: null operand");
  SDMI_CHECK(p.BH >= 1 && p.heads >= 1 && p.BH % p.heads == 0 && p.nq >= 1 && p.nkv >= 1, "split-fp16 attention: bad shape");
  SDMI_CHECK(p.nkv_pad >= p.nkv && p.nkv_pad % 8 == 0, "split-fp16 attention: nkv_pad must be >= nkv and a multiple of 8");
  SDMI_CHECK(p.BH <= 65535, "split-fp16 attention: more than 65535 (batch, head) pairs");
  // 2 x MACs of Q K^T and P V (algorithmic); the kernel executes three MFMA passes of each
  const double flops = 4.0 * p.BH * (double)p.nq * p.nkv * p.d;
  const double bytes = 2.0 * 2.0 * p.BH * ((double)p.nq * p.d * 2 + (double)p.nkv * p.d + (double)p.d * p.nkv_pad);
  ProfScope ps(p.causal ? "attention_split16_causal" : "attention_split16", flops, bytes, stream, 3.0 * flops);
  if (p.causal) {
    SDMI_CHECK(p.nq == p.nkv, "split-fp16 causal attention: nq must equal nkv");
    switch (p.d) {
      case 32: return launch_d<32, true>(p, stream);
      case 64: return launch_d<64, true>(p, stream);
      case 128: return launch_d<128, true>(p, stream);
      default:
        return fail("split-fp16 causal attention: head dim " + std::to_string(p.d) + " has no instantiation (32, 64, 128)");
    }
  }
  switch (p.d) {
    case 24: return launch_d<24>(p, stream);       // (the staging writes zeros into the unused half of the second k-step and the V^T rows past d)
    case 32: return launch_d<32>(p, stream);
    case 40: return launch_d<40>(p, stream);
    case 48: return launch_d<48>(p, stream);
    case 64: return launch_d<64>(p, stream);
    case 80: return launch_d<80>(p, stream);
    case 96: return launch_d<96>(p, stream);
    case 128: return launch_d<128>(p, stream);
    case 160: return launch_d<160>(p, stream);
    default:
      if (p.d > 160 && p.d <= 1024 && p.d % 64 == 0) return launch_attention_wide_split16(p, stream);     // attn_wide_split16.hip
      return fail("split-fp16 attention: head dim " + std::to_string(p.d) +
                  " has no instantiation (24, 32, 40, 48, 64, 80, 96, 128, 160, and 192 .. 1024 in steps of 64)");
  }
}

}  // namespace sdmi
