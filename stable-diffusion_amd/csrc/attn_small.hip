// One-pass attention for short key ranges (nkv <= 256): the 16 x 16 and 8 x 8 self-attention and every cross-attention below 64 x 64.
//
// attn_dma_kernel (attn.hip) is built for thousands of keys: an LDS-DMA ring, one barrier and one online-softmax rescale per 64-key tile.
// With <= 256 keys there is nothing to stream -- the ring's start-up and the tile-by-tile dependency are its whole run time, on 32
// workgroups.  Here one wave owns 32 queries of one head for the WHOLE key range and shares nothing with any other wave:
//   * S^T = K Q^T for all NKB = ceil(nkv / 32) key blocks on v_mfma_f32_32x32x16_f16, the scores stay in registers (16 fp32 per block);
//   * softmax in ONE pass: the exact row maximum over all blocks, one exp2 per score (the convention of attn.hip: exp2 of the score times
//     scale * log2e, masked beyond nkv), P rounded to fp16, the denominator summed from the rounded P.  No running maximum, no rescale;
//   * O^T = V^T P^T with P fed back from the accumulator registers, as in attn.hip.
// K and V^T fragments come straight from global memory (L2): no LDS, no barrier, so the waves of a workgroup are independent and the
// workgroup size is a launch parameter (1, 2 or 4 waves over the same head).
// The score rows of a block are the keys in the order of attn_dma_kernel's LDS image (bits 2 and 3 of the row swapped), which makes the
// eight keys a lane owns in a P^T fragment contiguous in the V^T row: one 16-byte load per V^T fragment.
// Addresses past a tensor are clamped INTO it (the last key row, the last 8-column chunk of a V^T row, the last row of V^T, the last query):
// what they fetch is finite data of the same tensor, and the score mask (P = 0 exactly), the zero pad columns of V^T (the contract in
// include/sdmi.h) and the store guard keep it out of every stored value.  Nothing outside the four tensors is read or written.
#include "common.h"

namespace sdmi {
namespace {

template <int D, int NKB>
__global__ void __launch_bounds__(256) attn_small_kernel(const AttnParams p) {
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert(D % 16 == 0 && NKB >= 1 && NKB <= 8, "whole k-steps over the head dim; at most 256 keys");
  constexpr int DKS = D / 16;          // k-steps of 16 over the head dim (QK^T)
  constexpr int DVT = (D + 31) / 32;   // 32-row tiles over the head dim (PV)
  constexpr int NST = NKB * 2;         // 16-key steps of the PV product
  constexpr int KPF = D > 80 ? 3 : 4;  // key blocks of K fragments / 16-key steps of V^T fragments in flight ahead of their MFMAs
  constexpr int VPF = D > 80 ? 6 : 8;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, lg = lane >> 5;
  const int bh = blockIdx.y;
  const int q0 = (blockIdx.x * (blockDim.x >> 6) + wave) * 32;
  if (q0 >= p.nq) return;              // (wave-uniform; the kernel has no barrier)
  const f16* Qg = p.q + (size_t)bh * p.nq * D;
  const f16* Kg = p.k + (size_t)bh * p.nkv * D;
  const f16* Vg = p.vt + (size_t)bh * D * p.nkv_pad;

  // Q^T fragments (MFMA B operand): lane (q = l31, g = lg) holds Q[q][16*ks + 8*g .. +8]
  f16x8 qf[DKS];
  {
    const f16* qp = Qg + min(q0 + l31, p.nq - 1) * D + lg * 8;
#pragma unroll
    for (int ks = 0; ks < DKS; ++ks) qf[ks] = *(const f16x8*)(qp + ks * 16);
  }
  // K fragments (A operand): lane (row = l31, g) holds K[key][16*ks + 8*g .. +8], key = the block's first + perm(row)
  const int prow = (l31 & ~12) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);
  f16x8 kf[NKB][DKS];
  auto load_k = [&](int kb) {
    const int key = kb == NKB - 1 ? min(kb * 32 + prow, p.nkv - 1) : kb * 32 + prow;
    const f16* kp = Kg + key * D + lg * 8;
#pragma unroll
    for (int ks = 0; ks < DKS; ++ks) kf[kb][ks] = *(const f16x8*)(kp + ks * 16);
  };
  // V^T fragments (A operand of the PV product) of 16-key step st: lane (row = l31, g) holds V^T[32*dt + row][16*st + 8*g .. +8]
  f16x8 vf[NST][DVT];
  auto load_v = [&](int st) {
    int col = st * 16 + lg * 8;
    if (st >= NST - 2) col = min(col, p.nkv_pad - 8);        // (only the last key block can reach past nkv_pad, a multiple of 8)
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt) {
      const int row = dt * 32 + 31 < D ? dt * 32 + l31 : min(dt * 32 + l31, D - 1);
      vf[st][dt] = *(const f16x8*)(Vg + row * p.nkv_pad + col);
    }
  };

  // The compiler schedules for register pressure and sinks a load to just before its MFMA, which would expose the L2 latency once per MFMA:
  // a sched_barrier pins each group of loads ahead of the MFMAs of the step it is issued in.  In flight ahead of their use: KPF key blocks
  // of K fragments, then VPF 16-key steps of V^T fragments, the first of them issued behind the last K loads so that they travel under the
  // tail of the score MFMAs and the row maximum.
  // ---- S^T = K Q^T, every key block ----
  constexpr int KPFE = KPF < NKB ? KPF : NKB, VPFE = VPF < NST ? VPF : NST, VPER = (VPFE + KPFE - 1) / KPFE;
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 s[NKB];
#pragma unroll
  for (int kb = 0; kb < KPFE; ++kb) load_k(kb);
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    if (kb + KPFE < NKB) {
      load_k(kb + KPFE);
    } else {
#pragma unroll
      for (int st = (kb + KPFE - NKB) * VPER; st < (kb + KPFE - NKB + 1) * VPER && st < VPFE; ++st) load_v(st);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < DKS; ++ks)
      s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[kb][ks], qf[ks], ks == 0 ? zero16 : s[kb], 0, 0, 0);
  }

  // ---- softmax, one pass (per query = per lane column; the halves lg = 0 / 1 hold disjoint keys) ----
#pragma unroll
  for (int r = 0; r < 16; ++r) {       // only the last block can hold keys beyond nkv
    const int kv = (NKB - 1) * 32 + (r & 3) + 4 * ((r >> 2) & 1) + 8 * lg + 16 * (r >> 3);   // (permuted rows)
    if (kv >= p.nkv) s[NKB - 1][r] = -1e30f;
  }
  float mx = -1e30f;
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float sc = p.scale * 1.4426950408889634f;   // scores are compared / exponentiated in log2 units
  const float m = mx * sc;
  f16x8 pf[NST];
  float l4[4] = {0.f, 0.f, 0.f, 0.f};
  auto exp_step = [&](int st) {        // P of 16-key step st: registers 8 (st & 1) .. + 8 of block st / 2 = eight consecutive keys
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const f16 h = (f16)__builtin_amdgcn_exp2f(fmaf(s[st >> 1][8 * (st & 1) + e], sc, -m));
      pf[st][e] = h;
      l4[e & 3] += (float)h;           // the denominator sums what the PV product sums: the rounded P
    }
  };
  exp_step(0);

  // ---- O^T = V^T P^T; the exponentials of step st + 1 run beside the MFMAs of step st ----
  f32x16 o[DVT];
#pragma unroll
  for (int st = 0; st < NST; ++st) {
    if (st + VPFE < NST) load_v(st + VPFE);
    __builtin_amdgcn_sched_barrier(0);
    if (st + 1 < NST) exp_step(st + 1);
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt)
      o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[st][dt], pf[st], st == 0 ? zero16 : o[dt], 0, 0, 0);
  }
  float l = (l4[0] + l4[1]) + (l4[2] + l4[3]);
  l += __shfl_xor(l, 32);

  // ---- normalise and store: O[b][q][head*D + dd] ----
  const float inv = 1.0f / l;
  const int q = q0 + l31;
  if (q < p.nq) {
    const int b = bh / p.heads, head = bh - b * p.heads;
    f16* orow = p.out + ((size_t)b * p.nq + q) * ((size_t)p.heads * D) + (size_t)head * D;
#pragma unroll
    for (int dt = 0; dt < DVT; ++dt)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int dd = dt * 32 + 8 * r4 + 4 * lg;
        if (dd < D) {
          f16x4 v = {(f16)(o[dt][r4 * 4 + 0] * inv), (f16)(o[dt][r4 * 4 + 1] * inv), (f16)(o[dt][r4 * 4 + 2] * inv),
                     (f16)(o[dt][r4 * 4 + 3] * inv)};
          SDMI_ST(f16x4, orow + dd, v);
        }
      }
  }
#endif  // __HIP_DEVICE_COMPILE__
}

template <int D>
int launch_small_d(const AttnParams& p, int nw, hipStream_t stream) {
  const dim3 grid(cdiv(cdiv(p.nq, 32), nw), p.BH), block(64 * nw);
  switch (cdiv(p.nkv, 32)) {
    case 1: SDMI_LAUNCH((attn_small_kernel<D, 1>), grid, block, 0, stream, p); break;
    case 2: SDMI_LAUNCH((attn_small_kernel<D, 2>), grid, block, 0, stream, p); break;
    case 3: SDMI_LAUNCH((attn_small_kernel<D, 3>), grid, block, 0, stream, p); break;
    case 4: SDMI_LAUNCH((attn_small_kernel<D, 4>), grid, block, 0, stream, p); break;
    case 5: SDMI_LAUNCH((attn_small_kernel<D, 5>), grid, block, 0, stream, p); break;
    case 6: SDMI_LAUNCH((attn_small_kernel<D, 6>), grid, block, 0, stream, p); break;
    case 7: SDMI_LAUNCH((attn_small_kernel<D, 7>), grid, block, 0, stream, p); break;
    default: SDMI_LAUNCH((attn_small_kernel<D, 8>), grid, block, 0, stream, p); break;
  }
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace

bool attn_small_supported(int d, int nq, int nkv, int causal) {
  return (d == 80 || d == 160) && !causal && nq > 0 && nkv > 0 && nkv <= 256;
}

int launch_attention_small(const AttnParams& p, int nw, hipStream_t stream) {
  SDMI_CHECK(attn_small_supported(p.d, p.nq, p.nkv, p.causal), "attn_small_kernel: d = 80 / 160, non-causal, at most 256 keys");
  SDMI_CHECK(nw == 1 || nw == 2 || nw == 4, "attn_small_kernel: 1, 2 or 4 waves per workgroup");
  SDMI_CHECK((int64_t)p.nq * p.d < (1ll << 31) && (int64_t)p.d * p.nkv_pad < (1ll << 31), "attn_small_kernel: 32-bit offsets inside a head");
  return p.d == 80 ? launch_small_d<80>(p, nw, stream) : launch_small_d<160>(p, nw, stream);
}

}  // namespace sdmi
