// Kernels of the full-precision UNet mode (sdmi_unet_create_with_precision(..., SDMI_PRECISION_FULL)): every MFMA operand is a
// split-fp16 pair hi = fp16(x), lo = fp16(x - float(hi)), every product a_hi*b_hi + a_lo*b_hi + a_hi*b_lo with fp32 accumulation.
// The default (mixed) mode does not launch any of them.
#pragma once
#include "common.h"

namespace sdmi {

// Split-fp16 flash attention (attn_split16.hip): softmax(Q K^T * scale) V with every operand as a hi / lo pair in the layouts of
// AttnParams (q / k [BH][n][d], v^T [BH][d][nkv_pad] with zero pad keys); out / out_lo [B][nq][heads * d] (heads merged).
struct AttnSplitParams {
  const f16* q = nullptr; const f16* q_lo = nullptr;
  const f16* k = nullptr; const f16* k_lo = nullptr;
  const f16* vt = nullptr; const f16* vt_lo = nullptr;
  f16* out = nullptr; f16* out_lo = nullptr;
  int BH = 0, heads = 0, nq = 0, nkv = 0, nkv_pad = 0, d = 0;
  float scale = 1.f;
  int causal = 0;      // 1: query i sees keys <= i (nq == nkv; d = 32, 64, 128 -- the text encoders' full-precision mode)
};
int launch_attention_split16(const AttnSplitParams& p, hipStream_t stream);
// ... its wide-head form (attn_wide_split16.hip: d = 192 .. 1024 in steps of 64; the V^T pad columns may hold anything there).
// launch_attention_split16 checks the operands and dispatches to it by d: call that one.
int launch_attention_wide_split16(const AttnSplitParams& p, hipStream_t stream);

// The producers of the split operands (split_ops.hip).  Each reads an fp32 GEMM output and writes hi / lo.
// Per-head scatter of columns [col0, col0 + heads * dh) of src [B * ntok][ld]:
//   kind 0: dst[((b * heads + head) * ntok + tok) * dh + dd]           (q, k)
//   kind 1: dst[((b * heads + head) * dh + dd) * ntok_pad + tok]       (v^T; pad tokens ntok .. ntok_pad - 1 written as zero)
int launch_split_heads(const float* src, int ld, int col0, f16* dst, f16* dst_lo, int kind, int B, int ntok, int ntok_pad, int heads,
                       int dh, hipStream_t stream);
// GEGLU (attention.py:222-225): src [M][2 * F] = proj(x) with bias, columns [0, F) the value, [F, 2F) the gate;
// out / out_lo [M][F] = value * gelu(gate) (erf form)
int launch_geglu_split(const float* src, int M, int F, f16* out, f16* out_lo, hipStream_t stream);
// LayerNorm over the C channels of every row of x [M][C] (two-pass fp32 statistics) -> out / out_lo [M][C]
int launch_layernorm_split(const float* x, const float* gamma, const float* beta, f16* out, f16* out_lo, int M, int C, float eps,
                           hipStream_t stream);

}  // namespace sdmi
