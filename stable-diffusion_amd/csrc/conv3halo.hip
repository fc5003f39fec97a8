// Halo-staged 3x3 convolutions for gfx950 (MI355X): ResBlock in_layers / out_layers convs
// (ldm/modules/diffusionmodules/openaimodel.py:201-204,225-231) -- see the kernel comments.  Split from igemm.hip (round 3) so that
// the two kernel families compile in parallel; the shared device code (epilogue, counted waits) is igemm_dev.h.
#include "igemm_dev.h"

namespace sdmi {
namespace {

// ---- halo-staged 3x3 convolution (stride 1, pad 1) --------------------------------------------------------------------
// ResBlock in_layers / out_layers convs (openaimodel.py:204,230) at the 64x64 .. 16x16 levels.  The generic kernel above
// streams the A operand once per TAP: the nine shifted copies of the same pixels are nine separate k-tiles, so a 3x3 conv
// moves 9x its activation bytes through the CU's vector-memory path -- and that path (64 B/clk/CU), not MFMA issue, is
// what bounds these 15 GFLOP launches.  Here a block owns TH = BM / W whole image rows; for every 64-channel chunk it
// stages the (TH + 2) x (W + 2) input HALO once (LDS-DMA; out-of-image pixels are out-of-range buffer offsets and read as
// zeros) and all nine taps read their A fragments from it at a row offset -- only the weights stream per tap.
// Bytes through the vector-memory path per chunk, 256 x 64 tile: 51 KB halo + 72 KB weights vs 9 x 40 KB = 360 KB.
//   LDS: [halo buffer 0 | halo buffer 1 | NS weight stages]; halo rows are pixels (128 B = 64 channels), XOR-swizzled by
//   the absolute LDS row exactly like the generic tiles, so fragment reads at any row offset stay conflict free.
//   The nine taps are unrolled: every DMA issue and every counted vmcnt wait is static.
// TAIL: a 1x1 GEMM phase behind the chunk loop, into the same accumulators (IGemmParams::tail_*) -- its own instantiations, so the
// launches without a tail keep the code the tuner measured.
template <int BM, int BN, int WARPS_M, int WARPS_N, int NS, bool TAIL = false>
__global__ void __launch_bounds__(WARPS_M* WARPS_N * 64) conv3halo_kernel(const IGemmParams p, const int tiles_m,
                                                                           const int tiles_n, const int chunks_per_split) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int NT = WARPS_M * WARPS_N * 64;
  constexpr int RPP = NT / 8;
  constexpr int PB = BN / RPP;                         // weight DMA pieces per thread per tap
  constexpr int WTM = BM / WARPS_M, WTN = BN / WARPS_N;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int HPMAX = (BM / 64 + 2) * 66;            // halo pixels at W = 64 (the largest for W in {16, 32, 64})
  constexpr int AHP = (HPMAX + RPP - 1) / RPP;         // halo DMA pieces per thread per chunk
  constexpr int HALO_BYTES = AHP * RPP * 128;
  constexpr int BSTAGE = BN * 128;
  constexpr int LDS_BYTES = 2 * HALO_BYTES + NS * BSTAGE;
  // The weight stream is what needs depth: every block reads every (chunk, tap) weight tile exactly once, and the blocks
  // of an XCD walk the taps in step, so most weight tiles are first touches of that XCD's L2 (HBM / Infinity-Cache
  // latency, ~1 us).  NS weight stages = NS - 1 taps of look-ahead; the halo of the NEXT chunk must be complete NS - 2
  // taps before the chunk switch, so it is issued at taps 0 .. LASTA.
  constexpr int LASTA = 10 - NS;
  constexpr int PA = (AHP + LASTA) / (LASTA + 1);      // halo pieces of the NEXT chunk issued per tap (taps 0 .. LASTA)
  constexpr int KS = BK / 16;
  constexpr int G = (TM * TN >= 4) ? 1 : 2;            // k-steps per pipeline unit (>= 4 MFMAs of cover)
  constexpr int U = KS / G;
  constexpr int MPU = G * TM * TN;
  static_assert(PB >= 1 && TM >= 1 && TN >= 1 && RPP % 16 == 0 && NS >= 2 && NS <= 9, "tile/wave shape");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");

  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];

  const int nblk = gridDim.x;
  const int bid = blockIdx.x;
  const int q8 = nblk >> 3, r8 = nblk & 7, xcd = bid & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int tiles_mn = tiles_m * tiles_n;
  const int split = wgid / tiles_mn;
  const int tmn = wgid - split * tiles_mn;
  // which operand an XCD keeps to itself: an XCD runs a contiguous range of tile numbers, and its L2 is private.  With more
  // A bytes than weight bytes (M > N) the range walks N fastest -- few row panels of A, every weight panel -- so A is
  // fetched from the fabric by ONE XCD instead of all eight; the weight-heavy shapes (M <= N) keep walking M fastest.
  int tile_m, tile_n;
  if (p.tile_n_fastest) { tile_m = tmn / tiles_n; tile_n = tmn - tile_m * tiles_n; }
  else { tile_n = tmn / tiles_m; tile_m = tmn - tile_n * tiles_m; }
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int nch = (p.c0 + p.c1 + p.c2) / BK;
  const int c_begin = split * chunks_per_split;
  const int c_end = min(nch, c_begin + chunks_per_split);
  if (c_begin >= c_end) return;

  const int tid = threadIdx.x;
  SDMI_STAMP(dbg_t0);
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int cpos = tid & 7, lrow = tid >> 3;
  const int gch = cpos ^ ((lrow >> 1) & 7);
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int wm = wave / WARPS_N, wn = wave - wm * WARPS_N;
  const int l31 = lane & 31, lg = lane >> 5;
  const int rsw = (l31 >> 1) & 7;

  // tile geometry: BM <= H*W: TH = BM / W rows of one image; BM > H*W: BM / (H*W) whole images (each with its own halo)
  const int W = p.Wout, H = p.Hout, HW = H * W, W2 = W + 2, ld = p.lda0;
  const int bimg = m0 / HW;
  const int THI = p.halo_thi;                     // output rows per image inside the tile
  const int HPI = (THI + 2) * W2;                 // halo pixels per image
  const int y0 = p.halo_ipt > 1 ? 0 : (m0 - bimg * HW) >> p.log2w;
  const int HP = p.halo_ipt * HPI;
  constexpr int OOB = (int)0x80000000;

  // per-lane source byte offset of every halo piece (constant over the chunks: the chunk moves the scalar offset)
  int hvoff[AHP];
#pragma unroll
  for (int q = 0; q < AHP; ++q) {
    const int hp = q * RPP + lrow;
    const int ip = fast_div(hp, p.magic_hpi), hr = hp - ip * HPI;
    const int hy = fast_div(hr, p.magic_w2), hx = hr - hy * W2;
    const int y = y0 + hy - 1, x = hx - 1;
    const bool valid = hp < HP && y >= 0 && y < H && x >= 0 && x < W;
    hvoff[q] = valid ? ((((bimg + ip) * H + y) * W + x) * ld + gch * 8) * 2 : OOB;
  }
  int b_off[PB];
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    const int n = min(n0 + i * RPP + lrow, p.N - 1);
    b_off[i] = (n * p.K + gch * 8) * 2;
  }
  // halo row of tap (0, 0) for the rows of this lane's MFMA tiles
  int hr0[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int ml = wm * WTM + i * 32 + l31;
    const int ip = ml >> p.log2_tpi, mr = ml & ((1 << p.log2_tpi) - 1);     // image inside the tile, pixel inside the image part
    hr0[i] = ip * HPI + (mr >> p.log2w) * W2 + (mr & (W - 1));
  }
  const int b_lds = 2 * HALO_BYTES + (wn * WTN + l31) * 128;

  const char* const srcA0 = (const char*)p.a0; const char* const srcA1 = (const char*)p.a1;
  const char* const srcA2 = (const char*)p.a2;
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, OOB, 0x00020000);
  const int pc0 = p.c0, pc01 = p.c0 + p.c1;
  struct ChunkSrc { __amdgpu_buffer_rsrc_t rsrc; int soff; };
  auto chunk_src = [&](int c) {
    const int cin0 = c * BK;
    const char* src; int coff;
    if (cin0 < pc0) { src = srcA0; coff = cin0; }
    else if (cin0 < pc01) { src = srcA1; coff = cin0 - pc0; }
    else { src = srcA2; coff = cin0 - pc01; }
    ChunkSrc r; r.rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, OOB, 0x00020000); r.soff = coff * 2;
    return r;
  };
  auto issue_halo = [&](const ChunkSrc& cs, int hbuf, int q) {
    auto dst = (__attribute__((address_space(3))) void*)(smem + hbuf * HALO_BYTES + (q * RPP + wave_u * 8) * 128);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(cs.rsrc, dst, 16, hvoff[q], cs.soff, 0, 0);
  };
  auto issue_b = [&](int kt, int stage, int q) {
    auto dst = (__attribute__((address_space(3))) void*)(smem + 2 * HALO_BYTES + stage * BSTAGE + (q * RPP + wave_u * 8) * 128);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_w, dst, 16, b_off[q], kt * (BK * 2), 0, SDMI_W_AUX);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // LDS byte address (k-step 0) of the A fragment rows of MFMA tile i for tap (ky, kx) in halo buffer hbuf;
  // k-step ks is that address ^ (ks << 5) (the 16-byte chunk index is (2 ks + lg) ^ swizzle(row))
  auto a_base = [&](int i, int ky, int kx, int hbuf) -> int {
    const int rowt = hr0[i] + ky * W2 + kx;
    return hbuf * HALO_BYTES + ((rowt << 7) | ((lg ^ ((rowt >> 1) & 7)) << 4));
  };
  auto read_frags = [&](const int (&ab)[TM], int bstage, int ks, f16x8 (&a)[TM], f16x8 (&b)[TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i) a[i] = *(const f16x8*)(smem + (ab[i] ^ (ks << 5)));
    const unsigned char* st = smem + bstage * BSTAGE + b_lds + (((ks * 2 + lg) ^ rsw) << 4);
#pragma unroll
    for (int j = 0; j < TN; ++j) b[j] = *(const f16x8*)(st + j * 32 * 128);
  };
  auto mfma_step = [&](const f16x8 (&a)[TM], const f16x8 (&b)[TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i][j], 0, 0, 0);
  };

  // DMA pieces this thread issues at tap t (t taken mod 9): halo pieces [a_lo, a_hi) of the next chunk, then PB weight
  // pieces.  What may still be in flight when tile kt + 1 is needed = everything issued in the last NS - 2 taps.
  auto a_lo = [](int t) { return t <= LASTA ? (t * PA < AHP ? t * PA : AHP) : AHP; };
  auto a_hi = [](int t) { return t <= LASTA ? ((t + 1) * PA < AHP ? (t + 1) * PA : AHP) : AHP; };
  auto in_flight_ok = [&](int t) {
    int n = 0;
    for (int d = 0; d < NS - 2; ++d) { const int tt = (t - d + 18) % 9; n += a_hi(tt) - a_lo(tt) + PB; }
    return n;
  };

  // ---- prologue: the first halo, then the last NS - 1 taps of a virtual previous chunk (their halo pieces re-issue
  // piece 0: same bytes, same issue counts as the steady state, so the vmcnt literals hold from the first tap on) ----
  const int kt_first = c_begin * 9, kt_last = c_end * 9 - 1;
  {
    const ChunkSrc cs = chunk_src(c_begin);
#pragma unroll
    for (int q = 0; q < AHP; ++q) issue_halo(cs, 0, q);
#pragma unroll
    for (int s2 = 0; s2 < NS - 1; ++s2) {
      const int vt = 9 - (NS - 1) + s2;
#pragma unroll
      for (int e = a_lo(vt); e < a_hi(vt); ++e) issue_halo(cs, 0, 0);
#pragma unroll
      for (int q = 0; q < PB; ++q) issue_b(min(kt_first + s2, kt_last), s2, q);
    }
  }
  wait_vmcnt_n(in_flight_ok(8));
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  SDMI_STAMP(dbg_t1);
  f16x8 fa[2][G][TM], fb[2][G][TN];
  int ab[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) ab[i] = a_base(i, 0, 0, 0);
#pragma unroll
  for (int g = 0; g < G; ++g) read_frags(ab, 0, g, fa[0][g], fb[0][g]);

  int cur = 0, nxt = NS - 1, hb = 0;
  for (int c = c_begin; c < c_end; ++c) {
    // the next chunk's halo streams in during taps 0..7 (the last chunk of the split reloads itself: same issue counts,
    // so every vmcnt literal below stays valid)
    const ChunkSrc csn = chunk_src(min(c + 1, c_end - 1));
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int kt = c * 9 + tap;
      const int tap1 = tap == 8 ? 0 : tap + 1;
      const int hb1 = tap == 8 ? (hb ^ 1) : hb;
      const int cur1 = (cur + 1 == NS) ? 0 : cur + 1;
      int ab1[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) ab1[i] = a_base(i, tap1 / 3, tap1 % 3, hb1);
      const int alo = a_lo(tap);
      const int na = a_hi(tap) - alo;                   // compile-time after unrolling
      const int npieces = na + PB;
      const int ppu = (npieces + U - 2) / (U - 1);
      const int bt = min(kt + NS - 1, kt_last);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (u + 1 < U) {
#pragma unroll
          for (int g = 0; g < G; ++g) read_frags(ab, cur, (u + 1) * G + g, fa[(u + 1) & 1][g], fb[(u + 1) & 1][g]);
#pragma unroll
          for (int e = u * ppu; e < (u + 1) * ppu && e < npieces; ++e) {
            if (e < na) issue_halo(csn, hb ^ 1, alo + e);         // halo pieces first: older than this tap's weights
            else issue_b(bt, nxt, e - na);
          }
        } else {
          // allowed in flight: what the last NS - 2 taps issued.  Weight tile kt + 1 -- and, at tap 8, the whole next halo
          // (issued at taps <= LASTA) -- has landed for this wave; the barrier makes it everybody's, and tells everybody
          // this tile's LDS reads are done
          wait_vmcnt_n(in_flight_ok(tap));
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
          for (int g = 0; g < G; ++g) read_frags(ab1, cur1, g, fa[0][g], fb[0][g]);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) mfma_step(fa[u & 1][g], fb[u & 1][g]);
        __builtin_amdgcn_sched_group_barrier(0x100, G * (TM + TN), 0);
#pragma unroll
        for (int e = 0; e < MPU; ++e) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          if (u + 1 < U && e < ppu && u * ppu + e < npieces) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        }
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) ab[i] = ab1[i];
      cur = cur1;
      nxt = (nxt + 1 == NS) ? 0 : nxt + 1;
      hb = hb1;
    }
  }
  wait_vmcnt<0>();
  if constexpr (TAIL) {
    // ---- 1x1 tail phase (a ResBlock's skip_connection): the k-tiles [t_begin, t_end) of out += A_t W_t^T, A_t = the tile's BM output
    // pixels as rows of up to three K-concatenated fp16 [M][tail_c] sources, W_t = [N][tail_kt] row-major.  The loop is the DMA main
    // loop of igemm_kernel<..., KIND_1X1> (stages of (BM + BN) x 128 B, the same swizzle and fragment reads, one raw barrier per k-tile,
    // counted vmcnt waits: the phase issues nothing but LDS-DMA) over the LDS the drained halo buffers and weight stages leave free.
    // split / p.splitk / p.tail_kt are scalars: the range and the branch around the phase are the same for every wave of the workgroup,
    // and a workgroup with an empty range takes no barrier of it.
    int t_begin, t_end;
    tail_split_range(p.tail_kt / BK, p.splitk, split, &t_begin, &t_end);
    if (t_begin < t_end) {
      constexpr int A_PASSES = BM / RPP;
      constexpr int STAGE_T = (BM + BN) * 128;
      constexpr int NS_T = LDS_BYTES / STAGE_T < 4 ? LDS_BYTES / STAGE_T : 4;
      constexpr int LPT = A_PASSES + PB;               // DMA instructions per thread per k-tile
      constexpr int PPU = (LPT + U - 2) / (U - 1);     // ... issued in each of the first U - 1 units
      static_assert(A_PASSES >= 1 && NS_T >= 3 && NS_T * STAGE_T <= LDS_BYTES && LPT * (NS_T - 2) <= 48, "tail ring");
      // every wave is out of the chunk loop and its surplus DMA has landed: halo buffers and weight stages are free LDS
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      int ta_off[A_PASSES], tb_off[PB];
#pragma unroll
      for (int i = 0; i < A_PASSES; ++i) ta_off[i] = (min(m0 + i * RPP + lrow, p.M - 1) * p.tail_ld + gch * 8) * 2;
#pragma unroll
      for (int i = 0; i < PB; ++i) tb_off[i] = (min(n0 + i * RPP + lrow, p.N - 1) * p.tail_kt + gch * 8) * 2;
      const __amdgpu_buffer_rsrc_t rsrc_tw = __builtin_amdgcn_make_buffer_rsrc((void*)p.tail_w, 0, OOB, 0x00020000);
      const char* const srcT0 = (const char*)p.tail_a0; const char* const srcT1 = (const char*)p.tail_a1;
      const char* const srcT2 = (const char*)p.tail_a2;
      const int tc = p.tail_c;
      // load cursor (wave-uniform): the next k-tile to issue; it stops on the last k-tile of the range
      // (the NS_T - 1 surplus issues at the end reload that tile: in bounds, never consumed)
      int ld_kt = t_begin;
      const int tc2 = 2 * tc;
      struct TailCursor { __amdgpu_buffer_rsrc_t rsrc_a; int a_soff, b_soff; unsigned lds; };
      auto next_tile = [&](int stage) {
        TailCursor c;
        const int k0 = ld_kt * BK;                     // first column of the tile in the concatenated K
        const char* src; int coff;
        if (k0 < tc) { src = srcT0; coff = k0; }
        else if (k0 < tc2) { src = srcT1; coff = k0 - tc; }
        else { src = srcT2; coff = k0 - tc2; }
        c.rsrc_a = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, OOB, 0x00020000);
        c.a_soff = coff * 2; c.b_soff = k0 * 2; c.lds = stage * STAGE_T;
        if (ld_kt + 1 < t_end) ++ld_kt;
        return c;
      };
      auto issue_piece = [&](const TailCursor& c, int q) {
        const unsigned row0 = (q < A_PASSES ? q * RPP : BM + (q - A_PASSES) * RPP) + wave_u * 8;
        auto dst = (__attribute__((address_space(3))) void*)(smem + c.lds + row0 * 128);
        if (q < A_PASSES) __builtin_amdgcn_raw_ptr_buffer_load_lds(c.rsrc_a, dst, 16, ta_off[q], c.a_soff, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_tw, dst, 16, tb_off[q - A_PASSES], c.b_soff, 0, SDMI_W_AUX);
      };
      const int ta_lds = (wm * WTM + l31) * 128, tb_lds = BM * 128 + (wn * WTN + l31) * 128;
      auto read_tail = [&](int stage, int ks, f16x8 (&a)[TM], f16x8 (&b)[TN]) {
        const unsigned char* st = smem + stage * STAGE_T + (((ks * 2 + lg) ^ rsw) << 4);
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i] = *(const f16x8*)(st + ta_lds + i * 32 * 128);
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j] = *(const f16x8*)(st + tb_lds + j * 32 * 128);
      };
#pragma unroll
      for (int s2 = 0; s2 < NS_T - 1; ++s2) {
        const TailCursor c = next_tile(s2);
#pragma unroll
        for (int q = 0; q < LPT; ++q) issue_piece(c, q);
      }
      wait_vmcnt<LPT*(NS_T - 2)>();
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
      for (int g = 0; g < G; ++g) read_tail(0, g, fa[0][g], fb[0][g]);
      int tcur = 0, tnxt = NS_T - 1;
      for (int kt = t_begin; kt < t_end; ++kt) {
        const TailCursor c = next_tile(tnxt);
        const int tcur1 = (tcur + 1 == NS_T) ? 0 : tcur + 1;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (u + 1 < U) {
#pragma unroll
            for (int g = 0; g < G; ++g) read_tail(tcur, (u + 1) * G + g, fa[(u + 1) & 1][g], fb[(u + 1) & 1][g]);
#pragma unroll
            for (int q = u * PPU; q < (u + 1) * PPU && q < LPT; ++q) issue_piece(c, q);
          } else {
            wait_vmcnt<LPT*(NS_T - 2)>();               // this wave's share of tile kt + 1 has landed
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // ... and everybody's; tile kt is fully read
#pragma unroll
            for (int g = 0; g < G; ++g) read_tail(tcur1, g, fa[0][g], fb[0][g]);
          }
#pragma unroll
          for (int g = 0; g < G; ++g) mfma_step(fa[u & 1][g], fb[u & 1][g]);
          __builtin_amdgcn_sched_group_barrier(0x100, G * (TM + TN), 0);
#pragma unroll
          for (int e = 0; e < MPU; ++e) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (u + 1 < U && e < PPU && u * PPU + e < LPT) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
          }
        }
        tcur = tcur1;
        tnxt = (tnxt + 1 == NS_T) ? 0 : tnxt + 1;
      }
      wait_vmcnt<0>();
    }
  }
  SDMI_STAMP(dbg_t2);
  igemm_epilogue<BM, BN, WARPS_M, WARPS_N, LDS_BYTES>(p, acc, m0, n0, split, tile_m, tile_n, smem);
#ifdef SDMI_IGEMM_TIMING
  if (p.dbg_times && tid == 0) {
    long long* d = p.dbg_times + 6 * (size_t)blockIdx.x;
    d[0] = dbg_t0; d[1] = dbg_t1; d[2] = dbg_t2; d[4] = (long long)__builtin_readcyclecounter();
  }
#endif
#endif  // __HIP_DEVICE_COMPILE__
}

}  // namespace

// halo-staged 3x3 convolution: supported iff stride 1, pad 1, no upsampling, power-of-two width 16..64 and tiles of whole
// image rows that do not straddle samples
bool halo_supported(const IGemmParams& p, int bm) {
  const int W = p.Wout, HW = p.Hout * p.Wout;
  // (whole 64-channel chunks only: a source that ends in a half k-tile stays on the generic kernel)
  if (p.c0 % BK || p.c1 % BK || p.c2 % BK) return false;
  if (!(p.ksize == 3 && p.stride == 1 && p.pad == 1 && !p.up && p.Hin == p.Hout && p.Win == p.Wout && W >= 8 && W <= 64 &&
        (W & (W - 1)) == 0 && bm % W == 0))
    return false;
  const int cap = (((bm / 64 + 2) * 66 + bm / 4 - 1) / (bm / 4)) * (bm / 4);    // halo rows an LDS buffer holds (AHP * RPP)
  if (bm <= HW) return HW % bm == 0 && (bm / W + 2) * (W + 2) <= cap;
  return bm % HW == 0 && p.M % bm == 0 && (bm / HW) * (p.Hout + 2) * (W + 2) <= cap;    // whole images per tile
}

template <int BM, int BN, int WARPS_M, int WARPS_N, int NS>
int launch_halo_cfg(const IGemmParams& p, int splitk, hipStream_t stream) {
  SDMI_CHECK(halo_supported(p, BM), "halo-staged conv tile requested for an unsupported shape");
  if (p.tail_kt) {      // the 1x1 tail phase (IGemmParams::tail_*): whole 64-channel k-tiles of one to three equally wide sources
    const int nsrc = p.tail_c > 0 ? p.tail_kt / p.tail_c : 0;
    SDMI_CHECK(p.tail_c > 0 && p.tail_c % BK == 0 && nsrc >= 1 && nsrc <= 3 && nsrc * p.tail_c == p.tail_kt && p.tail_w && p.tail_a0 &&
                   (nsrc < 2 || p.tail_a1) && (nsrc < 3 || p.tail_a2) && p.tail_ld >= p.tail_c && p.tail_ld % 8 == 0,
               "1x1 tail: one to three sources of tail_c % 64 == 0 channels, tail_kt = sources * tail_c, pitch >= tail_c and % 8 == 0");
    SDMI_CHECK((int64_t)p.M * p.tail_ld * 2 < ((int64_t)1 << 31) - 65536 && (int64_t)p.N * p.tail_kt * 2 < ((int64_t)1 << 31) - 65536,
               "1x1 tail: tensor too large for 31-bit byte offsets (buffer addressing)");
    SDMI_CHECK(p.mode == EPI_PLAIN && p.M % BM == 0, "1x1 tail: plain mode, whole row tiles");
  }
  const int tiles_m = cdiv(p.M, BM), tiles_n = cdiv(p.N, BN);
  const int nch = (p.c0 + p.c1 + p.c2) / BK;
  const int chunks_per_split = cdiv(nch, splitk);
  const int nsplit = cdiv(nch, chunks_per_split);
  IGemmParams q = p;
  q.splitk = nsplit;
  q.tile_n_fastest = tile_order_n_fastest(p);
  q.splitk_fused = 0;
  slab_layout(q, BM, BN, WARPS_M, WARPS_N, nsplit);
  q.epi_vec = epi_vec_ok(p);
  SDMI_CHECK(splitk_ws_need(p, BM, BN, nsplit) <= p.splitk_ws_floats, "split-K workspace too small");
  SDMI_CHECK((int64_t)p.M < (int64_t)65536 * p.Hout * p.Wout, "fast_div_hw: at most 65535 samples per launch");
  q.magic_hw = div_magic_hw(p.Hout * p.Wout);
  q.magic_w = div_magic(p.Wout);
  q.magic_w2 = div_magic(p.Wout + 2);
  q.log2w = 0;
  while ((1 << q.log2w) < p.Wout) ++q.log2w;
  {
    const int HW = p.Hout * p.Wout;
    q.halo_ipt = BM <= HW ? 1 : BM / HW;
    q.halo_thi = BM <= HW ? BM / p.Wout : p.Hout;
    q.magic_hpi = div_magic((q.halo_thi + 2) * (p.Wout + 2));
    const int tpi = q.halo_thi * p.Wout;             // output pixels per image part: a power of two when halo_ipt > 1
    q.log2_tpi = 0;
    while ((1 << q.log2_tpi) < tpi) ++q.log2_tpi;
    if (q.halo_ipt == 1) q.log2_tpi = 30;            // one image: every row of the tile belongs to part 0
  }
  for (int t = 0; t < p.gn_n; ++t) q.gn_magic[t] = div_magic(p.gn_cpg[t]);
  dim3 grid(tiles_m * tiles_n * nsplit), block(WARPS_M * WARPS_N * 64);
  static const int by_shape = env_int("SDMI_PROF_SHAPES", 0);
  std::string pname = std::string("conv3halo_") + std::to_string(BM) + "x" + std::to_string(BN) + "w" +
                      std::to_string(WARPS_M * WARPS_N) + "s" + std::to_string(NS);
  if (by_shape && prof_enabled())
    pname += "_M" + std::to_string(p.M) + "_N" + std::to_string(p.N) + "_K" + std::to_string(p.K) + "_s" + std::to_string(nsplit) +
             (p.tail_kt ? "_t" + std::to_string(p.tail_kt) : std::string());
  const double src_pix = (double)p.B * p.Hin * p.Win;
  // (the tail counts as the reference 1x1 conv: tail_c channels, whatever the number of passes -- as launch_cfg counts k_alg)
  ProfScope ps(pname.c_str(), 2.0 * p.M * (double)p.N * (p.K + (p.tail_kt ? p.tail_c : 0)),
               src_pix * (p.c0 + p.c1) * 2.0 + (double)p.N * p.K * 2.0 + (double)p.M * p.N * ((p.out_f32 ? 4.0 : 0.0) + (p.out_f16 ? 2.0 : 0.0)) +
                   (p.residual ? (double)p.M * p.N * 4.0 : 0.0) + (p.tail_kt ? ((double)p.M + p.N) * p.tail_c * 2.0 : 0.0),
               stream);
  if (p.tail_kt) SDMI_LAUNCH((conv3halo_kernel<BM, BN, WARPS_M, WARPS_N, NS, true>), grid, block, 0, stream, q, tiles_m, tiles_n, chunks_per_split);
  else SDMI_LAUNCH((conv3halo_kernel<BM, BN, WARPS_M, WARPS_N, NS>), grid, block, 0, stream, q, tiles_m, tiles_n, chunks_per_split);
  SDMI_HIP_OK(hipGetLastError());
  ps.end();
  if (nsplit > 1) return launch_splitk_reduce(q, nsplit, stream);
  if (q.ln_out) return launch_layernorm(q.out_f32, q.ln_gamma, q.ln_beta, q.ln_out, q.M, q.N, q.ln_eps, stream);
  return 0;
}

// tile ids 14 .. 17 of the table in igemm.hip (kTiles)
int launch_halo_tile(int tile, const IGemmParams& p, int splitk, hipStream_t stream) {
  switch (tile) {
    case 14: return launch_halo_cfg<256, 64, 4, 2, 5>(p, splitk, stream);
    case 15: return launch_halo_cfg<256, 128, 4, 2, 3>(p, splitk, stream);
    case 16: return launch_halo_cfg<128, 64, 2, 2, 8>(p, splitk, stream);
    case 17: return launch_halo_cfg<128, 128, 2, 2, 5>(p, splitk, stream);
    default: return fail("not a halo-staged conv tile id");
  }
}

}  // namespace sdmi
