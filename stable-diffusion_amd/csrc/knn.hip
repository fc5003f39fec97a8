// Exact k-nearest-neighbour search by cosine over a database of raw fp32 embeddings: the `Searcher.search` of the reference's
// scripts/knn2img.py (scann score_brute_force, dot_product between unit vectors), kept on the device.
//   * knn_inv_norm_kernel:  inv_norm[row] = 1 / ||x_row||, one wave per row; knn_first_bad_kernel finds the first row whose norm is zero or
//     not finite (one workgroup, no atomics).
//   * knn_scan_kernel<QB, J>: workgroup (slab, query chunk) streams the slab's rows once with 16-byte loads; the chunk's QB queries sit
//     normalised in LDS.  A wave takes four rows per step, every lane 4 J floats of each row (J = ceil(D / 256)), and accumulates the
//     4 x QB partial dot products with VALU FMAs in one fixed order.  A butterfly over the lane masks 32, 16, .. 1 sums the partials and
//     leaves value (row r, query b) on its own lane: the tree is the same for every row, slot, slab and QB, so a (query, row) score has the
//     same bits wherever the row sits.  score = dot * inv_norm[row].
//     Every wave keeps a list per query in LDS behind a threshold held in registers (the k-th best, under the order "score descending, row
//     index ascending", as of the list's last compaction): a row that beats it is appended, a full list is cut back to its k best by rank
//     counting, which tightens the threshold; after warm-up a row costs one compare.  The eight wave lists are merged at the end of the slab
//     and written as candidates [B][n_slabs][k], sorted, short lists padded with (-inf, INT_MAX).
//   * knn_merge_kernel:     one workgroup per (query, group of lists) reduces its candidates with the same wave lists; the last compaction
//     leaves the k survivors in rank order: descending score, ties to the lower row index.  The handle runs it twice above 64 slabs: groups
//     of 32 lists first, then the group results.
//   * knn_gather_kernel:    out[b][slot][:] = x[idx] * inv_norm[idx]; the conditioning form copies slot 0 from c[b][0][:] bit for bit.
// No atomics, no cross-workgroup communication, every loop bounded; every sum has one fixed order.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "knn.h"
#include "prof.h"

namespace sdmi {
namespace {

constexpr int KNN_WAVES = 8;        // waves per workgroup (scan and merge)
constexpr int KNN_R = 4;            // rows per wave step
constexpr int KNN_MAXK = 64;
constexpr int KNN_MAXD = 1024;
constexpr int KNN_MAXB = 64;

__device__ __forceinline__ bool knn_better(float s1, int i1, float s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

// sum over the 64 lanes in the fixed order of the masks 32, 16, .. 1; every lane gets the same bits (a + b == b + a)
__device__ __forceinline__ float knn_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// A wave's top-k list for one query: up to CAP (score, row index) pairs in LDS, n of them in use, and a threshold (thr_s, thr_i) = the k-th
// best entry as of the last compaction, (-inf, INT_MAX) while the list holds fewer than k.  Candidates that beat the threshold are APPENDED;
// when the list runs out of room, knn_wave_compact keeps the k best by rank counting and tightens the threshold.  The state (n, threshold)
// lives in registers, the same on every lane that works for that query.  Only this wave touches the list.
struct KnnEntry { float s; int i; };

// rank every entry among the n (lane takes entries lane and lane + 64; the order is total, so the ranks are 0 .. n - 1), keep ranks < k
// at position = rank: the list leaves sorted, best first
__device__ __forceinline__ void knn_wave_compact(volatile KnnEntry* list, int k, int lane, int& n, float& thr_s, int& thr_i) {
  const int nu = __builtin_amdgcn_readfirstlane(n);        // (the same on every lane; scalar for the loop and the lane reads below)
  const int e0 = lane, e1 = lane + 64;
  const float s0 = e0 < nu ? list[e0].s : -INFINITY, s1 = e1 < nu ? list[e1].s : -INFINITY;
  const int i0 = e0 < nu ? list[e0].i : INT_MAX, i1 = e1 < nu ? list[e1].i : INT_MAX;
  int r0 = 0, r1 = 0;
  const int na = nu < 64 ? nu : 64;
  for (int t = 0; t < na; ++t) {           // entry t sits in lane t's registers: a lane read, no LDS round trip
    const float ts = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s0), t));
    const int ti = __builtin_amdgcn_readlane(i0, t);
    r0 += knn_better(ts, ti, s0, i0) ? 1 : 0;
    r1 += knn_better(ts, ti, s1, i1) ? 1 : 0;
  }
  for (int t = 64; t < nu; ++t) {
    const float ts = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s1), t - 64));
    const int ti = __builtin_amdgcn_readlane(i1, t - 64);
    r0 += knn_better(ts, ti, s0, i0) ? 1 : 0;
    r1 += knn_better(ts, ti, s1, i1) ? 1 : 0;
  }
  __builtin_amdgcn_wave_barrier();
  if (e0 < nu && r0 < k) { list[r0].s = s0; list[r0].i = i0; }
  if (e1 < nu && r1 < k) { list[r1].s = s1; list[r1].i = i1; }
  __builtin_amdgcn_wave_barrier();
  n = nu < k ? nu : k;
  if (n == k) { thr_s = list[k - 1].s; thr_i = list[k - 1].i; }
  else { thr_s = -INFINITY; thr_i = INT_MAX; }
}

// Make room for `room` more entries in every list of the wave: lists [QB] of CAP entries at `lists`, lane's list is lq, lane's copy of
// that list's state is (n, thr_s, thr_i).  At most QB compactions.
template <int CAP>
__device__ __forceinline__ void knn_wave_ensure_room(volatile KnnEntry* lists, int nlists, int k, int lane, int lq, int room, int& n, float& thr_s,
                                                     int& thr_i) {
  for (int turn = 0; turn < nlists; ++turn) {
    const unsigned long long need = __ballot(n + room > CAP);
    if (need == 0ull) break;
    const int src = __ffsll((long long)need) - 1;
    const int cq = __shfl(lq, src);
    int cn = __shfl(n, src);
    float cs; int ci;
    knn_wave_compact(lists + cq * CAP, k, lane, cn, cs, ci);
    if (lq == cq) { n = cn; thr_s = cs; thr_i = ci; }
  }
}

// Append the candidates that beat their list's threshold.  same_q: the lanes that may offer to this lane's list (the lane itself included);
// the caller has made room for all of them.
template <int CAP>
__device__ __forceinline__ void knn_wave_offer(volatile KnnEntry* lists, int lane, int lq, unsigned long long same_q, bool valid, float score, int idx,
                                               int& n, float thr_s, int thr_i) {
  const bool pend = valid && knn_better(score, idx, thr_s, thr_i);
  const unsigned long long mine = __ballot(pend) & same_q;
  if (pend) {
    const int slot = n + __popcll(mine & ((1ull << lane) - 1ull));
    lists[lq * CAP + slot].s = score;
    lists[lq * CAP + slot].i = idx;
  }
  n += __popcll(mine);
  __builtin_amdgcn_wave_barrier();
}

__global__ void __launch_bounds__(512) knn_inv_norm_kernel(const float* __restrict__ db, float* __restrict__ inv_norm, int64_t N, int D) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * KNN_WAVES + (threadIdx.x >> 6);
  if (row >= N) return;
  const f32x4* p = (const f32x4*)(db + row * D);
  const int D4 = D >> 2;
  float ss = 0.f;
  for (int c = lane; c < D4; c += 64) {
    const f32x4 v = p[c];
    ss = fmaf(v[0], v[0], ss); ss = fmaf(v[1], v[1], ss); ss = fmaf(v[2], v[2], ss); ss = fmaf(v[3], v[3], ss);
  }
  ss = knn_wave_sum(ss);
  if (lane == 0) inv_norm[row] = 1.0f / sqrtf(ss);
}

// first row whose inverse norm is not a positive finite number (norm zero, infinite or NaN), or -1
__global__ void __launch_bounds__(1024) knn_first_bad_kernel(const float* __restrict__ inv_norm, int64_t N, long long* __restrict__ out) {
  __shared__ long long s_first[1024];
  long long first = LLONG_MAX;
  for (int64_t r = threadIdx.x; r < N; r += 1024) {
    const float v = inv_norm[r];
    if (!(v > 0.f && v < INFINITY)) { first = r; break; }
  }
  s_first[threadIdx.x] = first;
  __syncthreads();
  for (int n = 512; n >= 1; n >>= 1) {
    if ((int)threadIdx.x < n && s_first[threadIdx.x + n] < s_first[threadIdx.x]) s_first[threadIdx.x] = s_first[threadIdx.x + n];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s_first[0] == LLONG_MAX ? -1ll : s_first[0];
}

template <int J>
struct KnnRows {
  f32x4 x[KNN_R][J];
  float inr;
};

template <int QB, int J>
__global__ void __launch_bounds__(512) knn_scan_kernel(const float* __restrict__ db, const float* __restrict__ inv_norm,
                                                       const float* __restrict__ queries, float* __restrict__ cand_s, int* __restrict__ cand_i,
                                                       int64_t N, int D, int B, int k, int64_t slab_rows, int n_slabs) {
  constexpr int V = KNN_R * QB;          // values per wave step; a power of two <= 64
  constexpr int LPV = 64 / V;            // lanes that end up with the same value
  constexpr int SQ = J * 256;            // floats per query in LDS: D rounded up to whole wave loads, the pad columns zero
  __shared__ __attribute__((aligned(16))) float s_q[QB * SQ];            // the chunk's queries, normalised: [QB][SQ]
  constexpr int CAP = QB < 16 ? 128 : (J < 4 ? 96 : 80);                // entries per wave list: what the 160 KB of LDS leave (k + 16 <= CAP)
  __shared__ KnnEntry s_list[KNN_WAVES * QB * CAP];                      // wave lists [wave][QB][CAP]
  __shared__ int s_cnt[KNN_WAVES * QB];                                  // their sizes at the end of the slab
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (scalar: row addresses stay in SGPRs)
  const int D4 = D >> 2;
  const int q0 = blockIdx.y * QB;
  const int nq = B - q0 < QB ? B - q0 : QB;
  const int slab = blockIdx.x;

  // queries of the chunk: q / ||q||, the norm summed as the rows' norms are; slots past nq hold zeros
  for (int b = wave; b < QB; b += KNN_WAVES) {
    f32x4 v[J];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int c = j * 64 + lane;
      v[j] = (b < nq && c < D4) ? ((const f32x4*)(queries + (int64_t)(q0 + b) * D))[c] : f32x4{0.f, 0.f, 0.f, 0.f};
      ss = fmaf(v[j][0], v[j][0], ss); ss = fmaf(v[j][1], v[j][1], ss); ss = fmaf(v[j][2], v[j][2], ss); ss = fmaf(v[j][3], v[j][3], ss);
    }
    ss = knn_wave_sum(ss);
    const float nrm = b < nq ? sqrtf(ss) : 1.f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int c = j * 64 + lane;
      ((f32x4*)(s_q + b * SQ))[c] = f32x4{v[j][0] / nrm, v[j][1] / nrm, v[j][2] / nrm, v[j][3] / nrm};       // (columns past D: 0 / nrm = 0)
    }
  }
  volatile KnnEntry* my_lists = s_list + wave * QB * CAP;
  __syncthreads();

  const int vidx = lane / LPV;           // the value this lane holds after the butterfly: row slot vidx / QB, query vidx % QB
  const int my_r = vidx / QB, my_b = vidx % QB;
  const bool active = lane % LPV == 0 && my_b < nq;
  unsigned long long same_q = 0ull;      // the lanes that offer to this lane's query: one per row slot
#pragma unroll
  for (int r = 0; r < KNN_R; ++r) same_q |= 1ull << ((r * QB + my_b) * LPV);
  float thr_s = -INFINITY;
  int thr_i = INT_MAX, n_list = 0;

  const int64_t r0 = (int64_t)slab * slab_rows;
  const int64_t r1 = r0 + slab_rows < N ? r0 + slab_rows : N;
  constexpr int64_t STEP = KNN_WAVES * KNN_R;

  // Loads are clamped, not predicated: a row past the slab's end re-reads the slab's last row (its values are never offered) and a column
  // past D re-reads the row's last 16 bytes, which meet the zero pad columns of the queries (0 * finite = 0: finalize admits finite rows only).
  int cc[J];
#pragma unroll
  for (int j = 0; j < J; ++j) cc[j] = j * 64 + lane < D4 ? j * 64 + lane : D4 - 1;
  auto load = [&](int64_t row, KnnRows<J>& t) {
#pragma unroll
    for (int r = 0; r < KNN_R; ++r) {
      const int64_t rc = row + r < r1 ? row + r : r1 - 1;
      const f32x4* p = (const f32x4*)(db + rc * D);
#pragma unroll
      for (int j = 0; j < J; ++j) t.x[r][j] = p[cc[j]];
    }
    t.inr = inv_norm[row + my_r < r1 ? row + my_r : r1 - 1];
  };

  // the next step's rows are loaded ahead of this step's FMAs where the registers allow it (the wider variants rely on the SIMD's second wave)
  constexpr bool PF = V + 2 * KNN_R * J * 4 + 16 <= 200;
  KnnRows<J> cur, nxt;
  int64_t row = r0 + (int64_t)wave * KNN_R;
  if (PF && row < r1) load(row, cur);
  for (; row < r1; row += STEP) {
    const bool more = PF && row + STEP < r1;
    if (!PF) load(row, cur);
    if (more) load(row + STEP, nxt);
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    // (query vectors come from LDS one group of G ahead of their FMAs; the scheduling barrier keeps the compiler from hoisting them all)
    constexpr int G = QB >= 4 ? 4 : 1;
    auto ldq = [&](int t) { return ((const f32x4*)(s_q + (t % QB) * SQ))[(t / QB) * 64 + lane]; };
    f32x4 qn[G];
#pragma unroll
    for (int g = 0; g < G; ++g) qn[g] = ldq(g);
#pragma unroll
    for (int t0 = 0; t0 < J * QB; t0 += G) {
      f32x4 qv[G];
#pragma unroll
      for (int g = 0; g < G; ++g) qv[g] = qn[g];
      if (t0 + G < J * QB) {
#pragma unroll
        for (int g = 0; g < G; ++g) qn[g] = ldq(t0 + G + g);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int j = (t0 + g) / QB, b = (t0 + g) % QB;
#pragma unroll
        for (int r = 0; r < KNN_R; ++r) {
          float a = acc[r * QB + b];
          a = fmaf(cur.x[r][j][0], qv[g][0], a); a = fmaf(cur.x[r][j][1], qv[g][1], a);
          a = fmaf(cur.x[r][j][2], qv[g][2], a); a = fmaf(cur.x[r][j][3], qv[g][3], a);
          acc[r * QB + b] = a;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // butterfly: at mask m a lane keeps half of its values and hands the other half to lane ^ m; log2(V) steps leave one value per lane
    int m = 32;
#pragma unroll
    for (int n = V / 2; n >= 1; n >>= 1, m >>= 1) {
      const bool up = (lane & m) != 0;
#pragma unroll
      for (int i = 0; i < n; ++i) {
        const float lo = acc[i], hi = acc[i + n];
        const float got = __shfl_xor(up ? lo : hi, m);
        acc[i] = (up ? hi : lo) + got;
      }
    }
#pragma unroll
    for (; m >= 1; m >>= 1) acc[0] += __shfl_xor(acc[0], m);      // (V < 64: the remaining masks, summed on every lane of the group)

    const int64_t rr = row + my_r;
    const float score = acc[0] * cur.inr;
    knn_wave_ensure_room<CAP>(my_lists, QB, k, lane, my_b, KNN_R, n_list, thr_s, thr_i);
    knn_wave_offer<CAP>(my_lists, lane, my_b, same_q, active && rr < r1, score, (int)rr, n_list, thr_s, thr_i);
    if (more) cur = nxt;
  }
  // every wave sorts its lists down to k and publishes their sizes
  for (int b = 0; b < QB; ++b) {
    int cn = __shfl(n_list, b * LPV);
    float cs; int ci;
    knn_wave_compact(my_lists + b * CAP, k, lane, cn, cs, ci);
    if (lane == 0) s_cnt[wave * QB + b] = cn;
  }
  __syncthreads();

  // merge the eight wave lists of a query into wave 0's list (wave w takes queries w, w + 8, ..), then write the slab's candidates
  for (int b = wave; b < nq; b += KNN_WAVES) {
    volatile KnnEntry* dst = s_list + b * CAP;
    int dn = s_cnt[b];
    float ts = -INFINITY;
    int ti = INT_MAX;
    if (dn == k) { ts = dst[k - 1].s; ti = dst[k - 1].i; }
    for (int w = 1; w < KNN_WAVES; ++w) {
      const KnnEntry* src = s_list + (w * QB + b) * CAP;
      const int sn = s_cnt[w * QB + b];
      for (int c0 = 0; c0 < sn; c0 += 16) {          // 16 at a time: k + 16 <= CAP, so a compacted list has the room
        if (dn + 16 > CAP) knn_wave_compact(dst, k, lane, dn, ts, ti);
        const bool in = lane < 16 && c0 + lane < sn;
        const float cs = in ? src[c0 + lane].s : -INFINITY;
        const int ci = in ? src[c0 + lane].i : INT_MAX;
        knn_wave_offer<CAP>(dst, lane, 0, ~0ull, in, cs, ci, dn, ts, ti);
      }
    }
    knn_wave_compact(dst, k, lane, dn, ts, ti);
    if (lane < k) {
      const int64_t o = ((int64_t)(q0 + b) * n_slabs + slab) * k + lane;
      cand_s[o] = lane < dn ? dst[lane].s : -INFINITY;
      cand_i[o] = lane < dn ? dst[lane].i : INT_MAX;
    }
  }
}

// one workgroup per query: candidates [n_lists][k] -> idx / score [k], descending score, ties to the lower row index
// grid (groups, B): group g of query q reduces lists [g * per_group, ..) to k entries at out[(q * groups + g) * k]; one group = the final order
__global__ void __launch_bounds__(512) knn_merge_kernel(const float* __restrict__ cand_s, const int* __restrict__ cand_i, int n_lists, int per_group,
                                                        int k, int* __restrict__ idx_out, float* __restrict__ score_out) {
  constexpr int CAP = 128;
  __shared__ KnnEntry s_list[KNN_WAVES * CAP];
  __shared__ int s_cnt[KNN_WAVES];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = blockIdx.y, g = blockIdx.x;
  const int l0 = g * per_group;
  const int total = (n_lists - l0 < per_group ? n_lists - l0 : per_group) * k;
  const float* cs = cand_s + ((int64_t)q * n_lists + l0) * k;
  const int* ci = cand_i + ((int64_t)q * n_lists + l0) * k;
  volatile KnnEntry* mine = s_list + wave * CAP;
  float ts = -INFINITY;
  int ti = INT_MAX, n = 0;
  for (int c0 = wave * 64; c0 < total; c0 += KNN_WAVES * 64) {
    const int c = c0 + lane;
    const bool in = c < total;
    const float s = in ? cs[c] : -INFINITY;
    const int i = in ? ci[c] : INT_MAX;
    if (n + 64 > CAP) knn_wave_compact(mine, k, lane, n, ts, ti);       // (k <= 64: a compacted list has room for 64 more)
    knn_wave_offer<CAP>(mine, lane, 0, ~0ull, in && i != INT_MAX, s, i, n, ts, ti);
  }
  knn_wave_compact(mine, k, lane, n, ts, ti);
  if (lane == 0) s_cnt[wave] = n;
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < KNN_WAVES; ++w) {
    const int sn = s_cnt[w];
    const bool in = lane < sn;
    const float s = in ? s_list[w * CAP + lane].s : -INFINITY;
    const int i = in ? s_list[w * CAP + lane].i : INT_MAX;
    if (n + 64 > CAP) knn_wave_compact(mine, k, lane, n, ts, ti);
    knn_wave_offer<CAP>(mine, lane, 0, ~0ull, in, s, i, n, ts, ti);
  }
  knn_wave_compact(mine, k, lane, n, ts, ti);       // sorted: position = rank
  if (lane < k) {
    const int64_t o = ((int64_t)q * gridDim.x + g) * k + lane;
    idx_out[o] = lane < n ? mine[lane].i : INT_MAX;
    score_out[o] = lane < n ? mine[lane].s : -INFINITY;
  }
}

// grid (k + (c0 != null), B): out row b * (k + has_c0) + slot, at pitch ldo floats
__global__ void __launch_bounds__(256) knn_gather_kernel(const float* __restrict__ db, const float* __restrict__ inv_norm, int64_t N, int D,
                                                         const int* __restrict__ idx, int k, const float* __restrict__ c0, float* __restrict__ out,
                                                         int64_t ldo) {
  const int b = blockIdx.y, slot = blockIdx.x, has = c0 != nullptr ? 1 : 0;
  const int c = threadIdx.x;
  if (c >= (D >> 2)) return;
  f32x4 v;
  if (slot < has) {
    v = ((const f32x4*)(c0 + (int64_t)b * D))[c];
  } else {
    const int64_t i = idx[(int64_t)b * k + (slot - has)];
    if (i < 0 || i >= N) {
      v = f32x4{0.f, 0.f, 0.f, 0.f};       // (an index the merge never writes for k <= N; nothing outside the database is read)
    } else {
      const float s = inv_norm[i];
      const f32x4 x = ((const f32x4*)(db + i * D))[c];
      v = f32x4{x[0] * s, x[1] * s, x[2] * s, x[3] * s};
    }
  }
  ((f32x4*)(out + ((int64_t)b * (k + has) + slot) * ldo))[c] = v;
}

// a plain 16-byte read-only sweep of n4 float4s: the bandwidth ceiling the scan is measured against (tools/bench_knn.py)
__global__ void __launch_bounds__(256) knn_stream_kernel(const f32x4* __restrict__ p, int64_t n4, float* __restrict__ sink) {
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  const int64_t stride = (int64_t)gridDim.x * 256;
#pragma unroll 8
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const f32x4 v = p[i];
    a[0] += v[0]; a[1] += v[1]; a[2] += v[2]; a[3] += v[3];
  }
  const float t = (a[0] + a[1]) + (a[2] + a[3]);
  if (t == 1.2345678e-30f) sink[0] = t;          // (keeps the loads alive; practically never stores)
}

inline bool knn_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int QB>
void knn_launch_scan(int J, dim3 grid, hipStream_t s, const float* db, const float* inv_norm, const float* q, float* cs, int* ci, int64_t N, int D,
                     int B, int k, int64_t slab_rows, int n_slabs) {
  switch (J) {
    case 1: SDMI_LAUNCH((knn_scan_kernel<QB, 1>), grid, dim3(512), 0, s, db, inv_norm, q, cs, ci, N, D, B, k, slab_rows, n_slabs); break;
    case 2: SDMI_LAUNCH((knn_scan_kernel<QB, 2>), grid, dim3(512), 0, s, db, inv_norm, q, cs, ci, N, D, B, k, slab_rows, n_slabs); break;
    case 3: SDMI_LAUNCH((knn_scan_kernel<QB, 3>), grid, dim3(512), 0, s, db, inv_norm, q, cs, ci, N, D, B, k, slab_rows, n_slabs); break;
    default: SDMI_LAUNCH((knn_scan_kernel<QB, 4>), grid, dim3(512), 0, s, db, inv_norm, q, cs, ci, N, D, B, k, slab_rows, n_slabs); break;
  }
}

}  // namespace

int knn_check_args(int64_t N, int D, int B, int k) {
  SDMI_CHECK(D >= 4 && D % 4 == 0 && D <= KNN_MAXD, "knn: D = " + std::to_string(D) + " must be a multiple of 4, at most 1024");
  SDMI_CHECK(N >= 1 && N <= INT_MAX, "knn: the database holds " + std::to_string(N) + " rows; 1 .. 2^31 - 1 are supported");
  SDMI_CHECK(B >= 1 && B <= KNN_MAXB, "knn: B = " + std::to_string(B) + " queries; 1 .. 64 are supported");
  SDMI_CHECK(k >= 1 && k <= KNN_MAXK, "knn: k = " + std::to_string(k) + " neighbours; 1 .. 64 are supported");
  SDMI_CHECK(k <= N, "knn: k = " + std::to_string(k) + " exceeds the " + std::to_string(N) + " rows of the database");
  return 0;
}

int64_t knn_default_slab_rows(int64_t N) {      // about 512 slabs, whole wave steps
  const int64_t step = KNN_WAVES * KNN_R;
  return round_up(std::max<int64_t>(step, (N + 511) / 512), step);
}

int launch_knn_inv_norm(const float* db, int64_t N, int D, float* inv_norm, hipStream_t s) {
  SDMI_CHECK(db && inv_norm && N >= 1 && N <= INT_MAX && D >= 4 && D % 4 == 0 && D <= KNN_MAXD, "knn_inv_norm: bad arguments (D % 4, D <= 1024)");
  SDMI_CHECK(knn_al16(db), "knn_inv_norm: the database must be 16-byte aligned");
  ProfScope ps("knn_inv_norm", 2.0 * N * D, (double)N * D * 4.0, s);
  SDMI_LAUNCH(knn_inv_norm_kernel, dim3((unsigned)((N + KNN_WAVES - 1) / KNN_WAVES)), dim3(512), 0, s, db, inv_norm, N, D);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_knn_first_bad(const float* inv_norm, int64_t N, long long* out, hipStream_t s) {
  SDMI_CHECK(inv_norm && out && N >= 1, "knn_first_bad: bad arguments");
  SDMI_LAUNCH(knn_first_bad_kernel, dim3(1), dim3(1024), 0, s, inv_norm, N, out);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_knn_stream_read(const float* p, int64_t n_floats, float* sink, hipStream_t s) {
  SDMI_CHECK(p && sink && n_floats >= 4 && n_floats % 4 == 0 && knn_al16(p), "knn_stream_read: a 16-byte aligned buffer of whole float4s");
  ProfScope ps("knn_stream_read", 0.0, (double)n_floats * 4.0, s);
  SDMI_LAUNCH(knn_stream_kernel, dim3(256 * 8), dim3(256), 0, s, (const f32x4*)p, n_floats / 4, sink);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_knn_scan(const float* db, const float* inv_norm, int64_t N, int D, const float* queries, int B, int k, int64_t slab_rows, float* cand_s,
                    int* cand_i, hipStream_t s) {
  if (knn_check_args(N, D, B, k)) return -1;
  SDMI_CHECK(db && inv_norm && queries && cand_s && cand_i, "knn_scan: null operand");
  SDMI_CHECK(slab_rows >= 1, "knn_scan: slab_rows must be positive");
  SDMI_CHECK(knn_al16(db) && knn_al16(queries), "knn_scan: the database and the queries must be 16-byte aligned");
  const int64_t n_slabs = (N + slab_rows - 1) / slab_rows;
  SDMI_CHECK(n_slabs <= 65535, "knn_scan: " + std::to_string(n_slabs) + " slabs; at most 65535 per launch");
  // queries per workgroup: the smallest of 1, 4, 8, 16 that holds B (16 and several chunks beyond that): one pass over the database per chunk
  const int QB = B <= 1 ? 1 : B <= 4 ? 4 : B <= 8 ? 8 : 16;
  const int chunks = (B + QB - 1) / QB, J = (D / 4 + 63) / 64;
  ProfScope ps("knn_scan", 2.0 * N * D * B, (double)N * D * 4.0 * chunks, s);
  const dim3 grid((unsigned)n_slabs, (unsigned)chunks);
  if (QB == 1) knn_launch_scan<1>(J, grid, s, db, inv_norm, queries, cand_s, cand_i, N, D, B, k, slab_rows, (int)n_slabs);
  else if (QB == 4) knn_launch_scan<4>(J, grid, s, db, inv_norm, queries, cand_s, cand_i, N, D, B, k, slab_rows, (int)n_slabs);
  else if (QB == 8) knn_launch_scan<8>(J, grid, s, db, inv_norm, queries, cand_s, cand_i, N, D, B, k, slab_rows, (int)n_slabs);
  else knn_launch_scan<16>(J, grid, s, db, inv_norm, queries, cand_s, cand_i, N, D, B, k, slab_rows, (int)n_slabs);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_knn_merge(const float* cand_s, const int* cand_i, int B, int n_lists, int k, int* idx_out, float* score_out, hipStream_t s,
                     int per_group) {
  SDMI_CHECK(cand_s && cand_i && idx_out && score_out, "knn_merge: null operand");
  SDMI_CHECK(B >= 1 && B <= KNN_MAXB && k >= 1 && k <= KNN_MAXK && n_lists >= 1 && n_lists <= 65535, "knn_merge: 1 <= B <= 64, 1 <= k <= 64, 1 <= lists <= 65535");
  if (per_group <= 0 || per_group > n_lists) per_group = n_lists;
  const int groups = (n_lists + per_group - 1) / per_group;
  ProfScope ps("knn_merge", 0.0, (double)B * n_lists * k * 8.0, s);
  SDMI_LAUNCH(knn_merge_kernel, dim3(groups, B), dim3(512), 0, s, cand_s, cand_i, n_lists, per_group, k, idx_out, score_out);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_knn_gather(const float* db, const float* inv_norm, int64_t N, int D, const int* idx, int B, int k, const float* c0, float* out,
                      int64_t ldo, hipStream_t s) {
  if (knn_check_args(N, D, B, k)) return -1;
  SDMI_CHECK(db && inv_norm && idx && out, "knn_gather: null operand");
  SDMI_CHECK(ldo >= D && ldo % 4 == 0, "knn_gather: the output pitch must be a multiple of 4 floats, at least D");
  SDMI_CHECK(knn_al16(db) && knn_al16(out) && (!c0 || knn_al16(c0)), "knn_gather: operands must be 16-byte aligned");
  ProfScope ps("knn_gather", 0.0, (double)B * k * D * 8.0, s);
  SDMI_LAUNCH(knn_gather_kernel, dim3(k + (c0 ? 1 : 0), B), dim3(256), 0, s, db, inv_norm, N, D, idx, k, c0, out, ldo);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

// ---- the sdmi_knn handle: the raw rows once, plus one inverse norm per row ---------------------------------------------------------
Knn::~Knn() {
  if (db_) (void)hipFree(db_);
  if (inv_norm_) (void)hipFree(inv_norm_);
  if (first_bad_) (void)hipFree(first_bad_);
}

int Knn::build(int D, int64_t capacity) {
  SDMI_CHECK(D >= 4 && D % 4 == 0 && D <= KNN_MAXD, "knn: D = " + std::to_string(D) + " must be a multiple of 4, at most 1024");
  SDMI_CHECK(capacity >= 1 && capacity <= INT_MAX, "knn: capacity of " + std::to_string(capacity) + " rows; 1 .. 2^31 - 1 are supported");
  D_ = D; cap_ = capacity;
  size_t free_b = 0, total_b = 0;
  SDMI_HIP_OK(hipMemGetInfo(&free_b, &total_b));
  const int64_t need = capacity * ((int64_t)D + 1) * 4;
  SDMI_CHECK(need <= (int64_t)free_b, "knn: the database needs " + std::to_string(need) + " bytes of device memory, " + std::to_string(free_b) +
                                          " bytes are free");
  SDMI_HIP_OK(hipMalloc((void**)&db_, (size_t)capacity * D * sizeof(float)));
  SDMI_HIP_OK(hipMalloc((void**)&inv_norm_, (size_t)capacity * sizeof(float)));
  SDMI_HIP_OK(hipMalloc((void**)&first_bad_, sizeof(long long)));
  return 0;
}

int Knn::set_rows(int64_t first_row, int64_t n, const float* rows, hipStream_t s) {
  SDMI_CHECK(rows != nullptr, "knn_set_rows: rows is NULL");
  SDMI_CHECK(first_row >= 0 && n >= 1 && first_row + n <= cap_, "knn_set_rows: rows " + std::to_string(first_row) + " .. " +
                                                                      std::to_string(first_row + n) + " exceed the capacity of " +
                                                                      std::to_string(cap_) + " rows");
  SDMI_CHECK(first_row <= n_, "knn_set_rows: rows " + std::to_string(n_) + " .. " + std::to_string(first_row) + " would be left unset");
  SDMI_HIP_OK(hipMemcpyAsync(db_ + first_row * D_, rows, (size_t)n * D_ * sizeof(float), hipMemcpyDefault, s));
  n_ = std::max(n_, first_row + n);
  finalized_ = false;
  return 0;
}

int Knn::finalize(hipStream_t s) {
  SDMI_CHECK(n_ >= 1, "knn_finalize: no rows have been set");
  if (launch_knn_inv_norm(db_, n_, D_, inv_norm_, s)) return -1;
  if (launch_knn_first_bad(inv_norm_, n_, first_bad_, s)) return -1;
  long long bad = -1;
  SDMI_HIP_OK(hipMemcpyAsync(&bad, first_bad_, sizeof(bad), hipMemcpyDeviceToHost, s));
  SDMI_HIP_OK(hipStreamSynchronize(s));
  SDMI_CHECK(bad < 0, "knn_finalize: row " + std::to_string(bad) + " has a zero or non-finite norm (the first such row)");
  finalized_ = true;
  return 0;
}

// the merge runs in two stages above this many slabs: groups of KNN_MERGE_GROUP lists first (one workgroup each), then the group results
constexpr int KNN_MERGE_GROUP = 32;

int64_t Knn::workspace_bytes(int B, int k) const {
  const int64_t slab = knn_default_slab_rows(n_ > 0 ? n_ : 1), n_slabs = ((n_ > 0 ? n_ : 1) + slab - 1) / slab;
  const int64_t groups = (n_slabs + KNN_MERGE_GROUP - 1) / KNN_MERGE_GROUP;
  return round_up((int64_t)B * (n_slabs + groups) * k * 8, 256) + 256;
}

int Knn::search(const float* queries, int B, int k, int* idx_out, float* score_out, float* nn_out, const float* c0, void* workspace,
                int64_t ws_bytes, hipStream_t s) {
  SDMI_CHECK(finalized_, "sdmi_knn_finalize() has not succeeded yet");
  if (knn_check_args(n_, D_, B, k)) return -1;
  SDMI_CHECK(queries && idx_out && score_out, "knn_search: queries / idx_out / score_out is NULL");
  SDMI_CHECK(!c0 || nn_out, "knn_search: the conditioning form needs an output");
  const int64_t need = workspace_bytes(B, k);
  SDMI_CHECK(workspace != nullptr && ws_bytes >= need, "knn_search: workspace too small: need " + std::to_string(need) + " bytes, got " +
                                                           std::to_string(ws_bytes));
  SDMI_CHECK(knn_al16(workspace), "knn_search: the workspace must be 16-byte aligned");
  const int64_t slab = knn_default_slab_rows(n_), n_slabs = (n_ + slab - 1) / slab;
  const int64_t groups = (n_slabs + KNN_MERGE_GROUP - 1) / KNN_MERGE_GROUP;
  float* cand_s = (float*)workspace;
  int* cand_i = (int*)(cand_s + (size_t)B * n_slabs * k);
  float* grp_s = (float*)(cand_i + (size_t)B * n_slabs * k);
  int* grp_i = (int*)(grp_s + (size_t)B * groups * k);
  if (launch_knn_scan(db_, inv_norm_, n_, D_, queries, B, k, slab, cand_s, cand_i, s)) return -1;
  if (groups > 2) {       // [B][n_slabs][k] -> [B][groups][k] -> [B][k]: the same order either way (a total order has one top k)
    if (launch_knn_merge(cand_s, cand_i, B, (int)n_slabs, k, grp_i, grp_s, s, KNN_MERGE_GROUP)) return -1;
    if (launch_knn_merge(grp_s, grp_i, B, (int)groups, k, idx_out, score_out, s, 0)) return -1;
  } else if (launch_knn_merge(cand_s, cand_i, B, (int)n_slabs, k, idx_out, score_out, s, 0)) {
    return -1;
  }
  if (nn_out && launch_knn_gather(db_, inv_norm_, n_, D_, idx_out, B, k, c0, nn_out, D_, s)) return -1;
  return 0;
}

}  // namespace sdmi
