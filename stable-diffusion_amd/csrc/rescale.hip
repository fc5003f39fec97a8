// The conditioning stage of the semantic-synthesis model (models/ldm/semantic_synthesis*/config.yaml): SpatialRescaler with method
// 'bilinear' and multiplier 0.5 -- n_stages halvings of an fp32 NCHW map, then a 1x1 convolution to <= 8 channels -- in one pass
// over the input, and the same result straight from an int32 label map without the one-hot tensor.
//
// Arithmetic (the library's definition; bilinear at scale 0.5 with align_corners=False samples exactly between two pixels):
//   * one stage: out[i][j] = ((a + b) + (c + d)) * 0.25f, a b at row 2i, cols 2j, 2j+1, c d at row 2i+1; every stage rounded to fp32,
//     no contraction; an odd last row or column is never read (sizes H >> n, W >> n)
//   * channel map: out[o] = bias[o] + sum_c w[o][c] p[c] in fp32 (fmaf).  Channels go in chunks of RS_CH to the RS_NW waves of a
//     workgroup round-robin (chunk k -> wave k % RS_NW); a wave sums its channels in ascending order from 0, and the RS_NW wave sums
//     are added to the bias in ascending wave order through LDS.  The tree is a function of Cin alone: no atomics, the same bits
//     whatever B, H, W, the load path or the entry point.
//   * label entry: p[c] = count_c * 2^(-2n) over the pixel's 2^n x 2^n block (exactly what the stages give on a one-hot map: every
//     intermediate is a multiple of 2^(-2n) below 1), every class in ascending order through the same accumulation code.
// One output pixel per lane (flattened over the output map, so narrow maps keep their lanes), RS_NW waves per workgroup splitting
// the channels; RS_U channels' loads are issued before the first is used.  16-byte (n = 2) / 8-byte (n = 1) loads when the rows
// allow it, element loads otherwise: the same expression on the same values.
#include "common.h"
#include "prof.h"
#include "rescale.h"

namespace sdmi {
namespace {

#pragma clang fp contract(off)

constexpr int RS_NW = 8;       // waves per workgroup (channel split)
constexpr int RS_CH = 8;       // channels per chunk
constexpr int RS_U = 4;        // channels in flight per wave
constexpr int RS_MAXO = 8;     // output channels

__device__ __forceinline__ float pool4(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }

// the 2^N x 2^N block at p (row stride W) -> blk[(1 << N) * (1 << N)], row-major
template <int N, bool VEC, typename T>
__device__ __forceinline__ void load_block(const T* __restrict__ p, int W, T* blk) {
  constexpr int S = 1 << N;
  if constexpr (N == 0) {
    blk[0] = p[0];
  } else if constexpr (!VEC) {
#pragma unroll
    for (int r = 0; r < S; ++r)
#pragma unroll
      for (int c = 0; c < S; ++c) blk[r * S + c] = p[(size_t)r * W + c];
  } else if constexpr (N == 1) {
    struct alignas(8) T2 { T a, b; };
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const T2 v = *(const T2*)(p + (size_t)r * W);
      blk[r * 2] = v.a; blk[r * 2 + 1] = v.b;
    }
  } else {
    struct alignas(16) T4 { T a, b, c, d; };
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const T4 v = *(const T4*)(p + (size_t)r * W);
      blk[r * 4] = v.a; blk[r * 4 + 1] = v.b; blk[r * 4 + 2] = v.c; blk[r * 4 + 3] = v.d;
    }
  }
}

template <int N>
__device__ __forceinline__ float pool_block(const float* blk) {
  if constexpr (N == 0) {
    return blk[0];
  } else if constexpr (N == 1) {
    return pool4(blk[0], blk[1], blk[2], blk[3]);
  } else {
    float h[4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        h[i * 2 + j] = pool4(blk[(2 * i) * 4 + 2 * j], blk[(2 * i) * 4 + 2 * j + 1], blk[(2 * i + 1) * 4 + 2 * j], blk[(2 * i + 1) * 4 + 2 * j + 1]);
    return pool4(h[0], h[1], h[2], h[3]);
  }
}

// acc[o] += w[o][c] * p for the RS_MAXO accumulators; rows o >= Cout repeat row Cout - 1 (in bounds, never stored); c is wave-uniform
__device__ __forceinline__ void map_acc(float* acc, const float* __restrict__ w, int Cin, int Cout, int c, float p) {
#pragma unroll
  for (int o = 0; o < RS_MAXO; ++o) acc[o] = __builtin_fmaf(w[(size_t)min(o, Cout - 1) * Cin + c], p, acc[o]);
}

// bias + the RS_NW wave sums in ascending wave order; wave o stores output channel o
__device__ __forceinline__ void map_finish(const float* acc, float (*s_part)[RS_MAXO][64], const float* __restrict__ bias,
                                           float* __restrict__ out, int Cout, int64_t b, int64_t HWo, int64_t pix, bool live, int wave,
                                           int lane) {
#pragma unroll
  for (int o = 0; o < RS_MAXO; ++o) s_part[wave][o][lane] = acc[o];
  __syncthreads();
  if (wave >= Cout || !live) return;
  float r = bias ? bias[wave] : 0.f;
#pragma unroll
  for (int k = 0; k < RS_NW; ++k) r = r + s_part[k][wave][lane];
  out[((size_t)b * Cout + wave) * HWo + pix] = r;
}

template <int N, bool VEC>
__global__ void __launch_bounds__(RS_NW * 64, 4) rescale_map_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, float* __restrict__ out, int Cin,
                                                                    int H, int W, int Cout, int Wo, int64_t HWo, int blocks_per_sample) {
  __shared__ float s_part[RS_NW][RS_MAXO][64];
  constexpr int S = 1 << N;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.x / blocks_per_sample;
  const int64_t pix = (int64_t)(blockIdx.x % blocks_per_sample) * 64 + lane;
  const bool live = pix < HWo;
  const int64_t q = live ? pix : 0;                  // (an idle lane reads pixel 0 and stores nothing)
  const int i = (int)(q / Wo), j = (int)(q - (int64_t)i * Wo);
  const size_t plane = (size_t)H * W;
  const float* xb = x + (size_t)b * Cin * plane;     // wave-uniform; the lane's part of the address is one offset into a plane
  const size_t lane_off = (size_t)i * S * W + (size_t)j * S;
  const float* base = xb + lane_off;
  float acc[RS_MAXO];
#pragma unroll
  for (int o = 0; o < RS_MAXO; ++o) acc[o] = 0.f;
  for (int c0 = wave * RS_CH; c0 < Cin; c0 += RS_NW * RS_CH) {
    const int c1 = min(c0 + RS_CH, Cin);
    int c = c0;
    for (; c + RS_U <= c1; c += RS_U) {
      float blk[RS_U][S * S];
      if constexpr (VEC) {
        // RS_U x S row loads, all issued before the first use: the empty asm reads every row, so no load can sink below it (left to
        // itself the scheduler pairs each channel's loads with its arithmetic: S loads in flight per wave instead of RS_U x S)
        typedef float rowv __attribute__((ext_vector_type(S)));
        rowv r[RS_U][S];
#pragma unroll
        for (int u = 0; u < RS_U; ++u)
#pragma unroll
          for (int k = 0; k < S; ++k)      // (vec_ok: a plane's offsets fit 32 bits)
            r[u][k] = *(const rowv*)(xb + (size_t)(c + u) * plane + (size_t)k * W + (unsigned)lane_off);
        static_assert(RS_U == 4, "the operand list below names RS_U x S rows");
        if constexpr (S == 4)
          asm volatile("" : "+v"(r[0][0]), "+v"(r[0][1]), "+v"(r[0][2]), "+v"(r[0][3]), "+v"(r[1][0]), "+v"(r[1][1]), "+v"(r[1][2]),
                       "+v"(r[1][3]), "+v"(r[2][0]), "+v"(r[2][1]), "+v"(r[2][2]), "+v"(r[2][3]), "+v"(r[3][0]), "+v"(r[3][1]),
                       "+v"(r[3][2]), "+v"(r[3][3]));
        else
          asm volatile("" : "+v"(r[0][0]), "+v"(r[0][1]), "+v"(r[1][0]), "+v"(r[1][1]), "+v"(r[2][0]), "+v"(r[2][1]), "+v"(r[3][0]),
                       "+v"(r[3][1]));
#pragma unroll
        for (int u = 0; u < RS_U; ++u)
#pragma unroll
          for (int k = 0; k < S; ++k)
#pragma unroll
            for (int e = 0; e < S; ++e) blk[u][k * S + e] = r[u][k][e];
      } else {
#pragma unroll
        for (int u = 0; u < RS_U; ++u) load_block<N, false>(base + (size_t)(c + u) * plane, W, blk[u]);
      }
#pragma unroll
      for (int u = 0; u < RS_U; ++u) map_acc(acc, w, Cin, Cout, c + u, pool_block<N>(blk[u]));
    }
    for (; c < c1; ++c) {
      float blk[S * S];
      load_block<N, VEC>(base + (size_t)c * plane, W, blk);
      map_acc(acc, w, Cin, Cout, c, pool_block<N>(blk));
    }
  }
  map_finish(acc, s_part, bias, out, Cout, b, HWo, pix, live, wave, lane);
}

template <int N, bool VEC>
__global__ void __launch_bounds__(RS_NW * 64) rescale_labels_kernel(const int* __restrict__ labels, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, float* __restrict__ out, int Cin,
                                                                    int H, int W, int Cout, int Wo, int64_t HWo, int blocks_per_sample) {
  __shared__ float s_part[RS_NW][RS_MAXO][64];
  constexpr int S = 1 << N;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = blockIdx.x / blocks_per_sample;
  const int64_t pix = (int64_t)(blockIdx.x % blocks_per_sample) * 64 + lane;
  const bool live = pix < HWo;
  const int64_t q = live ? pix : 0;
  const int i = (int)(q / Wo), j = (int)(q - (int64_t)i * Wo);
  int lab[S * S];
  load_block<N, VEC>(labels + (size_t)b * H * W + (size_t)i * S * W + (size_t)j * S, W, lab);
  constexpr float scale = 1.0f / (float)(S * S);
  float acc[RS_MAXO];
#pragma unroll
  for (int o = 0; o < RS_MAXO; ++o) acc[o] = 0.f;
  for (int c0 = wave * RS_CH; c0 < Cin; c0 += RS_NW * RS_CH) {
    const int c1 = min(c0 + RS_CH, Cin);
    for (int c = c0; c < c1; ++c) {
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < S * S; ++k) cnt += lab[k] == c ? 1 : 0;
      map_acc(acc, w, Cin, Cout, c, (float)cnt * scale);
    }
  }
  map_finish(acc, s_part, bias, out, Cout, b, HWo, pix, live, wave, lane);
}

// no channel_mapper: every plane pooled on its own, one thread per output element
template <int N, bool VEC>
__global__ void __launch_bounds__(256) rescale_pool_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int Wo,
                                                           int64_t HWo, int64_t total) {
  constexpr int S = 1 << N;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t pl = e / HWo, q = e - pl * HWo;
    const int i = (int)(q / Wo), j = (int)(q - (int64_t)i * Wo);
    float blk[S * S];
    load_block<N, VEC>(x + (size_t)pl * H * W + (size_t)i * S * W + (size_t)j * S, W, blk);
    out[e] = pool_block<N>(blk);
  }
}

int check_common(const void* in, const float* w, const float* bias, const float* out, int B, int Cin, int H, int W, int n, int Cout) {
  SDMI_CHECK(in && out, "spatial_rescale: null input or output");
  SDMI_CHECK(n >= 0 && n <= 2, "spatial_rescale: n_stages 0 .. 2");
  SDMI_CHECK(B >= 1 && Cin >= 1, "spatial_rescale: B >= 1 and Cin >= 1");
  SDMI_CHECK(!w || (Cout >= 1 && Cout <= RS_MAXO), "spatial_rescale: 1 .. 8 output channels");
  SDMI_CHECK(w || !bias, "spatial_rescale: a bias needs the channel map's weight");
  SDMI_CHECK(H >= (1 << n) && W >= (1 << n), "spatial_rescale: H and W at least 2^n_stages");
  return 0;
}

bool vec_ok(const void* p, int H, int W, int n) {
  return n >= 1 && W % (1 << n) == 0 && ((uintptr_t)p & 15) == 0 && (int64_t)H * W <= (1 << 29);
}

}  // namespace

#define RS_DISPATCH(KERNEL, ...)                                                                       \
  do {                                                                                                 \
    if (n == 0) SDMI_LAUNCH((KERNEL<0, false>), __VA_ARGS__);                                          \
    else if (n == 1 && vec) SDMI_LAUNCH((KERNEL<1, true>), __VA_ARGS__);                               \
    else if (n == 1) SDMI_LAUNCH((KERNEL<1, false>), __VA_ARGS__);                                     \
    else if (vec) SDMI_LAUNCH((KERNEL<2, true>), __VA_ARGS__);                                         \
    else SDMI_LAUNCH((KERNEL<2, false>), __VA_ARGS__);                                                 \
  } while (0)

int launch_spatial_rescale(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int H, int W, int n, int Cout,
                           hipStream_t s) {
  if (int r = check_common(x, w, bias, out, B, Cin, H, W, n, Cout)) return r;
  const int Ho = H >> n, Wo = W >> n;
  const int64_t HWo = (int64_t)Ho * Wo;
  const bool vec = vec_ok(x, H, W, n);
  ProfScope ps("spatial_rescale", 0.0, (double)B * Cin * H * W * 4.0, s);
  if (!w) {
    const int64_t total = (int64_t)B * Cin * HWo;
    const dim3 grid((unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32));
    RS_DISPATCH(rescale_pool_kernel, grid, dim3(256), 0, s, x, out, H, W, Wo, HWo, total);
  } else {
    const int64_t bps = (HWo + 63) / 64;
    SDMI_CHECK(bps * B <= 0x7fffffff, "spatial_rescale: too many output pixels for one launch");
    RS_DISPATCH(rescale_map_kernel, dim3((unsigned)(bps * B)), dim3(RS_NW * 64), 0, s, x, w, bias, out, Cin, H, W, Cout, Wo, HWo,
                (int)bps);
  }
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_spatial_rescale_labels(const int* labels, const float* w, const float* bias, float* out, int B, int Cin, int H, int W, int n,
                                  int Cout, hipStream_t s) {
  if (int r = check_common(labels, w, bias, out, B, Cin, H, W, n, Cout)) return r;
  SDMI_CHECK(w, "spatial_rescale_labels: the channel map's weight (the pooled one-hot map alone has no label entry)");
  const int Ho = H >> n, Wo = W >> n;
  const int64_t HWo = (int64_t)Ho * Wo;
  const bool vec = vec_ok(labels, H, W, n);
  const int64_t bps = (HWo + 63) / 64;
  SDMI_CHECK(bps * B <= 0x7fffffff, "spatial_rescale_labels: too many output pixels for one launch");
  ProfScope ps("spatial_rescale_labels", 0.0, (double)B * H * W * 4.0, s);
  RS_DISPATCH(rescale_labels_kernel, dim3((unsigned)(bps * B)), dim3(RS_NW * 64), 0, s, labels, w, bias, out, Cin, H, W, Cout, Wo, HWo,
              (int)bps);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace sdmi
