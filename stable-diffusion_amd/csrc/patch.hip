// The sliding-window mechanism of LatentDiffusion.split_input_params (ldm/models/diffusion/ddpm.py:601-651, 715-752, 826-858, 902-984):
//   * patch_unfold_kernel: torch.nn.Unfold(kernel_size, stride) of an fp32 NCHW tensor x (and of a second one, c, behind it on the channel
//     axis: the torch.cat([x] + c_concat, 1) of DiffusionWrapper.forward, ddpm.py:1411-1413) for a range of windows, written as the rows
//     (window, sample) of one NCHW batch -- what the reference gets from unfold().view(...)[:, :, :, :, i] one window at a time.
//   * patch_fold_kernel: fold(o * weighting) / fold(weighting) in gather form: one thread per output element (or per four of them along x)
//     visits the windows that cover it in ascending window index, so there are no atomics and the order of the sum is fixed.
// Both are memory movement: the 16-byte path is taken when every row start it touches is 16-byte aligned (chosen by the launcher).
#include "common.h"
#include "prof.h"

namespace sdmi {
namespace {

// (the reference rounds o * weighting before fold adds it: no contraction into FMAs)
#pragma clang fp contract(off)

template <int V> struct Vec;
template <> struct Vec<1> { using T = float; };
template <> struct Vec<4> { using T = float4; };

// one thread per V consecutive output elements of a window row; n = nl * B * (Cx + Cc) * kh * (kw / V)
template <int V>
__global__ void __launch_bounds__(256) patch_unfold_kernel(const float* __restrict__ x, const float* __restrict__ c, float* __restrict__ out,
                                                           int B, int Cx, int Cc, int H, int W, int kh, int kw, int sy, int sx, int Lx,
                                                           int l0, int64_t n) {
  using T = typename Vec<V>::T;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int kwv = kw / V, C = Cx + Cc;
  const int xx = (int)(i % kwv) * V;
  int64_t r = i / kwv;
  const int yy = (int)(r % kh);
  r /= kh;
  const int ch = (int)(r % C);
  r /= C;                                       // output row (l - l0) * B + b
  const int b = (int)(r % B);
  const int l = l0 + (int)(r / B);
  const int y = (l / Lx) * sy + yy, xs = (l % Lx) * sx + xx;
  const float* src = ch < Cx ? x + ((size_t)b * Cx + ch) * H * W : c + ((size_t)b * Cc + (ch - Cx)) * H * W;
  *(T*)(out + i * V) = *(const T*)(src + (size_t)y * W + xs);
}

// one thread per V consecutive output elements along x; n = B * C * Ho * (Wo / V).  o [L * B][C][kh][kw] (row l * B + b), w [L][kh][kw].
// V == 4: kw, sx, Wo are multiples of 4, so an aligned quad lies inside or outside a window as a whole.
template <int V>
__global__ void __launch_bounds__(256) patch_fold_kernel(const float* __restrict__ o, const float* __restrict__ w, float* __restrict__ out,
                                                         int B, int C, int Ho, int Wo, int kh, int kw, int sy, int sx, int Ly, int Lx,
                                                         int norm_only, int64_t n) {
  using T = typename Vec<V>::T;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int wov = Wo / V;
  const int x = (int)(i % wov) * V;
  int64_t r = i / wov;
  const int y = (int)(r % Ho);
  r /= Ho;
  const int ch = (int)(r % C);
  const int b = (int)(r / C);
  // windows ly with ly * sy <= y < ly * sy + kh
  const int ly1 = min(Ly - 1, y / sy), ly0 = y < kh ? 0 : (y - kh) / sy + 1;
  const int lx1 = min(Lx - 1, x / sx), lx0 = x < kw ? 0 : (x - kw) / sx + 1;
  float acc[V], den[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f, den[j] = 0.f;
  for (int ly = ly0; ly <= ly1; ++ly) {
    for (int lx = lx0; lx <= lx1; ++lx) {
      const int l = ly * Lx + lx;
      const size_t off = (size_t)(y - ly * sy) * kw + (x - lx * sx);
      const T wv = *(const T*)(w + (size_t)l * kh * kw + off);
      const float* wp = (const float*)&wv;
      if (norm_only) {
#pragma unroll
        for (int j = 0; j < V; ++j) den[j] = den[j] + wp[j];
      } else {
        const T ov = *(const T*)(o + (((size_t)l * B + b) * C + ch) * kh * kw + off);
        const float* op = (const float*)&ov;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          acc[j] = acc[j] + wp[j] * op[j];
          den[j] = den[j] + wp[j];
        }
      }
    }
  }
  T res;
  float* rp = (float*)&res;
#pragma unroll
  for (int j = 0; j < V; ++j) rp[j] = norm_only ? den[j] : acc[j] / den[j];
  *(T*)(out + i * V) = res;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int launch_patch_unfold(const float* x, const float* c, float* out, int B, int Cx, int Cc, int H, int W, int kh, int kw, int sy, int sx,
                        int l0, int nl, hipStream_t s) {
  SDMI_CHECK(x && out && B >= 1 && Cx >= 1 && Cc >= 0 && (Cc == 0 || c) && H >= 1 && W >= 1 && kh >= 1 && kw >= 1 && sy >= 1 && sx >= 1,
             "patch unfold: bad arguments");
  SDMI_CHECK(kh <= H && kw <= W, "patch unfold: the window is larger than the input");
  SDMI_CHECK((H - kh) % sy == 0 && (W - kw) % sx == 0, "patch unfold: H - kh and W - kw must be multiples of the stride (uncovered pixels)");
  const int Ly = (H - kh) / sy + 1, Lx = (W - kw) / sx + 1;
  SDMI_CHECK(l0 >= 0 && nl >= 1 && (int64_t)l0 + nl <= (int64_t)Ly * Lx, "patch unfold: window range outside [0, Ly * Lx)");
  const bool v4 = W % 4 == 0 && kw % 4 == 0 && sx % 4 == 0 && aligned16(x) && aligned16(out) && (Cc == 0 || aligned16(c));
  const int64_t n = (int64_t)nl * B * (Cx + Cc) * kh * (kw / (v4 ? 4 : 1));
  SDMI_CHECK((n + 255) / 256 <= 0x7fffffff, "patch unfold: too many elements for one launch");
  ProfScope ps("patch_unfold", 0.0, 8.0 * nl * B * (Cx + Cc) * kh * (double)kw, s);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (v4) SDMI_LAUNCH(patch_unfold_kernel<4>, grid, dim3(256), 0, s, x, c, out, B, Cx, Cc, H, W, kh, kw, sy, sx, Lx, l0, n);
  else SDMI_LAUNCH(patch_unfold_kernel<1>, grid, dim3(256), 0, s, x, c, out, B, Cx, Cc, H, W, kh, kw, sy, sx, Lx, l0, n);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

int launch_patch_fold(const float* o, const float* w, float* out, int B, int C, int H, int W, int kh, int kw, int sy, int sx, int uf, int df,
                      int norm_only, hipStream_t s) {
  SDMI_CHECK(w && out && (norm_only || o) && B >= 1 && C >= 1 && H >= 1 && W >= 1 && kh >= 1 && kw >= 1 && sy >= 1 && sx >= 1 && uf >= 1 &&
                 df >= 1, "patch fold: bad arguments");
  SDMI_CHECK(kh <= H && kw <= W, "patch fold: the window is larger than the input");
  SDMI_CHECK((H - kh) % sy == 0 && (W - kw) % sx == 0, "patch fold: H - kh and W - kw must be multiples of the stride (uncovered pixels)");
  SDMI_CHECK(uf == 1 || df == 1, "patch fold: uf > 1 and df > 1 together");
  SDMI_CHECK((uf == 1 && df == 1) || kh == kw, "patch fold: a non-square window with uf != 1 or df != 1 (get_fold_unfold scales kernel_size[0] on both axes)");
  SDMI_CHECK(H % df == 0 && W % df == 0 && kh % df == 0 && kw % df == 0 && sy % df == 0 && sx % df == 0,
             "patch fold: df must divide the input, the window and the stride");
  const int Ly = (H - kh) / sy + 1, Lx = (W - kw) / sx + 1;
  const int Ho = H * uf / df, Wo = W * uf / df, kho = kh * uf / df, kwo = kw * uf / df, syo = sy * uf / df, sxo = sx * uf / df;
  if (norm_only) B = C = 1;
  const bool v4 = Wo % 4 == 0 && kwo % 4 == 0 && sxo % 4 == 0 && aligned16(w) && aligned16(out) && (norm_only || aligned16(o));
  const int64_t n = (int64_t)B * C * Ho * (Wo / (v4 ? 4 : 1));
  SDMI_CHECK((n + 255) / 256 <= 0x7fffffff, "patch fold: too many elements for one launch");
  const double cover = ((double)kho / syo) * ((double)kwo / sxo);
  ProfScope ps("patch_fold", 2.0 * B * C * Ho * (double)Wo * cover, 4.0 * B * C * Ho * (double)Wo * (1.0 + cover), s);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (v4) SDMI_LAUNCH(patch_fold_kernel<4>, grid, dim3(256), 0, s, o, w, out, B, C, Ho, Wo, kho, kwo, syo, sxo, Ly, Lx, norm_only, n);
  else SDMI_LAUNCH(patch_fold_kernel<1>, grid, dim3(256), 0, s, o, w, out, B, C, Ho, Wo, kho, kwo, syo, sxo, Ly, Lx, norm_only, n);
  SDMI_HIP_OK(hipGetLastError());
  return 0;
}

}  // namespace sdmi
