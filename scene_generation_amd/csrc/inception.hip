// The Inception score (scene_generation_amd/inception.py): what torchvision's Inception-v3 and scripts/inception_score.py of the
// reference need beyond the entry points that already exist.
//
//   sg_conv2d_rect_fwd      forward convolution with a KH x KW kernel and separate padH / padW (1x7, 7x1, 1x3, 3x1, 5x5 and the square
//                           ones), bias + activation fused, written into a channel slice of a wider NCHW tensor: the implicit GEMM of
//                           igemm_core.h (fp32 MFMA) with a rectangular gather loader; the existing EpNCHW epilogue already takes a
//                           total channel count, so a slice is its ``out`` pointer moved by out_c0 planes
//   sg_maxpool3s2v_fwd      max_pool2d(3, stride=2) without padding, into a channel slice
//   sg_avgpool3s1_fwd       avg_pool2d(3, stride=1, padding=1), count_include_pad=True
//   sg_avgpool3s1x_fwd      the same with count_include_pad=False, and
//   sg_maxpool3s1_fwd       max_pool2d(3, stride=1, padding=1): the branch pools of the FID form of the network
//   sg_resize_bilinear_fwd  F.interpolate(mode='bilinear', align_corners=False)
//   sg_softmax_rows         softmax of logits rows into a row window of a caller-owned buffer
//   sg_inception_score      exp(mean KL(p(y|x) || p(y))) per split, mean and population std over the splits, in fp64
//
// Forward only, fp32 (the score in fp64).  No float atomics and no float sum whose order depends on the launch: every result is
// bit-identical from run to run.
#include "igemm_core.h"
#include "rect_gather.h"
#include <math.h>

namespace {

constexpr int TPB = 256;
constexpr int WPB = TPB / SG_WAVE;
constexpr int RECT_MAX_TAPS = 25;          // 5x5 is the largest kernel of the network
template <int BN> using RectGather = LoadGatherRect<BN, RECT_MAX_TAPS>;      // (rect_gather.h)

__device__ __forceinline__ bool is_nan(float v) { return v != v; }

// ---- the launch plan ------------------------------------------------------------------------------------------------------------
// tile: 32 rows x 128 pixels for the convs of at most 32 output channels (the first two of the stem); 64 x 128 when that still gives
// three workgroups per compute unit (the library's measured threshold for the square gathers: twice the MFMAs per gathered element of
// 64 x 64); 64 x 64 otherwise.  vec: 16-byte loads of the weight rows (K % 4 == 0 and an aligned base).  splits: the reduction cut
// into k-chunks of whole k-tiles, at least 256 deep, when the tiles alone leave compute units idle (the 8 x 8 blocks: K = 1280 / 2048
// over 64 pixels per image); the chunks are written as slabs and added in order by rect_reduce_kernel.
inline RectPlan rect_plan(const sgRectDesc* d, bool w16) {
  const RectDims n(d);
  RectPlan p;
  p.vec = (n.K % 4 == 0 && w16) ? 1 : 0;
  if (n.M <= 32) { p.tile = SG_RECT_TILE_32X128; p.bm = 32; p.bn = 128; }
  else if ((long)sg_cdiv(n.M, 64) * sg_cdiv(n.Npix, 128) >= 768) { p.tile = SG_RECT_TILE_64X128; p.bm = 64; p.bn = 128; }
  else { p.tile = SG_RECT_TILE_64X64; p.bm = 64; p.bn = 64; }
  rect_plan_splits(p, n.M, n.K, n.Npix);
  return p;
}

inline bool rect_desc_ok(const sgRectDesc* d) { return rect_desc_ok(d, RECT_MAX_TAPS, RECT_MAX_TAPS, RECT_MAX_TAPS, 2); }

// ---- max_pool2d(3, stride=2), no padding ------------------------------------------------------------------------------------------
// torch's scan: rows then columns of the window, from -inf, taking a value when it is greater than the running maximum or a NaN
__global__ void __launch_bounds__(TPB) maxpool3s2v_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned total, int C,
                                                         int H, int W, int OH, int OW, int c0, int ctot, FastDiv fow, FastDiv foh,
                                                         FastDiv fc) {
  const unsigned i = blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const unsigned r = fow.div(i), ow = i - r * (unsigned)OW;
  const unsigned nc = foh.div(r), oh = r - nc * (unsigned)OH;
  const unsigned n = fc.div(nc), c = nc - n * (unsigned)C;
  const float* xp = x + (size_t)nc * H * W + (size_t)(2 * oh) * W + 2 * ow;
  float m = -__builtin_inff();
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const float v = xp[kh * W + kw];
      if (v > m || is_nan(v)) m = v;
    }
  y[(((size_t)n * ctot + c0 + c) * OH + oh) * OW + ow] = m;
}

// ---- avg_pool2d(3, stride=1, padding=1), count_include_pad=True ---------------------------------------------------------------------
// the taps inside the plane are added in (kh, kw) order -- rows, then columns -- starting from 0; the sum is divided by 9
__global__ void __launch_bounds__(TPB) avgpool3s1_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned total, int H, int W,
                                                        FastDiv fw, FastDiv fh) {
  const unsigned i = blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const unsigned r = fw.div(i), w = i - r * (unsigned)W;
  const unsigned nc = fh.div(r), h = r - nc * (unsigned)H;
  const float* xp = x + (size_t)nc * H * W;
  float sum = 0.f;
#pragma unroll
  for (int kh = -1; kh <= 1; ++kh) {
    const int ih = (int)h + kh;
    if (ih < 0 || ih >= H) continue;
#pragma unroll
    for (int kw = -1; kw <= 1; ++kw) {
      const int iw = (int)w + kw;
      if (iw < 0 || iw >= W) continue;
      sum += xp[ih * W + iw];
    }
  }
  y[i] = sum / 9.f;
}

// ---- avg_pool2d(3, stride=1, padding=1), count_include_pad=False (the FID form of the network) ----------------------------------------
// the same taps in the same order as avgpool3s1_kernel; the divisor is the number of taps inside the plane
__global__ void __launch_bounds__(TPB) avgpool3s1x_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned total, int H, int W,
                                                         FastDiv fw, FastDiv fh) {
  const unsigned i = blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const unsigned r = fw.div(i), w = i - r * (unsigned)W;
  const unsigned nc = fh.div(r), h = r - nc * (unsigned)H;
  const float* xp = x + (size_t)nc * H * W;
  float sum = 0.f;
  int taps = 0;
#pragma unroll
  for (int kh = -1; kh <= 1; ++kh) {
    const int ih = (int)h + kh;
    if (ih < 0 || ih >= H) continue;
#pragma unroll
    for (int kw = -1; kw <= 1; ++kw) {
      const int iw = (int)w + kw;
      if (iw < 0 || iw >= W) continue;
      sum += xp[ih * W + iw];
      ++taps;
    }
  }
  y[i] = sum / (float)taps;
}

// ---- max_pool2d(3, stride=1, padding=1) (the FID form of the network) ------------------------------------------------------------------
// the scan of maxpool3s2v_kernel over the taps inside the plane (the padding is -inf: it never wins)
__global__ void __launch_bounds__(TPB) maxpool3s1_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned total, int H, int W,
                                                        FastDiv fw, FastDiv fh) {
  const unsigned i = blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const unsigned r = fw.div(i), w = i - r * (unsigned)W;
  const unsigned nc = fh.div(r), h = r - nc * (unsigned)H;
  const float* xp = x + (size_t)nc * H * W;
  float m = -__builtin_inff();
#pragma unroll
  for (int kh = -1; kh <= 1; ++kh) {
    const int ih = (int)h + kh;
    if (ih < 0 || ih >= H) continue;
#pragma unroll
    for (int kw = -1; kw <= 1; ++kw) {
      const int iw = (int)w + kw;
      if (iw < 0 || iw >= W) continue;
      const float v = xp[ih * W + iw];
      if (v > m || is_nan(v)) m = v;
    }
  }
  y[i] = m;
}

// ---- F.interpolate(mode='bilinear', align_corners=False) ----------------------------------------------------------------------------
// src = (dst + 0.5) * in / out - 0.5, clamped below at 0; the upper tap is clamped to the last row / column.  The coordinate is
// computed in fp64 and the weights rounded to fp32 once.
__device__ __forceinline__ void bilinear_axis(unsigned o, int in, int out, int& i0, int& i1, float& l0, float& l1) {
  double src = ((double)o + 0.5) * ((double)in / (double)out) - 0.5;
  src = src < 0.0 ? 0.0 : src;
  i0 = (int)src;
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 < in - 1 ? i0 + 1 : i0;
  l1 = (float)(src - (double)i0);
  l0 = 1.f - l1;
}

__global__ void __launch_bounds__(TPB) resize_bilinear_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned total, int H,
                                                             int W, int OH, int OW, FastDiv fow, FastDiv foh) {
  const unsigned i = blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const unsigned r = fow.div(i), ow = i - r * (unsigned)OW;
  const unsigned nc = foh.div(r), oh = r - nc * (unsigned)OH;
  int h0, h1, w0, w1;
  float lh0, lh1, lw0, lw1;
  bilinear_axis(oh, H, OH, h0, h1, lh0, lh1);
  bilinear_axis(ow, W, OW, w0, w1, lw0, lw1);
  const float* xp = x + (size_t)nc * H * W;
  const float a = xp[h0 * W + w0], b = xp[h0 * W + w1], c = xp[h1 * W + w0], d = xp[h1 * W + w1];
  y[i] = lh0 * (lw0 * a + lw1 * b) + lh1 * (lw0 * c + lw1 * d);
}

// ---- softmax rows -----------------------------------------------------------------------------------------------------------------
// a wave per row: the row maximum, e = exp(x - max), p = e / sum(e).  Every lane adds its classes in ascending order and the lanes
// meet in a butterfly, so the sum has one fixed order.
__global__ void __launch_bounds__(TPB) softmax_rows_kernel(const float* __restrict__ logits, float* __restrict__ out, int rows, int classes) {
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, row = blockIdx.x * WPB + wid;
  if (row >= rows) return;                                        // wave-uniform
  const float* lp = logits + (size_t)row * classes;
  float* op = out + (size_t)row * classes;
  float m = -__builtin_inff();
  for (int c = lane; c < classes; c += SG_WAVE) m = fmaxf(m, lp[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float sum = 0.f;
  for (int c = lane; c < classes; c += SG_WAVE) sum += expf(lp[c] - m);
  sum = sg_wave_sum(sum);
  for (int c = lane; c < classes; c += SG_WAVE) op[c] = expf(lp[c] - m) / sum;
}

// ---- the score ----------------------------------------------------------------------------------------------------------------------
// fixed-order fp64 block sum: each thread's partial, then a tree over LDS
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = TPB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// py[k][j] = mean over the rows of part k of p[row][j]; a thread per column walks the rows in ascending order (four running sums
// over rows r % 4, met as (s0 + s1) + (s2 + s3))
__global__ void __launch_bounds__(TPB) score_colmean_kernel(const float* __restrict__ p, double* __restrict__ py, int per, int classes) {
  const int j = blockIdx.x * TPB + threadIdx.x, k = blockIdx.y;
  if (j >= classes) return;
  const float* base = p + (size_t)k * per * classes + j;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int r = 0;
  for (; r + 4 <= per; r += 4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += (double)base[(size_t)(r + e) * classes];
  }
  for (int e = 0; r < per; ++r, ++e) s[e] += (double)base[(size_t)r * classes];
  py[(size_t)k * classes + j] = ((s[0] + s[1]) + (s[2] + s[3])) / (double)per;
}

// kl[row] = sum_j ph log(ph / qh) with ph = p[row] / sum(p[row]), qh = py / sum(py) (scipy.stats.entropy normalises both); a term
// with p = 0 is 0.  A workgroup per row.
__global__ void __launch_bounds__(TPB) score_kl_kernel(const float* __restrict__ p, const double* __restrict__ py, double* __restrict__ kl,
                                                      int per, int classes) {
  __shared__ double red[TPB];
  const int row = blockIdx.x, k = row / per;
  const float* pr = p + (size_t)row * classes;
  const double* q = py + (size_t)k * classes;
  double sp = 0.0, sq = 0.0;
  for (int j = threadIdx.x; j < classes; j += TPB) { sp += (double)pr[j]; sq += q[j]; }
  sp = block_sum_f64(sp, red);
  sq = block_sum_f64(sq, red);
  double acc = 0.0;
  for (int j = threadIdx.x; j < classes; j += TPB) {
    const double a = (double)pr[j] / sp;
    if (a > 0.0) acc += a * log(a / (q[j] / sq));
  }
  acc = block_sum_f64(acc, red);
  if (threadIdx.x == 0) kl[row] = acc;
}

// out = {mean, std, score_0 .. score_{splits-1}}: score_k = exp(mean of the part's kl), mean / population std over the splits
__global__ void __launch_bounds__(TPB) score_final_kernel(const double* __restrict__ kl, double* __restrict__ out, int per, int splits) {
  __shared__ double red[TPB];
  for (int k = 0; k < splits; ++k) {
    double s = 0.0;
    for (int r = threadIdx.x; r < per; r += TPB) s += kl[(size_t)k * per + r];
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) out[2 + k] = exp(s / (double)per);        // per == 0: 0 / 0 = NaN, as numpy's mean of an empty list
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = 0.0;
    for (int k = 0; k < splits; ++k) m += out[2 + k];
    m /= (double)splits;
    double v = 0.0;
    for (int k = 0; k < splits; ++k) { const double d = out[2 + k] - m; v += d * d; }
    out[0] = m;
    out[1] = sqrt(v / (double)splits);
  }
}

}  // namespace

// ================================================================================================================================
// C ABI
// ================================================================================================================================
extern "C" int sg_conv2d_rect_plan(const sgRectDesc* d, int w_aligned16, sgRectPlan* plan) {
  SG_ARG_CHECK(rect_desc_ok(d), "sg_conv2d_rect_plan: bad desc");
  SG_ARG_CHECK(plan != nullptr, "sg_conv2d_rect_plan: null plan");
  rect_plan_copy(rect_plan(d, w_aligned16 != 0), plan);
  return 0;
}

extern "C" size_t sg_conv2d_rect_ws_bytes(const sgRectDesc* d) { return rect_desc_ok(d) ? rect_ws_bytes(rect_plan(d, true), d) : 0; }

extern "C" int sg_conv2d_rect_fwd(const sgRectDesc* d, const float* x, const float* w, const float* bias, float* y, int act, void* ws,
                                  size_t ws_bytes, sgStream stream) {
  SG_ARG_CHECK(rect_desc_ok(d), "sg_conv2d_rect_fwd: bad desc (KH * KW <= %d, stride 1 or 2, 0 <= pad < kernel, OH / OW of the "
               "zero-padded conv, out_c0 + Cout <= out_ctot, tensors below 2^29 elements)", RECT_MAX_TAPS);
  hipStream_t s = (hipStream_t)stream;
  const RectPlan pl = rect_plan(d, aligned16(w));
  const bool vec = pl.vec != 0;
  const int kind = pl.tile == SG_RECT_TILE_32X128 ? SG_K_RECT_CONV_T32 : pl.tile == SG_RECT_TILE_64X128 ? SG_K_RECT_CONV_T64W : SG_K_RECT_CONV_T64;
  return rect_fwd("sg_conv2d_rect", kind, pl, d, x, w, bias, y, act, ws, ws_bytes, s,
                  [&](const Gather& g, const KEntry* ktab, const EpNCHW& ep, int M, int K, int Npix) {
    switch (pl.tile) {
      case SG_RECT_TILE_32X128:
        rect_launch<CfgFor<3>::C32, 32, 128>(w, K, M, vec, RectGather<128>{g, Npix, ktab, d->KH, d->KW, d->padH, d->padW}, ep, Npix,
                                             pl.splits, s);
        break;
      case SG_RECT_TILE_64X128:
        rect_launch<CfgFor<3>::C64W, 64, 128>(w, K, M, vec, RectGather<128>{g, Npix, ktab, d->KH, d->KW, d->padH, d->padW}, ep, Npix,
                                              pl.splits, s);
        break;
      default:
        rect_launch<CfgFor<3>::C64, 64, 64>(w, K, M, vec, RectGather<64>{g, Npix, ktab, d->KH, d->KW, d->padH, d->padW}, ep, Npix,
                                            pl.splits, s);
        break;
    }
  });
}

extern "C" int sg_maxpool3s2v_fwd(const float* x, float* y, int N, int C, int H, int W, int OH, int OW, int out_c0, int out_ctot,
                                  sgStream stream) {
  SG_ARG_CHECK(N >= 0 && C >= 1 && H >= 3 && W >= 3 && OH == (H - 3) / 2 + 1 && OW == (W - 3) / 2 + 1 && out_c0 >= 0 &&
               out_c0 + C <= out_ctot && (double)N * C * H * W < 2147483647.0 && (double)N * out_ctot * OH * OW < 2147483647.0,
               "sg_maxpool3s2v_fwd: bad sizes (N=%d C=%d H=%d W=%d OH=%d OW=%d out_c0=%d out_ctot=%d)", N, C, H, W, OH, OW, out_c0, out_ctot);
  if (N == 0) return 0;
  SG_ARG_CHECK(x && y, "sg_maxpool3s2v_fwd: null operand");
  hipStream_t s = (hipStream_t)stream;
  const unsigned total = (unsigned)N * C * OH * OW;
  SgProfScope prof(SG_K_INCEPTION_POOL, s, 0.0, 4.0 * ((double)N * C * H * W + (double)total));
  hipLaunchKernelGGL(maxpool3s2v_kernel, dim3(sg_cdiv(total, TPB)), dim3(TPB), 0, s, x, y, total, C, H, W, OH, OW, out_c0, out_ctot,
                     FastDiv((unsigned)OW), FastDiv((unsigned)OH), FastDiv((unsigned)C));
  SG_LAUNCH_CHECK("sg_maxpool3s2v_fwd");
  return 0;
}

extern "C" int sg_avgpool3s1_fwd(const float* x, float* y, int NC, int H, int W, sgStream stream) {
  SG_ARG_CHECK(NC >= 0 && H >= 1 && W >= 1 && (double)NC * H * W < 2147483647.0, "sg_avgpool3s1_fwd: bad sizes (NC=%d H=%d W=%d)", NC, H, W);
  if (NC == 0) return 0;
  SG_ARG_CHECK(x && y, "sg_avgpool3s1_fwd: null operand");
  hipStream_t s = (hipStream_t)stream;
  const unsigned total = (unsigned)NC * H * W;
  SgProfScope prof(SG_K_INCEPTION_POOL, s, 0.0, 8.0 * (double)total);
  hipLaunchKernelGGL(avgpool3s1_kernel, dim3(sg_cdiv(total, TPB)), dim3(TPB), 0, s, x, y, total, H, W, FastDiv((unsigned)W),
                     FastDiv((unsigned)H));
  SG_LAUNCH_CHECK("sg_avgpool3s1_fwd");
  return 0;
}

extern "C" int sg_avgpool3s1x_fwd(const float* x, float* y, int NC, int H, int W, sgStream stream) {
  SG_ARG_CHECK(NC >= 0 && H >= 1 && W >= 1 && (double)NC * H * W < 2147483647.0, "sg_avgpool3s1x_fwd: bad sizes (NC=%d H=%d W=%d)", NC, H, W);
  if (NC == 0) return 0;
  SG_ARG_CHECK(x && y, "sg_avgpool3s1x_fwd: null operand");
  hipStream_t s = (hipStream_t)stream;
  const unsigned total = (unsigned)NC * H * W;
  SgProfScope prof(SG_K_INCEPTION_POOL, s, 0.0, 8.0 * (double)total);
  hipLaunchKernelGGL(avgpool3s1x_kernel, dim3(sg_cdiv(total, TPB)), dim3(TPB), 0, s, x, y, total, H, W, FastDiv((unsigned)W),
                     FastDiv((unsigned)H));
  SG_LAUNCH_CHECK("sg_avgpool3s1x_fwd");
  return 0;
}

extern "C" int sg_maxpool3s1_fwd(const float* x, float* y, int NC, int H, int W, sgStream stream) {
  SG_ARG_CHECK(NC >= 0 && H >= 1 && W >= 1 && (double)NC * H * W < 2147483647.0, "sg_maxpool3s1_fwd: bad sizes (NC=%d H=%d W=%d)", NC, H, W);
  if (NC == 0) return 0;
  SG_ARG_CHECK(x && y, "sg_maxpool3s1_fwd: null operand");
  hipStream_t s = (hipStream_t)stream;
  const unsigned total = (unsigned)NC * H * W;
  SgProfScope prof(SG_K_INCEPTION_POOL, s, 0.0, 8.0 * (double)total);
  hipLaunchKernelGGL(maxpool3s1_kernel, dim3(sg_cdiv(total, TPB)), dim3(TPB), 0, s, x, y, total, H, W, FastDiv((unsigned)W),
                     FastDiv((unsigned)H));
  SG_LAUNCH_CHECK("sg_maxpool3s1_fwd");
  return 0;
}

extern "C" int sg_resize_bilinear_fwd(const float* x, float* y, int NC, int H, int W, int OH, int OW, sgStream stream) {
  SG_ARG_CHECK(NC >= 0 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1 && (double)NC * H * W < 2147483647.0 &&
               (double)NC * OH * OW < 2147483647.0, "sg_resize_bilinear_fwd: bad sizes (NC=%d H=%d W=%d OH=%d OW=%d)", NC, H, W, OH, OW);
  if (NC == 0) return 0;
  SG_ARG_CHECK(x && y, "sg_resize_bilinear_fwd: null operand");
  hipStream_t s = (hipStream_t)stream;
  const unsigned total = (unsigned)NC * OH * OW;
  SgProfScope prof(SG_K_RESIZE_BILINEAR, s, 0.0, 4.0 * ((double)NC * H * W + (double)total));
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3(sg_cdiv(total, TPB)), dim3(TPB), 0, s, x, y, total, H, W, OH, OW, FastDiv((unsigned)OW),
                     FastDiv((unsigned)OH));
  SG_LAUNCH_CHECK("sg_resize_bilinear_fwd");
  return 0;
}

extern "C" int sg_softmax_rows(const float* logits, int rows, int classes, float* out, int row0, int capacity, sgStream stream) {
  SG_ARG_CHECK(rows >= 0 && classes >= 1 && row0 >= 0 && (int64_t)row0 + rows <= (int64_t)capacity,
               "sg_softmax_rows: bad sizes (rows=%d classes=%d row0=%d capacity=%d)", rows, classes, row0, capacity);
  if (rows == 0) return 0;
  SG_ARG_CHECK(logits && out, "sg_softmax_rows: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_SOFTMAX_ROWS, s, 0.0, 8.0 * (double)rows * classes);
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(sg_cdiv(rows, WPB)), dim3(TPB), 0, s, logits, out + (size_t)row0 * classes, rows, classes);
  SG_LAUNCH_CHECK("sg_softmax_rows");
  return 0;
}

extern "C" size_t sg_inception_score_ws_bytes(int n, int classes, int splits) {
  if (n < 0 || classes < 1 || splits < 1) return 0;
  return ((size_t)splits * classes + (size_t)n) * sizeof(double) + 16;
}

extern "C" int sg_inception_score(const float* probs, int n, int classes, int splits, void* out, void* ws, size_t ws_bytes,
                                  sgStream stream) {
  SG_ARG_CHECK(n >= 0 && classes >= 1 && splits >= 1 && splits <= 65535, "sg_inception_score: bad sizes (n=%d classes=%d splits=%d)", n,
               classes, splits);
  SG_ARG_CHECK(out && ws && ws_bytes >= sg_inception_score_ws_bytes(n, classes, splits) && (n == 0 || probs),
               "sg_inception_score: null operand or a workspace below sg_inception_score_ws_bytes");
  SG_ARG_CHECK((reinterpret_cast<uintptr_t>(out) & 7) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
               "sg_inception_score: out and ws must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int per = n / splits;              // the tail rows n - per * splits are dropped
  double* py = reinterpret_cast<double*>(ws);
  double* kl = py + (size_t)splits * classes;
  SgProfScope prof(SG_K_INCEPTION_SCORE, s, 0.0, 8.0 * (double)per * splits * classes);
  if (per > 0) {
    hipLaunchKernelGGL(score_colmean_kernel, dim3(sg_cdiv(classes, TPB), splits), dim3(TPB), 0, s, probs, py, per, classes);
    hipLaunchKernelGGL(score_kl_kernel, dim3(per * splits), dim3(TPB), 0, s, probs, (const double*)py, kl, per, classes);
  }
  hipLaunchKernelGGL(score_final_kernel, dim3(1), dim3(TPB), 0, s, (const double*)kl, reinterpret_cast<double*>(out), per, splits);
  SG_LAUNCH_CHECK("sg_inception_score");
  return 0;
}
