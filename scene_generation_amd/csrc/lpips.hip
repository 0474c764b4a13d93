// The diversity score (scene_generation_amd/lpips.py): what LPIPS on AlexNet / VGG-16 needs beyond the entry points that already exist.
//
//   sg_conv2d_wide_fwd      sg_conv2d_rect_fwd's contract for kernels up to 11 x 11 and strides 1..4 (AlexNet's 11 x 11 stride-4 stem):
//                           the same implicit GEMM (fp32 MFMA) and the same rectangular gather loader (rect_gather.h), instantiated with
//                           a 121-tap LDS table on 64 x 64 tiles only (see WIDE_MAX_TAPS below for the LDS budget)
//   sg_lpips_input          the scaling layer: (x - shift[c]) / scale[c] from fp32 in [-1, 1] or from uint8
//   sg_lpips_layer          one tap of the distance: channel-normalise both feature maps, weighted squared difference summed over the
//                           channels (fp32), spatial mean in fp64 -- one pass over the features
//   sg_lpips_layer_bwd      the gradient of a tap with respect to f0 (LPIPS as a training loss), in the forward kernel's shape
//   sg_lpips_input_bwd      the scaling layer's backward: gy / scale[c]
//
// The convolution is forward only (the loss runs on VGG-16, whose layers have their own backward).  No float atomics and no sum whose order depends on the launch: every result is bit-identical from run to run.
#include "igemm_core.h"
#include "rect_gather.h"
#include <math.h>

namespace {

constexpr int TPB = 256;
// The LDS tap table of the gather is (taps + 1) x BN ints.  121 taps on a 64-pixel tile are 31 232 bytes, 51 712 with the two
// double-buffered operand tiles of a 64 x 64 workgroup: three workgroups fit the 160 KB of a compute unit.  A 128-pixel tile would
// need 62 464 bytes for the table alone (one workgroup per CU with its operand tiles, and past the 64 KB a workgroup may declare), so
// the wide entry point runs 64 x 64 tiles for every shape.
constexpr int WIDE_MAX_K = 11, WIDE_MAX_TAPS = WIDE_MAX_K * WIDE_MAX_K, WIDE_MAX_STRIDE = 4;
using WideGather = LoadGatherRect<64, WIDE_MAX_TAPS>;
static_assert((WideGather::LDS_INTS + 2 * (64 + 64) * LDK) * 4 <= 80 * 1024, "wide gather: two workgroups per compute unit");

inline bool wide_desc_ok(const sgRectDesc* d) { return rect_desc_ok(d, WIDE_MAX_K, WIDE_MAX_K, WIDE_MAX_TAPS, WIDE_MAX_STRIDE); }

inline RectPlan wide_plan(const sgRectDesc* d, bool w16) {
  const RectDims n(d);
  RectPlan p;
  p.vec = (n.K % 4 == 0 && w16) ? 1 : 0;
  p.tile = SG_RECT_TILE_64X64; p.bm = 64; p.bn = 64;
  rect_plan_splits(p, n.M, n.K, n.Npix);
  return p;
}

// ---- the scaling layer ---------------------------------------------------------------------------------------------------------------
// v = u / 127.5 - 1 for uint8 sources; y = (v - shift[c]) / scale[c]; every operation rounded on its own (no contraction).  NHWC: the
// source is [N, HW, 3] (the pictures a sampler hands out); the result is [N, 3, HW] either way.
template <bool U8, bool NHWC>
__global__ void __launch_bounds__(TPB) lpips_input_kernel(const void* __restrict__ src, float* __restrict__ y, unsigned total, int HW,
                                                         FastDiv fhw) {
  const unsigned i = blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const unsigned plane = fhw.div(i), n = plane / 3u, c = plane - n * 3u;
  const unsigned j = NHWC ? (n * (unsigned)HW + (i - plane * (unsigned)HW)) * 3u + c : i;
  float v;
  if (U8) v = __fsub_rn(__fdiv_rn((float)reinterpret_cast<const uint8_t*>(src)[j], 127.5f), 1.f);
  else v = reinterpret_cast<const float*>(src)[j];
  const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
  const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
  y[i] = __fdiv_rn(__fsub_rn(v, shift), scale);
}

// ---- one tap of the distance -----------------------------------------------------------------------------------------------------------
// A workgroup takes TP consecutive pixels of one pair; its 256 threads are G = 256 / TP channel groups of TP pixels, so a wave reads
// runs of TP consecutive pixels of 64 / TP channels.  Thread (g, px) owns the channels g, g + G, g + 2G, ...: the first RC of them stay
// in registers between the two passes (every shape the launcher picks this instantiation for fits entirely); channels beyond are read
// again (they come from cache: the workgroup read them a moment ago).
//   pass 1: q = sum_c f^2 per side; the G partials of a pixel meet in LDS in ascending g; n = sqrt(q)
//   pass 2: s = sum_c w_c * (f0_c / (n0 + eps) - f1_c / (n1 + eps))^2, direct form, both sides by the same code => d(x, x) = 0 exactly
// Then the pixel sums in fp64: an LDS tree over the TP pixels of the workgroup, one partial per (pair, tile); the tiles of a pair are
// added in ascending order by lpips_finish_kernel (or here, when the pair has a single tile).
__device__ __forceinline__ double lpips_store(double mean, double* out, int accumulate) { return accumulate ? *out + mean : mean; }

template <int TP, int RC>
__global__ void __launch_bounds__(TPB) lpips_layer_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                         const float* __restrict__ w, int C, int HW, int ntiles, float eps,
                                                         double* __restrict__ part, double* __restrict__ out, int accumulate) {
  constexpr int G = TPB / TP;
  __shared__ float red[2][G][TP];
  __shared__ double dred[TP];
  const int px = threadIdx.x % TP, g = threadIdx.x / TP;
  const int p = blockIdx.x / ntiles, tile = blockIdx.x - p * ntiles;
  const int pix = tile * TP + px;
  const bool inside = pix < HW;
  const size_t base = (size_t)p * C * HW + (inside ? pix : 0);
  const float* a = f0 + base;
  const float* b = f1 + base;
  float r0[RC], r1[RC];
  float q0 = 0.f, q1 = 0.f;
#pragma unroll
  for (int i = 0; i < RC; ++i) {
    const int c = g + i * G;
    const bool ok = inside && c < C;
    r0[i] = ok ? a[(size_t)c * HW] : 0.f;
    r1[i] = ok ? b[(size_t)c * HW] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < RC; ++i) { q0 = fmaf(r0[i], r0[i], q0); q1 = fmaf(r1[i], r1[i], q1); }
  if (inside)
    for (int c = g + RC * G; c < C; c += G) {
      const float u = a[(size_t)c * HW], v = b[(size_t)c * HW];
      q0 = fmaf(u, u, q0); q1 = fmaf(v, v, q1);
    }
  red[0][g][px] = q0; red[1][g][px] = q1;
  __syncthreads();
  float n0 = 0.f, n1 = 0.f;
#pragma unroll
  for (int j = 0; j < G; ++j) { n0 += red[0][j][px]; n1 += red[1][j][px]; }
  const float d0 = __fadd_rn(__fsqrt_rn(n0), eps), d1 = __fadd_rn(__fsqrt_rn(n1), eps);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < RC; ++i) {
    const int c = g + i * G;
    const float t = __fsub_rn(__fdiv_rn(r0[i], d0), __fdiv_rn(r1[i], d1));      // a channel past C holds 0 on both sides: t = 0
    const float wc = (w && c < C) ? w[c] : 1.f;
    s = fmaf(wc, __fmul_rn(t, t), s);
  }
  if (inside)
    for (int c = g + RC * G; c < C; c += G) {
      const float t = __fsub_rn(__fdiv_rn(a[(size_t)c * HW], d0), __fdiv_rn(b[(size_t)c * HW], d1));
      s = fmaf(w ? w[c] : 1.f, __fmul_rn(t, t), s);
    }
  __syncthreads();
  red[0][g][px] = s;
  __syncthreads();
  if (g == 0) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < G; ++j) t += red[0][j][px];
    dred[px] = inside ? (double)t : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int o = TP / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) dred[threadIdx.x] += dred[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (ntiles == 1) out[p] = lpips_store(dred[0] / (double)HW, out + p, accumulate);
    else part[(size_t)p * ntiles + tile] = dred[0];
  }
}

// out[p] (+)= (sum of the pair's tile partials, each lane its tiles in ascending order, the lanes met by an LDS tree) / HW
__global__ void __launch_bounds__(64) lpips_finish_kernel(const double* __restrict__ part, int ntiles, int HW, double* __restrict__ out,
                                                         int accumulate) {
  __shared__ double dred[64];
  const int p = blockIdx.x;
  double v = 0.0;
  for (int t = threadIdx.x; t < ntiles; t += 64) v += part[(size_t)p * ntiles + t];
  dred[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) dred[threadIdx.x] += dred[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[p] = lpips_store(dred[0] / (double)HW, out + p, accumulate);
}

// ---- the gradient of one tap with respect to f0 (the perceptual loss: scene_generation_amd/lpips.py LPIPSLoss) ---------------------------
// The forward kernel's shape: the same (channel group, pixel) threads, the same registers, the same pass 1 and the same t_c, so
// f0 == f1 bit for bit gives t_c = 0 and a gradient of exactly +0.  Three phases, two LDS reductions in ascending g per pixel:
//   phase 1: q0, q1 -> n = sqrt(q), s = n + eps per side                                            (reduction 1)
//   phase 2: g_c = 2 w_c t_c * (float)(gout[p] / HW), kept in the registers f1 occupied; dot = sum_c g_c f0_c     (reduction 2)
//   phase 3: gf0_k = g_k / s0 - (f0_k / s0) * ((dot / s0) / n0): every factor stays in the fp32 range while n0 is a normal float
//            (|dot| <= |g| n0, so (dot / s0) / n0 <= |g| / s0; the denominator n0 * s0^2 ~ 1e-35 of the textbook form is never formed)
// A pixel with n0 == 0 gets the finite g_k / s0 (second term 0), where autograd of the formula gives NaN (the derivative of sqrt at
// 0): every tap is a ReLU output, so a pixel whose channels are all 0 has every pre-activation <= 0 and the ReLU backward drops
// whatever arrives there -- torch's by selection, this library's act_bwd by the factor 0, which needs the value finite.  Every element of gf0 is written exactly once (no atomics, no
// workspace): two reads and one write of the feature map, bit-identical from run to run.
template <int TP, int RC>
__global__ void __launch_bounds__(TPB) lpips_layer_bwd_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                             const float* __restrict__ w, const double* __restrict__ gout, int C,
                                                             int HW, int ntiles, float eps, float* __restrict__ gf0) {
  constexpr int G = TPB / TP;
  __shared__ float red[2][G][TP];
  const int px = threadIdx.x % TP, g = threadIdx.x / TP;
  const int p = blockIdx.x / ntiles, tile = blockIdx.x - p * ntiles;
  const int pix = tile * TP + px;
  const bool inside = pix < HW;
  const size_t base = (size_t)p * C * HW + (inside ? pix : 0);
  const float* a = f0 + base;
  const float* b = f1 + base;
  float* o = gf0 + base;
  const float gs = (float)(gout[p] / (double)HW);
  float r0[RC], r1[RC];
  float q0 = 0.f, q1 = 0.f;
#pragma unroll
  for (int i = 0; i < RC; ++i) {
    const int c = g + i * G;
    const bool ok = inside && c < C;
    r0[i] = ok ? a[(size_t)c * HW] : 0.f;
    r1[i] = ok ? b[(size_t)c * HW] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < RC; ++i) { q0 = fmaf(r0[i], r0[i], q0); q1 = fmaf(r1[i], r1[i], q1); }
  if (inside)
    for (int c = g + RC * G; c < C; c += G) {
      const float u = a[(size_t)c * HW], v = b[(size_t)c * HW];
      q0 = fmaf(u, u, q0); q1 = fmaf(v, v, q1);
    }
  red[0][g][px] = q0; red[1][g][px] = q1;
  __syncthreads();
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int j = 0; j < G; ++j) { s0 += red[0][j][px]; s1 += red[1][j][px]; }
  const float n0 = __fsqrt_rn(s0);
  const float d0 = __fadd_rn(n0, eps), d1 = __fadd_rn(__fsqrt_rn(s1), eps);
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < RC; ++i) {
    const int c = g + i * G;
    const float t = __fsub_rn(__fdiv_rn(r0[i], d0), __fdiv_rn(r1[i], d1));      // the forward's t: a channel past C holds 0 on both sides
    const float wc = (w && c < C) ? w[c] : 1.f;
    r1[i] = __fmul_rn(__fmul_rn(__fmul_rn(2.f, wc), t), gs);
    dot = fmaf(r1[i], r0[i], dot);
  }
  if (inside)
    for (int c = g + RC * G; c < C; c += G) {
      const float u = a[(size_t)c * HW];
      const float t = __fsub_rn(__fdiv_rn(u, d0), __fdiv_rn(b[(size_t)c * HW], d1));
      dot = fmaf(__fmul_rn(__fmul_rn(__fmul_rn(2.f, w ? w[c] : 1.f), t), gs), u, dot);
    }
  __syncthreads();
  red[0][g][px] = dot;
  __syncthreads();
  float ds = 0.f;
#pragma unroll
  for (int j = 0; j < G; ++j) ds += red[0][j][px];
  const float k = n0 > 0.f ? __fdiv_rn(__fdiv_rn(ds, d0), n0) : 0.f;
  if (!inside) return;
#pragma unroll
  for (int i = 0; i < RC; ++i) {
    const int c = g + i * G;
    // (+ 0: a gradient of -0 -- t = 0 under a negative gout -- leaves as +0)
    if (c < C) o[(size_t)c * HW] = __fadd_rn(__fsub_rn(__fdiv_rn(r1[i], d0), __fmul_rn(__fdiv_rn(r0[i], d0), k)), 0.f);
  }
  for (int c = g + RC * G; c < C; c += G) {
    const float u = a[(size_t)c * HW];
    const float t = __fsub_rn(__fdiv_rn(u, d0), __fdiv_rn(b[(size_t)c * HW], d1));
    const float gc = __fmul_rn(__fmul_rn(__fmul_rn(2.f, w ? w[c] : 1.f), t), gs);
    o[(size_t)c * HW] = __fadd_rn(__fsub_rn(__fdiv_rn(gc, d0), __fmul_rn(__fdiv_rn(u, d0), k)), 0.f);
  }
}

// the scaling layer's backward: gx = gy / scale[c], one rounding like the forward's division
__global__ void __launch_bounds__(TPB) lpips_input_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx, unsigned total,
                                                             FastDiv fhw) {
  const unsigned i = blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const unsigned c = fhw.div(i) % 3u;
  gx[i] = __fdiv_rn(gy[i], c == 0 ? .458f : (c == 1 ? .448f : .450f));
}

// the launch of a tap: 64-pixel tiles (a wave reads 256 contiguous bytes per channel) while a thread's C / 4 channels fit its 32
// registers per side and the launch still gives every compute unit a workgroup; 16-pixel tiles otherwise (C / 16 channels per thread: up to 512 in registers)
struct LayerPlan { int tp, rc, ntiles; };

inline LayerPlan layer_plan(int P, int C, int HW) {
  LayerPlan p;
  const bool wide = sg_cdiv(C, 4) <= 32 && HW >= 64 && (long)P * sg_cdiv(HW, 64) >= 256;
  p.tp = wide ? 64 : 16;
  p.rc = sg_cdiv(C, TPB / p.tp) <= 16 ? 16 : 32;
  p.ntiles = sg_cdiv(HW, p.tp);
  return p;
}

inline bool layer_sizes_ok(int P, int C, int HW) {
  return P >= 0 && C >= 1 && HW >= 1 && (double)P * C * HW < 2147483647.0 && (double)P * sg_cdiv(HW, 16) < 2147483647.0;
}

}  // namespace

// ================================================================================================================================
// C ABI
// ================================================================================================================================
extern "C" int sg_conv2d_wide_plan(const sgRectDesc* d, int w_aligned16, sgRectPlan* plan) {
  SG_ARG_CHECK(wide_desc_ok(d), "sg_conv2d_wide_plan: bad desc");
  SG_ARG_CHECK(plan != nullptr, "sg_conv2d_wide_plan: null plan");
  rect_plan_copy(wide_plan(d, w_aligned16 != 0), plan);
  return 0;
}

extern "C" size_t sg_conv2d_wide_ws_bytes(const sgRectDesc* d) { return wide_desc_ok(d) ? rect_ws_bytes(wide_plan(d, true), d) : 0; }

extern "C" int sg_conv2d_wide_fwd(const sgRectDesc* d, const float* x, const float* w, const float* bias, float* y, int act, void* ws,
                                  size_t ws_bytes, sgStream stream) {
  SG_ARG_CHECK(wide_desc_ok(d), "sg_conv2d_wide_fwd: bad desc (KH, KW <= %d, stride 1..%d, 0 <= pad < kernel, OH / OW of the "
               "zero-padded conv, out_c0 + Cout <= out_ctot, tensors below 2^29 elements)", WIDE_MAX_K, WIDE_MAX_STRIDE);
  hipStream_t s = (hipStream_t)stream;
  const RectPlan pl = wide_plan(d, aligned16(w));
  return rect_fwd("sg_conv2d_wide", SG_K_WIDE_CONV, pl, d, x, w, bias, y, act, ws, ws_bytes, s,
                  [&](const Gather& g, const KEntry* ktab, const EpNCHW& ep, int M, int K, int Npix) {
    rect_launch<CfgFor<3>::C64, 64, 64>(w, K, M, pl.vec != 0, WideGather{g, Npix, ktab, d->KH, d->KW, d->padH, d->padW}, ep, Npix,
                                        pl.splits, s);
  });
}

extern "C" int sg_lpips_input(const void* x, int x_uint8, int x_nhwc, int N, int HW, float* y, sgStream stream) {
  SG_ARG_CHECK(N >= 0 && HW >= 1 && (double)N * 3.0 * HW < 2147483647.0, "sg_lpips_input: bad sizes (N=%d HW=%d)", N, HW);
  if (N == 0) return 0;
  SG_ARG_CHECK(x && y, "sg_lpips_input: null operand");
  hipStream_t s = (hipStream_t)stream;
  const unsigned total = (unsigned)N * 3u * (unsigned)HW;
  const dim3 grid(sg_cdiv(total, TPB));
  const FastDiv fhw((unsigned)HW);
  SgProfScope prof(SG_K_LPIPS_INPUT, s, 0.0, (x_uint8 ? 5.0 : 8.0) * (double)total);
  if (x_uint8 && x_nhwc) hipLaunchKernelGGL((lpips_input_kernel<true, true>), grid, dim3(TPB), 0, s, x, y, total, HW, fhw);
  else if (x_uint8) hipLaunchKernelGGL((lpips_input_kernel<true, false>), grid, dim3(TPB), 0, s, x, y, total, HW, fhw);
  else if (x_nhwc) hipLaunchKernelGGL((lpips_input_kernel<false, true>), grid, dim3(TPB), 0, s, x, y, total, HW, fhw);
  else hipLaunchKernelGGL((lpips_input_kernel<false, false>), grid, dim3(TPB), 0, s, x, y, total, HW, fhw);
  SG_LAUNCH_CHECK("sg_lpips_input");
  return 0;
}

extern "C" size_t sg_lpips_layer_ws_bytes(int P, int C, int HW) {
  if (!layer_sizes_ok(P, C, HW)) return 0;
  const LayerPlan pl = layer_plan(P, C, HW);
  return pl.ntiles > 1 ? (size_t)P * pl.ntiles * sizeof(double) : 0;
}

extern "C" int sg_lpips_layer(const float* f0, const float* f1, const float* w, int P, int C, int HW, float eps, double* out,
                              int accumulate, void* ws, size_t ws_bytes, sgStream stream) {
  SG_ARG_CHECK(layer_sizes_ok(P, C, HW), "sg_lpips_layer: bad sizes (P=%d C=%d HW=%d; P * C * HW below 2^31)", P, C, HW);
  SG_ARG_CHECK(eps >= 0.f, "sg_lpips_layer: eps must not be negative");
  if (P == 0) return 0;
  SG_ARG_CHECK(f0 && f1 && out, "sg_lpips_layer: null operand");
  const LayerPlan pl = layer_plan(P, C, HW);
  const size_t need = pl.ntiles > 1 ? (size_t)P * pl.ntiles * sizeof(double) : 0;
  SG_ARG_CHECK(need == 0 || (ws && ws_bytes >= need), "sg_lpips_layer: workspace of %zu bytes, sg_lpips_layer_ws_bytes asks for %zu",
               ws_bytes, need);
  SG_ARG_CHECK((reinterpret_cast<uintptr_t>(out) & 7) == 0 && (need == 0 || (reinterpret_cast<uintptr_t>(ws) & 7) == 0),
               "sg_lpips_layer: out and ws must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(ws);
  const dim3 grid((unsigned)P * (unsigned)pl.ntiles);
  SgProfScope prof(SG_K_LPIPS_LAYER, s, 0.0, 8.0 * (double)P * C * HW);
#define SG_LPIPS_LAUNCH(TP, RC)                                                                                                 \
  hipLaunchKernelGGL((lpips_layer_kernel<TP, RC>), grid, dim3(TPB), 0, s, f0, f1, w, C, HW, pl.ntiles, eps, part, out, accumulate)
  if (pl.tp == 64) { if (pl.rc == 16) SG_LPIPS_LAUNCH(64, 16); else SG_LPIPS_LAUNCH(64, 32); }
  else { if (pl.rc == 16) SG_LPIPS_LAUNCH(16, 16); else SG_LPIPS_LAUNCH(16, 32); }
#undef SG_LPIPS_LAUNCH
  SG_LAUNCH_CHECK("sg_lpips_layer");
  if (pl.ntiles > 1) {
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(P), dim3(64), 0, s, (const double*)part, pl.ntiles, HW, out, accumulate);
    SG_LAUNCH_CHECK("sg_lpips_layer (tile sum)");
  }
  return 0;
}

extern "C" int sg_lpips_layer_bwd(const float* f0, const float* f1, const float* w, const double* gout, int P, int C, int HW, float eps,
                                  float* gf0, sgStream stream) {
  SG_ARG_CHECK(layer_sizes_ok(P, C, HW), "sg_lpips_layer_bwd: bad sizes (P=%d C=%d HW=%d; P * C * HW below 2^31)", P, C, HW);
  SG_ARG_CHECK(eps >= 0.f, "sg_lpips_layer_bwd: eps must not be negative");
  if (P == 0) return 0;
  SG_ARG_CHECK(f0 && f1 && gout && gf0, "sg_lpips_layer_bwd: null operand");
  SG_ARG_CHECK((reinterpret_cast<uintptr_t>(gout) & 7) == 0, "sg_lpips_layer_bwd: gout must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const LayerPlan pl = layer_plan(P, C, HW);                     // the forward's plan: the same tiles and registers
  const dim3 grid((unsigned)P * (unsigned)pl.ntiles);
  SgProfScope prof(SG_K_LPIPS_LAYER, s, 0.0, 12.0 * (double)P * C * HW);
#define SG_LPIPS_LAUNCH(TP, RC)                                                                                                 \
  hipLaunchKernelGGL((lpips_layer_bwd_kernel<TP, RC>), grid, dim3(TPB), 0, s, f0, f1, w, gout, C, HW, pl.ntiles, eps, gf0)
  if (pl.tp == 64) { if (pl.rc == 16) SG_LPIPS_LAUNCH(64, 16); else SG_LPIPS_LAUNCH(64, 32); }
  else { if (pl.rc == 16) SG_LPIPS_LAUNCH(16, 16); else SG_LPIPS_LAUNCH(16, 32); }
#undef SG_LPIPS_LAUNCH
  SG_LAUNCH_CHECK("sg_lpips_layer_bwd");
  return 0;
}

extern "C" int sg_lpips_input_bwd(const float* gy, int N, int HW, float* gx, sgStream stream) {
  SG_ARG_CHECK(N >= 0 && HW >= 1 && (double)N * 3.0 * HW < 2147483647.0, "sg_lpips_input_bwd: bad sizes (N=%d HW=%d)", N, HW);
  if (N == 0) return 0;
  SG_ARG_CHECK(gy && gx, "sg_lpips_input_bwd: null operand");
  hipStream_t s = (hipStream_t)stream;
  const unsigned total = (unsigned)N * 3u * (unsigned)HW;
  SgProfScope prof(SG_K_LPIPS_INPUT, s, 0.0, 8.0 * (double)total);
  hipLaunchKernelGGL(lpips_input_bwd_kernel, dim3(sg_cdiv(total, TPB)), dim3(TPB), 0, s, gy, gx, total, FastDiv((unsigned)HW));
  SG_LAUNCH_CHECK("sg_lpips_input_bwd");
  return 0;
}
