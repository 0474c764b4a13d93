// The object-accuracy classifier (scene_generation_amd/accuracy.py): what a torchvision ResNet needs beyond the convolutions,
// BatchNorm, global pooling, dense layer and cross-entropy that already exist -- the stem's padded 3x3 stride-2 max-pool, the
// block tail relu(a + b), the fold of an eval-mode BatchNorm into the convolution before it, the SGD-momentum step of
// scripts/train_accuracy_net.py:265 and the device-side bookkeeping of scripts/sample_images.py:233-239.
//
// No float atomics and no float sum whose order depends on the launch: every result is bit-identical from run to run.  The only
// atomics are the three int64 counters of sg_classify_stats.  Base pointers may be unaligned; the element-wise kernels take
// 16-byte loads only when every operand starts on a 16-byte boundary.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int WPB = TPB / SG_WAVE;

__device__ __forceinline__ bool is_nan(float v) { return v != v; }

// ---- nn.MaxPool2d(3, stride=2, padding=1) -----------------------------------------------------------------------------------------
// The winner of window (oh, ow): torch's scan, rows then columns over the part of the window inside the plane, starting from -inf,
// taking a value when it is greater than the running maximum or a NaN -- the first maximum in scan order, and the last NaN.
__device__ __forceinline__ int pool_winner(const float* __restrict__ xp, int H, int W, int oh, int ow, float& best) {
  const int h0 = 2 * oh - 1, w0 = 2 * ow - 1;
  const int hb = h0 < 0 ? 0 : h0, wb = w0 < 0 ? 0 : w0;
  const int he = h0 + 3 < H ? h0 + 3 : H, we = w0 + 3 < W ? w0 + 3 : W;
  float m = -__builtin_inff();
  int at = hb * W + wb;
  for (int h = hb; h < he; ++h)
    for (int w = wb; w < we; ++w) {
      const float v = xp[h * W + w];
      if (v > m || is_nan(v)) { m = v; at = h * W + w; }
    }
  best = m;
  return at;
}

__global__ void __launch_bounds__(TPB) maxpool3s2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t total, int H,
                                                            int W, int OH, int OW, FastDiv fow, FastDiv foh) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  // total < 2^31 is checked by the host, so the index fits FastDiv
  const unsigned r = fow.div((unsigned)i), ow = (unsigned)i - r * OW;
  const unsigned nc = foh.div(r), oh = r - nc * OH;
  float m;
  pool_winner(x + (size_t)nc * H * W, H, W, (int)oh, (int)ow, m);
  y[i] = m;
}

// a gather: input pixel (h, w) lies in the windows oh in {h / 2, (h + 1) / 2}, ow likewise (one per axis when the coordinate is
// even); each window's winner is recomputed from x, and the pixel takes the gradients of the windows it won, summed in (oh, ow) order
__global__ void __launch_bounds__(TPB) maxpool3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                            float* __restrict__ gx, int64_t total, int H, int W, int OH, int OW,
                                                            FastDiv fw, FastDiv fh) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= total) return;
  const unsigned r = fw.div((unsigned)i), w = (unsigned)i - r * W;
  const unsigned nc = fh.div(r), h = r - nc * H;
  const float* xp = x + (size_t)nc * H * W;
  const float* gp = gy + (size_t)nc * OH * OW;
  const int me = (int)(h * W + w);
  const int oh0 = (int)h >> 1, oh1 = ((int)h + 1) >> 1, ow0 = (int)w >> 1, ow1 = ((int)w + 1) >> 1;
  float g = 0.f;
  for (int oh = oh0; oh <= oh1 && oh < OH; ++oh)
    for (int ow = ow0; ow <= ow1 && ow < OW; ++ow) {
      float m;
      if (pool_winner(xp, H, W, oh, ow, m) == me) g += gp[oh * OW + ow];
    }
  gx[i] = g;
}

// ---- relu(a + b) ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float add_relu1(float a, float b) {
  const float v = a + b;
  return (v > 0.f || is_nan(v)) ? v : 0.f;      // a NaN stays a NaN, as in torch.relu
}

template <bool VEC>
__global__ void __launch_bounds__(TPB) add_relu_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y,
                                                      int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (VEC) {
    const int64_t e = i * 4;
    if (e + 3 < n) {
      const float4 p = *reinterpret_cast<const float4*>(a + e), q = *reinterpret_cast<const float4*>(b + e);
      float4 o;
      o.x = add_relu1(p.x, q.x); o.y = add_relu1(p.y, q.y); o.z = add_relu1(p.z, q.z); o.w = add_relu1(p.w, q.w);
      *reinterpret_cast<float4*>(y + e) = o;
    } else {
      for (int64_t k = e; k < n; ++k) y[k] = add_relu1(a[k], b[k]);
    }
  } else if (i < n) {
    y[i] = add_relu1(a[i], b[i]);
  }
}

// ---- eval-mode BatchNorm folded into the convolution before it ----------------------------------------------------------------------
// blockIdx.y = output channel; s = gamma / sqrt(var + eps), w' = w * s, b' = beta - mean * s
__global__ void __launch_bounds__(TPB) bn_fold_kernel(const float* __restrict__ w, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ mean,
                                                     const float* __restrict__ var, float eps, float* __restrict__ w_out,
                                                     float* __restrict__ b_out, int K) {
#pragma clang fp contract(off)
  const int co = blockIdx.y;
  const float s = gamma[co] / sqrtf(var[co] + eps);
  const float* wp = w + (size_t)co * K;
  float* op = w_out + (size_t)co * K;
  for (int k = blockIdx.x * TPB + threadIdx.x; k < K; k += gridDim.x * TPB) op[k] = wp[k] * s;
  if (blockIdx.x == 0 && threadIdx.x == 0) b_out[co] = beta[co] - mean[co] * s;
}

// ---- torch.optim.SGD(lr, momentum) ---------------------------------------------------------------------------------------------------
// every product and every sum rounded on its own (contraction off), so the step equals torch's sequence of separate operations
__device__ __forceinline__ void sgd1(float& p, float g, float& buf, float lr, float momentum, int first, float grad_scale) {
#pragma clang fp contract(off)
  const float gs = g * grad_scale;
  float t;
  if (first) {
    t = gs;
  } else {
    const float mb = momentum * buf;
    t = mb + gs;
  }
  buf = t;
  const float u = lr * t;
  p = p - u;
}

template <bool VEC>
__global__ void __launch_bounds__(TPB) sgd_momentum_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                          int64_t n, float lr, float momentum, int first, float grad_scale) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (VEC) {
    const int64_t e = i * 4;
    if (e + 3 < n) {
      float4 pp = *reinterpret_cast<float4*>(p + e), bb = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 gg = *reinterpret_cast<const float4*>(g + e);
      if (!first) bb = *reinterpret_cast<float4*>(buf + e);
      sgd1(pp.x, gg.x, bb.x, lr, momentum, first, grad_scale);
      sgd1(pp.y, gg.y, bb.y, lr, momentum, first, grad_scale);
      sgd1(pp.z, gg.z, bb.z, lr, momentum, first, grad_scale);
      sgd1(pp.w, gg.w, bb.w, lr, momentum, first, grad_scale);
      *reinterpret_cast<float4*>(p + e) = pp;
      *reinterpret_cast<float4*>(buf + e) = bb;
    } else {
      for (int64_t k = e; k < n; ++k) {
        float pv = p[k], bv = first ? 0.f : buf[k];
        sgd1(pv, g[k], bv, lr, momentum, first, grad_scale);
        p[k] = pv; buf[k] = bv;
      }
    }
  } else if (i < n) {
    float pv = p[i], bv = first ? 0.f : buf[i];
    sgd1(pv, g[i], bv, lr, momentum, first, grad_scale);
    p[i] = pv; buf[i] = bv;
  }
}

// ---- torch.max(logits, 1) and the accuracy record ---------------------------------------------------------------------------------------
// (value, index) a beats b: a NaN beats a number, of two NaNs or two equal numbers the lower index wins -- the first index of the
// maximum with NaN counted as the maximum, whatever the order the candidates are met in
__device__ __forceinline__ bool beats(float av, int ai, float bv, int bi) {
  const bool an = is_nan(av), bn = is_nan(bv);
  if (an != bn) return an;
  if (an || av == bv) return ai < bi;
  return av > bv;
}

// a wave per row; acc = {correct, counted, rows}
__global__ void __launch_bounds__(TPB) classify_stats_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                            int rows, int classes, int64_t ignore_label, int64_t* __restrict__ preds,
                                                            unsigned long long* __restrict__ acc) {
  __shared__ unsigned tally[2 * WPB];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, row = blockIdx.x * WPB + wid;
  unsigned correct = 0u, counted = 0u;
  if (row < rows) {                              // wave-uniform
    const float* lp = logits + (size_t)row * classes;
    float bv = -__builtin_inff();
    int bi = 0x7fffffff;                         // a lane without a class: loses to every candidate but an equal -inf with a lower index
    for (int c = lane; c < classes; c += SG_WAVE) {
      const float v = lp[c];
      if (beats(v, c, bv, bi)) { bv = v; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
      if (preds) preds[row] = (int64_t)bi;
      const int64_t t = target[row];
      counted = t != ignore_label ? 1u : 0u;
      correct = (counted && t == (int64_t)bi) ? 1u : 0u;
    }
  }
  if (lane == 0) { tally[2 * wid] = correct; tally[2 * wid + 1] = counted; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned c = 0u, n = 0u;
#pragma unroll
    for (int w = 0; w < WPB; ++w) { c += tally[2 * w]; n += tally[2 * w + 1]; }
    if (c) atomicAdd(&acc[0], (unsigned long long)c);
    if (n) atomicAdd(&acc[1], (unsigned long long)n);
    if (blockIdx.x == 0) atomicAdd(&acc[2], (unsigned long long)rows);
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

static int pool_sizes_ok(int NC, int H, int W, int OH, int OW) {
  return NC >= 0 && H >= 1 && W >= 1 && OH == (H - 1) / 2 + 1 && OW == (W - 1) / 2 + 1 && (int64_t)NC * H * W < ((int64_t)1 << 31);
}

extern "C" int sg_maxpool3s2_fwd(const float* x, float* y, int NC, int H, int W, int OH, int OW, sgStream stream) {
  SG_ARG_CHECK(pool_sizes_ok(NC, H, W, OH, OW), "sg_maxpool3s2_fwd: bad sizes (NC=%d H=%d W=%d OH=%d OW=%d)", NC, H, W, OH, OW);
  if (NC == 0) return 0;
  SG_ARG_CHECK(x && y, "sg_maxpool3s2_fwd: null operand");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)NC * OH * OW;
  SgProfScope prof(SG_K_MAXPOOL3S2, s, 0.0, 4.0 * ((double)NC * H * W + (double)total));
  hipLaunchKernelGGL(maxpool3s2_fwd_kernel, dim3(sg_cdiv(total, TPB)), dim3(TPB), 0, s, x, y, total, H, W, OH, OW,
                     FastDiv((unsigned)OW), FastDiv((unsigned)OH));
  SG_LAUNCH_CHECK("sg_maxpool3s2_fwd");
  return 0;
}

extern "C" int sg_maxpool3s2_bwd(const float* x, const float* gy, float* gx, int NC, int H, int W, int OH, int OW, sgStream stream) {
  SG_ARG_CHECK(pool_sizes_ok(NC, H, W, OH, OW), "sg_maxpool3s2_bwd: bad sizes (NC=%d H=%d W=%d OH=%d OW=%d)", NC, H, W, OH, OW);
  if (NC == 0) return 0;
  SG_ARG_CHECK(x && gy && gx, "sg_maxpool3s2_bwd: null operand");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)NC * H * W;
  SgProfScope prof(SG_K_MAXPOOL3S2, s, 0.0, 4.0 * (2.0 * (double)total + (double)NC * OH * OW));
  hipLaunchKernelGGL(maxpool3s2_bwd_kernel, dim3(sg_cdiv(total, TPB)), dim3(TPB), 0, s, x, gy, gx, total, H, W, OH, OW,
                     FastDiv((unsigned)W), FastDiv((unsigned)H));
  SG_LAUNCH_CHECK("sg_maxpool3s2_bwd");
  return 0;
}

extern "C" int sg_add_relu_fwd(const float* a, const float* b, float* y, int64_t n, sgStream stream) {
  SG_ARG_CHECK(n >= 0, "sg_add_relu_fwd: bad size (n=%lld)", (long long)n);
  if (n == 0) return 0;
  SG_ARG_CHECK(a && b && y, "sg_add_relu_fwd: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_ADD_RELU, s, 0.0, 12.0 * (double)n);
  if (al16(a) && al16(b) && al16(y))
    hipLaunchKernelGGL(add_relu_kernel<true>, dim3(sg_cdiv(sg_cdiv(n, 4), TPB)), dim3(TPB), 0, s, a, b, y, n);
  else
    hipLaunchKernelGGL(add_relu_kernel<false>, dim3(sg_cdiv(n, TPB)), dim3(TPB), 0, s, a, b, y, n);
  SG_LAUNCH_CHECK("sg_add_relu_fwd");
  return 0;
}

extern "C" int sg_bn_fold(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                          float* w_out, float* b_out, int Cout, int K, sgStream stream) {
  SG_ARG_CHECK(Cout >= 0 && Cout <= 65535 && K >= 1, "sg_bn_fold: bad sizes (Cout=%d K=%d, Cout <= 65535)", Cout, K);
  if (Cout == 0) return 0;
  SG_ARG_CHECK(w && gamma && beta && mean && var && w_out && b_out, "sg_bn_fold: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_BN_FOLD, s, 0.0, 8.0 * (double)Cout * K + 20.0 * Cout);
  const int bx = sg_cdiv(K, TPB) < 64 ? sg_cdiv(K, TPB) : 64;
  hipLaunchKernelGGL(bn_fold_kernel, dim3(bx, Cout), dim3(TPB), 0, s, w, gamma, beta, mean, var, eps, w_out, b_out, K);
  SG_LAUNCH_CHECK("sg_bn_fold");
  return 0;
}

extern "C" int sg_sgd_momentum_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, int first,
                                    float grad_scale, sgStream stream) {
  SG_ARG_CHECK(n >= 0, "sg_sgd_momentum_step: bad size (n=%lld)", (long long)n);
  if (n == 0) return 0;
  SG_ARG_CHECK(p && g && buf, "sg_sgd_momentum_step: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_SGD, s, 0.0, (first ? 16.0 : 20.0) * (double)n);
  if (al16(p) && al16(g) && al16(buf))
    hipLaunchKernelGGL(sgd_momentum_kernel<true>, dim3(sg_cdiv(sg_cdiv(n, 4), TPB)), dim3(TPB), 0, s, p, g, buf, n, lr, momentum,
                       first, grad_scale);
  else
    hipLaunchKernelGGL(sgd_momentum_kernel<false>, dim3(sg_cdiv(n, TPB)), dim3(TPB), 0, s, p, g, buf, n, lr, momentum, first,
                       grad_scale);
  SG_LAUNCH_CHECK("sg_sgd_momentum_step");
  return 0;
}

extern "C" int sg_classify_stats(const float* logits, const int64_t* target, int rows, int classes, int64_t ignore_label,
                                 int64_t* preds, int64_t* acc, sgStream stream) {
  SG_ARG_CHECK(rows >= 0 && classes >= 1, "sg_classify_stats: bad sizes (rows=%d classes=%d)", rows, classes);
  if (rows == 0) return 0;
  SG_ARG_CHECK(logits && target && acc, "sg_classify_stats: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_CLASSIFY_STATS, s, 0.0, (double)rows * (4.0 * classes + 8.0 + (preds ? 8.0 : 0.0)));
  hipLaunchKernelGGL(classify_stats_kernel, dim3(sg_cdiv(rows, WPB)), dim3(TPB), 0, s, logits, target, rows, classes, ignore_label,
                     preds, reinterpret_cast<unsigned long long*>(acc));
  SG_LAUNCH_CHECK("sg_classify_stats");
  return 0;
}
