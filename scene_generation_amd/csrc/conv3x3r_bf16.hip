// bf16-operand implicit GEMM for the ResnetBlock convs (ReflectionPad2d(1) + Conv2d(C, C, 3), reference layers.py:251-270):
// the opt-in mixed-precision path of the generator's residual trunk (GlobalGenerator.set_trunk_precision('bf16')).
//
// Every product of the forward, data-gradient and weight-gradient GEMMs takes operands rounded to bf16 (round to nearest
// even); the sums are fp32 (v_mfma_f32_16x16x32_bf16).  Inputs, outputs, weights and gradients stay fp32 in memory.
//
// Each direction is three launches, all stream-ordered in the caller's workspace (no allocation, no host sync):
//   1. pack  : both GEMM operands as K-contiguous, zero-padded bf16 images [rows_pad][Kpad] (the reflection is folded into
//              the gather: an im2col image of the padded input / a zero-extended gradient image), the weight re-laid once per
//              call,
//   2. gemm  : C[m][n] = sum_k A[m][k] * B[n][k] on 128 x 128 tiles, K split into S equal slices (S chosen per shape so
//              that the small fwd / dgrad grids still fill the chip), each slice writing its own fp32 slab,
//   3. reduce: the S slabs summed in a fixed order (deterministic: no float atomics) + bias / the dgrad reflection fold,
//              written to the NCHW output.
//   fwd  : M = Cout, N = N*H*W pixels,             K = 9*C      (k = ci*9 + tap)
//   dgrad: M = C,    N = N*(H+2)*(W+2) padded px,  K = 9*Cout   (gradient of the padded input, folded back by the reduce)
//   wgrad: M = Cout, N = 9*C (= gW's [C][3][3]),   K = N*H*W
#include "common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int LDK = BK + 8;       // LDS row stride in bf16 elements: 80 B rows (16-B aligned fragments, staggered banks)

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

enum PackMode { P_FWD_W, P_FWD_X, P_DG_W, P_DG_G, P_WG_G, P_WG_X };

struct Plan {
  int M, N, K;          // logical GEMM
  int Mp, Np, Kp, S;    // padded sizes, K slices
  size_t a_off, b_off, c_off, bytes;
};

static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

static Plan make_plan(const sgConvDesc* d, int kind) {
  Plan p;
  const int C = d->C1, Co = d->Cout, H = d->H, W = d->W, Nb = d->N;
  if (kind == 0) { p.M = Co; p.N = Nb * H * W; p.K = 9 * C; }
  else if (kind == 1) { p.M = C; p.N = Nb * (H + 2) * (W + 2); p.K = 9 * Co; }
  else { p.M = Co; p.N = 9 * C; p.K = Nb * H * W; }
  p.Mp = (p.M + BM - 1) / BM * BM;
  p.Np = (p.N + BN - 1) / BN * BN;
  const int tiles = (p.Mp / BM) * (p.Np / BN);
  // split K until the grid covers the 256 CUs, keeping every slice >= 1024 deep
  p.S = 1;
  while (p.S < 8 && tiles * p.S < 256 && p.K / (2 * p.S) >= 1024) p.S *= 2;
  const int q = 2 * BK * p.S;
  p.Kp = (p.K + q - 1) / q * q;
  p.a_off = 0;
  p.b_off = al256((size_t)p.Mp * p.Kp * 2);
  p.c_off = p.b_off + al256((size_t)p.Np * p.Kp * 2);
  p.bytes = p.c_off + al256((size_t)p.S * p.Mp * p.Np * sizeof(float));
  return p;
}

static bool shape_ok(const sgConvDesc* d) {
  if (!d) return false;
  if (d->C2 != 0 || d->KS != 3 || d->stride != 1 || d->pad != 1 || !d->pad_reflect || d->upsample != 1 || d->out_pad != 0 ||
      d->x2_broadcast != 0)
    return false;
  if (d->C1 != d->Cout || d->C1 < 64 || d->C1 % 64 != 0 || d->C1 > 4096) return false;
  if (d->N < 1 || d->H < 2 || d->W < 2 || d->OH != d->H || d->OW != d->W) return false;
  // every GEMM extent and every operand image stays well inside 32-bit element indices of one row / 64-bit image offsets
  const int64_t P = (int64_t)d->N * (d->H + 2) * (d->W + 2);
  return P <= (1 << 24) && (int64_t)d->H * d->W <= (1 << 20);
}

__device__ __forceinline__ uint16_t f2bf(float f) {   // round to nearest even, NaN stays NaN (= v_cvt_pk_bf16_f32)
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ int refl(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// One thread writes 8 consecutive k of one row of the [rows_pad][Kp] bf16 image (16-B store); padding is written as zeros.
struct PackArgs {
  const float* src;
  uint16_t* dst;
  int mode, rows, rows_pad, K, Kp, C, Co, H, W;
};

__device__ float pack_value(const PackArgs& a, int row, int k) {
  const int HW = a.H * a.W;
  switch (a.mode) {
    case P_FWD_W:   // A[co][ci*9+t] = W[co][ci][t]: W's own layout
      return a.src[(size_t)row * a.K + k];
    case P_DG_W: {  // A[ci][co*9+t] = W[co][ci][t]
      const int co = k / 9, t = k - co * 9;
      return a.src[((size_t)co * a.C + row) * 9 + t];
    }
    case P_FWD_X: { // B[p][ci*9+t] = reflectpad(x)[n][ci][h+kh][w+kw]
      const int ci = k / 9, t = k - ci * 9, kh = t / 3, kw = t - kh * 3;
      const int n = row / HW, hw = row - n * HW, h = hw / a.W, w = hw - h * a.W;
      return a.src[(((size_t)n * a.C + ci) * a.H + refl(h + kh - 1, a.H)) * a.W + refl(w + kw - 1, a.W)];
    }
    case P_DG_G: {  // B[q][co*9+t] = gy[n][co][r-kh][c-kw] (0 outside): q on the (H+2) x (W+2) padded grid
      const int co = k / 9, t = k - co * 9, kh = t / 3, kw = t - kh * 3;
      const int Q = (a.H + 2) * (a.W + 2), n = row / Q, rc = row - n * Q, r = rc / (a.W + 2), c = rc - r * (a.W + 2);
      const int oh = r - kh, ow = c - kw;
      if (oh < 0 || oh >= a.H || ow < 0 || ow >= a.W) return 0.f;
      return a.src[(((size_t)n * a.Co + co) * a.H + oh) * a.W + ow];
    }
    case P_WG_G: {  // A[co][p] = gy[n][co][hw]
      const int n = k / HW, hw = k - n * HW;
      return a.src[((size_t)n * a.Co + row) * HW + hw];
    }
    default: {      // P_WG_X: B[ci*9+t][p] = reflectpad(x)[n][ci][h+kh][w+kw]
      const int ci = row / 9, t = row - ci * 9, kh = t / 3, kw = t - kh * 3;
      const int n = k / HW, hw = k - n * HW, h = hw / a.W, w = hw - h * a.W;
      return a.src[(((size_t)n * a.C + ci) * a.H + refl(h + kh - 1, a.H)) * a.W + refl(w + kw - 1, a.W)];
    }
  }
}

__global__ __launch_bounds__(256) void k_pack(PackArgs a) {
  const int kc = a.Kp / 8;
  const size_t total = (size_t)a.rows_pad * kc;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / kc), k0 = (int)(i - (size_t)row * kc) * 8;
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int k = k0 + 2 * j;
      const float lo = (row < a.rows && k < a.K) ? pack_value(a, row, k) : 0.f;
      const float hi = (row < a.rows && k + 1 < a.K) ? pack_value(a, row, k + 1) : 0.f;
      v[j] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
    }
    *reinterpret_cast<uint4*>(a.dst + (size_t)row * a.Kp + k0) = make_uint4(v[0], v[1], v[2], v[3]);
  }
}

struct Stage {
  uint4 a0, a1, b0, b1;
};

// One 32-deep K step on LDS buffer CUR, with the global loads of step kt + 1 in flight meanwhile and written to the other
// buffer afterwards.  The last step re-loads its own tile instead of branching (same addresses: in bounds; the write lands in a
// buffer nobody reads again), so the staging registers never need a conditional path.
template <int CUR>
__device__ __forceinline__ void step(uint16_t (*lds)[2][BM * LDK], const uint16_t* ga0, const uint16_t* ga1,
                                     const uint16_t* gb0, const uint16_t* gb1, int so0, int so1, Stage& st,
                                     f32x4 (&acc)[4][4], int wm, int wn, int fr, int kt, int nk) {
  const size_t ko = (size_t)(kt + 1 < nk ? kt + 1 : kt) * BK;
  st.a0 = *reinterpret_cast<const uint4*>(ga0 + ko);
  st.a1 = *reinterpret_cast<const uint4*>(ga1 + ko);
  st.b0 = *reinterpret_cast<const uint4*>(gb0 + ko);
  st.b1 = *reinterpret_cast<const uint4*>(gb1 + ko);
  bf16x8 fa[4], fb[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    fa[i] = *reinterpret_cast<const bf16x8*>(&lds[CUR][0][(wm * 64 + i * 16) * LDK + fr]);
    fb[i] = *reinterpret_cast<const bf16x8*>(&lds[CUR][1][(wn * 64 + i * 16) * LDK + fr]);
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
  *reinterpret_cast<uint4*>(&lds[CUR ^ 1][0][so0]) = st.a0;
  *reinterpret_cast<uint4*>(&lds[CUR ^ 1][0][so1]) = st.a1;
  *reinterpret_cast<uint4*>(&lds[CUR ^ 1][1][so0]) = st.b0;
  *reinterpret_cast<uint4*>(&lds[CUR ^ 1][1][so1]) = st.b1;
  __syncthreads();
}

// slab[z][m][n] = sum_{k in slice z} A[m][k] * B[n][k]; A [Mp][Kp], B [Np][Kp] bf16, every extent a multiple of its tile
// (the packs zero-pad), so the kernel has no bounds checks.  256 threads = 4 waves in 2 x 2, each wave 64 x 64 = 4 x 4
// MFMA 16x16x32 tiles; LDS double-buffered with register staging, one barrier per 32-deep K step.
__global__ __launch_bounds__(256) void k_gemm(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                                              float* __restrict__ slab, int Mp, int Np, int Kp, int kslice) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][BM * LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN, kb = blockIdx.z * kslice, nk = kslice / BK;
  // staging: 128 rows x 4 16-B chunks per operand = 2 chunks per thread (rows tid / 4 and 64 + tid / 4)
  const int srow = tid >> 2, scol = (tid & 3) * 8;
  const uint16_t* ga0 = A + (size_t)(m0 + srow) * Kp + kb + scol;
  const uint16_t* ga1 = ga0 + (size_t)64 * Kp;
  const uint16_t* gb0 = B + (size_t)(n0 + srow) * Kp + kb + scol;
  const uint16_t* gb1 = gb0 + (size_t)64 * Kp;
  const int so0 = srow * LDK + scol, so1 = so0 + 64 * LDK;
  Stage st;
  st.a0 = *reinterpret_cast<const uint4*>(ga0);
  st.a1 = *reinterpret_cast<const uint4*>(ga1);
  st.b0 = *reinterpret_cast<const uint4*>(gb0);
  st.b1 = *reinterpret_cast<const uint4*>(gb1);
  *reinterpret_cast<uint4*>(&lds[0][0][so0]) = st.a0;
  *reinterpret_cast<uint4*>(&lds[0][0][so1]) = st.a1;
  *reinterpret_cast<uint4*>(&lds[0][1][so0]) = st.b0;
  *reinterpret_cast<uint4*>(&lds[0][1][so1]) = st.b1;
  __syncthreads();

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // fragment of lane l: row (l & 15) of a 16-row block, k = 8 * (l >> 4) .. + 7
  const int fr = (lane & 15) * LDK + (lane >> 4) * 8;

  // two K steps per trip so that the LDS buffer of each step is a compile-time choice (nk is even: kslice % 64 == 0)
  for (int kt = 0; kt < nk; kt += 2) {
    step<0>(lds, ga0, ga1, gb0, gb1, so0, so1, st, acc, wm, wn, fr, kt, nk);
    step<1>(lds, ga0, ga1, gb0, gb1, so0, so1, st, acc, wm, wn, fr, kt + 1, nk);
  }
  // C/D map of 16x16x32: col = lane & 15 (-> n), row = (lane >> 4) * 4 + r (-> m)
  float* out = slab + (size_t)blockIdx.z * Mp * Np;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int m = m0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r, n = n0 + wn * 64 + j * 16 + (lane & 15);
        out[(size_t)m * Np + n] = acc[i][j][r];
      }
}

// out[(n / nper)][m][n % nper] = sum_z slab[z][m][n] (+ bias[m]), z in order: fwd (nper = H*W) and wgrad (nper = N = 9*C)
__global__ __launch_bounds__(256) void k_reduce(const float* __restrict__ slab, const float* __restrict__ bias,
                                                float* __restrict__ out, int M, int N, int Mp, int Np, int S, int nper) {
  const size_t total = (size_t)M * N;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(i / N), n = (int)(i - (size_t)m * N);
    float v = slab[(size_t)m * Np + n];
    for (int z = 1; z < S; z++) v += slab[((size_t)z * Mp + m) * Np + n];
    if (bias) v += bias[m];
    const int b = n / nper, q = n - b * nper;
    out[((size_t)b * M + m) * nper + q] = v;
  }
}

// gx[b][c][h][w] = sum of the padded-grid gradient over the padded positions that reflect onto (h, w): row h + 1, plus row 0
// when h == 1 (reflect(-1) = 1), plus row H + 1 when h == H - 2 (reflect(H) = H - 2); the same for columns.  Fixed order.
__global__ __launch_bounds__(256) void k_fold(const float* __restrict__ slab, float* __restrict__ gx, int Nb, int C, int H,
                                              int W, int Mp, int Np, int S) {
  const size_t total = (size_t)Nb * C * H * W;
  const int W2 = W + 2, Q = (H + 2) * W2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int w = (int)(i % W), h = (int)((i / W) % H), c = (int)((i / ((size_t)W * H)) % C), b = (int)(i / ((size_t)W * H * C));
    int rs[3], cs[3], nr = 0, nc = 0;
    rs[nr++] = h + 1;
    if (h == 1) rs[nr++] = 0;
    if (h == H - 2) rs[nr++] = H + 1;
    cs[nc++] = w + 1;
    if (w == 1) cs[nc++] = 0;
    if (w == W - 2) cs[nc++] = W + 1;
    float v = 0.f;
    for (int z = 0; z < S; z++) {
      const float* row = slab + ((size_t)z * Mp + c) * Np + (size_t)b * Q;
      for (int a = 0; a < nr; a++)
        for (int e = 0; e < nc; e++) v += row[rs[a] * W2 + cs[e]];
    }
    gx[i] = v;
  }
}

static int grid_for(size_t work) {
  const size_t g = (work + 255) / 256;
  return (int)(g < 8192 ? (g ? g : 1) : 8192);
}

static void pack(int mode, const float* src, uint16_t* dst, int rows, int rows_pad, int K, int Kp, const sgConvDesc* d,
                 hipStream_t s) {
  PackArgs a{src, dst, mode, rows, rows_pad, K, Kp, d->C1, d->Cout, d->H, d->W};
  hipLaunchKernelGGL(k_pack, dim3(grid_for((size_t)rows_pad * (Kp / 8))), dim3(256), 0, s, a);
}

static void gemm(const Plan& p, char* ws, hipStream_t s) {
  hipLaunchKernelGGL(k_gemm, dim3(p.Np / BN, p.Mp / BM, p.S), dim3(256), 0, s, (const uint16_t*)(ws + p.a_off),
                     (const uint16_t*)(ws + p.b_off), (float*)(ws + p.c_off), p.Mp, p.Np, p.Kp, p.Kp / p.S);
}

}  // namespace

extern "C" int sg_conv3x3r_bf16_supported(const sgConvDesc* d) { return shape_ok(d) ? 1 : 0; }

extern "C" size_t sg_conv3x3r_bf16_ws_bytes(const sgConvDesc* d) {
  if (!shape_ok(d)) return 0;
  size_t b = sg_channel_sum_ws_bytes(d->Cout);
  for (int kind = 0; kind < 3; kind++) {
    const size_t k = make_plan(d, kind).bytes;
    b = k > b ? k : b;
  }
  return b;
}

extern "C" int sg_conv3x3r_bf16_fwd(const sgConvDesc* d, const float* x, const float* w, const float* bias, float* y,
                                    void* ws, size_t ws_bytes, sgStream stream) {
  SG_ARG_CHECK(shape_ok(d), "sg_conv3x3r_bf16_fwd: unsupported shape");
  SG_ARG_CHECK(x && w && y && ws, "sg_conv3x3r_bf16_fwd: null pointer");
  SG_ARG_CHECK(ws_bytes >= sg_conv3x3r_bf16_ws_bytes(d), "sg_conv3x3r_bf16_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const Plan p = make_plan(d, 0);
  char* wsc = (char*)ws;
  pack(P_FWD_W, w, (uint16_t*)(wsc + p.a_off), p.M, p.Mp, p.K, p.Kp, d, s);
  pack(P_FWD_X, x, (uint16_t*)(wsc + p.b_off), p.N, p.Np, p.K, p.Kp, d, s);
  gemm(p, wsc, s);
  hipLaunchKernelGGL(k_reduce, dim3(grid_for((size_t)p.M * p.N)), dim3(256), 0, s, (const float*)(wsc + p.c_off), bias, y,
                     p.M, p.N, p.Mp, p.Np, p.S, d->H * d->W);
  SG_LAUNCH_CHECK("sg_conv3x3r_bf16_fwd");
  return 0;
}

extern "C" int sg_conv3x3r_bf16_dgrad(const sgConvDesc* d, const float* gy, const float* w, float* gx, void* ws,
                                      size_t ws_bytes, sgStream stream) {
  SG_ARG_CHECK(shape_ok(d), "sg_conv3x3r_bf16_dgrad: unsupported shape");
  SG_ARG_CHECK(gy && w && gx && ws, "sg_conv3x3r_bf16_dgrad: null pointer");
  SG_ARG_CHECK(ws_bytes >= sg_conv3x3r_bf16_ws_bytes(d), "sg_conv3x3r_bf16_dgrad: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const Plan p = make_plan(d, 1);
  char* wsc = (char*)ws;
  pack(P_DG_W, w, (uint16_t*)(wsc + p.a_off), p.M, p.Mp, p.K, p.Kp, d, s);
  pack(P_DG_G, gy, (uint16_t*)(wsc + p.b_off), p.N, p.Np, p.K, p.Kp, d, s);
  gemm(p, wsc, s);
  hipLaunchKernelGGL(k_fold, dim3(grid_for((size_t)d->N * d->C1 * d->H * d->W)), dim3(256), 0, s,
                     (const float*)(wsc + p.c_off), gx, d->N, d->C1, d->H, d->W, p.Mp, p.Np, p.S);
  SG_LAUNCH_CHECK("sg_conv3x3r_bf16_dgrad");
  return 0;
}

extern "C" int sg_conv3x3r_bf16_wgrad(const sgConvDesc* d, const float* gy, const float* x, float* gw, float* gb, void* ws,
                                      size_t ws_bytes, sgStream stream) {
  SG_ARG_CHECK(shape_ok(d), "sg_conv3x3r_bf16_wgrad: unsupported shape");
  SG_ARG_CHECK(gy && x && gw && ws, "sg_conv3x3r_bf16_wgrad: null pointer");
  SG_ARG_CHECK(ws_bytes >= sg_conv3x3r_bf16_ws_bytes(d), "sg_conv3x3r_bf16_wgrad: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const Plan p = make_plan(d, 2);
  char* wsc = (char*)ws;
  pack(P_WG_G, gy, (uint16_t*)(wsc + p.a_off), p.M, p.Mp, p.K, p.Kp, d, s);
  pack(P_WG_X, x, (uint16_t*)(wsc + p.b_off), p.N, p.Np, p.K, p.Kp, d, s);
  gemm(p, wsc, s);
  hipLaunchKernelGGL(k_reduce, dim3(grid_for((size_t)p.M * p.N)), dim3(256), 0, s, (const float*)(wsc + p.c_off),
                     (const float*)nullptr, gw, p.M, p.N, p.Mp, p.Np, p.S, p.N);
  SG_LAUNCH_CHECK("sg_conv3x3r_bf16_wgrad");
  // the bias gradient (fp32 sum of gy): stream-ordered after the reduce, so the workspace is free again
  if (gb) return sg_channel_sum(gy, gb, d->N, d->Cout, d->H * d->W, ws, ws_bytes, stream);
  return 0;
}
