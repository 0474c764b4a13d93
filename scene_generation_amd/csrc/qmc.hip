// Quasi-random inputs of the generator (scene_generation_amd/qmc.py): one scrambled Sobol point per image, made and consumed on the
// device.  sg_sobol_points writes the 30-bit integer states of a run of points from the direction numbers and the digital shift of a
// torch.quasirandom.SobolEngine; sg_qmc_unpack cuts the points of a batch into the mask-noise rows (inverse normal CDF in fp64), the
// per-object bank picks and the per-object attribute uniforms; sg_bank_draw scales a pick to a row of the object's class and copies
// that row out of the packed appearance bank.  The exact definitions are the comment of the three entry points in
// include/sg2im_hip.h.
//
// Integer arithmetic but for normcdfinv; every output element is written by exactly one thread with an ordinary store; no atomics, no
// LDS, no scratch.  Results are bit-identical from run to run.  Nothing here allocates or synchronises.  The kernels move a few
// kilobytes: they sit at the launch floor, and are laid out for clarity and for uniform control flow, not for bandwidth.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int DIMS_PER_WG = 128;
constexpr int MAXBIT = SG_QMC_MAXBIT;
constexpr int64_t NPOINTS = (int64_t)1 << MAXBIT;

#define QMC_CHECK(code, cond, ...)  \
  do {                              \
    if (!(cond)) {                  \
      sg_set_error(__VA_ARGS__);    \
      return (code);                \
    }                               \
  } while (0)

// Workgroup (tile of DIMS_PER_WG dimensions; point i = blockIdx.y, blockIdx.y + gridDim.y, ...): a thread per dimension.  g is the
// same in every thread of the workgroup, so the test of each bit is a scalar branch and only the set bits load a direction number.
__global__ void __launch_bounds__(DIMS_PER_WG) sobol_points_kernel(const int32_t* __restrict__ dirs, const int32_t* __restrict__ shift,
                                                                  int32_t* __restrict__ out, long long first, long long n, int D,
                                                                  int ld) {
  const int d = (int)blockIdx.x * DIMS_PER_WG + (int)threadIdx.x;
  if (d >= D) return;
  const int32_t* dir = dirs + (size_t)d * MAXBIT;
  const int32_t sh = shift[d];
  for (long long i = blockIdx.y; i < n; i += gridDim.y) {
    const unsigned k = (unsigned)(first + i);             // < 2^30
    const unsigned g = k ^ (k >> 1);
    int32_t x = sh;
#pragma unroll
    for (int b = 0; b < MAXBIT; ++b)
      if ((g >> b) & 1u) x ^= dir[b];
    out[(size_t)i * (size_t)ld + (size_t)d] = x;
  }
}

// A thread per element of noise (the first N * noise_dim threads), then a thread per object.
__global__ void __launch_bounds__(TPB) qmc_unpack_kernel(const int32_t* __restrict__ points, int ld, const int64_t* __restrict__ obj_to_img,
                                                        const int32_t* __restrict__ seg_off, float* __restrict__ noise,
                                                        int32_t* __restrict__ pick, float* __restrict__ u, int N, int O, int noise_dim,
                                                        int max_objects, int n_noise, FastDiv fd) {
  const int t = (int)blockIdx.x * TPB + (int)threadIdx.x;
  if (t < n_noise) {
    const int n = (int)fd.div((unsigned)t), d = t - n * noise_dim;
    const int32_t x = points[(size_t)n * (size_t)ld + (size_t)d];
    noise[t] = (float)normcdfinv(((double)x + 0.5) * 0x1p-30);
    return;
  }
  const int o = t - n_noise;
  if (o >= O) return;
  const int64_t n = obj_to_img[o];
  int32_t p = -1;
  float u0 = 0.f, u1 = 0.f;
  if (n >= 0 && n < (int64_t)N) {
    const int j = o - seg_off[n];
    if (j >= 0 && j < max_objects) {
      const int32_t* row = points + (size_t)n * (size_t)ld + (size_t)noise_dim + 3 * (size_t)j;
      p = row[0];
      u0 = (float)(row[1] >> 6) * 0x1p-24f;               // a 24-bit integer: exact, and below 1
      u1 = (float)(row[2] >> 6) * 0x1p-24f;
    }
  }
  pick[o] = p;
  u[2 * (size_t)o] = u0;
  u[2 * (size_t)o + 1] = u1;
}

template <int V> struct Vec;
template <> struct Vec<4> { typedef float4 type; };
template <> struct Vec<2> { typedef float2 type; };
template <> struct Vec<1> { typedef float type; };
__device__ __forceinline__ void clear(float4& v) { v.x = v.y = v.z = v.w = 0.f; }
__device__ __forceinline__ void clear(float2& v) { v.x = v.y = 0.f; }
__device__ __forceinline__ void clear(float& v) { v = 0.f; }

// A thread per (object, group of V adjacent columns); the thread of group 0 also writes row_idx.  V divides rep and both bases are
// 4 V-byte aligned (the launcher's choice), so every access of every row is aligned.
template <int V>
__global__ void __launch_bounds__(TPB) bank_draw_kernel(const float* __restrict__ bank, const int64_t* __restrict__ class_off,
                                                       const int64_t* __restrict__ objs, const int32_t* __restrict__ pick,
                                                       int32_t* __restrict__ row_idx, float* __restrict__ rows, int O, int C, int rep,
                                                       long long R, int groups, FastDiv fd) {
  typedef typename Vec<V>::type vec_t;
  const int e = (int)blockIdx.x * TPB + (int)threadIdx.x;
  if (e >= O * groups) return;
  const int o = (int)fd.div((unsigned)e), gcol = e - o * groups;
  const int64_t c = objs[o];
  const int32_t p = pick[o];
  long long idx = -1, src = -1;
  if (c >= 0 && c < (int64_t)C && p >= 0 && (long long)p < NPOINTS) {
    const long long lo = class_off[c], nrows = class_off[c + 1] - lo;
    if (nrows > 0 && nrows < ((long long)1 << 31)) {
      idx = ((long long)p * nrows) >> MAXBIT;             // < nrows
      src = lo + idx;
      if (src < 0 || src >= R) idx = src = -1;
    }
  }
  vec_t v;
  clear(v);
  if (src >= 0) v = *reinterpret_cast<const vec_t*>(bank + (size_t)src * (size_t)rep + (size_t)gcol * V);
  *reinterpret_cast<vec_t*>(rows + (size_t)o * (size_t)rep + (size_t)gcol * V) = v;
  if (gcol == 0) row_idx[o] = (int32_t)idx;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int sg_sobol_points(const int32_t* dirs, const int32_t* shift, int32_t* out, int64_t first, int64_t n, int D, int ld,
                               sgStream stream) {
  QMC_CHECK(SG_QMC_ERR_COUNT, n >= 0, "sg_sobol_points: n=%lld is negative", (long long)n);
  QMC_CHECK(SG_QMC_ERR_DIMS, D >= 1 && D <= SG_QMC_MAX_DIMS, "sg_sobol_points: D=%d must be in 1..%d", D, SG_QMC_MAX_DIMS);
  QMC_CHECK(SG_QMC_ERR_LD, ld >= D, "sg_sobol_points: row stride ld=%d is below D=%d", ld, D);
  QMC_CHECK(SG_QMC_ERR_RANGE, first >= 0 && first <= NPOINTS && n <= NPOINTS - first,
            "sg_sobol_points: points %lld .. %lld + %lld leave the sequence's 2^%d points", (long long)first, (long long)first,
            (long long)n, MAXBIT);
  if (n == 0) return 0;
  QMC_CHECK(SG_QMC_ERR_NULL, dirs && shift && out, "sg_sobol_points: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_OTHER, s, 0.0, 4.0 * (double)n * D + 124.0 * D);
  const dim3 grid((unsigned)sg_cdiv(D, DIMS_PER_WG), (unsigned)(n < 65535 ? n : 65535));
  hipLaunchKernelGGL(sobol_points_kernel, grid, dim3(DIMS_PER_WG), 0, s, dirs, shift, out, (long long)first, (long long)n, D, ld);
  SG_LAUNCH_CHECK("sg_sobol_points");
  return 0;
}

extern "C" int sg_qmc_unpack(const int32_t* points, int ld, const int64_t* obj_to_img, const int32_t* seg_off, float* noise, int32_t* pick,
                             float* u, int N, int O, int noise_dim, int max_objects, sgStream stream) {
  QMC_CHECK(SG_QMC_ERR_COUNT, N >= 0 && O >= 0, "sg_qmc_unpack: bad counts (N=%d O=%d)", N, O);
  const int64_t D = (int64_t)noise_dim + 3 * (int64_t)max_objects;
  QMC_CHECK(SG_QMC_ERR_DIMS, noise_dim >= 0 && max_objects >= 0 && D >= 1 && D <= SG_QMC_MAX_DIMS,
            "sg_qmc_unpack: noise_dim=%d + 3 * max_objects=%d must be in 1..%d, neither negative", noise_dim, max_objects, SG_QMC_MAX_DIMS);
  QMC_CHECK(SG_QMC_ERR_LD, (int64_t)ld >= D, "sg_qmc_unpack: row stride ld=%d is below noise_dim + 3 * max_objects = %lld", ld, (long long)D);
  const int64_t n_noise = (int64_t)N * noise_dim, total = n_noise + O;
  QMC_CHECK(SG_QMC_ERR_COUNT, total < ((int64_t)1 << 31), "sg_qmc_unpack: N * noise_dim + O must stay below 2^31 (N=%d O=%d)", N, O);
  if (total == 0) return 0;
  QMC_CHECK(SG_QMC_ERR_NULL, (N == 0 || (points && seg_off)) && (n_noise == 0 || noise) && (O == 0 || (obj_to_img && pick && u)),
            "sg_qmc_unpack: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_OTHER, s, 0.0, 8.0 * (double)n_noise + 32.0 * O);
  hipLaunchKernelGGL(qmc_unpack_kernel, dim3((unsigned)sg_cdiv(total, TPB)), dim3(TPB), 0, s, points, ld, obj_to_img, seg_off, noise, pick,
                     u, N, O, noise_dim, max_objects, (int)n_noise, FastDiv((unsigned)(noise_dim > 0 ? noise_dim : 1)));
  SG_LAUNCH_CHECK("sg_qmc_unpack");
  return 0;
}

extern "C" int sg_bank_draw(const float* bank, const int64_t* class_off, const int64_t* objs, const int32_t* pick, int32_t* row_idx,
                            float* rows, int O, int C, int rep, int64_t R, sgStream stream) {
  QMC_CHECK(SG_QMC_ERR_COUNT, O >= 0 && R >= 0, "sg_bank_draw: bad counts (O=%d R=%lld)", O, (long long)R);
  QMC_CHECK(SG_QMC_ERR_DIMS, C >= 1 && rep >= 1, "sg_bank_draw: C=%d and rep=%d must be at least 1", C, rep);
  QMC_CHECK(SG_QMC_ERR_COUNT, (int64_t)O * rep < ((int64_t)1 << 31), "sg_bank_draw: O * rep must stay below 2^31 (O=%d rep=%d)", O, rep);
  if (O == 0) return 0;
  QMC_CHECK(SG_QMC_ERR_NULL, (R == 0 || bank) && class_off && objs && pick && row_idx && rows, "sg_bank_draw: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_OTHER, s, 0.0, (double)O * (8.0 * rep + 32.0));
  const int V = (rep % 4 == 0 && aligned(bank, 16) && aligned(rows, 16)) ? 4 : ((rep % 2 == 0 && aligned(bank, 8) && aligned(rows, 8)) ? 2 : 1);
  const int groups = rep / V;
  const dim3 grid((unsigned)sg_cdiv((int64_t)O * groups, TPB));
  const FastDiv fd((unsigned)groups);
  if (V == 4)
    hipLaunchKernelGGL(bank_draw_kernel<4>, grid, dim3(TPB), 0, s, bank, class_off, objs, pick, row_idx, rows, O, C, rep, (long long)R, groups, fd);
  else if (V == 2)
    hipLaunchKernelGGL(bank_draw_kernel<2>, grid, dim3(TPB), 0, s, bank, class_off, objs, pick, row_idx, rows, O, C, rep, (long long)R, groups, fd);
  else
    hipLaunchKernelGGL(bank_draw_kernel<1>, grid, dim3(TPB), 0, s, bank, class_off, objs, pick, row_idx, rows, O, C, rep, (long long)R, groups, fd);
  SG_LAUNCH_CHECK("sg_bank_draw");
  return 0;
}
