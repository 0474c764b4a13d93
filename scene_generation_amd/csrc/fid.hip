// The Frechet Inception Distance (scene_generation_amd/fid.py): the float64 raw moments of the pooled Inception features, kept on the
// device for the whole evaluation.
//
//   sg_fid_moments_update    sum[j] += sum_k x[k][j],  outer[i][j] += sum_k x[k][i] x[k][j] for i <= j  (x fp32, the moments fp64)
//   sg_fid_moments_finalize  mu = sum / n,  sigma = (outer - sum sum^T / n) / (n - 1), the full symmetric matrix (numpy.cov, ddof 1)
//
// The update is a rank-`rows` update of a D x D matrix on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).  Each fp32 value is converted
// to fp64, so every product is exact and only the sums round.  One workgroup owns one 64 x 64 tile pair (ti <= tj) of the block upper
// triangle: it reads that tile of ``outer``, adds its products and writes the tile back.  No atomics, k in ascending order: the same
// call sequence gives bit-identical moments.  Raw (unshifted) moments, so two accumulators merge by plain addition.
//
// The 64 x 64 tile (SG_F64_FT: four waves, 2 x 2, each 32 x 32 = 2 x 2 MFMA tiles), the f64 MFMA's lane map and the tile-pair enumeration
// are f64_tile.h's; the stage here is k-major, so the product loop is this file's own.
#include "f64_tile.h"

namespace {

constexpr int TPB = 256;
constexpr int FKB = 32;          // rows of x staged per pass (the evaluation's batch)
constexpr int FLD = SG_F64_FT + 16;  // LDS row stride in doubles: 640 B, so the two rows a 32-lane half reads (k, k + 1) sit on
                                 // opposite halves of the 64 banks
constexpr int ST = 32;           // tile of the finalize kernel

__global__ void __launch_bounds__(TPB) fid_moments_kernel(const float* __restrict__ x, int rows, int D, size_t ldx, double* sum,
                                                         double* outer, int nt) {
  __shared__ double sA[FKB * FLD];          // sA[k][i] = x[k0 + k][ti * SG_F64_FT + i]  (A of the MFMA is its transpose)
  __shared__ double sB[FKB * FLD];          // sB[k][j] = x[k0 + k][tj * SG_F64_FT + j]
  int ti, tj;
  sg_f64_tile_pair(blockIdx.x, nt, ti, tj);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wj = wave & 1;
  const int c = tid & (SG_F64_FT - 1), r0 = tid >> 6;   // loader: column c of rows r0, r0 + 4, ...
  const int ca = ti * SG_F64_FT + c, cb = tj * SG_F64_FT + c;
  const bool oka = ca < D, okb = cb < D;                // D tail: columns past D are staged as zeros
  const int fr = lane & 15, fk = lane >> 4;
  f64x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};
  double colsum = 0.0;
  for (int k0 = 0; k0 < rows; k0 += FKB) {
    const int kc = rows - k0 < FKB ? rows - k0 : FKB;
    const int kp = (kc + 3) & ~3;                       // k tail: the rows up to the next multiple of 4 are staged as zeros
    __syncthreads();
    for (int r = r0; r < kp; r += TPB / SG_F64_FT) {
      const bool okr = r < kc;
      const float* xr = x + (size_t)(k0 + (okr ? r : 0)) * ldx;
      sA[r * FLD + c] = (okr && oka) ? (double)xr[ca] : 0.0;
      sB[r * FLD + c] = (okr && okb) ? (double)xr[cb] : 0.0;
    }
    __syncthreads();
    if (ti == tj && wave == 0)                          // the diagonal workgroups also own their 64 entries of sum
      for (int r = 0; r < kc; ++r) colsum += sA[r * FLD + lane];
    for (int ks = 0; ks < kp; ks += 4) {
      double a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = sA[(ks + fk) * FLD + wi * 32 + m * 16 + fr];
#pragma unroll
      for (int n = 0; n < 2; ++n) b[n] = sB[(ks + fk) * FLD + wj * 32 + n * 16 + fr];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
    }
  }
  // read-modify-write of the tile: C/D of the f64 MFMA has col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = ti * SG_F64_FT + wi * 32 + m * 16 + fk + 4 * reg;
        const int col = tj * SG_F64_FT + wj * 32 + n * 16 + fr;
        if (row < D && col < D) {
          double* p = outer + (size_t)row * D + col;
          *p = *p + acc[m][n][reg];
        }
      }
  if (ti == tj && wave == 0 && ti * SG_F64_FT + lane < D) sum[ti * SG_F64_FT + lane] += colsum;
}

// mu and the full symmetric sigma from the upper triangle of outer.  One workgroup per 32 x 32 tile pair (ti <= tj): it writes the
// tile and, through LDS, its transpose, both with rows contiguous.  A diagonal tile reads (min, max) of its indices, so the lower
// triangle of outer is never read and sigma == sigma^T bit for bit.
__global__ void __launch_bounds__(TPB) fid_finalize_kernel(const double* __restrict__ sum, const double* __restrict__ outer, double n,
                                                          int D, double* __restrict__ mu, double* __restrict__ sigma, int nt) {
  __shared__ double tile[ST][ST + 1];
  int ti, tj;
  sg_f64_tile_pair(blockIdx.x, nt, ti, tj);
  const int cx = threadIdx.x & (ST - 1), ry = threadIdx.x >> 5;
  const int j = tj * ST + cx;
  for (int r = ry; r < ST; r += TPB / ST) {
    const int i = ti * ST + r;
    double v = 0.0;
    if (i < D && j < D) {
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      v = (outer[(size_t)lo * D + hi] - sum[lo] * sum[hi] / n) / (n - 1.0);
      sigma[(size_t)i * D + j] = v;
    }
    tile[r][cx] = v;
  }
  if (ti == tj) {
    if (ry == 0 && j < D) mu[j] = sum[j] / n;
    return;                                             // workgroup-uniform
  }
  __syncthreads();
  const int jt = ti * ST + cx;                          // the transposed tile: rows of tj, columns of ti
  for (int r = ry; r < ST; r += TPB / ST) {
    const int it = tj * ST + r;
    if (it < D && jt < D) sigma[(size_t)it * D + jt] = tile[cx][r];
  }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" int sg_fid_moments_update(const float* x, int rows, int D, int ldx, double* sum, double* outer, sgStream stream) {
  SG_ARG_CHECK(rows >= 0 && D >= 1 && ldx >= D, "sg_fid_moments_update: bad sizes (rows=%d D=%d ldx=%d; D >= 1, ldx >= D)", rows, D, ldx);
  const long nt = (D + SG_F64_FT - 1) / SG_F64_FT;
  SG_ARG_CHECK(nt * (nt + 1) / 2 <= 2147483647L, "sg_fid_moments_update: D=%d is beyond the launch grid", D);
  SG_ARG_CHECK(sum && outer && (rows == 0 || x), "sg_fid_moments_update: null operand");
  SG_ARG_CHECK(aligned8(sum) && aligned8(outer), "sg_fid_moments_update: sum and outer must be 8-byte aligned");
  if (rows == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const double tri = 0.5 * (double)D * ((double)D + 1.0);
  SgProfScope prof(SG_K_FID_MOMENTS, s, 2.0 * rows * tri, 4.0 * (double)rows * D + 16.0 * tri);
  hipLaunchKernelGGL(fid_moments_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(TPB), 0, s, x, rows, D, (size_t)ldx, sum, outer, (int)nt);
  SG_LAUNCH_CHECK("sg_fid_moments_update");
  return 0;
}

extern "C" int sg_fid_moments_finalize(const double* sum, const double* outer, long long n, int D, double* mu, double* sigma,
                                       sgStream stream) {
  SG_ARG_CHECK(n >= 2 && D >= 1, "sg_fid_moments_finalize: bad sizes (n=%lld D=%d; a covariance needs n >= 2)", n, D);
  const long nt = (D + ST - 1) / ST;
  SG_ARG_CHECK(nt * (nt + 1) / 2 <= 2147483647L, "sg_fid_moments_finalize: D=%d is beyond the launch grid", D);
  SG_ARG_CHECK(sum && outer && mu && sigma, "sg_fid_moments_finalize: null operand");
  SG_ARG_CHECK(aligned8(sum) && aligned8(outer) && aligned8(mu) && aligned8(sigma),
               "sg_fid_moments_finalize: sum, outer, mu and sigma must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_FID_MOMENTS, s, 0.0, 12.0 * (double)D * D);
  hipLaunchKernelGGL(fid_finalize_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(TPB), 0, s, sum, outer, (double)n, D, mu, sigma, (int)nt);
  SG_LAUNCH_CHECK("sg_fid_moments_finalize");
  return 0;
}
