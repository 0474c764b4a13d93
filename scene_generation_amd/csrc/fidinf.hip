// FID-infinity (scene_generation_amd/fidinf.py): the Frechet Inception Distance of every subset of n < D fake rows from two n x n
// Gram matrices that are computed once.  With Z = X - 1 mu_r^T (the fake rows shifted by the REAL mean) and Y = Z Sigma_r,
//
//   sg_fidinf_grams         P = Z Z^T,  G = Y Z^T = Z Sigma_r Z^T                        (x fp32, everything else fp64)
//   sg_fidinf_subset_terms  per subset q of n_q rows: sums[q] = (sum_i P_ii, sum_ij P_ij) and the centred block
//                           M[q] = H G_SS H / (n_q - 1), H = I - 1 1^T / n_q, whose eigenvalues are the non-zero ones of Sigma_r Sigma_S
//
// The three products (Y, P, G) are X Y^T over the feature dimension on the f64 matrix cores (f64_tile.h: one workgroup per 64 x 64
// tile, four waves of 2 x 2 v_mfma_f64_16x16x4_f64 tiles, k ascending).  P and G run over the tile pairs ti <= tj of the block upper
// triangle and write each value to (i, j) and (j, i) -- inside a diagonal tile only the entries i <= j are used -- so both equal their
// transposes bit for bit.  No atomics anywhere: every sum has one owner and a fixed order, a call repeats bit for bit.
#include "f64_tile.h"

namespace {

constexpr int TPB = 256;
constexpr int MR = 32;           // rows of M per workgroup of the centring kernel (its columns: SG_F64_FT)

// z[i][k] = fl64((double)x[i][k] - mu[k]): one rounding.  Workgroup (row i, chunk of 256 columns).
__global__ void __launch_bounds__(TPB) fidinf_shift_kernel(const float* __restrict__ x, int D, size_t ldx, const double* __restrict__ mu,
                                                          double* __restrict__ z) {
  const size_t i = blockIdx.x;
  const int k = (int)blockIdx.y * TPB + (int)threadIdx.x;
  if (k < D) z[i * (size_t)D + k] = (double)x[i * ldx + k] - mu[k];
}

// ab[r][k] = src[row0 + r][k0 + k] of a row-major operand (k contiguous), r < 64, k < 32; zero for rows >= nrows and k >= kc
__device__ __forceinline__ void stage_rows(double* ab, const double* __restrict__ src, int row0, int nrows, size_t ld, int k0, int kc) {
  const int lk = threadIdx.x & (SG_F64_KB - 1), lr = threadIdx.x >> 5;      // column lk of rows lr, lr + 8, ...
#pragma unroll
  for (int p = 0; p < SG_F64_FT / (TPB / SG_F64_KB); ++p) {
    const int r = lr + p * (TPB / SG_F64_KB), g = row0 + r;
    ab[r * SG_F64_LDK + lk] = (lk < kc && g < nrows) ? src[(size_t)g * ld + (size_t)(k0 + lk)] : 0.0;
  }
}

// ab[j][k] = src[k0 + k][col0 + j]: column col0 + j of a row-major matrix as row j of the stage; zero for columns >= ncols and k >= kc
__device__ __forceinline__ void stage_cols(double* ab, const double* __restrict__ src, int col0, int ncols, size_t ld, int k0, int kc) {
  const int j = threadIdx.x & (SG_F64_FT - 1), kq = threadIdx.x >> 6;       // column j (contiguous in memory) of rows kq, kq + 4, ...
#pragma unroll
  for (int p = 0; p < SG_F64_KB / (TPB / SG_F64_FT); ++p) {
    const int k = kq + p * (TPB / SG_F64_FT);
    ab[j * SG_F64_LDK + k] = (k < kc && col0 + j < ncols) ? src[(size_t)(k0 + k) * ld + (size_t)(col0 + j)] : 0.0;
  }
}

// y[i][c] = sum_l z[i][l] sigma[l][c]: workgroup (row tile, column tile)
__global__ void __launch_bounds__(TPB) fidinf_y_kernel(const double* __restrict__ z, int n, int D, const double* __restrict__ sigma,
                                                      double* __restrict__ y) {
  __shared__ double ab[2 * SG_F64_FT * SG_F64_LDK];
  const int bi = blockIdx.x, bj = blockIdx.y;
  f64x4 acc[2][2];
  sg_f64_tile_zero(acc);
  for (int k0 = 0; k0 < D; k0 += SG_F64_KB) {
    const int kc = D - k0 < SG_F64_KB ? D - k0 : SG_F64_KB;
    const int kp = (kc + 3) & ~3;                         // D tail: the k up to the next multiple of 4 are staged as zeros
    __syncthreads();
    stage_rows(ab, z, bi * SG_F64_FT, n, (size_t)D, k0, kc);
    stage_cols(ab + SG_F64_FT * SG_F64_LDK, sigma, bj * SG_F64_FT, D, (size_t)D, k0, kc);
    __syncthreads();
    sg_f64_tile_mma(ab, kp, acc);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wi = wave >> 1, wj = wave & 1, fr = lane & 15, fk = lane >> 4;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = bi * SG_F64_FT + wi * 32 + m * 16 + fk + 4 * reg;
        const int col = bj * SG_F64_FT + wj * 32 + nn * 16 + fr;
        if (row < n && col < D) y[(size_t)row * D + col] = acc[m][nn][reg];
      }
}

// Workgroups [0, ntri): the tile pairs of P = Z Z^T; [ntri, 2 ntri): those of G = Y Z^T.
__global__ void __launch_bounds__(TPB) fidinf_gram_kernel(const double* __restrict__ z, const double* __restrict__ y, int n, int D, int nt,
                                                         int ntri, double* __restrict__ P, double* __restrict__ G) {
  __shared__ double ab[2 * SG_F64_FT * SG_F64_LDK];
  const int which = (int)blockIdx.x >= ntri;
  int ti, tj;
  sg_f64_tile_pair((int)blockIdx.x - which * ntri, nt, ti, tj);
  const double* a = which ? y : z;
  double* out = which ? G : P;
  f64x4 acc[2][2];
  sg_f64_tile_zero(acc);
  for (int k0 = 0; k0 < D; k0 += SG_F64_KB) {
    const int kc = D - k0 < SG_F64_KB ? D - k0 : SG_F64_KB;
    const int kp = (kc + 3) & ~3;
    __syncthreads();
    stage_rows(ab, a, ti * SG_F64_FT, n, (size_t)D, k0, kc);
    stage_rows(ab + SG_F64_FT * SG_F64_LDK, z, tj * SG_F64_FT, n, (size_t)D, k0, kc);
    __syncthreads();
    sg_f64_tile_mma(ab, kp, acc);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wi = wave >> 1, wj = wave & 1, fr = lane & 15, fk = lane >> 4;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int gi = ti * SG_F64_FT + wi * 32 + m * 16 + fk + 4 * reg;
        const int gj = tj * SG_F64_FT + wj * 32 + nn * 16 + fr;
        // a diagonal tile holds (i, j) and (j, i), rounded differently for G: the one with i <= j goes to both places
        if (gi < n && gj < n && (ti < tj || gi <= gj)) out[(size_t)gi * n + gj] = acc[m][nn][reg];
      }
  // the mirror image through LDS (over the operand stage), so that its rows are written contiguously too
  static_assert(SG_F64_FT * (SG_F64_FT + 1) <= 2 * SG_F64_FT * SG_F64_LDK, "the tile lies over the operand stage");
  __syncthreads();                                        // every wave has read its last operands
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        ab[(wi * 32 + m * 16 + fk + 4 * reg) * (SG_F64_FT + 1) + wj * 32 + nn * 16 + fr] = acc[m][nn][reg];
  __syncthreads();
  const int c = threadIdx.x & (SG_F64_FT - 1);            // row r of the mirrored tile = column r of this one; c runs along the lanes
  const int gc = ti * SG_F64_FT + c;
#pragma unroll 4
  for (int r = threadIdx.x >> 6; r < SG_F64_FT; r += TPB / 64) {
    const int gr = tj * SG_F64_FT + r;
    if (gr < n && gc < n && (ti < tj || c < r)) out[(size_t)gr * n + gc] = ab[c * (SG_F64_FT + 1) + r];
  }
}

// the size of subset q as the kernels use it: never beyond the table's row
__device__ __forceinline__ int subset_size(const int* __restrict__ sizes, int q, int smax) {
  const int s = sizes[q];
  return s < 0 ? 0 : (s > smax ? smax : s);
}

// One wave per (subset q, position i): rows[q][0][i] = r_i = sum_j G[t_i][t_j], rows[q][1][i] = sum_j P[t_i][t_j], rows[q][2][i] =
// P[t_i][t_i], j over the subset; lane l takes j = l, l + 64, ... in ascending order, then the butterfly.  A table entry outside
// [0, n) forms no address: its row and column read as zeros.
__global__ void __launch_bounds__(TPB) fidinf_rowsums_kernel(const double* __restrict__ P, const double* __restrict__ G, int n,
                                                            const int* __restrict__ idx, const int* __restrict__ sizes, int smax, int nb,
                                                            double* __restrict__ rows) {
  const int q = blockIdx.x / nb, b = blockIdx.x - q * nb;
  const int i = b * (TPB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int nq = subset_size(sizes, q, smax);
  if (i >= nq) return;                                    // wave-uniform
  const int* tab = idx + (size_t)q * smax;
  const int ri = tab[i];
  const bool oki = ri >= 0 && ri < n;
  double sg = 0.0, sp = 0.0;
  for (int j = lane; j < nq; j += 64) {
    const int rj = tab[j];
    if (oki && rj >= 0 && rj < n) {
      sg += G[(size_t)ri * n + rj];
      sp += P[(size_t)ri * n + rj];
    }
  }
  sg = sg_wave_sum_f64(sg);
  sp = sg_wave_sum_f64(sp);
  if (lane == 0) {
    double* r = rows + (size_t)q * 3 * smax;
    r[i] = sg;
    r[(size_t)smax + i] = sp;
    r[2 * (size_t)smax + i] = oki ? P[(size_t)ri * n + ri] : 0.0;
  }
}

// One workgroup per subset: tot[q] = t = sum_i r_i, sums[q] = (sum_i P_ii, sum_ij P_ij): thread t takes i = t, t + 256, ..., then the
// butterfly of each wave and the four waves as (0 + 1) + (2 + 3).  A size below 2 gives NaNs.
__global__ void __launch_bounds__(TPB) fidinf_totals_kernel(const double* __restrict__ rows, const int* __restrict__ sizes, int smax,
                                                           double* __restrict__ sums, double* __restrict__ tot) {
  __shared__ double red[3][TPB / 64];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nq = subset_size(sizes, q, smax);
  const double* r = rows + (size_t)q * 3 * smax;
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < nq; i += TPB) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] += r[(size_t)c * smax + i];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v[c] = sg_wave_sum_f64(v[c]);
    if (lane == 0) red[c][wave] = v[c];
  }
  __syncthreads();
  if (tid == 0) {
    double t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = (red[c][0] + red[c][1]) + (red[c][2] + red[c][3]);
    const bool ok = nq >= 2;
    tot[q] = ok ? t[0] : __builtin_nan("");
    sums[2 * (size_t)q] = ok ? t[2] : __builtin_nan("");
    sums[2 * (size_t)q + 1] = ok ? t[1] : __builtin_nan("");
  }
}

// M[q][i][j] = ((G[t_i][t_j] - (r_i + r_j) / n_q) + t / n_q^2) / (n_q - 1) for i, j < n_q: workgroup (subset, 32-row block, 64-column
// block); thread = one column, 8 rows.  Symmetric bit for bit: G is, and r_i + r_j commutes.  Nothing is written outside the block.
__global__ void __launch_bounds__(TPB) fidinf_center_kernel(const double* __restrict__ G, int n, const int* __restrict__ idx,
                                                           const int* __restrict__ sizes, int smax, const double* __restrict__ rows,
                                                           const double* __restrict__ tot, int tcols, int tper, double* __restrict__ M) {
  const int q = blockIdx.x / tper, b = blockIdx.x - q * tper;
  const int tr = b / tcols, tc = b - tr * tcols;
  const int nq = subset_size(sizes, q, smax);
  if (nq < 2 || tr * MR >= nq || tc * SG_F64_FT >= nq) return;   // workgroup-uniform: a tile past the ragged edge
  const int j = tc * SG_F64_FT + (threadIdx.x & (SG_F64_FT - 1));
  if (j >= nq) return;                                    // (no barrier below)
  const int* tab = idx + (size_t)q * smax;
  const double* r = rows + (size_t)q * 3 * smax;
  const int cj = tab[j];
  const bool okj = cj >= 0 && cj < n;
  const double rj = r[j], dn = (double)nq, c = tot[q] / (dn * dn), dm = dn - 1.0;
  double* Mq = M + (size_t)q * smax * smax;
#pragma unroll
  for (int p = 0; p < MR / (TPB / SG_F64_FT); ++p) {
    const int i = tr * MR + (threadIdx.x >> 6) + p * (TPB / SG_F64_FT);
    if (i < nq) {
      const int ci = tab[i];
      const double g = (okj && ci >= 0 && ci < n) ? G[(size_t)ci * n + cj] : 0.0;
      Mq[(size_t)i * smax + j] = ((g - (r[i] + rj) / dn) + c) / dm;
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" size_t sg_fidinf_grams_ws_bytes(int n, int D) {
  if (n < 1 || D < 1) return 0;
  return 2 * (size_t)n * (size_t)D * sizeof(double);      // Z, then Y
}

extern "C" int sg_fidinf_grams(const float* x, int n, int D, int ldx, const double* mu, const double* sigma, double* P, double* G,
                               void* ws, size_t ws_bytes, sgStream stream) {
  SG_ARG_CHECK(n >= 2 && D >= 1 && ldx >= D, "sg_fidinf_grams: bad sizes (n=%d D=%d ldx=%d; n >= 2, D >= 1, ldx >= D)", n, D, ldx);
  const long nt = ((long)n + SG_F64_FT - 1) / SG_F64_FT, ntri = nt * (nt + 1) / 2, ntd = ((long)D + SG_F64_FT - 1) / SG_F64_FT;
  SG_ARG_CHECK(2 * ntri <= 2147483647L && ntd <= 65535,
               "sg_fidinf_grams: n=%d rows of D=%d are beyond the launch grid", n, D);
  SG_ARG_CHECK(x && mu && sigma && P && G && ws, "sg_fidinf_grams: null operand");
  SG_ARG_CHECK(aligned(x, 4), "sg_fidinf_grams: x must be 4-byte aligned");
  SG_ARG_CHECK(aligned(mu, 8) && aligned(sigma, 8) && aligned(P, 8) && aligned(G, 8) && aligned(ws, 8),
               "sg_fidinf_grams: mu, sigma, P, G and ws must be 8-byte aligned");
  SG_ARG_CHECK(ws_bytes >= sg_fidinf_grams_ws_bytes(n, D), "sg_fidinf_grams: workspace of %zu bytes, %zu needed", ws_bytes,
               sg_fidinf_grams_ws_bytes(n, D));
  hipStream_t st = (hipStream_t)stream;
  double* z = (double*)ws;
  double* y = z + (size_t)n * (size_t)D;
  const double tiles = (double)nt * ntd + 2.0 * ntri;
  SgProfScope prof(SG_K_FIDINF_GRAMS, st, 2.0 * tiles * SG_F64_FT * SG_F64_FT * D, 8.0 * tiles * 2.0 * SG_F64_FT * D + 4.0 * (double)n * D);
  hipLaunchKernelGGL(fidinf_shift_kernel, dim3((unsigned)n, (unsigned)(((long)D + TPB - 1) / TPB)), dim3(TPB), 0, st, x, D, (size_t)ldx, mu, z);
  hipLaunchKernelGGL(fidinf_y_kernel, dim3((unsigned)nt, (unsigned)ntd), dim3(TPB), 0, st, (const double*)z, n, D, sigma, y);
  hipLaunchKernelGGL(fidinf_gram_kernel, dim3((unsigned)(2 * ntri)), dim3(TPB), 0, st, (const double*)z, (const double*)y, n, D, (int)nt,
                     (int)ntri, P, G);
  SG_LAUNCH_CHECK("sg_fidinf_grams");
  return 0;
}

extern "C" size_t sg_fidinf_subset_terms_ws_bytes(int S, int smax) {
  if (S < 1 || smax < 1) return 0;
  return ((size_t)S * 3 * (size_t)smax + (size_t)S) * sizeof(double);      // the three row vectors of every subset, then t
}

extern "C" int sg_fidinf_subset_terms(const double* P, const double* G, int n, const int* idx, const int* sizes, int S, int smax, double* M,
                                      double* sums, void* ws, size_t ws_bytes, sgStream stream) {
  SG_ARG_CHECK(n >= 2 && S >= 0 && smax >= 2, "sg_fidinf_subset_terms: bad sizes (n=%d S=%d smax=%d; n >= 2, S >= 0, smax >= 2)", n, S, smax);
  if (S == 0) return 0;
  const long nb = ((long)smax + TPB / 64 - 1) / (TPB / 64);
  const long tcols = ((long)smax + SG_F64_FT - 1) / SG_F64_FT, trows = ((long)smax + MR - 1) / MR, tper = tcols * trows;
  SG_ARG_CHECK((double)S * (double)nb <= 2147483647.0 && (double)S * (double)tper <= 2147483647.0,
               "sg_fidinf_subset_terms: S=%d subsets of up to smax=%d rows are beyond the launch grid", S, smax);
  SG_ARG_CHECK(P && G && idx && sizes && M && sums && ws, "sg_fidinf_subset_terms: null operand");
  SG_ARG_CHECK(aligned(idx, 4) && aligned(sizes, 4), "sg_fidinf_subset_terms: idx and sizes must be 4-byte aligned");
  SG_ARG_CHECK(aligned(P, 8) && aligned(G, 8) && aligned(M, 8) && aligned(sums, 8) && aligned(ws, 8),
               "sg_fidinf_subset_terms: P, G, M, sums and ws must be 8-byte aligned");
  SG_ARG_CHECK(ws_bytes >= sg_fidinf_subset_terms_ws_bytes(S, smax), "sg_fidinf_subset_terms: workspace of %zu bytes, %zu needed", ws_bytes,
               sg_fidinf_subset_terms_ws_bytes(S, smax));
  hipStream_t st = (hipStream_t)stream;
  double* rows = (double*)ws;
  double* tot = rows + (size_t)S * 3 * (size_t)smax;
  const double cells = (double)S * smax * smax;
  SgProfScope prof(SG_K_FIDINF_TERMS, st, 6.0 * cells, 32.0 * cells);
  hipLaunchKernelGGL(fidinf_rowsums_kernel, dim3((unsigned)(S * nb)), dim3(TPB), 0, st, P, G, n, idx, sizes, smax, (int)nb, rows);
  hipLaunchKernelGGL(fidinf_totals_kernel, dim3((unsigned)S), dim3(TPB), 0, st, (const double*)rows, sizes, smax, sums, tot);
  hipLaunchKernelGGL(fidinf_center_kernel, dim3((unsigned)(S * tper)), dim3(TPB), 0, st, G, n, idx, sizes, smax, (const double*)rows,
                     (const double*)tot, (int)tcols, (int)tper, M);
  SG_LAUNCH_CHECK("sg_fidinf_subset_terms");
  return 0;
}
