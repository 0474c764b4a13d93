// Statistics of all pairs of retained feature rows (scene_generation_amd/featsets.py): the Kernel Inception Distance's polynomial-kernel
// sums and the k-NN manifold estimate behind improved precision / recall and density / coverage.
//
//   sg_feat_poly_sums        per subset q: sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j) over rows gathered
//                            through index tables, k(a, b) = (gamma a.b + coef0)^degree
//   sg_feat_knn_radius       r2[i] = the k-th smallest of { d2(x_i, x_j) : j != i }
//   sg_feat_manifold_counts  count[j] = #{ i : d2(b_j, a_i) <= r2[i] },  mind2[i] = min_j d2(a_i, b_j)
//
// All three are X Y^T over the feature dimension with a small epilogue.  One workgroup owns one 64 x 64 tile of the product: four
// waves, 2 x 2, each 32 x 32 = 2 x 2 tiles of v_mfma_f64_16x16x4_f64.  Each fp32 value is converted to fp64, so every product is exact
// and only the sums round; k runs in ascending order.  The product never leaves the registers: no s x s matrix and no gathered copy
// is written.  No floating-point atomics: the tile sums go to the workspace and are added in a fixed order by a second kernel, the
// top-k lists likewise; the membership counts are integer atomics and the minima are unsigned-integer atomic minima of the bit
// patterns of non-negative doubles (the same order as the values) -- all order-independent, so a call repeats bit for bit.
//
// The tile, its lane map and the step from the LDS stage to the accumulators are f64_tile.h's, shared with fid.hip and fidinf.hip.
#include "f64_tile.h"

namespace {

constexpr int TPB = 256;
constexpr int KMAX = 8;          // longest neighbour list
constexpr int QL = 4;            // threads (column quarters) per row in the neighbour scan

struct Tile {
  double ab[2 * SG_F64_FT * SG_F64_LDK];   // ab[i][k] = row i of the A side, columns k0 .. k0 + 31; the B side from row SG_F64_FT on
  const float* pa[SG_F64_FT];              // the 64 rows of each side (nullptr: a zero row)
  const float* pb[SG_F64_FT];
};

// acc[m][n] = sum_k A[i][k] B[j][k] for the rows T.pa / T.pb name (set, and synchronised, by the caller).  Element reg of acc[m][n] is
// row (wave >> 1) * 32 + m * 16 + (lane >> 4) + 4 * reg, column (wave & 1) * 32 + n * 16 + (lane & 15) of the tile.
__device__ __forceinline__ void tile_product(Tile& T, int D, f64x4 (&acc)[2][2]) {
  const int tid = threadIdx.x;
  const int lk = tid & (SG_F64_KB - 1), lr = tid >> 5;    // loader: column lk of rows lr, lr + 8, ...
  sg_f64_tile_zero(acc);
  for (int k0 = 0; k0 < D; k0 += SG_F64_KB) {
    const int kc = D - k0 < SG_F64_KB ? D - k0 : SG_F64_KB;
    const int kp = (kc + 3) & ~3;                         // D tail: the columns up to the next multiple of 4 are staged as zeros
    const bool okk = lk < kc;
    __syncthreads();
#pragma unroll
    for (int p = 0; p < SG_F64_FT / (TPB / SG_F64_KB); ++p) {
      const int r = lr + p * (TPB / SG_F64_KB);
      const float* ra = T.pa[r];
      const float* rb = T.pb[r];
      T.ab[r * SG_F64_LDK + lk] = (okk && ra) ? (double)ra[k0 + lk] : 0.0;
      T.ab[(SG_F64_FT + r) * SG_F64_LDK + lk] = (okk && rb) ? (double)rb[k0 + lk] : 0.0;
    }
    __syncthreads();
    sg_f64_tile_mma(T.ab, kp, acc);
  }
}

// ---- the KID sums ---------------------------------------------------------------------------------------------------------------------
// Workgroup b of subset q: tiles [0, ntri) are the pairs ti <= tj of x against x, [ntri, 2 ntri) of y against y, the rest the nt x nt
// tiles of x against y.  part[q * T + b] = the tile's sum (off-diagonal tiles of the symmetric cases doubled).
__global__ void __launch_bounds__(TPB) feat_poly_kernel(const float* __restrict__ x, int n, size_t ldx, const float* __restrict__ y, int m,
                                                       size_t ldy, int D, const int* __restrict__ ix, const int* __restrict__ iy, int s,
                                                       int nt, int ntri, int T, double gamma, double coef0, int degree,
                                                       double* __restrict__ part) {
  __shared__ Tile tile;
  __shared__ double red[TPB / 64];
  const int q = blockIdx.x / T, b = blockIdx.x - q * T;
  int which, ti, tj;
  if (b < 2 * ntri) {
    which = b >= ntri;
    sg_f64_tile_pair(b - which * ntri, nt, ti, tj);
  } else {
    which = 2;
    ti = (b - 2 * ntri) / nt;
    tj = (b - 2 * ntri) - ti * nt;
  }
  const int tid = threadIdx.x;
  if (tid < 2 * SG_F64_FT) {                              // the gather: one table entry per tile row, checked before it forms an address
    const bool sideb = tid >= SG_F64_FT;
    const int pos = (sideb ? tj : ti) * SG_F64_FT + (tid & (SG_F64_FT - 1));
    const bool fromy = which == 1 || (which == 2 && sideb);
    const int* tab = fromy ? iy : ix;
    const float* base = fromy ? y : x;
    const size_t ld = fromy ? ldy : ldx;
    const int lim = fromy ? m : n;
    const float* p = nullptr;
    if (pos < s) {
      const int r = tab[(size_t)q * s + pos];
      if (r >= 0 && r < lim) p = base + (size_t)r * ld;   // an index outside the set reads as a zero row
    }
    (sideb ? tile.pb : tile.pa)[tid & (SG_F64_FT - 1)] = p;
  }
  f64x4 acc[2][2];
  tile_product(tile, D, acc);                             // (its first barrier publishes the row pointers)
  const int lane = tid & 63, wave = tid >> 6, wi = wave >> 1, wj = wave & 1, fr = lane & 15, fk = lane >> 4;
  double sum = 0.0;
#pragma unroll
  for (int mm = 0; mm < 2; ++mm)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int pi = ti * SG_F64_FT + wi * 32 + mm * 16 + fk + 4 * reg;
        const int pj = tj * SG_F64_FT + wj * 32 + nn * 16 + fr;
        const double t = gamma * acc[mm][nn][reg] + coef0;
        double v = t;
        for (int e = 1; e < degree; ++e) v *= t;          // repeated multiplication, never pow
        if (pi < s && pj < s && (which == 2 || pi != pj)) sum += v;      // i != j by position
      }
  sum = sg_wave_sum_f64(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    const double t = (red[0] + red[1]) + (red[2] + red[3]);
    part[(size_t)q * T + b] = (which < 2 && ti != tj) ? 2.0 * t : t;
  }
}

// out[q][c] = the tile sums of case c in ascending tile order
__global__ void feat_poly_final_kernel(const double* __restrict__ part, int S, int ntri, int T, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * S) return;
  const int q = t / 3, c = t - 3 * q;
  const int lo = c * ntri, hi = c == 2 ? T : lo + ntri;
  const double* p = part + (size_t)q * T;
  double v = 0.0;
  for (int b = lo; b < hi; ++b) v += p[b];
  out[t] = v;
}

// ---- squared norms ----------------------------------------------------------------------------------------------------------------------
// nrm[r] = sum_k x[r][k]^2 in fp64: one wave per row, lane l takes columns l, l + 64, ... in ascending order
__global__ void __launch_bounds__(TPB) feat_norms_kernel(const float* __restrict__ x, int rows, int D, size_t ldx, double* __restrict__ nrm) {
  const int r = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;                                  // wave-uniform
  const float* p = x + (size_t)r * ldx;
  double v = 0.0;
  for (int k = lane; k < D; k += 64) {
    const double t = (double)p[k];
    v += t * t;
  }
  v = sg_wave_sum_f64(v);
  if (lane == 0) nrm[r] = v;
}

__device__ __forceinline__ double dist2(double na, double nb, double g) {
  const double d = (na + nb) - 2.0 * g;
  return d > 0.0 ? d : 0.0;                               // clamped at (+)0
}

// sorted insertion into an ascending list held in registers (static indices only: no scratch)
__device__ __forceinline__ void topk_insert(double (&best)[KMAX], double v) {
  if (v < best[KMAX - 1]) {
#pragma unroll
    for (int e = 0; e < KMAX; ++e) {
      const double lo = v < best[e] ? v : best[e];
      const double hi = v < best[e] ? best[e] : v;
      best[e] = lo;
      v = hi;
    }
  }
}

// ---- the manifold radii -----------------------------------------------------------------------------------------------------------------
// Workgroup (row block bi, column split z): the 64 rows of block bi against the column tiles z, z + CS, ...  Each distance tile goes
// through LDS (over the operand stage) to four threads per row, which keep the KMAX smallest of their column quarter.  The lists go to
// part[((z * QL + quarter) * KMAX + e) * n + row]; feat_knn_merge_kernel merges the CS * QL lists of a row.
__global__ void __launch_bounds__(TPB) feat_knn_kernel(const float* __restrict__ x, int n, int D, size_t ldx, const double* __restrict__ nrm,
                                                      int ntc, int CS, double* __restrict__ part) {
  __shared__ Tile tile;
  static_assert(sizeof(double) * SG_F64_FT * (SG_F64_FT + 1) <= sizeof(double) * 2 * SG_F64_FT * SG_F64_LDK, "the distance tile lies over the operand stage");
  double* dt = tile.ab;                                   // dt[row][col], row stride SG_F64_FT + 1
  const int bi = blockIdx.x, z = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wi = wave >> 1, wj = wave & 1, fr = lane & 15, fk = lane >> 4;
  const int srow = tid >> 2, sq = tid & 3;                // the scan: row srow of the block, columns sq * 16 .. sq * 16 + 15
  const int grow = bi * SG_F64_FT + srow;
  double best[KMAX];
#pragma unroll
  for (int e = 0; e < KMAX; ++e) best[e] = __builtin_inf();
  for (int tj = z; tj < ntc; tj += CS) {
    __syncthreads();                                      // the previous tile's scan is over: the stage may be overwritten
    if (tid < 2 * SG_F64_FT) {
      const bool sideb = tid >= SG_F64_FT;
      const int r = (sideb ? tj : bi) * SG_F64_FT + (tid & (SG_F64_FT - 1));
      (sideb ? tile.pb : tile.pa)[tid & (SG_F64_FT - 1)] = r < n ? x + (size_t)r * ldx : nullptr;
    }
    f64x4 acc[2][2];
    tile_product(tile, D, acc);
    __syncthreads();                                      // every wave has read its last operands
#pragma unroll
    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int row = wi * 32 + mm * 16 + fk + 4 * reg, col = wj * 32 + nn * 16 + fr;
          const int gi = bi * SG_F64_FT + row, gj = tj * SG_F64_FT + col;
          double d = __builtin_inf();                     // outside the set, or the row itself (by index): never a neighbour
          if (gi < n && gj < n && gi != gj) d = dist2(nrm[gi], nrm[gj], acc[mm][nn][reg]);
          dt[row * (SG_F64_FT + 1) + col] = d;
        }
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < SG_F64_FT / QL; ++c) topk_insert(best, dt[srow * (SG_F64_FT + 1) + sq * (SG_F64_FT / QL) + c]);
  }
  if (grow < n) {
#pragma unroll
    for (int e = 0; e < KMAX; ++e) part[((size_t)(z * QL + sq) * KMAX + e) * n + grow] = best[e];
  }
}

__global__ void feat_knn_merge_kernel(const double* __restrict__ part, int n, int lists, int k, double* __restrict__ r2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double best[KMAX];
#pragma unroll
  for (int e = 0; e < KMAX; ++e) best[e] = __builtin_inf();
  for (int l = 0; l < lists; ++l) {
#pragma unroll
    for (int e = 0; e < KMAX; ++e) topk_insert(best, part[((size_t)l * KMAX + e) * n + i]);
  }
  double v = best[0];
#pragma unroll
  for (int e = 1; e < KMAX; ++e) v = e < k ? best[e] : v; // the k-th smallest, selected without a dynamic register index
  r2[i] = v;
}

// ---- the membership pass ----------------------------------------------------------------------------------------------------------------
__global__ void feat_counts_init_kernel(int* __restrict__ count, int m, unsigned long long* __restrict__ mind2, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m) count[t] = 0;
  if (t < n) mind2[t] = 0x7FF0000000000000ull;            // +inf
}

// Workgroup (ti, tj): references ti * 64 .. against queries tj * 64 ..; rows of the tile are references, columns queries.
__global__ void __launch_bounds__(TPB) feat_counts_kernel(const float* __restrict__ a, int n, size_t lda, const double* __restrict__ r2,
                                                         const float* __restrict__ b, int m, size_t ldb, int D,
                                                         const double* __restrict__ na, const double* __restrict__ nb,
                                                         int* __restrict__ count, unsigned long long* __restrict__ mind2) {
  __shared__ Tile tile;
  const int ti = blockIdx.x, tj = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wi = wave >> 1, wj = wave & 1, fr = lane & 15, fk = lane >> 4;
  if (tid < 2 * SG_F64_FT) {
    const bool sideb = tid >= SG_F64_FT;
    const int r = (sideb ? tj : ti) * SG_F64_FT + (tid & (SG_F64_FT - 1));
    if (sideb) tile.pb[tid & (SG_F64_FT - 1)] = r < m ? b + (size_t)r * ldb : nullptr;
    else tile.pa[tid & (SG_F64_FT - 1)] = r < n ? a + (size_t)r * lda : nullptr;
  }
  f64x4 acc[2][2];
  tile_product(tile, D, acc);
  int cnt[2] = {0, 0};                                    // per column block nn: references of this lane's rows that hold the query
#pragma unroll
  for (int mm = 0; mm < 2; ++mm)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int gi = ti * SG_F64_FT + wi * 32 + mm * 16 + fk + 4 * reg;
      const bool oki = gi < n;
      const double ni = oki ? na[gi] : 0.0, ri = oki ? r2[gi] : 0.0;
      double rmin = __builtin_inf();
#pragma unroll
      for (int nn = 0; nn < 2; ++nn) {
        const int gj = tj * SG_F64_FT + wj * 32 + nn * 16 + fr;
        if (oki && gj < m) {
          const double d = dist2(ni, nb[gj], acc[mm][nn][reg]);
          cnt[nn] += d <= ri ? 1 : 0;
          rmin = d < rmin ? d : rmin;
        }
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {                  // over the 16 lanes that share the row
        const double t = __shfl_xor(rmin, o, 64);
        rmin = t < rmin ? t : rmin;
      }
      // non-negative doubles order like their bit patterns: an integer minimum, independent of the order of arrival
      if (fr == 0 && oki && rmin < __builtin_inf()) atomicMin(mind2 + gi, (unsigned long long)__double_as_longlong(rmin));
    }
#pragma unroll
  for (int nn = 0; nn < 2; ++nn) {
    int c = cnt[nn];
    c += __shfl_xor(c, 16, 64);                           // over the 4 lane groups that share the column
    c += __shfl_xor(c, 32, 64);
    const int gj = tj * SG_F64_FT + wj * 32 + nn * 16 + fr;
    if (fk == 0 && gj < m && c) atomicAdd(count + gj, c);
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }

// column splits of the neighbour sweep: enough workgroups to fill the chip at small n, never more than there are column tiles
inline int knn_splits(int n) {
  const int nb = (n + SG_F64_FT - 1) / SG_F64_FT;
  int cs = (512 + nb - 1) / nb;
  return cs < 1 ? 1 : (cs > nb ? nb : cs);
}

}  // namespace

extern "C" size_t sg_feat_poly_sums_ws_bytes(int S, int s) {
  if (S < 1 || s < 1) return 0;
  const size_t nt = ((size_t)s + SG_F64_FT - 1) / SG_F64_FT;
  return (size_t)S * (nt * (nt + 1) + nt * nt) * sizeof(double);
}

extern "C" int sg_feat_poly_sums(const float* x, int n, int ldx, const float* y, int m, int ldy, int D, const int* ix, const int* iy,
                                 int S, int s, double gamma, double coef0, int degree, double* out, void* ws, size_t ws_bytes,
                                 sgStream stream) {
  SG_ARG_CHECK(S >= 0 && s >= 1 && n >= 1 && m >= 1 && D >= 1 && ldx >= D && ldy >= D,
               "sg_feat_poly_sums: bad sizes (n=%d m=%d D=%d ldx=%d ldy=%d S=%d s=%d; n, m, D, s >= 1, S >= 0, ldx and ldy >= D)", n, m, D,
               ldx, ldy, S, s);
  SG_ARG_CHECK(degree >= 1 && degree <= 4, "sg_feat_poly_sums: degree=%d is outside 1..4", degree);
  if (S == 0) return 0;
  const long nt = ((long)s + SG_F64_FT - 1) / SG_F64_FT, ntri = nt * (nt + 1) / 2, T = 2 * ntri + nt * nt;
  SG_ARG_CHECK((double)S * (double)T <= 2147483647.0, "sg_feat_poly_sums: S=%d subsets of s=%d are beyond the launch grid", S, s);
  SG_ARG_CHECK(x && y && ix && iy && out && ws, "sg_feat_poly_sums: null operand");
  SG_ARG_CHECK(aligned(x, 4) && aligned(y, 4) && aligned(ix, 4) && aligned(iy, 4), "sg_feat_poly_sums: x, y, ix and iy must be 4-byte aligned");
  SG_ARG_CHECK(aligned(out, 8) && aligned(ws, 8), "sg_feat_poly_sums: out and ws must be 8-byte aligned");
  SG_ARG_CHECK(ws_bytes >= sg_feat_poly_sums_ws_bytes(S, s), "sg_feat_poly_sums: workspace of %zu bytes, %zu needed", ws_bytes,
               sg_feat_poly_sums_ws_bytes(S, s));
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  const double pairs = (double)S * (double)T * SG_F64_FT * SG_F64_FT;
  SgProfScope prof(SG_K_FEAT_POLY, st, 2.0 * pairs * D, 4.0 * (double)S * T * 2.0 * SG_F64_FT * D);
  hipLaunchKernelGGL(feat_poly_kernel, dim3((unsigned)(S * T)), dim3(TPB), 0, st, x, n, (size_t)ldx, y, m, (size_t)ldy, D, ix, iy, s, (int)nt,
                     (int)ntri, (int)T, gamma, coef0, degree, part);
  hipLaunchKernelGGL(feat_poly_final_kernel, dim3((unsigned)((3 * (long)S + 255) / 256)), dim3(256), 0, st, part, S, (int)ntri, (int)T, out);
  SG_LAUNCH_CHECK("sg_feat_poly_sums");
  return 0;
}

extern "C" size_t sg_feat_knn_radius_ws_bytes(int n) {
  if (n < 1) return 0;
  return ((size_t)n + (size_t)knn_splits(n) * QL * KMAX * (size_t)n) * sizeof(double);
}

extern "C" int sg_feat_knn_radius(const float* x, int n, int D, int ldx, int k, double* r2, void* ws, size_t ws_bytes, sgStream stream) {
  SG_ARG_CHECK(n >= 0 && D >= 1 && ldx >= D, "sg_feat_knn_radius: bad sizes (n=%d D=%d ldx=%d; n >= 0, D >= 1, ldx >= D)", n, D, ldx);
  if (n == 0) return 0;
  SG_ARG_CHECK(k >= 1 && k <= KMAX && k < n, "sg_feat_knn_radius: k=%d is outside 1..%d or not below n=%d (the row itself is no neighbour)", k,
               KMAX, n);
  SG_ARG_CHECK(x && r2 && ws, "sg_feat_knn_radius: null operand");
  SG_ARG_CHECK(aligned(x, 4) && aligned(r2, 8) && aligned(ws, 8), "sg_feat_knn_radius: x must be 4-byte, r2 and ws 8-byte aligned");
  SG_ARG_CHECK(ws_bytes >= sg_feat_knn_radius_ws_bytes(n), "sg_feat_knn_radius: workspace of %zu bytes, %zu needed", ws_bytes,
               sg_feat_knn_radius_ws_bytes(n));
  hipStream_t st = (hipStream_t)stream;
  const int nb = (n + SG_F64_FT - 1) / SG_F64_FT, CS = knn_splits(n);
  double* nrm = (double*)ws;
  double* part = nrm + n;
  const double pairs = (double)nb * nb * SG_F64_FT * SG_F64_FT;
  SgProfScope prof(SG_K_FEAT_MANIFOLD, st, 2.0 * pairs * D, 4.0 * (double)nb * nb * 2.0 * SG_F64_FT * D);
  hipLaunchKernelGGL(feat_norms_kernel, dim3((unsigned)((n + 3) / 4)), dim3(TPB), 0, st, x, n, D, (size_t)ldx, nrm);
  hipLaunchKernelGGL(feat_knn_kernel, dim3((unsigned)nb, (unsigned)CS), dim3(TPB), 0, st, x, n, D, (size_t)ldx, (const double*)nrm, nb, CS, part);
  hipLaunchKernelGGL(feat_knn_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double*)part, n, CS * QL, k, r2);
  SG_LAUNCH_CHECK("sg_feat_knn_radius");
  return 0;
}

extern "C" size_t sg_feat_manifold_counts_ws_bytes(int n, int m) {
  if (n < 1 || m < 1) return 0;
  return ((size_t)n + (size_t)m) * sizeof(double);
}

extern "C" int sg_feat_manifold_counts(const float* a, int n, int lda, const double* r2, const float* b, int m, int ldb, int D, int* count,
                                       double* mind2, void* ws, size_t ws_bytes, sgStream stream) {
  SG_ARG_CHECK(n >= 0 && m >= 0 && D >= 1 && lda >= D && ldb >= D,
               "sg_feat_manifold_counts: bad sizes (n=%d m=%d D=%d lda=%d ldb=%d; n, m >= 0, D >= 1, lda and ldb >= D)", n, m, D, lda, ldb);
  if (n == 0 || m == 0) return 0;
  const int nta = (n + SG_F64_FT - 1) / SG_F64_FT, ntb = (m + SG_F64_FT - 1) / SG_F64_FT;
  SG_ARG_CHECK(ntb <= 65535, "sg_feat_manifold_counts: m=%d is beyond the launch grid", m);
  SG_ARG_CHECK(a && r2 && b && count && mind2 && ws, "sg_feat_manifold_counts: null operand");
  SG_ARG_CHECK(aligned(a, 4) && aligned(b, 4) && aligned(count, 4), "sg_feat_manifold_counts: a, b and count must be 4-byte aligned");
  SG_ARG_CHECK(aligned(r2, 8) && aligned(mind2, 8) && aligned(ws, 8), "sg_feat_manifold_counts: r2, mind2 and ws must be 8-byte aligned");
  SG_ARG_CHECK(ws_bytes >= sg_feat_manifold_counts_ws_bytes(n, m), "sg_feat_manifold_counts: workspace of %zu bytes, %zu needed", ws_bytes,
               sg_feat_manifold_counts_ws_bytes(n, m));
  hipStream_t st = (hipStream_t)stream;
  double* na = (double*)ws;
  double* nb = na + n;
  const double pairs = (double)nta * ntb * SG_F64_FT * SG_F64_FT;
  SgProfScope prof(SG_K_FEAT_MANIFOLD, st, 2.0 * pairs * D, 4.0 * (double)nta * ntb * 2.0 * SG_F64_FT * D);
  const int big = n > m ? n : m;
  hipLaunchKernelGGL(feat_counts_init_kernel, dim3((unsigned)((big + 255) / 256)), dim3(256), 0, st, count, m, (unsigned long long*)mind2, n);
  hipLaunchKernelGGL(feat_norms_kernel, dim3((unsigned)((n + 3) / 4)), dim3(TPB), 0, st, a, n, D, (size_t)lda, na);
  hipLaunchKernelGGL(feat_norms_kernel, dim3((unsigned)((m + 3) / 4)), dim3(TPB), 0, st, b, m, D, (size_t)ldb, nb);
  hipLaunchKernelGGL(feat_counts_kernel, dim3((unsigned)nta, (unsigned)ntb), dim3(TPB), 0, st, a, n, (size_t)lda, r2, b, m, (size_t)ldb, D,
                     (const double*)na, (const double*)nb, count, (unsigned long long*)mind2);
  SG_LAUNCH_CHECK("sg_feat_manifold_counts");
  return 0;
}
