// IS-infinity (scene_generation_amd/isinf.py): the Inception score of every subset of the softmax rows an InceptionScore holds, from
// one pass over the rows and one gathered column reduction.  With p the stored fp32 row, s_i its fp64 sum and ph_ij = (double)p_ij / s_i:
//
//   sg_isinf_row_terms      rs[i] = s_i,  h[i] = sum_j ph_ij log ph_ij                      (a term whose ph is not > 0 is 0)
//   sg_isinf_subset_scores  per subset q of n_q rows t_i:  q_j = sum_i p[t_i][j],  m_j = sum_i ph[t_i][j],
//                           log score = (sum_i h[t_i]) / n_q - sum_j (m_j / n_q) log(q_j / sum_j q_j)
//
// -- the definition of sg_inception_score (inception.hip: score_colmean_kernel, score_kl_kernel), cut so that the per-row part is
// computed once and every subset costs one read of its rows.  The column reduction is the hot path: workgroup (subset, chunk of
// SG_ISINF_ROWS_PER_WG rows, tile of 1024 columns), a thread per 4 adjacent columns (one 16-byte load per row where the rows are
// 16-byte aligned), the rows gathered through the table in the loader, ROWS_IN_FLIGHT loads issued before the first is used.  Chunk
// partials go to the workspace; one finishing workgroup per subset adds them in ascending chunk order.  No atomics: every sum has one
// owner and a fixed order, so a call repeats bit for bit.
#include "f64_tile.h"

namespace {

constexpr int TPB = 256;
constexpr int R = SG_ISINF_ROWS_PER_WG;
constexpr int COLS = 4;                  // columns per thread
constexpr int TILE = TPB * COLS;         // columns per workgroup
constexpr int ROWS_IN_FLIGHT = 8;        // loads a thread issues before it uses the first (8 x 16 B x 256 threads = 32 KiB per workgroup)
constexpr int FTPB = 1024;               // threads of the finishing workgroup
constexpr int CHUNKS_IN_FLIGHT = 8;
static_assert(R % SG_WAVE == 0 && R <= TPB && R % ROWS_IN_FLIGHT == 0, "a chunk's table is staged by one pass of the workgroup");

// One wave per row: lane l adds the classes l, l + 64, ... in ascending order, then the butterfly (every lane ends with the same bits).
__global__ void __launch_bounds__(TPB) isinf_row_terms_kernel(const float* __restrict__ p, int n, int classes, size_t ldp,
                                                             double* __restrict__ rs, double* __restrict__ h) {
  const int row = (int)blockIdx.x * (TPB / SG_WAVE) + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;                                   // wave-uniform
  const float* pr = p + (size_t)row * ldp;
  double s = 0.0;
#pragma unroll 4
  for (int j = lane; j < classes; j += SG_WAVE) s += (double)pr[j];
  s = sg_wave_sum_f64(s);
  double acc = 0.0;
#pragma unroll 4
  for (int j = lane; j < classes; j += SG_WAVE) {         // (the row is 4 KB: the second read comes from the cache)
    const double a = (double)pr[j] / s;
    if (a > 0.0) acc += a * log(a);
  }
  acc = sg_wave_sum_f64(acc);
  if (lane == 0) {
    rs[row] = s;
    h[row] = acc;
  }
}

// the size of subset q as the kernels use it: never beyond the table's row
__device__ __forceinline__ int subset_size(const int* __restrict__ sizes, int q, int smax) {
  const int s = sizes[q];
  return s < 0 ? 0 : (s > smax ? smax : s);
}

// columns [0, ncol) of the four at ``at``; the others read as 0
template <bool ALIGNED>
__device__ __forceinline__ float4 load_cols(const float* __restrict__ at, int ncol) {
  if (ALIGNED && ncol == COLS) return *reinterpret_cast<const float4*>(at);
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (ncol > 0) v.x = at[0];
  if (ncol > 1) v.y = at[1];
  if (ncol > 2) v.z = at[2];
  if (ncol > 3) v.w = at[3];
  return v;
}

__device__ __forceinline__ void add_col(double x, double s, double& q, double& m) {
  q += x;
  const double a = x / s;
  m += a > 0.0 ? a : 0.0;
}

// Workgroup (subset q, chunk c; column tile): the chunk's partial q_j and m_j over its rows in ascending position, to
// part[0 .. classes) and part[classes .. 2 classes); the first column tile also writes the chunk's sum of h to part[2 classes].
// A table entry outside [0, n) forms no address: it is staged as a row of zeros with sum 1, which adds +0 everywhere, and so are the
// positions past a ragged chunk's end.  ALIGNED: p is 16-byte aligned and ldp a multiple of 4.
template <bool ALIGNED>
__global__ void __launch_bounds__(TPB) isinf_chunk_kernel(const float* __restrict__ p, int n, int classes, size_t ldp,
                                                         const double* __restrict__ rs, const double* __restrict__ h,
                                                         const int* __restrict__ idx, const int* __restrict__ sizes, int smax, int nchunk,
                                                         double* __restrict__ ws) {
  __shared__ int s_row[R];
  __shared__ double s_sum[R];
  const int q = (int)blockIdx.x / nchunk, c = (int)blockIdx.x - q * nchunk, tid = threadIdx.x;
  const int nq = subset_size(sizes, q, smax);
  if (c * R >= nq) return;                                // workgroup-uniform: a chunk past the subset's end
  const int rows = nq - c * R < R ? nq - c * R : R;
  if (tid < R) {
    const int t = tid < rows ? idx[(size_t)q * smax + (size_t)(c * R + tid)] : -1;
    const bool ok = t >= 0 && t < n;
    s_row[tid] = ok ? t : -1;
    s_sum[tid] = ok ? rs[t] : 1.0;
  }
  __syncthreads();
  const int c0 = (int)blockIdx.y * TILE + tid * COLS;
  const int ncol = classes - c0 < COLS ? classes - c0 : COLS;          // <= 0: this thread has no column
  double aq[COLS] = {0.0, 0.0, 0.0, 0.0}, am[COLS] = {0.0, 0.0, 0.0, 0.0};
  if (ncol > 0) {
    for (int i0 = 0; i0 < rows; i0 += ROWS_IN_FLIGHT) {
      float4 v[ROWS_IN_FLIGHT];
#pragma unroll
      for (int e = 0; e < ROWS_IN_FLIGHT; ++e) {
        const int t = s_row[i0 + e];                      // (i0 + e < R; past ``rows`` the entry is -1)
        v[e] = t >= 0 ? load_cols<ALIGNED>(p + (size_t)t * ldp + (size_t)c0, ncol) : float4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int e = 0; e < ROWS_IN_FLIGHT; ++e) {
        const double s = s_sum[i0 + e];
        add_col((double)v[e].x, s, aq[0], am[0]);
        add_col((double)v[e].y, s, aq[1], am[1]);
        add_col((double)v[e].z, s, aq[2], am[2]);
        add_col((double)v[e].w, s, aq[3], am[3]);
      }
    }
  }
  const size_t slot = 2 * (size_t)classes + 1;
  double* part = ws + (size_t)q * ((size_t)nchunk * slot + slot) + (size_t)c * slot;
#pragma unroll
  for (int k = 0; k < COLS; ++k)
    if (k < ncol) {
      part[c0 + k] = aq[k];
      part[(size_t)classes + c0 + k] = am[k];
    }
  if (blockIdx.y == 0 && tid < SG_WAVE) {                 // the first wave: lane l adds the positions l, l + 64, ..., then the butterfly
    double hs = 0.0;
#pragma unroll
    for (int i = tid; i < R; i += SG_WAVE) {
      const int t = s_row[i];
      hs += t >= 0 ? h[t] : 0.0;
    }
    hs = sg_wave_sum_f64(hs);
    if (tid == 0) part[2 * (size_t)classes] = hs;
  }
}

// the sum of one value per thread of the finishing workgroup: the butterfly of each wave, then the waves in ascending order
__device__ __forceinline__ double finish_sum(double v, double* red) {
  v = sg_wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < FTPB / SG_WAVE; ++w) t += red[w];
  return t;
}

// One workgroup per subset.  Every entry e of the chunk slots (q_j, m_j, the sum of h) is added over the subset's chunks in ascending
// order by one thread, CHUNKS_IN_FLIGHT loads at a time, into the subset's totals slot; then Q = sum_j q_j, T = sum_j (m_j / n_q)
// log(q_j / Q) over the m_j > 0 (thread t adds j = t, t + 1024, ... in ascending order), and out[q] = {H / n_q - T, exp of it}.
// A size below 2 gives NaNs.
__global__ void __launch_bounds__(FTPB) isinf_finish_kernel(const int* __restrict__ sizes, int smax, int nchunk, int classes,
                                                           double* __restrict__ ws, double* __restrict__ out) {
  __shared__ double red[FTPB / SG_WAVE];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int nq = subset_size(sizes, q, smax);
  const int nch = (nq + R - 1) / R;
  const size_t slot = 2 * (size_t)classes + 1;
  const double* part = ws + (size_t)q * ((size_t)nchunk * slot + slot);
  double* tot = ws + (size_t)q * ((size_t)nchunk * slot + slot) + (size_t)nchunk * slot;
  double qp = 0.0;
  for (size_t e = tid; e < slot; e += FTPB) {
    double s = 0.0;
    for (int c0 = 0; c0 < nch; c0 += CHUNKS_IN_FLIGHT) {
      double v[CHUNKS_IN_FLIGHT];
#pragma unroll
      for (int k = 0; k < CHUNKS_IN_FLIGHT; ++k) v[k] = c0 + k < nch ? part[(size_t)(c0 + k) * slot + e] : 0.0;
#pragma unroll
      for (int k = 0; k < CHUNKS_IN_FLIGHT; ++k) s += v[k];
    }
    tot[e] = s;
    if (e < (size_t)classes) qp += s;
  }
  const double Q = finish_sum(qp, red);
  const double dn = (double)nq;
  double tp = 0.0;
  for (int j = tid; j < classes; j += FTPB) {             // (the barriers of finish_sum lie between the totals' stores and these loads)
    const double mh = tot[(size_t)classes + j] / dn;
    if (mh > 0.0) tp += mh * log(tot[j] / Q);
  }
  const double T = finish_sum(tp, red);
  if (tid == 0) {
    const double ls = tot[2 * (size_t)classes] / dn - T;
    const bool ok = nq >= 2;
    out[2 * (size_t)q] = ok ? ls : __builtin_nan("");
    out[2 * (size_t)q + 1] = ok ? exp(ls) : __builtin_nan("");
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int sg_isinf_row_terms(const float* probs, int n, int classes, int ldp, double* rs, double* h, sgStream stream) {
  SG_ARG_CHECK(n >= 1 && classes >= 1 && ldp >= classes, "sg_isinf_row_terms: bad sizes (n=%d classes=%d ldp=%d; n >= 1, classes >= 1, "
               "ldp >= classes)", n, classes, ldp);
  SG_ARG_CHECK(probs && rs && h, "sg_isinf_row_terms: null operand");
  SG_ARG_CHECK(aligned(probs, 4), "sg_isinf_row_terms: probs must be 4-byte aligned");
  SG_ARG_CHECK(aligned(rs, 8) && aligned(h, 8), "sg_isinf_row_terms: rs and h must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  SgProfScope prof(SG_K_ISINF_ROWS, st, 0.0, 4.0 * (double)n * classes + 16.0 * n);
  hipLaunchKernelGGL(isinf_row_terms_kernel, dim3((unsigned)sg_cdiv(n, TPB / SG_WAVE)), dim3(TPB), 0, st, probs, n, classes, (size_t)ldp,
                     rs, h);
  SG_LAUNCH_CHECK("sg_isinf_row_terms");
  return 0;
}

extern "C" size_t sg_isinf_subset_scores_ws_bytes(int S, int smax, int classes) {
  if (S < 1 || smax < 1 || classes < 1) return 0;
  const size_t nchunk = ((size_t)smax + R - 1) / R, slot = 2 * (size_t)classes + 1;
  return (size_t)S * (nchunk * slot + slot) * sizeof(double);           // per subset: a slot per chunk, then the totals slot
}

extern "C" int sg_isinf_subset_scores(const float* probs, int n, int classes, int ldp, const double* rs, const double* h, const int* idx,
                                      const int* sizes, int S, int smax, double* out, void* ws, size_t ws_bytes, sgStream stream) {
  SG_ARG_CHECK(n >= 1 && classes >= 1 && ldp >= classes && S >= 0 && smax >= 2, "sg_isinf_subset_scores: bad sizes (n=%d classes=%d "
               "ldp=%d S=%d smax=%d; n >= 1, classes >= 1, ldp >= classes, S >= 0, smax >= 2)", n, classes, ldp, S, smax);
  if (S == 0) return 0;
  const long nchunk = ((long)smax + R - 1) / R, tiles = ((long)classes + TILE - 1) / TILE;
  SG_ARG_CHECK((double)S * (double)nchunk <= 2147483647.0 && tiles <= 65535,
               "sg_isinf_subset_scores: S=%d subsets of up to smax=%d rows of %d classes are beyond the launch grid", S, smax, classes);
  SG_ARG_CHECK(probs && rs && h && idx && sizes && out && ws, "sg_isinf_subset_scores: null operand");
  SG_ARG_CHECK(aligned(probs, 4) && aligned(idx, 4) && aligned(sizes, 4), "sg_isinf_subset_scores: probs, idx and sizes must be 4-byte "
               "aligned");
  SG_ARG_CHECK(aligned(rs, 8) && aligned(h, 8) && aligned(out, 8) && aligned(ws, 8),
               "sg_isinf_subset_scores: rs, h, out and ws must be 8-byte aligned");
  SG_ARG_CHECK(ws_bytes >= sg_isinf_subset_scores_ws_bytes(S, smax, classes), "sg_isinf_subset_scores: workspace of %zu bytes, %zu needed",
               ws_bytes, sg_isinf_subset_scores_ws_bytes(S, smax, classes));
  hipStream_t st = (hipStream_t)stream;
  const bool vec = aligned(probs, 16) && ldp % COLS == 0;
  const double cells = (double)S * smax * classes;        // (an upper estimate: the subsets are ragged)
  SgProfScope prof(SG_K_ISINF_SUBSETS, st, 0.0, 4.0 * cells + 32.0 * (double)S * (double)nchunk * classes);
  const dim3 grid((unsigned)(S * nchunk), (unsigned)tiles);
  if (vec)
    hipLaunchKernelGGL(isinf_chunk_kernel<true>, grid, dim3(TPB), 0, st, probs, n, classes, (size_t)ldp, rs, h, idx, sizes, smax,
                       (int)nchunk, (double*)ws);
  else
    hipLaunchKernelGGL(isinf_chunk_kernel<false>, grid, dim3(TPB), 0, st, probs, n, classes, (size_t)ldp, rs, h, idx, sizes, smax,
                       (int)nchunk, (double*)ws);
  hipLaunchKernelGGL(isinf_finish_kernel, dim3((unsigned)S), dim3(FTPB), 0, st, sizes, smax, (int)nchunk, classes, (double*)ws, out);
  SG_LAUNCH_CHECK("sg_isinf_subset_scores");
  return 0;
}
