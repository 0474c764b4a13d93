// Segmented k-means for the appearance bank (scene_generation_amd/bank.py): many independent small k-means problems -- one per
// object class, and one more per restart -- over one fp32 array x [P, D] whose rows are grouped by class (offsets [C + 1], CSR).
// The reference runs 3 x (number of classes) sklearn.cluster.KMeans fits on the CPU (scripts/encode_features.py:83-100); here one
// launch serves every class and every restart, and convergence is tracked on the device (state [R, C]).
//
// Work is cut into TILES of SG_KMEANS_TILE rows that never straddle a class (tiles [T, 2] = (class, first row relative to the
// class's start), built once per clustering by the host from the offsets).  A tile's position is relative to its class, so
// everything a class produces depends on its own rows only: the same class among other classes, or at another offset, gives the
// same bits.  state: 0 = running, 1 = finished, 2 = converged by centre shift (or k = 1): labels / inertia still to be refreshed
// by the final pass.  Workgroups of a class that is not running exit at once.
//
// No floating-point atomics anywhere: sums are taken in a fixed order (rows of a centre in ascending row order inside a tile, tiles
// in ascending order).  The integer counters (labels changed, rows per centre) use integer atomics, which no order can change.
#include "common.h"

namespace {

constexpr int TPB = 256;
typedef float f2 __attribute__((ext_vector_type(2)));
constexpr int TILE = SG_KMEANS_TILE;           // rows per tile
constexpr int RPTH = TILE / TPB;               // rows per thread and tile (update)
constexpr int KMAX = SG_KMEANS_MAX_K;
constexpr int CHUNK = 8192;                    // floats of LDS that hold centres (32 KB): K is walked in chunks of CHUNK / DP

__device__ __forceinline__ bool skip_class(const int32_t* __restrict__ state, int idx, int final_pass) {
  if (!state) return false;
  const int st = state[idx];
  return final_pass ? st == 1 : st != 0;
}

// ---- assign ------------------------------------------------------------------------------------------------------------------------
// One workgroup per (piece of a tile, restart): TPB * RPT rows.  A thread keeps RPT rows of x in registers (zero-padded to DP
// columns) and walks the class's centres, which the workgroup stages in LDS once (every lane reads the same address: broadcast
// ds_read_b128).  Direct form of the distance, sum_d (x_d - c_d)^2 (even and odd column pairs in two packed partial sums): exact zero for a row that IS a centre (the k-means++ rounds
// rely on it).  RPT trades registers (occupancy) against LDS reads per multiply-add; the pieces keep every SIMD supplied with waves
// at the bank's sizes (a 1024-row tile per workgroup leaves a 400 000-row bank with fewer than two workgroups per CU).
template <int DP, int RPT>
__global__ void __launch_bounds__(TPB) kmeans_assign_kernel(const float* __restrict__ x, const int32_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ tiles, const float* __restrict__ centers,
                                                           const int32_t* __restrict__ state, int32_t* __restrict__ labels,
                                                           float* __restrict__ mind2, int32_t* __restrict__ changed,
                                                           int32_t* __restrict__ acount, int P, int C, int K, int D, int final_pass) {
  __shared__ __attribute__((aligned(16))) float sc[CHUNK];
  __shared__ int hist[KMAX];
  __shared__ int nchanged;
  constexpr int ROWS = TPB * RPT, SPLIT = TILE / ROWS;
  const int tile = blockIdx.x / SPLIT, sub = blockIdx.x - tile * SPLIT;
  const int r = blockIdx.y, c = tiles[2 * tile], row0 = tiles[2 * tile + 1] + sub * ROWS, tid = threadIdx.x;
  const int cls = r * C + c;
  if (skip_class(state, cls, final_pass)) return;
  const int n0 = offsets[c], n = offsets[c + 1] - n0;
  if (row0 >= n) return;                              // a piece behind the end of a short tile
  const int k = n < K ? n : K;
  const int nrows = min(ROWS, n - row0);
  const float* cbase = centers + (size_t)cls * K * D;
  for (int j = tid; j < k; j += TPB) hist[j] = 0;
  if (tid == 0) nchanged = 0;
  constexpr int KC = CHUNK / DP;
  float best[RPT];
  int bj[RPT];
  float xr[RPT][DP];
  const bool vec = (D & 3) == 0;
#pragma unroll
  for (int rr = 0; rr < RPT; ++rr) {
    best[rr] = __builtin_inff();
    bj[rr] = 0;
    const int lr = rr * TPB + tid;
    const bool ok = lr < nrows;
    const float* xp = x + (size_t)(n0 + row0 + (ok ? lr : 0)) * D;
    if (vec) {
#pragma unroll
      for (int q = 0; q < DP / 4; ++q) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && 4 * q < D) v = *reinterpret_cast<const float4*>(xp + 4 * q);
        xr[rr][4 * q] = v.x; xr[rr][4 * q + 1] = v.y; xr[rr][4 * q + 2] = v.z; xr[rr][4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int d = 0; d < DP; ++d) xr[rr][d] = (ok && d < D) ? xp[d] : 0.f;
    }
  }
  for (int j0 = 0; j0 < k; j0 += KC) {
    const int kc = min(KC, k - j0);
    __syncthreads();
    for (int e = tid; e < kc * DP; e += TPB) {
      const int j = e / DP, d = e - j * DP;
      sc[e] = d < D ? cbase[(size_t)(j0 + j) * D + d] : 0.f;
    }
    __syncthreads();
    for (int j = 0; j < kc; ++j) {
      const float4* cp = reinterpret_cast<const float4*>(sc + j * DP);
      f2 acc2[RPT];                                   // two interleaved partial sums per row: packed fp32 math (v_pk_add / v_pk_fma)
#pragma unroll
      for (int rr = 0; rr < RPT; ++rr) acc2[rr] = f2{0.f, 0.f};
#pragma unroll
      for (int q = 0; q < DP / 4; ++q) {
        const float4 cv = cp[q];
        const f2 c01 = f2{cv.x, cv.y}, c23 = f2{cv.z, cv.w};
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
          f2 t = f2{xr[rr][4 * q], xr[rr][4 * q + 1]} - c01;
          acc2[rr] = __builtin_elementwise_fma(t, t, acc2[rr]);
          t = f2{xr[rr][4 * q + 2], xr[rr][4 * q + 3]} - c23;
          acc2[rr] = __builtin_elementwise_fma(t, t, acc2[rr]);
        }
      }
      float acc[RPT];
#pragma unroll
      for (int rr = 0; rr < RPT; ++rr) acc[rr] = acc2[rr].x + acc2[rr].y;
#pragma unroll
      for (int rr = 0; rr < RPT; ++rr)
        if (acc[rr] < best[rr]) { best[rr] = acc[rr]; bj[rr] = j0 + j; }       // strict: a tie keeps the lower index
    }
  }
  int nch = 0;
#pragma unroll
  for (int rr = 0; rr < RPT; ++rr) {
    const int lr = rr * TPB + tid;
    if (lr < nrows) {
      const size_t g = (size_t)r * P + n0 + row0 + lr;
      nch += labels[g] != bj[rr];
      labels[g] = bj[rr];
      mind2[g] = best[rr];
      atomicAdd(&hist[bj[rr]], 1);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nch += __shfl_xor(nch, o, 64);
  if ((tid & 63) == 0 && nch) atomicAdd(&nchanged, nch);
  __syncthreads();
  if (tid == 0 && nchanged) atomicAdd(&changed[cls], nchanged);
  for (int j = tid; j < k; j += TPB)
    if (hist[j]) atomicAdd(&acount[(size_t)cls * K + j], hist[j]);
}

// ---- update, stage 1 ---------------------------------------------------------------------------------------------------------------
// One workgroup per (tile, restart): a stable counting sort of the tile's rows by label (ranks from wave ballots, no atomics on
// the order), then every (centre, column) sum is one sequential walk over the centre's rows in ascending row order.
//   psum [R, T, K, D], pcnt [R, T, K] (rows of the tile per centre), pin [R, T] (sum of mind2 over the tile)
__global__ void __launch_bounds__(TPB) kmeans_partial_kernel(const float* __restrict__ x, const int32_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ tiles, const int32_t* __restrict__ state,
                                                            const int32_t* __restrict__ labels, const float* __restrict__ mind2,
                                                            float* __restrict__ psum, int32_t* __restrict__ pcnt,
                                                            float* __restrict__ pin, int P, int C, int K, int D, int T,
                                                            int final_pass) {
  __shared__ int whist[TPB / 64][KMAX];          // rows of wave w with label j -> exclusive prefix over the waves
  __shared__ int start[KMAX + 1];
  __shared__ short perm[TILE];
  __shared__ float red[16];
  const int r = blockIdx.y, c = tiles[2 * blockIdx.x], row0 = tiles[2 * blockIdx.x + 1], tid = threadIdx.x;
  const int cls = r * C + c;
  if (skip_class(state, cls, final_pass)) return;
  const int n0 = offsets[c], n = offsets[c + 1] - n0;
  const int k = n < K ? n : K;
  const int nrows = min(TILE, n - row0);
  const int lane = tid & 63, w = tid >> 6;
  // local row of (wave w, slot rr, lane) = w * (TILE / 4) + rr * 64 + lane: ascending in (w, rr, lane)
  int lab[RPTH], rank[RPTH];
  float in = 0.f;
#pragma unroll
  for (int rr = 0; rr < RPTH; ++rr) {
    const int lr = w * (TILE / (TPB / 64)) + rr * 64 + lane;
    lab[rr] = -1;
    rank[rr] = 0;
    if (lr < nrows) {
      const size_t g = (size_t)r * P + n0 + row0 + lr;
      const int l = labels[g];
      lab[rr] = (l >= 0 && l < k) ? l : -1;       // a label outside the class's centres takes part in nothing
      in += mind2[g];
    }
  }
  for (int j = 0; j < k; ++j) {
    int base = 0;
#pragma unroll
    for (int rr = 0; rr < RPTH; ++rr) {
      const unsigned long long m = __ballot(lab[rr] == j);
      if (lab[rr] == j) rank[rr] = base + __popcll(m & ((1ull << lane) - 1ull));
      base += __popcll(m);
    }
    if (lane == 0) whist[w][j] = base;
  }
  const float inertia = sg_block_sum(in, red);       // (contains the barrier that publishes whist)
  for (int j = tid; j < k; j += TPB) {
    int run = 0;
#pragma unroll
    for (int ww = 0; ww < TPB / 64; ++ww) { const int v = whist[ww][j]; whist[ww][j] = run; run += v; }
    start[j + 1] = run;                               // count for now
    pcnt[((size_t)r * T + blockIdx.x) * K + j] = run;
  }
  __syncthreads();
  if (tid == 0) {
    pin[(size_t)r * T + blockIdx.x] = inertia;
    int run = 0;
    start[0] = 0;
    for (int j = 0; j < k; ++j) { run += start[j + 1]; start[j + 1] = run; }
  }
  __syncthreads();
  if (final_pass) return;                             // counts and inertia only
#pragma unroll
  for (int rr = 0; rr < RPTH; ++rr)
    if (lab[rr] >= 0) perm[start[lab[rr]] + whist[w][lab[rr]] + rank[rr]] = (short)(w * (TILE / (TPB / 64)) + rr * 64 + lane);
  __syncthreads();
  if ((D & 3) == 0) {
    // A WALKER of D / 4 threads (a float4 of columns each) sums the rows of one (centre, part): a centre's row list is cut into
    // ``parts`` contiguous pieces (a power of two, as many as keep every walker busy) whose sums are folded in ascending order.
    // The cut depends on the class's k and on the tile's labels only.
    const int tpw = D >> 2, wk = tid / tpw, q = tid - wk * tpw;
    int parts = 1;
    while (parts < 16 && k * parts * 2 <= TPB / tpw) parts <<= 1;
    const int W = (TPB / tpw) / parts * parts;        // walkers in use: a multiple of ``parts``
    __shared__ float4 comb[TPB];
    const float* xb = x + (size_t)(n0 + row0) * D + 4 * q;
    float* ps = psum + ((size_t)r * T + blockIdx.x) * K * D + 4 * q;
    for (int base = 0; base < k * parts; base += W) { // block-uniform trip count
      const int item = base + wk;
      const bool act = wk < W && item < k * parts;
      const int j = act ? item / parts : 0, part = act ? item - j * parts : 1;
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      if (act) {
        const int a0 = start[j], len = start[j + 1] - a0;
        const int a = a0 + len * part / parts, b = a0 + len * (part + 1) / parts;
        int i = a;
        for (; i + 8 <= b; i += 8) {                  // eight loads in flight, added in row order
          float4 v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = *reinterpret_cast<const float4*>(xb + (size_t)perm[i + e] * D);
#pragma unroll
          for (int e = 0; e < 8; ++e) { s.x += v[e].x; s.y += v[e].y; s.z += v[e].z; s.w += v[e].w; }
        }
        for (; i < b; ++i) {
          const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)perm[i] * D);
          s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
      }
      if (parts > 1) {
        comb[tid] = s;
        __syncthreads();
        if (act && part == 0)
          for (int pp = 1; pp < parts; ++pp) {
            const float4 v = comb[tid + pp * tpw];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
          }
        __syncthreads();
      }
      if (act && part == 0) *reinterpret_cast<float4*>(ps + (size_t)j * D) = s;
    }
    return;
  }
  const int slots = TPB / D;                          // any D: one thread per (centre slot, column)
  const int d = tid % D, slot = tid / D;
  if (slot >= slots) return;
  const float* xb = x + (size_t)(n0 + row0) * D + d;
  float* ps = psum + ((size_t)r * T + blockIdx.x) * K * D + d;
  for (int j = slot; j < k; j += slots) {
    const int a = start[j], b = start[j + 1];
    float s = 0.f;
    int i = a;
    for (; i + 4 <= b; i += 4) {                      // four loads in flight, added in row order
      const float v0 = xb[(size_t)perm[i] * D], v1 = xb[(size_t)perm[i + 1] * D], v2 = xb[(size_t)perm[i + 2] * D],
                  v3 = xb[(size_t)perm[i + 3] * D];
      s += v0; s += v1; s += v2; s += v3;
    }
    for (; i < b; ++i) s += xb[(size_t)perm[i] * D];
    ps[(size_t)j * D] = s;
  }
}

// ---- update, stage 2 ---------------------------------------------------------------------------------------------------------------
// One workgroup per (class, restart): partials of the class's tiles in ascending order -> centres, counts, inertia, squared
// centre shift; then the class's bookkeeping (n_iter, state) and the reset of the integer counters for the next assign.
__global__ void __launch_bounds__(TPB) kmeans_finish_kernel(const int32_t* __restrict__ offsets, const int32_t* __restrict__ tile_off,
                                                           const float* __restrict__ psum, const int32_t* __restrict__ pcnt,
                                                           const float* __restrict__ pin, float* __restrict__ centers,
                                                           int32_t* __restrict__ counts, float* __restrict__ inertia,
                                                           float* __restrict__ shift, const float* __restrict__ tolvar,
                                                           int32_t* __restrict__ state, int32_t* __restrict__ n_iter,
                                                           int32_t* __restrict__ changed, int32_t* __restrict__ acount, int C, int K,
                                                           int D, int T, int final_pass) {
  __shared__ int cnt[KMAX];
  __shared__ float red[16];
  const int r = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int cls = r * C + c;
  if (skip_class(state, cls, final_pass)) return;
  const int n = offsets[c + 1] - offsets[c];
  const int k = n < K ? n : K;
  const int t0 = tile_off[c], t1 = tile_off[c + 1];
  for (int j = tid; j < K; j += TPB) {
    int s = 0;
    if (j < k)
      for (int t = t0; t < t1; ++t) s += pcnt[((size_t)r * T + t) * K + j];
    cnt[j] = s;
    counts[(size_t)cls * K + j] = s;
    if (acount) acount[(size_t)cls * K + j] = 0;
  }
  __syncthreads();
  float sh = 0.f;
  if (!final_pass) {
    float* cb = centers + (size_t)cls * K * D;
    for (int e = tid; e < k * D; e += TPB) {
      const int j = e / D;
      if (cnt[j] > 0) {                               // (a centre without rows keeps its place)
        const float s = sg_sum_strided(psum + ((size_t)r * T + t0) * K * D + e, (size_t)K * D, t1 - t0);
        const float nc = s / (float)cnt[j], df = nc - cb[e];
        cb[e] = nc;
        sh = fmaf(df, df, sh);
      }
    }
  }
  sh = sg_block_sum(sh, red);
  if (tid == 0) {
    inertia[cls] = sg_sum_strided(pin + (size_t)r * T + t0, 1, t1 - t0);
    int ch = 0;
    if (changed) { ch = changed[cls]; changed[cls] = 0; }
    if (final_pass) {
      if (state) state[cls] = 1;
    } else {
      shift[cls] = sh;
      if (n_iter && n > 0) n_iter[cls] += 1;
      if (state) {
        int st = 0;
        if (n == 0 || ch == 0) st = 1;                // no label moved: the centres just written are the ones the labels belong to
        else if (k == 1 || (tolvar && sh <= tolvar[c])) st = 2;
        state[cls] = st;
      }
    }
  }
}

// ---- relocate ----------------------------------------------------------------------------------------------------------------------
// One workgroup per (class, restart); a class whose centres all have rows leaves at once.  Per empty centre (ascending): the row
// with the largest mind2 (ties: lower row) among the rows whose centre has more than one row takes the empty centre's label.
__global__ void __launch_bounds__(TPB) kmeans_relocate_kernel(const int32_t* __restrict__ offsets, const int32_t* __restrict__ state,
                                                             int32_t* __restrict__ labels, const float* __restrict__ mind2,
                                                             const int32_t* __restrict__ acount, int P, int C, int K) {
  __shared__ int cnt[KMAX];
  __shared__ int nempty;
  __shared__ float bv[TPB / 64];
  __shared__ int bi[TPB / 64];
  const int r = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int cls = r * C + c;
  if (skip_class(state, cls, 0)) return;
  const int n0 = offsets[c], n = offsets[c + 1] - n0;
  const int k = n < K ? n : K;
  if (tid == 0) nempty = 0;
  __syncthreads();
  int mine = 0;
  for (int j = tid; j < k; j += TPB) {
    cnt[j] = acount[(size_t)cls * K + j];
    mine += cnt[j] == 0;
  }
  if (mine) atomicAdd(&nempty, mine);
  __syncthreads();
  if (nempty == 0) return;
  int32_t* lb = labels + (size_t)r * P + n0;
  const float* md = mind2 + (size_t)r * P + n0;
  for (int e = 0; e < k; ++e) {                       // bounded: at most k rounds
    if (cnt[e] != 0) continue;                        // block-uniform (LDS)
    float v = -1.f;
    int idx = -1;
    for (int i = tid; i < n; i += TPB) {              // ascending i per thread: '>' keeps the lowest row of a tie
      const int l = lb[i];
      const float m = md[i];
      if (l >= 0 && l < k && cnt[l] > 1 && m > v) { v = m; idx = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      if (oi >= 0 && (idx < 0 || ov > v || (ov == v && oi < idx))) { v = ov; idx = oi; }
    }
    if ((tid & 63) == 0) { bv[tid >> 6] = v; bi[tid >> 6] = idx; }
    __syncthreads();
    if (tid == 0) {
      for (int ww = 1; ww < TPB / 64; ++ww)
        if (bi[ww] >= 0 && (bi[0] < 0 || bv[ww] > bv[0] || (bv[ww] == bv[0] && bi[ww] < bi[0]))) { bv[0] = bv[ww]; bi[0] = bi[ww]; }
      if (bi[0] >= 0) {
        cnt[lb[bi[0]]] -= 1;
        cnt[e] = 1;
        lb[bi[0]] = e;
      }
    }
    __syncthreads();                                  // the new label and counts are visible to the next round
  }
}

// ---- one round of k-means++ seeding ----------------------------------------------------------------------------------------------
// Round 0 picks row floor(u * n).  Round t >= 1 is two launches.  (1) kmeans_pp_dist_kernel, one workgroup per (tile, restart):
// mind2 = min(mind2, |x - centre t-1|^2) and the tile's sum of mind2 (fixed order).  (2) kmeans_pp_pick_kernel, one workgroup per
// (class, restart): running offsets of the class's tiles in ascending order, the first tile whose end exceeds u * total, then the
// first row of that tile whose running sum does.  Inside the tile threads own two consecutive rows; the running sum of a thread
// restarts from zero and is added to the thread's offset exactly as the offsets were formed, so a crossing is only ever found at
// a row that added something: a row already chosen (mind2 = 0) is never chosen again.  Should the tile's own order of summation
// place its end below the target (the two orders differ by rounding), the tile's last row with a distance is taken.
__global__ void __launch_bounds__(TPB) kmeans_pp_dist_kernel(const float* __restrict__ x, const int32_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ tiles, const float* __restrict__ centers,
                                                            float* __restrict__ mind2, float* __restrict__ tsum, int P, int C, int K,
                                                            int D, int T, int round) {
  __shared__ float red[16];
  const int r = blockIdx.y, c = tiles[2 * blockIdx.x], row0 = tiles[2 * blockIdx.x + 1], tid = threadIdx.x;
  const int cls = r * C + c;
  const int n0 = offsets[c], n = offsets[c + 1] - n0;
  const int k = n < K ? n : K;
  if (round >= k) return;
  const int nrows = min(TILE, n - row0);
  const float* cen = centers + ((size_t)cls * K + (round - 1)) * D;
  const float* xb = x + (size_t)(n0 + row0) * D;
  float* md = mind2 + (size_t)r * P + n0 + row0;
  float sum = 0.f;
  const int tpw = D >> 2;
  if ((D & 3) == 0 && (tpw & (tpw - 1)) == 0) {       // D / 4 lanes per row (a power of two <= 32): coalesced float4 loads
    const int g = tid / tpw, q = tid - g * tpw, G = TPB / tpw;
    const float4 cv = *reinterpret_cast<const float4*>(cen + 4 * q);
    for (int i0 = 0; i0 < nrows; i0 += 4 * G) {       // block-uniform trip count (the shuffles below need whole waves)
      float acc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e * G + g;
        float4 v = cv;
        if (i < nrows) v = *reinterpret_cast<const float4*>(xb + (size_t)i * D + 4 * q);
        const float tx = v.x - cv.x, ty = v.y - cv.y, tz = v.z - cv.z, tw = v.w - cv.w;
        acc[e] = fmaf(tw, tw, fmaf(tz, tz, fmaf(ty, ty, tx * tx)));
      }
      for (int o = tpw >> 1; o > 0; o >>= 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e * G + g;
        if (q == 0 && i < nrows) {
          const float m = round == 1 ? acc[e] : fminf(md[i], acc[e]);
          md[i] = m;
          sum += m;
        }
      }
    }
  } else {
    for (int i = tid; i < nrows; i += TPB) {
      const float* xp = xb + (size_t)i * D;
      float acc = 0.f;
      for (int d = 0; d < D; ++d) { const float t = xp[d] - cen[d]; acc = fmaf(t, t, acc); }
      const float m = round == 1 ? acc : fminf(md[i], acc);
      md[i] = m;
      sum += m;
    }
  }
  sum = sg_block_sum(sum, red);
  if (tid == 0) tsum[(size_t)r * T + blockIdx.x] = sum;
}

constexpr int PPT = TILE / 2;                         // threads of the pick: two consecutive rows of a tile each
__global__ void __launch_bounds__(PPT) kmeans_pp_pick_kernel(const float* __restrict__ x, const int32_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ tile_off, const float* __restrict__ u,
                                                            float* __restrict__ centers, const float* __restrict__ mind2,
                                                            const float* __restrict__ tsum, int32_t* __restrict__ picks, int P,
                                                            int C, int K, int D, int T, int round) {
  __shared__ float part[PPT + 1];
  __shared__ int pick, tile_sel;
  __shared__ float target_s;
  const int r = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int cls = r * C + c;
  const int n0 = offsets[c], n = offsets[c + 1] - n0;
  const int k = n < K ? n : K;
  if (round >= k) return;
  const float uu = u[(size_t)cls * K + round];
  const float* md = mind2 + (size_t)r * P + n0;
  const int first = min((int)(uu * (float)n), n - 1);
  int chosen = first;
  if (round > 0) {
    const int t0 = tile_off[c], nt = tile_off[c + 1] - t0;
    if (tid == 0) {
      const float* ts = tsum + (size_t)r * T + t0;
      float total = 0.f;
      for (int t = 0; t < nt; ++t) total += ts[t];    // bounded by the class's tiles
      const float target = uu * total;
      float run = 0.f;
      int sel = -1;
      float base = 0.f;
      for (int t = 0; t < nt; ++t) {
        const float nxt = run + ts[t];
        if (sel < 0 && nxt > target) { sel = t; base = run; }
        run = nxt;
      }
      tile_sel = sel;
      target_s = target - base;                       // what the rows of the tile have to exceed
      pick = 0x7fffffff;
    }
    __syncthreads();
    const int sel = tile_sel;
    if (sel >= 0) {                                   // block-uniform
      const int row0 = sel * TILE, nrows = min(TILE, n - row0);
      const float tgt = target_s;
      const int a = 2 * tid;
      const float m0 = a < nrows ? md[row0 + a] : 0.f, m1 = a + 1 < nrows ? md[row0 + a + 1] : 0.f;
      part[tid + 1] = m0 + m1;
      if (tid == 0) part[0] = 0.f;
      __syncthreads();
      if (tid == 0)
        for (int t = 0; t < PPT; ++t) part[t + 1] = part[t] + part[t + 1];      // exclusive offsets, one order
      __syncthreads();
      const float off = part[tid];
      if (part[tid + 1] > tgt) {
        if (off + m0 > tgt) atomicMin(&pick, row0 + a);
        else if (off + (m0 + m1) > tgt) atomicMin(&pick, row0 + a + 1);
      }
      __syncthreads();
      chosen = pick;
      if (chosen == 0x7fffffff) {                     // the tile's own order ends below the target: its last row with a distance
        __syncthreads();
        if (tid == 0) pick = -1;
        __syncthreads();
        if (m1 > 0.f) atomicMax(&pick, row0 + a + 1);
        else if (m0 > 0.f) atomicMax(&pick, row0 + a);
        __syncthreads();
        chosen = pick >= 0 ? pick : first;
      }
    }
    // sel < 0: every row coincides with a chosen centre (total = 0), or u * total rounded up to the total: row floor(u * n)
  }
  const float* xb = x + (size_t)n0 * D;
  float* cb = centers + (size_t)cls * K * D;
  for (int d = tid; d < D; d += PPT) cb[(size_t)round * D + d] = xb[(size_t)chosen * D + d];
  if (tid == 0) picks[(size_t)cls * K + round] = chosen;
}

}  // namespace

static int kmeans_check(const char* who, int P, int C, int K, int D, int R) {
  SG_ARG_CHECK(P >= 0 && C > 0 && R > 0 && R <= 65535, "%s: bad sizes (P=%d C=%d R=%d)", who, P, C, R);
  SG_ARG_CHECK(D >= 1 && D <= SG_KMEANS_MAX_D, "%s: D=%d outside 1..%d", who, D, SG_KMEANS_MAX_D);
  SG_ARG_CHECK(K >= 1 && K <= SG_KMEANS_MAX_K, "%s: K=%d outside 1..%d", who, K, SG_KMEANS_MAX_K);
  SG_ARG_CHECK((int64_t)P * R < ((int64_t)1 << 31), "%s: P * R too large", who);
  return 0;
}

extern "C" int sg_kmeans_assign(const float* x, const int32_t* offsets, const int32_t* tiles, const float* centers,
                                const int32_t* state, int32_t* labels, float* mind2, int32_t* changed, int32_t* acount, int P,
                                int C, int K, int D, int R, int T, int final_pass, sgStream stream) {
  if (int rc = kmeans_check("sg_kmeans_assign", P, C, K, D, R)) return rc;
  SG_ARG_CHECK(x && offsets && tiles && centers && labels && mind2 && changed && acount && T >= 0, "sg_kmeans_assign: null operand");
  if (T == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_KMEANS_ASSIGN, s, 3.0 * P * R * (double)K * D, (double)P * R * (4.0 * D + 12.0));
#define LAUNCH_ASSIGN(DP, RPT)                                                                                                  \
  hipLaunchKernelGGL((kmeans_assign_kernel<DP, RPT>), dim3(T * (SG_KMEANS_TILE / (TPB * RPT)), R), dim3(TPB), 0, s, x, offsets,  \
                     tiles, centers, state, labels, mind2, changed, acount, P, C, K, D, final_pass)
  if (D <= 8) LAUNCH_ASSIGN(8, 4);
  else if (D <= 16) LAUNCH_ASSIGN(16, 4);
  else if (D <= 32) LAUNCH_ASSIGN(32, 2);
  else if (D <= 64) LAUNCH_ASSIGN(64, 1);
  else LAUNCH_ASSIGN(128, 1);
#undef LAUNCH_ASSIGN
  SG_LAUNCH_CHECK("sg_kmeans_assign");
  return 0;
}

extern "C" size_t sg_kmeans_update_ws_bytes(int T, int K, int D, int R) {
  if (T <= 0 || K <= 0 || D <= 0 || R <= 0) return 16;
  return (size_t)R * T * ((size_t)K * D * sizeof(float) + (size_t)K * sizeof(int32_t) + sizeof(float)) + 16;
}

extern "C" int sg_kmeans_update(const float* x, const int32_t* offsets, const int32_t* tiles, const int32_t* tile_off,
                                const int32_t* labels, const float* mind2, float* centers, int32_t* counts, float* inertia,
                                float* shift, const float* tolvar, int32_t* state, int32_t* n_iter, int32_t* changed,
                                int32_t* acount, void* ws, size_t ws_bytes, int P, int C, int K, int D, int R, int T, int final_pass,
                                sgStream stream) {
  if (int rc = kmeans_check("sg_kmeans_update", P, C, K, D, R)) return rc;
  SG_ARG_CHECK(x && offsets && tiles && tile_off && labels && mind2 && centers && counts && inertia && shift && ws && T >= 0,
               "sg_kmeans_update: null operand");
  SG_ARG_CHECK(ws_bytes >= sg_kmeans_update_ws_bytes(T, K, D, R), "sg_kmeans_update: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* psum = reinterpret_cast<float*>(ws);
  float* pin = psum + (size_t)R * T * K * D;
  int32_t* pcnt = reinterpret_cast<int32_t*>(pin + (size_t)R * T);
  SgProfScope prof(SG_K_KMEANS_UPDATE, s, (double)P * R * D, (double)P * R * (4.0 * D + 8.0) + 2.0 * R * T * (double)K * D * 4.0);
  if (T > 0)
    hipLaunchKernelGGL(kmeans_partial_kernel, dim3(T, R), dim3(TPB), 0, s, x, offsets, tiles, state, labels, mind2, psum, pcnt, pin,
                       P, C, K, D, T, final_pass);
  hipLaunchKernelGGL(kmeans_finish_kernel, dim3(C, R), dim3(TPB), 0, s, offsets, tile_off, (const float*)psum, (const int32_t*)pcnt,
                     (const float*)pin, centers, counts, inertia, shift, tolvar, state, n_iter, changed, acount, C, K, D, T,
                     final_pass);
  SG_LAUNCH_CHECK("sg_kmeans_update");
  return 0;
}

extern "C" int sg_kmeans_relocate(const int32_t* offsets, const int32_t* state, int32_t* labels, const float* mind2,
                                  const int32_t* acount, int P, int C, int K, int R, sgStream stream) {
  if (int rc = kmeans_check("sg_kmeans_relocate", P, C, K, 1, R)) return rc;
  SG_ARG_CHECK(offsets && labels && mind2 && acount, "sg_kmeans_relocate: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_KMEANS_RELOCATE, s, 0, (double)R * C * K * 4.0);
  hipLaunchKernelGGL(kmeans_relocate_kernel, dim3(C, R), dim3(TPB), 0, s, offsets, state, labels, mind2, acount, P, C, K);
  SG_LAUNCH_CHECK("sg_kmeans_relocate");
  return 0;
}

extern "C" size_t sg_kmeans_pp_step_ws_bytes(int T, int R) {
  if (T <= 0 || R <= 0) return 16;
  return (size_t)T * R * sizeof(float) + 16;
}

extern "C" int sg_kmeans_pp_step(const float* x, const int32_t* offsets, const int32_t* tiles, const int32_t* tile_off,
                                 const float* u, float* centers, float* mind2, int32_t* picks, void* ws, size_t ws_bytes, int P,
                                 int C, int K, int D, int R, int T, int round, sgStream stream) {
  if (int rc = kmeans_check("sg_kmeans_pp_step", P, C, K, D, R)) return rc;
  SG_ARG_CHECK(x && offsets && tiles && tile_off && u && centers && mind2 && picks && ws && round >= 0 && round < K && T >= 0,
               "sg_kmeans_pp_step: bad arguments");
  SG_ARG_CHECK(ws_bytes >= sg_kmeans_pp_step_ws_bytes(T, R), "sg_kmeans_pp_step: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* tsum = reinterpret_cast<float*>(ws);
  SgProfScope prof(SG_K_KMEANS_PP, s, round ? 3.0 * P * R * (double)D : 0.0, round ? (double)P * R * (4.0 * D + 8.0) : 0.0);
  if (round > 0 && T > 0)
    hipLaunchKernelGGL(kmeans_pp_dist_kernel, dim3(T, R), dim3(TPB), 0, s, x, offsets, tiles, (const float*)centers, mind2, tsum, P, C,
                       K, D, T, round);
  hipLaunchKernelGGL(kmeans_pp_pick_kernel, dim3(C, R), dim3(PPT), 0, s, x, offsets, tile_off, u, centers, (const float*)mind2,
                     (const float*)tsum, picks, P, C, K, D, T, round);
  SG_LAUNCH_CHECK("sg_kmeans_pp_step");
  return 0;
}
