// Scene graphs from layouts (scene_generation_amd/scenegraph.py): the step of CocoSceneGraphDataset.__getitem__ that turns boxes
// and masks into attribute bits and geometric predicates (data/coco.py:323-416), which the reference runs in Python loops over
// objects, and the agreement counters that say whether a layout honours the graph it was generated from.
//
// Every decision is an exact function of fp32 inputs.  A mask is reduced to three INTEGERS (count, sum of set columns, sum of set
// rows), so there is no floating-point sum whose order could matter; the centre is then one fp64 expression rounded to fp32 once.
// The agreement counters are integer atomics.  Nothing here allocates or synchronises.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int WPB = TPB / SG_WAVE;             // waves (= objects of the wave plan) per workgroup
typedef long long ll2 __attribute__((ext_vector_type(2)));

struct Tally {
  unsigned c, sx, sy;                          // M <= 256: sx, sy <= 65536 * 255 < 2^24
  __device__ __forceinline__ void add(bool set, int e, const FastDiv& fd, int M) {
    const int row = (int)fd.div((unsigned)e), col = e - row * M;
    c += set ? 1u : 0u;
    sx += set ? (unsigned)col : 0u;
    sy += set ? (unsigned)row : 0u;
  }
  __device__ __forceinline__ void wave_reduce() {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      c += __shfl_xor(c, o, 64);
      sx += __shfl_xor(sx, o, 64);
      sy += __shfl_xor(sy, o, 64);
    }
  }
};

// the n = M * M elements of one mask, dealt to ``nl`` lanes; vec: 16-byte loads (two int64 / four fp32), which the host allows
// only when every object's mask starts on a 16-byte boundary
template <bool I64>
__device__ __forceinline__ Tally tally_mask(const void* __restrict__ mp, int n, int lane, int nl, bool vec, const FastDiv& fd, int M) {
  Tally t{0u, 0u, 0u};
  if (I64) {
    const long long* m = reinterpret_cast<const long long*>(mp);
    if (vec) {
      const int nv = n >> 1;
      for (int v = lane; v < nv; v += nl) {
        const ll2 q = *reinterpret_cast<const ll2*>(m + 2 * v);
        t.add(q.x == 1, 2 * v, fd, M);
        t.add(q.y == 1, 2 * v + 1, fd, M);
      }
    } else {
      for (int e = lane; e < n; e += nl) t.add(m[e] == 1, e, fd, M);
    }
  } else {
    const float* m = reinterpret_cast<const float*>(mp);
    if (vec) {
      const int nv = n >> 2;
      for (int v = lane; v < nv; v += nl) {
        const float4 q = *reinterpret_cast<const float4*>(m + 4 * v);
        t.add(q.x > 0.5f, 4 * v, fd, M);
        t.add(q.y > 0.5f, 4 * v + 1, fd, M);
        t.add(q.z > 0.5f, 4 * v + 2, fd, M);
        t.add(q.w > 0.5f, 4 * v + 3, fd, M);
      }
    } else {
      for (int e = lane; e < n; e += nl) t.add(m[e] > 0.5f, e, fd, M);
    }
  }
  return t;
}

__device__ __forceinline__ void finish_center(const float* __restrict__ boxes, int o, int M, const Tally& t,
                                              float* __restrict__ centers, int32_t* __restrict__ count) {
  const float x0 = boxes[4 * o], y0 = boxes[4 * o + 1], x1 = boxes[4 * o + 2], y1 = boxes[4 * o + 3];
  float cx, cy;
  if (t.c == 0) {                               // coco.py:335-337
    cx = 0.5f * (x0 + x1);
    cy = 0.5f * (y0 + y1);
  } else if (M == 1) {                          // torch.linspace(x0, x1, 1) is [x0]
    cx = x0;
    cy = y0;
  } else {
    const double den = (double)t.c * (double)(M - 1);
    cx = (float)((double)x0 + ((double)x1 - (double)x0) * (double)t.sx / den);
    cy = (float)((double)y0 + ((double)y1 - (double)y0) * (double)t.sy / den);
  }
  centers[2 * o] = cx;
  centers[2 * o + 1] = cy;
  count[o] = (int32_t)t.c;
}

// M <= 16: a wave per object, WPB objects per workgroup (a 16 x 16 int64 mask is two 16-byte loads per lane)
template <bool I64>
__global__ void __launch_bounds__(TPB) centers_wave_kernel(const float* __restrict__ boxes, const void* __restrict__ masks,
                                                          float* __restrict__ centers, int32_t* __restrict__ count, int O, int M,
                                                          int vec, FastDiv fd) {
  const int o = blockIdx.x * WPB + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (o >= O) return;                           // wave-uniform
  const int n = M * M;
  const char* mp = reinterpret_cast<const char*>(masks) + (size_t)o * n * (I64 ? 8 : 4);
  Tally t = tally_mask<I64>(mp, n, lane, SG_WAVE, vec != 0, fd, M);
  t.wave_reduce();
  if (lane == 0) finish_center(boxes, o, M, t, centers, count);
}

// M > 16: a workgroup per object; a thread walks the mask in steps of TPB vectors (M = 64: eight 16-byte loads of int64)
template <bool I64>
__global__ void __launch_bounds__(TPB) centers_block_kernel(const float* __restrict__ boxes, const void* __restrict__ masks,
                                                           float* __restrict__ centers, int32_t* __restrict__ count, int M, int vec,
                                                           FastDiv fd) {
  __shared__ unsigned red[3 * WPB];
  const int o = blockIdx.x, tid = threadIdx.x, n = M * M;
  const char* mp = reinterpret_cast<const char*>(masks) + (size_t)o * n * (I64 ? 8 : 4);
  Tally t = tally_mask<I64>(mp, n, tid, TPB, vec != 0, fd, M);
  t.wave_reduce();
  if ((tid & 63) == 0) {
    red[3 * (tid >> 6)] = t.c;
    red[3 * (tid >> 6) + 1] = t.sx;
    red[3 * (tid >> 6) + 2] = t.sy;
  }
  __syncthreads();
  if (tid == 0) {
    Tally a{0u, 0u, 0u};
#pragma unroll
    for (int w = 0; w < WPB; ++w) {
      a.c += red[3 * w];
      a.sx += red[3 * w + 1];
      a.sy += red[3 * w + 2];
    }
    finish_center(boxes, o, M, a, centers, count);
  }
}

__device__ __forceinline__ int clamp_rint(double v, int hi) {
  const double r = rint(v);                     // round half to even: Python's round() on a double
  return r >= (double)hi ? hi : (r > 0.0 ? (int)r : 0);      // a NaN lands on 0
}

__device__ __forceinline__ void attribute_indices(const float* __restrict__ boxes, const float* __restrict__ centers, int o, int S,
                                                  int g, int& si, int& li) {
  const float w = boxes[4 * o + 2] - boxes[4 * o], h = boxes[4 * o + 3] - boxes[4 * o + 1];
  si = clamp_rint((double)(S - 1) * (double)w * (double)h, S - 1);
  const int lx = clamp_rint((double)centers[2 * o] * (double)(g - 1), g - 1);
  const int ly = clamp_rint((double)centers[2 * o + 1] * (double)(g - 1), g - 1);
  li = lx + g * ly;
}

__global__ void __launch_bounds__(TPB) attributes_kernel(const float* __restrict__ boxes, const float* __restrict__ centers,
                                                        int32_t* __restrict__ size_idx, int32_t* __restrict__ loc_idx,
                                                        float* __restrict__ onehot, int O, int S, int g) {
  const int o = blockIdx.x * TPB + threadIdx.x;
  if (o >= O) return;
  int si, li;
  attribute_indices(boxes, centers, o, S, g, si, li);
  size_idx[o] = si;
  loc_idx[o] = li;
  if (onehot) {
    const int A = S + g * g;
    float* row = onehot + (size_t)o * A;
    for (int a = 0; a < A; ++a) row[a] = (a == si || a == S + li) ? 1.f : 0.f;
  }
}

// coco.py:368-385 without atan2: the comparisons below select the same class as the reference's thresholds on theta for every
// fp32 (dx, dy), ties included (exact diagonals: below / left of / left of / right of; dx = dy = 0: right of)
__device__ __forceinline__ int derive_predicate(const float* __restrict__ boxes, const float* __restrict__ centers, int s, int o) {
  const float sx0 = boxes[4 * s], sy0 = boxes[4 * s + 1], sx1 = boxes[4 * s + 2], sy1 = boxes[4 * s + 3];
  const float ox0 = boxes[4 * o], oy0 = boxes[4 * o + 1], ox1 = boxes[4 * o + 2], oy1 = boxes[4 * o + 3];
  if (sx0 < ox0 && sx1 > ox1 && sy0 < oy0 && sy1 > oy1) return 6;
  if (sx0 > ox0 && sx1 < ox1 && sy0 > oy0 && sy1 < oy1) return 5;
  const float dx = centers[2 * s] - centers[2 * o], dy = centers[2 * s + 1] - centers[2 * o + 1];
  const float ax = fabsf(dx), ay = fabsf(dy);
  if (dx < 0.f && ay <= ax) return 1;
  if (dy < 0.f && ay > ax) return 3;
  if (dy > 0.f && ay >= ax) return 4;
  return 2;
}

__device__ __forceinline__ bool id_ok(int64_t v, int O) { return v >= 0 && v < (int64_t)O; }

__global__ void __launch_bounds__(TPB) predicates_kernel(const float* __restrict__ boxes, const float* __restrict__ centers,
                                                        const int64_t* __restrict__ s, const int64_t* __restrict__ o, int idx_stride,
                                                        int64_t* __restrict__ p, int p_stride, int T, int O) {
  const int t = blockIdx.x * TPB + threadIdx.x;
  if (t >= T) return;
  const int64_t si = s[(size_t)t * idx_stride], oi = o[(size_t)t * idx_stride];
  p[(size_t)t * p_stride] = (id_ok(si, O) && id_ok(oi, O)) ? (int64_t)derive_predicate(boxes, centers, (int)si, (int)oi) : (int64_t)-1;
}

// one workgroup per image; thread e writes the image's e-th triple
__global__ void __launch_bounds__(TPB) draw_pairs_kernel(const int32_t* __restrict__ seg_off, const int32_t* __restrict__ tri_off,
                                                        const float* __restrict__ u, const float* __restrict__ boxes,
                                                        const float* __restrict__ centers, int64_t* __restrict__ triples,
                                                        int64_t* __restrict__ triple_to_img, int O, int T, int r) {
  const int n = blockIdx.x;
  const int base = seg_off[n], k = seg_off[n + 1] - base - 1;       // real objects: all but the trailing __image__
  const int t0 = tri_off[n], nt = tri_off[n + 1] - t0;
  if (k < 0 || base < 0 || base + k >= O) return;
  const int nsp = k >= 2 ? k * r : 0;
  if (nt != nsp + k || t0 < 0 || t0 + nt > T) return;
  for (int e = threadIdx.x; e < nt; e += TPB) {
    int64_t s, p, o;
    if (e < nsp) {
      const int i = e / r, q = e - i * r;
      const float* up = u + ((size_t)(base + i) * r + q) * 2;
      int j = (int)((double)up[0] * (double)(k - 1));
      j = j < k - 2 ? j : k - 2;
      j = j < 0 ? 0 : j;
      j += j >= i ? 1 : 0;
      const int a = up[1] > 0.5f ? i : j, b = up[1] > 0.5f ? j : i;
      s = base + a;
      o = base + b;
      p = derive_predicate(boxes, centers, base + a, base + b);
    } else {
      s = base + (e - nsp);
      p = 0;
      o = base + k;
    }
    int64_t* row = triples + (size_t)(t0 + e) * 3;
    row[0] = s;
    row[1] = p;
    row[2] = o;
    triple_to_img[t0 + e] = n;
  }
}

__global__ void __launch_bounds__(TPB) triple_agreement_kernel(const int64_t* __restrict__ triples, const float* __restrict__ boxes,
                                                              const float* __restrict__ centers, unsigned long long* __restrict__ counts,
                                                              int T, int O, int P) {
  __shared__ unsigned hist[2 * SG_SCENEGRAPH_MAX_P];
  const int tid = threadIdx.x, t = blockIdx.x * TPB + tid;
  for (int j = tid; j < 2 * P; j += TPB) hist[j] = 0u;
  __syncthreads();
  if (t < T) {
    const int64_t s = triples[(size_t)t * 3], p = triples[(size_t)t * 3 + 1], o = triples[(size_t)t * 3 + 2];
    if (p >= 1 && p < (int64_t)P && id_ok(s, O) && id_ok(o, O)) {
      atomicAdd(&hist[2 * (int)p], 1u);
      if (derive_predicate(boxes, centers, (int)s, (int)o) == (int)p) atomicAdd(&hist[2 * (int)p + 1], 1u);
    }
  }
  __syncthreads();
  for (int j = tid; j < 2 * P; j += TPB)
    if (hist[j]) atomicAdd(&counts[j], (unsigned long long)hist[j]);
}

__global__ void __launch_bounds__(TPB) attribute_agreement_kernel(const float* __restrict__ attrs, const int32_t* __restrict__ size_idx,
                                                                 const int32_t* __restrict__ loc_idx,
                                                                 unsigned long long* __restrict__ counts, int O, int S, int g) {
  __shared__ unsigned tot[4];
  const int tid = threadIdx.x, o = blockIdx.x * TPB + tid;
  if (tid < 4) tot[tid] = 0u;
  __syncthreads();
  unsigned v[4] = {0u, 0u, 0u, 0u};             // size seen, size agrees, location seen, location agrees
  if (o < O) {
    const int G = g * g;
    const float* row = attrs + (size_t)o * (S + G);
    int ns = 0, is = -1, nl = 0, il = -1;
    for (int a = 0; a < S; ++a)
      if (row[a] > 0.5f) { ++ns; is = a; }
    for (int a = 0; a < G; ++a)
      if (row[S + a] > 0.5f) { ++nl; il = a; }
    if (ns == 1) { v[0] = 1u; v[1] = is == size_idx[o] ? 1u : 0u; }
    if (nl == 1) { v[2] = 1u; v[3] = il == loc_idx[o] ? 1u : 0u; }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) v[e] += __shfl_xor(v[e], sh, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (v[e]) atomicAdd(&tot[e], v[e]);
  }
  __syncthreads();
  if (tid < 4 && tot[tid]) atomicAdd(&counts[tid], (unsigned long long)tot[tid]);
}

}  // namespace

extern "C" int sg_object_centers(const float* boxes, const void* masks, int masks_i64, float* centers, int32_t* count, int O, int M,
                                 sgStream stream) {
  SG_ARG_CHECK(O >= 0 && M >= 1 && M <= SG_SCENEGRAPH_MAX_M, "sg_object_centers: bad sizes (O=%d M=%d, M <= %d)", O, M,
               SG_SCENEGRAPH_MAX_M);
  if (O == 0) return 0;
  SG_ARG_CHECK(boxes && masks && centers && count, "sg_object_centers: null operand");
  hipStream_t s = (hipStream_t)stream;
  const int n = M * M, esz = masks_i64 ? 8 : 4;
  // 16-byte loads need every object's mask on a 16-byte boundary: an aligned base and a multiple of 16 bytes per mask
  const int vec = (reinterpret_cast<uintptr_t>(masks) & 15) == 0 && ((size_t)n * esz) % 16 == 0;
  const FastDiv fd((unsigned)M);
  SgProfScope prof(SG_K_SCENEGRAPH_CENTERS, s, 0.0, (double)O * ((double)n * esz + 28.0));
  if (M <= 16) {
    const dim3 grid(sg_cdiv(O, WPB));
    if (masks_i64) hipLaunchKernelGGL(centers_wave_kernel<true>, grid, dim3(TPB), 0, s, boxes, masks, centers, count, O, M, vec, fd);
    else hipLaunchKernelGGL(centers_wave_kernel<false>, grid, dim3(TPB), 0, s, boxes, masks, centers, count, O, M, vec, fd);
  } else {
    if (masks_i64) hipLaunchKernelGGL(centers_block_kernel<true>, dim3(O), dim3(TPB), 0, s, boxes, masks, centers, count, M, vec, fd);
    else hipLaunchKernelGGL(centers_block_kernel<false>, dim3(O), dim3(TPB), 0, s, boxes, masks, centers, count, M, vec, fd);
  }
  SG_LAUNCH_CHECK("sg_object_centers");
  return 0;
}

extern "C" int sg_object_attributes(const float* boxes, const float* centers, int32_t* size_idx, int32_t* loc_idx, float* onehot,
                                    int O, int S, int g, sgStream stream) {
  SG_ARG_CHECK(O >= 0 && S >= 1 && g >= 1 && g <= 1024, "sg_object_attributes: bad sizes (O=%d S=%d g=%d)", O, S, g);
  if (O == 0) return 0;
  SG_ARG_CHECK(boxes && centers && size_idx && loc_idx, "sg_object_attributes: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_SCENEGRAPH_DERIVE, s, 0.0, (double)O * (32.0 + (onehot ? 4.0 * (S + g * g) : 0.0)));
  hipLaunchKernelGGL(attributes_kernel, dim3(sg_cdiv(O, TPB)), dim3(TPB), 0, s, boxes, centers, size_idx, loc_idx, onehot, O, S, g);
  SG_LAUNCH_CHECK("sg_object_attributes");
  return 0;
}

extern "C" int sg_pair_predicates(const float* boxes, const float* centers, const int64_t* s, const int64_t* o, int idx_stride,
                                  int64_t* p, int p_stride, int T, int O, sgStream stream) {
  SG_ARG_CHECK(T >= 0 && O >= 0 && idx_stride >= 1 && p_stride >= 1, "sg_pair_predicates: bad sizes (T=%d O=%d)", T, O);
  if (T == 0) return 0;
  SG_ARG_CHECK(boxes && centers && s && o && p, "sg_pair_predicates: null operand");
  hipStream_t st = (hipStream_t)stream;
  SgProfScope prof(SG_K_SCENEGRAPH_DERIVE, st, 0.0, (double)T * 72.0);
  hipLaunchKernelGGL(predicates_kernel, dim3(sg_cdiv(T, TPB)), dim3(TPB), 0, st, boxes, centers, s, o, idx_stride, p, p_stride, T, O);
  SG_LAUNCH_CHECK("sg_pair_predicates");
  return 0;
}

extern "C" int sg_draw_pairs(const int32_t* seg_off, const int32_t* tri_off, const float* u, const float* boxes, const float* centers,
                             int64_t* triples, int64_t* triple_to_img, int N, int O, int T, int r, sgStream stream) {
  SG_ARG_CHECK(N >= 0 && O >= 0 && T >= 0 && r >= 1, "sg_draw_pairs: bad sizes (N=%d O=%d T=%d r=%d)", N, O, T, r);
  if (N == 0 || T == 0) return 0;
  SG_ARG_CHECK(seg_off && tri_off && u && boxes && centers && triples && triple_to_img, "sg_draw_pairs: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_SCENEGRAPH_DERIVE, s, 0.0, (double)T * 32.0 + (double)O * (8.0 * r + 24.0));
  hipLaunchKernelGGL(draw_pairs_kernel, dim3(N), dim3(TPB), 0, s, seg_off, tri_off, u, boxes, centers, triples, triple_to_img, O, T, r);
  SG_LAUNCH_CHECK("sg_draw_pairs");
  return 0;
}

extern "C" int sg_triple_agreement(const int64_t* triples, const float* boxes, const float* centers, int64_t* counts, int T, int O,
                                   int P, sgStream stream) {
  SG_ARG_CHECK(T >= 0 && O >= 0 && P >= 1 && P <= SG_SCENEGRAPH_MAX_P, "sg_triple_agreement: bad sizes (T=%d O=%d P=%d, P <= %d)", T, O,
               P, SG_SCENEGRAPH_MAX_P);
  if (T == 0) return 0;
  SG_ARG_CHECK(triples && boxes && centers && counts, "sg_triple_agreement: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_SCENEGRAPH_AGREE, s, 0.0, (double)T * 72.0);
  hipLaunchKernelGGL(triple_agreement_kernel, dim3(sg_cdiv(T, TPB)), dim3(TPB), 0, s, triples, boxes, centers,
                     reinterpret_cast<unsigned long long*>(counts), T, O, P);
  SG_LAUNCH_CHECK("sg_triple_agreement");
  return 0;
}

extern "C" int sg_attribute_agreement(const float* attrs, const int32_t* size_idx, const int32_t* loc_idx, int64_t* counts, int O,
                                      int S, int g, sgStream stream) {
  SG_ARG_CHECK(O >= 0 && S >= 1 && g >= 1 && g <= 1024, "sg_attribute_agreement: bad sizes (O=%d S=%d g=%d)", O, S, g);
  if (O == 0) return 0;
  SG_ARG_CHECK(attrs && size_idx && loc_idx && counts, "sg_attribute_agreement: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_SCENEGRAPH_AGREE, s, 0.0, (double)O * (4.0 * (S + g * g) + 8.0));
  hipLaunchKernelGGL(attribute_agreement_kernel, dim3(sg_cdiv(O, TPB)), dim3(TPB), 0, s, attrs, size_idx, loc_idx,
                     reinterpret_cast<unsigned long long*>(counts), O, S, g);
  SG_LAUNCH_CHECK("sg_attribute_agreement");
  return 0;
}
