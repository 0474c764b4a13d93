// Size and location attributes from class statistics (scene_generation_amd/attributes.py): the two ends of the reference's
// attribute sampler.  sg_attribute_histogram counts, per object class, how often each size bucket and each location cell occurs
// (scripts/create_attributes_file.py); sg_sample_attributes draws every object's missing size / location bit from those counts,
// the locations constrained by the graph's relations (data/coco_panoptic.py:336-340,389-391,432-449,468-521).  The exact rules
// are the comment of the two entry points in include/sg2im_hip.h.
//
// Everything is integer arithmetic but one fp64 product per draw, whose operands do not depend on any evaluation order: the
// weights are int64, their prefix sums are exact, and the threshold is double(u) * double(sum).  The histogram uses integer
// atomics.  Results are bit-identical from run to run.  Nothing here allocates or synchronises.
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int MAXO = SG_ATTR_MAX_OBJS;
constexpr unsigned char F_REAL = 1, F_SIZE_GIVEN = 2;

__global__ void __launch_bounds__(TPB) attribute_histogram_kernel(const int64_t* __restrict__ objs, const float* __restrict__ attrs,
                                                                 unsigned long long* __restrict__ counts, int O, int C, int S, int G,
                                                                 int image_class) {
  const int o = blockIdx.x * TPB + threadIdx.x;
  if (o >= O) return;
  const int64_t c = objs[o];
  if (c < 0 || c >= (int64_t)C || c == (int64_t)image_class) return;
  const int A = S + G;
  const float* row = attrs + (size_t)o * A;
  unsigned long long* out = counts + (size_t)c * A;
  for (int a = 0; a < S; ++a)
    if (row[a] > 0.5f) { atomicAdd(&out[a], 1ull); break; }
  for (int a = 0; a < G; ++a)
    if (row[S + a] > 0.5f) { atomicAdd(&out[S + a], 1ull); break; }
}

// first index of the sorted vector v [n] that is >= key (every lane of the wave walks the same path)
__device__ __forceinline__ int lower_bound(const int64_t* __restrict__ v, int n, int64_t key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ long long wave_inclusive_scan(long long v, int lane) {
#pragma unroll
  for (int d = 1; d < SG_WAVE; d <<= 1) {
    const long long t = __shfl_up(v, d, SG_WAVE);
    if (lane >= d) v += t;
  }
  return v;
}

// draw(w, allowed, u) with one lane per cell; called by the whole wave with wave-uniform hist / n / u.  hist: the n int64 counts
// of the class, or null for a class outside the table (all zero).  allowed implies lane < n.
__device__ __forceinline__ int wave_draw(const int64_t* __restrict__ hist, int n, bool allowed, float u, int lane) {
  long long p = wave_inclusive_scan((hist && allowed) ? (long long)hist[lane] : 0ll, lane);
  long long sum = __shfl(p, SG_WAVE - 1, SG_WAVE);
  if (sum == 0) {                               // never seen, or never seen in the allowed cells: uniform over the allowed cells
    p = wave_inclusive_scan(allowed ? 1ll : 0ll, lane);
    sum = __shfl(p, SG_WAVE - 1, SG_WAVE);
  }
  u = fminf(fmaxf(u, 0.f), 0x1.fffffep-1f);     // [0, 1 - 2^-24]; a NaN lands on 0
  const double t = (double)u * (double)sum;
  const unsigned long long m = __ballot(lane < n && (double)p > t);
  return m ? __ffsll((long long)m) - 1 : n - 1;         // (m == 0 needs negative counts)
}

// One wavefront (= one workgroup) per image.  Phases: per-object loads; given bits, size draws and the __image__ object; the
// serial triple walk; the unrestricted draws of what is left; the outputs.  Per-object state lives in LDS, written by lane 0
// and read by every lane at one address (a broadcast), so every branch below is wave-uniform.
__global__ void __launch_bounds__(SG_WAVE) sample_attributes_kernel(
    const int64_t* __restrict__ objs, const int64_t* __restrict__ obj_to_img, const int64_t* __restrict__ triples,
    const int64_t* __restrict__ triple_to_img, const int64_t* __restrict__ counts, const float* __restrict__ u,
    const float* __restrict__ given, int32_t* __restrict__ size_idx, int32_t* __restrict__ loc_idx, float* __restrict__ attrs, int N,
    int O, int T, int C, int S, int g, int image_class, int rule, FastDiv fd) {
  __shared__ short s_size[MAXO], s_loc[MAXO];
  __shared__ int s_cls[MAXO];
  __shared__ float s_u1[MAXO];
  __shared__ unsigned char s_flag[MAXO];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int G = g * g, A = S + G;
  const int ob = lower_bound(obj_to_img, O, n), oe = lower_bound(obj_to_img, O, (int64_t)n + 1);
  const int k = n < N ? (oe - ob < MAXO ? oe - ob : MAXO) : 0;      // objects of the image that take part
  const int tb = k > 0 ? lower_bound(triple_to_img, T, n) : 0, te = k > 0 ? lower_bound(triple_to_img, T, (int64_t)n + 1) : 0;

  for (int i = lane; i < k; i += SG_WAVE) {
    const int64_t c = objs[ob + i];
    s_cls[i] = (c >= 0 && c < (int64_t)C) ? (int)c : -1;
    s_u1[i] = u[2 * (size_t)(ob + i) + 1];
    s_flag[i] = c != (int64_t)image_class ? F_REAL : 0;
  }
  __syncthreads();

  // given bits win; a real object without a size draws one; the __image__ object takes the last size and the centre cell
  const int cc = (int)rint(0.5 * (double)(g - 1)), image_cell = cc + g * cc;
  for (int i = 0; i < k; ++i) {
    const int o = ob + i;
    int sz = -1, lc = -1;
    if (given) {
      const float* row = given + (size_t)o * A;
      const unsigned long long ms = __ballot(lane < S && row[lane] > 0.5f);
      const unsigned long long ml = __ballot(lane < G && row[S + lane] > 0.5f);
      sz = ms ? __ffsll((long long)ms) - 1 : -1;
      lc = ml ? __ffsll((long long)ml) - 1 : -1;
    }
    unsigned char flag = s_flag[i];
    const bool real = (flag & F_REAL) != 0;
    if (sz >= 0) {
      flag |= F_SIZE_GIVEN;
    } else if (real) {
      const int c = s_cls[i];
      sz = wave_draw(c >= 0 ? counts + (size_t)c * A : nullptr, S, lane < S, u[2 * (size_t)o], lane);
    } else {
      sz = S - 1;
    }
    if (lc < 0 && !real) lc = image_cell;
    if (lane == 0) {
      s_size[i] = (short)sz;
      s_loc[i] = (short)lc;
      s_flag[i] = flag;
    }
  }
  __syncthreads();

  // step(a, q, b) of the rules; every argument is wave-uniform
  auto step = [&](int a, int q, int b) {
    if (s_loc[a] >= 0) return;
    const int lb = s_loc[b], c = s_cls[a];
    const int64_t* hist = c >= 0 ? counts + (size_t)c * A + S : nullptr;
    int la, sa = -1;
    if (lb < 0) {
      la = wave_draw(hist, G, lane < G, s_u1[a], lane);
    } else if (q >= 5) {
      la = lb;
      if (!(s_flag[a] & F_SIZE_GIVEN)) {
        const int za = s_size[a], zb = s_size[b];
        const int up = zb + 1 < S - 1 ? zb + 1 : S - 1, down = zb - 1 > 0 ? zb - 1 : 0;
        if (rule == SG_ATTR_RULE_REFERENCE) {
          if (q == 6 && zb <= za) sa = down;
          if (q == 5 && zb >= za) sa = up;
        } else {
          if (q == 6 && za <= zb) sa = up;
          if (q == 5 && za >= zb) sa = down;
        }
      }
    } else {
      const int colb = lb % g, rowb = lb / g, col = lane % g, row = lane / g;
      bool allowed;
      if (q == 1) allowed = col <= (colb - 1 > 0 ? colb - 1 : 0);
      else if (q == 2) allowed = col >= (colb + 1 < g - 1 ? colb + 1 : g - 1);
      else if (q == 3) allowed = row <= (rowb - 1 > 0 ? rowb - 1 : 0);
      else allowed = row >= (rowb + 1 < g - 1 ? rowb + 1 : g - 1);
      la = wave_draw(hist, G, allowed && lane < G, s_u1[a], lane);
    }
    if (lane == 0) {
      s_loc[a] = (short)la;
      if (sa >= 0) s_size[a] = (short)sa;
    }
    __syncthreads();
  };

  // the triples in stored order, 64 at a time: a lane loads and screens one, then the kept ones are walked serially
  for (int base = tb; base < te; base += SG_WAVE) {
    const int t = base + lane;
    int a = -1, b = -1, p = 0;
    if (t < te) {
      const int64_t s = triples[(size_t)t * 3], pp = triples[(size_t)t * 3 + 1], o = triples[(size_t)t * 3 + 2];
      if (pp >= 1 && pp <= 6 && s != o && s >= ob && s < (int64_t)ob + k && o >= ob && o < (int64_t)ob + k) {
        a = (int)(s - ob);
        b = (int)(o - ob);
        p = (int)pp;
        if (!(s_flag[a] & F_REAL) || !(s_flag[b] & F_REAL)) a = -1;
      }
    }
    unsigned long long m = __ballot(a >= 0);
    while (m) {
      const int j = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int aj = __shfl(a, j, SG_WAVE), bj = __shfl(b, j, SG_WAVE), pj = __shfl(p, j, SG_WAVE);
      step(aj, pj, bj);
      step(bj, ((pj - 1) ^ 1) + 1, aj);
    }
  }

  // real objects no relation reached
  for (int i = 0; i < k; ++i) {
    if (s_loc[i] >= 0 || !(s_flag[i] & F_REAL)) continue;
    const int c = s_cls[i];
    const int la = wave_draw(c >= 0 ? counts + (size_t)c * A + S : nullptr, G, lane < G, s_u1[i], lane);
    if (lane == 0) s_loc[i] = (short)la;
  }
  __syncthreads();

  // every element of the outputs: the first and the last wave also cover objects that belong to no image of the call
  const int lo = n == 0 ? 0 : ob, hi = n >= N - 1 ? O : oe;
  for (int o = lo + lane; o < hi; o += SG_WAVE) {
    const int i = o - ob;
    const bool in = i >= 0 && i < k;
    size_idx[o] = in ? (int)s_size[i] : -1;
    loc_idx[o] = in ? (int)s_loc[i] : -1;
  }
  for (int e = lo * A + lane; e < hi * A; e += SG_WAVE) {
    const int o = (int)fd.div((unsigned)e), a = e - o * A, i = o - ob;
    const bool in = i >= 0 && i < k;
    const int hot = !in ? -1 : (a < S ? (int)s_size[i] : ((int)s_loc[i] >= 0 ? S + (int)s_loc[i] : -1));
    attrs[e] = a == hot ? 1.f : 0.f;
  }
}

}  // namespace

extern "C" int sg_attribute_histogram(const int64_t* objs, const float* attrs, int64_t* counts, int O, int C, int S, int g,
                                      int image_class, sgStream stream) {
  SG_ARG_CHECK(O >= 0 && C >= 1 && S >= 1 && g >= 1 && g <= 1024, "sg_attribute_histogram: bad sizes (O=%d C=%d S=%d g=%d)", O, C, S, g);
  if (O == 0) return 0;
  SG_ARG_CHECK(objs && attrs && counts, "sg_attribute_histogram: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_ATTRIBUTES_HIST, s, 0.0, (double)O * (4.0 * (S + g * g) + 24.0));
  hipLaunchKernelGGL(attribute_histogram_kernel, dim3(sg_cdiv(O, TPB)), dim3(TPB), 0, s, objs, attrs,
                     reinterpret_cast<unsigned long long*>(counts), O, C, S, g * g, image_class);
  SG_LAUNCH_CHECK("sg_attribute_histogram");
  return 0;
}

extern "C" int sg_sample_attributes(const int64_t* objs, const int64_t* obj_to_img, const int64_t* triples, const int64_t* triple_to_img,
                                    const int64_t* counts, const float* u, const float* given, int32_t* size_idx, int32_t* loc_idx,
                                    float* attrs, int N, int O, int T, int C, int S, int g, int image_class, int size_rule,
                                    sgStream stream) {
  SG_ARG_CHECK(N >= 0 && O >= 0 && T >= 0 && C >= 1, "sg_sample_attributes: bad sizes (N=%d O=%d T=%d C=%d)", N, O, T, C);
  SG_ARG_CHECK(S >= 1 && S <= SG_WAVE && g >= 1 && g * g <= SG_WAVE,
               "sg_sample_attributes: a draw holds one cell per lane: S=%d and g*g=%d must be in 1..%d", S, g * g, SG_WAVE);
  SG_ARG_CHECK((int64_t)O * (S + g * g) < ((int64_t)1 << 31), "sg_sample_attributes: O * (S + g*g) must stay below 2^31 (O=%d)", O);
  SG_ARG_CHECK(size_rule == SG_ATTR_RULE_REFERENCE || size_rule == SG_ATTR_RULE_GEOMETRIC, "sg_sample_attributes: size_rule %d",
               size_rule);
  if (O == 0) return 0;
  SG_ARG_CHECK(objs && obj_to_img && counts && u && size_idx && loc_idx && attrs && (T == 0 || (triples && triple_to_img)),
               "sg_sample_attributes: null operand");
  hipStream_t s = (hipStream_t)stream;
  SgProfScope prof(SG_K_ATTRIBUTES_SAMPLE, s, 0.0, (double)O * (8.0 * (S + g * g) + 40.0) + (double)T * 32.0);
  hipLaunchKernelGGL(sample_attributes_kernel, dim3(N > 0 ? N : 1), dim3(SG_WAVE), 0, s, objs, obj_to_img, triples, triple_to_img,
                     counts, u, given, size_idx, loc_idx, attrs, N, O, T, C, S, g, image_class, size_rule, FastDiv((unsigned)(S + g * g)));
  SG_LAUNCH_CHECK("sg_sample_attributes");
  return 0;
}
