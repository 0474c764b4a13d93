// Pillow's uint8 Image.resize (bilinear / bicubic), bit for bit, over a ragged batch of packed RGB images, with the loader's
// ToTensor + Normalize(0.5, 0.5) as a 256-entry table lookup (scene_generation_amd/imageprep.py, ops/imageprep.py).
//
//   sg_pil_resize_plan   host only: the device table and the workspace layout of a batch from its (offset, H, W) rows
//   sg_pil_resize        pil_coef_kernel (the fixed-point coefficients of every image and axis), pil_horizontal_kernel
//                        ([H, W, 3] -> [H, OW, 3] in the workspace), pil_vertical_kernel ([H, OW, 3] -> y8 [OH, OW, 3] and / or y [3, OH, OW])
//
// Two separable passes, as Pillow runs them: the horizontal one first, its result rounded to uint8, then the vertical one; a pass whose
// input and output length agree is skipped (the vertical kernel then copies, or reads the source image itself).  The coefficients are
// float64 arithmetic with NO contraction (an fma changes the last bit of center, of a weight or of their sum, and with it an occasional
// xmin or coefficient): every function of this file that computes them is under ``#pragma clang fp contract(off)``.  The passes are
// int32: 2^21 + sum pixel * k, >> 22, clamped to 0..255 -- exact, so the order of the taps is free.
//
// One thread owns one output BYTE column (pixel xx = c / 3, channel c % 3) in both passes.  The horizontal pass stages HROWS source
// rows in LDS as dwords loaded from the 4-byte aligned addresses below the rows' arbitrary starts, HCHUNK bytes of a row at a time (a
// tile's taps span a whole 8192-pixel row at the largest reduction: the tap loop runs over as many chunks as that takes).  Its ragged
// work -- ceil(H_i / HROWS) workgroups per image -- is found by a binary search of the host-computed prefix in the table; no grid is
// sized by the largest image.
#include <math.h>
#include "common.h"

namespace {

constexpr int TC = SG_PIL_TABLE_COLS;
// columns of the device table (int64 [N + 1][TC]; row N holds the totals of the prefix columns)
enum { T_OFF = 0, T_H, T_W, T_COEF_H, T_COEF_V, T_KSIZE_H, T_KSIZE_V, T_INTER, T_HBLOCK, T_COLS };
static_assert(T_COLS == TC, "table columns");

constexpr int PRECISION_BITS = 22;
constexpr int TPB = 256;            // threads = output byte columns of a tile, both passes
constexpr int HROWS = 8;            // source rows a horizontal workgroup resamples
constexpr int HCHUNK = SG_PIL_LDS_CHUNK;   // bytes of a source row staged in LDS at once
constexpr int HLD = HCHUNK / 4 + 1; // dwords per staged row: the chunk plus the up to 3 bytes below its first one
constexpr int VROWS = 4;            // output rows a vertical workgroup writes

// ---- the coefficients: float64, every operation rounded once -----------------------------------------------------------------------
#pragma clang fp contract(off)
__device__ __forceinline__ double pil_filter(double t, int bicubic) {
#pragma clang fp contract(off)
  if (t < 0.0) t = -t;
  if (!bicubic) return t < 1.0 ? 1.0 - t : 0.0;
  const double a = -0.5;
  if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
  if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * a;
  return 0.0;
}

// one thread per (image, axis, output index): p = {xmin, count, k[0 .. count)}, stride ksize + 2
__global__ void __launch_bounds__(TPB) pil_coef_kernel(const int64_t* __restrict__ table, int N, int OH, int OW, int bicubic,
                                                       int* __restrict__ coef) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int per = OW + OH;
  if (idx >= (int64_t)N * per) return;
  const int i = (int)(idx / per), r = (int)(idx - (int64_t)i * per);
  const int axis = r < OW ? 0 : 1, xx = axis ? r - OW : r;
  const int64_t* row = table + (size_t)i * TC;
  const int64_t base = row[T_COEF_H + axis];
  if (base < 0) return;                                     // a skipped pass
  const int n_in = (int)row[axis ? T_H : T_W], n_out = axis ? OH : OW, ksize = (int)row[T_KSIZE_H + axis];
  const double S = bicubic ? 2.0 : 1.0;
  const double scale = (double)n_in / (double)n_out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = S * fs;
  const double ss = 1.0 / fs;
  const double center = ((double)xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > n_in) xmax = n_in;
  int count = xmax - xmin;
  count = count < 0 ? 0 : (count > ksize ? ksize : count);  // never taken: the plan's ksize is Pillow's, which bounds the count
  double ww = 0.0;
  for (int x = 0; x < count; ++x) ww += pil_filter(((double)(x + xmin) - center + 0.5) * ss, bicubic);
  int* p = coef + base + (size_t)xx * (ksize + 2);
  p[0] = xmin;
  p[1] = count;
  for (int x = 0; x < count; ++x) {
    double w = pil_filter(((double)(x + xmin) - center + 0.5) * ss, bicubic);
    if (ww != 0.0) w = w / ww;
    const double f = w * (double)(1 << PRECISION_BITS);
    p[2 + x] = w < 0.0 ? (int)(-0.5 + f) : (int)(0.5 + f);
  }
}

// ---- the passes ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// the aligned dword at byte ``pos`` (a multiple of 4) of a buffer of ``len`` bytes; bytes past the end read as zero
__device__ __forceinline__ uint32_t load_dword(const uint8_t* __restrict__ buf, int64_t len, int64_t pos) {
  if (pos + 4 <= len) return *reinterpret_cast<const uint32_t*>(buf + pos);
  uint32_t v = 0;
  for (int b = 0; b < 4; ++b)
    if (pos + b < len) v |= (uint32_t)buf[pos + b] << (8 * b);
  return v;
}

// the image whose horizontal workgroups include number b: the last row i of the prefix column with table[i][T_HBLOCK] <= b
__device__ __forceinline__ int find_image(const int64_t* __restrict__ table, int N, int64_t b) {
  int lo = 0, hi = N;                                       // invariant: prefix[lo] <= b < prefix[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[(size_t)mid * TC + T_HBLOCK] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// [H, W, 3] -> inter [H, OW, 3].  grid.x: the images' row groups back to back (prefix in the table), grid.y: tiles of TPB byte columns
__global__ void __launch_bounds__(TPB) pil_horizontal_kernel(const uint8_t* __restrict__ packed, int64_t packed_bytes,
                                                             const int64_t* __restrict__ table, int N, int OW,
                                                             const int* __restrict__ coef, uint8_t* __restrict__ inter) {
  __shared__ uint32_t lds[HROWS * HLD];
  const int tid = threadIdx.x;
  const int i = find_image(table, N, blockIdx.x);
  const int64_t* row = table + (size_t)i * TC;
  const int H = (int)row[T_H], W = (int)row[T_W], ksize = (int)row[T_KSIZE_H];
  const int y0 = (int)((int64_t)blockIdx.x - row[T_HBLOCK]) * HROWS;
  const int nrows = H - y0 < HROWS ? H - y0 : HROWS;
  const int64_t rowbytes = (int64_t)W * 3, src0 = row[T_OFF] + (int64_t)y0 * rowbytes;
  const int* cf = coef + row[T_COEF_H];
  const int cols = OW * 3, c0 = blockIdx.y * TPB, c = c0 + tid;
  const bool active = c < cols;
  const int xx = active ? c / 3 : 0, ch = c - 3 * (c / 3);
  const int* p = cf + (size_t)xx * (ksize + 2);
  const int first = active ? p[0] * 3 + ch : 0, count = active ? p[1] : 0;      // my taps: source bytes first, first + 3, ...
  // the tile's span of source bytes (xmin and xmin + count do not decrease with xx)
  const int xa = c0 / 3, xb = (c0 + TPB - 1 < cols ? c0 + TPB - 1 : cols - 1) / 3;
  const int* pa = cf + (size_t)xa * (ksize + 2);
  const int* pb = cf + (size_t)xb * (ksize + 2);
  const int b0 = pa[0] * 3, b1 = (pb[0] + pb[1]) * 3;
  int acc[HROWS];
#pragma unroll
  for (int r = 0; r < HROWS; ++r) acc[r] = 1 << (PRECISION_BITS - 1);
  for (int s = b0; s < b1; s += HCHUNK) {
    const int len = b1 - s < HCHUNK ? b1 - s : HCHUNK;
    __syncthreads();
    for (int e = tid; e < nrows * HLD; e += TPB) {
      const int r = e / HLD, d = e - r * HLD;
      const int64_t g = src0 + (int64_t)r * rowbytes + s;   // first byte of the chunk in row r
      const int sh = (int)(g & 3);
      if (d * 4 < sh + len) lds[e] = load_dword(packed, packed_bytes, (g - sh) + 4 * (int64_t)d);
    }
    __syncthreads();
    // my taps inside [s, s + len): j with s <= first + 3 j < s + len
    int jlo = s > first ? (s - first + 2) / 3 : 0;
    int jhi = (s + len - first + 2) / 3;
    jhi = s + len > first ? (jhi < count ? jhi : count) : 0;
    const uint8_t* lb[HROWS];                                // row r's byte ``s`` in LDS
#pragma unroll
    for (int r = 0; r < HROWS; ++r) lb[r] = reinterpret_cast<const uint8_t*>(lds) + r * (HLD * 4) + (int)((src0 + (int64_t)r * rowbytes + s) & 3);
    for (int j = jlo; j < jhi; ++j) {
      const int k = p[2 + j], at = first + 3 * j - s;
#pragma unroll
      for (int r = 0; r < HROWS; ++r) acc[r] += (int)lb[r][at] * k;      // rows past nrows read stale LDS and are not stored
    }
  }
  if (!active) return;
  uint8_t* out = inter + row[T_INTER] + (int64_t)y0 * cols + c;
#pragma unroll
  for (int r = 0; r < HROWS; ++r)
    if (r < nrows) out[(int64_t)r * cols] = (uint8_t)clip8(acc[r]);
}

// [H, OW, 3] (the workspace, or the source itself when the horizontal pass was skipped) -> y8 [N, OH, OW, 3] and / or y [N, 3, OH, OW].
// grid.x = N * ceil(OH / VROWS), grid.y: tiles of TPB byte columns.  The taps of an output row are the same for every thread of the
// workgroup (scalar loads); the source bytes of one tap are TPB consecutive bytes.
__global__ void __launch_bounds__(TPB) pil_vertical_kernel(const uint8_t* __restrict__ packed, const int64_t* __restrict__ table,
                                                           int OH, int OW, int vgroups, const int* __restrict__ coef,
                                                           const uint8_t* __restrict__ inter, const float* __restrict__ lut,
                                                           uint8_t* __restrict__ y8, float* __restrict__ y) {
  const int i = blockIdx.x / vgroups, yy0 = (blockIdx.x - i * vgroups) * VROWS;
  const int64_t* row = table + (size_t)i * TC;
  const int cols = OW * 3, c = blockIdx.y * TPB + threadIdx.x;
  if (c >= cols) return;
  const int xx = c / 3, ch = c - 3 * xx;
  const uint8_t* src = row[T_COEF_H] >= 0 ? inter + row[T_INTER] : packed + row[T_OFF];
  const int64_t cv = row[T_COEF_V];
  const int ksize = (int)row[T_KSIZE_V];
  for (int yy = yy0; yy < yy0 + VROWS && yy < OH; ++yy) {
    int v;
    if (cv < 0) {
      v = src[(int64_t)yy * cols + c];                        // H == OH: the identity
    } else {
      const int* p = coef + cv + (size_t)yy * (ksize + 2);
      const int ymin = p[0], count = p[1];
      const uint8_t* s = src + (int64_t)ymin * cols + c;
      int acc = 1 << (PRECISION_BITS - 1);
      for (int j = 0; j < count; ++j) acc += (int)s[(int64_t)j * cols] * p[2 + j];
      v = clip8(acc);
    }
    if (y8) y8[((int64_t)i * OH + yy) * cols + c] = (uint8_t)v;
    if (y) y[(((int64_t)i * 3 + ch) * OH + yy) * OW + xx] = lut[v];
  }
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }
inline int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// Pillow's ksize: (int)ceil(support) * 2 + 1, support = S * max(in / out, 1), in doubles
inline int64_t pil_ksize(int n_in, int n_out, int bicubic) {
  const double scale = (double)n_in / (double)n_out;
  const double support = (bicubic ? 2.0 : 1.0) * (scale < 1.0 ? 1.0 : scale);
  return (int64_t)ceil(support) * 2 + 1;
}

}  // namespace

extern "C" int sg_pil_resize_plan(const int64_t* desc_host, int N, int64_t packed_bytes, int OH, int OW, int filter, int64_t* table_host,
                                  int64_t* totals_host) {
  SG_ARG_CHECK(N >= 0 && N <= SG_PIL_MAX_IMAGES, "sg_pil_resize_plan: N=%d is outside 0..%d", N, SG_PIL_MAX_IMAGES);
  SG_ARG_CHECK(OH >= 1 && OW >= 1 && OH <= SG_PIL_MAX_OUT && OW <= SG_PIL_MAX_OUT, "sg_pil_resize_plan: target %d x %d is outside 1..%d",
               OH, OW, SG_PIL_MAX_OUT);
  SG_ARG_CHECK(filter == SG_PIL_BILINEAR || filter == SG_PIL_BICUBIC, "sg_pil_resize_plan: filter=%d is neither bilinear nor bicubic", filter);
  SG_ARG_CHECK(table_host && totals_host && (desc_host || N == 0), "sg_pil_resize_plan: null operand");
  const int bicubic = filter == SG_PIL_BICUBIC;
  int64_t coef = 0, inter = 0, hblocks = 0;
  for (int i = 0; i < N; ++i) {
    const int64_t off = desc_host[3 * i], H = desc_host[3 * i + 1], W = desc_host[3 * i + 2];
    SG_ARG_CHECK(H >= 1 && W >= 1 && H <= SG_PIL_MAX_IN && W <= SG_PIL_MAX_IN, "sg_pil_resize_plan: image %d is %lld x %lld, outside 1..%d",
                 i, (long long)H, (long long)W, SG_PIL_MAX_IN);
    SG_ARG_CHECK(off >= 0 && off + H * W * 3 <= packed_bytes, "sg_pil_resize_plan: image %d (%lld bytes at offset %lld) leaves the buffer of %lld bytes",
                 i, (long long)(H * W * 3), (long long)off, (long long)packed_bytes);
    int64_t* row = table_host + (size_t)i * TC;
    const bool horizontal = W != OW, vertical = H != OH;
    row[T_OFF] = off; row[T_H] = H; row[T_W] = W;
    row[T_KSIZE_H] = horizontal ? pil_ksize((int)W, OW, bicubic) : 0;
    row[T_KSIZE_V] = vertical ? pil_ksize((int)H, OH, bicubic) : 0;
    row[T_COEF_H] = horizontal ? coef : -1;
    if (horizontal) coef += (row[T_KSIZE_H] + 2) * OW;
    row[T_COEF_V] = vertical ? coef : -1;
    if (vertical) coef += (row[T_KSIZE_V] + 2) * OH;
    row[T_INTER] = horizontal ? inter : -1;
    if (horizontal) inter += H * OW * 3;
    row[T_HBLOCK] = hblocks;
    if (horizontal) hblocks += (H + HROWS - 1) / HROWS;
  }
  int64_t* last = table_host + (size_t)N * TC;
  for (int k = 0; k < TC; ++k) last[k] = 0;
  last[T_HBLOCK] = hblocks;
  SG_ARG_CHECK(hblocks <= 2147483647LL, "sg_pil_resize_plan: %lld row groups are beyond the launch grid", (long long)hblocks);
  totals_host[0] = coef;
  totals_host[1] = inter;
  totals_host[2] = hblocks;
  totals_host[3] = round_up(coef * 4, 16) + round_up(inter, 16);
  return 0;
}

extern "C" int sg_pil_resize(const void* packed, int64_t packed_bytes, const int64_t* table, int N, int OH, int OW, int filter,
                             int64_t coef_ints, int64_t inter_bytes, int64_t hblocks, const float* lut, void* y8, float* y, void* ws,
                             size_t ws_bytes, int phases, sgStream stream) {
  SG_ARG_CHECK(N >= 0 && N <= SG_PIL_MAX_IMAGES, "sg_pil_resize: N=%d is outside 0..%d", N, SG_PIL_MAX_IMAGES);
  SG_ARG_CHECK(OH >= 1 && OW >= 1 && OH <= SG_PIL_MAX_OUT && OW <= SG_PIL_MAX_OUT, "sg_pil_resize: target %d x %d is outside 1..%d", OH, OW,
               SG_PIL_MAX_OUT);
  SG_ARG_CHECK(filter == SG_PIL_BILINEAR || filter == SG_PIL_BICUBIC, "sg_pil_resize: filter=%d is neither bilinear nor bicubic", filter);
  SG_ARG_CHECK(phases >= 1 && phases <= SG_PIL_ALL, "sg_pil_resize: phases=%d is outside 1..%d", phases, SG_PIL_ALL);
  if (N == 0) return 0;
  SG_ARG_CHECK(coef_ints >= 0 && inter_bytes >= 0 && hblocks >= 0 && hblocks <= 2147483647LL && packed_bytes >= 3,
               "sg_pil_resize: bad totals (coef_ints=%lld inter_bytes=%lld hblocks=%lld packed_bytes=%lld)", (long long)coef_ints,
               (long long)inter_bytes, (long long)hblocks, (long long)packed_bytes);
  SG_ARG_CHECK(packed && table && (y8 || y) && ws && (lut || !y), "sg_pil_resize: null operand");
  SG_ARG_CHECK(aligned(packed, 4) && aligned(table, 8) && aligned(lut, 4) && aligned(y, 4) && aligned(ws, 16),
               "sg_pil_resize: packed, lut and y must be 4-byte, the table 8-byte and ws 16-byte aligned");
  const size_t need = (size_t)(round_up(coef_ints * 4, 16) + round_up(inter_bytes, 16));
  SG_ARG_CHECK(ws_bytes >= need, "sg_pil_resize: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  int* coef = (int*)ws;
  uint8_t* inter = (uint8_t*)ws + round_up(coef_ints * 4, 16);
  const int tiles = sg_cdiv((int64_t)OW * 3, TPB), vgroups = sg_cdiv(OH, VROWS);
  const double out_bytes = (double)N * OH * OW * 3 * ((y8 ? 1.0 : 0.0) + (y ? 4.0 : 0.0));
  SgProfScope prof(SG_K_PIL_RESIZE, st, 0.0, (double)packed_bytes + 2.0 * (double)inter_bytes + 8.0 * (double)coef_ints + out_bytes);
  if (coef_ints > 0 && (phases & SG_PIL_COEF))
    hipLaunchKernelGGL(pil_coef_kernel, dim3((unsigned)sg_cdiv((int64_t)N * (OW + OH), TPB)), dim3(TPB), 0, st, table, N, OH, OW,
                       filter == SG_PIL_BICUBIC ? 1 : 0, coef);
  if (hblocks > 0 && (phases & SG_PIL_HORIZONTAL))
    hipLaunchKernelGGL(pil_horizontal_kernel, dim3((unsigned)hblocks, (unsigned)tiles), dim3(TPB), 0, st, (const uint8_t*)packed,
                       packed_bytes, table, N, OW, coef, inter);
  if (phases & SG_PIL_VERTICAL)
    hipLaunchKernelGGL(pil_vertical_kernel, dim3((unsigned)(N * vgroups), (unsigned)tiles), dim3(TPB), 0, st, (const uint8_t*)packed, table,
                       OH, OW, vgroups, coef, inter, lut, (uint8_t*)y8, y);
  SG_LAUNCH_CHECK("sg_pil_resize");
  return 0;
}
