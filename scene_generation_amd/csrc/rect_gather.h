// The rectangular gather of the forward convolutions with separate kernel extents and paddings: sg_conv2d_rect_fwd (inception.hip,
// at most 25 taps) and sg_conv2d_wide_fwd (lpips.hip, up to 11 x 11) instantiate it with their own tap-table size, and run the one
// host body below (rect_fwd) behind their own limits, tile choice and tile dispatch.  Included after igemm_core.h by those two units;
// everything has internal linkage.
#pragma once
#include "igemm_core.h"
#include <string>

namespace {

constexpr int RECT_TPB = 256;

// ---- B operand of the rectangular forward conv: k = (c, kh, kw), n = (img, oh, ow) ------------------------------------------------
// LoadGatherKN (igemm_core.h) with the kernel extents and the two paddings as run-time fields: the per-workgroup LDS table
// tap[t][pixel] of plane offsets is built from (KH, KW, padH, padW) and has room for MAXTAPS taps plus the all-invalid row the
// k-table's tail entries (k >= K) select; the k -> (channel offset, tap row) split is the same device table (build_ktab_kernel with
// KS2 = KH * KW).  Zero padding only, one source.
template <int BN, int MAXTAPS>
struct LoadGatherRect {
  Gather g; int Npix; const KEntry* ktab; int KH, KW, padH, padW;
  static constexpr int LDS_INTS = (MAXTAPS + 1) * BN;
  static constexpr int ROWS = BN * BK / 256;
  static constexpr bool BUF = SG_BUFLOAD != 0;
  struct Stage { float r[ROWS]; unsigned ok; KEntry e[ROWS]; };
  unsigned img1_;
  int nl_, kr_;
  const int* tab_;
  __device__ __forceinline__ void set_batch(int, int, int) {}
  __device__ __forceinline__ void init(int n0, int tid, int* tab, int, int) {
    nl_ = tid % BN;
    const int grp = tid / BN;
    kr_ = __builtin_amdgcn_readfirstlane(grp * ROWS);          // wave-uniform (BN >= 64) => ktab entries live in SGPRs
    const int n = n0 + nl_;
    const bool okn = n < Npix;
    const int nn = okn ? n : 0;
    const int phw = g.PH * g.PW;
    const int img = nn / phw;
    const int pix = nn - img * phw;
    const int ph = pix / g.PW, pw = pix - ph * g.PW;
    const int ah = ph * g.stride - padH, aw = pw * g.stride - padW;
    img1_ = (unsigned)img * (unsigned)g.C1 * (unsigned)(g.SH * g.SW);
    const int KS2 = KH * KW;
    constexpr int G = 256 / BN;
    for (int t = grp; t <= KS2; t += G) {
      const int kh = t / KW, kw = t - kh * KW;
      const int ih = ah + kh, iw = aw + kw;
      const bool inside = okn && t < KS2 && (unsigned)ih < (unsigned)g.SH && (unsigned)iw < (unsigned)g.SW;
      tab[t * BN + nl_] = inside ? ih * g.SW + iw : TAP_INVALID;
    }
    tab_ = tab + nl_;
  }
  __device__ __forceinline__ void prefetch(Stage& st, int k0) const {
    const KEntry* e = ktab + (k0 + kr_);          // uniform address => scalar loads
#pragma unroll
    for (int i = 0; i < ROWS; ++i) st.e[i] = e[i];
  }
  __device__ __forceinline__ void load(Stage& st, int, int) const {
    st.ok = 0;
#if SG_BUFLOAD
    const __amdgpu_buffer_rsrc_t r1 = sg_rsrc(g.src1);
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const unsigned tp = (unsigned)tab_[(st.e[i].tapsel & 255u) * BN];
      st.r[i] = sg_bufload(r1, img1_ + st.e[i].choff + tp);        // an invalid tap lands beyond the range check => 0
    }
#else
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const int tp = tab_[(st.e[i].tapsel & 255u) * BN];
      const bool ok = tp >= 0;
      st.r[i] = g.src1[ok ? img1_ + st.e[i].choff + (unsigned)tp : 0u];
      st.ok |= ok ? (1u << i) : 0u;
    }
#endif
  }
  __device__ __forceinline__ void store(const Stage& st, float* T) const {
    if (BUF) store_krun<ROWS, false>(T, nl_, kr_, st.r, 0u);
    else store_krun<ROWS, true>(T, nl_, kr_, st.r, st.ok);
  }
};

// split-K epilogue: y[img][c0 + m][pix] = act(sum_z ws[z][img][m][pix] + bias[m]), slabs added in ascending z
__global__ void __launch_bounds__(RECT_TPB) rect_reduce_kernel(const float* __restrict__ ws, float* __restrict__ y, unsigned n, int S,
                                                         const float* __restrict__ bias, int PHW, int M, int c0, int ctot, int act,
                                                         FastDiv fphw, FastDiv fm) {
  const unsigned i = blockIdx.x * RECT_TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned plane = fphw.div(i), pix = i - plane * (unsigned)PHW;
  const unsigned img = fm.div(plane), m = plane - img * (unsigned)M;
  float v = sg_sum_strided(ws + i, n, S);
  if (bias) v += bias[m];
  y[((size_t)img * ctot + c0 + m) * PHW + pix] = sg_apply_act(v, act, 0.f);
}

struct RectPlan { int tile, bm, bn, vec, splits, kchunk; };

// splits: the reduction cut into k-chunks of whole k-tiles, at least 256 deep, when the tiles alone leave compute units idle; the
// chunks are written as slabs and added in order by rect_reduce_kernel.  Fills splits / kchunk of a plan whose tile is chosen.
inline void rect_plan_splits(RectPlan& p, int M, int K, long Npix) {
  const long tiles = (long)sg_cdiv(M, p.bm) * sg_cdiv(Npix, p.bn);
  int sp = 1;
  if (K >= 1024 && tiles <= 256) {
    sp = (int)(512 / tiles);
    if (sp > K / 256) sp = K / 256;
    if (sp > 8) sp = 8;
    if (sp > 2 && (sp & 1)) ++sp;          // (odd counts measured slower than their even neighbours on the square gathers)
    if (sp > 8) sp = 8;
  }
  p.splits = 1; p.kchunk = K;
  if (sp > 1) {
    p.kchunk = sg_cdiv(sg_cdiv(K, sp), BK * SG_NSUB) * (BK * SG_NSUB);      // what launch_cfg rounds a chunk to
    p.splits = sg_cdiv(K, p.kchunk);
    if (p.splits < 2) { p.splits = 1; p.kchunk = K; }
  }
}

// what both entry-point families check of a desc; they differ in the taps (the size of the LDS tap table) and strides they take
inline bool rect_desc_ok(const sgRectDesc* d, int max_kh, int max_kw, int max_taps, int max_stride) {
  if (!d) return false;
  if (d->N < 0 || d->C < 1 || d->H < 1 || d->W < 1 || d->Cout < 1 || d->KH < 1 || d->KW < 1) return false;
  if (d->KH > max_kh || d->KW > max_kw || d->KH * d->KW > max_taps || d->stride < 1 || d->stride > max_stride) return false;
  if (d->padH < 0 || d->padW < 0 || d->padH >= d->KH || d->padW >= d->KW) return false;
  if (d->H + 2 * d->padH < d->KH || d->W + 2 * d->padW < d->KW) return false;
  if (d->OH != (d->H + 2 * d->padH - d->KH) / d->stride + 1 || d->OW != (d->W + 2 * d->padW - d->KW) / d->stride + 1) return false;
  if (d->out_c0 < 0 || d->out_ctot < d->out_c0 + d->Cout) return false;
  const double in = (double)d->N * d->C * d->H * d->W, out = (double)d->N * d->out_ctot * d->OH * d->OW;
  const double k = (double)d->C * d->KH * d->KW;
  return in < SG_MAX_ELEMS && out < 2147483647.0 && k * d->Cout < SG_MAX_ELEMS && k < 16777216.0;
}

template <class CFG, int BM, int BN, int MAXTAPS>
int rect_launch(const float* w, int K, int M, bool vec, const LoadGatherRect<BN, MAXTAPS>& bl, const EpNCHW& ep, int Npix, int splits,
                hipStream_t s) {
  if (vec) return launch_cfg<CFG>(LoadKContig<BM, true>{w, K, M}, bl, ep, M, Npix, K, splits, s);
  return launch_cfg<CFG>(LoadKContig<BM, false>{w, K, M}, bl, ep, M, Npix, K, splits, s);
}

// ---- the host side both families share: a unit keeps its limits, its tile choice (a RectPlan from the desc) and its tile dispatch ---
struct RectDims {
  int M, K; long Npix;
  explicit RectDims(const sgRectDesc* d) : M(d->Cout), K(d->C * d->KH * d->KW), Npix((long)d->N * d->OH * d->OW) {}
};

inline void rect_plan_copy(const RectPlan& p, sgRectPlan* plan) {
  plan->tile = p.tile; plan->bm = p.bm; plan->bn = p.bn; plan->vec = p.vec; plan->splits = p.splits; plan->kchunk = p.kchunk;
}

// the slabs of a split plan
inline size_t rect_ws_bytes(const RectPlan& p, const sgRectDesc* d) {
  const RectDims n(d);
  return p.splits > 1 ? (size_t)p.splits * n.M * n.Npix * sizeof(float) : 0;
}

// sg_<stem>_fwd behind the unit's desc check: the remaining argument checks, the k-split table, the gather and the epilogue, the GEMM
// through launch(g, ktab, ep, M, K, Npix) -- the unit's rect_launch dispatch on pl.tile -- under profile kind ``kind``, then the slab reduction.
template <class Launch>
int rect_fwd(const char* stem, int kind, const RectPlan& pl, const sgRectDesc* d, const float* x, const float* w, const float* bias,
             float* y, int act, void* ws, size_t ws_bytes, hipStream_t s, Launch launch) {
  SG_ARG_CHECK(act == SG_ACT_NONE || act == SG_ACT_RELU, "%s_fwd: act must be SG_ACT_NONE or SG_ACT_RELU", stem);
  if (d->N == 0) return 0;
  SG_ARG_CHECK(x && w && y, "%s_fwd: null operand", stem);
  const RectDims n(d);
  const int M = n.M, K = n.K, PHW = d->OH * d->OW, Npix = (int)n.Npix;
  const size_t nout = (size_t)M * Npix;
  SG_ARG_CHECK(pl.splits == 1 || (ws && ws_bytes >= rect_ws_bytes(pl, d)), "%s_fwd: workspace of %zu bytes, %s_ws_bytes asks for %zu",
               stem, ws_bytes, stem, rect_ws_bytes(pl, d));
  const int KS2 = d->KH * d->KW, Kpad = sg_cdiv(K, 64) * 64 + 128;      // the k-loop prefetches entries up to two tiles past the end
  const unsigned shw = (unsigned)(d->H * d->W);
  // the k-split table (and cache key) of the square and rectangular gathers: it depends on (K, taps per channel, C, plane size) only
  const KEntry* ktab = reinterpret_cast<const KEntry*>(cached_table(
      TabKey{0, K, Kpad, KS2, d->C, 0, shw, 0, 0, 0, 0, 0}, (size_t)Kpad * sizeof(KEntry), s, [&](void* dst) {
        hipLaunchKernelGGL(build_ktab_kernel, dim3(sg_cdiv(Kpad, 256)), dim3(256), 0, s, reinterpret_cast<KEntry*>(dst), K, Kpad, KS2,
                           d->C, 0, shw, 0, 0, 0u);
      }));
  SG_ARG_CHECK(ktab != nullptr, "%s_fwd: device allocation of the k-split table failed", stem);
  const Gather g = make_gather(x, nullptr, d->C, 0, d->H, d->W, 1, d->OH, d->OW, d->stride, 0, 0);
  float* slabs = reinterpret_cast<float*>(ws);
  EpNCHW ep{y + (size_t)d->out_c0 * PHW, bias, PHW, d->out_ctot, M, Npix, act, 0.f, 0, 0, 1, 0, 0, 0, 0};
  if (pl.splits > 1) ep = EpNCHW{slabs, nullptr, PHW, M, M, Npix, SG_ACT_NONE, 0.f, nout, 0, 1, 0, 0, 0, 0};
  const double flops = 2.0 * M * (double)K * Npix;
  sgk::t_alg_bytes = 4.0 * ((double)d->N * d->C * shw + (double)M * K + (double)nout);
  {
    SgProfScope prof(kind, s, flops, sgk::t_alg_bytes);
    launch(g, ktab, ep, M, K, Npix);
  }
  SG_LAUNCH_CHECK((std::string(stem) + "_fwd").c_str());
  if (pl.splits > 1) {
    SgProfScope prof(SG_K_RECT_REDUCE, s, 0.0, 4.0 * (double)nout * (pl.splits + 1));
    hipLaunchKernelGGL(rect_reduce_kernel, dim3(sg_cdiv(nout, RECT_TPB)), dim3(RECT_TPB), 0, s, (const float*)slabs, y, (unsigned)nout,
                       pl.splits, bias, PHW, M, d->out_c0, d->out_ctot, act, FastDiv((unsigned)PHW), FastDiv((unsigned)M));
    SG_LAUNCH_CHECK((std::string(stem) + "_fwd (slab reduction)").c_str());
  }
  return 0;
}

}  // namespace
