// weight-gradient GEMMs: K = (image, pixel), N = (channel, tap) (see igemm_core.h / igemm.hip)
#include "igemm_core.h"

namespace {
// ---- wgrad-shaped GEMM: K = (img, pix), N = (c, taps) --------------------------------------------
// inverse of the per-image channel lists: inv[b][c] = position of c in list[b] or -1
__global__ void sparse_inv_kernel(const int* list, const int* cnt, int L, int C, int* inv) {
  const int b = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  int pos = -1;
  const int n = cnt[b];
  for (int j = 0; j < n; ++j) pos = list[b * L + j] == c ? j : pos;
  inv[b * C + c] = pos;
}
// gw[m][c][t] = sum_b slab[b][m][t][inv[b][c]]  (images in ascending order => deterministic)
__global__ void sparse_wgrad_reduce_kernel(const float* slabs, const int* inv, float* gw, int M, int C, int KS2, int cpad,
                                           int NB) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)M * C * KS2) return;
  const int t = (int)(i % KS2);
  const int c = (int)((i / KS2) % C);
  const int m = (int)(i / ((size_t)KS2 * C));
  float v = 0.f;
  for (int b = 0; b < NB; ++b) {
    const int j = inv[b * C + c];
    if (j >= 0) v += slabs[(((size_t)b * M + m) * KS2 + t) * cpad + j];
  }
  gw[i] = v;
}
// out[b][i] = sum_q ws[(b*S + q)][i]: k-chunks of one image (fixed order)
__global__ void slab_group_reduce_kernel(const float* ws, float* out, size_t n, int S, int NB) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * NB) return;
  const size_t b = i / n, r = i - b * n;
  float v = 0.f;
  for (int q = 0; q < S; ++q) v += ws[(b * S + q) * n + r];
  out[i] = v;
}
// gwimg[b][m][j][t] = slab[b][m][t][j] (per-image weight gradients of a factored layout conv; zero beyond the image's list)
__global__ void sparse_wgrad_perimage_kernel(const float* slabs, const int* cnt, float* gwimg, int M, int L, int KS2, int cpad,
                                             int NB) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)NB * M * L * KS2) return;
  const int t = (int)(i % KS2);
  const int j = (int)((i / KS2) % L);
  const size_t bm = i / ((size_t)KS2 * L);
  const int b = (int)(bm / M);
  gwimg[i] = j < cnt[b] ? slabs[(bm * KS2 + t) * cpad + j] : 0.f;
}
// gw[m][c][t] = sum_z slab[z][m][t][c]: un-permutes the tap-major slabs of the weight-gradient GEMM (the GEMM epilogue
// writes them coalesced; scattering 4-byte stores at stride KS2*4 from there cost 8x write amplification in HBM)
__global__ void wgrad_unpermute_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ gw, int M, int C, int KS2,
                                              int cpad, int S, const float* __restrict__ rowsum, float* __restrict__ gb) {
  // grid (ceil(C*KS2 / 256), M): one 32-bit division per thread.  (An LDS-transposed variant with fully coalesced slab reads
  // was measured SLOWER -- 21.7 vs 15.7 us per launch: the strided reads hit in L2, the extra barrier and the thinner loops
  // do not pay.)
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = blockIdx.y;
  if (gb && j == 0) {                     // bias gradient: the k-chunks' row sums of gy (LoadPixK*::rowsum), fixed order
    const float b = sg_sum_strided(rowsum + m, (size_t)M, S);
    gb[m] = b;
  }
  if (j >= (unsigned)(C * KS2)) return;
  const unsigned c = j / (unsigned)KS2, t = j - c * (unsigned)KS2;
  const size_t zs = (size_t)M * KS2 * cpad;
  const float* p = slabs + ((size_t)m * KS2 + t) * cpad + c;
  // eight slab loads in flight per thread, added in slab order (sg_sum_strided; the plain loop compiled to one dependent load /
  // wait / add per slab: 95 % of the wave cycles parked in s_waitcnt on 8..64 L2 round trips, profiles/r06_pmc_classes_cycles.md)
  const float v = sg_sum_strided(p, zs, S);
  gw[(size_t)m * C * KS2 + j] = v;
}
// pp[b][j][PHp][PWp] = ReflectionPad2d(pad) of plane list[b][j] of image b, j < cnt[b] (planes beyond the list are never read:
// LoadPaddedNK masks their columns).  grid (ceil(PHp PWp / 256), L, N): one 32-bit multiply-high per element, coalesced stores.
__global__ void reflect_pad_planes_kernel(const float* __restrict__ x, const int* __restrict__ list, const int* __restrict__ cnt,
                                          float* __restrict__ pp, int C, int L, int H, int W, int pad, int PWp, int PP,
                                          FastDiv dPWp) {
  const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y, b = blockIdx.z;
  if (e >= (unsigned)PP || j >= cnt[b]) return;
  const unsigned oh = dPWp.div(e), ow = e - oh * (unsigned)PWp;
  int ih = (int)oh - pad, iw = (int)ow - pad;
  ih = ih < 0 ? -ih : (ih >= H ? 2 * H - 2 - ih : ih);
  iw = iw < 0 ? -iw : (iw >= W ? 2 * W - 2 - iw : iw);
  const int c = list[b * L + j];
  pp[((size_t)b * L + j) * PP + e] = x[((size_t)b * C + c) * ((size_t)H * W) + (unsigned)(ih * W + iw)];
}
// the per-image weight gradient of the factored 7x7 stem over padded planes: launch_nk_general's three forms with LoadPaddedNK
void launch_nk_padded(int tile, bool vecA, const float* A, int M, int Mtot, int PQ, const Gather& g, int Ncols, const EpRowMajor& ep,
                      int Kpix, hipStream_t s, const Sparse& sp, const float* pp, const LaunchMods& lm) {
  float* const rowsum = nullptr;
  const FastDiv dPQ((unsigned)PQ), dPW((unsigned)g.PW);
  const int PWp = g.SW + 2 * g.pad, PP = (g.SH + 2 * g.pad) * PWp;
  const unsigned bytes = (unsigned)((size_t)(Kpix / PQ) * sp.L * PP * sizeof(float));
#define SG_PAD_B(BNv) LoadPaddedNK<BNv, 7, NSW>{pp, bytes, PQ, g.PW, PWp, PP, sp.L, sp.cnt, dPQ, dPW}
  if (tile == 2)
    launch_cfg<CfgW32>(LoadPixK<32>{A, M, Mtot, PQ, dPQ, rowsum}, SG_PAD_B(128), ep, M, Ncols, Kpix, 1, s, lm);
  else if (vecA)
    launch_cfg<CfgW64>(LoadPixKVec<64>{A, M, Mtot, PQ, dPQ, rowsum}, SG_PAD_B(64), ep, M, Ncols, Kpix, 1, s, lm);
  else
    launch_cfg<CfgW64>(LoadPixK<64>{A, M, Mtot, PQ, dPQ, rowsum}, SG_PAD_B(64), ep, M, Ncols, Kpix, 1, s, lm);
#undef SG_PAD_B
}
// general (c, tap)-ordered loader: only for few-channel inputs (RGB crops / images)
template <int KS>
void launch_nk_general(int tile, bool vecA, const float* A, int M, int Mtot, int PQ, const Gather& g, int Ncols, const EpRowMajor& ep,
                       int Kpix, int splits, hipStream_t s, const LaunchMods& lm, const Sparse* sp = nullptr, int zdiv = 1) {
  float* const rowsum = nullptr;
  const FastDiv dPQ((unsigned)PQ);
  const int* sl = sp ? sp->list : nullptr; const int* sc = sp ? sp->cnt : nullptr; const int L = sp ? sp->L : 0;
  if (tile == 2)
    launch_cfg<CfgW32>(LoadPixK<32>{A, M, Mtot, PQ, dPQ, rowsum}, LoadGatherNK<128, KS, false, true, NSW>{g, Ncols, sl, sc, L, zdiv}, ep,
                       M, Ncols, Kpix, splits, s, lm);
  else if (KS == 7 && vecA)
    // (nk_launch_plan: vecA only with KS == 7, per-image lists, PQ % 4 == 0, A 16-byte aligned)
    // the per-image weight gradient of the factored 7x7 stem (64 x 9*49 x 16 384 per image: the slowest GEMM launch of the step,
    // 45 TFLOP/s): the output gradient is read with 16-byte loads -- one vector-memory instruction per thread and k-tile instead of
    // four next to the four gathered elements of B (same-box A/B, two pairs: 31.24 vs 31.31 ms/step, +0.2 %)
    launch_cfg<CfgW64>(LoadPixKVec<64>{A, M, Mtot, PQ, dPQ, rowsum}, LoadGatherNK<64, KS, false, true, NSW>{g, Ncols, sl, sc, L, zdiv}, ep,
                       M, Ncols, Kpix, splits, s, lm);
  else
    launch_cfg<CfgW64>(LoadPixK<64>{A, M, Mtot, PQ, dPQ, rowsum}, LoadGatherNK<64, KS, false, true, NSW>{g, Ncols, sl, sc, L, zdiv}, ep,
                       M, Ncols, Kpix, splits, s, lm);
}

template <class CFG, int BMv, int BNv>
void launch_nk_tap(const float* A, int M, int Mtot, int PQ, bool vecA, const Gather& g, int KS, int Ccols, int cpad,
                   const Sparse* sp, bool nomask, const EpWgrad& ep, int Kpix, int splits, hipStream_t s, float* rowsum,
                   const LaunchMods& lm) {
  const FastDiv dPQ((unsigned)PQ), dPW((unsigned)g.PW);
  const int* sl = sp ? sp->list : nullptr; const int* sc = sp ? sp->cnt : nullptr; const int L = sp ? sp->L : 0;
  const int Nv = KS * KS * cpad;
  const bool two = g.C2 > 0;
#define SG_TAP_B(TWOv, MASKv) LoadTapNK<BNv, TWOv, MASKv, CFG::NSUB>{g, KS, Ccols, cpad, sl, sc, L, dPQ, dPW}
  if (vecA) {
    const LoadPixKVec<BMv> al{A, M, Mtot, PQ, dPQ, rowsum};
    if (two) launch_cfg<CFG>(al, SG_TAP_B(true, true), ep, M, Nv, Kpix, splits, s, lm);
    else if (nomask) launch_cfg<CFG>(al, SG_TAP_B(false, false), ep, M, Nv, Kpix, splits, s, lm);
    else launch_cfg<CFG>(al, SG_TAP_B(false, true), ep, M, Nv, Kpix, splits, s, lm);
  } else {
    const LoadPixK<BMv> al{A, M, Mtot, PQ, dPQ, rowsum};
    if (two) launch_cfg<CFG>(al, SG_TAP_B(true, true), ep, M, Nv, Kpix, splits, s, lm);
    else if (nomask) launch_cfg<CFG>(al, SG_TAP_B(false, false), ep, M, Nv, Kpix, splits, s, lm);
    else launch_cfg<CFG>(al, SG_TAP_B(false, true), ep, M, Nv, Kpix, splits, s, lm);
  }
#undef SG_TAP_B
}

int run_nk_ks(int KS, const float* A, int M, int Mtot, const Gather& g, int NB, float* out, void* ws, size_t ws_bytes,
              double flops, hipStream_t s, const Sparse* sp, float* gb, bool* gb_done) {
  if (gb_done) *gb_done = false;
  const int PQ = g.PH * g.PW, KS2 = KS * KS;
  const int Kpix = NB * PQ;
  const int C = g.C1 + g.C2;
  // channel-sparse input (see run_kn_sparse): one k-chunk per image, compact columns, per-image slabs that
  // sparse_wgrad_reduce_kernel scatters back to the dense gradient in a fixed order
  const int Ccols = sp ? sp->L : C;
  const int Ncols = Ccols * KS2;
  // every decision below is nk_launch_plan's (igemm_core.h), which sg_conv2d_wgrad_plan reports
  const NkLaunch nl = nk_launch_plan(nk_shape(KS, M, Mtot, g, NB), sp != nullptr, sp ? sp->L : 0, sp && sp->gwimg, aligned16(A), gb != nullptr,
                                     ws ? ws_bytes : 0, sp ? sp->pad_off : 0);
  SG_ARG_CHECK(nl.err == nullptr, "%s", nl.err);
  const sgWgradPlan& pl = nl.p;
  const bool vecA = pl.a_vec != 0;
  if (nl.few) {
    // a handful of channels per image (factored layout convs): the (channel, tap)-ordered gather, L*KS2 columns, k-chunks inside
    // each image for occupancy
    const int tile = nl.tile, S = nl.S;
    const size_t mnc = nl.mn;
    float* dstp = S > 1 ? reinterpret_cast<float*>(ws) : sp->gwimg;
    const EpRowMajor ep{dstp, nullptr, M, Ncols, Ncols, SG_ACT_NONE, 0.f, mnc};
    if (pl.form == SG_WG_PADDED) {                   // the listed planes reflect-padded once, behind the slabs (nk_launch_plan)
      float* pp = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + sp->pad_off);
      const int PWp = g.SW + 2 * g.pad, PP = (g.SH + 2 * g.pad) * PWp;
      hipLaunchKernelGGL(reflect_pad_planes_kernel, dim3(sg_cdiv(PP, 256), Ccols, NB), dim3(256), 0, s, g.src1, sp->list, sp->cnt, pp,
                         g.C1, Ccols, g.SH, g.SW, g.pad, PWp, PP, FastDiv((unsigned)PWp));
      SgProfScope prof(sg_igemm_kind(2, KS, tile), s, 2.0 * M * (double)Ncols * Kpix, 0);
      launch_nk_padded(tile, vecA, A, M, Mtot, PQ, g, Ncols, ep, Kpix, s, *sp, pp, nl.mods);
    } else {
      SgProfScope prof(sg_igemm_kind(2, KS, tile), s, 2.0 * M * (double)Ncols * Kpix, 0);
      switch (KS) {
        case 1: launch_nk_general<1>(tile, vecA, A, M, Mtot, PQ, g, Ncols, ep, Kpix, 1, s, nl.mods, sp, S); break;
        case 3: launch_nk_general<3>(tile, vecA, A, M, Mtot, PQ, g, Ncols, ep, Kpix, 1, s, nl.mods, sp, S); break;
        case 4: launch_nk_general<4>(tile, vecA, A, M, Mtot, PQ, g, Ncols, ep, Kpix, 1, s, nl.mods, sp, S); break;
        case 7: launch_nk_general<7>(tile, vecA, A, M, Mtot, PQ, g, Ncols, ep, Kpix, 1, s, nl.mods, sp, S); break;
      }
    }
    if (pl.reduce == SG_WR_GROUP)
      hipLaunchKernelGGL(slab_group_reduce_kernel, dim3(sg_cdiv(mnc * NB, 256)), dim3(256), 0, s, (const float*)ws, sp->gwimg,
                         mnc, S, NB);
    return 0;
  }
  const bool tap = pl.form == SG_WG_TAP;
  const int splits = nl.splits;
  const size_t mn = nl.mn;
  float* const rowsum = pl.rowsum_fused ? reinterpret_cast<float*>(ws) + nl.rowsum_off : nullptr;
  if (sp) flops = 2.0 * M * (double)Ncols * Kpix;
  float* dst = (splits > 1 || sp || tap) ? reinterpret_cast<float*>(ws) : out;
  {
    SgProfScope prof(sg_igemm_kind(2, KS, nl.tile), s, flops, 0);
    if (tap) {
      const EpWgrad ep{dst, M, pl.cpad, KS2, mn};
      // (nomask is passed as planned for one source; launch_nk_tap ignores it for two)
      const bool nomask = pl.nomask != 0;
      switch (nl.tile) {
        case 0: launch_nk_tap<CfgW128, 128, 128>(A, M, Mtot, PQ, vecA, g, KS, Ccols, pl.cpad, sp, nomask, ep, Kpix, splits, s, rowsum, nl.mods); break;
        case 1: launch_nk_tap<CfgW64, 64, 64>(A, M, Mtot, PQ, vecA, g, KS, Ccols, pl.cpad, sp, nomask, ep, Kpix, splits, s, rowsum, nl.mods); break;
        default: launch_nk_tap<CfgW32, 32, 128>(A, M, Mtot, PQ, vecA, g, KS, Ccols, pl.cpad, sp, nomask, ep, Kpix, splits, s, rowsum, nl.mods); break;
      }
    } else {
      const EpRowMajor ep{dst, nullptr, M, Ncols, Ncols, SG_ACT_NONE, 0.f, mn};
      switch (KS) {
        case 1: launch_nk_general<1>(nl.tile, vecA, A, M, Mtot, PQ, g, Ncols, ep, Kpix, splits, s, nl.mods); break;
        case 3: launch_nk_general<3>(nl.tile, vecA, A, M, Mtot, PQ, g, Ncols, ep, Kpix, splits, s, nl.mods); break;
        case 4: launch_nk_general<4>(nl.tile, vecA, A, M, Mtot, PQ, g, Ncols, ep, Kpix, splits, s, nl.mods); break;
        case 7: launch_nk_general<7>(nl.tile, vecA, A, M, Mtot, PQ, g, Ncols, ep, Kpix, splits, s, nl.mods); break;
      }
    }
  }
  const size_t nout = (size_t)M * C * KS2;
  switch (pl.reduce) {
    case SG_WR_PERIMAGE: {
      const size_t n = (size_t)NB * M * sp->L * KS2;
      hipLaunchKernelGGL(sparse_wgrad_perimage_kernel, dim3(sg_cdiv(n, 256)), dim3(256), 0, s, (const float*)ws, sp->cnt,
                         sp->gwimg, M, sp->L, KS2, pl.cpad, NB);
      break;
    }
    case SG_WR_SPARSE: {
      int* inv = reinterpret_cast<int*>(reinterpret_cast<float*>(ws) + (size_t)NB * mn);
      hipLaunchKernelGGL(sparse_inv_kernel, dim3(sg_cdiv(C, 256), NB), dim3(256), 0, s, sp->list, sp->cnt, sp->L, C, inv);
      hipLaunchKernelGGL(sparse_wgrad_reduce_kernel, dim3(sg_cdiv(nout, 256)), dim3(256), 0, s, (const float*)ws,
                         (const int*)inv, out, M, C, KS2, pl.cpad, NB);
      break;
    }
    case SG_WR_UNPERMUTE:
      hipLaunchKernelGGL(wgrad_unpermute_reduce_kernel, dim3(sg_cdiv((size_t)C * KS2, 256), M), dim3(256), 0, s, (const float*)ws, out,
                         M, C, KS2, pl.cpad, splits, (const float*)rowsum, rowsum ? gb : nullptr);
      if (rowsum && gb_done) *gb_done = true;
      break;
    case SG_WR_WIDE:
      hipLaunchKernelGGL(slab_reduce_wide_kernel, dim3(sg_cdiv(mn, 16)), dim3(256), 0, s, (const float*)ws, out, mn, splits);
      break;
    case SG_WR_SLAB:
      hipLaunchKernelGGL(slab_reduce_kernel, dim3(sg_cdiv(mn, 256)), dim3(256), 0, s, (const float*)ws, out, mn, splits);
      break;
    default: break;
  }
  return 0;
}


}  // namespace

int sgk::nk_run(int KS, const float* A, int M, int Mtot, const Gather& g, int NB, float* out, void* ws, size_t ws_bytes,
                double flops, hipStream_t s, const Sparse* sp, float* gb, bool* gb_done) {
  return run_nk_ks(KS, A, M, Mtot, g, NB, out, ws, ws_bytes, flops, s, sp, gb, gb_done);
}

#ifdef SG_TIMELINE
// debugging build only (tools/probe/build_timeline.sh): hand this translation unit's igemm_kernel instantiations a stamp buffer of
// ``cap`` workgroups x 8 x u64 (nullptr: off)
extern "C" int sg_debug_timeline_set_igemm_nk(void* buf, unsigned cap) {
  unsigned long long* p = reinterpret_cast<unsigned long long*>(buf);
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_sg_tl), &p, sizeof(p)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_sg_tl_cap), &cap, sizeof(cap)) != hipSuccess) return -1;
  return 0;
}
#endif
