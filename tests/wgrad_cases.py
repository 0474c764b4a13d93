"""Case table, input builders, float64 references and rounding bounds of the weight-gradient GEMM tests: run_nk_ks of
csrc/igemm_nk.hip, planned by nk_launch_plan of csrc/igemm_core.h, behind sg_conv2d_wgrad, sg_conv2d_wgrad_sparse,
sg_conv2d_wgrad_perimage and sg_convT2d_wgrad.  Shared by tests/test_wgrad_cases_cpu.py (the references agree with autograd, every
row has the plan it claims, the table reaches every plan value, the Python restatement of the plan equals the query) and
tests/test_gpu_wgrad.py (every row against float64 on the device).

NumPy only.  The references restate the operation tap by tap from its index formula (dtype-generic: the one-hot probes run them in
float32, where a single product is exact):
    gw[m,c,kh,kw] = sum_{n,oh,ow} gy[n,m,oh,ow] * X[n,c,oh*s-p+kh, ow*s-p+kw],     gb[m] = sum_{n,oh,ow} gy[n,m,oh,ow]
X the logical input grid: the stored planes nearest-upsampled x2 (optional), zero- or reflection-padded; channels >= C1 come from a
second source, optionally a per-sample row [N, C2] broadcast over the plane.  The sparse form sums, for every channel, the images
whose list names it (list[b][:cnt[b]]); the per-image form keeps the images apart, [N][M][L][KS][KS] in list order, zero beyond
cnt[b].

The launch plans come from the library's host-side query (include/sg2im_hip.h: sg_conv2d_wgrad_plan), the function the launcher
runs from; py_plan() restates it and is compared with it over a grid of shapes.

Bounds.  Every output is an fp32 fma chain over its n structurally non-zero terms per k-chunk (a tap outside the plane, a padding
row of a k-tile, an empty chunk add 0 exactly), the chunks joined by at most c further adds:
    |got - ref64| <= gamma(n + c) sum|a||b|,      n = the restatement run on ones, sum|a||b| = the restatement run on absolute values.
c from the code (igemm_nk.hip), for the plan the query reports for THAT launch:
  dense forms       c = grid_z: slab_reduce / slab_reduce_wide / wgrad_unpermute_reduce add the grid_z slabs of one element
  sparse scatter    c = N: sparse_wgrad_reduce_kernel adds one slab per image that lists the channel
  per-image forms   c = S = grid_z / N chunks of an image meet in slab_group_reduce_kernel (the per-image copy adds nothing: c = 1)
  bias gradient     gamma(N*OH*OW) sum|gy|: a sum of N*OH*OW terms, in whatever order (row sums per chunk, or sg_channel_sum)
"""
import ctypes

import numpy as np

from scene_generation_amd._hip import CONST, plan_dict, sgWgradPlan

from dense_pointwise_cases import gamma, rng_of, f32, option  # noqa: F401  (re-exported)
from transposed_conv_cases import make_desc, conv_out_size, bound  # noqa: F401

# ---- kernel constants the plan is built around (tests/test_wgrad_cases_cpu.py reads them back from the sources)
BK = 16                 # igemm_core.h: sub-tile depth (= the k-tile depth of the weight-gradient tiles, NSW = 1)
KBLK = 256              # pixels decoded per LDS table block (LoadTapNK / LoadPixKVec / LoadPaddedNK)
CHUNK_ROUND = 64        # nk_launch_plan: split chunks are rounded to 64 pixels before the split count is fixed
CAP_TAP, CAP_GATHER = 64, 256       # nk_plan: most k-chunks of a tap-major / (channel, tap) launch
TARGET_128, TARGET = 768, 1024      # nk_plan: workgroups aimed at with 128x128 tiles / otherwise
FEW_TARGET, FEW_COLS, FEW_PIX = 1024, 128, 256     # nk_launch_plan, few-channel per-image form: S <= 128 / L, S <= PQ / 256
PAD_MAX_BYTES = 1 << 30

# include/sg2im_hip.h, under the short names the tables use
WG_CONV, WG_SPARSE, WG_PERIMAGE, WG_CONVT = (CONST['SG_WG_' + n] for n in ('CONV', 'SPARSE', 'PERIMAGE', 'CONVT'))
WG_TAP, WG_GATHER, WG_PADDED = (CONST['SG_WG_' + n] for n in ('TAP', 'GATHER', 'PADDED'))
WR_NONE, WR_SLAB, WR_WIDE, WR_UNPERMUTE, WR_SPARSE, WR_PERIMAGE, WR_GROUP = (
    CONST['SG_WR_' + n] for n in ('NONE', 'SLAB', 'WIDE', 'UNPERMUTE', 'SPARSE', 'PERIMAGE', 'GROUP'))
ENTRY_OF = {'dense': WG_CONV, 'sparse': WG_SPARSE, 'perimage': WG_PERIMAGE}
PLAN_FIELDS = tuple(n for n, t in sgWgradPlan._fields_ if t is ctypes.c_int32)      # the int32 fields, ``reserved`` among them
OPTIONS = ('wgrad_xcd', 'wgrad_rowsum', 'wgrad_padded')
AMPLE = 4 << 20         # bytes: more workspace than any row's plan needs


def wgrad_plan(lib, desc, entry, L=0, a_mod16=0, ws_bytes=AMPLE):
    """sg_conv2d_wgrad_plan under the current options -> dict, or None when the query returns non-zero"""
    p = sgWgradPlan()
    rc = lib.sg_conv2d_wgrad_plan(ctypes.byref(desc), int(entry), int(L), int(a_mod16), int(ws_bytes), ctypes.byref(p))
    return None if rc else plan_dict(p)


# =============================================================================================
# the plan, restated (nk_plan + nk_launch_plan of csrc/igemm_core.h)
# =============================================================================================
def _cdiv(a, b):
    return -(-a // b)


def sparse_base_ws(N, M, C, L, KS):
    """what the sparse / per-image entry points require: slabs padded to 128 channels + the inverse lists, or sg_channel_sum's bytes"""
    return max(N * M * _cdiv(L, 128) * 128 * KS * KS * 4 + N * C * 4, M * 64 * 4)


def padded_bytes(KS, N, L, C2, H, W, ups, OH, OW, stride, pad, reflect):
    if not (KS == 7 and reflect and C2 == 0 and ups == 1 and stride == 1 and 1 <= pad < min(H, W) and N > 0 and L > 0):
        return 0
    if OH != H + 2 * pad - KS + 1 or OW != W + 2 * pad - KS + 1 or OH < 1 or OW < 1:
        return 0
    b = N * L * (H + 2 * pad) * (W + 2 * pad) * 4
    return b if b <= PAD_MAX_BYTES else 0


def py_plan(entry, N, C1, C2, H, W, M, KS, stride, pad, reflect, ups, OH, OW, L=0, a_mod16=0, ws_bytes=AMPLE, xcd=1, rowsum=1,
            padded=1):
    """-> the dict wgrad_plan() returns, or None where the query refuses.  M = Cout; for WG_CONVT the caller passes the swapped GEMM
    (M = C1 of the desc, C1 = its Cout, H x W = its output grid, OH x OW = its input grid)"""
    PQ, KS2, C = OH * OW, KS * KS, C1 + C2
    Kpix = N * PQ
    sparse, perimage = entry in (WG_SPARSE, WG_PERIMAGE), entry == WG_PERIMAGE
    pad_off = 0
    if sparse:
        if not 0 < L <= C:
            return None
        base = sparse_base_ws(N, M, C, L, KS)
        if ws_bytes < base:
            return None
        pb = padded_bytes(KS, N, L, C2, H, W, ups, OH, OW, stride, pad, reflect)
        off = _cdiv(base, 256) * 256
        if perimage and pb and ws_bytes >= off + pb:
            pad_off = off
    Ccols = L if sparse else C
    Ncols = Ccols * KS2
    vec_ok = PQ % 4 == 0 and a_mod16 == 0
    # nk_plan
    tap = Ccols >= 48 or C2 > 0
    tile = 2 if M <= 32 else 1
    if M > 64 and tap and _cdiv(M, 128) * 128 * _cdiv(Ccols, 128) * 128 * 0.7 < _cdiv(M, 64) * 64 * _cdiv(Ccols, 64) * 64:
        tile = 0
    bm, bn = {0: (128, 128), 1: (64, 64), 2: (32, 128)}[tile]
    cpad = _cdiv(Ccols, bn) * bn if tap else 0
    tiles = _cdiv(M, bm) * (KS2 * (cpad // bn) if tap else _cdiv(Ccols * KS2, bn))
    s = _cdiv(TARGET_128 if tile == 0 else TARGET, tiles)
    maxs = max(Kpix // (BK * 8), 1)
    s = min(s, maxs, CAP_TAP if tap else CAP_GATHER)
    if xcd and s >= 6:
        s8 = _cdiv(s, 8) * 8
        if s8 > maxs:
            s8 = maxs // 8 * 8
        if s8 >= 8:
            s = s8
    s = max(s, 1)
    if sparse and perimage and C2 == 0 and _cdiv(Ccols, 64) * 64 >= 3 * Ccols:
        tile = 2 if M <= 32 else 1
        bm, bn = (32, 128) if tile == 2 else (64, 64)
        tiles = _cdiv(M, bm) * _cdiv(Ncols, bn) * N
        S = max(min(_cdiv(FEW_TARGET, tiles), FEW_COLS // Ccols, PQ // FEW_PIX), 1)
        kcs = _cdiv(_cdiv(PQ, S), BK) * BK
        S = _cdiv(PQ, kcs)
        slabs = M * Ncols * 4 * S * N
        if ws_bytes < slabs:
            return None
        pb = padded_bytes(KS, N, Ccols, C2, H, W, ups, OH, OW, stride, pad, reflect)
        pd = bool(padded and pb and pad_off >= slabs and N <= 65535 and ws_bytes >= pad_off + pb)
        z = N * S
        return dict(form=WG_PADDED if pd else WG_GATHER, bm=bm, bn=bn, cpad=0, a_vec=int(tile != 2 and KS == 7 and vec_ok), two=0,
                    nomask=0, kchunk=kcs, chunks=z, grid_z=z, xcd=2 if (xcd and z >= 8 and z % 8 == 0) else 0,
                    reduce=WR_GROUP if S > 1 else WR_NONE, rowsum_fused=0, ws_needed=pad_off + pb if pd else (slabs if S > 1 else 0))
    if sparse:
        tap = True
        if cpad == 0:
            cpad = _cdiv(Ccols, bn) * bn
    splits = N if sparse else s
    mn = M * KS2 * cpad if tap else M * Ncols
    if not sparse and splits > 1 and ws_bytes < mn * 4 * splits:
        splits = ws_bytes // (mn * 4)
    if not sparse and splits < 2:
        splits = 1
    if tap and ws_bytes < mn * 4 * splits:
        return None
    kchunk = PQ if sparse else _cdiv(_cdiv(Kpix, splits), CHUNK_ROUND) * CHUNK_ROUND
    splits = _cdiv(Kpix, kchunk)
    zpad = 0
    if xcd and not sparse and splits >= 6:
        z8 = _cdiv(splits, 8) * 8
        if ws_bytes >= (mn + M) * 4 * z8:
            zpad = splits = z8
    fused = int(bool(rowsum and entry == WG_CONV and tap and ws_bytes >= (mn + M) * 4 * splits))
    if sparse:
        kc, chunks = PQ, N
    else:
        kc = _cdiv(_cdiv(Kpix, splits), BK) * BK if splits > 1 else Kpix
        chunks = _cdiv(Kpix, kc) if splits > 1 else 1
    grid_z = max(chunks, zpad)
    two = int(tap and C2 > 0)
    nomask = int(bool(tap and not two and reflect and Kpix % BK == 0 and (not sparse or PQ % BK == 0) and chunks == grid_z))
    if sparse:
        red, need = (WR_PERIMAGE if perimage else WR_SPARSE), N * mn * 4 + (0 if perimage else N * C * 4)
    elif tap:
        red, need = WR_UNPERMUTE, (mn + (M if fused else 0)) * 4 * splits
    else:
        red = WR_WIDE if splits >= 32 else (WR_SLAB if splits > 1 else WR_NONE)
        need = mn * 4 * splits if splits > 1 else 0
    return dict(form=WG_TAP if tap else WG_GATHER, bm=bm, bn=bn, cpad=cpad if tap else 0, a_vec=int(tap and vec_ok), two=two,
                nomask=nomask, kchunk=kc, chunks=chunks, grid_z=grid_z, xcd=int(zpad > 0 and grid_z >= 8 and grid_z % 8 == 0),
                reduce=red, rowsum_fused=fused, ws_needed=need)


# =============================================================================================
# float64 (dtype-generic) restatements, tap by tap
# =============================================================================================
def _reflect(i, n):
    i = -i if i < 0 else i
    return 2 * n - 2 - i if i >= n else i


def _axis(n_out, s, p, k, n_log, reflect, ups):
    """stored coordinate read by output position o at tap k, and whether there is one: l = o*s - p + k on the logical axis of n_log
    (mirrored into it under reflection padding, outside it = a zero under zero padding), stored coordinate l // ups"""
    idx, ok = [], []
    for o in range(n_out):
        l = o * s - p + k
        if reflect:
            l = _reflect(l, n_log)
        v = 0 <= l < n_log
        idx.append(l // ups if v else 0)
        ok.append(v)
    return np.array(idx), np.array(ok)


def sources(x1, x2, bcast):
    """the channel concat [N, C1 + C2, H, W]; x2 [N, C2] is a row per sample broadcast over the plane when bcast"""
    if x2 is None:
        return x1
    if bcast:
        x2 = np.broadcast_to(x2[:, :, None, None], x2.shape + x1.shape[2:])
    return np.concatenate([x1, x2.astype(x1.dtype)], axis=1)


def wgrad_images(gy, x, KS, s, p, reflect, ups):
    """g[n,m,c,kh,kw] = sum_{oh,ow} gy[n,m,oh,ow] X[n,c,oh*s-p+kh,ow*s-p+kw]: the weight gradient image by image"""
    N, M, OH, OW = gy.shape
    C, H, W = x.shape[1:]
    g = np.zeros((N, M, C, KS, KS), dtype=gy.dtype)
    for kh in range(KS):
        ih, vh = _axis(OH, s, p, kh, H * ups, reflect, ups)
        for kw in range(KS):
            iw, vw = _axis(OW, s, p, kw, W * ups, reflect, ups)
            xs = x[:, :, ih][:, :, :, iw] * (vh[:, None] & vw[None, :]).astype(x.dtype)
            g[:, :, :, kh, kw] = np.einsum('nmhw,nchw->nmc', gy, xs)
    return g


def conv_wgrad(gy, x, KS, s, p, reflect, ups):
    return wgrad_images(gy, x, KS, s, p, reflect, ups).sum(axis=0)


def sparse_wgrad(gimg, lists, cnt):
    """dense gradient [M, C, KS, KS] of a channel-sparse input: channel c takes the images that list it"""
    out = np.zeros(gimg.shape[1:], dtype=gimg.dtype)
    for b in range(gimg.shape[0]):
        ch = [int(c) for c in lists[b][:cnt[b]]]
        out[:, ch] += gimg[b][:, ch]
    return out


def perimage_wgrad(gimg, lists, cnt):
    """[N, M, L, KS, KS] in list order, zero beyond cnt[b]"""
    N, M = gimg.shape[:2]
    out = np.zeros((N, M, lists.shape[1]) + gimg.shape[3:], dtype=gimg.dtype)
    for b in range(N):
        out[b, :, :cnt[b]] = gimg[b][:, [int(c) for c in lists[b][:cnt[b]]]]
    return out


def bias_grad(gy):
    return gy.sum(axis=(0, 2, 3))


# =============================================================================================
# the case table
# =============================================================================================
def _case(name, kind, Cout, C1, KS, N, H, W, stride=1, pad=None, reflect=False, ups=1, C2=0, bcast=0, L=0, gb=True, opts=None,
          ws=AMPLE, a_off=0, claims=None, why=''):
    """kind: 'dense' (sg_conv2d_wgrad), 'sparse', 'perimage'.  H x W: the stored input plane.  opts: library options of the row
    (default otherwise); ws: bytes of workspace offered, or a function of the ample-workspace plan and the row; a_off: floats gy is
    offset from a 16-byte boundary; claims: the plan fields the row is there for"""
    pad = (KS - 1) // 2 if pad is None else pad
    OH, OW = conv_out_size(H * ups, KS, stride, pad), conv_out_size(W * ups, KS, stride, pad)
    return dict(name=name, kind=kind, Cout=Cout, C1=C1, C2=C2, KS=KS, N=N, H=H, W=W, stride=stride, pad=pad, reflect=reflect, ups=ups,
                bcast=bcast, L=L, gb=gb and kind != 'perimage', opts=dict(opts or {}), ws=ws, a_off=a_off, claims=dict(claims or {}),
                why=why, OH=OH, OW=OW, shape_key='%s|%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d' % (
                    kind, Cout, C1, C2, KS, N, H, W, stride, pad, int(reflect), ups, bcast, L, 0))


def _slabs(k, rowsum=False):
    """workspace for exactly k slabs of the row's plan (with or without room for their row sums)"""
    def fn(plan, case):
        mn = case['Cout'] * case['KS'] ** 2 * (plan['cpad'] if plan['form'] == WG_TAP else case['C1'] + case['C2'])
        return (mn + (case['Cout'] if rowsum else 0)) * 4 * (plan['grid_z'] if k is None else k)
    return fn


def _sparse_base(plan, case):
    return sparse_base_ws(case['N'], case['Cout'], case['C1'] + case['C2'], case['L'], case['KS'])


T64, T32, T128 = dict(bm=64, bn=64), dict(bm=32, bn=128), dict(bm=128, bn=128)
GATHER = dict(form=WG_GATHER, cpad=0, a_vec=0, two=0, nomask=0, rowsum_fused=0)
TAP = dict(form=WG_TAP, two=0)


def _c(*ds, **kw):
    out = {}
    for d in ds:
        out.update(d)
    out.update(kw)
    return out


CASES = [
    # ---- (channel, tap) gather: C < 48, one source ---------------------------------------------------------------------
    _case('g_40x3_k3_5x5', 'dense', 40, 3, 3, 1, 5, 5, claims=_c(GATHER, T64, chunks=1, grid_z=1, reduce=WR_NONE, xcd=0),
          why='64-tile, the GEMM stores the result itself; PQ = 25: k tail inside one 16-row tile'),
    _case('g_8x3_k3_5x5', 'dense', 8, 3, 3, 1, 5, 5, claims=_c(GATHER, T32, chunks=1, reduce=WR_NONE), why='32x128 tile'),
    _case('g_40x3_k4s2_16x16', 'dense', 40, 3, 4, 2, 32, 32, stride=2, pad=1,
          claims=_c(GATHER, T64, chunks=4, grid_z=4, reduce=WR_SLAB, xcd=0), why='4 chunks, slab_reduce'),
    _case('g_64x3_k4s2_32x32', 'dense', 64, 3, 4, 6, 64, 64, stride=2, pad=1,
          claims=_c(GATHER, T64, chunks=48, grid_z=48, reduce=WR_WIDE, xcd=1), why='48 chunks, slab_reduce_wide, XCD-pinned'),
    _case('g_64x3_k4s2_32x32_xcd0', 'dense', 64, 3, 4, 6, 64, 64, stride=2, pad=1, opts={'wgrad_xcd': 0},
          claims=_c(GATHER, T64, reduce=WR_WIDE, xcd=0), why='the same chunks numbered plainly'),
    _case('g_40x5_k1_6x6', 'dense', 40, 5, 1, 2, 6, 6, claims=_c(GATHER, T64, reduce=WR_NONE), why='KS 1'),
    _case('g_40x3_k7r_8x8', 'dense', 40, 3, 7, 1, 8, 8, reflect=True, claims=_c(GATHER, T64, reduce=WR_NONE), why='KS 7, reflect pad 3'),
    _case('g_40x4_k3_up2_8x8', 'dense', 40, 4, 3, 1, 4, 4, ups=2, claims=_c(GATHER, T64, reduce=WR_NONE), why='nearest x2 upsample'),
    _case('g_24x5_k3_13x20_slab', 'dense', 24, 5, 3, 3, 13, 20, claims=_c(GATHER, T32, reduce=WR_SLAB),
          why='32x128 tile with slabs; odd plane'),
    _case('g_40x3_k4s2_16x16_ws1', 'dense', 40, 3, 4, 2, 32, 32, stride=2, pad=1, ws=_slabs(1),
          claims=_c(GATHER, T64, chunks=1, grid_z=1, reduce=WR_NONE), why='workspace of one slab: the split shrinks to 1, direct store'),
    _case('g_40x3_k4s2_16x16_nows', 'dense', 40, 3, 4, 2, 32, 32, stride=2, pad=1, ws=0, gb=False,
          claims=_c(GATHER, T64, chunks=1, grid_z=1, reduce=WR_NONE), why='no workspace at all'),
    # ---- tap-major ---------------------------------------------------------------------------------------------------------
    _case('t_16x48_k3_8x8', 'dense', 16, 48, 3, 1, 8, 8, claims=_c(TAP, T32, cpad=128, a_vec=1, nomask=0, reduce=WR_UNPERMUTE, rowsum_fused=1),
          why='32x128 tile; cpad 128 against 48 real channels: the column tail'),
    _case('t_64x48_k3_8x8', 'dense', 64, 48, 3, 2, 8, 8, claims=_c(TAP, T64, cpad=64, a_vec=1, rowsum_fused=1), why='64x64 tile'),
    _case('t_40x70_k3_7x9', 'dense', 40, 70, 3, 1, 7, 9, claims=_c(TAP, T64, cpad=128, a_vec=0, rowsum_fused=1),
          why='ragged M and C; PQ = 63: scalar A, k tail'),
    _case('t_128x128_k3_8x8', 'dense', 128, 128, 3, 1, 8, 8, claims=_c(TAP, T128, cpad=128, a_vec=1, rowsum_fused=1), why='128x128 tile'),
    _case('t_130x140_k3_8x8', 'dense', 130, 140, 3, 4, 8, 8, claims=_c(TAP, T64, cpad=192, chunks=2, grid_z=2, rowsum_fused=1),
          why='M and C past two 64-tiles (the padding to 256 x 256 keeps it off the 128-tile); 2 chunks'),
    _case('t_128x140_k3_8x8', 'dense', 128, 140, 3, 1, 8, 8, claims=_c(TAP, T128, cpad=256, rowsum_fused=1),
          why='128x128 tile, C past one column tile: cpad 256 against 140 real channels'),
    _case('t_130x128_k3_8x8', 'dense', 130, 128, 3, 4, 8, 8, claims=_c(TAP, T128, cpad=128, chunks=2, grid_z=2, a_vec=1, rowsum_fused=1),
          why='128x128 tile with M one past a tile; 2 chunks'),
    _case('t_64x64_k3r_8x8', 'dense', 64, 64, 3, 2, 8, 8, reflect=True, claims=_c(TAP, T64, nomask=1, a_vec=1), why='mask-free loader'),
    _case('t_64x64_k3r_7x9', 'dense', 64, 64, 3, 1, 7, 9, reflect=True, claims=_c(TAP, T64, nomask=0, a_vec=0),
          why='reflect, masked since Kpix % 16 != 0'),
    _case('t_64x64_k3_16x16', 'dense', 64, 64, 3, 3, 16, 16, claims=_c(TAP, T64, kchunk=96, chunks=8, grid_z=8, xcd=1, rowsum_fused=1),
          why='6 planned chunks re-cut into 8 for XCD pinning, renumbered'),
    _case('t_64x64_k3_16x16_nogb', 'dense', 64, 64, 3, 3, 16, 16, gb=False, claims=_c(TAP, T64, chunks=8, grid_z=8, xcd=1), why='no bias gradient'),
    _case('t_64x64_k3_16x16_xcd0', 'dense', 64, 64, 3, 3, 16, 16, opts={'wgrad_xcd': 0},
          claims=_c(TAP, T64, kchunk=128, chunks=6, grid_z=6, xcd=0, rowsum_fused=1), why='option off: the 6 planned chunks'),
    _case('t_64x64_k3_43x48_empty', 'dense', 64, 64, 3, 1, 43, 48, claims=_c(TAP, T64, kchunk=144, chunks=15, grid_z=16, xcd=1, rowsum_fused=1),
          why='Kpix = 2064: 11 planned chunks re-cut for 16 leave 15 with pixels: one EMPTY chunk, whose slab and row sums must be zeros'),
    _case('t_64x64_k3r_43x48_empty', 'dense', 64, 64, 3, 1, 43, 48, reflect=True,
          claims=_c(TAP, T64, chunks=15, grid_z=16, xcd=1, nomask=0, rowsum_fused=1),
          why='the same under reflection padding, Kpix % 16 == 0: an empty chunk must not run the mask-free loader'),
    _case('t_3x64_k7r_16x16', 'dense', 3, 64, 7, 2, 16, 16, reflect=True, claims=_c(TAP, T32, cpad=128, nomask=1, rowsum_fused=1), why='M = 3, KS 7'),
    _case('t_16x64_k1_8x8', 'dense', 16, 64, 1, 2, 8, 8, claims=_c(TAP, T32, rowsum_fused=1), why='KS 1'),
    _case('t_16x48_k3_18x18_ws1', 'dense', 16, 48, 3, 1, 18, 18, ws=_slabs(1),
          claims=_c(TAP, T32, kchunk=324, chunks=1, grid_z=1, rowsum_fused=0),
          why='workspace of one slab: the split shrinks to 1 (no room for row sums: sg_channel_sum); one chunk of 324 pixels crosses '
              'the 256-pixel table block'),
    _case('t_16x48_k3_3x3', 'dense', 16, 48, 3, 1, 3, 3, claims=_c(TAP, T32, chunks=1, a_vec=0), why='Kpix = 9 < 16'),
    _case('t_64x64_k3_16x16_ws3', 'dense', 64, 64, 3, 3, 16, 16, ws=_slabs(3),
          claims=_c(TAP, T64, kchunk=256, chunks=3, grid_z=3, xcd=0, rowsum_fused=0), why='workspace of three slabs: 6 chunks shrink to 3'),
    _case('t_64x64_k3_16x16_norow', 'dense', 64, 64, 3, 3, 16, 16, ws=_slabs(6),
          claims=_c(TAP, T64, kchunk=128, chunks=6, grid_z=6, xcd=0, rowsum_fused=0),
          why='room for the slabs, none for row sums (nor for XCD padding): sg_channel_sum'),
    _case('t_130x128_k3_8x8_exact', 'dense', 130, 128, 3, 4, 8, 8, ws=_slabs(None, rowsum=True), claims=_c(TAP, T128, chunks=2, a_vec=1, rowsum_fused=1),
          why='exactly the bytes the plan needs: a row sum stored for a row m >= M of the last chunk lands on the guard words'),
    _case('t_40x70_k3_7x9_exact', 'dense', 40, 70, 3, 1, 7, 9, ws=_slabs(None, rowsum=True), claims=_c(TAP, T64, a_vec=0, rowsum_fused=1),
          why='the same for the scalar A loader, M = 40 in a 64-row tile'),
    _case('t_40x70_k3_8x8_exact', 'dense', 40, 70, 3, 2, 8, 8, ws=_slabs(None, rowsum=True), claims=_c(TAP, T64, a_vec=1, rowsum_fused=1),
          why='and for the vector A loader on the 64-row tile'),
    _case('t_130x128_k3_8x8_off', 'dense', 130, 128, 3, 4, 8, 8, a_off=1, claims=_c(TAP, T128, a_vec=0, rowsum_fused=1),
          why='gy 4 bytes off a 16-byte boundary: scalar A on the 128-row tile'),
    _case('t_128x128_k3r_8x8', 'dense', 128, 128, 3, 1, 8, 8, reflect=True, claims=_c(TAP, T128, nomask=1, a_vec=1),
          why='mask-free loader on the 128x128 tile (the operators send this shape to Winograd; the C ABI does not)'),
    _case('t_130x128_k3r_8x8_off', 'dense', 130, 128, 3, 4, 8, 8, reflect=True, a_off=1, claims=_c(TAP, T128, nomask=1, a_vec=0),
          why='the same with the scalar A loader'),
    _case('t_64x64_k3r_8x8_off', 'dense', 64, 64, 3, 2, 8, 8, reflect=True, a_off=1, claims=_c(TAP, T64, nomask=1, a_vec=0),
          why='mask-free B loader next to the scalar A loader'),
    _case('t_16x64_k3r_8x8_off', 'dense', 16, 64, 3, 2, 8, 8, reflect=True, a_off=1, claims=_c(TAP, T32, nomask=1, a_vec=0), why='the same, 32-row tile'),
    _case('t_40x70_k3_8x8_off', 'dense', 40, 70, 3, 2, 8, 8, a_off=1, claims=_c(TAP, T64, a_vec=0, rowsum_fused=1), why='the same, 64-row tile'),
    # ---- two sources (tap-major is forced) ---------------------------------------------------------------------------------
    _case('two_24x7+3_k4s2_9x10', 'dense', 24, 7, 4, 3, 17, 18, stride=2, pad=2, C2=3, claims=_c(T32, form=WG_TAP, two=1, nomask=0, cpad=128),
          why='C = 10 < 48, tap-major because of the second source'),
    _case('two_24x7+3_k4s2_9x10_bcast', 'dense', 24, 7, 4, 3, 17, 18, stride=2, pad=2, C2=3, bcast=1, claims=_c(T32, form=WG_TAP, two=1),
          why='second source a row per sample, broadcast'),
    _case('two_40x50+30_k3r_6x8', 'dense', 40, 50, 3, 2, 6, 8, C2=30, reflect=True, claims=_c(T64, form=WG_TAP, two=1, nomask=0, cpad=128),
          why='a 64-column tile straddles C1 = 50; reflect with two sources stays masked'),
    _case('two_40x50+30_k3_6x8_bcast', 'dense', 40, 50, 3, 2, 6, 8, C2=30, bcast=1, claims=_c(T64, form=WG_TAP, two=1), why='straddling tile, broadcast'),
    # ---- sg_conv2d_wgrad_sparse -------------------------------------------------------------------------------------------
    _case('sp_16_L2of6_k3_5x5', 'sparse', 16, 6, 3, 3, 5, 5, L=2, claims=_c(T32, form=WG_TAP, cpad=128, reduce=WR_SPARSE, chunks=3, grid_z=3, kchunk=25, nomask=0),
          why='L 2'),
    _case('sp_72_L48of80_k3r_4x4', 'sparse', 72, 80, 3, 2, 4, 4, L=48, reflect=True, claims=_c(T64, form=WG_TAP, cpad=64, reduce=WR_SPARSE, nomask=1, a_vec=1),
          why='M > 64, L 48; PQ = 16 with reflect: mask-free'),
    _case('sp_40_L70of80_k3r_5x7', 'sparse', 40, 80, 3, 2, 5, 7, L=70, reflect=True, claims=_c(T64, form=WG_TAP, cpad=128, reduce=WR_SPARSE, nomask=0, a_vec=0),
          why='L 70; PQ = 35: masked'),
    _case('sp_130_L70of80_k3_4x4', 'sparse', 130, 80, 3, 2, 4, 4, L=70, claims=_c(T128, form=WG_TAP, cpad=128, reduce=WR_SPARSE), why='128-row tile'),
    _case('sp_24_L3of8_k4s2_4x4', 'sparse', 24, 8, 4, 2, 8, 8, stride=2, pad=1, L=3, claims=_c(T32, form=WG_TAP, reduce=WR_SPARSE), why='KS 4 stride 2'),
    # ---- sg_conv2d_wgrad_perimage -----------------------------------------------------------------------------------------
    _case('pi_8_L3of5_k3_9x9', 'perimage', 8, 5, 3, 2, 9, 9, L=3, claims=_c(T32, form=WG_GATHER, reduce=WR_NONE, chunks=2, grid_z=2, xcd=0, a_vec=0),
          why='few-channel form, S = 1: the GEMM stores the per-image result'),
    _case('pi_16_L4of6_k4s2_6x6', 'perimage', 16, 6, 4, 2, 12, 12, stride=2, pad=1, L=4, claims=_c(T32, form=WG_GATHER, reduce=WR_NONE), why='KS 4 stride 2'),
    _case('pi_64_L1of3_k7r_32x32', 'perimage', 64, 3, 7, 1, 32, 32, reflect=True, L=1,
          claims=_c(T64, form=WG_PADDED, reduce=WR_GROUP, kchunk=256, chunks=4, grid_z=4, xcd=0, a_vec=1), why='S = 4 chunks inside the image; padded planes'),
    _case('pi_64_L1of3_k7r_32x32_gather', 'perimage', 64, 3, 7, 1, 32, 32, reflect=True, L=1, opts={'wgrad_padded': 0},
          claims=_c(T64, form=WG_GATHER, reduce=WR_GROUP, grid_z=4, a_vec=1), why='the same through the gather (bit-equal)'),
    _case('pi_64_L1of3_k7r_32x32_base', 'perimage', 64, 3, 7, 1, 32, 32, reflect=True, L=1, ws=_sparse_base,
          claims=_c(T64, form=WG_GATHER, reduce=WR_GROUP, grid_z=4), why='workspace without room for the planes: gather route'),
    _case('pi_40_L2of4_k7r_32x32_xcd', 'perimage', 40, 4, 7, 2, 32, 32, reflect=True, L=2,
          claims=_c(T64, form=WG_PADDED, reduce=WR_GROUP, chunks=8, grid_z=8, xcd=2), why='2 images x 4 chunks pinned to XCDs'),
    _case('pi_40_L2of4_k7r_32x32_xcd0', 'perimage', 40, 4, 7, 2, 32, 32, reflect=True, L=2, opts={'wgrad_xcd': 0},
          claims=_c(T64, form=WG_PADDED, reduce=WR_GROUP, grid_z=8, xcd=0), why='numbered plainly'),
    _case('pi_8_L3of5_k7r_9x10', 'perimage', 8, 5, 7, 2, 9, 10, reflect=True, L=3, claims=_c(T32, form=WG_PADDED, reduce=WR_NONE, a_vec=0),
          why='padded planes, S = 1, 32-row tile: scalar A'),
    _case('pi_40_L3of5_k7r_9x10_off', 'perimage', 40, 5, 7, 2, 9, 10, reflect=True, L=3, a_off=1, claims=_c(T64, form=WG_PADDED, a_vec=0), why='unaligned gy'),
    _case('pi_40_L22of30_k3_6x6', 'perimage', 40, 30, 3, 2, 6, 6, L=22,
          claims=_c(T64, form=WG_TAP, cpad=64, reduce=WR_PERIMAGE, chunks=2, grid_z=2, kchunk=36), why='L = 22 leaves the few-channel form: tap-major, per-image copy'),
    _case('pi_40_L21of30_k3_6x6', 'perimage', 40, 30, 3, 2, 6, 6, L=21, claims=_c(T64, form=WG_GATHER, reduce=WR_NONE), why='L = 21: the last few-channel length'),
]
BY_NAME = dict((c['name'], c) for c in CASES)
assert len(BY_NAME) == len(CASES)


def case_desc(case):
    d = make_desc(case['N'], case['C1'], case['H'], case['W'], case['Cout'], case['KS'], case['stride'], case['pad'], case['reflect'],
                  case['ups'], case['OH'], case['OW'], C2=case['C2'])
    d.x2_broadcast = case['bcast']
    return d


def case_py_plan(case, a_mod16, ws_bytes, opts=None):
    o = dict(wgrad_xcd=1, wgrad_rowsum=1, wgrad_padded=1)
    o.update(case['opts'])
    o.update(opts or {})
    return py_plan(ENTRY_OF[case['kind']], case['N'], case['C1'], case['C2'], case['H'], case['W'], case['Cout'], case['KS'],
                   case['stride'], case['pad'], int(case['reflect']), case['ups'], case['OH'], case['OW'], L=case['L'], a_mod16=a_mod16,
                   ws_bytes=ws_bytes, xcd=o['wgrad_xcd'], rowsum=o['wgrad_rowsum'], padded=o['wgrad_padded'])


def case_ws_bytes(case, plan_of):
    """bytes of workspace the row offers; plan_of(ws_bytes) -> the plan under the row's options for that offer"""
    return int(case['ws'](plan_of(AMPLE), case)) if callable(case['ws']) else int(case['ws'])


def case_lists(case):
    """(lists [N, L] int32, cnt [N]) of a sparse / per-image row: unsorted, no prefixes, images of different length, the last channel
    listed by nobody, channel ``only`` by image 0 alone; the tail of a short list repeats its first entry (never read)"""
    N, L, C = case['N'], case['L'], case['C1'] + case['C2']
    rng = rng_of(case['shape_key'] + '|lists')
    only = int(rng.randint(0, C - 1))
    pool = [c for c in range(C - 1) if c != only]
    lists, cnt = np.zeros((N, L), dtype=np.int32), np.zeros(N, dtype=np.int32)
    for b in range(N):
        n = L if b == 0 else max(1, min(L, len(pool)) - (1 + b) % 3)
        if b == 0:
            ch = [only] + [int(c) for c in rng.permutation(pool)[:n - 1]]
            ch = [int(c) for c in rng.permutation(ch)]
        else:
            ch = [int(c) for c in rng.permutation(pool)[:n]]
        if n > 1 and ch == sorted(ch):
            ch = ch[::-1]
        lists[b, :n], lists[b, n:], cnt[b] = ch, ch[0], n
    return lists, cnt


_INPUTS, _REFS = {}, {}


def case_inputs(case):
    """deterministic operands of the row's shape (shared by the rows of one shape; never modified)"""
    k = case['shape_key']
    if k not in _INPUTS:
        rng = rng_of(k)
        N, H, W = case['N'], case['H'], case['W']
        inp = dict(gy=f32(rng, (N, case['Cout'], case['OH'], case['OW'])), x1=f32(rng, (N, case['C1'], H, W)), x2=None)
        if case['C2']:
            inp['x2'] = f32(rng, (N, case['C2']) if case['bcast'] else (N, case['C2'], H, W))
        if case['kind'] != 'dense':
            inp['lists'], inp['cnt'] = case_lists(case)
        _INPUTS[k] = inp
    return _INPUTS[k]


def _result(case, inp, gy, x):
    g = wgrad_images(gy, x, case['KS'], case['stride'], case['pad'], case['reflect'], case['ups'])
    if case['kind'] == 'sparse':
        return sparse_wgrad(g, inp['lists'], inp['cnt'])
    if case['kind'] == 'perimage':
        return perimage_wgrad(g, inp['lists'], inp['cnt'])
    return g.sum(axis=0)


def case_refs(case):
    """float64 reference, the number of terms and sum|a||b| of every output element; the same for the bias gradient"""
    k = case['shape_key']
    if k not in _REFS:
        inp = case_inputs(case)
        gy = inp['gy'].astype(np.float64)
        x = sources(inp['x1'].astype(np.float64), None if inp['x2'] is None else inp['x2'].astype(np.float64), case['bcast'])
        _REFS[k] = dict(gw=_result(case, inp, gy, x), terms=_result(case, inp, np.ones_like(gy), np.ones_like(x)),
                        sabs=_result(case, inp, np.abs(gy), np.abs(x)), gb=bias_grad(gy),
                        gb_bound=gamma(case['N'] * case['OH'] * case['OW']) * bias_grad(np.abs(gy)))
    return _REFS[k]


def joins(case, plan):
    """c of the bound: the adds that join the k-chunks of one output element under this plan (module docstring)"""
    if case['kind'] == 'sparse':
        return case['N']
    if case['kind'] == 'perimage':
        return plan['grid_z'] // case['N']
    return plan['grid_z']


def gw_bound(case, plan):
    r = case_refs(case)
    return bound(r['terms'], joins(case, plan), r['sabs'])


def plan_classes(case, plan):
    """what distinguishes launches as code paths: the kernel instantiation (form, tile, A width, sources, mask, kernel size where it
    is a template argument), the chunking regime, the reduce kernel, the bias-gradient route"""
    ks = case['KS'] if plan['form'] != WG_TAP else 0
    out = {('kernel', plan['form'], plan['bm'], plan['bn'], plan['a_vec'], plan['two'], plan['nomask'], ks, case['kind'] != 'dense'),
           ('reduce', plan['reduce']), ('xcd', plan['xcd']),
           ('chunks', 'one' if plan['grid_z'] == 1 else ('empty' if plan['chunks'] < plan['grid_z'] else 'many'))}
    if case['kind'] == 'dense' and case['gb']:
        out.add(('gb', 'rowsum' if plan['rowsum_fused'] else 'channel_sum', plan['bm'], plan['a_vec']))
    return out
