"""Case table, input builders, float64 references and rounding bounds of the forward-gather convolution tests: run_kn<KS, 0> /
launch_ab of csrc/igemm_core.h and run_kn_sparse of csrc/igemm_kn0.hip, planned by kn_plan / kn_sparse_plan, behind sg_conv2d_fwd,
sg_conv2d_fwd_sparse and sg_conv2d_fwd_perimage.  Shared by tests/test_forward_conv_cases_cpu.py (the references agree with torch in
float64, every row has the plan it claims, the table reaches every plan class of a literal list, the Python restatement of the plan
equals the query over a grid) and tests/test_gpu_forward_conv.py (every row against float64 on the device).

NumPy only.  The reference restates the operation tap by tap from its definition (dtype-generic: the one-hot probes run it in
float32, where a single product is exact):
    y[n,m,oh,ow] = act(bias[m] + sum_{c,kh,kw} w[m,c,kh,kw] * X[n,c,oh*s-p+kh, ow*s-p+kw])
X the logical input grid: the stored planes nearest-upsampled x2 (optional) BEFORE padding, zero- or reflection-padded; channels
>= C1 come from a second source, optionally a row per sample [N, C2] broadcast over the plane.  The sparse entry sums, for image b,
the channels list[b][:cnt[b]] only; the per-image entry does the same with weights wimg[b][m][j] at list position j.

The launch plans come from the library's host-side query (include/sg2im_hip.h: sg_conv2d_fwd_plan), the functions the launchers run
from; py_plan() restates them and is compared with the query over a grid.

Bounds.  Every output element is an fp32 fma chain over the reduced K (structural zeros -- a tap outside the plane, the zero-padded
tail of the compact weights -- add 0 exactly), plus the bias add, plus the c joins of the plan:
    |got - ref64| <= ACT_LIPSCHITZ[act] * gamma(K + 1 + c) * (sum|w||x| + |bias|)        (+ 1e-6 max(1, |y|) for tanh, as dense_ref)
K = the plan's K (Cin*KS*KS, or the padded compact K of the list entries); c = splits - 1 for a split launch (the slab reduce adds
the slabs in order); c = tail_smax for an unsplit launch of more tiles than the chip has CUs, which the tail split (not reported
by the plan: it depends on the CU count) may run as up to tail_smax k-pieces; c = 0 otherwise.
"""
import ctypes

import numpy as np

from scene_generation_amd._hip import CONST, plan_dict, sgFwdPlan

from dense_pointwise_cases import gamma, rng_of, f32, act_ref, ACT_LIPSCHITZ, ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH  # noqa: F401
from transposed_conv_cases import option, make_desc, conv_out_size  # noqa: F401  (re-exported)
from wgrad_cases import _reflect, _axis, sources  # noqa: F401

# ---- constants the plan is built around (tests/test_forward_conv_cases_cpu.py reads them back from the sources)
BK = 16                 # igemm_core.h: sub-tile depth = k-tile depth of the gather tiles (SG_NSUB = 1)
KTAB_ROUND, KTAB_EXTRA, KENTRY_BYTES = 64, 128, 8        # ktab_bytes / sparse_kpad: entries rounded to 64, + 128 prefetched past the end
SPARSE_SLACK = 64       # sparse_fwd_ws: bytes per image behind the compact weights (kcnt)
SPLIT_TARGET_128, SPLIT_MAX = 1024, 8
N_CU = 256              # MI355X: launches of more tiles than this may be tail-split
OPTION_DEFAULTS = dict(tile=-1, t128_min=384, tile3=1, tile3_min=768, split_target=1536, split_kmin=2048, splits=-1, fixedtap=1)
TAIL_DEFAULTS = dict(w43_tail_split=2, tail_smax=4, tail_ktmin=8)
SLOPE = 0.2

# include/sg2im_hip.h, under the short names the tables use
FW_CONV, FW_SPARSE, FW_PERIMAGE = (CONST['SG_FW_' + n] for n in ('CONV', 'SPARSE', 'PERIMAGE'))
FW_TABLE, FW_FIXED = CONST['SG_FW_TABLE'], CONST['SG_FW_FIXED']
FR_NONE, FR_VEC, FR_SCALAR = (CONST['SG_FR_' + n] for n in ('NONE', 'VEC', 'SCALAR'))
ENTRY_OF = {'dense': FW_CONV, 'sparse': FW_SPARSE, 'perimage': FW_PERIMAGE}
ENTRY_FN = {'dense': 'sg_conv2d_fwd', 'sparse': 'sg_conv2d_fwd_sparse', 'perimage': 'sg_conv2d_fwd_perimage'}
PLAN_FIELDS = tuple(n for n, t in sgFwdPlan._fields_ if t is ctypes.c_int32)
AMPLE = 8 << 20         # bytes: more workspace than any row's plan needs
TILES = {0: (128, 128), 1: (64, 64), 2: (32, 128), 3: (64, 128)}


def fwd_plan(lib, desc, entry, L=0, w_mod16=0, y_mod16=0, ws_mod16=0, ws_bytes=AMPLE):
    """sg_conv2d_fwd_plan under the current options -> dict, or None when the query returns non-zero"""
    p = sgFwdPlan()
    rc = lib.sg_conv2d_fwd_plan(ctypes.byref(desc), int(entry), int(L), int(w_mod16), int(y_mod16), int(ws_mod16), int(ws_bytes),
                                ctypes.byref(p))
    return None if rc else plan_dict(p)


# =============================================================================================
# the plan, restated (pick_tile, kn_tiles, kn_splits, kn_plan, kn_sparse_plan, ktab_bytes, sparse_fwd_ws of csrc/igemm_core.h; the
# argument checks of csrc/igemm.hip)
# =============================================================================================
def _cdiv(a, b):
    return -(-a // b)


def pick_tile(M, N, o):
    if 0 <= o['tile'] <= 3:
        return o['tile']
    if M <= 32:
        return 2
    t128 = _cdiv(M, 128) * _cdiv(N, 128)
    low_waste = _cdiv(M, 128) * 128 * 20 <= M * 23 and N >= 512
    over = t128 % 512
    ragged128 = 512 < t128 < 1536 and 0 < over < 128
    if M >= 96 and low_waste and not ragged128 and (M >= 512 or t128 >= o['t128_min']):
        return 0
    if o['tile3'] and _cdiv(M, 64) * _cdiv(N, 128) >= o['tile3_min']:
        return 3
    return 1


def kn_tiles(M, Npix, o):
    bm, bn = TILES[pick_tile(M, Npix, o)]
    return (1 if bm == 32 else _cdiv(M, bm)) * _cdiv(Npix, bn)


def kn_splits(M, Npix, K, o):
    if o['splits'] > 0:
        return o['splits']
    tiles = kn_tiles(M, Npix, o)
    target = SPLIT_TARGET_128 if pick_tile(M, Npix, o) == 0 else o['split_target']
    kmin = o['split_kmin']
    if tiles * 4 >= target * 3 or K < kmin:
        return 1
    sp = (target + tiles // 2) // tiles
    if sp > 2 and sp & 1:
        sp += 1
    sp = min(sp, K // (kmin // 2), SPLIT_MAX)
    return 1 if sp < 2 else sp


def ktab_bytes(K):
    return (_cdiv(K, KTAB_ROUND) * KTAB_ROUND + KTAB_EXTRA) * KENTRY_BYTES


def sparse_kc(L, KS2):
    return _cdiv(L * KS2, BK) * BK


def sparse_fwd_ws(N, M, L, KS2):
    kc = sparse_kc(L, KS2)
    return N * ((_cdiv(kc, KTAB_ROUND) * KTAB_ROUND + KTAB_EXTRA) * KENTRY_BYTES + M * kc * 4 + SPARSE_SLACK)


def desc_ok(N, C1, C2, H, W, M, KS, stride, pad, reflect, ups, OH, OW):
    """check_desc of csrc/igemm.hip (without the 2^29-element limits, which no row or grid point approaches)"""
    if KS not in (1, 3, 4, 7) or stride not in (1, 2) or ups not in (1, 2):
        return False
    if min(N, C1, M, H, W, OH, OW) <= 0 or C2 < 0:
        return False
    if reflect:
        if not (0 <= pad < H * ups and pad < W * ups):
            return False
        if (OH - 1) * stride + KS > H * ups + 2 * pad or (OW - 1) * stride + KS > W * ups + 2 * pad:
            return False
    return True


def py_plan(entry, N, C1, C2, H, W, M, KS, stride, pad, reflect, ups, OH, OW, bcast=0, L=0, w_mod16=0, y_mod16=0, ws_mod16=0,
            ws_bytes=AMPLE, **options):
    """-> the dict fwd_plan() returns, or None where the query refuses; options: the library options at other than their defaults"""
    o = dict(OPTION_DEFAULTS)
    o.update(options)
    if entry not in (FW_CONV, FW_SPARSE, FW_PERIMAGE) or any(m not in (0, 4, 8, 12) for m in (w_mod16, y_mod16, ws_mod16)):
        return None
    if not desc_ok(N, C1, C2, H, W, M, KS, stride, pad, reflect, ups, OH, OW):
        return None
    KS2, C, PHW = KS * KS, C1 + C2, OH * OW
    Npix = N * PHW
    two = int(C2 > 0)
    out = dict(two=two, bcast=int(bool(two and bcast)))
    if entry == FW_CONV:
        K = C * KS2
        if ws_bytes < ktab_bytes(K):
            return None
        vec = K % 4 == 0 and w_mod16 == 0
        tile = pick_tile(M, Npix, o)
        if not vec and tile == 0:
            tile = 1
        bm, bn = TILES[tile]
        nomask = bool(vec and reflect and Npix % bn == 0 and M % bm == 0 and K % BK == 0)
        splits = kn_splits(M, Npix, K, o)
        if splits > 1 and ws_bytes < ktab_bytes(K) + splits * M * Npix * 4:
            splits = 1
        kchunk = K
        if splits > 1:
            kchunk = _cdiv(_cdiv(K, splits), BK) * BK
            splits = _cdiv(K, kchunk)
            if splits == 1:
                kchunk = K
        fixed = bool(o['fixedtap'] and KS in (1, 4) and vec and not two and K % BK == 0)
        reduce = FR_NONE
        if splits > 1:
            reduce = FR_VEC if ((M * Npix) % 4 == 0 and PHW % 4 == 0 and ws_mod16 == 0 and y_mod16 == 0) else FR_SCALAR
        out.update(bm=bm, bn=bn, a_vec=int(vec), loader=FW_FIXED if fixed else FW_TABLE, nomask=int(nomask and not fixed), K=K,
                   splits=splits, kchunk=kchunk, reduce=reduce, batched=0,
                   ws_needed=ktab_bytes(K) + (splits * M * Npix * 4 if splits > 1 else 0))
        return out
    if not 0 < L <= C:
        return None
    need = sparse_fwd_ws(N, M, L, KS2)
    if ws_bytes < need or ws_mod16 != 0:
        return None
    bm, bn = TILES[pick_tile(M, Npix, o)]
    kc = sparse_kc(L, KS2)
    out.update(bm=bm, bn=bn, a_vec=1, loader=FW_TABLE, nomask=int(bool(reflect and PHW % bn == 0 and M % bm == 0)), K=kc, splits=1,
               kchunk=kc, reduce=FR_NONE, batched=1, ws_needed=need)
    return out


# =============================================================================================
# float64 (dtype-generic) restatement, tap by tap
# =============================================================================================
def conv_images(x, wimg, KS, s, p, reflect, ups, OH, OW):
    """pre[n,m,oh,ow] = sum_{c,kh,kw} wimg[n,m,c,kh,kw] X[n,c,oh*s-p+kh,ow*s-p+kw]: the conv image by image, each with its own
    weights (x [N,C,H,W] the stored channel concat; wimg [N or 1, M, C, KS, KS])"""
    N, C, H, W = x.shape
    M = wimg.shape[1]
    y = np.zeros((N, M, OH * OW), dtype=x.dtype)
    for kh in range(KS):
        ih, vh = _axis(OH, s, p, kh, H * ups, reflect, ups)
        for kw in range(KS):
            iw, vw = _axis(OW, s, p, kw, W * ups, reflect, ups)
            xs = x[:, :, ih][:, :, :, iw] * (vh[:, None] & vw[None, :]).astype(x.dtype)
            y += np.matmul(wimg[:, :, :, kh, kw], xs.reshape(N, C, OH * OW))
    return y.reshape(N, M, OH, OW)


def list_weights(w, lists, cnt, C):
    """the sparse entry's weights image by image, [N, M, C, KS, KS]: w on the channels list[b][:cnt[b]], zero elsewhere"""
    out = np.zeros((len(cnt),) + w.shape, dtype=w.dtype)
    for b in range(len(cnt)):
        ch = [int(c) for c in lists[b][:cnt[b]]]
        out[b][:, ch] = w[:, ch]
    return out


def perimage_weights(wimg, lists, cnt, C):
    """the per-image entry's weights scattered to channels: [N, M, C, KS, KS] with wimg[b, :, j] at channel list[b][j], j < cnt[b]"""
    N, M, L = wimg.shape[:3]
    out = np.zeros((N, M, C) + wimg.shape[3:], dtype=wimg.dtype)
    for b in range(N):
        for j in range(int(cnt[b])):
            out[b][:, int(lists[b][j])] = wimg[b][:, j]
    return out


def gather_wimg(w, lists, cnt):
    """wimg [N, M, L, KS, KS] that makes sg_conv2d_fwd_perimage the same sum as sg_conv2d_fwd_sparse on w (NaN beyond cnt[b]: never read)"""
    N, L = lists.shape
    out = np.full((N, w.shape[0], L) + w.shape[2:], np.nan, dtype=w.dtype)
    for b in range(N):
        for j in range(int(cnt[b])):
            out[b][:, j] = w[:, int(lists[b][j])]
    return out


# =============================================================================================
# the case table
# =============================================================================================
def _case(name, entry, Cout, C1, KS, N, H, W, stride=1, pad=None, reflect=False, ups=1, C2=0, bcast=0, L=0, bias=True, act=ACT_NONE,
          opts=None, optsets=None, ws='ample', w_off=0, y_off=0, ws_off=0, claims=None, tags=(), why=''):
    """entry: 'dense' (sg_conv2d_fwd), 'sparse', 'perimage'.  H x W: the stored input plane.  opts: library options of the row;
    optsets: further options the row runs under one after the other (default: just opts); ws: 'ample' or 'ktab' (the k-table bytes
    alone); w_off / y_off / ws_off: floats the weights / the result / the workspace are offset from a 16-byte boundary; claims: the
    plan fields the row is there for; tags: the plan classes (plan_classes) it is there for"""
    pad = (KS - 1) // 2 if pad is None else pad
    OH, OW = conv_out_size(H * ups, KS, stride, pad), conv_out_size(W * ups, KS, stride, pad)
    signed = act in (ACT_RELU, ACT_LEAKY)
    return dict(name=name, entry=entry, Cout=Cout, C1=C1, C2=C2, KS=KS, N=N, H=H, W=W, stride=stride, pad=pad, reflect=bool(reflect),
                ups=ups, bcast=bcast, L=L, bias=bias, act=act, slope=SLOPE, opts=dict(opts or {}), optsets=list(optsets or [{}]), ws=ws,
                w_off=w_off, y_off=y_off, ws_off=ws_off, claims=dict(claims or {}), tags=tuple(tags), why=why, OH=OH, OW=OW, signed=signed,
                shape_key='%s|%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d' % (entry, Cout, C1, C2, KS, N, H, W, stride, pad, int(reflect), ups,
                                                                            bcast, L, int(bias), int(signed)))


def _kernel_rows():
    """one row per (tile, A width, loader, sources, mask) instantiation launch_ab reaches in MODE 0, the tile forced through the
    option ``tile`` so that the shapes stay small"""
    rows = []
    for t, (bm, bn) in sorted(TILES.items()):
        T = '%dx%d' % (bm, bn)
        o = {'tile': t}
        pl = dict(bm=bm, bn=bn)
        rows += [
            _case('k_%s_vec_one_mask' % T, 'dense', 40, 16, 3, 1, 6, 6, opts=o, claims=dict(pl, a_vec=1, loader=FW_TABLE, two=0, nomask=0),
                  tags=[('kernel', bm, bn, 1, 'table', 'one', 'mask')], why='float4 A, table loader, zero padding'),
            _case('k_%s_vec_one_nomask' % T, 'dense', bm, 16, 3, 2, 8, 8, reflect=True, opts=o, claims=dict(pl, a_vec=1, two=0, nomask=1),
                  tags=[('kernel', bm, bn, 1, 'table', 'one', 'nomask')], why='reflect, full tiles, K = 144: mask-free loader, plain loads'),
            _case('k_%s_vec_two_mask' % T, 'dense', 40, 10, 3, 1, 6, 6, C2=6, opts=o, claims=dict(pl, a_vec=1, two=1, bcast=0, nomask=0),
                  tags=[('kernel', bm, bn, 1, 'table', 'two', 'mask')], why='two sources'),
            _case('k_%s_vec_two_nomask' % T, 'dense', bm, 10, 3, 2, 8, 8, C2=6, reflect=True, opts=o, claims=dict(pl, a_vec=1, two=1, nomask=1),
                  tags=[('kernel', bm, bn, 1, 'table', 'two', 'nomask')], why='two sources, mask-free'),
            _case('k_%s_fixed' % T, 'dense', 40, 16, 4, 2, 8, 8, stride=2, pad=1, opts=o, claims=dict(pl, a_vec=1, loader=FW_FIXED, nomask=0),
                  tags=[('kernel', bm, bn, 1, 'fixed', 'one', 'mask')], why='4x4 stride 2, K = 256: fixed taps per thread'),
        ]
        if t != 0:
            rows += [
                _case('k_%s_scalar_one' % T, 'dense', 40, 16, 3, 1, 6, 6, w_off=1, opts=o, claims=dict(pl, a_vec=0, two=0, nomask=0),
                      tags=[('kernel', bm, bn, 0, 'table', 'one', 'mask'), ('scalar', 'w_off', bm, bn)], why='w 4 bytes off a 16-byte boundary: scalar A'),
                _case('k_%s_scalar_two' % T, 'dense', 40, 10, 3, 1, 6, 6, C2=6, w_off=1, opts=o, claims=dict(pl, a_vec=0, two=1, nomask=0),
                      tags=[('kernel', bm, bn, 0, 'table', 'two', 'mask')], why='scalar A, two sources'),
                _case('k_%s_k27' % T, 'dense', 40, 3, 3, 1, 6, 6, opts=o, claims=dict(pl, a_vec=0, K=27),
                      tags=[('scalar', 'k4', bm, bn)], why='K = 27, not a multiple of 4: scalar A though w is aligned; a k tail inside a tile'),
            ]
    return rows


NAT = dict(Cout=64, C1=16, KS=3, N=1, H=8, W=8)          # the shape most single-condition rows vary: 64x64 tile by the unforced pick_tile


def _nat(name, **kw):
    a = dict(NAT)
    a.update(kw)
    return _case(name, 'dense', a.pop('Cout'), a.pop('C1'), a.pop('KS'), a.pop('N'), a.pop('H'), a.pop('W'), **a)


T64 = dict(bm=64, bn=64)
CASES = _kernel_rows() + [
    # ---- tiles through the unforced pick_tile, and the downgrade -------------------------------------------------------------
    _case('nat_128', 'dense', 128, 16, 3, 2, 16, 16, opts={'t128_min': 1}, claims=dict(bm=128, bn=128, a_vec=1, splits=1),
          tags=[('natural_tile', 128, 128)], why='M = 128, 512 pixels, t128_min lowered: 128x128 by pick_tile'),
    _case('nat_128_off', 'dense', 128, 16, 3, 2, 16, 16, opts={'t128_min': 1}, w_off=1, claims=dict(bm=64, bn=64, a_vec=0),
          tags=[('downgrade',)], why='the same with w misaligned: the scalar-A kernel exists for the small tiles only, 128x128 -> 64x64'),
    _nat('nat_64', claims=dict(T64, a_vec=1, nomask=0, splits=1, loader=FW_TABLE), tags=[('natural_tile', 64, 64), ('nomask_off', 'zero')],
         why='64x64 by pick_tile; zero padding is all that keeps the mask on'),
    _case('nat_32', 'dense', 8, 16, 3, 1, 8, 8, claims=dict(bm=32, bn=128), tags=[('natural_tile', 32, 128)], why='M <= 32'),
    _case('nat_64x128', 'dense', 64, 16, 3, 1, 8, 16, opts={'tile3_min': 1}, claims=dict(bm=64, bn=128), tags=[('natural_tile', 64, 128)],
          why='tile3_min lowered: the wide tile by pick_tile'),
    # ---- sources ----------------------------------------------------------------------------------------------------------------
    _case('bcast_mask_k4s2', 'dense', 40, 7, 4, 3, 9, 10, stride=2, pad=2, C2=3, bcast=1, claims=dict(two=1, bcast=1, loader=FW_TABLE, nomask=0),
          tags=[('src', 'bcast', 'mask'), ('fixed_off', 'two')], why='second source a row per sample (the discriminators\' class map); 4x4 with two sources: table loader'),
    _nat('bcast_nomask', C1=12, C2=4, bcast=1, reflect=True, claims=dict(T64, two=1, bcast=1, nomask=1), tags=[('src', 'bcast', 'nomask')],
         why='broadcast source under the mask-free loader: its offset must ignore the tap'),
    _case('bcast_1x3_plane', 'dense', 40, 5, 3, 4, 1, 3, C2=3, bcast=1, claims=dict(two=1, bcast=1, nomask=0, a_vec=1, K=72), tags=[('src', 'bcast', 'mask')],
          why='a broadcast row on a 1x3 plane: a tap offset added to it by mistake stays within two floats of the row, so it shows as a value'),
    _case('c2_is_1', 'dense', 40, 7, 3, 2, 5, 5, C2=1, claims=dict(two=1), tags=[('c2', 1)], why='C2 = 1'),
    _case('c1_is_1', 'dense', 40, 1, 3, 2, 5, 5, claims=dict(a_vec=0, K=9), tags=[('c1', 1)], why='C1 = 1: K = 9'),
    # ---- fixed taps ---------------------------------------------------------------------------------------------------------------
    _case('fixed_k1', 'dense', 40, 32, 1, 2, 5, 5, claims=dict(loader=FW_FIXED, K=32), tags=[('fixed', 1)], why='1x1, K = 32'),
    _case('fixed_k4', 'dense', 40, 3, 4, 2, 9, 10, stride=2, pad=1, claims=dict(loader=FW_FIXED, K=48), tags=[('fixed', 4)], why='4x4, 3 channels'),
    _case('fixed_off_k16', 'dense', 40, 20, 1, 2, 5, 5, claims=dict(loader=FW_TABLE, a_vec=1, K=20), tags=[('fixed_off', 'k16')], why='1x1 with K = 20'),
    _case('fixed_off_option', 'dense', 40, 3, 4, 2, 9, 10, stride=2, pad=1, opts={'fixedtap': 0}, claims=dict(loader=FW_TABLE, a_vec=1),
          tags=[('fixed_off', 'option')], why='option fixedtap 0'),
    # ---- each single condition that keeps the mask on (base: nat_64 under reflection = k_64x64_vec_one_nomask) ---------------------
    _nat('mask_ragged_pixels', H=8, W=9, reflect=True, claims=dict(T64, nomask=0, a_vec=1), tags=[('nomask_off', 'pixel')], why='72 pixels'),
    _nat('mask_ragged_m', Cout=40, reflect=True, claims=dict(T64, nomask=0, a_vec=1), tags=[('nomask_off', 'm')], why='M = 40'),
    _nat('mask_k36', C1=4, reflect=True, claims=dict(T64, nomask=0, a_vec=1, K=36), tags=[('nomask_off', 'k16')], why='K = 36'),
    _nat('mask_scalar', reflect=True, w_off=1, claims=dict(T64, nomask=0, a_vec=0), tags=[('nomask_off', 'scalar')], why='w misaligned'),
    # ---- split-K ---------------------------------------------------------------------------------------------------------------------
    _nat('split2_vec', opts={'splits': 2}, claims=dict(T64, splits=2, kchunk=80, reduce=FR_VEC), tags=[('splits', 'vec')], why='two slabs of 80 and 64 k'),
    _nat('split2_y_off', opts={'splits': 2}, y_off=1, claims=dict(splits=2, reduce=FR_SCALAR), tags=[('scalar_reduce', 'y')], why='y misaligned'),
    _nat('split2_ws_off', opts={'splits': 2}, ws_off=1, claims=dict(splits=2, reduce=FR_SCALAR), tags=[('scalar_reduce', 'ws')], why='slabs misaligned'),
    _nat('split2_phw63', H=7, W=9, opts={'splits': 2}, claims=dict(splits=2, reduce=FR_SCALAR), tags=[('scalar_reduce', 'phw')],
         why='OH*OW = 63 (the total 64 * 63 is a multiple of 4)'),
    _nat('split2_odd', Cout=33, H=7, W=9, opts={'splits': 2}, claims=dict(splits=2, reduce=FR_SCALAR), tags=[('scalar_reduce', 'odd'), ('cout', 33)],
         why='33 * 63 outputs: an odd total'),
    _nat('split16_clipped', opts={'splits': 16}, claims=dict(splits=9, kchunk=16, reduce=FR_VEC), tags=[('forced_clipped',)],
         why='16 slabs asked of 9 k-tiles: the plan counts the chunks that exist'),
    _case('split_nat_fixed', 'dense', 64, 128, 4, 1, 16, 16, stride=2, pad=1, claims=dict(T64, K=2048, splits=2, kchunk=1024, loader=FW_FIXED, reduce=FR_VEC),
          tags=[('natural_split', 'fixed'), ('split+fixed',)], why='K = 2048 = split_kmin on one tile: kn_splits asks for 2; fixed taps'),
    _case('split_nat_nomask', 'dense', 64, 256, 3, 1, 8, 8, reflect=True, claims=dict(T64, K=2304, splits=2, kchunk=1152, nomask=1, reduce=FR_VEC),
          tags=[('natural_split', 'nomask'), ('split+nomask',)], why='K = 2304 on one tile, reflect: split with the mask-free loader'),
    _case('split_nat_ktab_only', 'dense', 64, 128, 4, 1, 16, 16, stride=2, pad=1, ws='ktab', claims=dict(K=2048, splits=1, kchunk=2048, reduce=FR_NONE),
          tags=[('split_dropped',)], why='a workspace of the k-table alone: split-K off, the GEMM stores the result itself'),
    # ---- geometry --------------------------------------------------------------------------------------------------------------------
    _case('k7_zero_9x10', 'dense', 40, 3, 7, 2, 9, 10, claims=dict(nomask=0, K=147), tags=[('ks', 7, 'mask'), ('plane', 'nonsquare', 'mask')], why='7x7 zero pad 3'),
    _case('k7_reflect_9x10', 'dense', 40, 3, 7, 2, 9, 10, reflect=True, claims=dict(nomask=0), tags=[('reflect_pad', 3, 'mask')], why='the stem\'s padding, masked'),
    _nat('k7_reflect_nomask', KS=7, reflect=True, claims=dict(T64, nomask=1, K=784), tags=[('ks', 7, 'nomask'), ('reflect_pad', 3, 'nomask')], why='pad 3 mask-free'),
    _nat('k7_reflect_pad_is_H-1', KS=7, N=2, H=4, W=8, reflect=True, claims=dict(T64, nomask=1), tags=[('reflect_pad', 'H-1'), ('plane', 'nonsquare', 'nomask')],
         why='pad 3 on a 4-row plane: the mirror reaches the far edge; mask-free, so a wrong offset is an address'),
    _case('k3_reflect_7x9', 'dense', 40, 16, 3, 1, 7, 9, reflect=True, claims=dict(nomask=0), tags=[('reflect_pad', 1, 'mask'), ('plane', 'odd')], why='odd plane'),
    _nat('k1_reflect_nomask', KS=1, pad=0, reflect=True, opts={'fixedtap': 0}, claims=dict(T64, nomask=1, K=16, loader=FW_TABLE), tags=[('ks', 1, 'nomask')],
         why='1x1 through the table loader (fixedtap 0), reflect flag with pad 0'),
    _nat('k4s2_reflect_nomask', KS=4, C1=4, H=16, W=16, stride=2, pad=1, reflect=True, opts={'fixedtap': 0}, claims=dict(T64, nomask=1, K=64),
         tags=[('ks', 4, 'nomask'), ('stride', 2, 'nomask')], why='4x4 stride 2 under reflection, table loader'),
    _case('k3_pad0', 'dense', 40, 16, 3, 2, 7, 7, pad=0, tags=[('zero_pad', 'p0')], claims=dict(nomask=0), why='no padding'),
    _case('k3_pad3', 'dense', 40, 16, 3, 2, 5, 5, pad=3, tags=[('zero_pad', 'big')], claims=dict(nomask=0), why='pad 3 > KS/2: a 9x9 output of a 5x5 input, whole rows of zeros'),
    _case('up2_zero', 'dense', 40, 16, 3, 1, 4, 5, ups=2, tags=[('ups', 'zero')], claims=dict(nomask=0), why='nearest x2 then zero pad'),
    _nat('up2_reflect', H=4, W=4, ups=2, reflect=True, claims=dict(T64, nomask=1), tags=[('ups', 'reflect')], why='nearest x2 then reflection: the mirror acts on the upsampled axis'),
    _case('up2_k4s2', 'dense', 40, 16, 4, 2, 4, 5, ups=2, stride=2, pad=1, tags=[('ups', 'stride2')], claims=dict(loader=FW_FIXED), why='nearest x2 read with stride 2'),
    _case('straddle_mask', 'dense', 40, 16, 3, 3, 5, 5, tags=[('straddle', 'mask')], claims=dict(T64), why='75 pixels: a 64-pixel tile holds image 0, 1 and 2'),
    _nat('straddle_nomask', N=8, H=4, W=6, reflect=True, claims=dict(T64, nomask=1), tags=[('straddle', 'nomask')], why='8 x 24 pixels = three full tiles across images'),
    _case('plane_1x1', 'dense', 40, 8, 3, 5, 1, 1, tags=[('plane', '1x1')], claims=dict(nomask=0), why='a 1x1 plane: eight of nine taps outside'),
    _case('cout_1', 'dense', 1, 16, 3, 2, 6, 6, tags=[('cout', 1)], claims=dict(bm=32, bn=128), why='one output channel'),
    # ---- epilogue: full 32x32 blocks against edge blocks, per activation -------------------------------------------------------------
    _nat('ep_none_full_nobias', bias=False, claims=dict(T64, splits=1), tags=[('ep', ACT_NONE, 'full'), ('bias', 0, 'full')], why='no bias'),
    _nat('ep_none_full', claims=dict(T64, splits=1), tags=[('bias', 1, 'full')], why='bias'),
    _nat('ep_relu_full', act=ACT_RELU, claims=dict(T64, splits=1), tags=[('ep', ACT_RELU, 'full')], why='ReLU in the full-block code'),
    _nat('ep_leaky_full', act=ACT_LEAKY, claims=dict(T64, splits=1), tags=[('ep', ACT_LEAKY, 'full')], why='LeakyReLU(0.2)'),
    _nat('ep_tanh_full', act=ACT_TANH, claims=dict(T64, splits=1), tags=[('ep', ACT_TANH, 'full')], why='tanh: the general loop even on full blocks'),
    _nat('ep_none_edge_nobias', Cout=40, H=7, W=9, bias=False, claims=dict(T64, splits=1), tags=[('ep', ACT_NONE, 'edge'), ('bias', 0, 'edge')], why='edge blocks'),
    _nat('ep_none_edge', Cout=40, H=7, W=9, claims=dict(T64, splits=1), tags=[('bias', 1, 'edge')], why='edge blocks with bias'),
    _nat('ep_relu_edge', Cout=40, H=7, W=9, act=ACT_RELU, claims=dict(T64, splits=1), tags=[('ep', ACT_RELU, 'edge')], why='ReLU, edge blocks'),
    _nat('ep_leaky_edge', Cout=40, H=7, W=9, act=ACT_LEAKY, claims=dict(T64, splits=1), tags=[('ep', ACT_LEAKY, 'edge')], why='LeakyReLU, edge blocks'),
    _nat('ep_tanh_edge', Cout=40, H=7, W=9, act=ACT_TANH, claims=dict(T64, splits=1), tags=[('ep', ACT_TANH, 'edge')], why='tanh, edge blocks'),
    _nat('ep_leaky_split', act=ACT_LEAKY, opts={'splits': 2}, claims=dict(splits=2, reduce=FR_VEC), tags=[('ep', ACT_LEAKY, 'reduce')],
         why='bias and activation move into the slab reduce: applied once'),
    # ---- the list entries ---------------------------------------------------------------------------------------------------------------
    _case('sp_64x64_k3', 'sparse', 64, 12, 3, 3, 8, 8, L=5, claims=dict(T64, K=48, nomask=0, batched=1, a_vec=1),
          tags=[('list_tile', 64, 64), ('list_nomask', 0), ('list_ragged_k',)], why='L*9 = 45 in a compact K of 48: three zero columns reduced over'),
    _case('sp_32x128_k3', 'sparse', 8, 12, 3, 3, 8, 8, L=5, claims=dict(bm=32, bn=128, K=48), tags=[('list_tile', 32, 128)], why='M = 8'),
    _case('sp_128x128_k3', 'sparse', 40, 12, 3, 3, 8, 8, L=5, opts={'tile': 0}, claims=dict(bm=128, bn=128), tags=[('list_tile', 128, 128)], why='tile forced'),
    _case('pi_64x128_k3', 'perimage', 40, 12, 3, 3, 8, 8, L=5, opts={'tile': 3}, claims=dict(bm=64, bn=128), tags=[('list_tile', 64, 128)], why='tile forced'),
    _case('sp_nomask_k3r', 'sparse', 64, 12, 3, 3, 8, 8, L=5, reflect=True, claims=dict(T64, nomask=1, K=48), tags=[('list_nomask', 1), ('list_ragged_nomask',)],
          why='mask-free with a ragged compact K: the k-table tail must name a VALID tap (Wc is zero there), and an empty image none'),
    _case('pi_stem_k7r', 'perimage', 64, 9, 7, 3, 8, 8, L=4, reflect=True, bias=False, act=ACT_LEAKY, claims=dict(T64, nomask=1, K=208),
          tags=[('list_geom', 'k7r'), ('perimage_nobias',)], why='the factored stem: reflect 7x7, per-image weights, no bias'),
    _case('sp_k3s2', 'sparse', 40, 12, 3, 3, 9, 9, L=5, stride=2, pad=1, act=ACT_LEAKY, claims=dict(nomask=0), tags=[('list_geom', 'k3s2')], why='stride-2 zero-padded 3x3'),
    _case('pi_k4s2', 'perimage', 40, 12, 4, 3, 9, 9, L=5, stride=2, pad=2, act=ACT_LEAKY, claims=dict(nomask=0, K=80), tags=[('list_geom', 'k4s2')],
          why='the discriminators\' factored 4x4 stride 2 pad 2'),
    _case('sp_two', 'sparse', 40, 8, 3, 3, 6, 6, C2=4, L=5, claims=dict(two=1, bcast=0), tags=[('list_second', 'plain')], why='listed channels in the second source'),
    _case('sp_two_bcast', 'sparse', 40, 8, 3, 3, 6, 6, C2=4, bcast=1, L=5, claims=dict(two=1, bcast=1), tags=[('list_second', 'bcast')], why='and in a broadcast second source'),
    # ---- the tail split ---------------------------------------------------------------------------------------------------------------------
    _case('tail_split_300_tiles', 'dense', 200, 32, 3, 3, 40, 40, optsets=[{'w43_tail_split': 2}, {'w43_tail_split': 0}], claims=dict(T64, K=288, splits=1, a_vec=1),
          tags=[('tail_split_row',)],
          why='M = 200: 4 x 75 = 300 tiles of 64x64, 18 k-tiles: on 256 CUs the 44 tiles of the ragged round run as k-pieces at w43_tail_split 2.  The plan '
              'does not report the tail split (it depends on the CU count), so the row cannot assert that it ran: both settings are held to the '
              'bound with c = tail_smax'),
]
BY_NAME = dict((c['name'], c) for c in CASES)
assert len(BY_NAME) == len(CASES)

# the plan classes the table must reach: tests/test_forward_conv_cases_cpu.py compares the union of the rows' claimed tags with this
KERNEL_CLASSES = ([('kernel', bm, bn, 1, ld, src, m) for (bm, bn) in TILES.values()
                   for (ld, src, m) in (('table', 'one', 'mask'), ('table', 'one', 'nomask'), ('table', 'two', 'mask'), ('table', 'two', 'nomask'),
                                        ('fixed', 'one', 'mask'))] +
                  [('kernel', bm, bn, 0, 'table', src, 'mask') for (bm, bn) in ((64, 64), (32, 128), (64, 128)) for src in ('one', 'two')])


def case_desc(case):
    d = make_desc(case['N'], case['C1'], case['H'], case['W'], case['Cout'], case['KS'], case['stride'], case['pad'], case['reflect'],
                  case['ups'], case['OH'], case['OW'], C2=case['C2'])
    d.x2_broadcast = case['bcast']
    return d


def case_option_sets(case):
    """the option dicts the row runs under, one after the other"""
    return [dict(case['opts'], **o) for o in case['optsets']]


def case_ws_bytes(case):
    if case['ws'] == 'ktab':
        return ktab_bytes((case['C1'] + case['C2']) * case['KS'] ** 2)
    return AMPLE


def case_py_plan(case, opts, w_mod16=None, y_mod16=None, ws_mod16=None, ws_bytes=None):
    o = dict((k, v) for k, v in opts.items() if k in OPTION_DEFAULTS)
    return py_plan(ENTRY_OF[case['entry']], case['N'], case['C1'], case['C2'], case['H'], case['W'], case['Cout'], case['KS'], case['stride'],
                   case['pad'], int(case['reflect']), case['ups'], case['OH'], case['OW'], bcast=case['bcast'], L=case['L'],
                   w_mod16=4 * case['w_off'] if w_mod16 is None else w_mod16, y_mod16=4 * case['y_off'] if y_mod16 is None else y_mod16,
                   ws_mod16=4 * case['ws_off'] if ws_mod16 is None else ws_mod16,
                   ws_bytes=case_ws_bytes(case) if ws_bytes is None else ws_bytes, **o)


def case_lists(case):
    """(lists [N, L] int32, cnt [N]) of a list row: image 0 lists L channels, image 1 NONE, the others fewer than L; when there is a
    second source every non-empty list reaches into it; odd images unsorted; the tail of a short list repeats channel 0 (never read)"""
    N, L, C1, C = case['N'], case['L'], case['C1'], case['C1'] + case['C2']
    rng = rng_of(case['shape_key'] + '|lists')
    lists, cnt = np.zeros((N, L), dtype=np.int32), np.zeros(N, dtype=np.int32)
    for b in range(N):
        n = L if b == 0 else (0 if b == 1 else max(1, L - 1 - b % 3))
        ch = [int(c) for c in rng.permutation(C)[:n]]
        if n and case['C2'] and max(ch) < C1:
            ch[0] = C1 + int(rng.randint(0, case['C2']))
        ch = sorted(set(ch))
        while len(ch) < n:                      # (the replacement above can only collide with nothing: max(ch) < C1)
            ch.append(ch[-1] + 1)
        if b % 2 == 1 and n > 1:
            ch = ch[::-1]
        lists[b, :n], cnt[b] = ch, n
    return lists, cnt


_INPUTS, _REFS = {}, {}


def case_inputs(case):
    """deterministic operands of the row's shape (shared by the rows of one shape; never modified).  ReLU / LeakyReLU rows: x > 0 and
    every weight row and its bias of one sign (alternating by output channel), so that every term of a pre-activation has that sign
    and |pre| = sum|w||x| + |bias| stays far from 0 -- or is a structural 0 exactly"""
    k = case['shape_key']
    if k not in _INPUTS:
        rng = rng_of(k)
        N, H, W, M, C, KS = case['N'], case['H'], case['W'], case['Cout'], case['C1'] + case['C2'], case['KS']
        inp = dict(x1=f32(rng, (N, case['C1'], H, W)), x2=None, w=f32(rng, (M, C, KS, KS), 0.5), b=f32(rng, (M,), 0.5) if case['bias'] else None)
        if case['C2']:
            inp['x2'] = f32(rng, (N, case['C2']) if case['bcast'] else (N, case['C2'], H, W))
        if case['entry'] != 'dense':
            inp['lists'], inp['cnt'] = case_lists(case)
        if case['entry'] == 'perimage':
            inp['wimg'] = f32(rng, (N, M, case['L'], KS, KS), 0.5)
        if case['signed']:
            sign = np.where(np.arange(M) % 2 == 0, 1.0, -1.0).astype(np.float32)
            for n in ('x1', 'x2'):
                if inp[n] is not None:
                    inp[n] = np.abs(inp[n]) + np.float32(0.125)
            inp['w'] = np.abs(inp['w']) * sign[:, None, None, None]
            if inp['b'] is not None:
                inp['b'] = (np.abs(inp['b']) + np.float32(0.125)) * sign
            if 'wimg' in inp:
                inp['wimg'] = np.abs(inp['wimg']) * sign[None, :, None, None, None]
        if 'wimg' in inp:
            for b in range(N):
                inp['wimg'][b][:, int(inp['cnt'][b]):] = np.nan        # beyond the image's list: never read
        _INPUTS[k] = inp
    return _INPUTS[k]


def image_weights(case, inp, dtype=np.float64):
    """the weights each image is convolved with, [N or 1, M, C, KS, KS]"""
    C = case['C1'] + case['C2']
    if case['entry'] == 'sparse':
        return list_weights(inp['w'].astype(dtype), inp['lists'], inp['cnt'], C)
    if case['entry'] == 'perimage':
        return perimage_weights(np.nan_to_num(inp['wimg']).astype(dtype), inp['lists'], inp['cnt'], C)
    return inp['w'].astype(dtype)[None]


def restate(case, x, wimg):
    return conv_images(x, wimg, case['KS'], case['stride'], case['pad'], case['reflect'], case['ups'], case['OH'], case['OW'])


def case_x(case, inp, dtype=np.float64):
    return sources(inp['x1'].astype(dtype), None if inp['x2'] is None else inp['x2'].astype(dtype), case['bcast'])


def case_refs(case):
    """float64: pre (the pre-activation), y, sabs = sum|w||x| + |bias| of every output element"""
    k = case['shape_key'] + '|%d' % case['act']
    if k not in _REFS:
        inp = case_inputs(case)
        x, wi = case_x(case, inp), image_weights(case, inp)
        b = np.zeros(case['Cout']) if inp['b'] is None else inp['b'].astype(np.float64)
        pre = restate(case, x, wi) + b[None, :, None, None]
        sabs = restate(case, np.abs(x), np.abs(wi)) + np.abs(b)[None, :, None, None]
        _REFS[k] = dict(pre=pre, y=act_ref(pre, case['act'], case['slope']), sabs=sabs)
    return _REFS[k]


def tiles_of(case, plan):
    n = case['N'] * case['OH'] * case['OW']
    return _cdiv(case['Cout'], plan['bm']) * (case['N'] * _cdiv(case['OH'] * case['OW'], plan['bn']) if plan['batched'] else _cdiv(n, plan['bn']))


def joins(case, plan, tail_smax=TAIL_DEFAULTS['tail_smax']):
    """c of the bound (module docstring)"""
    if plan['splits'] > 1:
        return plan['splits'] - 1
    if not plan['batched'] and tiles_of(case, plan) > N_CU:
        return tail_smax
    return 0


def pre_bound(case, plan):
    return gamma(plan['K'] + 1 + joins(case, plan)) * case_refs(case)['sabs']


def y_bound(case, plan):
    r = case_refs(case)
    b = ACT_LIPSCHITZ[case['act']] * pre_bound(case, plan)
    if case['act'] == ACT_TANH:
        b = b + 1e-6 * np.maximum(1.0, np.abs(r['y']))
    return b


# =============================================================================================
# plan classes: what distinguishes launches as code paths
# =============================================================================================
def plan_classes(case, plan, opts):
    o = dict(OPTION_DEFAULTS)
    o.update((k, v) for k, v in opts.items() if k in OPTION_DEFAULTS)
    M, N, KS, PHW = case['Cout'], case['N'], case['KS'], case['OH'] * case['OW']
    Npix, bm, bn = N * PHW, plan['bm'], plan['bn']
    m = 'nomask' if plan['nomask'] else 'mask'
    src = 'bcast' if plan['bcast'] else ('two' if plan['two'] else 'one')
    out = set()
    if case['entry'] == 'dense':
        K = plan['K']
        vec, fixed = plan['a_vec'] == 1, plan['loader'] == FW_FIXED
        out.add(('kernel', bm, bn, plan['a_vec'], 'fixed' if fixed else 'table', 'two' if plan['two'] else 'one', m))
        out.add(('src', src, m))
        if not vec:
            out.add(('scalar', 'w_off' if K % 4 == 0 else 'k4', bm, bn))
        if o['tile'] < 0:
            out.add(('natural_tile', bm, bn))
        if pick_tile(M, Npix, o) == 0 and bm == 64:
            out.add(('downgrade',))
        if fixed:
            out.add(('fixed', KS))
        elif KS in (1, 4):
            why = [r for r, hit in (('k16', K % BK != 0), ('two', plan['two'] == 1), ('option', o['fixedtap'] == 0), ('scalar', not vec)) if hit]
            if len(why) == 1:
                out.add(('fixed_off', why[0]))
        if not fixed and not plan['nomask']:
            why = [r for r, hit in (('pixel', Npix % bn != 0), ('m', M % bm != 0), ('k16', K % BK != 0 and vec), ('zero', not case['reflect']),
                                    ('scalar', not vec)) if hit]
            if len(why) == 1:
                out.add(('nomask_off', why[0]))
        forced = o['splits'] > 0
        if plan['splits'] > 1:
            out.add(('splits', 'vec' if plan['reduce'] == FR_VEC else 'scalar'))
            if plan['reduce'] == FR_SCALAR:
                why = [r for r, hit in (('y', case['y_off'] != 0), ('ws', case['ws_off'] != 0), ('phw', PHW % 4 != 0)) if hit]
                if len(why) == 1:
                    out.add(('scalar_reduce', 'odd' if (why[0] == 'phw' and (M * Npix) % 2) else why[0]))
            if forced and plan['splits'] < o['splits']:
                out.add(('forced_clipped',))
            if not forced:
                out.add(('natural_split', 'fixed' if fixed else m))
            if fixed:
                out.add(('split+fixed',))
            if plan['nomask']:
                out.add(('split+nomask',))
            if case['act'] != ACT_NONE:
                out.add(('ep', case['act'], 'reduce'))
        else:
            out.add(('splits', 'one'))
            if case['ws'] == 'ktab' and case_py_plan(case, opts, ws_bytes=AMPLE)['splits'] > 1:
                out.add(('split_dropped',))
            blocks = 'full' if (M % bm == 0 and Npix % bn == 0) else 'edge'
            out.add(('ep', case['act'], blocks))
            out.add(('bias', int(case['bias']), blocks))
            if tiles_of(case, plan) > N_CU:
                out.add(('tail_split_row',))
        out.add(('ks', KS, m))
        out.add(('stride', case['stride'], m))
        if case['reflect']:
            out.add(('reflect_pad', case['pad'], m))
            if case['pad'] == min(case['H'], case['W']) * case['ups'] - 1 and case['pad'] > 0:
                out.add(('reflect_pad', 'H-1'))
        else:
            out.add(('zero_pad', 'p0' if case['pad'] == 0 else ('p1' if case['pad'] == 1 else ('big' if case['pad'] > KS // 2 else 'half'))))
        if case['ups'] == 2:
            out.add(('ups', 'stride2' if case['stride'] == 2 else ('reflect' if case['reflect'] else 'zero')))
        if case['OH'] != case['OW']:
            out.add(('plane', 'nonsquare', m))
        if case['OH'] % 2 and case['OW'] % 2 and case['OH'] != case['OW']:
            out.add(('plane', 'odd'))
        if case['H'] == 1 and case['W'] == 1:
            out.add(('plane', '1x1'))
        if N > 1 and bn % PHW != 0 and PHW % bn != 0:
            out.add(('straddle', m))
        out.add(('cout', M))
        out.add(('c1', case['C1']))
        out.add(('c2', case['C2']))
    else:
        lists, cnt = case_lists(case)
        out.add(('list_tile', bm, bn))
        out.add(('list_nomask', plan['nomask']))
        if (case['L'] * KS * KS) % BK:
            out.add(('list_ragged_k',))
            if plan['nomask']:
                out.add(('list_ragged_nomask',))
        if len(set(int(n) for n in cnt)) > 1:
            out.add(('list_unequal',))
        if 0 in cnt:
            out.add(('list_empty_image',))
        if case['L'] in cnt:
            out.add(('list_full_image',))
        if case['C2'] and any(int(c) >= case['C1'] for b in range(N) for c in lists[b][:cnt[b]]):
            out.add(('list_second', 'bcast' if case['bcast'] else 'plain'))
        if not case['reflect'] and case['stride'] == 2 and KS in (3, 4):
            out.add(('list_geom', 'k%ds2' % KS))
        if case['reflect'] and KS == 7:
            out.add(('list_geom', 'k7r'))
        if case['entry'] == 'perimage' and not case['bias']:
            out.add(('perimage_nobias',))
    return out


# =============================================================================================
# one-hot probes: weights that select one (channel, tap) per output channel -- y is a shifted / strided / mirrored / upsampled copy
# =============================================================================================
def _p(name, KS, N, C, H, W, stride=1, pad=None, reflect=False, ups=1, M=None, opts=None, entry='dense', L=0, loader=FW_TABLE, nomask=0):
    pad = (KS - 1) // 2 if pad is None else pad
    M = KS * KS * 2 if M is None else M
    OH, OW = conv_out_size(H * ups, KS, stride, pad), conv_out_size(W * ups, KS, stride, pad)
    return dict(name=name, entry=entry, Cout=M, C1=C, C2=0, KS=KS, N=N, H=H, W=W, stride=stride, pad=pad, reflect=bool(reflect), ups=ups, bcast=0,
                L=L, bias=False, act=ACT_NONE, slope=SLOPE, opts=dict(opts or {}), optsets=[{}], ws='ample', w_off=0, y_off=0, ws_off=0, OH=OH, OW=OW,
                signed=False, claims=dict(loader=loader, nomask=nomask), tags=(), why='',
                shape_key='probe|%s' % name)


PROBES = [
    _p('p_k1', 1, 2, 20, 5, 6, M=20),
    _p('p_k1_fixed', 1, 2, 16, 5, 6, M=16, loader=FW_FIXED),
    _p('p_k3_zero', 3, 2, 4, 5, 6),
    _p('p_k3_zero_s2', 3, 2, 4, 7, 8, stride=2),
    _p('p_k3_reflect', 3, 2, 4, 5, 6, reflect=True),
    _p('p_k3_reflect_nomask', 3, 1, 16, 8, 8, reflect=True, M=64, nomask=1),
    _p('p_k3_up2_zero', 3, 2, 4, 3, 4, ups=2),
    _p('p_k3_up2_reflect_nomask', 3, 1, 16, 4, 4, ups=2, reflect=True, M=64, nomask=1),
    _p('p_k4_s2_fixed', 4, 2, 4, 8, 10, stride=2, pad=1, loader=FW_FIXED),
    _p('p_k4_s2_table', 4, 2, 4, 8, 10, stride=2, pad=1, opts={'fixedtap': 0}),
    _p('p_k4_s1_pad2', 4, 2, 4, 5, 6, stride=1, pad=2, loader=FW_FIXED),
    _p('p_k4_s2_reflect_nomask', 4, 1, 4, 16, 16, stride=2, pad=1, reflect=True, M=64, opts={'fixedtap': 0}, nomask=1),
    _p('p_k4_up2_s2_fixed', 4, 2, 4, 4, 5, ups=2, stride=2, pad=1, loader=FW_FIXED),
    _p('p_k7_zero', 7, 2, 3, 9, 10),
    _p('p_k7_reflect', 7, 2, 3, 9, 10, reflect=True),
    _p('p_k7_reflect_pad_is_H-1_nomask', 7, 2, 16, 4, 8, reflect=True, M=64, nomask=1),
    _p('p_k7_s2_zero', 7, 2, 3, 9, 10, stride=2),
    _p('p_list_k3', 3, 3, 12, 6, 6, entry='perimage', L=5),
    _p('p_list_k3_reflect_nomask', 3, 3, 12, 8, 8, entry='perimage', L=5, reflect=True, M=64, nomask=1),
    _p('p_list_k4_s2', 4, 3, 12, 9, 9, stride=2, pad=2, entry='perimage', L=5),
    _p('p_list_k7_reflect', 7, 3, 9, 8, 8, entry='perimage', L=4, reflect=True),
    _p('p_sparse_k3', 3, 3, 12, 6, 6, entry='sparse', L=5),
]


def probe_selection(case):
    """[(c or list position j, kh, kw)] per output channel m: every tap at least once, the channels / positions in rotation"""
    KS, n = case['KS'], (case['L'] if case['entry'] == 'perimage' else case['C1'])
    return [((m * 5 + m // (KS * KS)) % n, (m % (KS * KS)) // KS, m % KS) for m in range(case['Cout'])]


def probe_inputs(case):
    """x random fp32; the weights one-hot per output channel (probe_selection)"""
    rng = rng_of(case['shape_key'])
    N, M, KS = case['N'], case['Cout'], case['KS']
    inp = dict(x1=f32(rng, (N, case['C1'], case['H'], case['W'])), x2=None, b=None)
    sel = probe_selection(case)
    if case['entry'] != 'dense':
        inp['lists'], inp['cnt'] = case_lists(case)
    if case['entry'] == 'perimage':
        w = np.zeros((N, M, case['L'], KS, KS), dtype=np.float32)
        for m, (j, kh, kw) in enumerate(sel):
            w[:, m, j, kh, kw] = 1.0
        inp['wimg'] = w
    else:
        w = np.zeros((M, case['C1'], KS, KS), dtype=np.float32)
        for m, (c, kh, kw) in enumerate(sel):
            w[m, c, kh, kw] = 1.0
    inp['w'] = w if case['entry'] != 'perimage' else None
    return inp


def probe_restated(case, inp):
    """the restatement in float32 on the probe's operands"""
    if case['entry'] == 'perimage':
        wi = perimage_weights(inp['wimg'], inp['lists'], inp['cnt'], case['C1'])
    elif case['entry'] == 'sparse':
        wi = list_weights(inp['w'], inp['lists'], inp['cnt'], case['C1'])
    else:
        wi = inp['w'][None]
    y = restate(case, inp['x1'], wi)
    assert y.dtype == np.float32
    return y


def probe_placement(case, inp):
    """what the probe claims, by index arithmetic alone: y[n, m, oh, ow] = x[n, c_m, l_h // ups, l_w // ups] with l = o*s - p + k mirrored
    into the logical plane under reflection, 0 outside it under zero padding; for a list entry c_m = list[n][j_m] if j_m < cnt[n] (per-image)
    or c_m itself if image n lists it (sparse), else 0"""
    N, M, KS, s, p, ups = case['N'], case['Cout'], case['KS'], case['stride'], case['pad'], case['ups']
    LH, LW = case['H'] * ups, case['W'] * ups
    y = np.zeros((N, M, case['OH'], case['OW']), dtype=np.float32)
    for n in range(N):
        for m, (c, kh, kw) in enumerate(probe_selection(case)):
            if case['entry'] == 'perimage':
                if c >= inp['cnt'][n]:
                    continue
                c = int(inp['lists'][n][c])
            elif case['entry'] == 'sparse' and c not in [int(v) for v in inp['lists'][n][:inp['cnt'][n]]]:
                continue
            for oh in range(case['OH']):
                for ow in range(case['OW']):
                    lh, lw = oh * s - p + kh, ow * s - p + kw
                    if case['reflect']:
                        lh, lw = _reflect(lh, LH), _reflect(lw, LW)
                    if 0 <= lh < LH and 0 <= lw < LW:
                        y[n, m, oh, ow] = inp['x1'][n, c, lh // ups, lw // ups]
    return y
