"""Case table, input builders, float64 references and rounding bounds of the transposed-gather convolution tests: the entry points
sg_convT2d_fwd / _dgrad / _wgrad, sg_conv2d_dgrad, sg_conv2d_dgrad_folded and the sub-pixel form (sg_upconv3_fold_weights,
sg_upconv3_unfold_wgrad) of csrc/igemm.hip, which launch the parity-class and plain transposed gathers of csrc/igemm_kn1.hip.
Shared by tests/test_transposed_conv_cases_cpu.py (the references agree with an independent formulation, the adjoint pairs are
adjoint, the table reaches every launch plan) and tests/test_gpu_transposed_conv.py (every case against float64 on the device).

NumPy only.  The references restate the index formulas of the comments in csrc/igemm.hip tap by tap; they are dtype-generic, so the
one-hot probes evaluate them in float32, where a single product (plus one bias add) is exact.

The launch plans come from the library's own host-side query (include/sg2im_hip.h: sg_conv2d_tgather_plan) -- the functions the
launchers plan with -- so a table entry names a route by shape, channel window and workspace alignment alone.

Bounds.  Every output is an fp32 fma chain over its n terms (terms that are structurally zero -- a tap outside the plane, the
padding rows of a k-tile -- add 0 exactly), joined by at most c further adds:  |got - ref64| <= gamma(n + c) (sum|a||b| + |bias|),
gamma from dense_pointwise_cases, n = the number of terms of THAT output (the restatement run on ones), sum|a||b| the restatement
run on absolute values.  c per entry point, from the code:
  C_GATHER = 8   sg_convT2d_fwd, sg_conv2d_dgrad, sg_conv2d_dgrad_folded, sg_convT2d_dgrad (conv-shaped GEMM launches): the partial
                 sums of one output meet in at most 8 pieces = 7 adds -- split-K slabs (igemm_core.h kn_splits: ``if (sp > 8) sp = 8``;
                 the table forces at most 8), or the two halves of a parity split (split_schedule: ``bi.par.split[c] = sp2 ? 2 : 1``), or
                 tail-split pieces (split_schedule: ``smax = ... > 8 ? 8``); the three exclude each other (``splits <= 1`` in both
                 conditions) -- plus the bias add of the epilogue.
  c_wgrad(Kpix)  sg_convT2d_wgrad: the k range N*H*W is cut into chunks that are multiples of 64 (igemm_nk.hip: ``kchunk = ...
                 sg_cdiv(sg_cdiv(Kpix, splits), 64) * 64``), so at most ceil(Kpix / 64) slabs meet; the bias gradient is a plain sum of
                 n = N*OH*OW terms (row sums per chunk or sg_channel_sum: n - 1 adds in any order).
  C_VARIANT = 3  sg_conv2d_dgrad_folded: each gathered value is a pre-folded sum of up to four gy (reflect_variants_kernel: v00 + three
                 conditional adds) -- three more roundings on a term.
  C_FOLD = 3     sub-pixel form: a folded weight is the sum of up to four taps (upconv3_fold_kernel), the unfolded gradient the sum
                 of four (upconv3_unfold_kernel) -- three more roundings.
sg_pad_upsample_bwd behind a dgrad on the logical grid adds the m values that fold onto one pixel: m more roundings at most.
"""
import ctypes

import numpy as np

from scene_generation_amd._hip import CONST, plan_dict, sgTGatherPlan

from dense_pointwise_cases import gamma, rng_of, f32, option  # noqa: F401  (re-exported)

BK = 16                 # igemm_core.h: sub-tile depth; the fixed-tap loaders need K % BK == 0 in every class
KS_VALUES = (1, 3, 4, 7)
C_GATHER = 8
C_VARIANT = 3
C_FOLD = 3
WGRAD_CHUNK = 64


def c_wgrad(kpix):
    return -(-kpix // WGRAD_CHUNK)


# include/sg2im_hip.h, under the short names the tables use
TG_CONVT_FWD, TG_CONV_DGRAD, TG_DGRAD_FOLDED = (CONST['SG_TG_' + n] for n in ('CONVT_FWD', 'CONV_DGRAD', 'DGRAD_FOLDED'))
TG_PLAIN, TG_PARITY = CONST['SG_TG_PLAIN'], CONST['SG_TG_PARITY']
TG_TABLE, TG_FIXED = CONST['SG_TG_TABLE'], CONST['SG_TG_FIXED']
ENTRY_NAMES = {TG_CONVT_FWD: 'convT_fwd', TG_CONV_DGRAD: 'conv_dgrad', TG_DGRAD_FOLDED: 'dgrad_folded'}
PAR_SPLIT_VALUES = (1, 0)        # option par_split: every parity case runs under both
TAIL_SPLIT_VALUES = (0, 2)       # option w43_tail_split: every stride-1 case runs under both


def make_desc(N, C1, H, W, Cout, KS, stride, pad, reflect, ups, OH, OW, out_pad=0, C2=0):
    from scene_generation_amd._hip import sgConvDesc
    return sgConvDesc(N=N, C1=C1, C2=C2, H=H, W=W, Cout=Cout, KS=KS, stride=stride, pad=pad, pad_reflect=int(reflect),
                      upsample=ups, OH=OH, OW=OW, out_pad=out_pad, x2_broadcast=0)


def tgather_plan(lib, desc, entry, c0, c1, ws_mod16=0, ws_bytes=0):
    """sg_conv2d_tgather_plan under the current options -> dict (per-class lists cut to ncls)"""
    p = sgTGatherPlan()
    rc = lib.sg_conv2d_tgather_plan(ctypes.byref(desc), int(entry), int(c0), int(c1), int(ws_mod16), int(ws_bytes), ctypes.byref(p))
    assert rc == 0, lib.sg_last_error_string().decode()
    out = plan_dict(p)
    out['tile'] = (out.pop('bm'), out.pop('bn'))
    for n in ('taps', 'PH', 'PW', 'ph0', 'pw0', 'K'):
        out[n] = out[n][:p.ncls]
    return out


# =============================================================================================
# float64 (dtype-generic) restatements, tap by tap
# =============================================================================================
def _pairs(n_small, n_big, s, p, k):
    """index pairs (i, o) with o = i * s - p + k inside [0, n_big): tap k links position i of the strided (small) axis with position
    o of the dense (big) axis"""
    i = [j for j in range(n_small) if 0 <= j * s - p + k < n_big]
    return i, [j * s - p + k for j in i]


def convT_out_size(n, KS, s, p, op):
    return (n - 1) * s - 2 * p + KS + op


def conv_out_size(n, KS, s, p):
    return (n + 2 * p - KS) // s + 1


def convT_fwd(x, w, b, s, p, op):
    """y[n,co,oh,ow] = b[co] + sum_{ci,kh,kw} w[ci,co,kh,kw] x[n,ci,(oh+p-kh)/s,(ow+p-kw)/s]     x [N,Ci,H,W], w [Ci,Co,KS,KS]"""
    N, Ci, H, W = x.shape
    Co, KS = w.shape[1], w.shape[2]
    OH, OW = convT_out_size(H, KS, s, p, op), convT_out_size(W, KS, s, p, op)
    y = np.zeros((N, Co, OH, OW), dtype=x.dtype)
    for kh in range(KS):
        ih, oh = _pairs(H, OH, s, p, kh)
        for kw in range(KS):
            iw, ow = _pairs(W, OW, s, p, kw)
            if ih and iw:
                y[np.ix_(range(N), range(Co), oh, ow)] += np.einsum('nchw,cd->ndhw', x[np.ix_(range(N), range(Ci), ih, iw)], w[:, :, kh, kw])
    if b is not None:
        y += b.astype(x.dtype)[None, :, None, None]
    return y


def convT_dgrad(gy, w, s, p, H, W):
    """gx[n,ci,ih,iw] = sum_{co,kh,kw} w[ci,co,kh,kw] gy[n,co,ih*s-p+kh,iw*s-p+kw]"""
    N, Co, OH, OW = gy.shape
    Ci, KS = w.shape[0], w.shape[2]
    gx = np.zeros((N, Ci, H, W), dtype=gy.dtype)
    for kh in range(KS):
        ih, oh = _pairs(H, OH, s, p, kh)
        for kw in range(KS):
            iw, ow = _pairs(W, OW, s, p, kw)
            if ih and iw:
                gx[np.ix_(range(N), range(Ci), ih, iw)] += np.einsum('ndhw,cd->nchw', gy[np.ix_(range(N), range(Co), oh, ow)], w[:, :, kh, kw])
    return gx


def convT_wgrad(gy, x, KS, s, p):
    """gw[ci,co,kh,kw] = sum_{n,ih,iw} x[n,ci,ih,iw] gy[n,co,ih*s-p+kh,iw*s-p+kw]"""
    N, Ci, H, W = x.shape
    Co, OH, OW = gy.shape[1:]
    gw = np.zeros((Ci, Co, KS, KS), dtype=x.dtype)
    for kh in range(KS):
        ih, oh = _pairs(H, OH, s, p, kh)
        for kw in range(KS):
            iw, ow = _pairs(W, OW, s, p, kw)
            if ih and iw:
                gw[:, :, kh, kw] = np.einsum('nchw,ndhw->cd', x[np.ix_(range(N), range(Ci), ih, iw)], gy[np.ix_(range(N), range(Co), oh, ow)])
    return gw


def bias_grad(gy):
    return gy.sum(axis=(0, 2, 3))


def conv_dgrad_logical(gy, w, s, p, GH, GW, c0, c1):
    """Gradient of y[n,co,oh,ow] = sum w[co,c,kh,kw] xl[n,c,oh*s-p+kh,ow*s-p+kw] w.r.t. channels [c0, c1) of the logical GH x GW grid xl:
    gxl[n,c,gh,gw] = sum_{co,kh,kw} w[co,c,kh,kw] gy[n,co,(gh+p-kh)/s,(gw+p-kw)/s]     w [Co,C,KS,KS]; p = 0 on a reflect-padded grid"""
    N, Co, OH, OW = gy.shape
    KS = w.shape[2]
    g = np.zeros((N, c1 - c0, GH, GW), dtype=gy.dtype)
    for kh in range(KS):
        oh, gh = _pairs(OH, GH, s, p, kh)
        for kw in range(KS):
            ow, gw = _pairs(OW, GW, s, p, kw)
            if oh and ow:
                g[np.ix_(range(N), range(c1 - c0), gh, gw)] += np.einsum('ndhw,dc->nchw', gy[np.ix_(range(N), range(Co), oh, ow)],
                                                                          w[:, c0:c1, kh, kw])
    return g


def _reflect(i, L):
    i = -i if i < 0 else i
    return 2 * L - 2 - i if i >= L else i


def fold_pad_upsample(gp, H, W, pad, ups):
    """adjoint of reflect_pad(pad) o nearest_upsample(ups): gx[.., reflect(ph - pad) // ups, reflect(pw - pad) // ups] += gp[.., ph, pw]"""
    LH, LW = H * ups, W * ups
    assert gp.shape[-2:] == (LH + 2 * pad, LW + 2 * pad)
    ih = np.array([_reflect(ph - pad, LH) // ups for ph in range(LH + 2 * pad)])
    iw = np.array([_reflect(pw - pad, LW) // ups for pw in range(LW + 2 * pad)])
    gx = np.zeros(gp.shape[:-2] + (H, W), dtype=gp.dtype)
    np.add.at(gx, (Ellipsis, ih[:, None], iw[None, :]), gp)
    return gx


def conv_dgrad_folded(gy, w, H, W, c0, c1):
    """ReflectionPad2d(1) + 3x3 stride-1 conv, gradient w.r.t. channels [c0, c1) of the ACTUAL H x W input: the gradient of the padded
    (H + 2) x (W + 2) grid with every padded position added onto the pixel it mirrors"""
    return fold_pad_upsample(conv_dgrad_logical(gy, w, 1, 0, H + 2, W + 2, c0, c1), H, W, 1, 1)


_FOLD_R = ((2,), (1, 2), (0, 1), (0,))      # include/sg2im_hip.h: R(kh), the 3x3 taps that land on transposed-conv tap kh


def upconv3_fold(w):
    """wt[ci][co][kh][kw] = sum_{i in R(kh)} sum_{j in R(kw)} w[co][ci][i][j]; added in the kernel's order (i outer, j inner, from 0)"""
    Co, Ci = w.shape[:2]
    wt = np.zeros((Ci, Co, 4, 4), dtype=w.dtype)
    for kh in range(4):
        for kw in range(4):
            for i in _FOLD_R[kh]:
                for j in _FOLD_R[kw]:
                    wt[:, :, kh, kw] = wt[:, :, kh, kw] + w[:, :, i, j].T
    return wt


def upconv3_unfold(gwt):
    """gw[co][ci][i][j] = sum_{kh: i in R(kh)} sum_{kw: j in R(kw)} gwt[ci][co][kh][kw]; the kernel's order (a + b) + (c + d)"""
    Ci, Co = gwt.shape[:2]
    gw = np.zeros((Co, Ci, 3, 3), dtype=gwt.dtype)
    for i in range(3):
        khs = [kh for kh in range(4) if i in _FOLD_R[kh]]
        for j in range(3):
            kws = [kw for kw in range(4) if j in _FOLD_R[kw]]
            rows = [gwt[:, :, kh, kws[0]] + gwt[:, :, kh, kws[1]] for kh in khs]
            gw[:, :, i, j] = (rows[0] + rows[1]).T
    return gw


def nearest_up2(x):
    return np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)


def conv_fwd(x, w, s, p):
    """plain zero-padded conv (only to state what the sub-pixel form must equal): y[n,co,oh,ow] = sum w[co,c,kh,kw] x[n,c,oh*s-p+kh,..]"""
    N, C, H, W = x.shape
    Co, KS = w.shape[0], w.shape[2]
    OH, OW = conv_out_size(H, KS, s, p), conv_out_size(W, KS, s, p)
    y = np.zeros((N, Co, OH, OW), dtype=x.dtype)
    for kh in range(KS):
        oh, ih = _pairs(OH, H, s, p, kh)
        for kw in range(KS):
            ow, iw = _pairs(OW, W, s, p, kw)
            if oh and ow:
                y[np.ix_(range(N), range(Co), oh, ow)] += np.einsum('nchw,dc->ndhw', x[np.ix_(range(N), range(C), ih, iw)], w[:, :, kh, kw])
    return y


def bound(terms, c, sabs):
    """gamma(n + c) sum|a||b| element by element"""
    return gamma(np.asarray(terms, dtype=np.float64) + c) * np.asarray(sabs, dtype=np.float64)


# =============================================================================================
# class geometry of the parity route, restated independently of csrc/igemm_kn1.hip
# =============================================================================================
def parity_classes(KS, PH, PW, pad):
    """[(taps, PHa, PWb, ph0, pw0)] of the non-empty classes in launch order (a, b) = (0,0), (0,1), (1,0), (1,1).  Pixel (ph, pw) of
    the plane only receives taps kh = ph + pad, kw = pw + pad (mod 2): class (a, b) owns the pixels ph = a - pad, pw = b - pad (mod 2)"""
    out = []
    for a in (0, 1):
        for b in (0, 1):
            taps = [kh * KS + kw for kh in range(KS) if kh % 2 == a for kw in range(KS) if kw % 2 == b]
            rows = [ph for ph in range(PH) if (ph + pad - a) % 2 == 0]
            cols = [pw for pw in range(PW) if (pw + pad - b) % 2 == 0]
            if taps and rows and cols:
                out.append((taps, len(rows), len(cols), rows[0], cols[0]))
    return out


def expected_plan(entry, N, Cin, Cout, H, W, KS, stride, pad, reflect, ups, out_pad, c0, c1, ws_mod16=0):
    """the plan fields that follow from the shape alone (route, classes, loader kind, A read width); tile and split-K are claimed by
    the table rows that are there for them.  Assumes the default option fixedtap."""
    R = KS * KS
    if entry == TG_CONVT_FWD:
        Rdim, M, PH, PW, p = Cin, Cout, convT_out_size(H, KS, stride, pad, out_pad), convT_out_size(W, KS, stride, pad, out_pad), pad
        a_off = 0
    elif entry == TG_CONV_DGRAD:
        Rdim, M = Cout, c1 - c0
        PH, PW = H * ups + (2 * pad if reflect else 0), W * ups + (2 * pad if reflect else 0)
        p, a_off = (0 if reflect else pad), c0 * Cout * R
    else:
        Rdim, M, PH, PW, p, a_off = Cout, c1 - c0, H, W, 1, c0 * Cout * R
    if entry != TG_DGRAD_FOLDED and stride == 2 and KS >= 3:
        cls = parity_classes(KS, PH, PW, p)
        K = tuple(Rdim * len(t[0]) for t in cls)
        vec = ws_mod16 == 0 and all(k % 4 == 0 for k in K)
        fixed = KS <= 4 and all(k % BK == 0 for k in K) and vec
        return dict(route=TG_PARITY, ncls=len(cls), taps=tuple(len(t[0]) for t in cls), PH=tuple(t[1] for t in cls),
                    PW=tuple(t[2] for t in cls), ph0=tuple(t[3] for t in cls), pw0=tuple(t[4] for t in cls), K=K,
                    loader=TG_FIXED if fixed else TG_TABLE, a_vec=int(vec), M=M)
    K = Rdim * R
    vec = K % 4 == 0 and (ws_mod16 + 4 * a_off) % 16 == 0
    fixed = KS in (1, 4) and vec and K % BK == 0 and entry != TG_DGRAD_FOLDED
    return dict(route=TG_PLAIN, ncls=1, taps=(R,), PH=(PH,), PW=(PW,), ph0=(0,), pw0=(0,), K=(K,),
                loader=TG_FIXED if fixed else TG_TABLE, a_vec=int(vec), M=M)


def plan_classes(entry, KS, plan, forced=False):
    """what distinguishes launches as code paths and as index arithmetic: the kernel instantiation (route, kernel size, loader kind, A
    read width, per-tap source copies of the folded form), the number of classes, each class's tap count, the tile, split-K.  Under
    forced options only the tile and split-K count (the options exist to reach those at small shapes)."""
    out = {('tile', plan['route'], plan['tile'])}
    if plan['splits'] > 1:
        out.add(('splits>1', ENTRY_NAMES[entry]))
    if not forced:
        out.add(('path', plan['route'], KS, plan['loader'], plan['a_vec'], entry == TG_DGRAD_FOLDED))
        out.add(('ncls', plan['ncls']))
        out |= {('taps', t) for t in plan['taps']}
    return out


# =============================================================================================
# the case table
# =============================================================================================
def _case(kind, name, N, Cin, Cout, H, W, KS, stride, pad, out_pad=0, bias=True, reflect=False, ups=1, window=None, opts=None,
          claims=None, ws_off=0, why=''):
    """kind: 'convT' (Cin -> Cout transposed conv: forward, data, weight and bias gradient), 'dgrad' (data gradient of a Cin -> Cout
    conv on the logical grid, channel window), 'folded', 'subpixel'.  opts: library options forced for the case; claims: plan fields
    (tile, splits) the row is there for; ws_off: floats the workspace is offset from a 16-byte boundary"""
    return dict(kind=kind, name=name, N=N, Cin=Cin, Cout=Cout, H=H, W=W, KS=KS, stride=stride, pad=pad, out_pad=out_pad, bias=bias,
                reflect=reflect, ups=ups, window=window or (0, Cin), opts=dict(opts or {}), claims=dict(claims or {}),
                ws_off=ws_off, why=why)


def convT_valid(H, W, KS, s, p, op):
    return convT_out_size(H, KS, s, p, op) > 0 and convT_out_size(W, KS, s, p, op) > 0


def _build_convT_cases():
    cases = []
    planes = ((5, 7), (1, 1), (1, 5), (3, 4), (7, 5), (2, 9))
    chans = ((16, 16), (5, 3), (6, 10), (8, 40))       # K % 16 == 0 in every class; neither % 4 nor % 16; % 4 only in some; M > 32
    i = 0
    for KS in KS_VALUES:
        for s in (1, 2):
            for p in (0, 1, 2):
                if p > KS - 1:
                    continue
                for op in ((0, 1) if s == 2 else (0,)):
                    j = i
                    while not convT_valid(*planes[j % len(planes)], KS, s, p, op):
                        j += 1
                    H, W = planes[j % len(planes)]
                    Ci, Co = chans[i % len(chans)]
                    cases.append(_case('convT', 'convT_k%ds%dp%dop%d_%dx%d_%dto%d' % (KS, s, p, op, H, W, Ci, Co), 1 + i % 3, Ci, Co,
                                       H, W, KS, s, p, op, bias=i % 2 == 0, why='kernel size x stride x pad x output padding'))
                    i += 1
    cases += [
        _case('convT', 'convT_k7s2p3_16to16', 2, 16, 16, 5, 7, 7, 2, 3, 1, why='classes of 16 / 12 / 12 / 9 taps, K % 16 == 0 in each: the '
              'table loader all the same (lg = -1), the 16-tap class fills TapList'),
        _case('convT', 'convT_k7s2p0_5to3_1x1', 3, 5, 3, 1, 1, 7, 2, 0, 0, bias=False, why='1x1 plane, 7x7 output: every pixel one tap'),
        _case('convT', 'convT_k3s2p1op0_1x1', 2, 6, 10, 1, 1, 3, 2, 1, 0, why='1x1 plane, 1x1 output: one class of four'),
        _case('convT', 'convT_k3s2p1op0_1x5', 2, 16, 16, 1, 5, 3, 2, 1, 0, bias=False, why='1x9 output: two classes, the row classes empty'),
        _case('convT', 'convT_k4s2p1_1x5', 2, 16, 16, 1, 5, 4, 2, 1, 0, why='2x10 output from one input row'),
        _case('convT', 'convT_k3s2p1op1_16to40', 2, 16, 40, 5, 7, 3, 2, 1, 1, why='M > 32 on the parity route, fixed-tap loaders'),
        _case('convT', 'convT_k4s2p1_16to16', 2, 16, 16, 7, 5, 4, 2, 1, 0, bias=False, why='four classes of four taps, fixed-tap loaders'),
        _case('convT', 'convT_k4s2p1_8to40_off', 2, 8, 40, 5, 7, 4, 2, 1, 0, ws_off=1, why='workspace 4 bytes off: scalar A, table loaders'),
        _case('convT', 'convT_k4s1p1_16to16', 2, 16, 16, 5, 7, 4, 1, 1, why='stride 1, 4x4: kn1_run with the fixed-tap loader'),
        _case('convT', 'convT_k1s1_16to40', 2, 16, 40, 5, 7, 1, 1, 0, why='1x1 stride 1, fixed-tap loader, M > 32'),
        _case('convT', 'convT_k1s1_8to40', 3, 8, 40, 3, 4, 1, 1, 0, bias=False, why='K = 8: float4 A but no whole k-tile, the table loader at 1x1'),
        _case('convT', 'convT_k4s1p1_16to16_off', 2, 16, 16, 3, 4, 4, 1, 1, ws_off=1, why='4x4 stride 1 with the weights 4 bytes off: scalar A, table loader'),
        _case('convT', 'convT_k1s2op1_16to16', 2, 16, 16, 5, 7, 1, 2, 0, 1, bias=False, why='1x1 stride 2: plain route, three of four pixels bias only'),
        _case('convT', 'convT_k3s1p1_16to16_off', 2, 16, 16, 5, 7, 3, 1, 1, ws_off=2, why='K % 4 == 0 but the weights 8 bytes off: scalar A'),
        _case('convT', 'convT_k3s1p1_16to48_4x17x19', 4, 16, 48, 17, 19, 3, 1, 1, why='largest plane of the table, more than one pixel tile per row tile'),
        # ---- routes that shape alone does not reach at these sizes: forced through the options, asserted through the query
        _case('convT', 'route_splitk_plain', 2, 32, 16, 5, 7, 3, 1, 1, opts={'splits': 4}, claims={'splits': 4},
              why='split-K: four slabs + slab_reduce_nchw_kernel (70 pixels: the scalar reduce)'),
        _case('convT', 'route_splitk_plain_vecreduce', 2, 64, 16, 4, 8, 3, 1, 1, opts={'splits': 8}, claims={'splits': 8},
              why='split-K, eight slabs, 32-pixel planes: slab_reduce_nchw_vec_kernel'),
        _case('convT', 'route_tile128_plain', 2, 16, 48, 9, 9, 3, 1, 1, opts={'tile': 0}, claims={'tile': (128, 128)},
              why='128x128 tiles, ragged in both directions'),
        _case('convT', 'route_tile64x128_plain', 2, 16, 48, 9, 9, 4, 1, 1, opts={'tile': 3}, claims={'tile': (64, 128)}, why='64x128 tiles'),
        _case('convT', 'route_tile64x128_parity', 2, 16, 72, 9, 9, 3, 2, 1, 1, opts={'tile': 3}, claims={'tile': (64, 128)},
              why='64x128 tiles, parity classes: two row tiles, per-class pixel tiles'),
        _case('convT', 'route_tile64_parity_m64', 2, 64, 64, 5, 7, 3, 2, 1, 1, opts={'tile': 1}, claims={'tile': (64, 64)},
              why='M a whole 64-row tile, K = 256 / 128 / 128 / 64: the parity split is admitted (M % BM == 0, halves of 8 k-tiles)'),
    ]
    return cases


def conv_valid(H, W, KS, s, p, reflect=False, ups=1):
    return conv_out_size(H * ups, KS, s, p) > 0 and conv_out_size(W * ups, KS, s, p) > 0 and (not reflect or p < min(H, W) * ups)


def _windows(C):
    """[0, C), [c, C) with c odd, [0, c), one channel"""
    odd = 1 if C < 4 else 3
    return ((0, C), (odd, C), (0, max(1, C - 2)), (C // 2, C // 2 + 1))


def _build_dgrad_cases():
    cases = []
    planes = ((15, 17), (3, 3), (1, 9), (5, 7), (9, 6), (7, 1))
    chans = ((6, 10), (16, 16), (5, 3), (7, 8), (40, 12))        # (conv input channels C, Cout)
    i = 0
    for s in (2, 1):
        for KS in ((3, 4, 7) if s == 2 else KS_VALUES):
            for p in (0, 1, 2, 3):
                if p > KS - 1 or (p == 3 and KS != 7):
                    continue
                j = i
                while not conv_valid(*planes[j % len(planes)], KS, s, p):
                    j += 1
                H, W = planes[j % len(planes)]
                C, Co = chans[i % len(chans)]
                win = _windows(C)[i % 4]
                cases.append(_case('dgrad', 'dgrad_k%ds%dp%d_%dx%d_%dto%d_w%d_%d' % (KS, s, p, H, W, C, Co, win[0], win[1]), 1 + i % 3, C, Co,
                                   H, W, KS, s, p, window=win, why='stride x kernel size x pad x plane x window'))
                i += 1
    for k, (C, Co, KS, s, p, H, W) in enumerate(((6, 10, 3, 2, 1, 15, 17), (16, 16, 4, 2, 1, 9, 6), (5, 3, 7, 2, 3, 5, 7), (16, 16, 3, 1, 1, 5, 7),
                                                  (5, 3, 3, 1, 1, 5, 7), (7, 5, 1, 1, 0, 5, 7), (6, 16, 4, 1, 2, 5, 7), (4, 4, 7, 1, 3, 3, 3))):
        for win in _windows(C):          # every window form on one shape per loader / route kind
            cases.append(_case('dgrad', 'dgrad_win_k%ds%d_%dto%d_w%d_%d' % (KS, s, C, Co, win[0], win[1]), 2, C, Co, H, W, KS, s, p, window=win,
                               why='channel window: m0 of permute_sub_kernel / the offset weight pointer of kn1_run'))
    cases += [
        _case('dgrad', 'dgrad_k3s2p1_1x9', 2, 6, 10, 1, 9, 3, 2, 1, window=(1, 6), why='one-row plane: the odd-row classes are empty'),
        _case('dgrad', 'dgrad_k4s2p2_9x1', 2, 16, 16, 9, 1, 4, 2, 2, window=(3, 16), why='one-column plane, fixed-tap loaders, two classes'),
        _case('dgrad', 'dgrad_k7s2p3_3x3', 3, 5, 3, 3, 3, 7, 2, 3, window=(0, 5), why='3x3 plane under a 7x7 kernel: most taps outside'),
        _case('dgrad', 'dgrad_k3s2p1_64to64_m64', 2, 64, 64, 9, 9, 3, 2, 1, claims={'tile': (64, 64)},
              why='M = 64 rows of K = 256 / 128 / 128 / 64: the 4-tap class runs as two halves when the option par_split is on'),
        _case('dgrad', 'dgrad_reflect_k3p1', 2, 6, 10, 5, 7, 3, 1, 1, reflect=True, window=(1, 6), why='logical grid 7x9, pad 0 in the gather'),
        _case('dgrad', 'dgrad_reflect_k7p3', 2, 5, 3, 5, 7, 7, 1, 3, reflect=True, why='logical grid 11x13'),
        _case('dgrad', 'dgrad_reflect_k3p1s2', 2, 16, 16, 6, 8, 3, 2, 1, reflect=True, window=(3, 16), why='parity classes at pad 0 of the gather'),
        _case('dgrad', 'dgrad_ups2_k3p1', 2, 6, 10, 4, 5, 3, 1, 1, ups=2, window=(0, 6), why='logical grid 8x10, folded 2x2 by sg_pad_upsample_bwd'),
        _case('dgrad', 'dgrad_ups2_reflect_k3p1', 2, 16, 16, 3, 4, 3, 1, 1, ups=2, reflect=True, window=(1, 16), why='upsample and reflect together'),
        _case('dgrad', 'route_splitk_dgrad', 2, 16, 32, 5, 7, 3, 1, 1, window=(0, 16), opts={'splits': 2}, claims={'splits': 2}, why='split-K on a dgrad'),
        _case('dgrad', 'route_splitk_dgrad_window', 2, 16, 32, 5, 7, 3, 1, 1, window=(3, 16), opts={'splits': 2}, claims={'splits': 2},
              why='split-K with a window: Mtot == M holds for the window launch'),
    ]
    return cases


def _build_folded_cases():
    cases = []
    for (H, W) in ((3, 3), (3, 5), (8, 8), (9, 6)):
        for k, (C, Co) in enumerate(((6, 10), (16, 16), (5, 3), (40, 8))):
            win = _windows(C)[(k + H) % 4]
            cases.append(_case('folded', 'folded_%dx%d_%dto%d_w%d_%d' % (H, W, C, Co, win[0], win[1]), 1 + (H + k) % 3, C, Co, H, W, 3, 1, 1,
                               reflect=True, window=win, why='plane x window; 3x3: every pixel is a border pixel'))
    cases.append(_case('folded', 'route_splitk_folded', 2, 16, 32, 8, 8, 3, 1, 1, reflect=True, window=(0, 16), opts={'splits': 2},
                       claims={'splits': 2}, why='split-K over the nine source copies'))
    return cases


SUBPIXEL_FOLD_CHANNELS = ((1, 1), (5, 1), (1, 5), (5, 24), (24, 5), (24, 24))      # (Cin, Cout) of the fold and its adjoint alone


def _build_subpixel_cases():
    return [
        _case('subpixel', 'subpixel_1x1', 2, 5, 3, 1, 1, 3, 1, 1, ups=2, why='1x1 plane: every output pixel sees the same input pixel'),
        _case('subpixel', 'subpixel_5x7', 2, 6, 10, 5, 7, 3, 1, 1, ups=2, bias=False, why='odd plane'),
        _case('subpixel', 'subpixel_8x8', 3, 16, 24, 8, 8, 3, 1, 1, ups=2, why='fixed-tap loaders'),
    ]


CONVT_CASES = _build_convT_cases()
DGRAD_CASES = _build_dgrad_cases()
FOLDED_CASES = _build_folded_cases()
SUBPIXEL_CASES = _build_subpixel_cases()
ALL_CASES = CONVT_CASES + DGRAD_CASES + FOLDED_CASES + SUBPIXEL_CASES
BY_NAME = {c['name']: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES), 'duplicate case names'


def case_desc(case):
    """(entry, desc, c0, c1) of the transposed-gather launch of the case (convT: its forward)"""
    k = case['kind']
    N, Ci, Co, H, W, KS, s, p = [case[n] for n in ('N', 'Cin', 'Cout', 'H', 'W', 'KS', 'stride', 'pad')]
    if k == 'convT':
        op = case['out_pad']
        return TG_CONVT_FWD, make_desc(N, Ci, H, W, Co, KS, s, p, False, 1, convT_out_size(H, KS, s, p, op), convT_out_size(W, KS, s, p, op), op), 0, Co
    if k == 'subpixel':
        return TG_CONVT_FWD, make_desc(N, Ci, H, W, Co, 4, 2, 1, False, 1, 2 * H, 2 * W, 0), 0, Co
    ups, refl = case['ups'], case['reflect']
    pz = 0 if refl else p
    OH = conv_out_size(H * ups + (2 * p if refl else 0), KS, s, pz)
    OW = conv_out_size(W * ups + (2 * p if refl else 0), KS, s, pz)
    d = make_desc(N, Ci, H, W, Co, KS, s, p, refl, ups, OH, OW)
    return (TG_DGRAD_FOLDED if k == 'folded' else TG_CONV_DGRAD), d, case['window'][0], case['window'][1]


def case_expected_plan(case):
    entry, d, c0, c1 = case_desc(case)
    Cin = d.C1
    e = expected_plan(entry, d.N, Cin, d.Cout, d.H, d.W, d.KS, d.stride, d.pad, d.pad_reflect, d.upsample, d.out_pad, c0, c1, 4 * case['ws_off'])
    e.update(case['claims'])
    return entry, e


def case_options(case):
    """the option settings a case runs under: its forced options x both values of the parity split (stride-2 parity route) or of the
    tail split (stride-1 / plain route)"""
    entry, d, _, _ = case_desc(case)
    parity = entry != TG_DGRAD_FOLDED and d.stride == 2 and d.KS >= 3
    name, values = ('par_split', PAR_SPLIT_VALUES) if parity else ('w43_tail_split', TAIL_SPLIT_VALUES)
    return [dict(case['opts'], **{name: v}) for v in values]


# =============================================================================================
# inputs and references of a case
# =============================================================================================
def case_inputs(case):
    """-> dict of fp32 arrays.  convT / subpixel: x, w, b, gy; dgrad / folded: w [Cout, Cin, KS, KS], gy"""
    rng = rng_of(case['name'])
    entry, d, c0, c1 = case_desc(case)
    k = case['kind']
    if k == 'convT':
        w = f32(rng, (d.C1, d.Cout, d.KS, d.KS), 0.5)
    else:
        w = f32(rng, (d.Cout, d.C1, case['KS'], case['KS']), 0.5)
    out = dict(w=w, gy=f32(rng, (d.N, d.Cout, d.OH, d.OW)))
    if k in ('convT', 'subpixel'):
        out['x'] = f32(rng, (d.N, d.C1, d.H, d.W))
        out['b'] = f32(rng, (d.Cout,)) if case['bias'] else None
    return out


def _with_bound(fn, c, args):
    """(ref64, bound): fn on the float64 inputs, on their absolute values and on ones"""
    a64 = [None if a is None else np.asarray(a, dtype=np.float64) for a in args]
    ref = fn(*a64)
    sabs = fn(*[None if a is None else np.abs(a) for a in a64])
    terms = fn(*[None if a is None else np.ones_like(a) for a in a64])
    return ref, bound(terms, c, sabs)


def convT_refs(case, inp):
    """y, gx, gw, gb of a transposed conv with their bounds"""
    s, p, op, KS, H, W = case['stride'], case['pad'], case['out_pad'], case['KS'], case['H'], case['W']
    x, w, b, gy = inp['x'], inp['w'], inp['b'], inp['gy']
    r = {}
    # (the bias counts as one term of the ones-run: n + 1, and |b| joins the absolute sum)
    r['y'], r['y_bound'] = _with_bound(lambda x_, w_, b_: convT_fwd(x_, w_, b_, s, p, op), C_GATHER, (x, w, b))
    r['gx'], r['gx_bound'] = _with_bound(lambda g_, w_: convT_dgrad(g_, w_, s, p, H, W), C_GATHER, (gy, w))
    r['gw'], r['gw_bound'] = _with_bound(lambda g_, x_: convT_wgrad(g_, x_, KS, s, p), c_wgrad(case['N'] * H * W), (gy, x))
    r['gb'], r['gb_bound'] = _with_bound(bias_grad, 0, (gy,))
    return r


def dgrad_refs(case, inp):
    """the gradient on the logical grid ('g'), and folded onto the stored input ('gx') when the case reflects or upsamples"""
    entry, d, c0, c1 = case_desc(case)
    pz = 0 if case['reflect'] else case['pad']
    GH = d.H * d.upsample + (2 * d.pad if d.pad_reflect else 0)
    GW = d.W * d.upsample + (2 * d.pad if d.pad_reflect else 0)
    fn = lambda g_, w_: conv_dgrad_logical(g_, w_, d.stride, pz, GH, GW, c0, c1)
    r = {}
    r['g'], r['g_bound'] = _with_bound(fn, C_GATHER, (inp['gy'], inp['w']))
    if case['reflect'] or case['ups'] == 2:
        fp = d.pad if d.pad_reflect else 0
        fold = lambda g_, w_: fold_pad_upsample(fn(g_, w_), d.H, d.W, fp, d.upsample)
        # n of a folded pixel: all its terms; c: the gather's joins of each of its m parts plus the m adds of the fold
        m = fold_pad_upsample(np.ones((1, 1, GH, GW)), d.H, d.W, fp, d.upsample)
        g64, w64 = np.asarray(inp['gy'], dtype=np.float64), np.asarray(inp['w'], dtype=np.float64)
        r['gx'] = fold(g64, w64)
        r['gx_bound'] = bound(fold(np.ones_like(g64), np.ones_like(w64)) + m * (C_GATHER + 1), 0, fold(np.abs(g64), np.abs(w64)))
    return r


def folded_refs(case, inp):
    entry, d, c0, c1 = case_desc(case)
    return _with_bound(lambda g_, w_: conv_dgrad_folded(g_, w_, d.H, d.W, c0, c1), C_GATHER + C_VARIANT, (inp['gy'], inp['w']))


def subpixel_refs(case, inp):
    """conv3x3(pad 1)(nearest_up2(x)) and its gradients, through the fold: every bound carries the three extra roundings of a folded
    weight (forward, data gradient) or of the unfolded sum (weight gradient)"""
    H, W, N = case['H'], case['W'], case['N']
    x, w, b, gy = inp['x'], inp['w'], inp['b'], inp['gy']
    r = {}
    r['y'], r['y_bound'] = _with_bound(lambda x_, w_, b_: convT_fwd(x_, upconv3_fold(w_), b_, 2, 1, 0), C_GATHER + C_FOLD, (x, w, b))
    r['gx'], r['gx_bound'] = _with_bound(lambda g_, w_: convT_dgrad(g_, upconv3_fold(w_), 2, 1, H, W), C_GATHER + C_FOLD, (gy, w))
    r['gw'], r['gw_bound'] = _with_bound(lambda g_, x_: upconv3_unfold(convT_wgrad(g_, x_, 4, 2, 1)), c_wgrad(N * H * W) + C_FOLD, (gy, x))
    r['gb'], r['gb_bound'] = _with_bound(bias_grad, 0, (gy,))
    return r


# =============================================================================================
# one-hot probes
# =============================================================================================
def probe_positions(H, W):
    """the four corners, the middle of each edge and an interior pixel of an H x W plane (duplicates dropped on thin planes)"""
    rows, cols = sorted({0, H // 2, H - 1}), sorted({0, W // 2, W - 1})
    return [(r, c) for r in rows for c in cols]


def onehot(shape, n, c, pos):
    a = np.zeros(shape, dtype=np.float32)
    a[n, c, pos[0], pos[1]] = 1.0
    return a


def probe_sites(N, C, H, W):
    """(image, channel, (row, col)): every probe position, cycling the image and alternating the first and last channel"""
    return [(i % N, (0, C - 1)[i % 2], pos) for i, pos in enumerate(probe_positions(H, W))]


# the shapes the probes run on: small enough that every parity class and every border is hit by the nine positions, every kernel
# size at stride 2 (parity) and the 3x3 / 4x4 / 1x1 at stride 1 (plain), both loader kinds
PROBE_CONVT = [BY_NAME[n] for n in (
    'convT_k7s2p3_16to16', 'convT_k4s2p1_16to16', 'convT_k3s2p1op1_16to40', 'convT_k3s2p1op0_1x5', 'convT_k4s1p1_16to16',
    'convT_k1s2op1_16to16', 'convT_k3s1p1_16to16_off', 'convT_k7s2p0_5to3_1x1')]
PROBE_DGRAD = [BY_NAME[n] for n in (
    'dgrad_win_k3s2_6to10_w3_6', 'dgrad_win_k4s2_16to16_w3_16', 'dgrad_win_k7s2_5to3_w0_5', 'dgrad_win_k3s1_16to16_w3_16',
    'dgrad_win_k1s1_7to5_w3_7', 'dgrad_reflect_k3p1', 'dgrad_k3s2p1_1x9', 'dgrad_k7s2p3_3x3')]
PROBE_FOLDED = [BY_NAME[n] for n in ('folded_3x3_16to16_w0_16', 'folded_3x5_6to10_w3_4', 'folded_8x8_5to3_w0_3', 'folded_9x6_40to8_w0_40')]


# What a one-hot operand must produce, written as PLACEMENT (no sums): a single 1.0 at (n, c, row, col) copies taps of the other
# operand to the positions the index formula names, and leaves every other position 0 (or the bias).
def place_convT_fwd(site, xshape, w, b, s, p, op):
    """x = one-hot at (n, ci, ih, iw): y[n, :, ih*s-p+kh, iw*s-p+kw] = w[ci, :, kh, kw] (+ b), b elsewhere"""
    n, ci, (ih, iw) = site
    N, _, H, W = xshape
    Co, KS = w.shape[1], w.shape[2]
    OH, OW = convT_out_size(H, KS, s, p, op), convT_out_size(W, KS, s, p, op)
    y = np.zeros((N, Co, OH, OW), dtype=np.float32)
    for kh in range(KS):
        for kw in range(KS):
            oh, ow = ih * s - p + kh, iw * s - p + kw
            if 0 <= oh < OH and 0 <= ow < OW:
                y[n, :, oh, ow] = w[ci, :, kh, kw]
    return y if b is None else y + b.astype(np.float32)[None, :, None, None]


def place_convT_dgrad(site, gyshape, w, s, p, H, W):
    """gy = one-hot at (n, co, oh, ow): gx[n, :, ih, iw] = w[:, co, kh, kw] wherever ih*s-p+kh == oh and iw*s-p+kw == ow"""
    n, co, (oh, ow) = site
    gx = np.zeros((gyshape[0], w.shape[0], H, W), dtype=np.float32)
    KS = w.shape[2]
    for ih in range(H):
        for iw in range(W):
            kh, kw = oh - ih * s + p, ow - iw * s + p
            if 0 <= kh < KS and 0 <= kw < KS:
                gx[n, :, ih, iw] = w[:, co, kh, kw]
    return gx


def place_convT_wgrad(site, gy, Ci, KS, s, p):
    """x = one-hot at (n, ci, ih, iw): gw[ci, :, kh, kw] = gy[n, :, ih*s-p+kh, iw*s-p+kw] where that pixel exists"""
    n, ci, (ih, iw) = site
    Co, OH, OW = gy.shape[1:]
    gw = np.zeros((Ci, Co, KS, KS), dtype=np.float32)
    for kh in range(KS):
        for kw in range(KS):
            oh, ow = ih * s - p + kh, iw * s - p + kw
            if 0 <= oh < OH and 0 <= ow < OW:
                gw[ci, :, kh, kw] = gy[n, :, oh, ow]
    return gw


def place_conv_dgrad(site, gyshape, w, s, p, GH, GW, c0, c1):
    """gy = one-hot at (n, co, oh, ow): g[n, :, oh*s-p+kh, ow*s-p+kw] = w[co, c0:c1, kh, kw]"""
    n, co, (oh, ow) = site
    KS = w.shape[2]
    g = np.zeros((gyshape[0], c1 - c0, GH, GW), dtype=np.float32)
    for kh in range(KS):
        for kw in range(KS):
            gh, gw = oh * s - p + kh, ow * s - p + kw
            if 0 <= gh < GH and 0 <= gw < GW:
                g[n, :, gh, gw] = w[co, c0:c1, kh, kw]
    return g


def reflect_variant(g, kh, kw):
    """copy kh*3+kw of reflect_variants_kernel for planes g [.., H, W], in the dtype of g and in the kernel's order
    ((g[a][b] + g[ra][b]) + g[a][cb]) + g[ra][cb]:  tap 0 at row 2 also sees row 0, tap 2 at row H-3 also sees row H-1 (per axis)"""
    H, W = g.shape[-2:]
    ra = [0 if (kh == 0 and a == 2) else (H - 1 if (kh == 2 and a == H - 3) else -1) for a in range(H)]
    cb = [0 if (kw == 0 and b == 2) else (W - 1 if (kw == 2 and b == W - 3) else -1) for b in range(W)]
    v = g.copy()
    for a in range(H):
        if ra[a] >= 0:
            v[..., a, :] = v[..., a, :] + g[..., ra[a], :]
    for b in range(W):
        if cb[b] >= 0:
            v[..., :, b] = v[..., :, b] + g[..., :, cb[b]]
    for a in range(H):
        for b in range(W):
            if ra[a] >= 0 and cb[b] >= 0:
                v[..., a, b] = v[..., a, b] + g[..., ra[a], cb[b]]
    return v


def place_dgrad_folded_tap(gy, co, cm, kh, kw, M):
    """w = one-hot at (co, window channel cm, kh, kw): gx[n, cm, i, j] = variant_{kh,kw}(gy[n, co])[i + 1 - kh, j + 1 - kw] where that
    pixel exists (the zero-padded transposed gather of the folded form), every other channel 0"""
    N, _, H, W = gy.shape
    v = reflect_variant(gy[:, co], kh, kw)
    out = np.zeros((N, M, H, W), dtype=gy.dtype)
    for i in range(H):
        for j in range(W):
            a, b = i + 1 - kh, j + 1 - kw
            if 0 <= a < H and 0 <= b < W:
                out[:, cm, i, j] = v[:, a, b]
    return out
