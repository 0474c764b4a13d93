"""Case table, input builders, float64 references and criteria of the Winograd convolution tests: sg_conv2d_wino_fwd / _dgrad / _wgrad
(F(2x2,3x3) and F(4x4,3x3)), the fused pair sg_conv2d_wino_fwd_instnorm / _dgrad_instnorm and sg_conv2d_wino24_fwd / _dgrad /
_wgrad (F(2x2,4x4)) of csrc/igemm.hip.  Shared by tests/test_winograd_cases_cpu.py (the restatements equal the direct convolution,
the adjoint pairs are adjoint, mutants of the restatement are caught, the table reaches every plan value) and
tests/test_gpu_winograd.py (every case against float64 on the device).

NumPy only.  The reference of every entry is the DIRECT float64 convolution (transposed_conv_cases: conv_fwd, conv_dgrad_logical,
fold_pad_upsample, nearest_up2, bias_grad; conv_wgrad here).  Next to it the three Winograd forms are restated, dtype-generic, from
three matrices each (B^T, G, A^T: F(2x2,3x3) the classic set, F(4x4,3x3) parsed from csrc/igemm.hip, F(2x2,4x4) as derived by
tools/winograd_f24.py and transcribed in tests/test_host_logic.py):
  forward                  y  = A^T [sum_c (G g G^T) . (B^T d B)] A
  adjoint data gradient    gp = B [sum_co U . (A gy A^T)] B^T, overlap-added on the padded grid, then the reflection fold
  weight gradient          gw = G^T [sum_p (A gy A^T) . (B^T d B)] G
with every transform evaluated as the k-ordered products the kernels write (W43_ACC: a zero coefficient adds nothing, +-1 adds or
subtracts, anything else is a multiply-add from acc = 0).

The launch plans come from the library's host-side query (include/sg2im_hip.h: sg_conv2d_wino_plan); expected_plan() restates its
predicates independently, from the shape, the options, the operand alignment and the saved operands passed.

Criteria.
  hard bound, per element   |got - ref64| <= gamma(n + c) * Babs.  Babs: the form's restatement in float64 on the absolute values of
      the operands AND of the matrices.  n: the reduction length of the GEMM (input channels: forward; output channels: data
      gradient; tiles: weight gradient).  c, the roundings along one output's chain outside the GEMM, counted from the code for a
      form with a x a transformed tiles and r x r filters:
        2a      two 1-D passes of the moving operand's transform (at most a terms each: w43_input_xform, w43_gy_xform, ...)
        2r + 2  two 1-D passes of the filter transform (r terms each) + the two roundings of the coefficients that are no binary
                fractions (1/3, 1/15, 1/6: one per pass)
        2a      two 1-D passes of the result's transform (w43_output_xform, w43_patch_xform, w43_wgrad_xform: at most a terms)
        2a      the second moving operand of the weight gradient (both x and gy are transformed)
        C_JOIN = 8   joins of partial sums: chunks of the channel sum (TileCfg::KFOLD, 128 or 256: at most 4 at 512 channels), the k-chunks
                of the F(2x2,4x4) weight gradient (w24_wgrad_output_kernel: S <= 3 in the table), the overlap-add of up to four
                patches and the reflection / upsample fold of up to four positions (3 adds each), the bias add
      i.e. c = 6a + 2r + 2 + 8: 40 for F(2x2,3x3), 52 for F(4x4,3x3), 48 for F(2x2,4x4).  A worst-case line: Babs is 28x .. 257x
      sum|x||w| for F(4x4,3x3) at 128 channels, so it only catches gross errors (a missing term is about as large as the smallest
      bound); the sharp work is done by
  rms line, per output      rms(got - ref64) <= RMS_FACTOR * rms(restatement32 - ref64), RMS_FACTOR = 2: restatement32 is the same form
      in float32 with the reduction added sequentially, one product and one sum rounded per term.  The baseline comes from the
      reference alone.
  one-hot probes            a single 1.0 in one operand: the hard bound with n = 1, and exact zeros (or the bias) outside the tiles
      the one-hot reaches."""
import ctypes
import functools
import os
import re

import numpy as np

from scene_generation_amd._hip import CONST, plan_dict, sgWinoPlan

from dense_pointwise_cases import gamma, rng_of, f32, option  # noqa: F401  (re-exported)
from transposed_conv_cases import (conv_fwd, conv_dgrad_logical, fold_pad_upsample, nearest_up2, bias_grad, make_desc,  # noqa: F401
                                   probe_sites, onehot, _pairs, _reflect)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RMS_FACTOR = 2.0
C_JOIN = 8

# include/sg2im_hip.h, under the short names the tables use
(WINO_FWD, WINO_DGRAD, WINO_WGRAD, WINO_FWD_INSTNORM, WINO_DGRAD_INSTNORM, WINO24_FWD, WINO24_DGRAD, WINO24_WGRAD) = (
    CONST['SG_' + n] for n in ('WINO_FWD', 'WINO_DGRAD', 'WINO_WGRAD', 'WINO_FWD_INSTNORM', 'WINO_DGRAD_INSTNORM', 'WINO24_FWD',
                               'WINO24_DGRAD', 'WINO24_WGRAD'))
ENTRY_NAMES = ('fwd', 'dgrad', 'wgrad', 'fwd_instnorm', 'dgrad_instnorm', 'w24_fwd', 'w24_dgrad', 'w24_wgrad')
WA_X, WA_W, WA_Y, WA_GY, WA_GX, WA_GW, WA_ALL = (CONST['SG_WA_' + n] for n in ('X', 'W', 'Y', 'GY', 'GX', 'GW', 'ALL'))
WS_UT, WS_V, WS_YTP = (CONST['SG_WS_' + n] for n in ('UT', 'V', 'YTP'))
WF_UNSUPPORTED, WF_F23_GENERIC, WF_F23_ADJOINT, WF_F43, WF_F24 = (
    CONST['SG_WF_' + n] for n in ('UNSUPPORTED', 'F23_GENERIC', 'F23_ADJOINT', 'F43', 'F24'))
WK_NONE, WK_IN_LDS, WK_IN_GENERAL = (CONST['SG_WK_' + n] for n in ('NONE', 'IN_LDS', 'IN_GENERAL'))
WK_WT_LDS, WK_WT_PLAIN = CONST['SG_WK_WT_LDS'], CONST['SG_WK_WT_PLAIN']
WK_FOLD_CELLS, WK_FOLD_WALK, WK_FOLD_F43, WK_FOLD_PAD_UPSAMPLE = (
    CONST['SG_WK_FOLD_' + n] for n in ('CELLS', 'WALK', 'F43', 'PAD_UPSAMPLE'))
WSRC_SAVED, WSRC_REBUILT = CONST['SG_WSRC_SAVED'], CONST['SG_WSRC_REBUILT']
PLAN_FIELDS = tuple(n for n, _ in sgWinoPlan._fields_)
# the library's defaults of the options the plans depend on (csrc/runtime.hip; the CPU module checks them against the library)
OPTION_DEFAULTS = dict(wino_wt=1, wino_fold_cells=1, wino_reuse=1, wino_in_fuse=1, wino_pipe=2, wino_gemm_tile=0, wino43=1, wino_adjoint=1,
                       w43_kfold=256, w43_nsub=1, w43_wgrad_tile=0, w24_small=1, w24_s=-1, w24_gemm_tile=2, w24_pmin=256, wino24=1)


def wino_plan(lib, desc, entry, align_mask=WA_ALL, saved_mask=0):
    """sg_conv2d_wino_plan under the current options -> dict, or None when the query returns non-zero"""
    p = sgWinoPlan()
    rc = lib.sg_conv2d_wino_plan(ctypes.byref(desc), int(entry), int(align_mask), int(saved_mask), ctypes.byref(p))
    return None if rc else plan_dict(p)


# =============================================================================================
# the three matrix sets
# =============================================================================================
class Form:
    def __init__(self, name, BT, G, AT):
        self.name, self.BT, self.G, self.AT = name, np.array(BT, dtype=np.float64), np.array(G, dtype=np.float64), np.array(AT, dtype=np.float64)
        self.m, self.r, self.a = self.AT.shape[0], self.G.shape[1], self.BT.shape[0]
        assert self.a == self.m + self.r - 1 and self.G.shape[0] == self.a and self.AT.shape[1] == self.a
        self.c = 6 * self.a + 2 * self.r + 2 + C_JOIN

    def abs(self):
        return Form(self.name + '_abs', np.abs(self.BT), np.abs(self.G), np.abs(self.AT))

    def with_matrix(self, which, i, j, value):
        """a copy with one coefficient replaced (the mutants)"""
        mats = dict(BT=self.BT.copy(), G=self.G.copy(), AT=self.AT.copy())
        mats[which][i, j] = value
        return Form(self.name + '_mut', mats['BT'], mats['G'], mats['AT'])


def _parse_f43():
    src = open(os.path.join(ROOT, 'scene_generation_amd', 'csrc', 'igemm.hip')).read()

    def matrix(fn, rows, cols):
        body = re.search(r'%s\(int i, int j\) \{\s*constexpr float m\[%d\]\[%d\] = (\{.*?\});' % (fn, rows, cols), src, re.S).group(1)
        vals = [eval(v.replace('f', ''), {'__builtins__': {}}) for v in re.findall(r'-?\d+\.?\d*f(?:\s*/\s*\d+\.?\d*f)?', body)]
        assert len(vals) == rows * cols, (fn, len(vals))
        return np.array(vals, dtype=np.float64).reshape(rows, cols)
    return Form('F43', matrix('w43_bt', 6, 6), matrix('w43_g', 6, 3), matrix('w43_at', 4, 6))


F23 = Form('F23', [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]],
           [[1, 1, 1, 0], [0, 1, -1, -1]])
F43 = _parse_f43()
F24 = Form('F24', [[-2, -1, 2, 1, 0], [0, 2, 3, 1, 0], [0, -2, 1, 1, 0], [0, -1, 0, 1, 0], [0, -2, -1, 2, 1]],
           [[-1 / 2, 0, 0, 0], [1 / 6, 1 / 6, 1 / 6, 1 / 6], [1 / 2, -1 / 2, 1 / 2, -1 / 2], [-1 / 6, 1 / 3, -2 / 3, 4 / 3], [0, 0, 0, 1]],
           [[1, 1, 1, 1, 0], [0, 1, -1, -2, 1]])


# =============================================================================================
# dtype-generic restatements
# =============================================================================================
def kprod(mat, arr, axis):
    """out[i] = sum_k mat[i, k] arr[k] along ``axis`` in the dtype of arr, added in ascending k the way W43_ACC writes it"""
    arr = np.moveaxis(arr, axis, 0)
    ty = arr.dtype.type
    out = np.zeros((mat.shape[0],) + arr.shape[1:], dtype=arr.dtype)
    for i in range(mat.shape[0]):
        acc = None
        for k in range(mat.shape[1]):
            c = mat[i, k]
            if c == 0:
                continue
            term = arr[k] if c == 1 else (-arr[k] if c == -1 else ty(c) * arr[k])
            acc = term if acc is None else acc + term
        if acc is not None:
            out[i] = acc
    return np.moveaxis(out, 0, axis)


def xform(mat, t):
    """mat t mat^T over the two leading axes: rows first, then columns, as the kernels do"""
    return kprod(mat, kprod(mat, t, 0), 1)


def csum(A, B, chunk=0, drop_last=False):
    """out[.., i, j] = sum_k A[.., i, k] B[.., j, k].  float64: one einsum.  float32: added sequentially in ascending k, one product
    and one sum rounded per term; chunk > 0: partial sums of ``chunk`` terms each, joined in ascending order (TileCfg::KFOLD, the
    k-chunks of the F(2x2,4x4) weight gradient).  drop_last leaves the last chunk out (a mutant)."""
    K = A.shape[-1]
    if A.dtype == np.float64 and not drop_last:
        return np.einsum('...ik,...jk->...ij', A, B)
    bounds = [(0, K)] if chunk <= 0 or chunk >= K else [(k0, min(K, k0 + chunk)) for k0 in range(0, K, chunk)]
    if drop_last:
        assert len(bounds) > 1
        bounds = bounds[:-1]
    total = None
    for k0, k1 in bounds:
        acc = np.zeros(A.shape[:-1] + (B.shape[-2],), dtype=A.dtype)
        for k in range(k0, k1):
            acc = acc + A[..., :, None, k] * B[..., None, :, k]
        total = acc if total is None else total + acc
    return total


def tiles_of(xp, m, a, TH, TW, shift=0):
    """[a, a, N*TH*TW, C]: the a x a patch of tile (ti, tj) starts at (m ti, m tj) of xp [N, C, PH, PW], zero beyond it; ``shift``
    moves the column offset of the LAST tile column (a mutant)"""
    N, C, PH, PW = xp.shape
    big = np.zeros((N, C, max(PH, m * (TH - 1) + a), max(PW, m * (TW - 1) + a + abs(shift))), dtype=xp.dtype)
    big[:, :, :PH, :PW] = xp
    ih = m * np.arange(TH)[:, None] + np.arange(a)[None, :]                 # [TH, a]
    iw = m * np.arange(TW)[:, None] + np.arange(a)[None, :]
    if shift:
        iw[-1] += shift
    t = big[:, :, ih[:, None, :, None], iw[None, :, None, :]]               # [N, C, TH, TW, a, a]
    return np.ascontiguousarray(t.transpose(4, 5, 0, 2, 3, 1)).reshape(a, a, N * TH * TW, C)


def untile(Y, N, TH, TW, OH, OW, unclipped=False):
    """[m, m, M, N*TH*TW] -> [N, M, OH, OW], the tiles clipped at the plane's edge.  unclipped (a mutant): every tile element is stored
    at its flat offset row * OW + col, a clipped column landing on the next row, later tiles overwriting earlier ones"""
    m, M = Y.shape[0], Y.shape[2]
    full = Y.reshape(m, m, M, N, TH, TW).transpose(3, 2, 4, 0, 5, 1).reshape(N, M, TH * m, TW * m)
    if not unclipped:
        return np.ascontiguousarray(full[:, :, :OH, :OW])
    out = np.zeros((N, M, OH * OW + m * OW + m), dtype=Y.dtype)
    for ti in range(TH):
        for tj in range(TW):
            for i in range(m):
                for j in range(m):
                    out[:, :, (ti * m + i) * OW + tj * m + j] = full[:, :, ti * m + i, tj * m + j]
    return np.ascontiguousarray(out[:, :, :OH * OW].reshape(N, M, OH, OW))


def _ceil(a, b):
    return -(-a // b)


def wino_fwd(form, xp, w, OH, OW, chunk=0, drop_last=False, shift=0, unclipped=False):
    """y[n, co, oh, ow] = sum_{c, kh, kw} w[co, c, kh, kw] xp[n, c, oh + kh, ow + kw] through the form; xp is the PADDED logical input"""
    N, M = xp.shape[0], w.shape[0]
    TH, TW = _ceil(OH, form.m), _ceil(OW, form.m)
    V = xform(form.BT, tiles_of(xp, form.m, form.a, TH, TW, shift))                    # [a, a, P, C]
    U = xform(form.G, np.ascontiguousarray(w.transpose(2, 3, 0, 1)))                   # [a, a, M, C]
    Y = xform(form.AT, csum(U, V, chunk, drop_last))                                   # [m, m, M, P]
    return untile(Y, N, TH, TW, OH, OW, unclipped)


def wino_dgrad_adjoint(form, gy, w, chunk=0, drop_last=False, reflect=_reflect):
    """gx [N, C, H, W] of ReflectionPad(1) + 3x3 conv over the OUTPUT tiles: Yt = A gy A^T, patch = B (sum_co U . Yt) B^T on the
    (H + 2) x (W + 2) grid at (m ti, m tj), overlap-add, reflection fold"""
    N, K, H, W = gy.shape
    C = w.shape[1]
    TH, TW = H // form.m, W // form.m
    Yt = xform(form.AT.T, tiles_of(gy, form.m, form.m, TH, TW))                        # [a, a, P, Cout]
    U = xform(form.G, np.ascontiguousarray(w.transpose(2, 3, 1, 0)))                   # [a, a, C, Cout]
    R = xform(form.BT.T, csum(U, Yt, chunk, drop_last))                                # [a, a, C, P]
    R = R.reshape(form.a, form.a, C, N, TH, TW)
    gp = np.zeros((N, C, H + 2, W + 2), dtype=gy.dtype)
    for ti in range(TH):
        for tj in range(TW):
            blk = R[:, :, :, :, ti, tj].transpose(3, 2, 0, 1)
            gp[:, :, form.m * ti:form.m * ti + form.a, form.m * tj:form.m * tj + form.a] += blk
    if reflect is _reflect:
        return fold_pad_upsample(gp, H, W, 1, 1)
    ih = np.array([reflect(p - 1, H) for p in range(H + 2)])
    iw = np.array([reflect(p - 1, W) for p in range(W + 2)])
    gx = np.zeros((N, C, H, W), dtype=gp.dtype)
    np.add.at(gx, (Ellipsis, ih[:, None], iw[None, :]), gp)
    return gx


def wino_wgrad(form, gy, xp, chunk=0, drop_last=False):
    """gw[co, c, kh, kw] = sum_{n, oh, ow} gy[n, co, oh, ow] xp[n, c, oh + kh, ow + kw] through the form (tiles of the output grid)"""
    N, M, OH, OW = gy.shape
    TH, TW = _ceil(OH, form.m), _ceil(OW, form.m)
    Yt = xform(form.AT.T, tiles_of(gy, form.m, form.m, TH, TW))                        # [a, a, P, M]
    V = xform(form.BT, tiles_of(xp, form.m, form.a, TH, TW))                           # [a, a, P, C]
    T = csum(np.ascontiguousarray(Yt.transpose(0, 1, 3, 2)), np.ascontiguousarray(V.transpose(0, 1, 3, 2)), chunk, drop_last)
    return np.ascontiguousarray(xform(form.G.T, T).transpose(2, 3, 0, 1))             # [M, C, r, r]


def conv_wgrad(gy, xp, KS):
    """direct: gw[co, c, kh, kw] = sum_{n, oh, ow} gy[n, co, oh, ow] xp[n, c, oh + kh, ow + kw]"""
    N, M, OH, OW = gy.shape
    gw = np.zeros((M, xp.shape[1], KS, KS), dtype=gy.dtype)
    for kh in range(KS):
        for kw in range(KS):
            gw[:, :, kh, kw] = np.einsum('nmhw,nchw->mc', gy, xp[:, :, kh:kh + OH, kw:kw + OW])
    return gw


def pad_input(x, pad, reflect, ups, clamp=False):
    """the padded logical input of a conv: nearest x2 upsample, then reflection (clamp: replicate -- a mutant) or zero padding"""
    if ups == 2:
        x = nearest_up2(x)
    if pad == 0:
        return x
    mode = ('edge' if clamp else 'reflect') if reflect else 'constant'
    return np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)), mode=mode)


def rot_swap(w):
    """the filter of the data gradient as a correlation: rotated by 180 degrees, channel roles swapped"""
    return np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


# =============================================================================================
# the case table
# =============================================================================================
def _case(family, name, N, Cin, Cout, H, W, reflect=True, ups=1, KS=3, pad=1, dgrad_form=None, off=None, opts=None, claims=None, why=''):
    """family: F43, F23A (adjoint data gradient), F23G (generic form, reflect), F23Z (zero padding), F23U (behind the x2 upsample), F24.
    off: {'x' | 'w' | 'gy': floats off a 16-byte boundary}.  opts: options the case is forced under.  claims: {entry name: plan fields}
    the row is there for (checked next to the full restated plan)."""
    if dgrad_form is None:
        dgrad_form = dict(F43=WF_F43, F23A=WF_F23_ADJOINT, F24=WF_F24).get(family, WF_F23_GENERIC)
    return dict(family=family, name=name, N=N, Cin=Cin, Cout=Cout, H=H, W=W, reflect=reflect, ups=ups, KS=KS, pad=pad, dgrad_form=dgrad_form,
                off=dict(off or {}), opts=dict(opts or {}), claims={k: dict(v) for k, v in (claims or {}).items()}, why=why)


_F43_SHAPES = (
    ('16_128to128_8x8', 16, 128, 128, 8, 8, 'one 64-column tile, no chunking'),
    ('16_384to128_8x8', 16, 384, 128, 8, 8, 'forward chunks of 256 + 128'),
    ('16_128to384_8x8', 16, 128, 384, 8, 8, 'data-gradient chunks of 256 + 128'),
    ('16_512to128_8x8', 16, 512, 128, 8, 8, 'two whole chunks'),
    ('4_128to256_16x16', 4, 128, 256, 16, 16, '16 tiles per plane'),
    ('16_128to128_4x16', 16, 128, 128, 4, 16, 'one tile row'),
    ('16_128to128_16x4', 16, 128, 128, 16, 4, 'one tile column'),
    ('64_128to128_4x4', 64, 128, 128, 4, 4, 'one tile per plane, reflected on both sides'),
    ('32_128to128_8x12', 32, 128, 128, 8, 12, 'six tiles per plane'),
)
_F23A_SHAPES = (
    ('8_128to128_8x8', 8, 128, 128, 8, 8, '32 F(4x4,3x3) tiles: no multiple of 64'),
    ('128_128to128_6x6', 128, 128, 128, 6, 6, 'planes that do not split into 4x4 tiles'),
    ('16_128to256_6x16', 16, 128, 256, 6, 16, 'H % 4 != 0'),
)


def _build_cases():
    cs = []
    for (nm, N, Ci, Co, H, W, why) in _F43_SHAPES:
        kf = lambda K: 256 if K > 256 else 0
        cs.append(_case('F43', 'f43_' + nm, N, Ci, Co, H, W, why=why,
                        claims={'fwd': dict(form=WF_F43, kfold=kf(Ci), bm=64, bn=64, nsub=1), 'dgrad': dict(form=WF_F43, kfold=kf(Co), fold_kernel=WK_FOLD_F43)}))
    for (nm, N, Ci, Co, H, W, why) in _F23A_SHAPES:
        cs.append(_case('F23A', 'f23a_' + nm, N, Ci, Co, H, W, why=why,
                        claims={'dgrad': dict(form=WF_F23_ADJOINT, fold_kernel=WK_FOLD_CELLS, in_kernel=WK_IN_LDS), 'fwd': dict(in_kernel=WK_IN_LDS, bm=128, bn=128)}))
    for (nm, N, Ci, Co, H, W, why) in _F43_SHAPES:
        cs.append(_case('F23A', 'f23a_wino43off_' + nm, N, Ci, Co, H, W, opts={'wino43': 0}, why='the F(4x4,3x3) shape under wino43 = 0',
                        claims={'dgrad': dict(form=WF_F23_ADJOINT), 'fwd': dict(form=WF_F23_GENERIC, kfold=0)}))
    cs.append(_case('F23G', 'f23g_16_128to128_18x16', 16, 128, 128, 18, 16, why='plane above 256 pixels; Pd = 16*10*9 padded to a multiple of 128',
                    claims={'dgrad': dict(form=WF_F23_GENERIC, Pd=1440, Pds=1536, in_kernel=WK_IN_GENERAL, fold_kernel=WK_FOLD_PAD_UPSAMPLE),
                            'fwd': dict(in_kernel=WK_IN_GENERAL)}))
    for (nm, N, Ci, Co, H, W, why) in _F23A_SHAPES:
        cs.append(_case('F23G', 'f23g_adjointoff_' + nm, N, Ci, Co, H, W, opts={'wino_adjoint': 0}, why='the adjoint shape under wino_adjoint = 0',
                        claims={'dgrad': dict(form=WF_F23_GENERIC, fold_kernel=WK_FOLD_PAD_UPSAMPLE, in_kernel=WK_IN_LDS)}))
    cs.append(_case('F23G', 'f23g_gyoff_8_128to128_8x8', 8, 128, 128, 8, 8, off={'gy': 1}, why='gy one float off alignment: the generic form, silently',
                    claims={'dgrad': dict(form=WF_F23_GENERIC, in_kernel=WK_IN_GENERAL, fold_kernel=WK_FOLD_PAD_UPSAMPLE)}))
    cs += [
        _case('F23Z', 'f23z_2_128to128_16x16', 2, 128, 128, 16, 16, reflect=False, why='zero padding, LDS input kernel',
              claims={'dgrad': dict(form=WF_F23_GENERIC, fold_kernel=WK_NONE, Pd=128, Pds=128), 'fwd': dict(in_kernel=WK_IN_LDS)}),
        _case('F23Z', 'f23z_16_128to256_8x12', 16, 128, 256, 8, 12, reflect=False, why='rectangular plane, Cout > Cin',
              claims={'dgrad': dict(form=WF_F23_GENERIC, fold_kernel=WK_NONE)}),
        _case('F23Z', 'f23z_16_128to128_16x18', 16, 128, 128, 16, 18, reflect=False, why='plane above 256 pixels: general input kernel',
              claims={'fwd': dict(in_kernel=WK_IN_GENERAL), 'dgrad': dict(in_kernel=WK_IN_GENERAL)}),
        _case('F23Z', 'f23z_xwoff_2_128to128_16x16', 2, 128, 128, 16, 16, reflect=False, off={'x': 1, 'w': 1},
              why='x and w one float off alignment: plain weight kernel and general input kernel',
              claims={'fwd': dict(in_kernel=WK_IN_GENERAL, wt_kernel=WK_WT_PLAIN), 'dgrad': dict(wt_kernel=WK_WT_PLAIN)}),
        _case('F23U', 'f23u_8_128to128_4x4', 8, 128, 128, 4, 4, reflect=False, ups=2, why='x2 upsample folded into the read, 8x8 logical',
              claims={'fwd': dict(in_kernel=WK_IN_GENERAL), 'dgrad': dict(form=WF_F23_GENERIC, fold_kernel=WK_FOLD_PAD_UPSAMPLE)}),
        _case('F23U', 'f23u_2_128to128_8x8', 2, 128, 128, 8, 8, reflect=False, ups=2, why='16x16 logical'),
        _case('F23U', 'f23u_16_128to128_4x6', 16, 128, 128, 4, 6, reflect=False, ups=2, why='8x12 logical'),
        _case('F24', 'f24_4_128to128_17x17_p2', 4, 128, 128, 17, 17, reflect=False, KS=4, pad=2, why='S = 1',
              claims={'w24_wgrad': dict(S=1), 'w24_fwd': dict(form=WF_F24, in_kernel=WK_IN_LDS, bm=64, bn=64)}),
        _case('F24', 'f24_8_128to256_20x14_p1', 8, 128, 256, 20, 14, reflect=False, KS=4, pad=1, why='odd 19x13 output, S = 2, zero-padded last chunk',
              claims={'w24_wgrad': dict(S=2, P=560, Pc=288), 'w24_fwd': dict(TH=10, TW=7, Ps=640)}),
        _case('F24', 'f24_8_256to128_19x19_p0', 8, 256, 128, 19, 19, reflect=False, KS=4, pad=0, why='no padding, Cin > Cout',
              claims={'w24_fwd': dict(TH=8, TW=8, P=512), 'w24_dgrad': dict(THd=10, TWd=10, Pd=800, Pds=896)}),
        _case('F24', 'f24_16_128to128_8x8_p3', 16, 128, 128, 8, 8, reflect=False, KS=4, pad=3, why='plane under 144 pixels: general input kernel',
              claims={'w24_fwd': dict(in_kernel=WK_IN_GENERAL), 'w24_dgrad': dict(in_kernel=WK_IN_GENERAL)}),
        _case('F24', 'f24_4_128to128_6x70_p1', 4, 128, 128, 6, 70, reflect=False, KS=4, pad=1, why='W above 64: general input kernel',
              claims={'w24_fwd': dict(in_kernel=WK_IN_GENERAL), 'w24_dgrad': dict(in_kernel=WK_IN_GENERAL)}),
    ]
    return cs


CASES = _build_cases()
BY_NAME = {c['name']: c for c in CASES}
assert len(BY_NAME) == len(CASES), 'duplicate case names'

# each option alone against the defaults, on cases that reach it: (case, {option: value}, {entry name: plan fields it must show})
OPTION_TOGGLES = (
    ('f23z_2_128to128_16x16', {'wino_wt': 0}, {'fwd': dict(wt_kernel=WK_WT_PLAIN), 'dgrad': dict(wt_kernel=WK_WT_PLAIN)}),
    ('f23a_8_128to128_8x8', {'wino_wt': 0}, {'dgrad': dict(wt_kernel=WK_WT_PLAIN)}),
    ('f23a_8_128to128_8x8', {'wino_fold_cells': 0}, {'dgrad': dict(fold_kernel=WK_FOLD_WALK)}),
    ('f23a_16_128to256_6x16', {'wino_fold_cells': 0}, {'dgrad': dict(fold_kernel=WK_FOLD_WALK)}),
    ('f23a_8_128to128_8x8', {'wino_reuse': 0}, {'wgrad': dict(wgrad_src=WSRC_REBUILT)}),
    ('f43_16_128to128_8x8', {'wino_reuse': 0}, {'wgrad': dict(form=WF_F43)}),
    ('f43_16_128to128_8x8', {'wino_in_fuse': 0}, {'fwd': dict(form=WF_F43)}),
    ('f23a_8_128to128_8x8', {'wino_pipe': 1}, {'fwd': dict(pipe=1)}),
    ('f23z_16_128to256_8x12', {'wino_pipe': 1}, {'fwd': dict(pipe=1), 'dgrad': dict(pipe=1)}),
    ('f23a_8_128to128_8x8', {'wino_gemm_tile': 1}, {'fwd': dict(bm=64, bn=128), 'dgrad': dict(bm=64, bn=128)}),
    ('f23z_16_128to256_8x12', {'wino_gemm_tile': 2}, {'fwd': dict(bm=64, bn=64), 'wgrad': dict(bm=64, bn=64)}),
    ('f43_16_384to128_8x8', {'w43_kfold': 0}, {'fwd': dict(kfold=0)}),
    ('f43_16_384to128_8x8', {'w43_kfold': 128}, {'fwd': dict(kfold=128), 'dgrad': dict(kfold=0)}),
    ('f43_16_128to384_8x8', {'w43_kfold': 128}, {'dgrad': dict(kfold=128)}),
    ('f43_4_128to256_16x16', {'w43_kfold': 128}, {'dgrad': dict(kfold=128), 'fwd': dict(kfold=0)}),
    ('f43_16_512to128_8x8', {'w43_nsub': 2}, {'fwd': dict(nsub=2), 'wgrad': dict(nsub=2)}),
    ('f43_32_128to128_8x12', {'w43_nsub': 2}, {'dgrad': dict(nsub=2)}),
    ('f43_16_128to128_8x8', {'w43_wgrad_tile': 1}, {'wgrad': dict(bm=128, bn=128)}),
    ('f43_4_128to256_16x16', {'w43_wgrad_tile': 2}, {'wgrad': dict(bm=64, bn=128)}),
    ('f24_4_128to128_17x17_p2', {'w24_small': 0}, {'w24_fwd': dict(in_kernel=WK_IN_GENERAL), 'w24_dgrad': dict(in_kernel=WK_IN_GENERAL)}),
    ('f24_8_128to256_20x14_p1', {'w24_s': 1}, {'w24_wgrad': dict(S=1, Pc=576)}),
    # (w24_plan caps S at P / 256: no shape of the table has the 768 tiles that S = 3 needs, the forced 3 is cut to 2)
    ('f24_8_256to128_19x19_p0', {'w24_s': 3}, {'w24_wgrad': dict(S=2, Pc=256)}),
    ('f24_4_128to128_17x17_p2', {'w24_gemm_tile': 0}, {'w24_fwd': dict(bm=128, bn=128)}),
    ('f24_8_128to256_20x14_p1', {'w24_gemm_tile': 1}, {'w24_fwd': dict(bm=64, bn=128), 'w24_wgrad': dict(bm=64, bn=128)}),
)
FUSED_CASES = ('f43_16_128to128_8x8', 'f43_4_128to256_16x16')        # norm template <1> / <4>
PROBE_CASES = ('f43_32_128to128_8x12', 'f23a_8_128to128_8x8', 'f23g_gyoff_8_128to128_8x8', 'f23z_2_128to128_16x16', 'f23u_8_128to128_4x4',
               'f24_8_128to256_20x14_p1')


def case_desc(case):
    N, Ci, Co, H, W, KS, p, ups = [case[k] for k in ('N', 'Cin', 'Cout', 'H', 'W', 'KS', 'pad', 'ups')]
    OH, OW = H * ups + 2 * p - KS + 1, W * ups + 2 * p - KS + 1
    return make_desc(N, Ci, H, W, Co, KS, 1, p, case['reflect'], ups, OH, OW)


def case_entries(case):
    return (WINO24_FWD, WINO24_DGRAD, WINO24_WGRAD) if case['family'] == 'F24' else (WINO_FWD, WINO_DGRAD, WINO_WGRAD)


def case_align(case, entry):
    """the alignment mask of the operands as the GPU module places them"""
    m = WA_ALL
    for k, bit in (('x', WA_X), ('w', WA_W), ('gy', WA_GY)):
        if case['off'].get(k, 0) % 4:
            m &= ~bit
    return m


def saved_masks(case, entry, opts=None):
    """every combination of saved operands the entry accepts for the case under the options"""
    o = dict(OPTION_DEFAULTS, **case['opts'])
    o.update(opts or {})
    if case['family'] == 'F24':
        return (0,)
    adjoint_shape = _adjoint_shape(case, o)
    f43 = _f43_shape(case, o)
    reuse = adjoint_shape and (o['wino_reuse'] or f43)
    if entry in (WINO_FWD, WINO_FWD_INSTNORM):
        ut_ok = adjoint_shape and (f43 or (o['wino_wt'] and not case['off'].get('w', 0)))
        v_ok = adjoint_shape and (f43 or o['wino_reuse'])
        return tuple(u | v for u in ((0, WS_UT) if ut_ok else (0,)) for v in ((0, WS_V) if v_ok else (0,)))
    if entry in (WINO_DGRAD, WINO_DGRAD_INSTNORM):
        adj = f43 or (adjoint_shape and not case['off'].get('gy', 0))
        return (0, WS_UT, WS_YTP, WS_UT | WS_YTP) if adj else (0,)
    return (0, WS_V | WS_YTP) if reuse and not case['off'].get('gy', 0) else (0,)      # (Ytp comes from the adjoint data gradient)


def _adjoint_shape(case, o):
    return bool(o['wino_adjoint'] and case['family'] != 'F24' and case['reflect'] and case['ups'] == 1 and case['H'] * case['W'] <= 256 and
                (case['H'] * case['W']) % 4 == 0)


def _f43_shape(case, o):
    return bool(o['wino43'] and _adjoint_shape(case, o) and case['H'] % 4 == 0 and case['W'] % 4 == 0 and
                (case['N'] * (case['H'] // 4) * (case['W'] // 4)) % 64 == 0)


def _pad128(n):
    return _ceil(n, 128) * 128


def expected_plan(case, entry, opts=None, align=None, saved=0):
    """the plan of an entry, restated from the comments of csrc/igemm.hip; opts on top of the case's own and the defaults"""
    o = dict(OPTION_DEFAULTS, **case['opts'])
    o.update(opts or {})
    align = case_align(case, entry) if align is None else align
    N, Ci, Co, H, W, ups, refl = [case[k] for k in ('N', 'Cin', 'Cout', 'H', 'W', 'ups', 'reflect')]
    e = dict.fromkeys(PLAN_FIELDS, 0)

    def bgemm(nb16, M, cols, K):
        t = o['wino_gemm_tile'] if nb16 else o['w24_gemm_tile']
        if t in (1, 2) and M % 64 == 0 and cols % 128 == 0 and K % 32 == 0:
            e.update(bm=64, bn=128 if t == 1 else 64, nsub=2)
        else:
            e.update(bm=128, bn=128, nsub=2, pipe=2 if o['wino_pipe'] == 2 else 1)

    def w43(K):
        kf = o['w43_kfold'] if (K > 256 or (K > 128 and o['w43_kfold'] == 128)) else 0
        e.update(bm=64, bn=64, nsub=1 if o['w43_nsub'] == 1 else 2, kfold=kf)

    if case['family'] == 'F24':
        p = case['pad']
        OH, OW = H + 2 * p - 3, W + 2 * p - 3
        TH, TW, THd, TWd = _ceil(OH, 2), _ceil(OW, 2), _ceil(H, 2), _ceil(W, 2)
        P, Pd = N * TH * TW, N * THd * TWd
        t = 25 * (Co // 128) * (Ci // 128)
        S = o['w24_s'] if o['w24_s'] > 0 else _ceil(400, t)
        S = max(1, min(S, max(P // 256, 1)))
        Pc = _ceil(_ceil(P, S), 32) * 32
        S = _ceil(P, Pc)
        e.update(form=WF_F24, P=P, Ps=_pad128(P), Pd=Pd, Pds=_pad128(Pd), TH=TH, TW=TW, THd=THd, TWd=TWd, S=S, Pc=Pc)

        def small(n_tiles_rows, C, h, w):
            if not (o['w24_small'] and h * w >= 144 and w <= 64):
                return False
            rows = max(1, _ceil((C // 64) * N * n_tiles_rows, 2048))
            return 64 * ((min(h, 2 * rows + 3) * w) | 1) * 4 <= 65536
        if entry == WINO24_FWD:
            e.update(in_kernel=WK_IN_LDS if small(TH, Ci, H, W) else WK_IN_GENERAL, wt_kernel=WK_WT_PLAIN)
            bgemm(False, Co, e['Ps'], Ci)
        elif entry == WINO24_DGRAD:
            e.update(in_kernel=WK_IN_LDS if small(THd, Co, OH, OW) else WK_IN_GENERAL, wt_kernel=WK_WT_PLAIN)
            bgemm(False, Ci, e['Pds'], Co)
        else:
            e.update(in_kernel=WK_IN_GENERAL, wgrad_src=WSRC_REBUILT)
            bgemm(False, Co, Ci, Pc)
        return e
    LH, LW = H * ups, W * ups
    x16, w16, gy16, gx16 = bool(align & WA_X), bool(align & WA_W), bool(align & WA_GY), bool(align & WA_GX)
    adjoint_shape, f43 = _adjoint_shape(case, o), _f43_shape(case, o)
    if f43:
        P4 = N * (H // 4) * (W // 4)
        e.update(form=WF_F43, P=P4, Ps=P4, Pd=P4, Pds=P4)
        if entry in (WINO_FWD, WINO_FWD_INSTNORM):
            e.update(in_kernel=WK_IN_LDS, wt_kernel=WK_WT_LDS)
            w43(Ci)
            if entry == WINO_FWD_INSTNORM:
                e['norm_tiles'] = 1 if (H // 4) * (W // 4) <= 4 else 4
        elif entry in (WINO_DGRAD, WINO_DGRAD_INSTNORM):
            e.update(in_kernel=WK_IN_LDS, wt_kernel=WK_NONE if saved & WS_UT else WK_WT_LDS, fold_kernel=WK_FOLD_F43)
            w43(Co)
        else:
            sv = (saved & (WS_V | WS_YTP)) == (WS_V | WS_YTP)
            e.update(wgrad_src=WSRC_SAVED if sv else WSRC_REBUILT, in_kernel=WK_NONE if sv else WK_IN_LDS)
            wt = o['w43_wgrad_tile']
            if wt == 1 and P4 % 32 == 0:
                e.update(bm=128, bn=128, nsub=2)
            elif wt == 2 and P4 % 32 == 0:
                e.update(bm=64, bn=128, nsub=2)
            else:
                e.update(bm=64, bn=64, nsub=1 if o['w43_nsub'] == 1 else 2)
        return e
    P = N * (LH // 2) * (LW // 2)
    Pd = N * (LH // 2 + 1) * (LW // 2 + 1) if refl else P
    e.update(form=WF_F23_GENERIC, P=P, Ps=P, Pd=Pd, Pds=_pad128(Pd))
    wt_lds = lambda: WK_WT_LDS if (o['wino_wt'] and w16) else WK_WT_PLAIN
    small = lambda C, ush, a16: WK_IN_LDS if (ush == 0 and LH * LW <= 256 and (LH * LW) % 4 == 0 and C % 64 == 0 and a16) else WK_IN_GENERAL
    if entry == WINO_FWD:
        e.update(wt_kernel=wt_lds(), in_kernel=small(Ci, 1 if ups == 2 else 0, x16))
        bgemm(True, Co, P, Ci)
    elif entry == WINO_DGRAD:
        if adjoint_shape and gy16 and gx16:
            e.update(form=WF_F23_ADJOINT, Pd=P, Pds=P, in_kernel=WK_IN_LDS, wt_kernel=WK_NONE if saved & WS_UT else wt_lds(),
                     fold_kernel=WK_FOLD_CELLS if o['wino_fold_cells'] else WK_FOLD_WALK)
            bgemm(True, P, Ci, Co)
        else:
            e.update(wt_kernel=wt_lds(), in_kernel=small(Co, 0, gy16), fold_kernel=WK_NONE if (not refl and ups == 1) else WK_FOLD_PAD_UPSAMPLE)
            bgemm(True, Ci, e['Pds'], Co)
    else:
        assert entry == WINO_WGRAD, entry
        if (saved & (WS_V | WS_YTP)) == (WS_V | WS_YTP):
            e.update(wgrad_src=WSRC_SAVED, bm=128, bn=128, nsub=2)
        else:
            e.update(wgrad_src=WSRC_REBUILT, in_kernel=WK_IN_GENERAL)
            bgemm(True, Co, Ci, P)
    return e


def plan_values(plan):
    """what the table has to reach: every value of every categorical plan field"""
    return {(k, plan[k]) for k in ('form', 'in_kernel', 'wt_kernel', 'fold_kernel', 'nsub', 'kfold', 'pipe', 'wgrad_src', 'norm_tiles')} | \
           {('tile', plan['bm'], plan['bn']), ('padded', plan['Ps'] > plan['P']), ('padded_d', plan['Pds'] > plan['Pd']),
            ('S', min(plan['S'], 3))}


# every value the header documents for a categorical field
ALL_PLAN_VALUES = (
    {('form', f) for f in (WF_F23_GENERIC, WF_F23_ADJOINT, WF_F43, WF_F24)} | {('in_kernel', k) for k in (WK_NONE, WK_IN_LDS, WK_IN_GENERAL)} |
    {('wt_kernel', k) for k in (WK_NONE, WK_WT_LDS, WK_WT_PLAIN)} |
    {('fold_kernel', k) for k in (WK_NONE, WK_FOLD_CELLS, WK_FOLD_WALK, WK_FOLD_F43, WK_FOLD_PAD_UPSAMPLE)} |
    {('nsub', 1), ('nsub', 2), ('kfold', 0), ('kfold', 128), ('kfold', 256), ('pipe', 0), ('pipe', 1), ('pipe', 2)} |
    {('wgrad_src', 0), ('wgrad_src', WSRC_SAVED), ('wgrad_src', WSRC_REBUILT), ('norm_tiles', 0), ('norm_tiles', 1), ('norm_tiles', 4)} |
    {('tile', 128, 128), ('tile', 64, 128), ('tile', 64, 64), ('padded', False), ('padded', True), ('padded_d', False), ('padded_d', True),
     ('S', 0), ('S', 1), ('S', 2)})


# =============================================================================================
# inputs, references, criteria
# =============================================================================================
def case_inputs(case):
    """fp32 x, w, b, gy"""
    rng = rng_of(case['name'])
    d = case_desc(case)
    return dict(x=f32(rng, (d.N, d.C1, d.H, d.W)), w=f32(rng, (d.Cout, d.C1, d.KS, d.KS), 0.05), b=f32(rng, (d.Cout,)),
                gy=f32(rng, (d.N, d.Cout, d.OH, d.OW)))


def case_form(case, opts=None):
    o = dict(OPTION_DEFAULTS, **case['opts'])
    o.update(opts or {})
    return F24 if case['family'] == 'F24' else (F43 if _f43_shape(case, o) else F23)


def restate(case, form, inp, dtype, which=('y', 'gx', 'gw'), fwd_chunk=0, dgrad_chunk=0, wgrad_chunk=0, mutant=None):
    """the Winograd forms of the case in ``dtype`` from the given matrices: {'y' (without bias), 'gx', 'gw'}.  The data gradient takes
    the form the case's entry runs (case['dgrad_form']).  mutant: see MUTANTS."""
    x, w, gy = [np.asarray(inp[k], dtype=dtype) for k in ('x', 'w', 'gy')]
    KS, p, refl, ups, H, W = case['KS'], case['pad'], case['reflect'], case['ups'], case['H'], case['W']
    OH, OW = gy.shape[2:]
    mu = mutant or {}
    xp = pad_input(x, p, refl, ups, clamp=mu.get('clamp', False))
    out = {}
    if 'y' in which:
        out['y'] = wino_fwd(form, xp, w, OH, OW, fwd_chunk, drop_last=mu.get('drop_fwd', False), shift=mu.get('shift', 0),
                            unclipped=mu.get('unclipped', False))
    if 'gw' in which:
        out['gw'] = wino_wgrad(form, gy, xp, wgrad_chunk, drop_last=mu.get('drop_wgrad', False))
    if 'gx' in which:
        if case['dgrad_form'] in (WF_F43, WF_F23_ADJOINT):
            refl_fn = (lambda i, L: min(max(i, 0), L - 1)) if mu.get('clamp') else _reflect
            out['gx'] = wino_dgrad_adjoint(form, gy, w, dgrad_chunk, drop_last=mu.get('drop_dgrad', False), reflect=refl_fn)
        else:
            # the forward form on the zero-extended gy with the rotated filter, on the padded / upsampled grid, then the fold
            q = KS - 1 - (0 if refl else p)
            GH, GW = H * ups + (2 * p if refl else 0), W * ups + (2 * p if refl else 0)
            gp = wino_fwd(form, np.pad(gy, ((0, 0), (0, 0), (q, q), (q, q))), rot_swap(w), GH, GW, dgrad_chunk)
            if refl or ups == 2:
                if mu.get('upsum'):         # the 2x2 sum-back misses one pixel
                    gp = gp.copy()
                    gp[:, :, 1::2, 1::2] = 0
                gp = fold_pad_upsample(gp, H, W, p if refl else 0, ups)
            out['gx'] = gp
    return out


def direct64(case, inp):
    """the direct float64 convolution and its gradients: y (without bias), gx, gw, gb"""
    x, w, gy = [np.asarray(inp[k], dtype=np.float64) for k in ('x', 'w', 'gy')]
    KS, p, refl, ups, H, W = case['KS'], case['pad'], case['reflect'], case['ups'], case['H'], case['W']
    xp = pad_input(x, p, refl, ups)
    GH, GW = xp.shape[2:]
    g = conv_dgrad_logical(gy, w, 1, 0, GH, GW, 0, w.shape[1])           # gradient of the padded logical grid
    if refl:
        gx = fold_pad_upsample(g, H, W, p, ups)
    else:
        g = g[:, :, p:GH - p, p:GW - p] if p else g
        gx = fold_pad_upsample(g, H, W, 0, ups) if ups == 2 else g
    return dict(y=conv_fwd(xp, w, 1, 0), gx=np.ascontiguousarray(gx), gw=conv_wgrad(gy, xp, KS), gb=bias_grad(gy))


def reduction_lengths(case):
    d = case_desc(case)
    form = case_form(case)
    tiles = d.N * _ceil(d.OH, form.m) * _ceil(d.OW, form.m)
    return dict(y=d.C1, gx=d.Cout, gw=tiles)


@functools.lru_cache(maxsize=None)
def _refs_cached(name, opts_key):
    case = BY_NAME[name]
    inp = case_inputs(case)
    form = case_form(case, dict(opts_key))
    ref = direct64(case, inp)
    absinp = {k: np.abs(v) for k, v in inp.items()}
    babs = restate(case, form.abs(), absinp, np.float64)
    r32 = restate(case, form, inp, np.float32)
    n = reduction_lengths(case)
    out = dict(inp=inp, ref=ref, form=form, n=n)
    for k in ('y', 'gx', 'gw'):
        out[k + '_bound'] = gamma(n[k] + form.c) * babs[k]
        out[k + '_rms32'] = rms(r32[k].astype(np.float64) - ref[k])
        out[k + '_r32'] = r32[k]
    for v in out['ref'].values():
        v.setflags(write=False)
    return out


def case_refs(case, opts=None):
    """inputs, direct float64 references, hard bounds and rms baselines of a case (computed once, read-only); opts only matter where
    they change the FORM (wino43)"""
    o = dict(opts or {})
    key = tuple(sorted((k, v) for k, v in o.items() if k in ('wino43', 'wino_adjoint')))
    return _refs_cached(case['name'], key)


def rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def check(got, ref, bound, rms32, name, note=None, rms_line=True):
    """the hard bound per element and the rms line -> (worst error / bound, rms / baseline); asserts both"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), '%s: non-finite values' % name
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    r = rms(got - ref) / rms32 if rms_line else 0.0
    if note is not None:
        note(name, ratio, r)
    i = int((err / np.maximum(bound, 1e-300)).argmax())
    assert ratio <= 1.0, '%s: error %.3e exceeds the hard bound %.3e (element %d)' % (name, err.reshape(-1)[i], np.asarray(bound).reshape(-1)[i], i)
    if rms_line:
        assert r <= RMS_FACTOR, '%s: rms error %.3e is %.2f x the float32 restatement\'s %.3e (limit %.1f)' % (
            name, rms(got - ref), r, rms32, RMS_FACTOR)
    return ratio, r


def fails(got, ref, bound, rms32):
    try:
        check(got, ref, bound, rms32, 'mutant')
    except AssertionError:
        return True
    return False


# mutants of the float32 restatement: (name, case, restate() arguments, outputs to look at)
def mutants():
    f43_off = F43.with_matrix('AT', 2, 3, F43.AT[2, 3] + 1.0)
    f23_off = F23.with_matrix('BT', 1, 2, F23.BT[1, 2] + 1.0)
    f24_off = F24.with_matrix('G', 3, 2, F24.G[3, 2] + 1.0)
    return (
        ('f43_output_coefficient_off_by_one', 'f43_16_128to128_8x8', dict(form=f43_off), ('y',)),
        ('f23_input_coefficient_off_by_one', 'f23z_2_128to128_16x16', dict(form=f23_off), ('y', 'gw')),
        ('f24_filter_coefficient_off_by_one', 'f24_4_128to128_17x17_p2', dict(form=f24_off), ('y',)),
        ('reflection_replaced_by_clamp', 'f43_64_128to128_4x4', dict(mutant={'clamp': True}), ('y', 'gx', 'gw')),
        ('reflection_replaced_by_clamp_f23', 'f23a_8_128to128_8x8', dict(mutant={'clamp': True}), ('y', 'gx')),
        ('last_tile_column_shifted', 'f43_32_128to128_8x12', dict(mutant={'shift': 1}), ('y',)),
        ('last_chunk_of_forward_sum_dropped', 'f43_16_384to128_8x8', dict(fwd_chunk=256, mutant={'drop_fwd': True}), ('y',)),
        ('last_chunk_of_dgrad_sum_dropped', 'f43_16_128to384_8x8', dict(dgrad_chunk=256, mutant={'drop_dgrad': True}), ('gx',)),
        ('last_k_chunk_of_f24_wgrad_dropped', 'f24_8_128to256_20x14_p1', dict(wgrad_chunk=288, mutant={'drop_wgrad': True}), ('gw',)),
        ('upsample_sum_back_misses_one_pixel', 'f23u_8_128to128_4x4', dict(mutant={'upsum': True}), ('gx',)),
        ('f24_clipped_edge_tile_written_unclipped', 'f24_8_128to256_20x14_p1', dict(mutant={'unclipped': True}), ('y',)),
    )


# =============================================================================================
# one-hot probes
# =============================================================================================
def probe_w_taps(KS):
    return [(kh, kw) for kh in range(KS) for kw in range(KS)]


def reach_mask_fwd(case, site):
    """outputs a one-hot x at ``site`` can reach: the KS x KS neighbourhood through pad / reflection / upsample (a superset of the
    non-zero outputs: exactly the positions whose direct reference is not structurally zero)"""
    n, c, (ih, iw) = site
    d = case_desc(case)
    x = np.zeros((d.N, 1, d.H, d.W))
    x[n, 0, ih, iw] = 1.0
    xp = pad_input(x, case['pad'], case['reflect'], case['ups'])
    y = conv_fwd(xp, np.ones((1, 1, d.KS, d.KS)), 1, 0)
    return y[:, 0] != 0                                                           # [N, OH, OW]
