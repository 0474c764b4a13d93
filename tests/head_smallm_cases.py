"""Case table, input builders, float64 references, rounding bounds and plan restatements of the vector-ALU convolution tests: the
kernels of csrc/smallm.hip behind sg_conv2d_smallm_fwd / _wgrad (ReflectionPad(3) + 7x7, Cout <= 4) and sg_conv2d_head_fwd / _dgrad /
_wgrad (one output channel, zero padding, k 1, 3 or 4, including the 1x1 stream kernel).  Shared by
tests/test_head_smallm_cases_cpu.py (the references agree with torch in float64, the table is self-consistent and reaches every
plan class, the Python restatement of both plans equals the library's queries) and tests/test_gpu_head_smallm.py (every row against
float64 on the device).

NumPy only.  The five operations, restated tap by tap from their definitions (dtype-generic: the probes run them in float32):
    forward   y[n,m,oh,ow]  = act(bias[m] + sum_{c,kh,kw} w[m,c,kh,kw] X[n,c,oh-p+kh,ow-p+kw])      (forward_conv_cases.conv_images)
    wgrad     gw[m,c,kh,kw] = sum_{n,oh,ow} gy[n,m,oh,ow] X[n,c,oh-p+kh,ow-p+kw]                    (wgrad_cases.conv_wgrad)
    dgrad     gx[n,c,h,w]   = sum_{kh,kw} w[0,c,kh,kw] gy[n,0,h+p-kh,w+p-kw]                        (head only: head_dgrad)
X the input plane, mirrored (small-M) or zero (head) outside.

The launch plans come from the library's host-side queries (include/sg2im_hip.h: sg_conv2d_head_plan, sg_conv2d_smallm_plan), the
functions the launchers run from; py_head_plan() / py_smallm_plan() restate them.

Bounds, per element, u = 2^-24, gamma(k) = k u / (1 - k u).  T = C1 * KS^2 products per output; every kernel accumulates by fma from
0 (one rounding per product); c counts the roundings a partial sum passes through after its chain, read from the kernels:
    small-M forward   gamma(T + C_SMALLM_FWD) (sum|w||x| + |bias|)      the exchange add of the two groups' sums, the bias add
    head, staged      gamma(T + C_HEAD_COMBINE + chunks) (...)          (r0 + r1) + (r2 + r3) of the four waves: two adds deep; the
                                                                        finish kernel adds the chunks to the bias one by one
    head, 1x1 stream  gamma(T) (...)                                    the chain starts from the bias: nothing extra
    head dgrad        gamma(KS^2) sum|w||gy|
    small-M wgrad     gamma(n + C_SMALLM_LANES + N) sum|gy||x|          n = N H W products per tap; five xor-shuffle adds over the 32
                                                                        column groups; the image reduce adds N partials to 0
    head wgrad        gamma(n + Q + N) sum|gy||x|                       n = N OH OW; the Q pixel parts of the channel's chunk are added to
                                                                        0 one by one; the image reduce as above
times ACT_LIPSCHITZ[act], plus 1e-6 max(1, |y|) for tanh (as every forward test of the suite)."""
import ctypes

import numpy as np

from scene_generation_amd._hip import CONST, plan_dict, sgHeadPlan, sgSmallmPlan

from dense_pointwise_cases import gamma, rng_of, f32, act_ref, ACT_LIPSCHITZ, ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH  # noqa: F401
from transposed_conv_cases import make_desc, conv_out_size, probe_positions  # noqa: F401  (re-exported)
from wgrad_cases import _reflect, conv_wgrad
from forward_conv_cases import conv_images

HEAD_FWD, HEAD_DGRAD, HEAD_WGRAD = (CONST['SG_HEAD_' + n] for n in ('FWD', 'DGRAD', 'WGRAD'))
HEAD_STREAM, HEAD_STAGED = CONST['SG_HEAD_STREAM'], CONST['SG_HEAD_STAGED']
SMALLM_FWD, SMALLM_WGRAD = CONST['SG_SMALLM_FWD'], CONST['SG_SMALLM_WGRAD']
HEAD_ENTRIES = {'fwd': HEAD_FWD, 'dgrad': HEAD_DGRAD, 'wgrad': HEAD_WGRAD}
SMALLM_ENTRIES = {'fwd': SMALLM_FWD, 'wgrad': SMALLM_WGRAD}
SLOPE = 0.2

# ---- constants of csrc/smallm.hip (tests/test_head_smallm_cases_cpu.py reads them back from the source)
HEAD_LDS_FLOATS = 12288          # 48 KB per workgroup
HEAD_CH_MAX = 16                 # channels per workgroup, at most
HEAD_OW_MAX = 256
HEAD_C1_MIN = 16
HEAD_WGRAD_LDS_MIN = 256         # floats: the Q parts meet in the first 256 floats of the staged planes
STREAM_GROUP = 8                 # channels a stream thread loads together
STREAM_N_MAX = 65535             # images = the grid's y extent
SM_TH, SM_TW = 16, 64            # small-M forward tile (rows x columns)
SM_RB, SM_CB = 16, 128           # small-M weight-gradient block
# ---- roundings behind the fma chain, read from the kernels (module docstring)
C_SMALLM_FWD = 2                 # smallm_fwd_kernel: acc[m][p] += o4 (exchange), acc + b
C_HEAD_COMBINE = 2               # head_fwd_kernel: (red0 + red1) + (red2 + red3)
C_SMALLM_LANES = 5               # smallm_wgrad_kernel: __shfl_xor over o = 16, 8, 4, 2, 1


def _cdiv(a, b):
    return -(-a // b)


# =============================================================================================
# the predicates and the plans, restated (smallm_ok, smallm_plan, head_ok, head_geom, head_plan, HEAD_WGRAD_PARTS of csrc/smallm.hip)
# =============================================================================================
def desc_fields(N, C1, H, W, Cout, KS, pad, reflect, stride=1, ups=1, C2=0, OH=None, OW=None):
    OH = conv_out_size(H * ups, KS, stride, pad) if OH is None else OH
    OW = conv_out_size(W * ups, KS, stride, pad) if OW is None else OW
    return dict(N=N, C1=C1, C2=C2, H=H, W=W, Cout=Cout, KS=KS, stride=stride, pad=pad, reflect=int(bool(reflect)), ups=ups, OH=OH, OW=OW)


def desc_of(f):
    return make_desc(f['N'], f['C1'], f['H'], f['W'], f['Cout'], f['KS'], f['stride'], f['pad'], f['reflect'], f['ups'], f['OH'], f['OW'], C2=f['C2'])


def smallm_supported(f):
    return (f['Cout'] <= 4 and f['KS'] == 7 and f['stride'] == 1 and f['ups'] == 1 and f['C2'] == 0 and bool(f['reflect']) and f['pad'] == 3
            and f['W'] % 4 == 0 and f['H'] >= 4 and f['W'] >= 4 and f['OH'] == f['H'] and f['OW'] == f['W'])


def head_lds_conditions(f):
    """the three LDS inequalities of head_ok -> (forward / weight gradient, channel floor, data gradient)"""
    PP, OP, E, KK = (f['H'] + 2 * f['pad']) * (f['W'] + 2 * f['pad']), f['OH'] * f['OW'], f['KS'] - 1, f['KS'] ** 2
    return (PP + 4 * OP <= HEAD_LDS_FLOATS, f['C1'] >= HEAD_C1_MIN, (f['OH'] + 2 * E) * (f['OW'] + 2 * E) + HEAD_CH_MAX * KK <= HEAD_LDS_FLOATS)


def head_supported(f):
    if f['Cout'] != 1 or f['stride'] != 1 or f['ups'] != 1 or f['C2'] != 0 or f['reflect'] or f['KS'] not in (1, 3, 4):
        return False
    if f['OH'] != f['H'] + 2 * f['pad'] - f['KS'] + 1 or f['OW'] != f['W'] + 2 * f['pad'] - f['KS'] + 1 or f['OW'] > HEAD_OW_MAX:
        return False
    return all(head_lds_conditions(f))


def smallm_ws_bytes(f):
    return f['N'] * f['Cout'] * f['C1'] * 49 * 4 if smallm_supported(f) else 0


def head_chunking(f):
    """(CH, chunks, last_chunk) of the staged kernels"""
    PP, OP = (f['H'] + 2 * f['pad']) * (f['W'] + 2 * f['pad']), f['OH'] * f['OW']
    ch = max(1, min(HEAD_CH_MAX, (HEAD_LDS_FLOATS - 4 * OP) // PP))
    chunks = _cdiv(f['C1'], ch)
    return ch, chunks, f['C1'] - (chunks - 1) * ch


def head_ws_bytes(f):
    if not head_supported(f):
        return 0
    return 4 * max(f['N'] * head_chunking(f)[1] * f['OH'] * f['OW'], f['N'] * f['C1'] * f['KS'] ** 2)


def wgrad_parts(pairs):
    return 1 if pairs >= 128 else 2 if pairs >= 64 else 4 if pairs >= 32 else 8 if pairs >= 16 else 16


def py_smallm_plan(f, entry):
    """-> the dict smallm_plan() returns, or None where the query refuses"""
    if not smallm_supported(f) or entry not in (SMALLM_FWD, SMALLM_WGRAD):
        return None
    MO = 3 if f['Cout'] == 3 else 4
    if entry == SMALLM_FWD:
        return dict(MO=MO, grid_x=_cdiv(f['W'], SM_TW), grid_y=_cdiv(f['H'], SM_TH), grid_z=f['N'], col_blocks=1, row_blocks=1,
                    iters=(f['C1'] + 1) // 2, idle_last=f['C1'] % 2)
    return dict(MO=MO, grid_x=f['C1'], grid_y=f['N'], grid_z=1, col_blocks=_cdiv(f['W'], SM_CB), row_blocks=_cdiv(f['H'], SM_RB), iters=0, idle_last=0)


def py_head_plan(f, entry, x_mod16=0, y_mod16=0):
    """-> the dict head_plan() returns, or None where the query refuses"""
    if not head_supported(f) or entry not in (HEAD_FWD, HEAD_DGRAD, HEAD_WGRAD) or x_mod16 not in (0, 4, 8, 12) or y_mod16 not in (0, 4, 8, 12):
        return None
    KK, PP, OP = f['KS'] ** 2, (f['H'] + 2 * f['pad']) * (f['W'] + 2 * f['pad']), f['OH'] * f['OW']
    CH, chunks, last = head_chunking(f)
    out = dict(kind=HEAD_STAGED, CH=CH, chunks=chunks, last_chunk=last, lds_bytes=0, Q_full=0, Q_last=0)
    if entry == HEAD_FWD:
        if f['KS'] == 1 and f['pad'] == 0 and (f['H'] * f['W']) % 4 == 0 and f['N'] <= STREAM_N_MAX and x_mod16 == 0 and y_mod16 == 0:
            g = _cdiv(f['C1'], STREAM_GROUP)
            out.update(kind=HEAD_STREAM, CH=STREAM_GROUP, chunks=g, last_chunk=f['C1'] - (g - 1) * STREAM_GROUP)
        else:
            out['lds_bytes'] = 4 * (CH * PP + 4 * OP)
    elif entry == HEAD_DGRAD:
        E = f['KS'] - 1
        out['lds_bytes'] = 4 * ((f['OH'] + 2 * E) * (f['OW'] + 2 * E) + CH * KK)
    else:
        out.update(lds_bytes=4 * max(HEAD_WGRAD_LDS_MIN, CH * PP + 2 * OP), Q_full=wgrad_parts(CH * KK), Q_last=wgrad_parts(last * KK))
    return out


def head_plan(lib, desc, entry, x_mod16=0, y_mod16=0):
    """sg_conv2d_head_plan -> dict, or None when the query returns non-zero"""
    p = sgHeadPlan()
    rc = lib.sg_conv2d_head_plan(ctypes.byref(desc), int(entry), int(x_mod16), int(y_mod16), ctypes.byref(p))
    return None if rc else plan_dict(p)


def smallm_plan(lib, desc, entry):
    p = sgSmallmPlan()
    rc = lib.sg_conv2d_smallm_plan(ctypes.byref(desc), int(entry), ctypes.byref(p))
    return None if rc else plan_dict(p)


# =============================================================================================
# the data gradient of the head, restated (the other two operations: conv_images, conv_wgrad)
# =============================================================================================
def head_dgrad(gy, w, pad, H, W):
    """gx[n,c,h,w] = sum_{kh,kw} w[0,c,kh,kw] gy[n,0,h+pad-kh,w+pad-kw], gy zero outside its plane     gy [N,1,OH,OW], w [1,C,KS,KS]"""
    N, _, OH, OW = gy.shape
    C, KS = w.shape[1], w.shape[2]
    gx = np.zeros((N, C, H, W), dtype=gy.dtype)
    for kh in range(KS):
        hs = [h for h in range(H) if 0 <= h + pad - kh < OH]
        for kw in range(KS):
            ws = [v for v in range(W) if 0 <= v + pad - kw < OW]
            if hs and ws:
                g = gy[:, 0][:, [h + pad - kh for h in hs]][:, :, [v + pad - kw for v in ws]]
                gx[np.ix_(range(N), range(C), hs, ws)] += w[0, :, kh, kw][None, :, None, None] * g[:, None]
    return gx


# =============================================================================================
# the case tables
# =============================================================================================
def _sm(name, Cout, C1, N, H, W, act=ACT_NONE, bias=True, claims=None, why=''):
    """a small-M row: forward and weight gradient of ReflectionPad(3) + 7x7 on N x C1 x H x W.  claims: {entry: plan fields}"""
    f = desc_fields(N, C1, H, W, Cout, 7, 3, True)
    return dict(f, name=name, family='smallm', act=act, bias=bias, slope=SLOPE, signed=act in (ACT_RELU, ACT_LEAKY), x_off=0, y_off=0,
                claims=dict(claims or {}), why=why, shape_key='smallm|%d,%d,%d,%d,%d,%d,%d' % (Cout, C1, N, H, W, int(bias), int(act in (ACT_RELU, ACT_LEAKY))))


def _hd(name, KS, pad, C1, N, H, W, act=ACT_NONE, bias=True, x_off=0, y_off=0, claims=None, why=''):
    """a head row: forward, data gradient and weight gradient of a zero-padded KS x KS conv to one channel.  x_off / y_off: floats x / the
    forward's result are offset from a 16-byte boundary.  claims: {entry: plan fields}"""
    f = desc_fields(N, C1, H, W, 1, KS, pad, False)
    return dict(f, name=name, family='head', act=act, bias=bias, slope=SLOPE, signed=act in (ACT_RELU, ACT_LEAKY), x_off=x_off, y_off=y_off,
                claims=dict(claims or {}), why=why, shape_key='head|%d,%d,%d,%d,%d,%d,%d,%d' % (KS, pad, C1, N, H, W, int(bias), int(act in (ACT_RELU, ACT_LEAKY))))


def _fw(**kw):
    return {'fwd': kw}


SMALLM_CASES = [
    _sm('sm_4x4_c1_m1', 1, 1, 1, 4, 4, claims={'fwd': dict(MO=4, grid_x=1, grid_y=1, iters=1, idle_last=1), 'wgrad': dict(MO=4, col_blocks=1, row_blocks=1)},
        why='the minimum plane: the mirror reaches H - 1 and the clamp acts on most of the 22 x 70 staging tile; one channel: the second group '
            'is never live; M = 1 of MO = 4 repeats row 0'),
    _sm('sm_4x4_c2_m2', 2, 2, 3, 4, 4, act=ACT_RELU, claims=_fw(MO=4, iters=1, idle_last=0), why='two channels: one iteration, both groups live; three images'),
    _sm('sm_4x4_c3_m3', 3, 3, 1, 4, 4, act=ACT_TANH, claims=_fw(MO=3, iters=2, idle_last=1), why='MO = 3 on the minimum plane; odd C'),
    _sm('sm_5x8_c5_m4', 4, 5, 3, 5, 8, act=ACT_LEAKY, claims=_fw(MO=4, iters=3, idle_last=1), why='all four rows of MO = 4; C = 5'),
    _sm('sm_5x8_c1_m3', 3, 1, 3, 5, 8, bias=False, claims=_fw(MO=3, iters=1, idle_last=1), why='one channel under MO = 3, null bias'),
    _sm('sm_16x64_c8_m3', 3, 8, 1, 16, 64, act=ACT_TANH, claims={'fwd': dict(MO=3, grid_x=1, grid_y=1, iters=4, idle_last=0), 'wgrad': dict(col_blocks=1, row_blocks=1)},
        why='exactly one forward tile; the RGB head with tanh; an even channel count >= 8'),
    _sm('sm_16x64_c3_m1', 1, 3, 3, 16, 64, claims=_fw(MO=4, grid_x=1, grid_y=1), why='one tile, one output row, three images'),
    _sm('sm_17x68_c5_m3', 3, 5, 1, 17, 68, claims={'fwd': dict(MO=3, grid_x=2, grid_y=2, idle_last=1), 'wgrad': dict(col_blocks=1, row_blocks=2)},
        why='one row and four columns into a second tile on each axis'),
    _sm('sm_17x68_c2_m4', 4, 2, 3, 17, 68, act=ACT_RELU, bias=False, claims=_fw(MO=4, grid_x=2, grid_y=2), why='the same plane, MO = 4, null bias'),
    _sm('sm_21x20_c3_m2', 2, 3, 3, 21, 20, act=ACT_LEAKY, claims=_fw(MO=4, grid_x=1, grid_y=2), why='five rows into a second row tile; M = 2'),
    _sm('sm_21x20_c8_m4', 4, 8, 1, 21, 20, claims=_fw(MO=4, iters=4, idle_last=0), why='eight channels, four rows'),
    _sm('sm_17x132_c5_m3', 3, 5, 3, 17, 132, act=ACT_TANH, claims={'fwd': dict(grid_x=3, grid_y=2), 'wgrad': dict(MO=3, col_blocks=2, row_blocks=2)},
        why='W = 132: the weight gradient walks a second column block of four columns and a second row block of one row'),
    _sm('sm_17x132_c2_m1', 1, 2, 1, 17, 132, bias=False, claims={'wgrad': dict(MO=4, col_blocks=2, row_blocks=2)}, why='the same blocks under MO = 4 with one row'),
]

_ST = dict(kind=HEAD_STREAM, CH=STREAM_GROUP)
HEAD_CASES = [
    # ---- the 1x1 stream kernel ---------------------------------------------------------------------------------------------------
    _hd('h1_stream_c16', 1, 0, 16, 1, 4, 6, claims=_fw(chunks=2, last_chunk=8, **_ST), why='two full groups of eight channels'),
    _hd('h1_stream_c17', 1, 0, 17, 3, 4, 6, act=ACT_RELU, claims=_fw(chunks=3, last_chunk=1, **_ST), why='a ragged group of eight: one channel'),
    _hd('h1_stream_c24', 1, 0, 24, 1, 2, 10, act=ACT_TANH, bias=False, claims=_fw(chunks=3, last_chunk=8, **_ST), why='24 channels, null bias'),
    _hd('h1_stream_c29', 1, 0, 29, 3, 6, 6, act=ACT_LEAKY, claims=_fw(chunks=4, last_chunk=5, **_ST), why='no multiple of 8 beyond 24'),
    _hd('h1_stream_1x256', 1, 0, 16, 1, 1, 256, claims=_fw(**_ST), why='OW = 256, the widest map head_ok takes'),
    # ---- 1x1, each reason the stream kernel is declined ----------------------------------------------------------------------------
    _hd('h1_staged_3x5', 1, 0, 17, 3, 3, 5, claims=_fw(kind=HEAD_STAGED, CH=16, chunks=2, last_chunk=1), why='H*W = 15 is no multiple of 4'),
    _hd('h1_staged_pad1', 1, 1, 16, 1, 4, 6, claims=_fw(kind=HEAD_STAGED, CH=16, chunks=1, last_chunk=16), why='pad 1: a border ring of bias alone'),
    _hd('h1_staged_x_off', 1, 0, 16, 1, 4, 6, x_off=1, claims=_fw(kind=HEAD_STAGED), why='x 4 bytes off a 16-byte boundary'),
    _hd('h1_staged_y_off', 1, 0, 16, 1, 4, 6, y_off=1, claims=_fw(kind=HEAD_STAGED), why='y 4 bytes off a 16-byte boundary'),
    _hd('h1_1x1_map', 1, 0, 16, 3, 1, 1, claims={'fwd': dict(kind=HEAD_STAGED), 'wgrad': dict(lds_bytes=4 * HEAD_WGRAD_LDS_MIN, Q_full=8)},
        why='a 1x1 map: 16 + 2 staged floats, the weight gradient asks for 256'),
    # ---- 3x3 ----------------------------------------------------------------------------------------------------------------------------
    _hd('k3p0_5x7', 3, 0, 16, 1, 5, 7, claims={'fwd': dict(kind=HEAD_STAGED, CH=16, chunks=1), 'wgrad': dict(Q_full=1, Q_last=1)},
        why='pad 0: border pixels of gx see fewer taps; OP = 15 < 64; one full chunk'),
    _hd('k3p1_7x9_c17', 3, 1, 17, 3, 7, 9, act=ACT_LEAKY, claims={'fwd': dict(CH=16, chunks=2, last_chunk=1), 'wgrad': dict(Q_full=1, Q_last=16)},
        why='a last chunk of one channel: waves 1-3 have none; OP = 63'),
    _hd('k3p1_9x11_c40', 3, 1, 40, 1, 9, 11, act=ACT_TANH, claims={'fwd': dict(CH=16, chunks=3, last_chunk=8), 'wgrad': dict(Q_last=2)},
        why='16 + 16 + 8 channels; OP = 99, no multiple of 64'),
    _hd('k3p1_6x5_c20', 3, 1, 20, 1, 6, 5, bias=False, claims={'wgrad': dict(Q_full=1, Q_last=4)}, why='a last chunk of four channels'),
    _hd('k3p1_5x6_c18', 3, 1, 18, 3, 5, 6, act=ACT_RELU, claims={'wgrad': dict(Q_full=1, Q_last=8)}, why='a last chunk of two channels'),
    _hd('k3p2_5x6_c24', 3, 2, 24, 1, 5, 6, claims={'fwd': dict(CH=16, last_chunk=8)}, why='pad 2 = KS - 1: every output sees at least one input'),
    _hd('k3p3_4x5_c20', 3, 3, 20, 3, 4, 5, claims={'fwd': dict(CH=16, last_chunk=4)}, why='pad 3 > KS - 1: a border ring of outputs is bias alone'),
    _hd('k3p1_28x32_c20', 3, 1, 20, 1, 28, 32, claims={'fwd': dict(CH=8, chunks=3, last_chunk=4), 'wgrad': dict(Q_full=2, Q_last=4)},
        why='the LDS budget gives CH = 8: 72 pairs, Q = 2 for a full chunk'),
    _hd('k3p1_32x36_c16', 3, 1, 16, 1, 32, 36, claims={'fwd': dict(CH=5, chunks=4, last_chunk=1), 'wgrad': dict(Q_full=4, Q_last=16)},
        why='CH = 5: 45 pairs, Q = 4 for a full chunk'),
    _hd('k3p1_40x40_c17', 3, 1, 17, 1, 40, 40, claims={'fwd': dict(CH=3, chunks=6, last_chunk=2), 'wgrad': dict(Q_full=8, Q_last=8)},
        why='CH = 3 from the LDS budget: 27 pairs, Q = 8'),
    _hd('k3p1_48x48_c18', 3, 1, 18, 1, 48, 48, claims={'fwd': dict(CH=1, chunks=18, last_chunk=1), 'wgrad': dict(Q_full=16, Q_last=16)},
        why='CH = 1: waves 1-3 never have a channel'),
    _hd('k3p1_49x49_c16', 3, 1, 16, 1, 49, 49, claims={'fwd': dict(CH=1, chunks=16)}, why='PP + 4 OP = 12205 <= 12288: the largest square k3 pad 1 plane'),
    _hd('k3p1_1x1_map', 3, 1, 16, 3, 1, 1, claims={'fwd': dict(CH=16), 'wgrad': dict(lds_bytes=4 * HEAD_WGRAD_LDS_MIN, Q_full=1)},
        why='a 1x1 map under 3x3: eight of nine taps outside; 16 * 9 + 2 staged floats, the weight gradient asks for 256'),
    _hd('k3p1_2x256_c16', 3, 1, 16, 1, 2, 256, claims={'fwd': dict(CH=9, chunks=2, last_chunk=7)}, why='OW = 256 on the staged path'),
    # ---- 4x4 ----------------------------------------------------------------------------------------------------------------------------
    _hd('k4p0_4x4_c16', 4, 0, 16, 3, 4, 4, claims={'fwd': dict(CH=16, chunks=1), 'wgrad': dict(Q_full=1, Q_last=1)}, why='one output per image'),
    _hd('k4p1_6x7_c20', 4, 1, 20, 1, 6, 7, act=ACT_LEAKY, claims={'wgrad': dict(Q_full=1, Q_last=2)}, why='a last chunk of four channels: 64 pairs'),
    _hd('k4p2_5x7_c18', 4, 2, 18, 3, 5, 7, claims={'wgrad': dict(Q_full=1, Q_last=4)}, why='the PatchGAN padding; a last chunk of two'),
    _hd('k4p3_4x6_c17', 4, 3, 17, 1, 4, 6, bias=False, claims={'wgrad': dict(Q_full=1, Q_last=8)}, why='pad 3 = KS - 1; a last chunk of one; OP = 63'),
    _hd('k4p4_3x5_c32', 4, 4, 32, 1, 3, 5, claims={'fwd': dict(chunks=2, last_chunk=16)}, why='pad 4 > KS - 1: a ring of bias alone; two full chunks'),
    _hd('k4p2_36x40_c17', 4, 2, 17, 1, 36, 40, claims={'fwd': dict(CH=3, chunks=6, last_chunk=2), 'wgrad': dict(Q_full=4, Q_last=4)},
        why='CH = 3 under 4x4: 48 pairs, Q = 4'),
]
CASES = SMALLM_CASES + HEAD_CASES
BY_NAME = dict((c['name'], c) for c in CASES)
assert len(BY_NAME) == len(CASES)
# the rows the operator-level test runs through ops.conv2d
OPERATOR_ROWS = ('sm_16x64_c8_m3', 'sm_21x20_c3_m2', 'h1_stream_c17', 'k3p1_7x9_c17', 'k4p2_5x7_c18')


def case_entries(case):
    return ('fwd', 'wgrad') if case['family'] == 'smallm' else ('fwd', 'dgrad', 'wgrad')


def case_py_plan(case, entry, x_mod16=None, y_mod16=None):
    if case['family'] == 'smallm':
        return py_smallm_plan(case, SMALLM_ENTRIES[entry])
    return py_head_plan(case, HEAD_ENTRIES[entry], 4 * case['x_off'] if x_mod16 is None else x_mod16, 4 * case['y_off'] if y_mod16 is None else y_mod16)


def case_lib_plan(lib, case, entry, x_mod16=None, y_mod16=None):
    d = desc_of(case)
    if case['family'] == 'smallm':
        return smallm_plan(lib, d, SMALLM_ENTRIES[entry])
    return head_plan(lib, d, HEAD_ENTRIES[entry], 4 * case['x_off'] if x_mod16 is None else x_mod16, 4 * case['y_off'] if y_mod16 is None else y_mod16)


def case_ws_bytes(case):
    return smallm_ws_bytes(case) if case['family'] == 'smallm' else head_ws_bytes(case)


_INPUTS, _REFS = {}, {}


def case_inputs(case):
    """deterministic operands of the row's shape (shared by the rows of one shape; never modified).  ReLU / LeakyReLU rows: x > 0 and
    every weight row and its bias of one sign (alternating by output channel), so that |pre| = sum|w||x| + |bias| stays far from 0"""
    k = case['shape_key']
    if k not in _INPUTS:
        rng = rng_of(k)
        N, C, H, W, M, KS = case['N'], case['C1'], case['H'], case['W'], case['Cout'], case['KS']
        inp = dict(x=f32(rng, (N, C, H, W)), w=f32(rng, (M, C, KS, KS), 0.5), b=f32(rng, (M,), 0.5) if case['bias'] else None,
                   gy=f32(rng, (N, M, case['OH'], case['OW'])))
        if case['signed']:
            sign = np.where(np.arange(M) % 2 == 0, 1.0, -1.0).astype(np.float32)
            inp['x'] = np.abs(inp['x']) + np.float32(0.125)
            inp['w'] = np.abs(inp['w']) * sign[:, None, None, None]
            if inp['b'] is not None:
                inp['b'] = (np.abs(inp['b']) + np.float32(0.125)) * sign
        _INPUTS[k] = inp
    return _INPUTS[k]


def restate_fwd(case, x, w):
    return conv_images(x, w[None], case['KS'], 1, case['pad'], bool(case['reflect']), 1, case['OH'], case['OW'])


def restate_wgrad(case, gy, x):
    return conv_wgrad(gy, x, case['KS'], 1, case['pad'], bool(case['reflect']), 1)


def restate_dgrad(case, gy, w):
    return head_dgrad(gy, w, case['pad'], case['H'], case['W'])


def case_refs(case):
    """float64: y (and its pre-activation), gw, gx (head) with the absolute sums (``*_sabs``) and the term counts (``*_terms``: the
    operation on ones) their bounds are made of"""
    k = case['shape_key'] + '|%d' % case['act']
    if k not in _REFS:
        inp = case_inputs(case)
        x, w, gy = (inp[n].astype(np.float64) for n in ('x', 'w', 'gy'))
        b = np.zeros(case['Cout']) if inp['b'] is None else inp['b'].astype(np.float64)
        pre = restate_fwd(case, x, w) + b[None, :, None, None]
        r = dict(pre=pre, y=act_ref(pre, case['act'], case['slope']), y_sabs=restate_fwd(case, np.abs(x), np.abs(w)) + np.abs(b)[None, :, None, None],
                 gw=restate_wgrad(case, gy, x), gw_sabs=restate_wgrad(case, np.abs(gy), np.abs(x)), gw_terms=restate_wgrad(case, np.ones_like(gy), np.ones_like(x)))
        if case['family'] == 'head':
            r.update(gx=restate_dgrad(case, gy, w), gx_sabs=restate_dgrad(case, np.abs(gy), np.abs(w)), gx_terms=restate_dgrad(case, np.ones_like(gy), np.ones_like(w)))
        _REFS[k] = r
    return _REFS[k]


def _act_bound(case, pre_bound, y):
    b = ACT_LIPSCHITZ[case['act']] * pre_bound
    return b + 1e-6 * np.maximum(1.0, np.abs(y)) if case['act'] == ACT_TANH else b


def y_bound(case, plan):
    """bound of the forward under the reported plan (module docstring)"""
    r, T = case_refs(case), case['C1'] * case['KS'] ** 2
    if case['family'] == 'smallm':
        c = C_SMALLM_FWD
    else:
        c = 0 if plan['kind'] == HEAD_STREAM else C_HEAD_COMBINE + plan['chunks']
    return _act_bound(case, gamma(T + c) * r['y_sabs'], r['y'])


def gx_bound(case):
    return gamma(case['KS'] ** 2) * case_refs(case)['gx_sabs']


def gw_bound(case, plan):
    r = case_refs(case)
    if case['family'] == 'smallm':
        return gamma(case['N'] * case['H'] * case['W'] + C_SMALLM_LANES + case['N']) * r['gw_sabs']
    q = np.full(case['C1'], plan['Q_full'])
    q[(plan['chunks'] - 1) * plan['CH']:] = plan['Q_last']
    return gamma(case['N'] * case['OH'] * case['OW'] + q + case['N'])[None, :, None, None] * r['gw_sabs']


# =============================================================================================
# plan classes the table must reach (tests/test_head_smallm_cases_cpu.py and the device module check the union over the rows)
# =============================================================================================
def plan_classes(case, plans):
    """plans: {entry: reported plan}"""
    out = set()
    if case['family'] == 'smallm':
        f, g = plans['fwd'], plans['wgrad']
        out.add(('MO', f['MO']))
        out.add(('second_group', 'idle' if f['idle_last'] else 'live'))
        if case['C1'] == 1:
            out.add(('second_group', 'never'))
        out.add(('fwd_cols', 'one' if f['grid_x'] == 1 else 'several'))
        out.add(('fwd_rows', 'one' if f['grid_y'] == 1 else 'several'))
        out.add(('wgrad_cols', 'one' if g['col_blocks'] == 1 else 'several'))
        out.add(('wgrad_rows', 'one' if g['row_blocks'] == 1 else 'several'))
        out.add(('images', 'one' if case['N'] == 1 else 'several'))
        out.add(('M', case['Cout']))
    else:
        f, g = plans['fwd'], plans['wgrad']
        out.add(('kind', f['kind']))
        if f['kind'] == HEAD_STAGED:
            out.add(('CH', 1 if f['CH'] == 1 else (16 if f['CH'] == 16 else '2..15')))
            out.add(('last_chunk', 'full' if f['last_chunk'] == f['CH'] else 'ragged'))
            out.add(('OP', '<64' if case['OH'] * case['OW'] < 64 else ('%64' if (case['OH'] * case['OW']) % 64 else '64n')))
        out.add(('Q_full', g['Q_full']))
        out.add(('Q_last', g['Q_last']))
        out.add(('ks_pad', case['KS'], case['pad']))
        if g['lds_bytes'] == 4 * HEAD_WGRAD_LDS_MIN:
            out.add(('wgrad_lds', 'raised'))
        out.add(('images', 'one' if case['N'] == 1 else 'several'))
    return out


REQUIRED_CLASSES = (
    [('MO', 3), ('MO', 4), ('second_group', 'idle'), ('second_group', 'live'), ('second_group', 'never')] +
    [(a, v) for a in ('fwd_cols', 'fwd_rows', 'wgrad_cols', 'wgrad_rows', 'images') for v in ('one', 'several')] + [('M', m) for m in (1, 2, 3, 4)] +
    [('kind', HEAD_STREAM), ('kind', HEAD_STAGED), ('CH', 1), ('CH', '2..15'), ('CH', 16), ('last_chunk', 'full'), ('last_chunk', 'ragged'),
     ('OP', '<64'), ('OP', '%64'), ('wgrad_lds', 'raised')] +
    [('Q_full', q) for q in (1, 2, 4, 8, 16)] + [('Q_last', q) for q in (1, 2, 4, 8, 16)] +
    [('ks_pad', 1, 0), ('ks_pad', 1, 1)] + [('ks_pad', 3, p) for p in (0, 1, 2, 3)] + [('ks_pad', 4, p) for p in (0, 1, 2, 3, 4)])


# =============================================================================================
# both sides of every inequality of the two predicates: (name, desc fields, supported)
# =============================================================================================
def _h(KS, pad, C1, H, W, **kw):
    return desc_fields(kw.pop('N', 1), C1, H, W, kw.pop('Cout', 1), KS, pad, kw.pop('reflect', False), **kw)


def _s(Cout, C1, H, W, **kw):
    return desc_fields(kw.pop('N', 1), C1, H, W, Cout, kw.pop('KS', 7), kw.pop('pad', 3), kw.pop('reflect', True), **kw)


HEAD_EDGES = [
    ('k3p1 49x49: PP + 4 OP = 12205', _h(3, 1, 16, 49, 49), True), ('k3p1 50x50: PP + 4 OP = 12704', _h(3, 1, 16, 50, 50), False),
    ('k3p1 49x50: 12452', _h(3, 1, 16, 49, 50), False), ('k3p1 48x50: 12200', _h(3, 1, 16, 48, 50), True),
    ('k4p2 47x47: 2601 + 4 * 2304 = 11817', _h(4, 2, 16, 47, 47), True), ('k4p2 48x48: 2704 + 4 * 2401 = 12308', _h(4, 2, 16, 48, 48), False),
    ('k1p0 49x50: 5 * 2450 = 12250', _h(1, 0, 16, 49, 50), True), ('k1p0 50x50: 12500', _h(1, 0, 16, 50, 50), False),
    ('OW = 256', _h(1, 0, 16, 1, 256), True), ('OW = 257', _h(1, 0, 16, 1, 257), False),
    ('k3p1 OW = 256', _h(3, 1, 16, 2, 256), True), ('k3p1 OW = 257', _h(3, 1, 16, 2, 257), False),
    ('C1 = 16', _h(3, 1, 16, 5, 6), True), ('C1 = 15', _h(3, 1, 15, 5, 6), False),
    ('k = 2', _h(2, 0, 16, 5, 6), False), ('k = 5', _h(5, 2, 16, 5, 6), False), ('k = 7', _h(7, 3, 16, 8, 8), False),
    ('stride 2', _h(3, 1, 16, 6, 6, stride=2), False), ('a second source', _h(3, 1, 16, 5, 6, C2=4), False),
    ('reflect padding', _h(3, 1, 16, 5, 6, reflect=True), False), ('upsample 2', _h(3, 1, 16, 5, 6, ups=2), False),
    ('two output channels', _h(3, 1, 16, 5, 6, Cout=2), False), ('OH that is not the conv\'s', _h(3, 1, 16, 5, 6, OH=6), False),
    ('OW that is not the conv\'s', _h(3, 1, 16, 5, 6, OW=5), False),
]
SMALLM_EDGES = [
    ('4x4', _s(3, 3, 4, 4), True), ('W = 6', _s(3, 3, 4, 6), False), ('W = 7', _s(3, 3, 8, 7), False), ('H = 3', _s(3, 3, 3, 4), False),
    ('W = 3', _s(3, 3, 4, 3), False), ('H = 5', _s(3, 3, 5, 4), True), ('Cout 4', _s(4, 3, 4, 4), True), ('Cout 5', _s(5, 3, 4, 4), False),
    ('k 5', _s(3, 3, 8, 8, KS=5, pad=2), False), ('pad 2', _s(3, 3, 8, 8, pad=2), False), ('zero padding', _s(3, 3, 8, 8, reflect=False), False),
    ('upsample 2', _s(3, 3, 4, 4, ups=2), False), ('stride 2', _s(3, 3, 8, 8, stride=2), False), ('a second source', _s(3, 3, 4, 4, C2=2), False),
    ('OH that is not H', _s(3, 3, 8, 8, OH=7), False),
]


# =============================================================================================
# one-hot probes: placement by index arithmetic alone
# =============================================================================================
PROBES = [
    _sm('p_sm_5x8_m4', 4, 3, 2, 5, 8, bias=False), _sm('p_sm_6x12_m3', 3, 3, 2, 6, 12, bias=False), _sm('p_sm_17x68_m2', 2, 3, 1, 17, 68, bias=False),
    _hd('p_h1_stream', 1, 0, 17, 2, 3, 4, bias=False), _hd('p_h1_staged', 1, 1, 17, 2, 3, 5, bias=False),
    _hd('p_k3p1', 3, 1, 17, 2, 5, 7, bias=False), _hd('p_k3p0', 3, 0, 20, 2, 5, 7, bias=False), _hd('p_k3p3', 3, 3, 16, 1, 3, 4, bias=False),
    _hd('p_k4p2', 4, 2, 18, 2, 5, 6, bias=False), _hd('p_k4p0', 4, 0, 16, 1, 5, 7, bias=False), _hd('p_k3p1_ch3', 3, 1, 17, 1, 40, 38, bias=False),
]


def probe_taps(case):
    """[(c, kh, kw)]: every tap at least once (a 1x1 kernel: its one tap eight times), the channel stepping by 7 so that first and
    last (t = 1: the ragged last chunk), even and odd channels and every wave of a head workgroup (c mod 4) are selected"""
    KS, C = case['KS'], case['C1']
    n = max(KS * KS, 8)
    return [(C - 1 if t == 1 else (t * 7 + t // 3) % C, (t % (KS * KS)) // KS, t % KS) for t in range(n)]


def _src(case, o, k, L):
    """the input coordinate output position o reads at tap k on an axis of length L, or None (zero padding, outside)"""
    i = o - case['pad'] + k
    if case['reflect']:
        return _reflect(i, L)
    return i if 0 <= i < L else None


def place_fwd(case, x, sel):
    """y for weights that are 1.0 at (m, c, kh, kw) for every m, (c, kh, kw) = sel[m]: a mirrored / zero-padded copy of plane c of x"""
    N, H, W = x.shape[0], case['H'], case['W']
    y = np.zeros((N, len(sel), case['OH'], case['OW']), dtype=np.float32)
    for m, (c, kh, kw) in enumerate(sel):
        for oh in range(case['OH']):
            ih = _src(case, oh, kh, H)
            for ow in range(case['OW']):
                iw = _src(case, ow, kw, W)
                if ih is not None and iw is not None:
                    y[:, m, oh, ow] = x[:, c, ih, iw]
    return y


def place_dgrad(case, gy, c, kh, kw):
    """gx of the head for a weight that is 1.0 at (c, kh, kw): channel c is gy placed at (h, w) = (oh - pad + kh, ow - pad + kw), the rest 0"""
    gx = np.zeros((gy.shape[0], case['C1'], case['H'], case['W']), dtype=np.float32)
    for oh in range(case['OH']):
        for ow in range(case['OW']):
            h, v = oh - case['pad'] + kh, ow - case['pad'] + kw
            if 0 <= h < case['H'] and 0 <= v < case['W']:
                gx[:, c, h, v] = gy[:, 0, oh, ow]
    return gx


def place_wgrad(case, x, site):
    """gw for a gy that is 1.0 at site = (n, m, (oh, ow)): row m holds the window of image n around (oh, ow), the other rows 0"""
    n, m, (oh, ow) = site
    KS = case['KS']
    gw = np.zeros((case['Cout'], case['C1'], KS, KS), dtype=np.float32)
    for kh in range(KS):
        ih = _src(case, oh, kh, case['H'])
        for kw in range(KS):
            iw = _src(case, ow, kw, case['W'])
            if ih is not None and iw is not None:
                gw[m, :, kh, kw] = x[n, :, ih, iw]
    return gw


def probe_sites(case):
    """(image, output channel, (row, col)) of the one-hot gy: corners, edge middles and an interior pixel, cycling image and channel"""
    return [(i % case['N'], i % case['Cout'], pos) for i, pos in enumerate(probe_positions(case['OH'], case['OW']))]
