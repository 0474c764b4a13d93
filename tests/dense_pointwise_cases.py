"""Case tables, input builders and float64 references of the dense-layer (csrc/skinny.hip, the run_dense configurations of
csrc/igemm.hip) and pooling / padding / pointwise (csrc/norm.hip, csrc/loss.hip, the fold kernels of csrc/igemm.hip) kernel tests,
shared by tests/test_dense_pointwise_cases_cpu.py (the tables reach every launch plan, the references agree with an independent
formulation, the adjoint pairs are adjoint) and tests/test_gpu_dense_pointwise.py (every case against float64 on the device).

The dense launch plans come from the library's own host-side query (include/sg2im_hip.h: sg_linear_plan) -- the function the
three entry points launch from -- so a table entry names a kernel form by shape and operand alignment alone.
"""
import ctypes
import zlib

import numpy as np

from scene_generation_amd._hip import CONST

from norm_cases import option  # noqa: F401  (re-exported: the option context manager)

# ---- kernel constants the tables are built around (tests/test_dense_pointwise_cases_cpu.py reads them back from the sources)
SK_TILE = 32            # skinny.hip: one workgroup per 32 x 32 output tile
SK_CHUNK = 16           # k values per chunk (8 per half-wave)
SK_ROUND = 4            # chunks per round
SK_WAVES = 4            # the waves of a workgroup split K
BK = 16                 # igemm_core.h: sub-tile depth of the LDS-tiled kernel
GRID_Y_MAX = 65535      # sg_pad_upsample_bwd: planes per launch
PLANES_PER_BLOCK = 4    # gap_fwd_kernel / cond_window_sums_kernel: one wave per plane, 256 threads
U = 2.0 ** -24          # unit roundoff of fp32

# include/sg2im_hip.h, under the short names the tables use
LINEAR_FWD, LINEAR_BWD_DATA, LINEAR_BWD_WEIGHT = (CONST['SG_LINEAR_' + n] for n in ('FWD', 'BWD_DATA', 'BWD_WEIGHT'))
ENTRY_NAMES = {LINEAR_FWD: 'fwd', LINEAR_BWD_DATA: 'bwd_data', LINEAR_BWD_WEIGHT: 'bwd_weight'}
LIN_SKINNY, LIN_TILED = CONST['SG_LIN_SKINNY'], CONST['SG_LIN_TILED']
LIN_ROWMAJOR, LIN_KSCALAR, LIN_KVEC = (CONST['SG_LIN_' + n] for n in ('ROWMAJOR', 'KSCALAR', 'KVEC'))
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH, ACT_SIGMOID = (CONST['SG_ACT_' + n] for n in ('NONE', 'RELU', 'LEAKY', 'TANH', 'SIGMOID'))
ACTS = (ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_TANH, ACT_SIGMOID)
ACT_LIPSCHITZ = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_LEAKY: 1.0, ACT_TANH: 1.0, ACT_SIGMOID: 0.25}

SKINNY_ALWAYS, SKINNY_NEVER = 1 << 30, 0      # values of the option linear_skinny that force one kernel
KERNELS = (('skinny', SKINNY_ALWAYS), ('tiled', SKINNY_NEVER))
NSUB_VALUES = (2, 1)
ALIGN_OF_OFFSET = {0: 16, 2: 8, 1: 4, 3: 4}    # float offset into a 16-byte aligned buffer -> alignment of the address


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative error bound of n fp32 roundings in sequence"""
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def rng_of(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def f32(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


# =============================================================================================
# dense layers
# =============================================================================================
def _ptr(v):
    return ctypes.cast(ctypes.pointer(v), ctypes.c_void_p)


def linear_plan(lib, entry, rows, in_f, out_f, a_align, b_align):
    """-> (kind, a_form, b_form, bm, bn, nsub) of sg_linear_plan under the current options linear_skinny / linear_nsub"""
    v = [ctypes.c_int(-1) for _ in range(6)]
    rc = lib.sg_linear_plan(int(entry), int(rows), int(in_f), int(out_f), int(a_align), int(b_align), *[_ptr(x) for x in v])
    assert rc == 0, rc
    return tuple(x.value for x in v)


def gemm_dims(entry, rows, in_f, out_f):
    """(M, N, K) of the entry point's GEMM C[M][N] = sum_k A(m, k) B(n, k)"""
    if entry == LINEAR_FWD:
        return rows, out_f, in_f
    if entry == LINEAR_BWD_DATA:
        return rows, in_f, out_f
    return out_f, in_f, rows


def skinny_wave_chunks(K):
    """16-deep chunks each of the four waves of the skinny kernel owns"""
    chunks = -(-K // SK_CHUNK)
    per, extra = divmod(chunks, SK_WAVES)
    return [per + (1 if w < extra else 0) for w in range(SK_WAVES)]


def operand_aligns(entry, case):
    """alignment in bytes of the addresses of the GEMM's A and B operands for a table row"""
    ox, ow, og = case['offs']
    if entry == LINEAR_FWD:
        return ALIGN_OF_OFFSET[ox], ALIGN_OF_OFFSET[ow]
    if entry == LINEAR_BWD_DATA:
        return ALIGN_OF_OFFSET[og], ALIGN_OF_OFFSET[ow]
    return ALIGN_OF_OFFSET[og], ALIGN_OF_OFFSET[ox]


def plan_class(entry, plan):
    """what distinguishes two launches as code paths: the entry point and the whole plan"""
    return (entry,) + tuple(plan)


def plan_kernel_pattern(entry, plan):
    """regular expression the demangled name of the kernel the plan launches must match"""
    kind, a, b, bm, bn, nsub = plan
    if kind == LIN_SKINNY:
        return r'skinny_gemm_kernel<%d, %d>' % (a, b)

    def loader(form, bx):
        if form == LIN_ROWMAJOR:
            return r'LoadXContig<%d>' % bx
        return r'LoadKContig<%d, %s, true>' % (bx, 'true' if form == LIN_KVEC else 'false')
    wgm = 1 if bm == 32 else 2
    return (r'igemm_kernel<TileCfg<%d, %d, %d, %d, \d+, 0, 1>, %s, %s, EpRowMajor>'
            % (bm, bn, wgm, nsub, loader(a, bm), loader(b, bn)))


def _case(name, rows, in_f, out_f, offs=(0, 0, 0), act=ACT_NONE, bias=True, gb=True, slope=0.2, why=''):
    return dict(name=name, rows=rows, in_f=in_f, out_f=out_f, offs=tuple(offs), act=act, bias=bias, gb=gb, slope=slope, why=why)


# K edges of the skinny kernel's split.  chunks = ceil(K / 16) are dealt to four waves, which run rounds of four chunks with
# two register buffers: per-wave counts of 0 (idle wave), 1, exactly one round (4), one round + 1 (5), two rounds (8), two + 1
# (9), three + 1 (13); chunks % 4 of 1, 2, 3; K % 4 == 0, K % 2 == 0 and odd K (the 16 / 8 / 4-byte loaders).
SKINNY_K_EDGES = (1, 7, 15, 16, 17, 48, 64, 65, 100, 256, 260, 288, 300, 512, 514, 777)
# K edges of the tiled loaders: below one sub-tile, one sub-tile, 60 (vector, below 64: depth 16 even at nsub = 2), 63, 64, a vector
# tail in the first (68) and in the second (84) 16-deep sub-tile of a 32-deep k-tile, scalar tails
TILED_K_EDGES = (4, 16, 60, 63, 64, 68, 84, 100, 130, 257)
K_EDGES = tuple(sorted(set(SKINNY_K_EDGES + TILED_K_EDGES)))
MN_EDGES = (1, 31, 32, 33, 64, 65, 129)


def _build_dense_cases():
    cases = []
    # ---- M, N edges: ragged and full 32 / 64 / 128 tiles in both output dimensions.  rows x out_f is the forward's tile grid,
    # rows x in_f the data gradient's, out_f x in_f the weight gradient's.
    for i, m in enumerate(MN_EDGES):
        n = MN_EDGES[(i + 3) % len(MN_EDGES)]
        k = MN_EDGES[(i + 5) % len(MN_EDGES)]
        cases.append(_case('mn_%d_%d_%d' % (m, k, n), m, k, n, why='M / N tile edges'))
    cases += [
        _case('m32_n257', 32, 64, 257, why='M <= 32 with N > 128: two 32x128 column tiles, the second ragged'),
        _case('m1_n130_k68', 1, 68, 130, why='one row, N > 128, vector tail'),
        _case('m129_n129', 129, 40, 129, why='M > 32: 3 x 3 64x64 tiles, 5 x 5 skinny tiles'),
        _case('wgrad_32x128_two_xcontig', 70, 40, 24, why='weight gradient with out_f <= 32 and rows >= 64: TileCfg<32, 128, 1, 2> '
              'with two row-index-major loaders; in_f > 32: only the first column tile writes the bias gradient'),
        _case('wgrad_rowsum_cols', 64, 100, 33, why='bias gradient with in_f > 32 and two row tiles of out_f'),
    ]
    # ---- K edges, placed on the K axis of each entry point: in_f (forward), out_f (data gradient), rows (weight gradient)
    for k in K_EDGES:
        cases.append(_case('kfwd_%d' % k, 33, k, 65, why='K edge of the forward'))
        cases.append(_case('kdat_%d' % k, 33, 65, k, why='K edge of the data gradient'))
        cases.append(_case('kwgt_%d' % k, k, 33, 65, why='K edge of the weight gradient'))
    # ---- operand alignment: x, w, gy one or two floats into a larger buffer.  in_f = out_f = 68 (multiple of 4: the widest
    # loader the address allows is the one taken), 66 (multiple of 2 only) and 67 (odd: dword loads whatever the address)
    for ox in (0, 2, 1):
        for ow in (0, 2, 1):
            cases.append(_case('align_x%d_w%d' % (ox, ow), 35, 68, 68, offs=(ox, ow, (ox + ow) % 3),
                               why='forward (AV, BV) pair / tiled vec off because of a pointer'))
    cases += [
        _case('align_g2_k66', 35, 66, 66, offs=(2, 0, 2), why='K % 2 == 0: 8-byte loaders at best'),
        _case('align_k66', 35, 66, 66, why='aligned pointers, K % 4 != 0: (2, 2) and the scalar tiled loaders'),
        _case('align_k67', 35, 67, 67, why='odd K: (1, 1)'),
        _case('align_x3_k68', 35, 68, 68, offs=(3, 0, 3), why='three floats in: 4-byte aligned'),
    ]
    # ---- epilogue: all five activation codes on a full and on a ragged tile, without bias, without bias gradient
    for act in ACTS:
        cases.append(_case('act%d_full' % act, 64, 48, 128, act=act, why='activation on full tiles (64x64, 32x32)'))
        cases.append(_case('act%d_ragged' % act, 33, 20, 70, act=act, slope=0.01, why='activation on ragged tiles'))
    cases += [
        _case('act3_full_m32', 32, 48, 128, act=ACT_TANH, why='tanh on a full 32x128 tile'),
        _case('nobias_full', 64, 32, 64, bias=False, gb=False, why='bias == NULL, gb == NULL, full tiles'),
        _case('nobias_ragged_relu', 40, 68, 50, bias=False, gb=False, act=ACT_RELU, why='bias == NULL on ragged tiles'),
        _case('nogb_wide', 24, 100, 70, gb=False, why='gb == NULL with in_f > 32'),
    ]
    names = [c['name'] for c in cases]
    assert len(set(names)) == len(names)
    return cases


DENSE_CASES = _build_dense_cases()
DENSE_BY_NAME = dict((c['name'], c) for c in DENSE_CASES)


def dense_inputs(case):
    """x [rows, in_f], w [out_f, in_f], b [out_f], gy [rows, out_f] (fp32)"""
    rng = rng_of('dense_' + case['name'])
    rows, in_f, out_f = case['rows'], case['in_f'], case['out_f']
    return (f32(rng, (rows, in_f)), f32(rng, (out_f, in_f), 0.5), f32(rng, (out_f,), 0.5), f32(rng, (rows, out_f)))


def act_ref(v, act, slope):
    v = np.asarray(v, dtype=np.float64)
    if act == ACT_RELU:
        return np.where(v > 0, v, 0.0)
    if act == ACT_LEAKY:
        return np.where(v > 0, v, v * np.float64(np.float32(slope)))
    if act == ACT_TANH:
        return np.tanh(v)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    return v


def dense_ref(case, x, w, b, gy):
    """float64 results and rounding bounds of the three entry points.  Every kernel is an fp32 fma chain over K plus at most
    three further adds (the four k-partials of the skinny kernel, the bias): |got - ref| <= gamma(K + 3) (sum_k |a||b| + |bias|)."""
    x64, w64, g64 = x.astype(np.float64), w.astype(np.float64), gy.astype(np.float64)
    b64 = b.astype(np.float64) if case['bias'] else np.zeros(case['out_f'])
    rows, in_f, out_f = case['rows'], case['in_f'], case['out_f']
    pre = x64 @ w64.T + b64
    pre_bound = gamma(in_f + 3) * (np.abs(x64) @ np.abs(w64).T + np.abs(b64))
    y = act_ref(pre, case['act'], case['slope'])
    y_bound = ACT_LIPSCHITZ[case['act']] * pre_bound
    if case['act'] in (ACT_TANH, ACT_SIGMOID):
        y_bound = y_bound + 1e-6 * np.maximum(1.0, np.abs(y))
    return dict(pre=pre, y=y, y_bound=y_bound,
                gx=g64 @ w64, gx_bound=gamma(out_f + 3) * (np.abs(g64) @ np.abs(w64)),
                gw=g64.T @ x64, gw_bound=gamma(rows + 3) * (np.abs(g64).T @ np.abs(x64)),
                gb=g64.sum(0), gb_bound=gamma(rows) * np.abs(g64).sum(0))


def onehot_case(entry, k, other=33, bias=True):
    """the exact probe: the K-contracted operand is the identity, so every k position is read exactly once and the result is
    the other operand (plus the bias), bit for bit.  -> (rows, in_f, out_f)"""
    if entry == LINEAR_FWD:              # x = I [k, k]: y = w^T + b, w [other, k]
        return k, k, other
    if entry == LINEAR_BWD_DATA:         # gy = I [k, k]: gx = w, w [k, other]
        return k, other, k
    return k, other, k                   # gy = I [k, k] (rows = out_f = k): gw = x, x [k, other]


# =============================================================================================
# linear plane operators as tap lists: y[o] += wgt * x[i].  The forward reference gathers, the adjoint scatters.
# =============================================================================================
class Taps(object):
    def __init__(self, n_in, n_out, o, i, w=None):
        self.n_in, self.n_out = int(n_in), int(n_out)
        self.o, self.i = np.asarray(o, dtype=np.int64).reshape(-1), np.asarray(i, dtype=np.int64).reshape(-1)
        self.w = np.ones(len(self.o)) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)

    def fwd(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.n_in)
        y = np.zeros((x.shape[0], self.n_out))
        np.add.at(y, (slice(None), self.o), x[:, self.i] * self.w)
        return y

    def adj(self, g):
        g = np.asarray(g, dtype=np.float64).reshape(-1, self.n_out)
        gx = np.zeros((g.shape[0], self.n_in))
        np.add.at(gx, (slice(None), self.i), g[:, self.o] * self.w)
        return gx

    def abs_(self):
        return Taps(self.n_in, self.n_out, self.o, self.i, np.abs(self.w))

    def terms_out(self):
        return np.bincount(self.o, minlength=self.n_out)

    def terms_in(self):
        return np.bincount(self.i, minlength=self.n_in)


def taps_avgpool3s2(H, W):
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    o, i, w = [], [], []
    for oh in range(OH):
        for ow in range(OW):
            hs = [h for h in (2 * oh - 1, 2 * oh, 2 * oh + 1) if 0 <= h < H]
            ws = [x for x in (2 * ow - 1, 2 * ow, 2 * ow + 1) if 0 <= x < W]
            for h in hs:
                for x in ws:
                    o.append(oh * OW + ow)
                    i.append(h * W + x)
                    w.append(1.0 / (len(hs) * len(ws)))
    return Taps(H * W, OH * OW, o, i, w)


def taps_avgpool(H, W, k):
    OH, OW = H // k, W // k
    o, i = [], []
    for oh in range(OH):
        for ow in range(OW):
            for a in range(k):
                for b in range(k):
                    o.append(oh * OW + ow)
                    i.append((oh * k + a) * W + ow * k + b)
    return Taps(H * W, OH * OW, o, i, np.full(len(o), 1.0 / (k * k)))


def taps_gap(HW):
    return Taps(HW, 1, np.zeros(HW), np.arange(HW), np.full(HW, 1.0 / HW))


def taps_upsample2(H, W):
    oh, ow = np.meshgrid(np.arange(2 * H), np.arange(2 * W), indexing='ij')
    return Taps(H * W, 4 * H * W, oh * 2 * W + ow, (oh // 2) * W + ow // 2)


def _reflect(j, L):
    return -j if j < 0 else (2 * L - 2 - j if j >= L else j)


def _clamp(j, L):
    return min(max(j, 0), L - 1)


def _taps_pad(H, W, pad, fold):
    PH, PW = H + 2 * pad, W + 2 * pad
    o, i = [], []
    for ph in range(PH):
        for pw in range(PW):
            o.append(ph * PW + pw)
            i.append(fold(ph - pad, H) * W + fold(pw - pad, W))
    return Taps(H * W, PH * PW, o, i)


def taps_reflect_pad(H, W, pad):
    assert pad < H and pad < W
    return _taps_pad(H, W, pad, _reflect)


def taps_replicate_pad(H, W, pad):
    return _taps_pad(H, W, pad, _clamp)


def taps_pad_upsample(H, W, pad, ups):
    """reflect_pad(pad) o nearest_upsample(ups) on an H x W plane; its adjoint is sg_pad_upsample_bwd"""
    LH, LW = H * ups, W * ups
    assert pad < LH and pad < LW
    PH, PW = LH + 2 * pad, LW + 2 * pad
    o, i = [], []
    for ph in range(PH):
        for pw in range(PW):
            o.append(ph * PW + pw)
            i.append((_reflect(ph - pad, LH) // ups) * W + _reflect(pw - pad, LW) // ups)
    return Taps(H * W, PH * PW, o, i)


def taps_window(OH, OW, H, W, KS, stride, pad):
    """sg_cond_conv_bias_act's sum: out[oh, ow] += P[kh * KS + kw] for the taps that land inside the H x W plane"""
    o, i = [], []
    for oh in range(OH):
        for ow in range(OW):
            for kh in range(KS):
                for kw in range(KS):
                    if 0 <= oh * stride - pad + kh < H and 0 <= ow * stride - pad + kw < W:
                        o.append(oh * OW + ow)
                        i.append(kh * KS + kw)
    return Taps(KS * KS, OH * OW, o, i)


_FOLD_R = {0: (2,), 1: (1, 2), 2: (0, 1), 3: (0,)}      # include/sg2im_hip.h: R(kh)


def taps_upconv3_fold(Cout, Cin):
    """w [Cout][Cin][3][3] -> wt [Cin][Cout][4][4]"""
    o, i = [], []
    for ci in range(Cin):
        for co in range(Cout):
            for kh in range(4):
                for kw in range(4):
                    for a in _FOLD_R[kh]:
                        for b in _FOLD_R[kw]:
                            o.append(((ci * Cout + co) * 4 + kh) * 4 + kw)
                            i.append(((co * Cin + ci) * 3 + a) * 3 + b)
    return Taps(Cout * Cin * 9, Cin * Cout * 16, o, i)


def taps_cond_split(M, C1, C2, R):
    """W [M][C1 + C2][R] -> [W1 [M][C1][R] | W2r [M * R][C2]] (one output vector, W1 first)"""
    o, i = [], []
    n1 = M * C1 * R
    for m in range(M):
        for c in range(C1 + C2):
            for t in range(R):
                i.append((m * (C1 + C2) + c) * R + t)
                o.append((m * C1 + c) * R + t if c < C1 else n1 + (m * R + t) * C2 + (c - C1))
    return Taps(M * (C1 + C2) * R, n1 + M * R * C2, o, i)


# ---- the case lists ------------------------------------------------------------------------------------------------
AVGPOOL3S2_SHAPES = ((1, 1), (1, 2), (2, 2), (3, 3), (2, 5), (8, 8), (9, 12), (7, 64))
POOL_NC = 3
# (H, W, k): odd and even sizes, uncovered tails, k = 1, k = H
POOL2D_CASES = ((4, 4, 1), (4, 4, 2), (5, 7, 2), (6, 6, 3), (7, 8, 3), (5, 5, 5), (11, 13, 5), (4, 4, 4), (9, 12, 2), (3, 9, 3))
MAXPOOL2_SHAPES = ((2, 2), (2, 3), (3, 2), (4, 4), (5, 7), (9, 12), (6, 64))
GAP_CASES = tuple((nc, hw) for nc in (1, 4, 5) for hw in (1, 63, 64, 65, 1000))
UPSAMPLE2_SHAPES = ((1, 1), (2, 3), (9, 12))
REFLECT_PAD_CASES = ((4, 5, 1), (4, 5, 3), (9, 12, 1), (9, 12, 3), (4, 6, 3), (2, 2, 1), (5, 5, 4))      # (H, W, pad); pad up to H - 1
REPLICATE_PAD_CASES = ((4, 5, 0), (4, 5, 1), (4, 5, 3), (1, 1, 1), (1, 6, 3), (6, 1, 1), (9, 12, 3), (2, 2, 1))
# (NC, H, W, pad, upsample): pad {0, 1, 3} x upsample {1, 2}, L = 2 with pad 1, the grid.y loop at 1 x 2 planes
PAD_UPSAMPLE_CASES = tuple((3, 5, 6, pad, ups) for pad in (0, 1, 3) for ups in (1, 2)) + (
    (3, 2, 2, 1, 1), (3, 1, 2, 1, 2), (2, 4, 4, 3, 1), (1, 17, 19, 3, 2),
    (GRID_Y_MAX, 1, 2, 0, 1), (GRID_Y_MAX + 1, 1, 2, 0, 2), (GRID_Y_MAX + 2, 1, 2, 1, 2))
CONCAT_CASES = ((2, 3, 5, 7), (1, 1, 1, 1), (3, 4, 1, 64), (2, 1, 6, 100))              # (N, Ca, Cb, HW)
COND_SPLIT_CASES = ((1, 1, 1, 1), (3, 2, 5, 9), (4, 7, 3, 16), (2, 5, 4, 1))            # (M, C1, C2, R)
COND_WINDOW_CASES = tuple((KS, stride, pad, NM, ohw)
                          for KS in (1, 3, 4) for stride in (1, 2) for pad in (0, 1, 2)
                          for NM in (1, 5, 8) for ohw in (1, 3, 8, 10))                 # OH = OW = ohw: OH * OW in {1, 9, 64, 100}
ACT_NS = (0, 1, 255, 256, 257)
ACT_SLOPES = (0.2, 0.01)
ACT_SPECIALS = (0.0, -0.0, 90.0, -90.0, 1e-3, -1e-3, 1.0, -1.0, 20.0, -20.0)
FOLD_CASES = ((1, 1), (3, 5), (24, 24))                                                 # (Cout, Cin)
EWISE_NS = (0, 1, 255, 257)
# (n, float offset of y, float offset of x): vector kernel, scalar kernels behind n % 4 != 0, a misaligned pointer with n % 4 == 0
AXPY_CASES = ((0, 0, 0), (4, 0, 0), (1024, 0, 0), (1028, 0, 0), (1, 0, 0), (255, 0, 0), (1027, 0, 0), (1024, 1, 0), (1024, 0, 2),
              (260, 1, 1))


def cond_window_geometry(KS, stride, pad, ohw):
    """(OH, OW, H, W) of a window case: the conv geometry where it exists, else a one-pixel plane (the kernels take all four)"""
    H = max(1, (ohw - 1) * stride + KS - 2 * pad)
    return ohw, ohw, H, H


def cond_window_consistent(KS, stride, pad, ohw):
    OH, OW, H, W = cond_window_geometry(KS, stride, pad, ohw)
    return H + 2 * pad >= KS and (H + 2 * pad - KS) // stride + 1 == OH


def tie_values(rng, shape):
    """inputs drawn from three values, so that the windows of a max pool hold ties"""
    return rng.choice(np.array([-1.0, 0.5, 2.0], dtype=np.float32), size=shape)


def maxpool_ref(x, k):
    """x [NC, H, W] -> (y [NC, OH, OW], arg [NC, OH, OW]: flat index into the plane of the FIRST maximum in row-major order)"""
    NC, H, W = x.shape
    OH, OW = H // k, W // k
    y = np.zeros((NC, OH, OW), dtype=x.dtype)
    arg = np.zeros((NC, OH, OW), dtype=np.int64)
    for oh in range(OH):
        for ow in range(OW):
            win = x[:, oh * k:(oh + 1) * k, ow * k:(ow + 1) * k].reshape(NC, k * k)
            a = win.argmax(1)                                   # numpy: the first occurrence
            y[:, oh, ow] = win[np.arange(NC), a]
            arg[:, oh, ow] = (oh * k + a // k) * W + ow * k + a % k
    return y, arg


def maxpool_bwd_ref(arg, gy, H, W):
    """gy routed to the first maximum; everything else, the uncovered tail included, zero"""
    NC = gy.shape[0]
    gx = np.zeros((NC, H * W), dtype=gy.dtype)
    flat = arg.reshape(NC, -1)
    gx[np.arange(NC)[:, None], flat] = gy.reshape(NC, -1)       # windows are disjoint: plain assignment
    return gx.reshape(NC, H, W)


def act_inputs(n, salt):
    rng = rng_of('act_%d_%s' % (n, salt))
    x = f32(rng, (n,), 2.0)
    m = min(n, len(ACT_SPECIALS))
    x[:m] = np.array(ACT_SPECIALS[:m], dtype=np.float32)
    return x


def act_bwd_ref(y, gy, act, slope):
    """float64 gradient from the activation OUTPUT (include/sg2im_hip.h: sg_act_bwd)"""
    y, gy = y.astype(np.float64), gy.astype(np.float64)
    if act == ACT_RELU:
        d = np.where(y > 0, 1.0, 0.0)
    elif act == ACT_LEAKY:
        d = np.where(y > 0, 1.0, np.float64(np.float32(slope)))
    elif act == ACT_TANH:
        d = 1.0 - y * y
    elif act == ACT_SIGMOID:
        d = y * (1.0 - y)
    else:
        d = np.ones_like(y)
    return gy * d


def unfold_fp32(gwt, Cout, Cin):
    """sg_upconv3_unfold_wgrad in fp32 in its documented order (a + b) + (c + d): gwt [Cin][Cout][4][4] -> gw [Cout][Cin][3][3]"""
    g = gwt.astype(np.float32).reshape(Cin, Cout, 4, 4).transpose(1, 0, 2, 3)
    gw = np.zeros((Cout, Cin, 3, 3), dtype=np.float32)
    for i in range(3):
        for j in range(3):
            a, b = 2 - i, 2 - j
            gw[:, :, i, j] = (g[:, :, a, b] + g[:, :, a, b + 1]) + (g[:, :, a + 1, b] + g[:, :, a + 1, b + 1])
    return gw
