"""The case tables of tests/dense_pointwise_cases.py, checked without a GPU: the dense table reaches every launch plan
sg_linear_plan can report (and every kernel those plans name exists in the built code object), the restated kernel constants are
the ones in the .hip sources, every float64 reference agrees with an independent formulation (torch double, autograd for the
gradients), and every forward / adjoint pair satisfies <A x, g> == <x, A^T g>."""
import functools
import os
import re
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_pointwise_cases as DP
from scene_generation_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'scene_generation_amd', 'csrc')
ENTRIES = (DP.LINEAR_FWD, DP.LINEAR_BWD_DATA, DP.LINEAR_BWD_WEIGHT)
GRID = (1, 4, 31, 32, 33, 63, 64, 66, 68, 129, 257, 3000)


def _default(name):
    return _hip.options()[name][1]


@functools.lru_cache(maxsize=None)
def _reachable():
    lib = _hip.lib()
    plans = set()
    for skinny in (0, _default('linear_skinny'), 1 << 30):
        with DP.option('linear_skinny', skinny):
            for nsub in (1, 2):
                with DP.option('linear_nsub', nsub):
                    for e in ENTRIES:
                        for rows in GRID:
                            for in_f in GRID:
                                for out_f in GRID:
                                    for aa in (16, 8, 4):
                                        for ba in (16, 8, 4):
                                            plans.add(DP.plan_class(e, DP.linear_plan(lib, e, rows, in_f, out_f, aa, ba)))
    return plans


@functools.lru_cache(maxsize=None)
def _covered():
    """{plan class: a case that reaches it} over the table as tests/test_gpu_dense_pointwise.py runs it"""
    lib = _hip.lib()
    plans = {}
    for _, skinny in DP.KERNELS:
        with DP.option('linear_skinny', skinny):
            for nsub in DP.NSUB_VALUES:
                with DP.option('linear_nsub', nsub):
                    for c in DP.DENSE_CASES:
                        for e in ENTRIES:
                            aa, ba = DP.operand_aligns(e, c)
                            p = DP.linear_plan(lib, e, c['rows'], c['in_f'], c['out_f'], aa, ba)
                            plans.setdefault(DP.plan_class(e, p), c['name'])
    return plans


def _rule(entry, rows, in_f, out_f, aa, ba, skinny_opt, nsub_opt):
    """the dispatch rule as the three entry points documented it before they shared a plan function, restated on its own"""
    M, N, K = DP.gemm_dims(entry, rows, in_f, out_f)

    def vec_of(align, ld):
        if align == 16 and ld % 4 == 0 and K % 4 == 0:
            return 4
        return 2 if align >= 8 and ld % 2 == 0 and K % 2 == 0 else 1
    if -(-M // DP.SK_TILE) * -(-N // DP.SK_TILE) <= skinny_opt:
        if entry == DP.LINEAR_FWD:
            return (DP.LIN_SKINNY, vec_of(aa, in_f), vec_of(ba, in_f), 32, 32, 1)
        if entry == DP.LINEAR_BWD_DATA:
            return (DP.LIN_SKINNY, vec_of(aa, out_f), 0, 32, 32, 1)
        return (DP.LIN_SKINNY, 0, 0, 32, 32, 1)
    nsub = 2 if nsub_opt == 2 and K >= 64 else 1
    bm, bn = (32, 128) if M <= 32 else (64, 64)
    if entry == DP.LINEAR_FWD:
        f = DP.LIN_KVEC if in_f % 4 == 0 and aa == 16 and ba == 16 else DP.LIN_KSCALAR
        return (DP.LIN_TILED, f, f, bm, bn, nsub)
    if entry == DP.LINEAR_BWD_DATA:
        return (DP.LIN_TILED, DP.LIN_KVEC if out_f % 4 == 0 and aa == 16 else DP.LIN_KSCALAR, 0, bm, bn, nsub)
    return (DP.LIN_TILED, 0, 0, bm, bn, nsub)


def test_plan_follows_the_documented_rule():
    lib = _hip.lib()
    grid = (1, 2, 4, 31, 32, 33, 62, 64, 66, 68, 129, 1100)
    n = 0
    for skinny in (0, 3, _default('linear_skinny'), 1 << 30):
        with DP.option('linear_skinny', skinny):
            for nsub in (1, 2):
                with DP.option('linear_nsub', nsub):
                    for e in ENTRIES:
                        for rows in grid:
                            for in_f in grid:
                                for out_f in grid:
                                    for aa, ba in ((16, 16), (16, 8), (8, 16), (4, 16), (16, 4), (8, 8), (4, 4), (8, 4), (4, 8)):
                                        got = DP.linear_plan(lib, e, rows, in_f, out_f, aa, ba)
                                        assert got == _rule(e, rows, in_f, out_f, aa, ba, skinny, nsub), (
                                            DP.ENTRY_NAMES[e], rows, in_f, out_f, aa, ba, skinny, nsub, got)
                                        n += 1
    assert n > 100000


def test_header_values_match():
    text = open(os.path.join(ROOT, 'include', 'sg2im_hip.h')).read()
    vals = dict((k, int(v)) for k, v in re.findall(r'(SG_LIN(?:EAR)?_\w+|SG_ACT_\w+)\s*=\s*(\d+)', text))
    assert vals['SG_LINEAR_FWD'] == DP.LINEAR_FWD and vals['SG_LINEAR_BWD_DATA'] == DP.LINEAR_BWD_DATA
    assert vals['SG_LINEAR_BWD_WEIGHT'] == DP.LINEAR_BWD_WEIGHT
    assert (vals['SG_LIN_SKINNY'], vals['SG_LIN_TILED']) == (DP.LIN_SKINNY, DP.LIN_TILED)
    assert (vals['SG_LIN_ROWMAJOR'], vals['SG_LIN_KSCALAR'], vals['SG_LIN_KVEC']) == (DP.LIN_ROWMAJOR, DP.LIN_KSCALAR, DP.LIN_KVEC)
    assert [vals['SG_ACT_' + n] for n in ('NONE', 'RELU', 'LEAKY', 'TANH', 'SIGMOID')] == list(DP.ACTS)
    assert 'sg_linear_plan' in _hip.PROTOS


def test_constants_match_the_sources():
    sk = open(os.path.join(CSRC, 'skinny.hip')).read()
    core = open(os.path.join(CSRC, 'igemm_core.h')).read()
    norm = open(os.path.join(CSRC, 'norm.hip')).read()
    assert re.search(r'constexpr int SK_ROUND = (\d+);', sk).group(1) == str(DP.SK_ROUND)
    assert 'n0 = blockIdx.x * %d, m0 = blockIdx.y * %d;' % (DP.SK_TILE, DP.SK_TILE) in sk
    assert 'grid(sg_cdiv(N, %d), sg_cdiv(M, %d))' % (DP.SK_TILE, DP.SK_TILE) in sk
    assert 'const int chunks = (K + %d) >> 4;' % (DP.SK_CHUNK - 1) in sk and DP.SK_CHUNK == 1 << 4
    assert 'const int per = chunks >> 2, extra = chunks & 3;' in sk and DP.SK_WAVES == 1 << 2
    assert re.search(r'constexpr int BK = (\d+);', core).group(1) == str(DP.BK)
    assert norm.count('n0 += %d' % DP.GRID_Y_MAX) == 1 and 'NC - n0 : %d' % DP.GRID_Y_MAX in norm
    for kernel, launch in (('gap_fwd_kernel', r'gap_fwd_kernel, dim3\(sg_cdiv\(NC, (\d+)\)\)'),
                           ('cond_window_sums_kernel', r'grid\(\(unsigned\)sg_cdiv\(NM, (\d+)\)\)')):
        assert re.search(launch, norm).group(1) == str(DP.PLANES_PER_BLOCK), kernel
    assert 'blockIdx.x * %d + (threadIdx.x >> 6)' % DP.PLANES_PER_BLOCK in norm


def test_python_view_of_the_split_matches_the_edges():
    per_wave = set()
    for k in DP.SKINNY_K_EDGES:
        per_wave |= set(DP.skinny_wave_chunks(k))
    assert {0, 1, 4, 5, 8, 9, 13} <= per_wave, sorted(per_wave)
    assert DP.skinny_wave_chunks(48) == [1, 1, 1, 0]                            # three chunks: wave 3 idle
    assert set(-(-k // DP.SK_CHUNK) % 4 for k in DP.SKINNY_K_EDGES) == {0, 1, 2, 3}
    for want in (4, 5, 8, 9, 13):
        assert any(max(DP.skinny_wave_chunks(k)) == want for k in DP.SKINNY_K_EDGES), want
    assert any(k % 4 == 0 for k in DP.SKINNY_K_EDGES) and any(k % 4 == 2 for k in DP.SKINNY_K_EDGES)
    assert any(k % 2 == 1 for k in DP.SKINNY_K_EDGES)
    # tiled: a vector tail in the first and in the second sub-tile of a 32-deep k-tile, and vector K below 64
    assert any(k % 4 == 0 and k >= 64 and 0 < k % 32 < 16 for k in DP.TILED_K_EDGES)
    assert any(k % 4 == 0 and k >= 64 and 16 < k % 32 for k in DP.TILED_K_EDGES)
    assert any(k % 4 == 0 and k % 16 != 0 and k < 64 for k in DP.TILED_K_EDGES)


def test_dense_cases_cover_every_reachable_plan(capsys):
    reachable, covered = _reachable(), _covered()
    assert set(covered) <= reachable
    missing = sorted(reachable - set(covered))
    assert not missing, 'dense plans no dense_pointwise_cases entry reaches: %s' % missing
    skinny = set(p[2:4] for p in reachable if p[1] == DP.LIN_SKINNY)
    tiled = set(p for p in reachable if p[1] == DP.LIN_TILED)
    assert len(skinny) == 13, sorted(skinny)
    assert set(p[2:4] for p in reachable if p[1] == DP.LIN_SKINNY and p[0] == DP.LINEAR_FWD) == set(
        (a, b) for a in (4, 2, 1) for b in (4, 2, 1))
    assert set(p[2:4] for p in reachable if p[1] == DP.LIN_SKINNY and p[0] == DP.LINEAR_BWD_DATA) == {(4, 0), (2, 0), (1, 0)}
    assert set(p[2:4] for p in reachable if p[1] == DP.LIN_SKINNY and p[0] == DP.LINEAR_BWD_WEIGHT) == {(0, 0)}
    # tiled: {vector, scalar} (or row-index-major only) x {64x64, 32x128} x NSUB {1, 2} per entry point
    assert len(tiled) == 8 + 8 + 4, sorted(tiled)
    with capsys.disabled():
        print('\ndense_pointwise_cases covers all %d reachable dense plans: %d skinny_gemm_kernel instantiations, %d tiled '
              'configurations, none missing' % (len(reachable), len(skinny), len(tiled)))


def test_table_rows_are_there_for_what_they_say():
    lib = _hip.lib()

    def plan(name, entry, skinny, nsub=2):
        c = DP.DENSE_BY_NAME[name]
        aa, ba = DP.operand_aligns(entry, c)
        with DP.option('linear_skinny', skinny), DP.option('linear_nsub', nsub):
            return DP.linear_plan(lib, entry, c['rows'], c['in_f'], c['out_f'], aa, ba)
    S, T = DP.SKINNY_ALWAYS, DP.SKINNY_NEVER
    # the nine forward pairs and the three data-gradient forms
    want = {0: 4, 2: 2, 1: 1}
    for ox in (0, 2, 1):
        for ow in (0, 2, 1):
            assert plan('align_x%d_w%d' % (ox, ow), DP.LINEAR_FWD, S)[1:3] == (want[ox], want[ow])
            vec = DP.LIN_KVEC if ox == 0 and ow == 0 else DP.LIN_KSCALAR            # vec false because of a pointer
            assert plan('align_x%d_w%d' % (ox, ow), DP.LINEAR_FWD, T)[1:3] == (vec, vec)
    assert plan('align_x0_w0', DP.LINEAR_BWD_DATA, S)[1:3] == (4, 0)
    assert plan('align_g2_k66', DP.LINEAR_BWD_DATA, S)[1:3] == (2, 0)
    assert plan('align_x3_k68', DP.LINEAR_BWD_DATA, S)[1:3] == (1, 0)
    assert plan('align_k66', DP.LINEAR_FWD, T)[1:3] == (DP.LIN_KSCALAR, DP.LIN_KSCALAR)   # vec false because of K
    assert plan('align_k66', DP.LINEAR_FWD, S)[1:3] == (2, 2) and plan('align_k67', DP.LINEAR_FWD, S)[1:3] == (1, 1)
    # depth: 60 stays 16 deep at nsub = 2; 64 and up are 32 deep; nsub = 1 restores 16
    assert plan('kfwd_60', DP.LINEAR_FWD, T) == (DP.LIN_TILED, DP.LIN_KVEC, DP.LIN_KVEC, 64, 64, 1)
    assert plan('kfwd_68', DP.LINEAR_FWD, T) == (DP.LIN_TILED, DP.LIN_KVEC, DP.LIN_KVEC, 64, 64, 2)
    assert plan('kfwd_68', DP.LINEAR_FWD, T, 1) == (DP.LIN_TILED, DP.LIN_KVEC, DP.LIN_KVEC, 64, 64, 1)
    assert plan('m32_n257', DP.LINEAR_FWD, T) == (DP.LIN_TILED, DP.LIN_KVEC, DP.LIN_KVEC, 32, 128, 2)
    assert plan('m1_n130_k68', DP.LINEAR_FWD, T) == (DP.LIN_TILED, DP.LIN_KVEC, DP.LIN_KVEC, 32, 128, 2)   # <128, true> tail
    assert plan('wgrad_32x128_two_xcontig', DP.LINEAR_BWD_WEIGHT, T) == (DP.LIN_TILED, 0, 0, 32, 128, 2)
    assert plan('wgrad_32x128_two_xcontig', DP.LINEAR_BWD_WEIGHT, S) == (DP.LIN_SKINNY, 0, 0, 32, 32, 1)
    # the default threshold routes by the number of 32 x 32 tiles
    d = _default('linear_skinny')
    with DP.option('linear_skinny', d):
        assert DP.linear_plan(lib, DP.LINEAR_FWD, 32, 64, 32 * d, 16, 16)[0] == DP.LIN_SKINNY
        assert DP.linear_plan(lib, DP.LINEAR_FWD, 33, 64, 32 * d, 16, 16)[0] == DP.LIN_TILED
    for bad in ((3, 1, 1, 1, 16, 16), (0, 0, 1, 1, 16, 16), (0, 1, 1, 1, 12, 16), (0, 1, 1, 1, 16, 2)):
        v = DP.ctypes.c_int(0)
        assert lib.sg_linear_plan(*bad, *[DP._ptr(v)] * 6) < 0


def test_every_epilogue_and_null_operand_is_in_the_table():
    acts_full = set(c['act'] for c in DP.DENSE_CASES if c['rows'] % 64 == 0 and c['out_f'] % 64 == 0)
    acts_ragged = set(c['act'] for c in DP.DENSE_CASES if c['rows'] % 32 and c['out_f'] % 32)
    assert acts_full == set(DP.ACTS) and acts_ragged == set(DP.ACTS)
    assert any(not c['bias'] for c in DP.DENSE_CASES) and any(not c['gb'] for c in DP.DENSE_CASES)
    assert any(c['gb'] and c['in_f'] > DP.SK_TILE and c['out_f'] > DP.SK_TILE for c in DP.DENSE_CASES)
    for e in ENTRIES:
        ms = set(DP.gemm_dims(e, c['rows'], c['in_f'], c['out_f'])[0] for c in DP.DENSE_CASES)
        ns = set(DP.gemm_dims(e, c['rows'], c['in_f'], c['out_f'])[1] for c in DP.DENSE_CASES)
        ks = set(DP.gemm_dims(e, c['rows'], c['in_f'], c['out_f'])[2] for c in DP.DENSE_CASES)
        assert set(DP.MN_EDGES) <= ms and set(DP.MN_EDGES) <= ns, DP.ENTRY_NAMES[e]
        assert set(DP.K_EDGES) <= ks, DP.ENTRY_NAMES[e]
    assert any(c['rows'] <= 32 and c['out_f'] > 128 for c in DP.DENSE_CASES)
    assert max(c['rows'] * c['in_f'] * c['out_f'] for c in DP.DENSE_CASES) <= 256 * 1152 * 900


def test_reachable_kernels_exist_in_the_code_object():
    from tools import isa_report
    if not (os.path.isfile(isa_report.DEFAULT_LIB) and shutil.which('objcopy')
            and os.path.isfile(os.path.join(isa_report.LLVM, 'clang-offload-bundler'))):
        pytest.skip('needs the built library and the ROCm LLVM tools')
    import tempfile
    with tempfile.TemporaryDirectory() as wd:
        ks = []
        for elf in isa_report.code_objects(isa_report.DEFAULT_LIB, wd):
            ks.extend(isa_report.kernels_of(elf))
    names = isa_report.demangle([k['mangled'] for k in ks])         # full names: the report's short form drops NSUB
    missing = []
    for p in sorted(_reachable()):
        pat = re.compile(DP.plan_kernel_pattern(p[0], p[1:]) + r'\(')
        if not any(pat.match(n) for n in names):
            missing.append((p, pat.pattern))
    assert not missing, missing


# =============================================================================================
# references against an independent formulation
# =============================================================================================
def t64(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).double()
    return t.requires_grad_() if grad else t


def agree(a, b, name, tol=1e-12):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    if a.size:
        assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), (name, np.abs(a - b).max())


def adjoint_identity(taps, name, nc=2):
    rng = DP.rng_of('adj_' + name)
    x, g = rng.standard_normal((nc, taps.n_in)), rng.standard_normal((nc, taps.n_out))
    lhs, rhs = (taps.fwd(x) * g).sum(), (x * taps.adj(g)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (name, lhs, rhs)


def autograd_check(taps, fn, in_shape, name, nc=2):
    """taps.fwd == fn and taps.adj == fn's autograd gradient, in float64.  fn: [nc, *in_shape] -> anything with nc rows"""
    rng = DP.rng_of('ag_' + name)
    x = t64(rng.standard_normal((nc,) + tuple(in_shape)), grad=True)
    y = fn(x)
    agree(taps.fwd(x.detach().numpy()), y.reshape(nc, -1), name + ' forward')
    g = rng.standard_normal(tuple(y.shape))
    y.backward(t64(g))
    agree(taps.adj(g), x.grad.reshape(nc, -1), name + ' adjoint')
    adjoint_identity(taps, name)


@pytest.mark.parametrize('case', DP.DENSE_CASES[::3] + [DP.DENSE_BY_NAME['nobias_ragged_relu']], ids=lambda c: c['name'])
def test_dense_reference_against_autograd(case):
    x, w, b, gy = DP.dense_inputs(case)
    ref = DP.dense_ref(case, x, w, b, gy)
    xt, wt, bt = t64(x, True), t64(w, True), t64(b, True)
    pre = F.linear(xt, wt, bt if case['bias'] else None)
    agree(ref['pre'], pre, 'pre')
    act = case['act']
    y = (F.relu(pre) if act == DP.ACT_RELU else F.leaky_relu(pre, float(np.float32(case['slope']))) if act == DP.ACT_LEAKY
         else torch.tanh(pre) if act == DP.ACT_TANH else torch.sigmoid(pre) if act == DP.ACT_SIGMOID else pre)
    agree(ref['y'], y, 'y')
    pre.backward(t64(gy))                     # the three GEMMs take gy directly: the gradient of the pre-activation
    agree(ref['gx'], xt.grad, 'gx')
    agree(ref['gw'], wt.grad, 'gw')
    if case['bias']:
        agree(ref['gb'], bt.grad, 'gb')
    assert (ref['y_bound'] >= 0).all() and (ref['gx_bound'] > 0).all() and (ref['gw_bound'] > 0).all()


def test_onehot_probe_shapes():
    for e in ENTRIES:
        for k in DP.K_EDGES:
            rows, in_f, out_f = DP.onehot_case(e, k)
            assert DP.gemm_dims(e, rows, in_f, out_f)[2] == k


@pytest.mark.parametrize('H,W', DP.AVGPOOL3S2_SHAPES)
def test_avgpool3s2_reference(H, W):
    t = DP.taps_avgpool3s2(H, W)
    autograd_check(t, lambda x: F.avg_pool2d(x[:, None], 3, 2, 1, count_include_pad=False), (H, W), 'avgpool3s2 %dx%d' % (H, W))
    assert t.terms_out().max() <= 9 and t.terms_in().max() <= 4
    assert t.n_out == ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)


@pytest.mark.parametrize('H,W,k', DP.POOL2D_CASES)
def test_avgpool_k_reference(H, W, k):
    autograd_check(DP.taps_avgpool(H, W, k), lambda x: F.avg_pool2d(x[:, None], k, k), (H, W), 'avgpool%d %dx%d' % (k, H, W))


@pytest.mark.parametrize('H,W,k', DP.POOL2D_CASES + tuple((h, w, 2) for h, w in DP.MAXPOOL2_SHAPES))
def test_maxpool_reference_routes_to_the_first_maximum(H, W, k):
    rng = DP.rng_of('maxpool_%d_%d_%d' % (H, W, k))
    x = DP.tie_values(rng, (DP.POOL_NC, H, W))
    y, arg = DP.maxpool_ref(x, k)
    if k > 1:
        assert any(np.sum(x[n, oh * k:(oh + 1) * k, ow * k:(ow + 1) * k] == y[n, oh, ow]) > 1 for n in range(DP.POOL_NC)
                   for oh in range(H // k) for ow in range(W // k)) or H * W <= 4, 'no window holds a tie'
    # explicit loop: strict '>' scan in row-major order
    for n in range(DP.POOL_NC):
        for oh in range(H // k):
            for ow in range(W // k):
                best, at = None, None
                for a in range(k):
                    for b in range(k):
                        v = x[n, oh * k + a, ow * k + b]
                        if best is None or v > best:
                            best, at = v, (oh * k + a) * W + ow * k + b
                assert y[n, oh, ow] == best and arg[n, oh, ow] == at
    xt = t64(x, True)
    yt = F.max_pool2d(xt[:, None], k, k)
    agree(y.astype(np.float64), yt[:, 0], 'maxpool forward', 0)
    gy = rng.standard_normal(y.shape).astype(np.float32)
    yt.backward(t64(gy)[:, None])
    gx = DP.maxpool_bwd_ref(arg, gy, H, W)
    agree(gx.astype(np.float64), xt.grad, 'maxpool backward', 0)
    assert (gx[:, (H // k) * k:, :] == 0).all() and (gx[:, :, (W // k) * k:] == 0).all()


@pytest.mark.parametrize('NC,HW', DP.GAP_CASES)
def test_gap_reference(NC, HW):
    autograd_check(DP.taps_gap(HW), lambda x: x.mean(1, keepdim=True), (HW,), 'gap %d' % HW, nc=NC)


@pytest.mark.parametrize('H,W', DP.UPSAMPLE2_SHAPES)
def test_upsample2_reference(H, W):
    autograd_check(DP.taps_upsample2(H, W), lambda x: F.interpolate(x[:, None], scale_factor=2, mode='nearest'), (H, W),
                   'upsample2 %dx%d' % (H, W))


@pytest.mark.parametrize('H,W,pad', DP.REFLECT_PAD_CASES)
def test_reflect_pad_reference(H, W, pad):
    autograd_check(DP.taps_reflect_pad(H, W, pad), lambda x: F.pad(x[:, None], (pad,) * 4, mode='reflect'), (H, W),
                   'reflect %dx%d p%d' % (H, W, pad))


@pytest.mark.parametrize('H,W,pad', DP.REPLICATE_PAD_CASES)
def test_replicate_pad_reference(H, W, pad):
    autograd_check(DP.taps_replicate_pad(H, W, pad), lambda x: F.pad(x[:, None], (pad,) * 4, mode='replicate'), (H, W),
                   'replicate %dx%d p%d' % (H, W, pad))


@pytest.mark.parametrize('NC,H,W,pad,ups', [c for c in DP.PAD_UPSAMPLE_CASES if c[0] < 100])
def test_pad_upsample_reference(NC, H, W, pad, ups):
    def fn(x):
        y = x[:, None]
        if ups == 2:
            y = F.interpolate(y, scale_factor=2, mode='nearest')
        return F.pad(y, (pad,) * 4, mode='reflect') if pad else y
    t = DP.taps_pad_upsample(H, W, pad, ups)
    autograd_check(t, fn, (H, W), 'pad_upsample %dx%d p%d u%d' % (H, W, pad, ups))
    assert t.terms_in().max() <= 9 * ups * ups
    # the explicit loop of the adjoint: every padded position adds into the pixel it was copied from
    g = DP.rng_of('pu').standard_normal((1, t.n_out))
    gx = np.zeros(H * W)
    PW = W * ups + 2 * pad
    for ph in range(H * ups + 2 * pad):
        for pw in range(PW):
            lh, lw = DP._reflect(ph - pad, H * ups), DP._reflect(pw - pad, W * ups)
            gx[(lh // ups) * W + lw // ups] += g[0, ph * PW + pw]
    agree(t.adj(g)[0], gx, 'explicit adjoint')


def test_pad_upsample_cases_cross_the_grid_limit():
    ncs = sorted(c[0] for c in DP.PAD_UPSAMPLE_CASES if c[0] >= DP.GRID_Y_MAX)
    assert ncs == [DP.GRID_Y_MAX, DP.GRID_Y_MAX + 1, DP.GRID_Y_MAX + 2]
    assert all(c[1:3] == (1, 2) for c in DP.PAD_UPSAMPLE_CASES if c[0] >= DP.GRID_Y_MAX)
    assert set((c[3], c[4]) for c in DP.PAD_UPSAMPLE_CASES) >= set((p, u) for p in (0, 1, 3) for u in (1, 2))
    assert any(c[1] * c[4] == 2 and c[3] == 1 for c in DP.PAD_UPSAMPLE_CASES)          # L = 2 with pad 1


@pytest.mark.parametrize('M,C1,C2,R', DP.COND_SPLIT_CASES)
def test_cond_split_reference(M, C1, C2, R):
    def fn(w):
        w = w.reshape(-1, M, C1 + C2, R)
        w1 = w[:, :, :C1].reshape(w.shape[0], -1)
        w2r = w[:, :, C1:].permute(0, 1, 3, 2).reshape(w.shape[0], -1)
        return torch.cat([w1, w2r], 1)
    t = DP.taps_cond_split(M, C1, C2, R)
    autograd_check(t, fn, (M * (C1 + C2) * R,), 'cond_split')
    assert (t.terms_out() == 1).all() and (t.terms_in() == 1).all()                  # a permutation


@pytest.mark.parametrize('KS,stride,pad,ohw', sorted(set((c[0], c[1], c[2], c[4]) for c in DP.COND_WINDOW_CASES)))
def test_cond_window_reference(KS, stride, pad, ohw):
    OH, OW, H, W = DP.cond_window_geometry(KS, stride, pad, ohw)
    t = DP.taps_window(OH, OW, H, W, KS, stride, pad)
    adjoint_identity(t, 'window')                                    # window_sums against bias_act's sum
    assert t.terms_out().max() <= KS * KS and t.terms_in().max() <= OH * OW
    if not DP.cond_window_consistent(KS, stride, pad, ohw):
        return
    # a conv of an all-ones plane with the tap table as its filter IS the window sum; its gradient the window sums
    autograd_check(t, lambda p: F.conv2d(torch.ones(1, 1, H, W, dtype=torch.float64), p.reshape(-1, 1, KS, KS), None, stride,
                                         pad)[0], (KS * KS,), 'window', nc=3)


def test_cond_window_cases_are_the_full_product():
    assert len(set(DP.COND_WINDOW_CASES)) == 3 * 2 * 3 * 3 * 4
    assert set(c[4] ** 2 for c in DP.COND_WINDOW_CASES) == {1, 9, 64, 100}
    assert set(c[3] for c in DP.COND_WINDOW_CASES) == {1, 5, 8} and 5 % DP.PLANES_PER_BLOCK and 8 % DP.PLANES_PER_BLOCK == 0


@pytest.mark.parametrize('Cout,Cin', DP.FOLD_CASES)
def test_upconv3_fold_reference(Cout, Cin):
    t = DP.taps_upconv3_fold(Cout, Cin)
    adjoint_identity(t, 'fold')
    assert t.terms_out().max() == 4 and t.terms_in().max() == 4
    # what the fold is for: conv3x3(pad 1) of the x2 nearest upsample == convT(k4, s2, p1) with the folded weights
    rng = DP.rng_of('fold_%d_%d' % (Cout, Cin))
    w, x = rng.standard_normal((Cout, Cin, 3, 3)), rng.standard_normal((2, Cin, 3, 4))
    wt = t.fwd(w.reshape(1, -1)).reshape(Cin, Cout, 4, 4)
    a = F.conv2d(F.interpolate(t64(x), scale_factor=2, mode='nearest'), t64(w), None, 1, 1)
    b = F.conv_transpose2d(t64(x), t64(wt), None, 2, 1)
    agree(b, a, 'sub-pixel identity', 1e-11)
    # the unfold in its documented fp32 order against the adjoint
    gwt = DP.f32(rng, (Cin, Cout, 4, 4))
    agree(DP.unfold_fp32(gwt, Cout, Cin).reshape(1, -1).astype(np.float64), t.adj(gwt.reshape(1, -1)), 'unfold', 1e-6)


@pytest.mark.parametrize('act', DP.ACTS)
def test_act_references(act):
    for slope in DP.ACT_SLOPES:
        x = DP.act_inputs(257, 'cpu')
        xt = t64(x, True)
        s = float(np.float32(slope))
        y = (F.relu(xt) if act == DP.ACT_RELU else F.leaky_relu(xt, s) if act == DP.ACT_LEAKY else torch.tanh(xt)
             if act == DP.ACT_TANH else torch.sigmoid(xt) if act == DP.ACT_SIGMOID else xt * 1.0)
        ref = DP.act_ref(x, act, slope)
        agree(ref, y, 'act forward')
        g = DP.f32(DP.rng_of('actg'), x.shape)
        y.backward(t64(g))
        got = DP.act_bwd_ref(ref, g, act, slope)          # from the float64 OUTPUT
        keep = np.ones(x.shape, bool) if act not in (DP.ACT_RELU, DP.ACT_LEAKY) else x != 0      # the kink: a convention
        agree(got[keep], xt.grad.numpy()[keep], 'act backward', 1e-9)
    assert set(DP.ACT_SPECIALS) >= {0.0, 90.0, -90.0} and any(np.signbit(np.float32(v)) and v == 0 for v in DP.ACT_SPECIALS)


def test_axpy_cases_reach_both_kernels():
    vec = [(n, oy, ox) for n, oy, ox in DP.AXPY_CASES if n and n % 4 == 0 and oy % 4 == 0 and ox % 4 == 0]
    scal_n = [(n, oy, ox) for n, oy, ox in DP.AXPY_CASES if n % 4]
    scal_p = [(n, oy, ox) for n, oy, ox in DP.AXPY_CASES if n and n % 4 == 0 and (oy % 4 or ox % 4)]
    assert vec and scal_n and scal_p and any(oy % 4 and not ox % 4 for _, oy, ox in scal_p) and any(
        ox % 4 and not oy % 4 for _, oy, ox in scal_p)
    assert any(n == 0 for n, _, _ in DP.AXPY_CASES)
