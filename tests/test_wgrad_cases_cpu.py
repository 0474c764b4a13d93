"""The case table of tests/wgrad_cases.py, checked without a GPU: the float64 restatements agree with torch.autograd on F.conv2d
over the explicitly padded, upsampled and concatenated input; one-hot probes in fp32 are exact; every row has the plan it claims
(the library's host-only query sg_conv2d_wgrad_plan, which loads without a device); the table as a whole reaches every value of
every plan field; the Python restatement of the plan equals the query over a grid of shapes; the query rejects bad arguments; and
the restated constants are the ones in the sources."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as WG
import transposed_conv_cases as T
from gpu_harness import options
from scene_generation_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'scene_generation_amd', 'csrc')
RTOL = 1e-12
SHAPES = list(dict((c['shape_key'], c) for c in WG.CASES).values())


def agree(got, want, name):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max())) if want.size else 1.0
    assert float(np.abs(got - want).max()) <= RTOL * scale, name


def case_plan(lib, case, a_mod16=None, opts=None):
    """(the plan the query reports for the row as tests/test_gpu_wgrad.py launches it, the bytes it offers)"""
    d = WG.case_desc(case)
    a = 4 * case['a_off'] if a_mod16 is None else a_mod16
    with options(dict(case['opts'], **(opts or {}))):
        q = lambda ws: WG.wgrad_plan(lib, d, WG.ENTRY_OF[case['kind']], case['L'], a, ws)
        ws = WG.case_ws_bytes(case, q)
        return q(ws), ws


# =============================================================================================
# the references
# =============================================================================================
def _torch_images(case, gy, x):
    """per-image weight gradients [N, M, C, KS, KS] by autograd over the explicitly built input"""
    xt = torch.from_numpy(x)
    if case['ups'] == 2:
        xt = F.interpolate(xt, scale_factor=2, mode='nearest')
    p = case['pad']
    if p:
        xt = F.pad(xt, (p,) * 4, mode='reflect' if case['reflect'] else 'constant')
    out = []
    for b in range(x.shape[0]):
        w = torch.zeros(case['Cout'], x.shape[1], case['KS'], case['KS'], dtype=torch.float64, requires_grad=True)
        F.conv2d(xt[b:b + 1], w, stride=case['stride']).backward(torch.from_numpy(gy[b:b + 1]))
        out.append(w.grad.numpy())
    return np.stack(out)


@pytest.mark.parametrize('case', SHAPES, ids=lambda c: c['name'])
def test_references_agree_with_autograd(case):
    inp = WG.case_inputs(case)
    gy = inp['gy'].astype(np.float64)
    x2 = None
    if inp['x2'] is not None:
        x2 = inp['x2'].astype(np.float64)
        if case['bcast']:
            x2 = np.ascontiguousarray(np.repeat(np.repeat(x2[:, :, None, None], case['H'], axis=2), case['W'], axis=3))
    x = inp['x1'].astype(np.float64) if x2 is None else np.concatenate([inp['x1'].astype(np.float64), x2], axis=1)
    g = _torch_images(case, gy, x)
    ref = WG.case_refs(case)
    if case['kind'] == 'dense':
        want = g.sum(axis=0)
    elif case['kind'] == 'sparse':
        want = np.zeros(g.shape[1:])
        for b in range(case['N']):
            for c in inp['lists'][b][:inp['cnt'][b]]:
                want[:, c] += g[b][:, c]
    else:
        want = np.zeros((case['N'], case['Cout'], case['L'], case['KS'], case['KS']))
        for b in range(case['N']):
            for j in range(inp['cnt'][b]):
                want[b, :, j] = g[b][:, inp['lists'][b][j]]
    agree(ref['gw'], want, 'gw')
    agree(ref['gb'], gy.sum(axis=(0, 2, 3)), 'gb')
    # the term counts are the restatement on ones: whole numbers, at most N * OH * OW (times the images for a sparse channel)
    assert np.array_equal(ref['terms'], np.round(ref['terms'])) and ref['terms'].max() <= case['N'] * case['OH'] * case['OW']
    assert (ref['sabs'] >= np.abs(ref['gw']) - 1e-9).all()


@pytest.mark.parametrize('case', [c for c in SHAPES if c['kind'] != 'dense'], ids=lambda c: c['name'])
def test_channel_lists_hold_what_the_table_says(case):
    lists, cnt = WG.case_lists(case)
    C = case['C1'] + case['C2']
    listed = [set(int(c) for c in lists[b][:cnt[b]]) for b in range(case['N'])]
    assert all(len(s) == cnt[b] for b, s in enumerate(listed)), 'a channel twice in one list'
    assert all(0 <= c < C for s in listed for c in s)
    assert C - 1 not in set().union(*listed), 'the last channel is listed by nobody'
    assert any(all(c not in s for s in listed[1:]) for c in listed[0]), 'a channel of image 0 alone'
    assert cnt[0] == case['L']
    if case['N'] > 1 and case['L'] > 1:
        assert len(set(int(n) for n in cnt)) > 1, 'images of different length'
    for b in range(case['N']):
        ch = [int(c) for c in lists[b][:cnt[b]]]
        assert cnt[b] < 2 or ch != sorted(ch), 'a sorted list'
    if case['kind'] == 'sparse':
        ref = WG.case_refs(case)
        assert not ref['gw'][:, C - 1].any() and not ref['terms'][:, C - 1].any()      # gradient exactly zero


def _onehot(shape, idx):
    a = np.zeros(shape, dtype=np.float32)
    a[idx] = 1.0
    return a


@pytest.mark.parametrize('case', [WG.BY_NAME[n] for n in ('g_40x3_k4s2_16x16', 'g_40x3_k7r_8x8', 'g_40x4_k3_up2_8x8',
                                                          'two_24x7+3_k4s2_9x10_bcast', 'two_40x50+30_k3r_6x8')], ids=lambda c: c['name'])
def test_onehot_probes_are_exact_in_fp32(case):
    """gy a one-hot at (n, m, oh, ow): gw[m, c, kh, kw] is the input value that pixel reads at that tap, bit for bit"""
    inp = WG.case_inputs(case)
    x = WG.sources(inp['x1'], inp['x2'], case['bcast'])
    rng = WG.rng_of(case['name'] + '|probe')
    KS, s, p, ups = case['KS'], case['stride'], case['pad'], case['ups']
    LH, LW = case['H'] * ups, case['W'] * ups
    for _ in range(6):
        n, m, oh, ow = (int(rng.randint(0, k)) for k in (case['N'], case['Cout'], case['OH'], case['OW']))
        gy = _onehot(inp['gy'].shape, (n, m, oh, ow))
        got = WG.conv_wgrad(gy, x, KS, s, p, case['reflect'], ups)
        assert got.dtype == np.float32
        want = np.zeros_like(got)
        for kh in range(KS):
            for kw in range(KS):
                lh, lw = oh * s - p + kh, ow * s - p + kw
                if case['reflect']:
                    lh, lw = WG._reflect(lh, LH), WG._reflect(lw, LW)
                if 0 <= lh < LH and 0 <= lw < LW:
                    want[m, :, kh, kw] = x[n, :, lh // ups, lw // ups]
        assert np.array_equal(got, want)


# =============================================================================================
# the plans
# =============================================================================================
def test_every_row_has_the_plan_it_claims():
    lib = _hip.lib()
    for c in WG.CASES:
        got, ws = case_plan(lib, c)
        assert got is not None, (c['name'], lib.sg_last_error_string().decode())
        assert c['claims'], c['name']
        for k, v in c['claims'].items():
            assert got[k] == v, '%s: plan field %s is %s, the table claims %s (%s)' % (c['name'], k, got[k], v, got)
        assert got == WG.case_py_plan(c, 4 * c['a_off'], ws), c['name']
        assert got['ws_needed'] <= max(ws, 0), (c['name'], got, ws)
        assert got['ws_needed'] <= WG.AMPLE


def test_the_table_reaches_every_plan_value():
    lib = _hip.lib()
    plans = [(c, case_plan(lib, c)[0]) for c in WG.CASES]
    seen = lambda f, kind=None: {p[f] for c, p in plans if kind is None or c['kind'] == kind}
    assert seen('form') == {WG.WG_TAP, WG.WG_GATHER, WG.WG_PADDED}
    assert {(p['form'], p['bm'], p['bn']) for c, p in plans} == {
        (WG.WG_TAP, 128, 128), (WG.WG_TAP, 64, 64), (WG.WG_TAP, 32, 128), (WG.WG_GATHER, 64, 64), (WG.WG_GATHER, 32, 128),
        (WG.WG_PADDED, 64, 64), (WG.WG_PADDED, 32, 128)}
    assert seen('cpad') == {0, 64, 128, 192, 256}
    assert seen('reduce') == {WG.WR_NONE, WG.WR_SLAB, WG.WR_WIDE, WG.WR_UNPERMUTE, WG.WR_SPARSE, WG.WR_PERIMAGE, WG.WR_GROUP}
    assert seen('xcd') == {0, 1, 2} and seen('rowsum_fused') == {0, 1} and seen('two') == {0, 1}
    # A width and mask per tap-major tile, dense and with channel lists
    assert {(p['bm'], p['a_vec']) for c, p in plans if p['form'] == WG.WG_TAP and c['kind'] == 'dense'} == {
        (128, 0), (128, 1), (64, 0), (64, 1), (32, 0), (32, 1)}
    assert {(p['a_vec'], p['nomask']) for c, p in plans if c['kind'] == 'sparse'} == {(0, 0), (1, 1), (1, 0)}
    assert {p['nomask'] for c, p in plans if p['form'] == WG.WG_TAP and c['kind'] == 'dense' and not p['two']} == {0, 1}
    assert {(p['form'], p['a_vec']) for c, p in plans if c['kind'] == 'perimage'} == {
        (WG.WG_GATHER, 0), (WG.WG_GATHER, 1), (WG.WG_PADDED, 0), (WG.WG_PADDED, 1), (WG.WG_TAP, 1)}
    # kernel sizes where the loader is instantiated per size
    assert {c['KS'] for c, p in plans if p['form'] == WG.WG_GATHER and c['kind'] == 'dense'} == {1, 3, 4, 7}
    assert {c['KS'] for c, p in plans if p['form'] == WG.WG_GATHER and c['kind'] == 'perimage'} == {3, 4, 7}
    assert {c['KS'] for c, p in plans if p['form'] == WG.WG_TAP} == {1, 3, 4, 7}
    # chunking: one chunk, several, an empty one; the three dense reduces; per-image chunks
    assert {(p['chunks'] == 1, p['chunks'] < p['grid_z']) for c, p in plans if c['kind'] == 'dense'} == {(True, False), (False, False), (False, True)}
    assert any(p['chunks'] < p['grid_z'] and c['reflect'] and p['kchunk'] % 16 == 0 and (c['N'] * c['OH'] * c['OW']) % 16 == 0 for c, p in plans)
    assert any(p['kchunk'] > WG.KBLK and p['kchunk'] % WG.KBLK for c, p in plans if p['form'] == WG.WG_TAP)
    assert any(c['N'] * c['OH'] * c['OW'] < WG.BK for c, p in plans)
    assert {p['grid_z'] // c['N'] for c, p in plans if c['kind'] == 'perimage'} == {1, 4}
    # the bias gradient: fused at every M of the issue, and the fallback
    fused = {c['Cout'] for c, p in plans if p['rowsum_fused']}
    assert fused >= {3, 40, 64, 130}
    assert any(c['gb'] and not p['rowsum_fused'] and p['form'] == WG.WG_TAP for c, p in plans if c['kind'] == 'dense')
    # shrunk splits: to one and to a value in between
    full = lambda c: case_plan(lib, dict(c, ws=WG.AMPLE))[0]['chunks']
    shrunk = {(p['grid_z'], full(c)) for c, p in plans if callable(c['ws']) and c['kind'] == 'dense'}
    assert any(a == 1 and b > 1 for a, b in shrunk) and any(1 < a < b for a, b in shrunk), shrunk
    # sparse rows: the list lengths of the issue, M > 64 with L >= 48
    assert {c['L'] for c in WG.CASES if c['kind'] == 'sparse'} >= {2, 48, 70}
    assert any(c['Cout'] > 64 and c['L'] >= 48 for c in WG.CASES if c['kind'] == 'sparse')
    assert {c['bcast'] for c in WG.CASES if c['C2']} == {0, 1}
    for c in WG.CASES:               # the size limits of the table
        assert c['N'] * c['OH'] * c['OW'] <= 6200 and max(c['Cout'], c['C1'] + c['C2']) <= 140, c['name']


def test_the_table_reaches_every_dense_tap_kernel():
    """plan_classes() of the table holds every one-source instantiation launch_nk_tap can pick: tile x A width x mask"""
    lib = _hip.lib()
    have = set()
    for c in WG.CASES:
        have |= WG.plan_classes(c, case_plan(lib, c)[0])
    kernels = {k for k in have if k[0] == 'kernel'}
    # every (form, tile, A width, sources, mask) instantiation launch_nk_tap / launch_nk_general / launch_nk_padded can pick
    want = set()
    for bm, bn in ((128, 128), (64, 64), (32, 128)):
        for a_vec in (0, 1):
            want |= {('kernel', WG.WG_TAP, bm, bn, a_vec, 0, 0, 0, False), ('kernel', WG.WG_TAP, bm, bn, a_vec, 0, 1, 0, False)}
    assert not want - kernels, sorted(want - kernels)


GRID_M = (3, 32, 33, 64, 65, 130)
GRID_C = ((3, 0), (47, 0), (48, 0), (64, 0), (70, 0), (129, 0), (7, 3), (50, 30))
GRID_PLANES = ((1, 3, 3), (1, 5, 5), (1, 7, 9), (2, 8, 8), (3, 16, 16), (1, 28, 28), (1, 43, 48), (6, 32, 32), (2, 32, 32), (5, 20, 20))


def test_python_plan_equals_the_query_over_a_grid():
    lib = _hip.lib()
    n = 0
    for xcd, rowsum in ((1, 1), (0, 1), (1, 0)):
        with options({'wgrad_xcd': xcd, 'wgrad_rowsum': rowsum}):
            for M, (C1, C2), (N, OH, OW), KS, reflect, a in itertools.product(GRID_M, GRID_C, GRID_PLANES, (1, 3, 4, 7), (0, 1), (0, 4)):
                pad = (KS - 1) // 2
                H, W = OH + KS - 1 - 2 * pad, OW + KS - 1 - 2 * pad
                if reflect and (pad == 0 or pad >= min(H, W)):
                    continue
                d = WG.make_desc(N, C1, H, W, M, KS, 1, pad, reflect, 1, OH, OW, C2=C2)
                mn = M * KS * KS * 256
                for ws in (WG.AMPLE, 3 * mn * 4 // 4, 0):
                    got = WG.wgrad_plan(lib, d, WG.WG_CONV, 0, a, ws)
                    want = WG.py_plan(WG.WG_CONV, N, C1, C2, H, W, M, KS, 1, pad, reflect, 1, OH, OW, a_mod16=a, ws_bytes=ws, xcd=xcd,
                                      rowsum=rowsum)
                    assert got == want, (M, C1, C2, N, OH, OW, KS, reflect, a, ws, got, want)
                    n += 1
    assert n > 3000
    # stride 2 / upsample / the transposed entry / the list forms
    for M, C, L, (N, OH, OW), KS, reflect, padded in itertools.product((8, 40, 72), (30, 80), (1, 3, 21, 22, 48, 70), GRID_PLANES[:6] + GRID_PLANES[8:9],
                                                                      (3, 4, 7), (0, 1), (0, 1)):
        if L > C:
            continue
        stride = 2 if KS == 4 else 1
        pad = 1 if KS == 4 else (KS - 1) // 2
        H, W = (OH * 2, OW * 2) if KS == 4 else (OH, OW)
        if reflect and pad >= min(H, W):
            continue
        d = WG.make_desc(N, C, H, W, M, KS, stride, pad, reflect, 1, OH, OW)
        with options({'wgrad_padded': padded}):
            for entry in (WG.WG_SPARSE, WG.WG_PERIMAGE):
                base = WG.sparse_base_ws(N, M, C, L, KS)
                assert base == lib.sg_conv2d_sparse_ws_bytes(ctypes.byref(d), L, 2) or WG.padded_bytes(KS, N, L, 0, H, W, 1, OH, OW, stride, pad, reflect)
                for ws in (max(WG.AMPLE, base), base, base - 4):
                    got = WG.wgrad_plan(lib, d, entry, L, 0, ws)
                    want = WG.py_plan(entry, N, C, 0, H, W, M, KS, stride, pad, reflect, 1, OH, OW, L=L, ws_bytes=ws, padded=padded)
                    assert got == want, (entry, M, C, L, N, OH, OW, KS, reflect, padded, ws, got, want)
                    n += 1
    for M, C, (N, OH, OW), KS in itertools.product((5, 40, 130), (3, 64), GRID_PLANES[:6], (1, 3, 4, 7)):
        # sg_convT2d_wgrad of a C -> M ... transposed conv runs the GEMM with the roles swapped: rows = its C1, gathered = its gy
        s, p = (2, 1) if KS >= 3 else (1, 0)
        TH, TW = T.convT_out_size(OH, KS, s, p, 0), T.convT_out_size(OW, KS, s, p, 0)
        d = WG.make_desc(N, M, OH, OW, C, KS, s, p, False, 1, TH, TW)
        got = WG.wgrad_plan(lib, d, WG.WG_CONVT, 0, 0, WG.AMPLE)
        want = WG.py_plan(WG.WG_CONVT, N, C, 0, TH, TW, M, KS, s, p, 0, 1, OH, OW, rowsum=1)
        assert got == want, (M, C, N, OH, OW, KS, got, want)
        assert got['rowsum_fused'] == 0
        n += 1
    print('%d plans compared' % n)


def test_query_rejects_bad_arguments():
    lib = _hip.lib()
    p = WG.sgWgradPlan()
    d = WG.make_desc(1, 4, 5, 5, 4, 3, 1, 1, False, 1, 5, 5)
    q = lambda d, e, L=0, a=0, ws=WG.AMPLE, plan=p: lib.sg_conv2d_wgrad_plan(None if d is None else ctypes.byref(d), e, L, a, ws,
                                                                           None if plan is None else ctypes.byref(plan))
    assert q(d, WG.WG_CONV) == 0
    assert q(None, WG.WG_CONV) != 0 and b'bad arguments' in lib.sg_last_error_string()
    assert q(d, WG.WG_CONV, plan=None) != 0
    assert q(d, -1) != 0 and q(d, 4) != 0
    assert q(d, WG.WG_CONV, a=2) != 0 and b'a_mod16' in lib.sg_last_error_string()
    assert q(d, WG.WG_SPARSE, L=0) != 0 and q(d, WG.WG_SPARSE, L=5) != 0 and b'L=5' in lib.sg_last_error_string()
    assert q(d, WG.WG_PERIMAGE, L=2, ws=16) != 0 and b'workspace too small' in lib.sg_last_error_string()
    bad = WG.make_desc(1, 4, 5, 5, 4, 5, 1, 1, False, 1, 5, 5)
    assert q(bad, WG.WG_CONV) != 0 and b'kernel size' in lib.sg_last_error_string()
    refl = WG.make_desc(1, 4, 5, 5, 4, 3, 1, 1, True, 1, 5, 5)
    assert q(refl, WG.WG_CONVT) != 0 and b'unsupported desc' in lib.sg_last_error_string()
    tap = WG.make_desc(1, 64, 8, 8, 64, 3, 1, 1, False, 1, 8, 8)
    assert q(tap, WG.WG_CONV, ws=0) != 0 and b'workspace too small' in lib.sg_last_error_string()      # tap-major needs its slab


# =============================================================================================
# constants against the sources
# =============================================================================================
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_restated_constants_match_the_sources():
    core, nk, ig = _src('igemm_core.h'), _src('igemm_nk.hip'), _src('igemm.hip')
    assert int(re.search(r'constexpr int BK = (\d+);', core).group(1)) == WG.BK
    assert int(re.search(r'constexpr int KBLK = (\d+);', core).group(1)) == WG.KBLK
    assert re.search(r'#define SG_NSW 1\b', core)                     # k-tile depth of the weight-gradient tiles = BK
    assert re.search(r'kchunk = sparse \? PQ : sg_cdiv\(sg_cdiv\(Kpix, splits\), %d\) \* %d;' % (WG.CHUNK_ROUND, WG.CHUNK_ROUND), core)
    assert 'const int cap = p.tap ? %d : %d;' % (WG.CAP_TAP, WG.CAP_GATHER) in core
    assert 'const int target = p.tile == 0 ? %d : %d;' % (WG.TARGET_128, WG.TARGET) in core
    assert 'int S = (int)((%d + tiles - 1) / tiles);' % WG.FEW_TARGET in core
    assert 'if (S > %d / Ccols) S = %d / Ccols;' % (WG.FEW_COLS, WG.FEW_COLS) in core and 'if (S > PQ / %d) S = PQ / %d;' % (WG.FEW_PIX, WG.FEW_PIX) in core
    assert 'constexpr size_t PAD_MAX_BYTES = (size_t)1 << 30;' in core and WG.PAD_MAX_BYTES == 1 << 30
    # ONE function holds the decisions: the launcher and the query call it, nobody restates it
    assert core.count('nk_launch_plan(') == 1 and nk.count('nk_launch_plan(') == 1 and ig.count('nk_launch_plan(') == 1
    assert 'sg_opt(' not in nk[nk.index('int run_nk_ks('):]
    assert 'CfgW64W' not in core + nk                               # the 64x128 tap tile nk_plan could never pick is gone
    body = core[core.index('inline NkPlan nk_plan('):core.index('// THE launch plan of a weight-gradient GEMM')]
    assert 'p.tile = M <= 32 ? 2 : 1;' in body and 'p.tile = 0;' in body and body.count('p.tile = ') == 2      # never tile 3
    text = open(os.path.join(ROOT, 'include', 'sg2im_hip.h')).read()
    vals = dict((k, int(v)) for k, v in re.findall(r'(SG_W[GR]_\w+)\s*=\s*(\d+)', text))
    assert [vals[k] for k in ('SG_WG_CONV', 'SG_WG_SPARSE', 'SG_WG_PERIMAGE', 'SG_WG_CONVT')] == [WG.WG_CONV, WG.WG_SPARSE, WG.WG_PERIMAGE, WG.WG_CONVT]
    assert [vals[k] for k in ('SG_WG_TAP', 'SG_WG_GATHER', 'SG_WG_PADDED')] == [WG.WG_TAP, WG.WG_GATHER, WG.WG_PADDED]
    assert [vals[k] for k in ('SG_WR_NONE', 'SG_WR_SLAB', 'SG_WR_WIDE', 'SG_WR_UNPERMUTE', 'SG_WR_SPARSE', 'SG_WR_PERIMAGE', 'SG_WR_GROUP')] == list(range(7))
    body = re.search(r'typedef struct sgWgradPlan \{(.*?)\} sgWgradPlan;', text, re.S).group(1)
    names = re.findall(r'(\w+)\s*[,;]', body)
    assert tuple(names) == WG.PLAN_FIELDS + ('ws_needed',) and 'int64_t ws_needed;' in body
    assert ctypes.sizeof(WG.sgWgradPlan) == 4 * len(WG.PLAN_FIELDS) + 8
