"""The case table of tests/transposed_conv_cases.py, checked without a GPU: every float64 restatement agrees with an independent
formulation (torch double, autograd for the gradients), every forward / adjoint pair satisfies <A x, g> == <x, A^T g>, the one-hot
placements equal the restatements, the parity-class geometry restated in Python is what sg_conv2d_tgather_plan reports over a grid
of descriptors, the table -- as tests/test_gpu_transposed_conv.py runs it -- reaches every plan class that grid can produce, and the
restated constants are the ones in the sources."""
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transposed_conv_cases as T
from gpu_harness import options
from scene_generation_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'scene_generation_amd', 'csrc')
RTOL = 1e-12


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def agree(got, want, name):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max())) if want.size else 1.0
    assert float(np.abs(got - want).max()) <= RTOL * scale, name


def in64(case):
    return {k: (None if v is None else v.astype(np.float64)) for k, v in T.case_inputs(case).items()}


# =============================================================================================
# the references against torch double
# =============================================================================================
@pytest.mark.parametrize('case', T.CONVT_CASES, ids=lambda c: c['name'])
def test_convT_references_agree_with_torch(case):
    s, p, op, KS = case['stride'], case['pad'], case['out_pad'], case['KS']
    i = in64(case)
    x, w = t64(i['x']).requires_grad_(), t64(i['w']).requires_grad_()
    b = None if i['b'] is None else t64(i['b']).requires_grad_()
    y = F.conv_transpose2d(x, w, b, stride=s, padding=p, output_padding=op)
    agree(T.convT_fwd(i['x'], i['w'], i['b'], s, p, op), y.detach().numpy(), 'y')
    y.backward(t64(i['gy']))
    agree(T.convT_dgrad(i['gy'], i['w'], s, p, case['H'], case['W']), x.grad.numpy(), 'gx')
    agree(T.convT_wgrad(i['gy'], i['x'], KS, s, p), w.grad.numpy(), 'gw')
    if b is not None:
        agree(T.bias_grad(i['gy']), b.grad.numpy(), 'gb')
    # adjoint pair: <convT(x), gy> == <x, convT_dgrad(gy)>, and the weight gradient is the adjoint in w
    y0 = T.convT_fwd(i['x'], i['w'], None, s, p, op)
    lhs = float((y0 * i['gy']).sum())
    assert abs(lhs - float((i['x'] * T.convT_dgrad(i['gy'], i['w'], s, p, case['H'], case['W'])).sum())) <= RTOL * max(1.0, abs(lhs))
    assert abs(lhs - float((i['w'] * T.convT_wgrad(i['gy'], i['x'], KS, s, p)).sum())) <= RTOL * max(1.0, abs(lhs))


def _logical_input(x, case):
    """the logical grid of a conv input as torch builds it: nearest x2, then ReflectionPad2d"""
    if case['ups'] == 2:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    if case['reflect']:
        x = F.pad(x, (case['pad'],) * 4, mode='reflect')
    return x


@pytest.mark.parametrize('case', T.DGRAD_CASES + T.FOLDED_CASES, ids=lambda c: c['name'])
def test_dgrad_references_agree_with_torch(case):
    entry, d, c0, c1 = T.case_desc(case)
    i = in64(case)
    rng = T.rng_of(case['name'] + '/x')
    x = t64(rng.standard_normal((d.N, d.C1, d.H, d.W))).requires_grad_()
    xl = _logical_input(x, case)
    xl.retain_grad()
    pz = 0 if case['reflect'] else case['pad']
    y = F.conv2d(xl, t64(i['w']), None, stride=d.stride, padding=pz)
    assert tuple(y.shape) == (d.N, d.Cout, d.OH, d.OW), (tuple(y.shape), d.OH, d.OW)
    y.backward(t64(i['gy']))
    if case['kind'] == 'folded':
        ref = T.conv_dgrad_folded(i['gy'], i['w'], d.H, d.W, c0, c1)
        agree(ref, x.grad.numpy()[:, c0:c1], 'folded gx')
        lhs = float((y.detach().numpy() * i['gy']).sum())         # <A x, g> == <x, A^T g> over all channels
        full = T.conv_dgrad_folded(i['gy'], i['w'], d.H, d.W, 0, d.C1)
        assert abs(lhs - float((x.detach().numpy() * full).sum())) <= RTOL * max(1.0, abs(lhs))
        return
    r = T.dgrad_refs(case, T.case_inputs(case))
    agree(r['g'], xl.grad.numpy()[:, c0:c1], 'logical-grid gradient')
    if 'gx' in r:
        agree(r['gx'], x.grad.numpy()[:, c0:c1], 'gradient folded onto the stored input')
    GH, GW = xl.shape[2:]
    full = T.conv_dgrad_logical(i['gy'], i['w'], d.stride, pz, GH, GW, 0, d.C1)
    lhs = float((y.detach().numpy() * i['gy']).sum())
    assert abs(lhs - float((xl.detach().numpy() * full).sum())) <= RTOL * max(1.0, abs(lhs))
    assert (np.asarray(r['g_bound']) >= 0).all()


def test_fold_pad_upsample_is_the_adjoint_of_pad_after_upsample():
    rng = T.rng_of('fold')
    for H, W, pad, ups in ((3, 4, 1, 1), (5, 7, 3, 1), (4, 5, 0, 2), (3, 4, 1, 2), (1, 1, 1, 2)):
        x = t64(rng.standard_normal((2, 3, H, W))).requires_grad_()
        xl = F.interpolate(x, scale_factor=2, mode='nearest') if ups == 2 else x
        xl = F.pad(xl, (pad,) * 4, mode='reflect') if pad else xl
        g = rng.standard_normal(tuple(xl.shape))
        xl.backward(t64(g))
        agree(T.fold_pad_upsample(g, H, W, pad, ups), x.grad.numpy(), (H, W, pad, ups))


@pytest.mark.parametrize('cin,cout', T.SUBPIXEL_FOLD_CHANNELS)
def test_weight_fold_and_its_adjoint(cin, cout):
    rng = T.rng_of('fold_%d_%d' % (cin, cout))
    w, gwt = rng.standard_normal((cout, cin, 3, 3)), rng.standard_normal((cin, cout, 4, 4))
    wt = T.upconv3_fold(w)
    lhs = float((wt * gwt).sum())
    assert abs(lhs - float((w * T.upconv3_unfold(gwt)).sum())) <= RTOL * max(1.0, abs(lhs))
    # the fold is what makes the transposed conv equal conv3x3(pad 1) of the upsampled input
    x = rng.standard_normal((2, cin, 3, 5))
    want = F.conv2d(F.interpolate(t64(x), scale_factor=2, mode='nearest'), t64(w), None, padding=1).numpy()
    agree(T.convT_fwd(x, wt, None, 2, 1, 0), want, 'sub-pixel forward')
    agree(T.conv_fwd(T.nearest_up2(x), w, 1, 1), want, 'plain conv restatement')
    # pure copies: the corner taps of wt are single taps of w
    for kh, i in ((0, 2), (3, 0)):
        for kw, j in ((0, 2), (3, 0)):
            assert np.array_equal(wt[:, :, kh, kw], w[:, :, i, j].T)


@pytest.mark.parametrize('case', T.SUBPIXEL_CASES, ids=lambda c: c['name'])
def test_subpixel_references_agree_with_torch(case):
    i = in64(case)
    x, w = t64(i['x']).requires_grad_(), t64(i['w']).requires_grad_()
    b = None if i['b'] is None else t64(i['b']).requires_grad_()
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, b, padding=1)
    r = T.subpixel_refs(case, T.case_inputs(case))
    agree(r['y'], y.detach().numpy(), 'y')
    y.backward(t64(i['gy']))
    agree(r['gx'], x.grad.numpy(), 'gx')
    agree(r['gw'], w.grad.numpy(), 'gw')
    if b is not None:
        agree(r['gb'], b.grad.numpy(), 'gb')


# =============================================================================================
# one-hot placements == restatements
# =============================================================================================
@pytest.mark.parametrize('case', T.PROBE_CONVT, ids=lambda c: c['name'])
def test_convT_onehot_placement_is_the_restatement(case):
    s, p, op, KS, H, W, N, Ci, Co = [case[k] for k in ('stride', 'pad', 'out_pad', 'KS', 'H', 'W', 'N', 'Cin', 'Cout')]
    inp = T.case_inputs(case)
    OH, OW = inp['gy'].shape[2:]
    classes = set()
    for site in T.probe_sites(N, Ci, H, W):
        x1 = T.onehot((N, Ci, H, W), *site)
        assert np.array_equal(T.place_convT_fwd(site, x1.shape, inp['w'], inp['b'], s, p, op), T.convT_fwd(x1, inp['w'], inp['b'], s, p, op))
        assert np.array_equal(T.place_convT_wgrad(site, inp['gy'], Ci, KS, s, p), T.convT_wgrad(inp['gy'], x1, KS, s, p))
    for site in T.probe_sites(N, Co, OH, OW):
        g1 = T.onehot((N, Co, OH, OW), *site)
        assert np.array_equal(T.place_convT_dgrad(site, g1.shape, inp['w'], s, p, H, W), T.convT_dgrad(g1, inp['w'], s, p, H, W))
        classes.add(((site[2][0] + p) % 2, (site[2][1] + p) % 2))
    if s == 2 and min(OH, OW) >= 3:
        assert len(classes) == 4, 'the probe positions miss a parity class of %s' % case['name']


@pytest.mark.parametrize('case', T.PROBE_DGRAD, ids=lambda c: c['name'])
def test_dgrad_onehot_placement_is_the_restatement(case):
    entry, d, c0, c1 = T.case_desc(case)
    inp = T.case_inputs(case)
    pz = 0 if case['reflect'] else case['pad']
    GH = d.H * d.upsample + (2 * d.pad if d.pad_reflect else 0)
    GW = d.W * d.upsample + (2 * d.pad if d.pad_reflect else 0)
    hit = np.zeros((GH, GW), dtype=bool)
    for site in T.probe_sites(d.N, d.Cout, d.OH, d.OW):
        g1 = T.onehot((d.N, d.Cout, d.OH, d.OW), *site)
        want = T.place_conv_dgrad(site, g1.shape, inp['w'], d.stride, pz, GH, GW, c0, c1)
        assert np.array_equal(want, T.conv_dgrad_logical(g1, inp['w'], d.stride, pz, GH, GW, c0, c1))
        hit |= (T.conv_dgrad_logical(g1.astype(np.float64), np.ones_like(inp['w'], dtype=np.float64), d.stride, pz, GH, GW, c0, c1) > 0).any(axis=(0, 1))
    if d.stride == 2 and d.KS >= 3:         # every non-empty parity class of the plane receives a copy
        for _, _, _, ph0, pw0 in T.parity_classes(d.KS, GH, GW, pz):
            assert hit[ph0::2, pw0::2].any(), (case['name'], ph0, pw0)
    for r, c in ((0, 0), (0, GW - 1), (GH - 1, 0), (GH - 1, GW - 1)):       # and every border
        reach = T.conv_dgrad_logical(np.ones((1, 1, d.OH, d.OW)), np.ones((1, 1, d.KS, d.KS)), d.stride, pz, GH, GW, 0, 1)[0, 0, r, c] > 0
        assert hit[r, c] or not reach, (case['name'], r, c)


@pytest.mark.parametrize('case', T.PROBE_FOLDED, ids=lambda c: c['name'])
def test_folded_onehot_placement_is_the_restatement(case):
    """the nine pre-folded copies, placed tap by tap, are the reflect-folded gradient of a one-hot weight"""
    entry, d, c0, c1 = T.case_desc(case)
    gy = in64(case)['gy']
    for kh in range(3):
        for kw in range(3):
            for co, c in ((0, c0), (d.Cout - 1, c1 - 1)):
                w1 = np.zeros((d.Cout, d.C1, 3, 3))
                w1[co, c, kh, kw] = 1.0
                agree(T.place_dgrad_folded_tap(gy, co, c - c0, kh, kw, c1 - c0), T.conv_dgrad_folded(gy, w1, d.H, d.W, c0, c1), (kh, kw, co, c))


# =============================================================================================
# plans: geometry restated, the table's reach
# =============================================================================================
GRID_PLANES = ((1, 1), (1, 5), (2, 2), (3, 3), (4, 1), (5, 7), (8, 8))
GRID_CHANNELS = ((16, 16), (5, 3), (6, 10), (4, 8), (8, 40), (64, 16))
FORCED = ({}, {'tile': 0}, {'tile': 1}, {'tile': 2}, {'tile': 3}, {'splits': 2})


def _grid():
    """(entry, desc, c0, c1, ws_mod16) over small descriptors of the three entry points"""
    for KS in T.KS_VALUES:
        for s in (1, 2):
            for p in (0, 1, 2, 3):
                if p > KS - 1:
                    continue
                for H, W in GRID_PLANES:
                    for Ci, Co in GRID_CHANNELS:
                        for mod in (0, 4, 8):
                            for op in ((0, 1) if s == 2 else (0,)):
                                if T.convT_valid(H, W, KS, s, p, op):
                                    OH, OW = T.convT_out_size(H, KS, s, p, op), T.convT_out_size(W, KS, s, p, op)
                                    yield T.TG_CONVT_FWD, T.make_desc(2, Ci, H, W, Co, KS, s, p, False, 1, OH, OW, op), 0, Co, mod
                            if T.conv_valid(H, W, KS, s, p):
                                OH, OW = T.conv_out_size(H, KS, s, p), T.conv_out_size(W, KS, s, p)
                                for c0, c1 in T._windows(Ci):
                                    yield T.TG_CONV_DGRAD, T.make_desc(2, Ci, H, W, Co, KS, s, p, False, 1, OH, OW), c0, c1, mod
                            if KS == 3 and s == 1 and p == 1 and H >= 3 and W >= 3:
                                for c0, c1 in T._windows(Ci):
                                    yield T.TG_DGRAD_FOLDED, T.make_desc(2, Ci, H, W, Co, 3, 1, 1, True, 1, H, W), c0, c1, mod


@functools.lru_cache(maxsize=None)
def _reachable():
    lib = _hip.lib()
    out = set()
    for forced in FORCED:
        with options(forced):
            for entry, d, c0, c1, mod in _grid():
                out |= T.plan_classes(entry, d.KS, T.tgather_plan(lib, d, entry, c0, c1, mod), bool(forced))
    return out


@functools.lru_cache(maxsize=None)
def _covered():
    """{plan class: a case that reaches it} over the table as tests/test_gpu_transposed_conv.py runs it"""
    lib = _hip.lib()
    out = {}
    for c in T.ALL_CASES:
        entry, d, c0, c1 = T.case_desc(c)
        for o in T.case_options(c):
            with options(o):
                pl = T.tgather_plan(lib, d, entry, c0, c1, 4 * c['ws_off'])
            for k in T.plan_classes(entry, d.KS, pl, bool(c['opts'])):
                out.setdefault(k, c['name'])
    return out


def test_table_reaches_every_plan_class():
    """fails when a case the table relies on is removed: the classes come from the table alone"""
    missing = sorted(_reachable() - set(_covered()), key=repr)
    assert not missing, 'plan classes no case reaches: %s' % missing
    assert {k[1] for k in _covered() if k[0] == 'taps'} == {1, 2, 4, 9, 12, 16, 49}
    assert {k[1] for k in _covered() if k[0] == 'ncls'} == {1, 2, 4}
    assert {k[2] for k in _covered() if k[0] == 'tile'} == {(32, 128), (64, 64), (64, 128), (128, 128)}
    assert {k[3:5] for k in _covered() if k[0] == 'path'} == {(a, b) for a in (T.TG_TABLE, T.TG_FIXED) for b in (0, 1)} - {(T.TG_FIXED, 0)}
    assert sum(k[0] == 'splits>1' for k in _covered()) == 3


def test_geometry_matches_the_query_over_the_grid():
    lib = _hip.lib()
    n = 0
    for entry, d, c0, c1, mod in _grid():
        got = T.tgather_plan(lib, d, entry, c0, c1, mod)
        want = T.expected_plan(entry, d.N, d.C1, d.Cout, d.H, d.W, d.KS, d.stride, d.pad, d.pad_reflect, d.upsample, d.out_pad, c0, c1, mod)
        for k, v in want.items():
            assert got[k] == v, (T.ENTRY_NAMES[entry], k, got, want)
        if got['route'] == T.TG_PARITY:           # the classes tile the plane: every pixel in exactly one class
            GH, GW = (d.OH, d.OW) if entry == T.TG_CONVT_FWD else (d.H, d.W)
            seen = np.zeros((GH + 2, GW + 2), dtype=int)
            for c in range(got['ncls']):
                seen[got['ph0'][c]:got['ph0'][c] + 2 * got['PH'][c]:2, got['pw0'][c]:got['pw0'][c] + 2 * got['PW'][c]:2] += 1
            assert (seen[:GH, :GW] == 1).all() and seen.sum() == GH * GW, (got, GH, GW)
        n += 1
    assert n > 5000


def test_every_case_has_the_plan_it_claims():
    lib = _hip.lib()
    for c in T.ALL_CASES:
        entry, d, c0, c1 = T.case_desc(c)
        e_entry, want = T.case_expected_plan(c)
        for o in T.case_options(c):
            with options(o):
                got = T.tgather_plan(lib, d, entry, c0, c1, 4 * c['ws_off'])
            for k, v in want.items():
                assert got[k] == v, (c['name'], k, got, want)


def test_case_table_holds_what_the_issue_lists():
    convT = {(c['KS'], c['stride'], c['pad'], c['out_pad']) for c in T.CONVT_CASES}
    for KS in T.KS_VALUES:
        for s in (1, 2):
            for p in (0, 1, 2):
                for op in ((0, 1) if s == 2 else (0,)):
                    if p <= KS - 1:
                        assert (KS, s, p, op) in convT, (KS, s, p, op)
    assert any(c['H'] == 1 and c['W'] == 1 for c in T.CONVT_CASES) and any(c['H'] == 1 and c['W'] == 5 for c in T.CONVT_CASES)
    assert any(c['bias'] for c in T.CONVT_CASES) and any(not c['bias'] for c in T.CONVT_CASES)
    assert any(c['Cout'] <= 32 for c in T.CONVT_CASES) and any(c['Cout'] > 32 for c in T.CONVT_CASES)
    dg = {(c['KS'], c['stride'], c['pad']) for c in T.DGRAD_CASES if not c['reflect'] and c['ups'] == 1}
    for KS, pads in ((3, (0, 1, 2)), (4, (0, 1, 2)), (7, (0, 1, 2, 3))):
        for p in pads:
            assert (KS, 2, p) in dg and (KS, 1, p) in dg, (KS, p)
    assert (1, 1, 0) in dg
    assert {(c['KS'], c['pad']) for c in T.DGRAD_CASES if c['reflect']} >= {(3, 1), (7, 3)}
    assert any(c['ups'] == 2 for c in T.DGRAD_CASES)
    assert {(c['H'], c['W']) for c in T.FOLDED_CASES} >= {(3, 3), (3, 5), (8, 8), (9, 6)}
    assert {(c['H'], c['W']) for c in T.SUBPIXEL_CASES} == {(1, 1), (5, 7), (8, 8)}
    s1 = [c for c in T.DGRAD_CASES if c['stride'] == 1 and not c['opts']]
    assert any(c['window'][0] > 0 and (c['window'][0] * c['Cout'] * c['KS'] ** 2) % 4 == 0 for c in s1)       # aligned offset pointer
    assert any(c['window'][0] > 0 and (c['Cout'] * c['KS'] ** 2) % 4 != 0 for c in s1)
    for c in T.ALL_CASES:           # the size limits of the table
        big = c['name'].startswith('route_')
        assert c['N'] <= 4 and c['H'] <= 17 and c['W'] <= 19 and (max(c['Cin'], c['Cout']) <= 128), c['name']
        assert c['opts'].get('splits', 1) <= 8, 'C_GATHER assumes at most eight slabs'
        assert big or not c['opts'], c['name']


# =============================================================================================
# constants against the sources
# =============================================================================================
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_restated_constants_match_the_sources():
    core, kn1, nk, ig = _src('igemm_core.h'), _src('igemm_kn1.hip'), _src('igemm_nk.hip'), _src('igemm.hip')
    assert int(re.search(r'constexpr int BK = (\d+);', core).group(1)) == T.BK
    # C_GATHER: at most eight split-K slabs, eight tail-split pieces, two parity-split halves; all need splits <= 1 of each other
    assert 'if (sp > 8) sp = 8;' in core
    assert re.search(r'sg_opt\(SG_OPT_TAIL_SMAX\) > 8 \? 8', core)
    assert 'bi.par.split[c] = sp2 ? 2 : 1;' in core
    assert core.count('splits <= 1') >= 2
    assert T.C_GATHER == (8 - 1) + 1
    # c_wgrad: k-chunks are multiples of 64
    # (the launcher's decisions live in nk_launch_plan of igemm_core.h, which run_nk_ks of igemm_nk.hip runs from)
    assert re.search(r'kchunk = sparse \? PQ : sg_cdiv\(sg_cdiv\(Kpix, splits\), %d\) \* %d;' % (T.WGRAD_CHUNK, T.WGRAD_CHUNK), core)
    assert 'nk_launch_plan(' in nk
    assert T.c_wgrad(64) == 1 and T.c_wgrad(65) == 2
    # C_VARIANT: a pre-folded value is v00 plus three conditional adds
    body = core[core.index('__global__ void reflect_variants_kernel'):core.index('// Wt[b][a][r] = W[a][b][r]')]
    assert body.count('v += g[') == T.C_VARIANT
    # C_FOLD: four taps at most per folded weight, four per unfolded gradient
    assert max(len(a) * len(b) for a in T._FOLD_R for b in T._FOLD_R) - 1 == T.C_FOLD
    assert 'lo = k == 0 ? 2 : (k == 1 ? 1 : 0);' in ig and 'hi = k == 0 ? 2 : (k == 1 ? 2 : (k == 2 ? 1 : 0));' in ig
    # the class geometry the Python restatement mirrors lives in ONE function shared by the launcher and the query
    assert kn1.count('parity_plan(') == 3 and core.count('kn_plan(') == 2 and kn1.count('kn_plan(') == 1
    text = open(os.path.join(ROOT, 'include', 'sg2im_hip.h')).read()
    vals = dict((k, int(v)) for k, v in re.findall(r'(SG_TG_\w+)\s*=\s*(\d+)', text))
    assert (vals['SG_TG_CONVT_FWD'], vals['SG_TG_CONV_DGRAD'], vals['SG_TG_DGRAD_FOLDED']) == (T.TG_CONVT_FWD, T.TG_CONV_DGRAD, T.TG_DGRAD_FOLDED)
    assert (vals['SG_TG_PLAIN'], vals['SG_TG_PARITY'], vals['SG_TG_TABLE'], vals['SG_TG_FIXED']) == (T.TG_PLAIN, T.TG_PARITY, T.TG_TABLE, T.TG_FIXED)
    assert len(T.sgTGatherPlan._fields_) == 2 + 6 + 6 and 'int32_t taps[4], PH[4], PW[4], ph0[4], pw0[4], K[4];' in text


def test_query_rejects_bad_arguments():
    lib = _hip.lib()
    p = T.sgTGatherPlan()
    import ctypes
    d = T.make_desc(1, 4, 5, 5, 4, 3, 1, 1, False, 1, 5, 5)
    assert lib.sg_conv2d_tgather_plan(ctypes.byref(d), 3, 0, 4, 0, 0, ctypes.byref(p)) != 0
    assert lib.sg_conv2d_tgather_plan(ctypes.byref(d), T.TG_CONV_DGRAD, 2, 2, 0, 0, ctypes.byref(p)) != 0
    assert lib.sg_conv2d_tgather_plan(ctypes.byref(d), T.TG_CONV_DGRAD, 0, 4, 2, 0, ctypes.byref(p)) != 0
    assert lib.sg_conv2d_tgather_plan(ctypes.byref(d), T.TG_DGRAD_FOLDED, 0, 4, 0, 0, ctypes.byref(p)) != 0      # zero padding: no folded form
    assert lib.sg_conv2d_tgather_plan(ctypes.byref(d), T.TG_CONV_DGRAD, 0, 4, 0, 0, None) != 0


def test_conv_transpose2d_rejects_what_torch_refuses():
    from scene_generation_amd import ops
    x, w = torch.zeros(1, 2, 3, 3), torch.zeros(2, 2, 3, 3)
    with pytest.raises(ValueError):
        ops.conv_transpose2d(x, w, None, stride=2, pad=1, out_pad=2)
    with pytest.raises(ValueError):
        ops.conv_transpose2d(x, w, None, stride=1, pad=0, out_pad=1)
    with pytest.raises(ValueError):
        ops.conv_transpose2d(torch.zeros(1, 2, 1, 1), w, None, stride=1, pad=2, out_pad=0)
    with pytest.raises(RuntimeError):
        F.conv_transpose2d(x, w, None, stride=2, padding=1, output_padding=2)
