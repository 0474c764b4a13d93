"""The case table of tests/forward_conv_cases.py, checked without a GPU: the float64 restatements agree with torch (F.conv2d on
float64 after F.interpolate / F.pad / torch.cat); every one-hot probe's restatement in fp32 is the placement it claims; every row
reports the plan it claims under each of its option sets (the library's host-only query sg_conv2d_fwd_plan, which loads without a
device); the union of the rows' plan classes is a literal list; the Python restatement of the plan equals the query over a grid;
the query rejects bad arguments and the descs whose reflection would read outside the plane; the restated constants are the ones in
the sources."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import forward_conv_cases as FC
from gpu_harness import options
from scene_generation_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'scene_generation_amd', 'csrc')
RTOL = 1e-12
SHAPES = list(dict((c['shape_key'], c) for c in FC.CASES).values())


def case_plan(lib, case, opts, **over):
    """the plan the query reports for the row as tests/test_gpu_forward_conv.py launches it (aligned buffers, the row's offsets)"""
    a = dict(w_mod16=4 * case['w_off'], y_mod16=4 * case['y_off'], ws_mod16=4 * case['ws_off'], ws_bytes=FC.case_ws_bytes(case))
    a.update(over)
    with options(opts):
        return FC.fwd_plan(lib, FC.case_desc(case), FC.ENTRY_OF[case['entry']], case['L'], **a)


# =============================================================================================
# the references
# =============================================================================================
def _torch_pre(case, inp):
    """the pre-activation by torch in float64: interpolate, pad, cat, conv2d -- image by image with that image's weights"""
    x = torch.from_numpy(inp['x1'].astype(np.float64))
    if inp['x2'] is not None:
        x2 = torch.from_numpy(inp['x2'].astype(np.float64))
        if case['bcast']:
            x2 = x2[:, :, None, None].expand(-1, -1, case['H'], case['W'])
        x = torch.cat([x, x2], dim=1)
    if case['ups'] == 2:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    if case['pad']:
        x = F.pad(x, (case['pad'],) * 4, mode='reflect' if case['reflect'] else 'constant')
    wi = torch.from_numpy(FC.image_weights(case, inp))
    b = None if inp['b'] is None else torch.from_numpy(inp['b'].astype(np.float64))
    out = [F.conv2d(x[n:n + 1], wi[n if wi.shape[0] > 1 else 0], b, stride=case['stride']) for n in range(case['N'])]
    return torch.cat(out).numpy()


@pytest.mark.parametrize('case', SHAPES, ids=lambda c: c['name'])
def test_restatement_agrees_with_torch(case):
    inp = FC.case_inputs(case)
    ref = FC.case_refs(case)
    want = _torch_pre(case, inp)
    assert ref['pre'].shape == want.shape == (case['N'], case['Cout'], case['OH'], case['OW'])
    scale = max(1.0, float(np.abs(want).max()))
    assert float(np.abs(ref['pre'] - want).max()) <= RTOL * scale
    assert (ref['sabs'] >= np.abs(ref['pre']) * (1 - 1e-12)).all()
    if case['entry'] != 'dense':               # an image that lists nothing: act(bias) exactly
        b = np.zeros(case['Cout']) if inp['b'] is None else inp['b'].astype(np.float64)
        for n in np.nonzero(inp['cnt'] == 0)[0]:
            assert np.array_equal(ref['pre'][n], np.broadcast_to(b[:, None, None], ref['pre'][n].shape))


@pytest.mark.parametrize('case', [c for c in FC.CASES if c['signed']], ids=lambda c: c['name'])
def test_no_preactivation_of_a_relu_row_lies_within_its_bound_of_zero(case):
    lib = _hip.lib()
    ref = FC.case_refs(case)
    for o in FC.case_option_sets(case):
        b = FC.pre_bound(case, case_plan(lib, case, o))
        structural = (ref['pre'] == 0) & (ref['sabs'] == 0)          # no term at all: 0 exactly on both sides, any slope
        assert ((np.abs(ref['pre']) > 4 * b) | structural).all()
        assert (ref['pre'] > 0).any() and (ref['pre'] < 0).any(), 'both branches of the activation'


@pytest.mark.parametrize('case', FC.PROBES, ids=lambda c: c['name'])
def test_probe_restatement_is_the_placement_it_claims(case):
    inp = FC.probe_inputs(case)
    got, want = FC.probe_restated(case, inp), FC.probe_placement(case, inp)
    assert np.array_equal(got, want)
    # (a list probe has an empty image, and the sparse one selects channels most images do not list)
    assert np.count_nonzero(want) > want.size // (8 if case['entry'] == 'dense' else 16), 'a probe that places next to nothing'
    taps = {(kh, kw) for (_, kh, kw) in FC.probe_selection(case)}
    assert len(taps) == case['KS'] ** 2, 'every tap selected by some output channel'


def test_probes_cover_every_loader_and_geometry():
    lib = _hip.lib()
    seen = set()
    for c in FC.PROBES:
        p = case_plan(lib, c, c['opts'])
        assert p is not None, (c['name'], lib.sg_last_error_string().decode())
        for k, v in c['claims'].items():
            assert p[k] == v, (c['name'], k, p)
        kind = 'fixed' if p['loader'] == FC.FW_FIXED else ('nomask' if p['nomask'] else 'table')
        seen |= {('loader', kind, c['entry'] != 'dense'), ('ks', c['KS']), ('stride', c['stride']), ('pad', 'reflect' if c['reflect'] else 'zero'),
                 ('ups', c['ups'])}
    want = {('loader', 'table', False), ('loader', 'fixed', False), ('loader', 'nomask', False), ('loader', 'table', True), ('loader', 'nomask', True),
            ('ups', 1), ('ups', 2), ('stride', 1), ('stride', 2), ('pad', 'reflect'), ('pad', 'zero')} | {('ks', k) for k in (1, 3, 4, 7)}
    assert seen == want, (sorted(want - seen), sorted(seen - want))


@pytest.mark.parametrize('case', [c for c in FC.CASES if c['entry'] != 'dense'], ids=lambda c: c['name'])
def test_channel_lists_hold_what_the_table_says(case):
    lists, cnt = FC.case_lists(case)
    C = case['C1'] + case['C2']
    for b in range(case['N']):
        ch = [int(c) for c in lists[b][:cnt[b]]]
        assert len(set(ch)) == len(ch) and all(0 <= c < C for c in ch)
    assert cnt[0] == case['L'] and cnt[1] == 0 and 0 < cnt[2] < case['L']
    assert any([int(c) for c in lists[b][:cnt[b]]] != sorted(int(c) for c in lists[b][:cnt[b]]) for b in range(case['N'])) or case['N'] < 4
    if case['C2']:
        assert all(max(int(c) for c in lists[b][:cnt[b]]) >= case['C1'] for b in range(case['N']) if cnt[b])


# =============================================================================================
# the plans
# =============================================================================================
def test_every_row_reports_the_plan_it_claims():
    lib = _hip.lib()
    for c in FC.CASES:
        assert c['claims'] and c['tags'] and c['why'], c['name']
        for o in FC.case_option_sets(c):
            got = case_plan(lib, c, o)
            assert got is not None, (c['name'], lib.sg_last_error_string().decode())
            for k, v in c['claims'].items():
                assert got[k] == v, '%s %s: plan field %s is %s, the table claims %s (%s)' % (c['name'], o, k, got[k], v, got)
            assert got == FC.case_py_plan(c, o), (c['name'], got, FC.case_py_plan(c, o))
            assert got['ws_needed'] <= FC.case_ws_bytes(c)
            have = FC.plan_classes(c, got, o)
            assert set(c['tags']) <= have, '%s %s: claims %s, reaches %s' % (c['name'], o, sorted(set(c['tags']) - have, key=str), sorted(have, key=str))


# the plan classes the table must reach (the issue's list, written out); tags a row reaches without claiming them do not count
REQUIRED = set(FC.KERNEL_CLASSES) | {
    ('scalar', 'w_off', 64, 64), ('scalar', 'w_off', 32, 128), ('scalar', 'w_off', 64, 128),
    ('scalar', 'k4', 64, 64), ('scalar', 'k4', 32, 128), ('scalar', 'k4', 64, 128),
    ('downgrade',),
    ('natural_tile', 128, 128), ('natural_tile', 64, 64), ('natural_tile', 32, 128), ('natural_tile', 64, 128),
    ('src', 'bcast', 'mask'), ('src', 'bcast', 'nomask'),
    ('fixed', 4), ('fixed', 1), ('fixed_off', 'k16'), ('fixed_off', 'two'), ('fixed_off', 'option'),
    ('nomask_off', 'pixel'), ('nomask_off', 'm'), ('nomask_off', 'k16'), ('nomask_off', 'zero'), ('nomask_off', 'scalar'),
    ('splits', 'vec'), ('scalar_reduce', 'y'), ('scalar_reduce', 'phw'), ('scalar_reduce', 'odd'), ('scalar_reduce', 'ws'),
    ('forced_clipped',), ('split_dropped',), ('split+fixed',), ('split+nomask',), ('natural_split', 'fixed'), ('natural_split', 'nomask'),
    ('ks', 7, 'mask'), ('ks', 7, 'nomask'), ('ks', 1, 'nomask'), ('ks', 4, 'nomask'), ('stride', 2, 'nomask'),
    ('zero_pad', 'p0'), ('zero_pad', 'big'),
    ('reflect_pad', 1, 'mask'), ('reflect_pad', 3, 'mask'), ('reflect_pad', 3, 'nomask'), ('reflect_pad', 'H-1'),
    ('ups', 'zero'), ('ups', 'reflect'), ('ups', 'stride2'),
    ('plane', 'nonsquare', 'mask'), ('plane', 'nonsquare', 'nomask'), ('plane', 'odd'), ('plane', '1x1'),
    ('straddle', 'mask'), ('straddle', 'nomask'),
    ('cout', 1), ('cout', 33), ('c1', 1), ('c2', 1),
    ('bias', 0, 'full'), ('bias', 1, 'full'), ('bias', 0, 'edge'), ('bias', 1, 'edge'),
    ('ep', FC.ACT_NONE, 'full'), ('ep', FC.ACT_RELU, 'full'), ('ep', FC.ACT_LEAKY, 'full'), ('ep', FC.ACT_TANH, 'full'),
    ('ep', FC.ACT_NONE, 'edge'), ('ep', FC.ACT_RELU, 'edge'), ('ep', FC.ACT_LEAKY, 'edge'), ('ep', FC.ACT_TANH, 'edge'),
    ('ep', FC.ACT_LEAKY, 'reduce'),
    ('list_tile', 128, 128), ('list_tile', 64, 64), ('list_tile', 32, 128), ('list_tile', 64, 128),
    ('list_nomask', 0), ('list_nomask', 1), ('list_ragged_k',), ('list_ragged_nomask',),
    ('list_second', 'plain'), ('list_second', 'bcast'), ('list_geom', 'k3s2'), ('list_geom', 'k4s2'), ('list_geom', 'k7r'),
    ('perimage_nobias',), ('tail_split_row',),
}
# classes every row of a kind reaches anyway (so no row is there FOR them): reached, checked below, not claimed
IMPLIED = {('splits', 'one'), ('ks', 1, 'mask'), ('ks', 3, 'mask'), ('ks', 3, 'nomask'), ('ks', 4, 'mask'), ('stride', 1, 'mask'), ('stride', 1, 'nomask'),
           ('stride', 2, 'mask'), ('zero_pad', 'p1'), ('reflect_pad', 1, 'nomask'), ('src', 'one', 'mask'), ('src', 'one', 'nomask'),
           ('src', 'two', 'mask'), ('src', 'two', 'nomask'), ('splits', 'scalar'), ('list_unequal',), ('list_empty_image',), ('list_full_image',)}


def test_the_table_claims_exactly_the_required_plan_classes():
    lib = _hip.lib()
    claimed, reached = set(), set()
    for c in FC.CASES:
        claimed |= set(c['tags'])
        for o in FC.case_option_sets(c):
            reached |= FC.plan_classes(c, case_plan(lib, c, o), o)
    assert claimed == REQUIRED, ('missing', sorted(REQUIRED - claimed, key=str), 'unclaimed by the list', sorted(claimed - REQUIRED, key=str))
    assert IMPLIED <= reached, sorted(IMPLIED - reached, key=str)
    lists = [c for c in FC.CASES if c['entry'] != 'dense']
    for c in lists:                      # every list row: unequal lists, an empty image, a full one
        assert {('list_unequal',), ('list_empty_image',), ('list_full_image',)} <= FC.plan_classes(c, case_plan(lib, c, c['opts']), c['opts'])
    assert {c['entry'] for c in lists} == {'sparse', 'perimage'}
    # at least two rows split by kn_splits itself, and the size limits of the table
    assert sum(1 for c in FC.CASES if 'splits' not in c['opts'] and case_plan(lib, c, c['opts'])['splits'] > 1) >= 2
    for c in FC.CASES:
        C = c['C1'] + c['C2']
        assert max(c['Cout'], C) <= 256 and c['N'] * c['OH'] * c['OW'] <= 8192, c['name']
        assert max(c['N'] * C * c['H'] * c['W'], c['Cout'] * C * c['KS'] ** 2, c['N'] * c['Cout'] * c['OH'] * c['OW']) <= 1 << 20, c['name']
    # only the tail-split row launches more tiles than the chip has CUs (joins(): c = tail_smax there, 0 on every other unsplit row)
    big = [c['name'] for c in FC.CASES if c['entry'] == 'dense' and FC.tiles_of(c, case_plan(lib, c, FC.case_option_sets(c)[0])) > FC.N_CU]
    assert big == ['tail_split_300_tiles']
    c = FC.BY_NAME['tail_split_300_tiles']
    p = case_plan(lib, c, {})
    tiles = FC.tiles_of(c, p)
    assert (p['bm'], p['bn']) == (64, 64) and FC.N_CU < tiles and tiles % FC.N_CU and p['K'] // FC.BK >= 16 and p['K'] >= 288
    assert [o.get('w43_tail_split') for o in FC.case_option_sets(c)] == [2, 0]


GRID_GEOM = (  # (KS, stride, pad, reflect, ups)
    (1, 1, 0, 0, 1), (1, 1, 0, 1, 1), (1, 2, 0, 0, 1), (3, 1, 1, 0, 1), (3, 1, 1, 1, 1), (3, 2, 1, 0, 1), (3, 1, 0, 0, 1), (3, 1, 3, 0, 1), (3, 1, 1, 1, 2),
    (3, 1, 1, 0, 2), (4, 2, 1, 0, 1), (4, 2, 1, 1, 1), (4, 2, 2, 0, 1), (4, 1, 2, 0, 1), (4, 2, 1, 0, 2), (7, 1, 3, 1, 1), (7, 1, 3, 0, 1), (7, 2, 3, 0, 1))
GRID_C = ((1, 0, 0), (3, 0, 0), (4, 0, 0), (16, 0, 0), (128, 0, 0), (7, 1, 0), (12, 4, 1))
GRID_M = (1, 32, 33, 64, 128, 130)
GRID_PLANES = ((1, 8, 8), (2, 8, 8), (1, 7, 9), (3, 5, 5), (2, 16, 16), (1, 32, 48), (5, 1, 1))          # (N, H, W) stored
GRID_OPTS = ({}, {'tile': 0}, {'tile': 3}, {'t128_min': 1}, {'t128_min': 4}, {'tile3': 0}, {'tile3': 2}, {'tile3_min': 1}, {'tile3_min': 8},
             {'split_target': 64}, {'split_target': 4096}, {'split_kmin': 64}, {'split_kmin': 256}, {'splits': 2}, {'splits': 16}, {'fixedtap': 0},
             {'fixedtap': 2}, {'split_kmin': 32, 'split_target': 256, 't128_min': 1})
GRID_ALIGN = ((0, 0, 0), (4, 0, 0), (0, 8, 0), (0, 0, 12))          # (w, y, ws) mod 16


def test_python_plan_equals_the_query_over_a_grid():
    lib = _hip.lib()
    n = refused = i = 0
    for o in GRID_OPTS:
        with options(o):
            for (KS, s, p, reflect, ups), (C1, C2, bc), M, (N, H, W) in itertools.product(GRID_GEOM, GRID_C, GRID_M, GRID_PLANES):
                # the full product is 95 256 shapes x option sets, each queried ~50 ways: every 29th (coprime with every axis length,
                # so each value of each axis meets each value of the others)
                i += 1
                if i % 29:
                    continue
                OH, OW = FC.conv_out_size(H * ups, KS, s, p), FC.conv_out_size(W * ups, KS, s, p)
                if OH < 1 or OW < 1:
                    continue
                d = FC.make_desc(N, C1, H, W, M, KS, s, p, reflect, ups, OH, OW, C2=C2)
                d.x2_broadcast = bc
                K = (C1 + C2) * KS * KS
                slab = M * N * OH * OW * 4
                sizes = (FC.AMPLE * 8, FC.ktab_bytes(K), FC.ktab_bytes(K) + 2 * slab + 4, FC.ktab_bytes(K) - 8)
                for (wm, ym, sm), ws in itertools.product(GRID_ALIGN, sizes):
                    got = FC.fwd_plan(lib, d, FC.FW_CONV, 0, wm, ym, sm, ws)
                    want = FC.py_plan(FC.FW_CONV, N, C1, C2, H, W, M, KS, s, p, reflect, ups, OH, OW, bcast=bc, w_mod16=wm, y_mod16=ym, ws_mod16=sm,
                                      ws_bytes=ws, **o)
                    assert got == want, (o, KS, s, p, reflect, ups, C1, C2, bc, M, N, H, W, wm, ym, sm, ws, got, want)
                    n += 1
                    refused += got is None
                C = C1 + C2
                for entry, L in itertools.product((FC.FW_SPARSE, FC.FW_PERIMAGE), sorted({1, min(5, C), C, C + 1, 0})):
                    need = FC.sparse_fwd_ws(N, M, max(L, 1), KS * KS)
                    if 0 < L <= C:
                        assert need == lib.sg_conv2d_sparse_ws_bytes(ctypes.byref(d), L, 0)
                    for sm, ws in ((0, FC.AMPLE * 8), (0, need), (0, need - 4), (4, FC.AMPLE * 8)):
                        got = FC.fwd_plan(lib, d, entry, L, 0, 0, sm, ws)
                        want = FC.py_plan(entry, N, C1, C2, H, W, M, KS, s, p, reflect, ups, OH, OW, bcast=bc, L=L, ws_mod16=sm, ws_bytes=ws, **o)
                        assert got == want, (o, entry, L, KS, s, p, reflect, ups, C1, C2, M, N, H, W, sm, ws, got, want)
                        n += 1
                        refused += got is None
    print('%d plans compared (%d of them refusals)' % (n, refused))
    assert n - refused >= 50000 and refused >= 10000


def test_query_rejects_bad_arguments_and_unreadable_reflections():
    lib = _hip.lib()
    p = FC.sgFwdPlan()
    err = lambda: lib.sg_last_error_string()

    def q(d, e=FC.FW_CONV, L=0, w=0, y=0, s=0, ws=FC.AMPLE, plan=p):
        return lib.sg_conv2d_fwd_plan(None if d is None else ctypes.byref(d), e, L, w, y, s, ws, None if plan is None else ctypes.byref(plan))
    d = FC.make_desc(1, 4, 5, 5, 4, 3, 1, 1, False, 1, 5, 5)
    assert q(d) == 0 and q(d, FC.FW_SPARSE, L=2) == 0 and q(d, FC.FW_PERIMAGE, L=4) == 0
    assert q(None) != 0 and b'bad arguments' in err()
    assert q(d, plan=None) != 0
    assert q(d, -1) != 0 and q(d, 3) != 0
    for bad in (dict(w=2), dict(y=16), dict(s=-4), dict(w=1)):
        assert q(d, **bad) != 0 and b'mod16' in err()
    assert q(d, FC.FW_SPARSE, L=0) != 0 and q(d, FC.FW_PERIMAGE, L=5) != 0 and b'L=5' in err()
    assert q(d, ws=FC.ktab_bytes(36) - 1) != 0 and b'workspace too small' in err()
    assert q(d, ws=FC.ktab_bytes(36)) == 0
    need = FC.sparse_fwd_ws(1, 4, 2, 9)
    assert q(d, FC.FW_SPARSE, L=2, ws=need) == 0 and q(d, FC.FW_SPARSE, L=2, ws=need - 1) != 0 and b'workspace too small' in err()
    for e in (FC.FW_SPARSE, FC.FW_PERIMAGE):
        for s in (4, 8, 12):
            assert q(d, e, L=2, s=s) != 0 and b'16-byte aligned' in err()
    assert q(d, s=4) == 0                      # the dense entry takes any workspace alignment (it picks the scalar reduce)
    assert q(FC.make_desc(1, 4, 5, 5, 4, 5, 1, 1, False, 1, 5, 5)) != 0 and b'kernel size' in err()
    # reflection that would mirror twice, or an output grid beyond the padded plane: refused (torch refuses the same pads)
    ok = FC.make_desc(1, 4, 8, 4, 4, 7, 1, 3, True, 1, 8, 4)
    assert q(ok) == 0
    for bad in (FC.make_desc(1, 4, 8, 3, 4, 7, 1, 3, True, 1, 8, 3),          # pad 3 on a 3-wide plane: tap column 5 mirrors to -1
                FC.make_desc(1, 4, 3, 8, 4, 7, 1, 3, True, 1, 3, 8),          # ... on a 3-high plane
                FC.make_desc(1, 4, 2, 1, 4, 7, 1, 3, True, 2, 4, 2),          # upsampled 4 x 2 plane
                FC.make_desc(1, 4, 8, 8, 4, 3, 1, -1, True, 1, 6, 6)):
        for e, L in ((FC.FW_CONV, 0), (FC.FW_SPARSE, 2), (FC.FW_PERIMAGE, 2)):
            assert q(bad, e, L=L) != 0 and b'reflect pad' in err(), (bad.H, bad.W)
    for bad in (FC.make_desc(1, 4, 8, 8, 4, 3, 1, 1, True, 1, 9, 8), FC.make_desc(1, 4, 8, 8, 4, 3, 1, 1, True, 1, 8, 9),
                FC.make_desc(1, 4, 8, 8, 4, 4, 2, 1, True, 1, 5, 4), FC.make_desc(1, 4, 4, 4, 4, 3, 1, 1, True, 2, 9, 8)):
        for e, L in ((FC.FW_CONV, 0), (FC.FW_SPARSE, 2), (FC.FW_PERIMAGE, 2)):
            assert q(bad, e, L=L) != 0 and b'beyond the reflect-padded' in err(), (bad.OH, bad.OW)
    # the same descs under zero padding are fine: the taps outside are zeros
    assert q(FC.make_desc(1, 4, 8, 3, 4, 7, 1, 3, False, 1, 8, 3)) == 0 and q(FC.make_desc(1, 4, 8, 8, 4, 3, 1, 1, False, 1, 9, 8)) == 0


ENTRY_POINTS = ('sg_conv2d_fwd', 'sg_conv2d_dgrad', 'sg_conv2d_dgrad_folded', 'sg_conv2d_wgrad', 'sg_conv2d_fwd_sparse', 'sg_conv2d_wgrad_sparse',
                'sg_conv2d_fwd_perimage', 'sg_conv2d_wgrad_perimage')


def test_every_conv_entry_point_refuses_the_unreadable_reflections():
    """return codes only: the desc check comes before any pointer is looked at, so null pointers are enough and nothing can launch"""
    lib = _hip.lib()
    n = None
    args = {'sg_conv2d_fwd': (n, n, n, n, n, 0, 0.0, n, 0, n), 'sg_conv2d_dgrad': (n, n, n, 0, 4, n, 0, n), 'sg_conv2d_dgrad_folded': (n, n, n, 0, 4, n, 0, n),
            'sg_conv2d_wgrad': (n, n, n, n, n, n, 0, n), 'sg_conv2d_fwd_sparse': (n, n, n, n, n, n, 2, n, 0, 0.0, n, 0, n),
            'sg_conv2d_wgrad_sparse': (n, n, n, n, n, 2, n, n, n, 0, n), 'sg_conv2d_fwd_perimage': (n, n, n, n, n, n, 2, n, 0, 0.0, n, 0, n),
            'sg_conv2d_wgrad_perimage': (n, n, n, n, n, 2, n, n, 0, n)}
    assert set(args) == set(ENTRY_POINTS)
    for bad, msg in ((FC.make_desc(1, 4, 8, 3, 4, 7, 1, 3, True, 1, 8, 3), b'reflect pad'),
                     (FC.make_desc(1, 4, 8, 8, 4, 3, 1, 1, True, 1, 9, 8), b'beyond the reflect-padded')):
        for name in ENTRY_POINTS:
            assert getattr(lib, name)(ctypes.byref(bad), *args[name]) != 0, name
            assert msg in lib.sg_last_error_string() and name.encode() in lib.sg_last_error_string(), (name, lib.sg_last_error_string())


# =============================================================================================
# constants against the sources
# =============================================================================================
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_restated_constants_match_the_sources():
    core, kn0, ig, rt = _src('igemm_core.h'), _src('igemm_kn0.hip'), _src('igemm.hip'), _src('runtime.hip')
    assert int(re.search(r'constexpr int BK = (\d+);', core).group(1)) == FC.BK
    assert re.search(r'#define SG_NSUB 1\b', core)                    # the k-tile depth of the gather tiles = BK
    assert 'inline size_t ktab_bytes(int K) { return (size_t)(sg_cdiv(K, %d) * %d + %d) * sizeof(KEntry); }' % (
        FC.KTAB_ROUND, FC.KTAB_ROUND, FC.KTAB_EXTRA) in core
    assert 'struct KEntry { unsigned choff; unsigned tapsel; };' in core and FC.KENTRY_BYTES == 8
    assert 'inline int sparse_kpad(int L, int KS2) { return sg_cdiv(sparse_kc(L, KS2), %d) * %d + %d; }' % (FC.KTAB_ROUND, FC.KTAB_ROUND, FC.KTAB_EXTRA) in core
    assert '(size_t)M * sparse_kc(L, KS2) * sizeof(float) + %d);' % FC.SPARSE_SLACK in core
    assert 'const int target = pick_tile(M, Npix) == 0 ? %d : sg_opt(SG_OPT_SPLIT_TARGET);' % FC.SPLIT_TARGET_128 in core
    assert 'if (sp > %d) sp = %d;' % (FC.SPLIT_MAX, FC.SPLIT_MAX) in core
    for text in ('if (M <= 32) return 2;', 'sg_cdiv(M, 128) * 128 * 20 <= M * 23 && N >= 512', 'const long over = t128 % 512;',
                 't128 > 512 && t128 < 1536 && over > 0 && over < 128', 'if (M >= 96 && low_waste && !ragged128 && (M >= 512 || t128 >= t128_min)) return 0;',
                 'if (tiles * 4 >= target * 3 || K < kmin) return 1;', 'int sp = (target + tiles / 2) / tiles;', 'if (sp > K / (kmin / 2)) sp = K / (kmin / 2);'):
        assert text in core, text
    defaults = dict((k, int(v)) for k, v in re.findall(r'\{"(\w+)", (-?\d+)\}', rt))
    for k, v in list(FC.OPTION_DEFAULTS.items()) + list(FC.TAIL_DEFAULTS.items()):
        assert defaults[k] == v, k
    # ONE function holds each decision: the launcher and the query call it, nobody restates it
    assert core.count('kn_sparse_plan(') == 1 and kn0.count('kn_sparse_plan(') == 1 and ig.count('kn_sparse_plan(') == 1
    body = kn0[kn0.index('int run_kn_sparse('):kn0.index('int sgk::kn0_run(')]
    assert 'pick_tile(' not in body and 'sg_opt(' not in body
    body = core[core.index('int run_kn(const float* A'):core.index('int run_kn_ks(')]
    assert 'pl.reduce == SG_FR_VEC' in body and 'aligned16(slabs)' not in body and 'sg_opt(' not in body and body.count('kn_plan(') == 1
    # launch modifiers are an argument (LaunchMods, variant_stride): the thread-locals that carried them are gone from every source
    gone = re.compile(r'\b(t_batch|t_grid_z|t_fixed_kchunk|t_xcd_z|t_min_z|t_variant_stride)\b')
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.h', '.hip', '.sh')):
            assert not gone.search(_src(name)), name
    assert ig.count('check_fwd_args(') == 5          # its definition, the three entry points, the query
    text = open(os.path.join(ROOT, 'include', 'sg2im_hip.h')).read()
    vals = dict((k, int(v)) for k, v in re.findall(r'(SG_F[WR]_\w+)\s*=\s*(\d+)', text))
    assert [vals[k] for k in ('SG_FW_CONV', 'SG_FW_SPARSE', 'SG_FW_PERIMAGE')] == [FC.FW_CONV, FC.FW_SPARSE, FC.FW_PERIMAGE]
    assert [vals[k] for k in ('SG_FW_TABLE', 'SG_FW_FIXED')] == [FC.FW_TABLE, FC.FW_FIXED]
    assert [vals[k] for k in ('SG_FR_NONE', 'SG_FR_VEC', 'SG_FR_SCALAR')] == [FC.FR_NONE, FC.FR_VEC, FC.FR_SCALAR]
    body = re.search(r'typedef struct sgFwdPlan \{(.*?)\} sgFwdPlan;', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S), re.S).group(1)
    assert tuple(re.findall(r'(\w+)\s*[,;]', body)) == FC.PLAN_FIELDS + ('ws_needed',) and 'int64_t ws_needed;' in body
    assert ctypes.sizeof(FC.sgFwdPlan) == 4 * len(FC.PLAN_FIELDS) + 8
