"""The case table of tests/head_smallm_cases.py, checked without a GPU: the float64 restatements of the five operations agree with
torch (F.conv2d and autograd on float64) and satisfy the adjoint identity; every probe's restatement in fp32 is the placement it
claims; every row reports the plans it claims (the library's host-only queries sg_conv2d_head_plan / sg_conv2d_smallm_plan, which
load without a device) and the rows reach every plan class of a literal list; the Python restatement of the predicates, the
workspace sizes and both plans equals the library over a sweep around every threshold; every entry point refuses what the
predicates refuse, null pointers, a short workspace and -- small-M -- a result or gradient that is not 16-byte aligned, on the host,
naming itself; the restated constants are the ones in the source."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_smallm_cases as HS
from gpu_harness import dref
from scene_generation_amd import _hip, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'scene_generation_amd', 'csrc', 'smallm.hip')
RTOL = 1e-12
SHAPES = list(dict((c['shape_key'], c) for c in HS.CASES).values())


def err(lib):
    return lib.sg_last_error_string().decode()


# =============================================================================================
# the references
# =============================================================================================
def _torch_all(case, inp):
    """pre-activation, gx and gw by torch in float64 (pad, conv2d, autograd of <pre, gy>)"""
    x = torch.from_numpy(inp['x'].astype(np.float64)).requires_grad_()
    w = torch.from_numpy(inp['w'].astype(np.float64)).requires_grad_()
    b = None if inp['b'] is None else torch.from_numpy(inp['b'].astype(np.float64))
    xp = F.pad(x, (case['pad'],) * 4, mode='reflect' if case['reflect'] else 'constant') if case['pad'] else x
    pre = F.conv2d(xp, w, b)
    gx, gw = torch.autograd.grad(pre, (x, w), torch.from_numpy(inp['gy'].astype(np.float64)))
    return pre.detach().numpy(), gx.numpy(), gw.numpy()


def _close(a, b):
    assert a.shape == b.shape
    assert float(np.abs(a - b).max()) <= RTOL * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize('case', SHAPES, ids=lambda c: c['name'])
def test_restatements_agree_with_torch_and_are_adjoint(case):
    inp, ref = HS.case_inputs(case), HS.case_refs(case)
    pre, gx, gw = _torch_all(case, inp)
    assert ref['pre'].shape == (case['N'], case['Cout'], case['OH'], case['OW'])
    _close(ref['pre'], pre)
    _close(ref['gw'], gw)
    assert (ref['y_sabs'] >= np.abs(ref['pre']) * (1 - 1e-12)).all() and (ref['gw_sabs'] >= np.abs(ref['gw']) * (1 - 1e-12)).all()
    x, w, gy = (inp[n].astype(np.float64) for n in ('x', 'w', 'gy'))
    lin = HS.restate_fwd(case, x, w)                       # (without the bias: the bilinear part)
    ip = float((lin * gy).sum())
    scale = float((ref['y_sabs'] * np.abs(gy)).sum())
    assert abs(ip - float((w * ref['gw']).sum())) <= 1e-12 * scale          # <y, gy> = <w, gw>
    if case['family'] == 'head':
        _close(ref['gx'], gx)
        assert abs(ip - float((x * ref['gx']).sum())) <= 1e-12 * scale      # <y, gy> = <x, gx>
        assert (ref['gx_terms'] <= case['KS'] ** 2).all() and ref['gx_terms'].max() >= 1
        if case['pad'] == 0 and case['KS'] > 1 and case['OH'] * case['OW'] > 1:
            assert ref['gx_terms'].min() < ref['gx_terms'].max(), 'pad 0: border pixels of gx see fewer taps'
    n_full = case['N'] * case['OH'] * case['OW']
    assert (ref['gw_terms'] <= n_full).all()
    if case['reflect']:
        assert (ref['gw_terms'] == n_full).all()


@pytest.mark.parametrize('case', [c for c in HS.CASES if c['signed']], ids=lambda c: c['name'])
def test_no_preactivation_of_a_relu_row_lies_within_its_bound_of_zero(case):
    ref = HS.case_refs(case)
    b = HS.y_bound(case, HS.case_py_plan(case, 'fwd'))
    structural = (ref['pre'] == 0) & (ref['y_sabs'] == 0)
    assert ((np.abs(ref['pre']) > 4 * b) | structural).all()
    if case['Cout'] > 1:
        assert (ref['pre'] > 0).any() and (ref['pre'] < 0).any(), 'both branches of the activation'


@pytest.mark.parametrize('case', HS.PROBES, ids=lambda c: c['name'])
def test_probe_restatement_is_the_placement_it_claims(case):
    x, gy = HS.case_inputs(case)['x'], HS.case_inputs(case)['gy']
    taps = HS.probe_taps(case)
    assert {(kh, kw) for _, kh, kw in taps} == set(itertools.product(range(case['KS']), repeat=2))
    M = case['Cout']
    for i in range(0, len(taps), M):
        sel = (taps[i:i + M] + taps[:M])[:M]
        w = np.zeros((M, case['C1'], case['KS'], case['KS']), dtype=np.float32)
        for m, (c, kh, kw) in enumerate(sel):
            w[m, c, kh, kw] = 1.0
        got = HS.restate_fwd(case, x, w)
        assert got.dtype == np.float32 and np.array_equal(got, HS.place_fwd(case, x, sel))
        if case['family'] == 'head':
            assert np.array_equal(HS.restate_dgrad(case, gy, w), HS.place_dgrad(case, gy, *sel[0]))
    for site in HS.probe_sites(case):
        g1 = np.zeros_like(gy)
        g1[site[0], site[1], site[2][0], site[2][1]] = 1.0
        assert np.array_equal(HS.restate_wgrad(case, g1, x), HS.place_wgrad(case, x, site))
    assert case['H'] != case['W'] and case['OH'] != case['OW'], 'non-square, so that an H / W swap cannot cancel'


# =============================================================================================
# the table and the plans
# =============================================================================================
def test_table_is_self_consistent():
    for c in HS.CASES + HS.PROBES:
        assert (HS.smallm_supported(c), HS.head_supported(c)) == ((True, False) if c['family'] == 'smallm' else (False, True)), c['name']
        for n in ('x', 'w', 'gy'):
            assert HS.case_inputs(c)[n].size <= 400000, (c['name'], n)
        assert set(c['claims']) <= set(HS.case_entries(c)), c['name']
        assert c['why'] or c in HS.PROBES, c['name']
    assert all(n in HS.BY_NAME for n in HS.OPERATOR_ROWS)
    assert any(c['H'] != c['W'] for c in HS.HEAD_CASES if c['KS'] == 3) and any(c['H'] != c['W'] for c in HS.HEAD_CASES if c['KS'] == 4)


@pytest.mark.parametrize('case', HS.CASES + HS.PROBES, ids=lambda c: c['name'])
def test_row_has_the_plans_it_claims(case):
    lib = _hip.lib()
    d = HS.desc_of(case)
    for entry in HS.case_entries(case):
        got = HS.case_lib_plan(lib, case, entry)
        assert got is not None, err(lib)
        assert got == HS.case_py_plan(case, entry), (case['name'], entry)
        for k, v in case['claims'].get(entry, {}).items():
            assert got[k] == v, '%s %s: plan field %s is %s, the table claims %s (%s)' % (case['name'], entry, k, got[k], v, got)
    pred, wsq = ('sg_conv2d_smallm_supported', 'sg_conv2d_smallm_ws_bytes') if case['family'] == 'smallm' else ('sg_conv2d_head_supported', 'sg_conv2d_head_ws_bytes')
    assert getattr(lib, pred)(dref(d)) == 1 and getattr(lib, wsq)(dref(d)) == HS.case_ws_bytes(case) > 0
    if case['family'] == 'head':           # the ops wrapper is the same query; the stream kernel needs both addresses aligned
        assert ops.conv2d_head_plan(d, ops.HEAD_FWD, 4 * case['x_off'], 4 * case['y_off']) == HS.case_py_plan(case, 'fwd')
        if HS.case_py_plan(case, 'fwd', 0, 0)['kind'] == HS.HEAD_STREAM:
            for xm, ym in ((4, 0), (0, 4), (8, 8), (12, 0)):
                assert HS.head_plan(lib, d, HS.HEAD_FWD, xm, ym)['kind'] == HS.HEAD_STAGED
        for e in (HS.HEAD_DGRAD, HS.HEAD_WGRAD):      # the addresses matter to the forward only
            assert HS.head_plan(lib, d, e, 4, 8) == HS.head_plan(lib, d, e, 0, 0)
    else:
        assert ops.conv2d_smallm_plan(d, ops.SMALLM_WGRAD) == HS.case_py_plan(case, 'wgrad')


def test_table_reaches_every_plan_class():
    """the classes come from the plans the library reports (the same host query the device module asks)"""
    lib = _hip.lib()
    seen = set()
    for c in HS.CASES:
        seen |= HS.plan_classes(c, {e: HS.case_lib_plan(lib, c, e) for e in HS.case_entries(c)})
    missing = [k for k in HS.REQUIRED_CLASSES if k not in seen]
    assert not missing, missing


def _lib_answers(lib, f):
    d = HS.desc_of(f)
    return (lib.sg_conv2d_head_supported(dref(d)), lib.sg_conv2d_head_ws_bytes(dref(d)), lib.sg_conv2d_smallm_supported(dref(d)),
            lib.sg_conv2d_smallm_ws_bytes(dref(d)),
            tuple(HS.head_plan(lib, d, e, xm, 0) for e in (HS.HEAD_FWD, HS.HEAD_DGRAD, HS.HEAD_WGRAD) for xm in (0, 4)),
            tuple(HS.smallm_plan(lib, d, e) for e in (HS.SMALLM_FWD, HS.SMALLM_WGRAD)))


def _py_answers(f):
    return (int(HS.head_supported(f)), HS.head_ws_bytes(f), int(HS.smallm_supported(f)), HS.smallm_ws_bytes(f),
            tuple(HS.py_head_plan(f, e, xm, 0) for e in (HS.HEAD_FWD, HS.HEAD_DGRAD, HS.HEAD_WGRAD) for xm in (0, 4)),
            tuple(HS.py_smallm_plan(f, e) for e in (HS.SMALLM_FWD, HS.SMALLM_WGRAD)))


@pytest.mark.parametrize('name,f,supported', HS.HEAD_EDGES + HS.SMALLM_EDGES, ids=[e[0] for e in HS.HEAD_EDGES + HS.SMALLM_EDGES])
def test_both_sides_of_every_inequality(name, f, supported):
    lib = _hip.lib()
    head = (name, f, supported) in HS.HEAD_EDGES
    assert (HS.head_supported(f) if head else HS.smallm_supported(f)) == supported
    assert _lib_answers(lib, f) == _py_answers(f)
    a = _py_answers(f)
    assert (a[0] if head else a[2]) == int(supported) and ((a[1] if head else a[3]) > 0) == supported
    assert all((p is not None) == supported for p in (a[4] if head else a[5]))


def test_restated_predicates_and_plans_equal_the_library_over_a_sweep():
    """shapes around every threshold: the LDS budget (planes 38..51 on a side), OW 255..257, C1 15..17 and the chunkings, W % 4 and
    the small-M minimum, every kernel size and padding, the refused strides / sources / paddings"""
    lib = _hip.lib()
    n = 0
    planes = [(1, 1), (1, 4), (3, 5), (4, 4), (4, 6), (5, 8), (8, 7), (16, 64), (17, 68), (17, 132), (2, 255), (2, 256), (2, 257), (1, 257), (30, 30),
              (28, 32), (32, 36), (36, 40), (40, 40), (44, 47), (47, 47), (48, 48), (48, 50), (49, 49), (49, 50), (50, 50), (51, 51), (3, 4), (4, 3)]
    for (H, W), KS, pad, C1, Cout, reflect in itertools.product(planes, (1, 2, 3, 4, 5, 7), range(5), (1, 3, 15, 16, 17, 40), (1, 3, 5), (0, 1)):
        if H + 2 * pad < KS or W + 2 * pad < KS or (reflect and pad >= min(H, W)):
            continue
        f = HS.desc_fields(3, C1, H, W, Cout, KS, pad, reflect)
        assert _lib_answers(lib, f) == _py_answers(f), f
        n += 1
    for kw in (dict(stride=2), dict(ups=2), dict(C2=3), dict(OH=9), dict(OW=9)):
        for f in (HS.desc_fields(2, 16, 8, 8, 1, 3, 1, False, **kw), HS.desc_fields(2, 3, 8, 8, 3, 7, 3, True, **kw)):
            assert _lib_answers(lib, f) == _py_answers(f) and not HS.head_supported(f) and not HS.smallm_supported(f), f
            n += 1
    assert n > 20000


def test_the_dgrad_inequality_of_head_ok_never_decides():
    """what reading head_ok found: (OH + 2E)(OW + 2E) + 16 KS^2 <= 12288 holds wherever PP + 4 OP <= 12288 and OW <= 256 do (OP <= 2457
    bounds the extended plane by 3930 + 256 floats), so it has no refused side of its own -- over every plane the other two admit"""
    for KS, pad in ((1, 0), (1, 1), (3, 0), (3, 1), (3, 2), (3, 3), (4, 0), (4, 1), (4, 2), (4, 3), (4, 4)):
        for H in range(1, 260):
            for W in (1, 2, 3, 4, 8, 16, 32, 48, 49, 50, 64, 128, 200, 253, 254, 255, 256, 257, 258, 259, 300):
                if H + 2 * pad < KS or W + 2 * pad < KS:
                    continue
                a, b, c = HS.head_lds_conditions(HS.desc_fields(1, 16, H, W, 1, KS, pad, False))
                f = HS.desc_fields(1, 16, H, W, 1, KS, pad, False)
                if a and f['OW'] <= HS.HEAD_OW_MAX:
                    assert c, (KS, pad, H, W)


def test_restated_constants_are_the_ones_in_the_source():
    src = open(SRC).read()
    assert re.search(r'constexpr int HEAD_LDS_FLOATS = %d;' % HS.HEAD_LDS_FLOATS, src)
    assert 'ch = ch > %d ? %d : ch;' % (HS.HEAD_CH_MAX, HS.HEAD_CH_MAX) in src and 'd->OW > %d' % HS.HEAD_OW_MAX in src and 'd->C1 >= %d' % HS.HEAD_C1_MIN in src
    assert 'if (floats < %d) floats = %d;' % (HS.HEAD_WGRAD_LDS_MIN, HS.HEAD_WGRAD_LDS_MIN) in src and 'd->N <= %d' % HS.STREAM_N_MAX in src
    assert 'TH = %d, TW = %d,' % (HS.SM_TH, HS.SM_TW) in src and 'RB = %d, CB = %d,' % (HS.SM_RB, HS.SM_CB) in src
    assert '#define HEAD_WGRAD_PARTS(pairs) ((pairs) >= 128 ? 1 : ((pairs) >= 64 ? 2 : ((pairs) >= 32 ? 4 : ((pairs) >= 16 ? 8 : 16))))' in src
    assert 'const int Q = HEAD_WGRAD_PARTS(pairs);' in src and 'p.Q_last = HEAD_WGRAD_PARTS(' in src        # the kernel and the plan share it
    assert 'for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);' in src                  # C_SMALLM_LANES = 5
    assert '(red[p] + red[OP + p]) + (red[2 * OP + p] + red[3 * OP + p])' in src                    # C_HEAD_COMBINE = 2


# =============================================================================================
# refusals, on the host
# =============================================================================================
class _Host:
    """host memory standing in for device buffers: a refused call never reads it"""

    def __init__(self):
        self.buf = (ctypes.c_float * 64)()
        self.base = ctypes.addressof(self.buf)
        self.base += (-self.base) % 16

    def at(self, off_bytes=0):
        return ctypes.c_void_p(self.base + off_bytes)


def _entry_calls(case, ws_bytes, x=None, w=None, gy=None, out=None, ws=None):
    """{entry point: argument tuple behind the desc}: every pointer a distinct host address unless overridden"""
    h = _Host()
    p = dict(x=h.at(0), w=h.at(16), gy=h.at(32), out=h.at(48), ws=h.at(64), b=h.at(80))
    p.update((k, v) for k, v in dict(x=x, w=w, gy=gy, out=out, ws=ws).items() if v is not None)
    z = lambda k: None if p[k] == 'null' else p[k]
    if case['family'] == 'smallm':
        return h, {'sg_conv2d_smallm_fwd': (z('x'), z('w'), z('b'), z('out'), 0, 0.0, None),
                   'sg_conv2d_smallm_wgrad': (z('gy'), z('x'), z('out'), z('ws'), ws_bytes, None)}
    return h, {'sg_conv2d_head_fwd': (z('x'), z('w'), z('b'), z('out'), 0, 0.0, z('ws'), ws_bytes, None),
               'sg_conv2d_head_dgrad': (z('gy'), z('w'), z('out'), None),
               'sg_conv2d_head_wgrad': (z('gy'), z('x'), z('out'), z('ws'), ws_bytes, None)}


def _refused(lib, d, calls, only=None, needle=''):
    for fn, args in calls.items():
        if only is None or fn in only:
            rc = getattr(lib, fn)(dref(d), *args)
            assert rc != 0, '%s accepted the call' % fn
            assert err(lib).startswith(fn + ':') and needle in err(lib) and 'launch failed' not in err(lib), err(lib)


REFUSED = [e for e in HS.HEAD_EDGES + HS.SMALLM_EDGES if not e[2]]


@pytest.mark.parametrize('name,f,supported', REFUSED, ids=[e[0] for e in REFUSED])
def test_entry_points_refuse_what_the_predicates_refuse(name, f, supported):
    lib = _hip.lib()
    d = HS.desc_of(f)
    assert not HS.head_supported(f) and not HS.smallm_supported(f), 'refused by one predicate, taken by the other'
    for fam in ('head', 'smallm'):
        _, calls = _entry_calls(dict(family=fam), 1 << 30)
        _refused(lib, d, calls, needle='unsupported desc')
    assert lib.sg_conv2d_head_plan(dref(d), HS.HEAD_FWD, 0, 0, dref(_hip.sgHeadPlan())) != 0 and err(lib).startswith('sg_conv2d_head_plan: unsupported desc')
    assert lib.sg_conv2d_smallm_plan(dref(d), HS.SMALLM_FWD, dref(_hip.sgSmallmPlan())) != 0 and err(lib).startswith('sg_conv2d_smallm_plan: unsupported desc')


@pytest.mark.parametrize('case', [HS.BY_NAME[n] for n in ('sm_5x8_c5_m4', 'k3p1_7x9_c17', 'h1_stream_c16')], ids=lambda c: c['name'])
def test_entry_points_refuse_null_pointers_and_a_short_workspace(case):
    lib = _hip.lib()
    d = HS.desc_of(case)
    need = HS.case_ws_bytes(case)
    uses = {'sg_conv2d_smallm_fwd': 'x w out', 'sg_conv2d_smallm_wgrad': 'gy x out ws', 'sg_conv2d_head_fwd': 'x w out ws',
            'sg_conv2d_head_dgrad': 'gy w out', 'sg_conv2d_head_wgrad': 'gy x out ws'}
    for k in ('x', 'w', 'gy', 'out', 'ws'):
        _, calls = _entry_calls(case, need, **{k: 'null'})
        _refused(lib, d, calls, only=[fn for fn in calls if k in uses[fn].split()])
    _, calls = _entry_calls(case, need - 1)
    _refused(lib, d, calls, only=[fn for fn in calls if 'ws' in uses[fn].split()], needle='bad arguments')
    # the plan queries: a null plan, an unknown entry, an address that is no multiple of 4 modulo 16
    if case['family'] == 'head':
        p = _hip.sgHeadPlan()
        for args in ((HS.HEAD_FWD, 0, 0, None), (3, 0, 0, dref(p)), (-1, 0, 0, dref(p)), (HS.HEAD_FWD, 2, 0, dref(p)), (HS.HEAD_FWD, 0, 16, dref(p))):
            assert lib.sg_conv2d_head_plan(dref(d), *args) != 0 and err(lib) == 'sg_conv2d_head_plan: bad arguments'
    else:
        p = _hip.sgSmallmPlan()
        for args in ((HS.SMALLM_FWD, None), (1, dref(p)), (3, dref(p))):
            assert lib.sg_conv2d_smallm_plan(dref(d), *args) != 0 and err(lib) == 'sg_conv2d_smallm_plan: bad arguments'


@pytest.mark.parametrize('off', (4, 8, 12))
def test_smallm_refuses_a_misaligned_result_or_gradient_before_any_launch(off):
    """smallm_fwd_kernel stores y, smallm_wgrad_kernel loads gy as float4: an address off a 16-byte boundary is refused on the host
    (the error string names the alignment: a call that got as far as a launch without a device would report a launch failure instead)"""
    lib = _hip.lib()
    case = HS.BY_NAME['sm_5x8_c5_m4']
    d = HS.desc_of(case)
    h = _Host()
    _, calls = _entry_calls(case, HS.case_ws_bytes(case), out=h.at(48 + off))
    _refused(lib, d, calls, only=['sg_conv2d_smallm_fwd'], needle='y must be 16-byte aligned')
    _, calls = _entry_calls(case, HS.case_ws_bytes(case), gy=h.at(32 + off))
    _refused(lib, d, calls, only=['sg_conv2d_smallm_wgrad'], needle='gy must be 16-byte aligned')


def test_special_predicates_stay_disjoint_on_the_new_rows():
    lib = _hip.lib()
    preds = ('sg_conv2d_wino24_supported', 'sg_conv2d_head_supported', 'sg_conv2d_wino_supported', 'sg_conv2d_smallm_supported')
    for f in HS.CASES + HS.PROBES + [e[1] for e in HS.HEAD_EDGES + HS.SMALLM_EDGES]:
        d = HS.desc_of(f)
        ans = [bool(getattr(lib, p)(dref(d))) for p in preds]
        assert sum(ans) <= 1, (f, ans)
        if f in HS.CASES:
            assert ans == [False, f['family'] == 'head', False, f['family'] == 'smallm'], (f['name'], ans)
