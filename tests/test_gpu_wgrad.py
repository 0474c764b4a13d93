"""The weight-gradient GEMMs of csrc/igemm_nk.hip through the C ABI -- sg_conv2d_wgrad, sg_conv2d_wgrad_sparse,
sg_conv2d_wgrad_perimage (the Python operators would send many of these shapes to Winograd, smallm or head) -- against the float64
restatements of tests/wgrad_cases.py, row by row of its table.

Every launch: outputs pre-filled with a guard value, the workspace with NaN over the bytes offered (a slab or row-sum row the
launch reads without having written it -- an empty XCD-padding chunk, say -- is a NaN in the result, not a stale value) and guard
words behind them; the plan the library reports for THIS call (same options, same alignment of gy, same bytes) is the one the row
claims and the one wgrad_cases.py restates; every element within its own bound of float64 (wgrad_cases: gamma(n + c), c from the
reported plan); guards intact; a second call bit-identical.  The worst error / bound ratio per plan goes to wgrad_margins.json
(profiles/wgrad_test_margins.md holds a run's)."""
import ctypes

import pytest
import torch

import wgrad_cases as WG
from gpu_harness import Margins, Workspace, _KEEP, call, margins_fixture, options, outbuf, place, ptr, same_bits, stream, take
from gpu_harness import L, _release_operands  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGINS = Margins()
within = MARGINS.within
_margins = margins_fixture(lambda: MARGINS.dump('wgrad_margins.json'))      # the worst error / bound ratio per plan


FORMS = {WG.WG_TAP: 'tap', WG.WG_GATHER: 'gather', WG.WG_PADDED: 'padded'}
REDUCES = ('none', 'slab', 'wide', 'unpermute', 'sparse', 'perimage', 'group')


def family(case, plan):
    return '%s %s %dx%d %s%s%s reduce=%s xcd=%d' % (case['kind'], FORMS[plan['form']], plan['bm'], plan['bn'], 'vecA' if plan['a_vec'] else 'scalarA',
                                                    ' two' if plan['two'] else '', ' nomask' if plan['nomask'] else '', REDUCES[plan['reduce']],
                                                    plan['xcd'])


def run(L, case, a_off=None):
    """one C-ABI call of the row under the current options -> dict(plan, ws_bytes, gw, gb)"""
    d = WG.case_desc(case)
    inp = WG.case_inputs(case)
    entry = WG.ENTRY_OF[case['kind']]
    gyd = place(inp['gy'], case['a_off'] if a_off is None else a_off)
    x1d, x2d = place(inp['x1']), (None if inp['x2'] is None else place(inp['x2']))
    q = lambda nbytes: WG.wgrad_plan(L, d, entry, case['L'], gyd.data_ptr() % 16, nbytes)
    ws_bytes = WG.case_ws_bytes(case, q)
    plan = q(ws_bytes)
    assert plan is not None, L.sg_last_error_string().decode()
    assert 0 <= plan['ws_needed'] <= ws_bytes, (plan, ws_bytes)
    ws = Workspace(ws_bytes)
    wsp = ptr(ws.buf) if ws_bytes else None
    M, C, KS, N = case['Cout'], case['C1'] + case['C2'], case['KS'], case['N']
    ob = outbuf(M) if case['gb'] else None
    if case['kind'] == 'dense':
        o, shape = outbuf(M * C * KS * KS), (M, C, KS, KS)
        call(L, 'sg_conv2d_wgrad', ctypes.byref(d), ptr(gyd), ptr(x1d), ptr(x2d), ptr(o), ptr(ob), wsp, ws_bytes, stream())
    else:
        ld, cd = torch.from_numpy(inp['lists']).to(DEV), torch.from_numpy(inp['cnt']).to(DEV)
        _KEEP.extend([ld, cd])
        if case['kind'] == 'sparse':
            o, shape = outbuf(M * C * KS * KS), (M, C, KS, KS)
            call(L, 'sg_conv2d_wgrad_sparse', ctypes.byref(d), ptr(gyd), ptr(x1d), ptr(x2d), ptr(ld), ptr(cd), case['L'], ptr(o), ptr(ob),
                 wsp, ws_bytes, stream())
        else:
            o, shape = outbuf(N * M * case['L'] * KS * KS), (N, M, case['L'], KS, KS)
            call(L, 'sg_conv2d_wgrad_perimage', ctypes.byref(d), ptr(gyd), ptr(x1d), ptr(x2d), ptr(ld), ptr(cd), case['L'], ptr(o), wsp,
                 ws_bytes, stream())
    torch.cuda.synchronize()
    ws.intact(case['name'])
    return dict(plan=plan, ws_bytes=ws_bytes, gw=take(o, shape), gb=take(ob, (M,)) if case['gb'] else None)


def check(case, r, name):
    ref = WG.case_refs(case)
    fam = family(case, r['plan'])
    within(fam, r['gw'], ref['gw'], WG.gw_bound(case, r['plan']), name + ' gw')
    if r['gb'] is not None:
        within('bias gradient: %s' % ('row sums %dx%d %s' % (r['plan']['bm'], r['plan']['bn'], 'vecA' if r['plan']['a_vec'] else 'scalarA')
                                    if r['plan']['rowsum_fused'] else 'sg_channel_sum'), r['gb'], ref['gb'], ref['gb_bound'], name + ' gb')
    if case['kind'] == 'sparse':          # a channel nobody lists: exactly zero
        assert not r['gw'][:, case['C1'] + case['C2'] - 1].any()
    if case['kind'] == 'perimage':
        cnt = WG.case_inputs(case)['cnt']
        for b in range(case['N']):
            assert not r['gw'][b, :, int(cnt[b]):].any(), 'columns beyond the image\'s channel list must be zero'


@pytest.mark.parametrize('case', WG.CASES, ids=lambda c: c['name'])
def test_wgrad_case(L, case):
    with options(case['opts']):
        r = run(L, case)
        for k, v in case['claims'].items():
            assert r['plan'][k] == v, '%s: plan field %s is %s, the table claims %s (%s)' % (case['name'], k, r['plan'][k], v, r['plan'])
        assert r['plan'] == WG.case_py_plan(case, 4 * case['a_off'], r['ws_bytes']), case['name']
        check(case, r, case['name'])
        r2 = run(L, case)
        same_bits(r['gw'], r2['gw'], case['name'] + ': gw of a second call')
        if r['gb'] is not None:
            same_bits(r['gb'], r2['gb'], case['name'] + ': gb of a second call')
        if r['plan']['rowsum_fused']:
            # the bias gradient through sg_channel_sum instead: the same GEMM, bit for bit, and a bias gradient within its bound
            with options({'wgrad_rowsum': 0}):
                r0 = run(L, case)
            assert r0['plan'] == dict(r['plan'], rowsum_fused=0, ws_needed=r0['plan']['ws_needed']) and r0['plan']['ws_needed'] < r['plan']['ws_needed']
            check(case, r0, case['name'] + ' [wgrad_rowsum=0]')
            same_bits(r['gw'], r0['gw'], case['name'] + ': gw with and without the fused bias gradient')


ALIGNED_VEC = [c for c in WG.CASES if c['a_off'] == 0 and not c['opts'] and not callable(c['ws']) and c['ws'] == WG.AMPLE and
               WG.case_py_plan(c, 0, WG.AMPLE)['a_vec'] == 1]


@pytest.mark.parametrize('case', ALIGNED_VEC, ids=lambda c: c['name'])
def test_wgrad_misaligned_gy(L, case):
    """gy 4 bytes off a 16-byte boundary: the plan reports the scalar A loader, nothing else changes -- the same k-chunks, the same
    products into the same accumulators in the same order -- so the weight gradient equals the aligned run bit for bit (the row sums
    of the bias gradient are added across other lanes: within bound)"""
    with options(case['opts']):
        a, m = run(L, case, a_off=0), run(L, case, a_off=1)
    assert a['plan']['a_vec'] == 1 and m['plan'] == dict(a['plan'], a_vec=0), (a['plan'], m['plan'])
    check(case, m, case['name'] + ' [gy + 4 bytes]')
    same_bits(a['gw'], m['gw'], case['name'] + ': gw, aligned against misaligned gy')


PADDED = [c for c in WG.CASES if c['claims'].get('form') == WG.WG_PADDED]


@pytest.mark.parametrize('case', PADDED, ids=lambda c: c['name'])
def test_wgrad_padded_planes_equal_the_gather(L, case):
    """the padded-plane route changes where a gathered element comes from, not which products meet in which order"""
    with options(case['opts']):
        on = run(L, case)
        with options({'wgrad_padded': 0}):
            off = run(L, case)
    assert on['plan']['form'] == WG.WG_PADDED and off['plan'] == dict(on['plan'], form=WG.WG_GATHER, ws_needed=off['plan']['ws_needed'])
    check(case, off, case['name'] + ' [wgrad_padded=0]')
    same_bits(on['gw'], off['gw'], case['name'] + ': padded planes against the gather')
