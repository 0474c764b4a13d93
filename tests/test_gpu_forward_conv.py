"""The forward gathers of csrc/igemm_kn0.hip through the C ABI -- sg_conv2d_fwd, sg_conv2d_fwd_sparse, sg_conv2d_fwd_perimage (the
Python operators would send many of these shapes to Winograd, head, small-M or sub-pixel kernels) -- against the float64
restatements of tests/forward_conv_cases.py, row by row of its table and under each option set of a row.

Every launch: the workspace filled with NaN over the bytes offered (a slab the reduce reads without a workgroup having written it
is a NaN in the result) and guard words behind them; NaN around each input; the result pre-filled with a guard value and one guard word behind it; the plan
the library reports for THIS call (same options, the actual addresses of w, y and the workspace modulo 16, the same bytes) is the
one the row claims and the one forward_conv_cases.py restates; every element within its own bound of float64 (gamma(K + 1 + c), c
from the reported plan); a second call bit-identical.  The worst error / bound ratio per plan goes to forward_conv_margins.json
(profiles/forward_conv_test_margins.md holds a run's)."""
import ctypes

import numpy as np
import pytest
import torch

import forward_conv_cases as FC
from gpu_harness import (GUARD, Margins, Workspace, _KEEP, call, margins_fixture, opt_tag, options, outbuf, place, place_fenced, ptr, same,
                         same_bits, stream, take, twice)
from gpu_harness import L, _release_operands  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGINS = Margins()
within = MARGINS.within
_margins = margins_fixture(lambda: MARGINS.dump('forward_conv_margins.json'))      # the worst error / bound ratio per plan


def family(case, plan):
    src = ' bcast' if plan['bcast'] else (' two' if plan['two'] else '')
    ld = 'fixed' if plan['loader'] == FC.FW_FIXED else ('nomask' if plan['nomask'] else 'table')
    red = ('', ' reduce=vec', ' reduce=scalar')[plan['reduce']]
    return '%s %dx%d %s %s%s k%d%s' % (case['entry'], plan['bm'], plan['bn'], 'vecA' if plan['a_vec'] else 'scalarA', ld, src, case['KS'], red)


def run(L, case, inp, w_off=None, y_off=None, ws_off=None, ws_bytes=None, entry=None, expect_refusal=False):
    """one C-ABI call of the row under the current options on the operands ``inp`` -> dict(plan, ws_bytes, y)"""
    d = FC.case_desc(case)
    entry = case['entry'] if entry is None else entry
    w_off, y_off, ws_off = (case[k] if v is None else v for k, v in (('w_off', w_off), ('y_off', y_off), ('ws_off', ws_off)))
    ws_bytes = FC.case_ws_bytes(case) if ws_bytes is None else ws_bytes
    x1d, x2d = place_fenced(inp['x1']), (None if inp['x2'] is None else place_fenced(inp['x2']))
    wd = place(inp['wimg'] if entry == 'perimage' else inp['w'], w_off)
    bd = None if inp['b'] is None else place(inp['b'])
    N, M = case['N'], case['Cout']
    n = N * M * case['OH'] * case['OW']
    o = outbuf(n, y_off)
    assert (o.data_ptr() - 4 * y_off) % 16 == 0
    ws = Workspace(ws_bytes, ws_off)
    plan = FC.fwd_plan(L, d, FC.ENTRY_OF[entry], case['L'], wd.data_ptr() % 16, o.data_ptr() % 16, ws.buf.data_ptr() % 16, ws_bytes)
    args = [ctypes.byref(d), ptr(x1d), ptr(x2d), ptr(wd), ptr(bd)]
    if entry != 'dense':
        ld, cd = torch.from_numpy(inp['lists']).to(DEV), torch.from_numpy(inp['cnt']).to(DEV)
        _KEEP.extend([ld, cd])
        args += [ptr(ld), ptr(cd), case['L']]
    args += [ptr(o), case['act'], case['slope'], ptr(ws.buf), ws_bytes, stream()]
    if expect_refusal:
        rc = getattr(L, FC.ENTRY_FN[entry])(*args)
        torch.cuda.synchronize()
        return dict(plan=plan, rc=rc, error=L.sg_last_error_string().decode(), out=o.cpu().numpy(), ws=ws.host())
    assert plan is not None, L.sg_last_error_string().decode()
    assert 0 <= plan['ws_needed'] <= ws_bytes, (plan, ws_bytes)
    call(L, FC.ENTRY_FN[entry], *args)
    torch.cuda.synchronize()
    ws.intact(case['name'])
    return dict(plan=plan, ws_bytes=ws_bytes, y=take(o, (N, M, case['OH'], case['OW'])))


def check(case, r, name):
    ref = FC.case_refs(case)
    within(family(case, r['plan']), r['y'], ref['y'], FC.y_bound(case, r['plan']), name)
    if case['entry'] != 'dense':              # an image that lists nothing: act(bias), exactly
        inp = FC.case_inputs(case)
        b = np.zeros(case['Cout'], dtype=np.float32) if inp['b'] is None else inp['b']
        want = b if case['act'] == FC.ACT_NONE else np.where(b > 0, b, b * (np.float32(case['slope']) if case['act'] == FC.ACT_LEAKY else np.float32(0)))
        for n in np.nonzero(inp['cnt'] == 0)[0]:
            same(r['y'][n], np.broadcast_to(want.astype(np.float32)[:, None, None], r['y'][n].shape), name + ': image %d lists no channel' % n)


def assert_plan(case, r, o, name, **over):
    for k, v in case['claims'].items():
        assert r['plan'][k] == v, '%s: plan field %s is %s, the table claims %s (%s)' % (name, k, r['plan'][k], v, r['plan'])
    assert r['plan'] == FC.case_py_plan(case, o, ws_bytes=r['ws_bytes'], **over), name


# =============================================================================================
# the case table
# =============================================================================================
@pytest.mark.parametrize('case', FC.CASES, ids=lambda c: c['name'])
def test_forward_case(L, case):
    inp = FC.case_inputs(case)
    for o in FC.case_option_sets(case):
        with options(o):
            name = '%s [%s]' % (case['name'], opt_tag(o))
            _, r = twice(lambda: (lambda r: (r['y'], r))(run(L, case, inp)), name)          # (a second call: bit-identical)
            assert_plan(case, r, o, name)
            check(case, r, name)


def _py(case, **over):
    return FC.case_py_plan(case, case['opts'], **over)


DENSE = [c for c in FC.CASES if c['entry'] == 'dense' and c['name'] != 'tail_split_300_tiles']
VEC_SMALL = [c for c in DENSE if c['w_off'] == 0 and _py(c)['a_vec'] == 1 and _py(c)['bm'] != 128]


@pytest.mark.parametrize('case', VEC_SMALL, ids=lambda c: c['name'])
def test_misaligned_weights_equal_the_aligned_run(L, case):
    """w 4 bytes off a 16-byte boundary: the plan reports the scalar A loader -- and with it the table loader and the mask, where
    the aligned run had fixed taps or the mask-free loader -- on the same tile with the same k-chunks: the same products into the same
    accumulators in the same order, so y equals the aligned run bit for bit"""
    inp = FC.case_inputs(case)
    with options(case['opts']):
        a, m = run(L, case, inp, w_off=0), run(L, case, inp, w_off=1)
    assert a['plan']['a_vec'] == 1 and m['plan'] == dict(a['plan'], a_vec=0, loader=FC.FW_TABLE, nomask=0), (a['plan'], m['plan'])
    assert m['plan'] == _py(case, w_mod16=4)
    check(case, m, case['name'] + ' [w + 4 bytes]')
    same_bits(a['y'], m['y'], case['name'] + ': aligned against misaligned w')


SPLIT = [c for c in DENSE if _py(c)['splits'] > 1]


@pytest.mark.parametrize('case', SPLIT, ids=lambda c: c['name'])
def test_split_rows_reduce_alike_and_run_unsplit_on_a_short_workspace(L, case):
    """the float4 and the scalar slab reduce add the same slabs in the same order: bit-equal.  With the workspace cut to the k-table
    the plan drops the split and the GEMM stores the result itself, within its (smaller) bound"""
    inp = FC.case_inputs(case)
    with options(case['opts']):
        v, s = run(L, case, inp, y_off=0, ws_off=0), run(L, case, inp, y_off=1, ws_off=0)
        k = run(L, case, inp, ws_bytes=FC.ktab_bytes(v['plan']['K']))
    assert v['plan']['reduce'] in (FC.FR_VEC, FC.FR_SCALAR) and s['plan'] == dict(v['plan'], reduce=FC.FR_SCALAR), (v['plan'], s['plan'])
    same_bits(v['y'], s['y'], case['name'] + ': the two slab reduces')
    assert k['plan']['splits'] == 1 and k['plan']['reduce'] == FC.FR_NONE and k['plan']['kchunk'] == k['plan']['K'], k['plan']
    check(case, k, case['name'] + ' [workspace = the k-table]')


FIXED = [c for c in DENSE + FC.PROBES if c['entry'] == 'dense' and 'fixedtap' not in c['opts'] and _py(c)['loader'] == FC.FW_FIXED]


@pytest.mark.parametrize('case', FIXED, ids=lambda c: c['name'])
def test_fixed_taps_equal_the_table_loader(L, case):
    inp = FC.case_inputs(case) if case in DENSE else FC.probe_inputs(case)
    with options(case['opts']):
        f = run(L, case, inp)
        with options({'fixedtap': 0}):
            t = run(L, case, inp)
    assert f['plan']['loader'] == FC.FW_FIXED and t['plan']['loader'] == FC.FW_TABLE and t['plan']['a_vec'] == 1
    assert dict(t['plan'], loader=FC.FW_FIXED, nomask=0) == f['plan'], (f['plan'], t['plan'])
    same_bits(f['y'], t['y'], case['name'] + ': fixedtap 1 against 0')


SPARSE = [c for c in FC.CASES if c['entry'] == 'sparse']


@pytest.mark.parametrize('case', SPARSE, ids=lambda c: c['name'])
def test_sparse_equals_dense_on_zero_filled_input_and_perimage_on_gathered_weights(L, case):
    inp = FC.case_inputs(case)
    with options(case['opts']):
        sp = run(L, case, inp)
        # the dense entry on the input with every unlisted channel zeroed: the same sum in another order
        z = dict(inp)
        C1 = case['C1']
        z['x1'] = inp['x1'].copy()
        z['x2'] = None if inp['x2'] is None else inp['x2'].copy()
        for b in range(case['N']):
            listed = set(int(c) for c in inp['lists'][b][:inp['cnt'][b]])
            for c in range(C1 + case['C2']):
                if c not in listed:
                    if c < C1:
                        z['x1'][b, c] = 0
                    else:
                        z['x2'][b, c - C1] = 0
        dn = run(L, case, z, entry='dense')
        both = FC.y_bound(case, sp['plan']) + FC.y_bound(case, dn['plan'])
        within('sparse against dense', sp['y'], dn['y'], both, case['name'])
        # the per-image entry with the weights gathered through the lists: the same compact rows, bit for bit
        pi = run(L, case, dict(inp, wimg=FC.gather_wimg(inp['w'], inp['lists'], inp['cnt'])), entry='perimage')
    assert pi['plan'] == sp['plan']
    same_bits(sp['y'], pi['y'], case['name'] + ': sparse against per-image')


@pytest.mark.parametrize('case', FC.PROBES, ids=lambda c: c['name'])
def test_onehot_probes_are_exact(L, case):
    """weights that select one (channel or list position, tap) per output channel: y is a copy of input values, bit for bit"""
    inp = FC.probe_inputs(case)
    with options(case['opts']):
        r = run(L, case, inp)
    for k, v in case['claims'].items():
        assert r['plan'][k] == v, (case['name'], k, r['plan'])
    same(r['y'], FC.probe_placement(case, inp), case['name'])


@pytest.mark.parametrize('case', [FC.BY_NAME['sp_64x64_k3'], FC.BY_NAME['pi_k4s2']], ids=lambda c: c['name'])
def test_list_entries_refuse_a_misaligned_workspace(L, case):
    """the compact weights are read as float4 from the workspace: one that is not 16-byte aligned is refused on the host -- a
    non-zero return, an error string, the result and the workspace untouched"""
    inp = FC.case_inputs(case)
    for off in (1, 2, 3):
        r = run(L, case, inp, ws_off=off, expect_refusal=True)
        assert r['rc'] != 0 and r['plan'] is None and '16-byte aligned' in r['error'] and FC.ENTRY_FN[case['entry']] in r['error'], r['error']
        assert (r['out'] == GUARD).all(), 'a refused call wrote to the result'
        words = (FC.case_ws_bytes(case) + 3) // 4
        assert np.isnan(r['ws'][off:off + words]).all() and (r['ws'][off + words:] == GUARD).all() and (r['ws'][:off] == GUARD).all()
