"""Every Winograd form of csrc/igemm.hip -- F(2x2,3x3) generic and adjoint, F(4x4,3x3), the fused F(4x4,3x3) + InstanceNorm pair and
F(2x2,4x4) -- through the C ABI against the direct float64 convolution.  The cases, their inputs, the references and the criteria
are tests/winograd_cases.py; tests/test_winograd_cases_cpu.py shows that the references are sound, that the criteria catch mutants
and that the table reaches every plan value.

Each case asserts the plan the library reports for the launch it makes (sg_conv2d_wino_plan, with the alignment of the operands as
placed and the saved operands as passed), runs every entry twice (bit-equal), with every combination of saved operands the entry
accepts, and holds each result to the hard bound per element and to the rms line (rms error <= 2 x the float32 restatement's).
One-hot probes carry the index logic: the hard bound with n = 1, which is exact equality wherever the form's tiles do not reach.
The worst ratios of every family go to winograd_margins.json."""
import time

import numpy as np
import pytest
import torch

import winograd_cases as WC
from gpu_harness import GUARD, Workspace, _dump, call, close, dref, opt_tag, options, outbuf, place, ptr, scratch, stream, take, twice
from gpu_harness import L, _release_operands  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 1e-5
_MARGINS = {}
_T0 = [0.0]


@pytest.fixture(scope='module', autouse=True)
def _margins():
    """after the module: per family the worst error / hard bound and the worst rms / float32-restatement rms -> winograd_margins.json"""
    _T0[0] = time.time()
    yield
    out = {k: {'ratio_of_hard_bound': v[0], 'hard_case': v[1], 'rms_over_baseline': v[2], 'rms_case': v[3]} for k, v in _MARGINS.items()}
    out['_module_seconds'] = time.time() - _T0[0]
    _dump('winograd_margins.json', out)


def noter(family):
    def note(name, ratio, r):
        m = _MARGINS.setdefault(family, [0.0, '', 0.0, ''])
        if ratio > m[0]:
            m[0], m[1] = float(ratio), name
        if r > m[2]:
            m[2], m[3] = float(r), name
        print('%s %s: error / hard bound %.4f, rms / baseline %.3f' % (family, name, ratio, r))
    return note


def option_sets(case):
    return [dict(case['opts'])] + [dict(case['opts'], **o) for (n, o, _) in WC.OPTION_TOGGLES if n == case['name']]


def align_of(**ops):
    """SG_WA_* mask of the operands as placed (a missing or null operand counts as aligned)"""
    bits = dict(x=WC.WA_X, w=WC.WA_W, y=WC.WA_Y, gy=WC.WA_GY, gx=WC.WA_GX, gw=WC.WA_GW)
    m = WC.WA_ALL
    for k, t in ops.items():
        if t is not None and t.data_ptr() % 16:
            m &= ~bits[k]
    return m


def assert_plan(L, case, d, entry, opts, align, saved, name):
    got = WC.wino_plan(L, d, entry, align, saved)
    assert got is not None, '%s: no plan (%s)' % (name, L.sg_last_error_string().decode())
    want = WC.expected_plan(case, entry, opts, align=align, saved=saved)
    assert got == want, '%s: plan %s, expected %s' % (name, {k: got[k] for k in got if got[k] != want[k]}, {k: want[k] for k in got if got[k] != want[k]})
    return got


def saved_sizes(d, plan):
    xi = 36 if plan['form'] == WC.WF_F43 else 16
    return xi * d.C1 * d.Cout, xi * plan['P'] * d.C1, xi * plan['P'] * d.Cout


# ---- the entry points, one C-ABI call each ---------------------------------------------------------------------------
def wino_ws(L, d, f24=False):
    n = int((L.sg_conv2d_wino24_ws_bytes if f24 else L.sg_conv2d_wino_ws_bytes)(dref(d)))
    assert n > 0
    return scratch(n), n


def run_fwd(L, d, xd, wd, bd, sizes=None, saved=0):
    """-> (y, ut_save buffer or None, v_save buffer or None)"""
    ws, n = wino_ws(L, d)
    ut = outbuf(sizes[0]) if saved & WC.WS_UT else None
    v = outbuf(sizes[1]) if saved & WC.WS_V else None
    o = outbuf(d.N * d.Cout * d.OH * d.OW)
    call(L, 'sg_conv2d_wino_fwd', dref(d), ptr(xd), ptr(wd), ptr(bd), ptr(o), 0, 0.0, ptr(ut), ptr(v), ptr(ws), n, stream())
    for s in (ut, v):
        if s is not None:
            assert float(s[-1]) == GUARD, 'a saved operand was written behind its size'
    return take(o, (d.N, d.Cout, d.OH, d.OW)), ut, v


def run_dgrad(L, d, gd, wd, sizes=None, ut=None, keep_ytp=False):
    ws, n = wino_ws(L, d)
    ytp = outbuf(sizes[2]) if keep_ytp else None
    o = outbuf(d.N * d.C1 * d.H * d.W)
    call(L, 'sg_conv2d_wino_dgrad', dref(d), ptr(gd), ptr(wd), ptr(o), ptr(ut), ptr(ytp), ptr(ws), n, stream())
    if ytp is not None:
        assert float(ytp[-1]) == GUARD, 'ytp_save was written behind its size'
    return take(o, (d.N, d.C1, d.H, d.W)), ytp


def run_wgrad(L, d, gd, xd, v=None, ytp=None):
    ws, n = wino_ws(L, d)
    o = outbuf(d.Cout * d.C1 * 9)
    call(L, 'sg_conv2d_wino_wgrad', dref(d), ptr(gd), ptr(xd), ptr(o), ptr(v), ptr(ytp), ptr(ws), n, stream())
    return (take(o, (d.Cout, d.C1, 3, 3)),)


def run24(L, d, what, a, b, bias=None):
    ws, n = wino_ws(L, d, f24=True)
    if what == 'fwd':
        o = outbuf(d.N * d.Cout * d.OH * d.OW)
        call(L, 'sg_conv2d_wino24_fwd', dref(d), ptr(a), ptr(b), ptr(bias), ptr(o), 0, 0.0, ptr(ws), n, stream())
        return (take(o, (d.N, d.Cout, d.OH, d.OW)),)
    if what == 'dgrad':
        o = outbuf(d.N * d.C1 * d.H * d.W)
        call(L, 'sg_conv2d_wino24_dgrad', dref(d), ptr(a), ptr(b), ptr(o), ptr(ws), n, stream())
        return (take(o, (d.N, d.C1, d.H, d.W)),)
    o = outbuf(d.Cout * d.C1 * 16)
    call(L, 'sg_conv2d_wino24_wgrad', dref(d), ptr(a), ptr(b), ptr(o), ptr(ws), n, stream())
    return (take(o, (d.Cout, d.C1, 4, 4)),)


def with_bias(r, b):
    """(reference, hard bound) of y + bias: the bias joins the absolute sum (its add is one of the C_JOIN roundings)"""
    b64 = np.asarray(b, dtype=np.float64)[None, :, None, None]
    n = r['n']['y']
    return r['ref']['y'] + b64, r['y_bound'] + WC.gamma(n + r['form'].c) * np.abs(b64)


# =============================================================================================
# the case table
# =============================================================================================
@pytest.mark.parametrize('case', WC.CASES, ids=lambda c: c['name'])
def test_winograd_case(L, case):
    d = WC.case_desc(case)
    r = WC.case_refs(case)
    inp, ref, fam = r['inp'], r['ref'], case['family']
    note = noter(fam)
    f24 = fam == 'F24'
    xd, wd, bd = place(inp['x'], case['off'].get('x', 0)), place(inp['w'], case['off'].get('w', 0)), place(inp['b'])
    gd = place(inp['gy'], case['off'].get('gy', 0))
    yref, ybound = with_bias(r, inp['b'])
    for opts in option_sets(case):
        with options(opts):
            tag = '%s [%s]' % (case['name'], opt_tag(opts, 'defaults'))
            if f24:
                for entry, what, a, b, bias, key in ((WC.WINO24_FWD, 'fwd', xd, wd, bd, 'y'), (WC.WINO24_DGRAD, 'dgrad', gd, wd, None, 'gx'),
                                                     (WC.WINO24_WGRAD, 'wgrad', gd, xd, None, 'gw')):
                    assert_plan(L, case, d, entry, opts, WC.WA_ALL, 0, tag)
                    got, = twice(lambda: run24(L, d, what, a, b, bias), tag + ' ' + what)
                    rf, bd_ = (yref, ybound) if key == 'y' else (ref[key], r[key + '_bound'])
                    WC.check(got, rf, bd_, r[key + '_rms32'], '%s %s' % (tag, key), note)
                continue
            # ---- forward, every combination of ut_save / v_save
            kept, first = {}, None
            for sm in WC.saved_masks(case, WC.WINO_FWD, opts):
                plan = assert_plan(L, case, d, WC.WINO_FWD, opts, align_of(x=xd, w=wd), sm, tag + ' fwd saved=%d' % sm)
                sizes = saved_sizes(d, plan)
                y, ut, v = twice(lambda: run_fwd(L, d, xd, wd, bd, sizes, sm), tag + ' fwd')[:3]
                WC.check(y, yref, ybound, r['y_rms32'], '%s y saved=%d' % (tag, sm), note)
                if plan['form'] == WC.WF_F43:
                    first = y if first is None else first
                    assert np.array_equal(y, first), '%s: the forward differs with saved operands %d' % (tag, sm)
                kept.update({k: t for k, t in (('ut', ut), ('v', v)) if t is not None})
            # ---- data gradient, every combination of ut_saved / ytp_save
            first = None
            for sm in WC.saved_masks(case, WC.WINO_DGRAD, opts):
                if sm & WC.WS_UT and 'ut' not in kept:
                    continue            # (the forward of this option set hands no filter transform on: wino_wt = 0)
                plan = assert_plan(L, case, d, WC.WINO_DGRAD, opts, align_of(gy=gd, w=wd), sm, tag + ' dgrad saved=%d' % sm)
                assert plan['form'] == case['dgrad_form'], tag
                sizes = saved_sizes(d, WC.wino_plan(L, d, WC.WINO_FWD, align_of(x=xd, w=wd), 0))
                ut = kept['ut'][:-1] if sm & WC.WS_UT else None
                gx, ytp = twice(lambda: run_dgrad(L, d, gd, wd, sizes, ut, bool(sm & WC.WS_YTP)), tag + ' dgrad')[:2]
                WC.check(gx, ref['gx'], r['gx_bound'], r['gx_rms32'], '%s gx saved=%d' % (tag, sm), note)
                if plan['form'] == WC.WF_F43:
                    first = gx if first is None else first
                    assert np.array_equal(gx, first), '%s: the data gradient differs with saved operands %d' % (tag, sm)
                if ytp is not None:
                    kept['ytp'] = ytp
            # ---- weight gradient, rebuilt and from the saved operands
            first = None
            for sm in WC.saved_masks(case, WC.WINO_WGRAD, opts):
                if sm and not ('v' in kept and 'ytp' in kept):
                    continue
                plan = assert_plan(L, case, d, WC.WINO_WGRAD, opts, align_of(x=xd, gy=gd), sm, tag + ' wgrad saved=%d' % sm)
                v, ytp = (kept['v'][:-1], kept['ytp'][:-1]) if sm else (None, None)
                gw, = twice(lambda: run_wgrad(L, d, gd, xd, v, ytp), tag + ' wgrad')
                WC.check(gw, ref['gw'], r['gw_bound'], r['gw_rms32'], '%s gw saved=%d' % (tag, sm), note)
                if plan['form'] == WC.WF_F43:
                    first = gw if first is None else first
                    assert np.array_equal(gw, first), '%s: the weight gradient differs between saved and rebuilt operands' % tag


# =============================================================================================
# one-hot probes
# =============================================================================================
def _sub_case(case, N=None, Cin=None, Cout=None):
    return dict(case, N=N or case['N'], Cin=Cin or case['Cin'], Cout=Cout or case['Cout'])


def _probe_check(case, form, got, sub_inp, key, place_fn, name, note, bias=None):
    """got: the full output; sub_inp: the operands cut to the image / channels the one-hot touches; place_fn(full-shaped zeros, sub
    result) -> where that sub result sits in the full output.  Hard bound with n = 1; outside it the output is exactly 0 / the bias."""
    sub = _sub_case(case, N=sub_inp['x'].shape[0], Cin=sub_inp['x'].shape[1], Cout=sub_inp['gy'].shape[1])
    ref = WC.direct64(sub, sub_inp)[key]
    babs = WC.restate(sub, form.abs(), {k: np.abs(v) for k, v in sub_inp.items()}, np.float64, which=(key,))[key]
    full_ref, full_abs = np.zeros(got.shape), np.zeros(got.shape)
    place_fn(full_ref, ref)
    place_fn(full_abs, babs)
    bound = WC.gamma(1 + form.c) * full_abs
    if bias is not None:
        b64 = np.asarray(bias, dtype=np.float64)[None, :, None, None]
        bound = np.where(full_abs > 0, bound + WC.gamma(1 + form.c) * np.abs(b64), 0.0)
        full_ref = full_ref + b64
    assert (full_abs > 0).any() and (full_abs == 0).any(), name
    WC.check(got, full_ref, bound, 1.0, name, note, rms_line=False)


@pytest.mark.parametrize('name', WC.PROBE_CASES)
def test_winograd_onehot_probes(L, name):
    case = WC.BY_NAME[name]
    d = WC.case_desc(case)
    r = WC.case_refs(case)
    inp, form, fam = r['inp'], r['form'], case['family']
    f24 = fam == 'F24'
    note = noter(fam + '_probe')
    goff = case['off'].get('gy', 0)
    with options(case['opts']):
        wd, bd, xd, gd = place(inp['w']), place(inp['b']), place(inp['x']), place(inp['gy'], goff)
        fwd = (lambda x_, w_: run24(L, d, 'fwd', x_, w_, bd)[0]) if f24 else (lambda x_, w_: run_fwd(L, d, x_, w_, bd)[0])
        dgrad = (lambda g_, w_: run24(L, d, 'dgrad', g_, w_)[0]) if f24 else (lambda g_, w_: run_dgrad(L, d, g_, w_)[0])
        wgrad = (lambda g_, x_: run24(L, d, 'wgrad', g_, x_)[0]) if f24 else (lambda g_, x_: run_wgrad(L, d, g_, x_)[0])
        # one-hot x: image n alone carries anything but the bias, and only where the tiles of the pixel reach
        for (n, c, pos) in WC.probe_sites(d.N, d.C1, d.H, d.W):
            x1 = WC.onehot((d.N, d.C1, d.H, d.W), n, c, pos)
            sub = dict(x=x1[n:n + 1, c:c + 1], w=inp['w'][:, c:c + 1], gy=inp['gy'][n:n + 1])

            def put(full, part, n=n):
                full[n] = part[0]
            _probe_check(case, form, fwd(place(x1), wd), sub, 'y', put, '%s x one-hot %s' % (name, (n, c, pos)), note, bias=inp['b'])
        # one-hot w, tap by tap: output channel co alone, y[:, co] = the shifted input channel ci
        for t, (kh, kw) in enumerate(WC.probe_w_taps(d.KS)):
            co, ci = (0, d.Cout - 1)[t % 2], (d.C1 - 1, 0)[t % 2]
            w1 = np.zeros(inp['w'].shape, dtype=np.float32)
            w1[co, ci, kh, kw] = 1.0
            sub = dict(x=inp['x'][:, ci:ci + 1], w=w1[co:co + 1, ci:ci + 1], gy=inp['gy'][:, co:co + 1])

            def put(full, part, co=co):
                full[:, co] = part[:, 0]
            _probe_check(case, form, fwd(xd, place(w1)), sub, 'y', put, '%s w one-hot %s' % (name, (co, ci, kh, kw)), note, bias=inp['b'])
        # one-hot gy: the data gradient of image n alone, the weight gradient of output channel co alone
        for (n, co, pos) in WC.probe_sites(d.N, d.Cout, d.OH, d.OW):
            g1 = place(WC.onehot((d.N, d.Cout, d.OH, d.OW), n, co, pos), goff)
            sub = dict(x=inp['x'][n:n + 1], w=inp['w'][co:co + 1], gy=WC.onehot((1, 1, d.OH, d.OW), 0, 0, pos))

            def put_gx(full, part, n=n):
                full[n] = part[0]

            def put_gw(full, part, co=co):
                full[co] = part[0]
            _probe_check(case, form, dgrad(g1, wd), sub, 'gx', put_gx, '%s gy one-hot %s gx' % (name, (n, co, pos)), note)
            _probe_check(case, form, wgrad(g1, xd), sub, 'gw', put_gw, '%s gy one-hot %s gw' % (name, (n, co, pos)), note)


# =============================================================================================
# the fused F(4x4,3x3) conv + InstanceNorm pair, stage by stage
# =============================================================================================
def _act(z, act, slope):
    return z if act == 0 else np.where(z > 0, z, (0.0 if act == 1 else slope) * z)


def _act_grad(z, act, slope):
    return np.ones_like(z) if act == 0 else np.where(z > 0, 1.0, 0.0 if act == 1 else slope)


def run_fused_fwd(L, d, xd, wd, bd, sd, act, slope, sizes, saved):
    ws, n = wino_ws(L, d)
    numel = d.N * d.Cout * d.H * d.W
    ut = outbuf(sizes[0]) if saved & WC.WS_UT else None
    v = outbuf(sizes[1]) if saved & WC.WS_V else None
    ypre, out, mean, rstd = outbuf(numel), outbuf(numel), outbuf(d.N * d.Cout), outbuf(d.N * d.Cout)
    call(L, 'sg_conv2d_wino_fwd_instnorm', dref(d), ptr(xd), ptr(wd), ptr(bd), ptr(sd), ptr(ypre), ptr(out), ptr(mean), ptr(rstd), EPS, act,
         slope, ptr(ut), ptr(v), ptr(ws), n, stream())
    shp = (d.N, d.Cout, d.H, d.W)
    return take(ypre, shp), take(out, shp), take(mean, (d.N, d.Cout)), take(rstd, (d.N, d.Cout)), ut, v, ypre, mean, rstd


def run_fused_bwd(L, d, god, ypre, mean, rstd, act, slope, wd, want_gx, want_gb, ut, sizes, keep_ytp):
    ws, n = wino_ws(L, d)
    gconv = outbuf(d.N * d.Cout * d.H * d.W)
    gx = outbuf(d.N * d.C1 * d.H * d.W) if want_gx else None
    gb = outbuf(d.Cout) if want_gb else None
    ytp = outbuf(sizes[2]) if keep_ytp else None
    call(L, 'sg_conv2d_wino_dgrad_instnorm', dref(d), ptr(god), ptr(ypre), ptr(mean), ptr(rstd), act, slope, ptr(wd), ptr(gconv), ptr(gx),
         ptr(gb), ptr(ut), ptr(ytp), ptr(ws), n, stream())
    return (take(gconv, (d.N, d.Cout, d.H, d.W)), take(gx, (d.N, d.C1, d.H, d.W)) if want_gx else None,
            take(gb, (d.Cout,)) if want_gb else None, ytp, gconv)


def fused_pair(L, case, act, with_skip, note):
    """the whole pair on the case -> dict of results, every stage checked against float64 of the stage's own (GPU) input"""
    d = WC.case_desc(case)
    r = WC.case_refs(case)
    inp, form = r['inp'], r['form']
    slope = 0.2
    rng = WC.rng_of(case['name'] + ' fused %d %d' % (act, with_skip))
    skip = WC.f32(rng, (d.N, d.Cout, d.H, d.W)) if with_skip else None
    gout = WC.f32(rng, (d.N, d.Cout, d.H, d.W))
    xd, wd, bd, god = place(inp['x']), place(inp['w']), place(inp['b']), place(gout)
    sd = place(skip) if with_skip else None
    tag = '%s fused act=%d skip=%d' % (case['name'], act, with_skip)
    plan = WC.wino_plan(L, d, WC.WINO_FWD_INSTNORM, WC.WA_ALL, WC.WS_UT | WC.WS_V)
    want = WC.expected_plan(case, WC.WINO_FWD_INSTNORM, saved=WC.WS_UT | WC.WS_V)
    assert plan == want and plan['norm_tiles'] == (1 if (d.H // 4) * (d.W // 4) <= 4 else 4), (tag, plan)
    sizes = saved_sizes(d, plan)
    f = twice(lambda: run_fused_fwd(L, d, xd, wd, bd, sd, act, slope, sizes, WC.WS_UT | WC.WS_V), tag + ' fwd')
    ypre, out, mean, rstd, ut, v, ypre_d, mean_d, rstd_d = f
    plain = run_fused_fwd(L, d, xd, wd, bd, sd, act, slope, sizes, 0)
    for a, b in zip(plain[:4], f[:4]):
        assert np.array_equal(a, b), tag + ': the fused forward differs without saved operands'
    yref, ybound = with_bias(r, inp['b'])
    WC.check(ypre, yref, ybound, r['y_rms32'], tag + ' ypre', note)
    # InstanceNorm in float64 of the GPU's own ypre
    y64 = ypre.astype(np.float64)
    m64 = y64.mean(axis=(2, 3))
    r64 = 1.0 / np.sqrt(y64.var(axis=(2, 3)) + EPS)
    z = (y64 - m64[:, :, None, None]) * r64[:, :, None, None]
    o64 = _act(z, act, slope) + (skip.astype(np.float64) if with_skip else 0.0)
    close(torch.from_numpy(out), o64, 2e-5, tag + ' out')
    close(torch.from_numpy(mean), m64, 2e-5, tag + ' mean')
    close(torch.from_numpy(rstd), r64, 2e-5, tag + ' rstd')
    # backward: the norm's gradient in float64 of (gout, GPU ypre); units at the activation kink are left out
    bplan = WC.wino_plan(L, d, WC.WINO_DGRAD_INSTNORM, WC.WA_ALL, WC.WS_UT | WC.WS_YTP)
    assert bplan == WC.expected_plan(case, WC.WINO_DGRAD_INSTNORM, saved=WC.WS_UT | WC.WS_YTP), (tag, bplan)
    bw = twice(lambda: run_fused_bwd(L, d, god, ypre_d[:-1], mean_d[:-1], rstd_d[:-1], act, slope, wd, True, True, ut[:-1], sizes, True)[:4],
               tag + ' bwd')
    gconv, gx, gb, ytp = bw
    gz = gout.astype(np.float64) * _act_grad(z, act, slope)
    g64 = r64[:, :, None, None] * (gz - gz.mean(axis=(2, 3), keepdims=True) - z * (gz * z).mean(axis=(2, 3), keepdims=True))
    kink = (np.abs(z) <= 1e-5) if act else np.zeros(z.shape, dtype=bool)
    assert kink.mean() <= 1e-4, '%s: %d of %d units at the kink' % (tag, int(kink.sum()), kink.size)
    close(torch.from_numpy(np.where(kink, g64, gconv)), g64, 1e-4, tag + ' gconv')
    # variants: rebuilt filter transform, gx NULL, gb NULL -- the same numbers
    for (want_gx, want_gb, use_ut) in ((True, True, False), (False, True, True), (True, False, True)):
        o = run_fused_bwd(L, d, god, ypre_d[:-1], mean_d[:-1], rstd_d[:-1], act, slope, wd, want_gx, want_gb, ut[:-1] if use_ut else None, sizes, False)
        assert np.array_equal(o[0], gconv), tag + ': gconv differs between variants'
        assert o[1] is None or np.array_equal(o[1], gx), tag + ': gx differs between variants'
        assert o[2] is None or np.array_equal(o[2], gb), tag + ': gb differs between variants'
    # gx, gw: the data- and weight-gradient criteria with gy := the GPU's gconv
    inp2 = dict(inp, gy=gconv)
    ref2 = WC.direct64(case, inp2)
    babs = WC.restate(case, form.abs(), {k: np.abs(t) for k, t in inp2.items()}, np.float64, which=('gx', 'gw'))
    r32 = WC.restate(case, form, inp2, np.float32, which=('gx', 'gw'))
    nred = WC.reduction_lengths(case)
    # (the saved Ytp is w43_gy_in_kernel's: transformed from gconv before it is rounded to fp32 for the store, so the weight gradient
    # on saved operands and the one rebuilt from the stored gconv are different roundings of the same sum -- both meet the criteria)
    gw_saved, = twice(lambda: run_wgrad(L, d, place(gconv), xd, v[:-1], ytp[:-1]), tag + ' wgrad saved')
    gw_rebuilt, = run_wgrad(L, d, place(gconv), xd)
    for key, got in (('gx', gx), ('gw', gw_saved), ('gw', gw_rebuilt)):
        WC.check(got, ref2[key], WC.gamma(nred[key] + form.c) * babs[key], WC.rms(r32[key].astype(np.float64) - ref2[key]), '%s %s' % (tag, key), note)
    gb64 = gconv.astype(np.float64).sum(axis=(0, 2, 3))
    gbound = WC.gamma(d.N * d.H * d.W) * np.abs(gconv.astype(np.float64)).sum(axis=(0, 2, 3))
    WC.check(gb, gb64, gbound, 1.0, tag + ' gb', noter('fused_gb'), rms_line=False)
    return dict(out=out, gx=gx, gw=gw_saved, gb=gb, skip=skip, gout=gout)


@pytest.mark.parametrize('with_skip', (0, 1))
@pytest.mark.parametrize('act', (0, 1, 2))
@pytest.mark.parametrize('name', WC.FUSED_CASES)
def test_fused_conv_instnorm_pair(L, name, act, with_skip):
    fused_pair(L, WC.BY_NAME[name], act, with_skip, noter('F43_fused'))


def test_fused_backward_bias_partials_stay_inside_the_workspace(L):
    """The fused data gradient keeps its [N][Cout] partial bias gradients in the workspace, behind G.  Per-object convolutions on
    4x4 planes are where that region is largest against the rest (N = 4672 > 36 * C1: 598 016 floats where the filter-sized block
    behind G has 589 824).  gx = NULL: no GEMM runs, so the reference is the InstanceNorm backward and a sum in float64.  The
    workspace is exactly what sg_conv2d_wino_ws_bytes reports, with guard values behind it."""
    N, C, H, W, act, slope = 4672, 128, 4, 4, 2, 0.2
    d = WC.make_desc(N, C, H, W, C, 3, 1, 1, True, 1, H, W)
    plan = WC.wino_plan(L, d, WC.WINO_DGRAD_INSTNORM, WC.WA_ALL, 0)
    assert plan is not None, L.sg_last_error_string().decode()
    assert (plan['form'], plan['P'], plan['wt_kernel'], plan['fold_kernel']) == (WC.WF_F43, N * (H // 4) * (W // 4), WC.WK_WT_LDS, WC.WK_FOLD_F43), plan
    rng = WC.rng_of('fused backward, 4672 images of 4x4')
    gout, ypre = WC.f32(rng, (N, C, H, W)), WC.f32(rng, (N, C, H, W))
    y64 = ypre.astype(np.float64)
    mean = y64.mean(axis=(2, 3)).astype(np.float32)
    rstd = (1.0 / np.sqrt(y64.var(axis=(2, 3)) + EPS)).astype(np.float32)
    nbytes = int(L.sg_conv2d_wino_ws_bytes(dref(d)))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Workspace(nbytes, guards=1024, nan=False)
    god, yd, md, rd, wd = place(gout), place(ypre), place(mean), place(rstd), place(np.zeros(C * C * 9, dtype=np.float32))
    gconv_d, gb_d = outbuf(N * C * H * W), outbuf(C)
    call(L, 'sg_conv2d_wino_dgrad_instnorm', dref(d), ptr(god), ptr(yd), ptr(md), ptr(rd), act, slope, ptr(wd), ptr(gconv_d), None,
         ptr(gb_d), None, None, ptr(ws.buf), nbytes, stream())
    gconv, gb = take(gconv_d, (N, C, H, W)), take(gb_d, (C,))
    ws.intact('the fused data gradient')
    # the norm's gradient in float64 of the operands as passed (mean / rstd rounded to fp32); units at the activation kink left out
    r64 = rstd.astype(np.float64)[:, :, None, None]
    z = (y64 - mean.astype(np.float64)[:, :, None, None]) * r64
    gz = gout.astype(np.float64) * _act_grad(z, act, slope)
    g64 = r64 * (gz - gz.mean(axis=(2, 3), keepdims=True) - z * (gz * z).mean(axis=(2, 3), keepdims=True))
    kink = np.abs(z) <= 1e-5
    assert kink.mean() <= 1e-4, '%d of %d units at the kink' % (int(kink.sum()), kink.size)
    close(torch.from_numpy(np.where(kink, g64, gconv)), g64, 1e-4, 'fused backward 4672x4x4 gconv')
    # gb: the sum of the GPU's own gconv, reduction length N * H * W; baseline of the rms line: the same sum in float32, per image
    # and then over the images in ascending order (w43_bias_sum_kernel's order)
    c64 = gconv.astype(np.float64)
    gb64 = c64.sum(axis=(0, 2, 3))
    gbound = WC.gamma(N * H * W) * np.abs(c64).sum(axis=(0, 2, 3))
    per_image = gconv.reshape(N, C, H * W).sum(axis=2, dtype=np.float32)
    gb32 = np.cumsum(per_image, axis=0, dtype=np.float32)[-1]
    WC.check(gb, gb64, gbound, WC.rms(gb32.astype(np.float64) - gb64), 'fused backward 4672x4x4 gb', noter('fused_gb_large_n'))


# =============================================================================================
# argument checks: non-zero before any launch, outputs untouched
# =============================================================================================
def _rejected(L, fn, args, outs, message):
    rc = getattr(L, fn)(*args)
    assert rc != 0, '%s accepted a bad call' % fn
    msg = L.sg_last_error_string().decode()
    assert message in msg, (fn, msg)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == GUARD).all()), '%s wrote to an output it rejected' % fn


def test_rejected_arguments(L):
    s = stream()
    c43, cz, c24 = WC.BY_NAME['f43_16_128to128_8x8'], WC.BY_NAME['f23z_2_128to128_16x16'], WC.BY_NAME['f24_4_128to128_17x17_p2']
    for case in (c43, cz):
        d = WC.case_desc(case)
        inp = WC.case_inputs(case)
        ws, n = wino_ws(L, d)
        numel = d.N * d.Cout * d.OH * d.OW
        x0, x1, w0, g0, g1 = place(inp['x']), place(inp['x'], 1), place(inp['w']), place(inp['gy']), place(inp['gy'], 1)
        y, gx, gw, sv = outbuf(numel), outbuf(d.N * d.C1 * d.H * d.W), outbuf(d.Cout * d.C1 * 9), outbuf(36 * d.C1 * d.Cout)
        if case is c43:
            # F(4x4,3x3): an unaligned operand is an argument error
            _rejected(L, 'sg_conv2d_wino_fwd', (dref(d), ptr(x1), ptr(w0), None, ptr(y), 0, 0.0, None, None, ptr(ws), n, s), (y,), '16-byte aligned')
            _rejected(L, 'sg_conv2d_wino_dgrad', (dref(d), ptr(g1), ptr(w0), ptr(gx), None, None, ptr(ws), n, s), (gx,), '16-byte aligned')
            _rejected(L, 'sg_conv2d_wino_wgrad', (dref(d), ptr(g0), ptr(x1), ptr(gw), None, None, ptr(ws), n, s), (gw,), '16-byte aligned')
            _rejected(L, 'sg_conv2d_wino_fwd', (dref(d), ptr(x0), ptr(w0), None, ptr(y[1:]), 0, 0.0, None, None, ptr(ws), n, s), (y,), '16-byte aligned')
            m, r_ = outbuf(d.N * d.Cout), outbuf(d.N * d.Cout)
            _rejected(L, 'sg_conv2d_wino_fwd_instnorm', (dref(d), ptr(x1), ptr(w0), None, None, ptr(y), ptr(gx), ptr(m), ptr(r_), EPS, 0, 0.0, None,
                                                         None, ptr(ws), n, s), (y, gx, m, r_), '16-byte aligned')
        else:
            # saved operands on a desc that cannot use them
            _rejected(L, 'sg_conv2d_wino_fwd', (dref(d), ptr(x0), ptr(w0), None, ptr(y), 0, 0.0, None, ptr(sv), ptr(ws), n, s), (y, sv), 'v_save given')
            _rejected(L, 'sg_conv2d_wino_fwd', (dref(d), ptr(x0), ptr(w0), None, ptr(y), 0, 0.0, ptr(sv), None, ptr(ws), n, s), (y, sv), 'ut_save given')
            _rejected(L, 'sg_conv2d_wino_dgrad', (dref(d), ptr(g0), ptr(w0), ptr(gx), None, ptr(sv), ptr(ws), n, s), (gx, sv), 'ytp_save given')
            _rejected(L, 'sg_conv2d_wino_wgrad', (dref(d), ptr(g0), ptr(x0), ptr(gw), ptr(sv), ptr(sv), ptr(ws), n, s), (gw,), 'saved operands given')
        # workspace one byte too small
        _rejected(L, 'sg_conv2d_wino_fwd', (dref(d), ptr(x0), ptr(w0), None, ptr(y), 0, 0.0, None, None, ptr(ws), n - 1, s), (y,), 'bad arguments')
        _rejected(L, 'sg_conv2d_wino_dgrad', (dref(d), ptr(g0), ptr(w0), ptr(gx), None, None, ptr(ws), n - 1, s), (gx,), 'bad arguments')
        _rejected(L, 'sg_conv2d_wino_wgrad', (dref(d), ptr(g0), ptr(x0), ptr(gw), None, None, ptr(ws), n - 1, s), (gw,), 'bad arguments')
    d = WC.case_desc(c24)
    inp = WC.case_inputs(c24)
    ws, n = wino_ws(L, d, f24=True)
    x0, w0, y = place(inp['x']), place(inp['w']), outbuf(d.N * d.Cout * d.OH * d.OW)
    _rejected(L, 'sg_conv2d_wino24_fwd', (dref(d), ptr(x0), ptr(w0), None, ptr(y), 0, 0.0, ptr(ws), n - 1, s), (y,), 'bad arguments')
    gw = outbuf(d.Cout * d.C1 * 16 + 1)
    _rejected(L, 'sg_conv2d_wino24_wgrad', (dref(d), ptr(place(inp['gy'])), ptr(x0), ptr(gw[1:]), ptr(ws), n, s), (gw,), '16-byte aligned')
    # unsupported descs: 192 channels, a tile count that is no multiple of 128, F(2x2,4x4) under w24_pmin tiles
    big = scratch(1 << 24)
    for dd, fn in ((WC.make_desc(8, 192, 8, 8, 192, 3, 1, 1, True, 1, 8, 8), 'sg_conv2d_wino_fwd'),
                   (WC.make_desc(4, 128, 8, 8, 128, 3, 1, 1, True, 1, 8, 8), 'sg_conv2d_wino_fwd'),
                   (WC.make_desc(2, 128, 12, 12, 128, 4, 1, 1, False, 1, 11, 11), 'sg_conv2d_wino24_fwd')):
        xx = place(np.zeros(dd.N * dd.C1 * dd.H * dd.W, dtype=np.float32))
        ww = place(np.zeros(dd.Cout * dd.C1 * dd.KS * dd.KS, dtype=np.float32))
        yy = outbuf(dd.N * dd.Cout * dd.OH * dd.OW)
        args = (dref(dd), ptr(xx), ptr(ww), None, ptr(yy), 0, 0.0) + ((None, None) if fn == 'sg_conv2d_wino_fwd' else ()) + (ptr(big), 1 << 24, s)
        _rejected(L, fn, args, (yy,), 'unsupported desc')


# =============================================================================================
# autograd wiring
# =============================================================================================
SUBSETS = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]


@pytest.mark.parametrize('name', ('f43_16_128to128_8x8', 'f23z_2_128to128_16x16', 'f24_4_128to128_17x17_p2'))
def test_conv2d_autograd_wiring(L, name):
    """ops.conv2d: every subset of {x, w, b} requiring a gradient gets it, held to the case's criteria; the others get none"""
    from scene_generation_amd import ops
    case = WC.BY_NAME[name]
    r = WC.case_refs(case)
    inp, ref = r['inp'], r['ref']
    note = noter(case['family'] + '_autograd')
    yref, ybound = with_bias(r, inp['b'])
    d = WC.case_desc(case)
    gb64 = ref['gb']
    gbound = WC.gamma(d.N * d.OH * d.OW) * np.abs(inp['gy'].astype(np.float64)).sum(axis=(0, 2, 3))
    for need in SUBSETS:
        x, w, b = [torch.from_numpy(inp[k]).to(DEV).requires_grad_(bool(f)) for k, f in zip(('x', 'w', 'b'), need)]
        y = ops.conv2d(x, w, b, stride=1, pad=case['pad'], reflect=case['reflect'], upsample=case['ups'])
        tag = '%s conv2d need=%s' % (name, need)
        WC.check(y.detach().cpu().numpy(), yref, ybound, r['y_rms32'], tag + ' y', note)
        if any(need):
            y.backward(torch.from_numpy(inp['gy']).to(DEV))
        for t, key, f in ((x, 'gx', need[0]), (w, 'gw', need[1])):
            assert (t.grad is not None) == bool(f), (tag, key)
            if f:
                WC.check(t.grad.cpu().numpy(), ref[key], r[key + '_bound'], r[key + '_rms32'], '%s %s' % (tag, key), note)
        assert (b.grad is not None) == bool(need[2]), tag
        if need[2]:
            WC.check(b.grad.cpu().numpy(), gb64, gbound, 1.0, tag + ' gb', noter('autograd_gb'), rms_line=False)


def test_conv2d_instnorm_autograd_wiring(L):
    """ops.conv2d_instnorm gives, for every subset of {x, w, b} requiring a gradient, the numbers of the C-ABI pair bit for bit"""
    from scene_generation_amd import ops
    case = WC.BY_NAME[WC.FUSED_CASES[0]]
    inp = WC.case_inputs(case)
    want = fused_pair(L, case, 1, 1, noter('F43_fused'))
    for need in SUBSETS:
        x, w, b = [torch.from_numpy(inp[k]).to(DEV).requires_grad_(bool(f)) for k, f in zip(('x', 'w', 'b'), need)]
        out = ops.conv2d_instnorm(x, w, b, skip=torch.from_numpy(want['skip']).to(DEV), eps=EPS, act=1, slope=0.2)
        assert np.array_equal(out.detach().cpu().numpy(), want['out']), need
        if any(need):
            out.backward(torch.from_numpy(want['gout']).to(DEV))
        for t, key, f in ((x, 'gx', need[0]), (w, 'gw', need[1]), (b, 'gb', need[2])):
            assert (t.grad is not None) == bool(f), (need, key)
            if f:
                assert np.array_equal(t.grad.cpu().numpy(), want[key]), 'conv2d_instnorm need=%s: %s differs from the C ABI' % (need, key)
