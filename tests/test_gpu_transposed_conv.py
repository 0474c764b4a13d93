"""The transposed gathers of csrc/igemm_kn1.hip through the entry points that feed them -- sg_convT2d_fwd / _dgrad / _wgrad,
sg_conv2d_dgrad (channel windows, reflect-padded and upsampled logical grids), sg_conv2d_dgrad_folded and the sub-pixel form
(sg_upconv3_fold_weights / sg_upconv3_unfold_wgrad) -- against a float64 restatement of the same operation.  The cases, their inputs,
the references and the bounds are tests/transposed_conv_cases.py; tests/test_transposed_conv_cases_cpu.py shows that the references
are sound and that the table reaches every launch plan.

Everything goes through the C ABI (ctypes): channel windows, null bias, null gb and offset workspaces reach the kernels as given.
Each case asserts the plan the library reports for it (sg_conv2d_tgather_plan), runs every entry twice (bit-equal) and holds the
result to |got - ref64| <= gamma(n + c) sum|a||b| element by element; one-hot probes -- the index logic -- and the weight fold are
held to bit equality.  The worst error / bound ratio of every family goes to transposed_conv_margins.json."""
import numpy as np
import pytest
import torch

import transposed_conv_cases as T
from gpu_harness import GUARD, Margins, call, dref, margins_fixture, opt_tag, options, outbuf, place, ptr, same, scratch, stream, take, twice
from gpu_harness import L, _release_operands  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGINS = Margins()
within = MARGINS.within
_margins = margins_fixture(lambda: MARGINS.dump('transposed_conv_margins.json'))      # the worst error / bound ratio per family


def conv_ws(L, d, kind, off=0):
    n = int(L.sg_conv2d_ws_bytes(dref(d), kind))
    return scratch(n, off), n


# ---- the entry points, one C-ABI call each ---------------------------------------------------------------------------
def convT_fwd(L, d, xd, wd, bd, off=0):
    ws, n = conv_ws(L, d, 0, off)
    o = outbuf(d.N * d.Cout * d.OH * d.OW)
    call(L, 'sg_convT2d_fwd', dref(d), ptr(xd), ptr(wd), ptr(bd), ptr(o), ptr(ws), n, stream())
    return take(o, (d.N, d.Cout, d.OH, d.OW)), ws


def convT_dgrad(L, d, gd, wd):
    ws, n = conv_ws(L, d, 1)
    o = outbuf(d.N * d.C1 * d.H * d.W)
    call(L, 'sg_convT2d_dgrad', dref(d), ptr(gd), ptr(wd), ptr(o), ptr(ws), n, stream())
    return take(o, (d.N, d.C1, d.H, d.W))


def convT_wgrad(L, d, gd, xd, want_gb):
    ws, n = conv_ws(L, d, 2)
    o, ob = outbuf(d.C1 * d.Cout * d.KS * d.KS), (outbuf(d.Cout) if want_gb else None)
    call(L, 'sg_convT2d_wgrad', dref(d), ptr(gd), ptr(xd), ptr(o), ptr(ob), ptr(ws), n, stream())
    # the plan the library reports for this launch (sg_conv2d_wgrad_plan; tests/wgrad_cases.py restates it): the GEMM runs with the
    # roles swapped -- rows = the input channels, the gathered operand = gy over the input grid -- and hands no bias gradient over
    import wgrad_cases as WG
    got = WG.wgrad_plan(L, d, WG.WG_CONVT, 0, xd.data_ptr() % 16, n)
    want = WG.py_plan(WG.WG_CONVT, d.N, d.Cout, 0, d.OH, d.OW, d.C1, d.KS, d.stride, d.pad, 0, 1, d.H, d.W, a_mod16=xd.data_ptr() % 16,
                      ws_bytes=n, xcd=_hip_option('wgrad_xcd'))
    assert got == want and got['rowsum_fused'] == 0 and got['ws_needed'] <= n, (got, want, n)
    return take(o, (d.C1, d.Cout, d.KS, d.KS)), (take(ob, (d.Cout,)) if want_gb else None)


def _hip_option(name):
    from scene_generation_amd import _hip
    return _hip.get_option(name)


def logical_grid(d):
    return (d.H * d.upsample + (2 * d.pad if d.pad_reflect else 0), d.W * d.upsample + (2 * d.pad if d.pad_reflect else 0))


def conv_dgrad(L, d, gd, wd, c0, c1, off=0):
    """-> (gradient on the logical grid, the same folded onto the stored input as ops/conv.py composes it or None, workspace)"""
    ws, n = conv_ws(L, d, 1, off)
    GH, GW = logical_grid(d)
    o = outbuf(d.N * (c1 - c0) * GH * GW)
    call(L, 'sg_conv2d_dgrad', dref(d), ptr(gd), ptr(wd), ptr(o), c0, c1, ptr(ws), n, stream())
    g, gx = take(o, (d.N, c1 - c0, GH, GW)), None
    if d.pad_reflect or d.upsample == 2:
        o2 = outbuf(d.N * (c1 - c0) * d.H * d.W)
        call(L, 'sg_pad_upsample_bwd', ptr(o[:-1]), ptr(o2), d.N * (c1 - c0), d.H, d.W, d.pad if d.pad_reflect else 0, d.upsample, stream())
        gx = take(o2, (d.N, c1 - c0, d.H, d.W))
    return g, gx, ws


def dgrad_folded(L, d, gd, wd, c0, c1, off=0):
    n = int(L.sg_conv2d_dgrad_folded_ws_bytes(dref(d)))
    assert n > 0 and L.sg_conv2d_dgrad_folded_supported(dref(d)) == 1
    ws = scratch(n, off)
    o = outbuf(d.N * (c1 - c0) * d.H * d.W)
    call(L, 'sg_conv2d_dgrad_folded', dref(d), ptr(gd), ptr(wd), ptr(o), c0, c1, ptr(ws), n, stream())
    return take(o, (d.N, c1 - c0, d.H, d.W)), ws


def assert_plan(L, case, d, entry, c0, c1, ws, name):
    """the plan the library reports for THIS launch (the address of its workspace) is the plan the table claims"""
    _, want = T.case_expected_plan(case)
    got = T.tgather_plan(L, d, entry, c0, c1, ws.data_ptr() % 16)
    for k, v in want.items():
        assert got[k] == v, '%s: plan field %s is %s, the table claims %s (%s)' % (name, k, got[k], v, got)


# =============================================================================================
# the case table
# =============================================================================================
@pytest.mark.parametrize('case', T.CONVT_CASES, ids=lambda c: c['name'])
def test_convT_case(L, case):
    entry, d, c0, c1 = T.case_desc(case)
    inp = T.case_inputs(case)
    ref = T.convT_refs(case, inp)
    xd, wd, gd = place(inp['x']), place(inp['w']), place(inp['gy'])
    bd = place(inp['b']) if case['bias'] else None
    for o in T.case_options(case):
        with options(o):
            name = '%s [%s]' % (case['name'], opt_tag(o))
            y, ws = twice(lambda: convT_fwd(L, d, xd, wd, bd, case['ws_off']), name + ' fwd')
            assert_plan(L, case, d, entry, c0, c1, ws, name)
            within('convT_fwd_%s' % ('parity' if d.stride == 2 and d.KS >= 3 else 'plain'), y, ref['y'], ref['y_bound'], name + ' y')
            gx, = twice(lambda: (convT_dgrad(L, d, gd, wd),), name + ' dgrad')
            within('convT_dgrad', gx, ref['gx'], ref['gx_bound'], name + ' gx')
            gw, gb = twice(lambda: convT_wgrad(L, d, gd, xd, case['bias']), name + ' wgrad')
            within('convT_wgrad', gw, ref['gw'], ref['gw_bound'], name + ' gw')
            if gb is not None:
                within('convT_bias_grad', gb, ref['gb'], ref['gb_bound'], name + ' gb')


@pytest.mark.parametrize('case', T.DGRAD_CASES, ids=lambda c: c['name'])
def test_conv_dgrad_case(L, case):
    entry, d, c0, c1 = T.case_desc(case)
    inp = T.case_inputs(case)
    ref = T.dgrad_refs(case, inp)
    wd, gd = place(inp['w']), place(inp['gy'])
    for o in T.case_options(case):
        with options(o):
            name = '%s [%s]' % (case['name'], opt_tag(o))
            g, gx, ws = twice(lambda: conv_dgrad(L, d, gd, wd, c0, c1, case['ws_off']), name)
            assert_plan(L, case, d, entry, c0, c1, ws, name)
            within('conv_dgrad_%s' % ('parity' if d.stride == 2 and d.KS >= 3 else 'plain'), g, ref['g'], ref['g_bound'], name + ' g')
            if gx is not None:
                within('conv_dgrad_pad_upsample_bwd', gx, ref['gx'], ref['gx_bound'], name + ' gx')


@pytest.mark.parametrize('case', T.FOLDED_CASES, ids=lambda c: c['name'])
def test_dgrad_folded_case(L, case):
    entry, d, c0, c1 = T.case_desc(case)
    inp = T.case_inputs(case)
    ref, bound = T.folded_refs(case, inp)
    wd, gd = place(inp['w']), place(inp['gy'])
    for o in T.case_options(case):
        with options(o):
            name = '%s [%s]' % (case['name'], opt_tag(o))
            gx, ws = twice(lambda: dgrad_folded(L, d, gd, wd, c0, c1, case['ws_off']), name)
            assert_plan(L, case, d, entry, c0, c1, ws, name)
            within('dgrad_folded', gx, ref, bound, name)


@pytest.mark.parametrize('cin,cout', T.SUBPIXEL_FOLD_CHANNELS)
def test_weight_fold_and_unfold(L, cin, cout):
    """both kernels add in a fixed, documented order: bit equality with the same order in fp32 (the corner taps are pure copies)"""
    rng = T.rng_of('gpu_fold_%d_%d' % (cin, cout))
    w, gwt = T.f32(rng, (cout, cin, 3, 3)), T.f32(rng, (cin, cout, 4, 4))
    o = outbuf(cin * cout * 16)
    call(L, 'sg_upconv3_fold_weights', ptr(place(w)), ptr(o), cout, cin, stream())
    same(take(o, (cin, cout, 4, 4)), T.upconv3_fold(w), 'fold %d -> %d' % (cin, cout))
    o = outbuf(cout * cin * 9)
    call(L, 'sg_upconv3_unfold_wgrad', ptr(place(gwt)), ptr(o), cout, cin, stream())
    same(take(o, (cout, cin, 3, 3)), T.upconv3_unfold(gwt), 'unfold %d -> %d' % (cin, cout))


@pytest.mark.parametrize('case', T.SUBPIXEL_CASES, ids=lambda c: c['name'])
def test_subpixel_case(L, case):
    """conv3x3(pad 1)(nearest_up2(x)) composed as ops/conv.py composes it: fold, transposed conv (k4, s2, p1), unfold"""
    entry, d, c0, c1 = T.case_desc(case)
    inp = T.case_inputs(case)
    ref = T.subpixel_refs(case, inp)
    xd, wd, gd = place(inp['x']), place(inp['w']), place(inp['gy'])
    bd = place(inp['b']) if case['bias'] else None
    wt = outbuf(d.C1 * d.Cout * 16)
    call(L, 'sg_upconv3_fold_weights', ptr(wd), ptr(wt), d.Cout, d.C1, stream())
    take(wt, (d.C1, d.Cout, 4, 4))
    wtd = wt[:-1]
    for o in T.case_options(case):
        with options(o):
            name = '%s [%s]' % (case['name'], opt_tag(o))
            y, ws = twice(lambda: convT_fwd(L, d, xd, wtd, bd), name + ' fwd')
            assert_plan(L, case, d, entry, c0, c1, ws, name)
            within('subpixel_fwd', y, ref['y'], ref['y_bound'], name + ' y')
            within('subpixel_dgrad', convT_dgrad(L, d, gd, wtd), ref['gx'], ref['gx_bound'], name + ' gx')
            ws2, n = conv_ws(L, d, 2)
            gwt, ob = outbuf(d.C1 * d.Cout * 16), (outbuf(d.Cout) if case['bias'] else None)
            call(L, 'sg_convT2d_wgrad', dref(d), ptr(gd), ptr(xd), ptr(gwt), ptr(ob), ptr(ws2), n, stream())
            take(gwt, (d.C1, d.Cout, 4, 4))
            gw = outbuf(d.Cout * d.C1 * 9)
            call(L, 'sg_upconv3_unfold_wgrad', ptr(gwt[:-1]), ptr(gw), d.Cout, d.C1, stream())
            within('subpixel_wgrad', take(gw, (d.Cout, d.C1, 3, 3)), ref['gw'], ref['gw_bound'], name + ' gw')
            if ob is not None:
                within('convT_bias_grad', take(ob, (d.Cout,)), ref['gb'], ref['gb_bound'], name + ' gb')


# =============================================================================================
# one-hot probes: the index logic, bit for bit
# =============================================================================================
@pytest.mark.parametrize('case', T.PROBE_CONVT, ids=lambda c: c['name'])
def test_convT_onehot_probe(L, case):
    """x (forward, weight gradient) or gy (data gradient) is a single 1.0: the result is a placed copy of taps of the other operand
    (plus the bias as one fp32 add); every position no tap reaches is exactly 0 (or the bias)"""
    entry, d, c0, c1 = T.case_desc(case)
    s, p, op = case['stride'], case['pad'], case['out_pad']
    inp = T.case_inputs(case)
    wd, gd = place(inp['w']), place(inp['gy'])
    bd = place(inp['b']) if case['bias'] else None
    for o in T.case_options(case):
        with options(o):
            for site in T.probe_sites(d.N, d.C1, d.H, d.W):
                name = '%s [%s] one-hot x at %s' % (case['name'], opt_tag(o), site)
                x1 = T.onehot((d.N, d.C1, d.H, d.W), *site)
                x1d = place(x1)
                same(convT_fwd(L, d, x1d, wd, bd, case['ws_off'])[0], T.place_convT_fwd(site, x1.shape, inp['w'], inp['b'], s, p, op), name + ' y')
                gw, gb = convT_wgrad(L, d, gd, x1d, False)
                same(gw, T.place_convT_wgrad(site, inp['gy'], d.C1, d.KS, s, p), name + ' gw')
            for site in T.probe_sites(d.N, d.Cout, d.OH, d.OW):
                name = '%s [%s] one-hot gy at %s' % (case['name'], opt_tag(o), site)
                g1 = T.onehot((d.N, d.Cout, d.OH, d.OW), *site)
                same(convT_dgrad(L, d, place(g1), wd), T.place_convT_dgrad(site, g1.shape, inp['w'], s, p, d.H, d.W), name + ' gx')
                if case['bias']:
                    gw, gb = convT_wgrad(L, d, place(g1), place(inp['x']), True)
                    want = np.zeros(d.Cout, dtype=np.float32)
                    want[site[1]] = 1.0
                    same(gb, want, name + ' gb')


@pytest.mark.parametrize('case', T.PROBE_DGRAD, ids=lambda c: c['name'])
def test_conv_dgrad_onehot_probe(L, case):
    """gy is a single 1.0 at (n, co, oh, ow): the window's rows of w[co] land at (oh*s - p + kh, ow*s - p + kw), everything else is 0"""
    entry, d, c0, c1 = T.case_desc(case)
    inp = T.case_inputs(case)
    wd = place(inp['w'])
    pz = 0 if case['reflect'] else case['pad']
    GH, GW = logical_grid(d)
    for o in T.case_options(case):
        with options(o):
            for site in T.probe_sites(d.N, d.Cout, d.OH, d.OW):
                name = '%s [%s] one-hot gy at %s' % (case['name'], opt_tag(o), site)
                g1 = T.onehot((d.N, d.Cout, d.OH, d.OW), *site)
                g, gx, _ = conv_dgrad(L, d, place(g1), wd, c0, c1, case['ws_off'])
                same(g, T.place_conv_dgrad(site, g1.shape, inp['w'], d.stride, pz, GH, GW, c0, c1), name)


@pytest.mark.parametrize('case', T.PROBE_FOLDED, ids=lambda c: c['name'])
def test_dgrad_folded_onehot_probe(L, case):
    """w is a single 1.0 at (co, c, kh, kw): channel c of the result is the pre-folded copy kh*3+kw of gy[:, co], shifted by the tap
    (reflect_variants_kernel's sums in its own order, in fp32), every other channel 0.  gy a single 1.0: positions one term reaches
    hold that tap of w bit for bit, positions reached by the reflection too hold the sum of two or four taps within the bound."""
    entry, d, c0, c1 = T.case_desc(case)
    inp = T.case_inputs(case)
    gd = place(inp['gy'])
    for i, (kh, kw) in enumerate((a, b) for a in range(3) for b in range(3)):
        co, c = (0, d.Cout - 1)[i % 2], (c0, c1 - 1)[(i // 2) % 2]
        w1 = np.zeros((d.Cout, d.C1, 3, 3), dtype=np.float32)
        w1[co, c, kh, kw] = 1.0
        got, _ = dgrad_folded(L, d, gd, place(w1), c0, c1)
        same(got, T.place_dgrad_folded_tap(inp['gy'], co, c - c0, kh, kw, c1 - c0), '%s one-hot w at %s' % (case['name'], (co, c, kh, kw)))
    wd = place(inp['w'])
    for site in T.probe_sites(d.N, d.Cout, d.OH, d.OW):
        name = '%s one-hot gy at %s' % (case['name'], site)
        g1 = T.onehot((d.N, d.Cout, d.OH, d.OW), *site)
        got, _ = dgrad_folded(L, d, place(g1), wd, c0, c1)
        cnt = T.conv_dgrad_folded(g1.astype(np.float64), np.ones_like(inp['w'], dtype=np.float64), d.H, d.W, c0, c1)
        ref, bound = T.folded_refs(case, dict(gy=g1, w=inp['w']))
        single = cnt <= 1
        same(np.where(single, got, 0), np.where(single, ref, 0).astype(np.float32), name + ' (single taps)')
        within('dgrad_folded_onehot_sums', np.where(single, 0, got), np.where(single, 0, ref), np.where(single, 0, bound), name + ' (reflected sums)')


# =============================================================================================
# autograd wiring, argument checks
# =============================================================================================
WIRING = ('convT_k4s2p1_16to16', 'convT_k7s2p3_16to16', 'convT_k1s2op1_16to16', 'convT_k3s1p1_16to48_4x17x19', 'convT_k3s2p0op0_5x7_6to10')


@pytest.mark.parametrize('name', WIRING)
def test_conv_transpose2d_autograd_wiring(L, name):
    """ops.conv_transpose2d and layers.ConvTranspose2d hand x, w, b and gy to the three entry points; a backward that wants only
    x, only the weight or only the bias computes that one (the bias alone: sg_channel_sum)"""
    from scene_generation_amd import layers, ops
    case = T.BY_NAME[name]
    s, p, op = case['stride'], case['pad'], case['out_pad']
    inp = T.case_inputs(case)
    if inp['b'] is None:
        inp['b'] = T.f32(T.rng_of(name + '/b'), (case['Cout'],))
        case = dict(case, bias=True)
    ref = T.convT_refs(case, inp)
    gy = torch.from_numpy(inp['gy']).to(DEV)
    for want in ('x', 'w', 'b', 'xwb', 'none_bias'):
        x, w, b = [torch.from_numpy(inp[k]).to(DEV) for k in ('x', 'w', 'b')]
        x.requires_grad_('x' in want)
        w.requires_grad_('w' in want and want != 'none_bias')
        b.requires_grad_('b' in want and want != 'none_bias')
        if want == 'none_bias':           # no bias at all, through the layer
            m = layers.ConvTranspose2d(case['Cin'], case['Cout'], case['KS'], stride=s, padding=p, output_padding=op, bias=False).to(DEV)
            with torch.no_grad():
                m.weight.copy_(w)
            y = m(x.requires_grad_())
            r0, b0 = T._with_bound(lambda x_, w_: T.convT_fwd(x_, w_, None, s, p, op), T.C_GATHER, (inp['x'], inp['w']))
            within('convT_autograd', y.detach().cpu().numpy(), r0, b0, name + ' layer without bias')
            y.backward(gy)
            within('convT_autograd', x.grad.cpu().numpy(), ref['gx'], ref['gx_bound'], name + ' layer gx')
            within('convT_autograd', m.weight.grad.cpu().numpy(), ref['gw'], ref['gw_bound'], name + ' layer gw')
            continue
        y = ops.conv_transpose2d(x, w, b, stride=s, pad=p, out_pad=op)
        within('convT_autograd', y.detach().cpu().numpy(), ref['y'], ref['y_bound'], '%s y (%s)' % (name, want))
        y.backward(gy)
        for k, t, key in (('x', x, 'gx'), ('w', w, 'gw'), ('b', b, 'gb')):
            if k in want:
                within('convT_autograd', t.grad.cpu().numpy(), ref[key], ref[key + '_bound'], '%s %s (%s)' % (name, key, want))
            else:
                assert t.grad is None, (name, want, k)


def test_convT_entries_reject_what_the_forward_rejects(L):
    """a second source, a folded upsample or reflection padding have no meaning for a transposed conv: all three entry points refuse
    them before launching anything"""
    N, C, Co, H, W = 1, 4, 4, 3, 3
    x, w, gy = place(np.zeros((N, C, H, W))), place(np.zeros((C, Co, 3, 3))), place(np.zeros((N, Co, H, W)))
    for kw in (dict(C2=2), dict(ups=2), dict(reflect=True)):
        d = T.make_desc(N, C, H, W, Co, 3, 1, 1, kw.get('reflect', False), kw.get('ups', 1), H, W, 0, C2=kw.get('C2', 0))
        ws = scratch(1 << 20)
        o = outbuf(4096)
        for fn, args in (('sg_convT2d_fwd', (ptr(x), ptr(w), None, ptr(o), ptr(ws), 1 << 20, stream())),
                         ('sg_convT2d_dgrad', (ptr(gy), ptr(w), ptr(o), ptr(ws), 1 << 20, stream())),
                         ('sg_convT2d_wgrad', (ptr(gy), ptr(x), ptr(o), None, ptr(ws), 1 << 20, stream()))):
            rc = getattr(L, fn)(dref(d), *args)
            assert rc != 0, '%s accepted %s' % (fn, kw)
            assert L.sg_last_error_string().decode() == '%s: unsupported desc' % fn
        take(o, (4096,))
        assert (o[:-1] == GUARD).all(), 'a rejected call wrote its output'
