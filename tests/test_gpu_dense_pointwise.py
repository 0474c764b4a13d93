"""Every dense-layer launch plan (csrc/skinny.hip, the run_dense configurations of csrc/igemm.hip) and every branch of the pooling,
padding and pointwise kernels (csrc/norm.hip, csrc/loss.hip, the fold kernels of csrc/igemm.hip) against a float64 reference of the
same operation.  The cases, their inputs and the references are tests/dense_pointwise_cases.py;
tests/test_dense_pointwise_cases_cpu.py shows that the cases reach every plan and that the references are sound.

Everything goes through the C ABI (ctypes), so gradients, null pointers and offset pointers reach the kernels as given; one test
passes through ops.linear for the autograd wiring.  Sums are held to |got - ref64| <= gamma(n) sum|terms| element by element
(n roundings, u = 2^-24); copies, selections and single products to bit-equality with their fp32 expectation.  The worst error /
bound ratio of every family is written to dense_pointwise_margins.json next to the suite's other calibration records."""
import numpy as np
import pytest
import torch

import dense_pointwise_cases as DP
from gpu_harness import GUARD, Margins, call, margins_fixture, options, outbuf, place, ptr, same, stream, take
from gpu_harness import L, _release_operands  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGINS = Margins()
within, close_noted = MARGINS.within, MARGINS.close_noted
_margins = margins_fixture(lambda: MARGINS.dump('dense_pointwise_margins.json'))      # the worst error / bound ratio per family
ENTRIES = (DP.LINEAR_FWD, DP.LINEAR_BWD_DATA, DP.LINEAR_BWD_WEIGHT)


# =============================================================================================
# dense layers
# =============================================================================================
def run_entry(L, entry, xd, wd, bd, gd, rows, in_f, out_f, act, slope, want_gb):
    """one C-ABI call -> (result, bias gradient or None)"""
    s = stream()
    if entry == DP.LINEAR_FWD:
        o = outbuf(rows * out_f)
        call(L, 'sg_linear_fwd', ptr(xd), ptr(wd), ptr(bd), ptr(o), rows, in_f, out_f, act, slope, s)
        return take(o, (rows, out_f)), None
    if entry == DP.LINEAR_BWD_DATA:
        o = outbuf(rows * in_f)
        call(L, 'sg_linear_bwd_data', ptr(gd), ptr(wd), ptr(o), rows, in_f, out_f, s)
        return take(o, (rows, in_f)), None
    o, ob = outbuf(out_f * in_f), outbuf(out_f) if want_gb else None
    call(L, 'sg_linear_bwd_weight', ptr(gd), ptr(xd), ptr(o), ptr(ob), rows, in_f, out_f, s)
    return take(o, (out_f, in_f)), (take(ob, (out_f,)) if want_gb else None)


def actual_plan(L, entry, xd, wd, gd, rows, in_f, out_f):
    al = lambda t: 16 if t.data_ptr() % 16 == 0 else (8 if t.data_ptr() % 8 == 0 else 4)
    a, b = {DP.LINEAR_FWD: (xd, wd), DP.LINEAR_BWD_DATA: (gd, wd), DP.LINEAR_BWD_WEIGHT: (gd, xd)}[entry]
    return DP.linear_plan(L, entry, rows, in_f, out_f, al(a), al(b))


@pytest.mark.parametrize('case', DP.DENSE_CASES, ids=lambda c: c['name'])
def test_dense_case(L, case):
    rows, in_f, out_f = case['rows'], case['in_f'], case['out_f']
    x, w, b, gy = DP.dense_inputs(case)
    ref = DP.dense_ref(case, x, w, b, gy)
    ox, ow, og = case['offs']
    xd, wd, gd = place(x, ox), place(w, ow), place(gy, og)
    bd = place(b) if case['bias'] else None
    keys = {DP.LINEAR_FWD: 'y', DP.LINEAR_BWD_DATA: 'gx', DP.LINEAR_BWD_WEIGHT: 'gw'}
    results = {}
    for kname, skinny in DP.KERNELS:
        for nsub in DP.NSUB_VALUES:
            with options({'linear_skinny': skinny, 'linear_nsub': nsub}):
                for e in ENTRIES:
                    name = '%s %s %s nsub%d' % (case['name'], DP.ENTRY_NAMES[e], kname, nsub)
                    plan = actual_plan(L, e, xd, wd, gd, rows, in_f, out_f)
                    assert plan == DP.linear_plan(L, e, rows, in_f, out_f, *DP.operand_aligns(e, case)), name
                    assert plan[0] == (DP.LIN_SKINNY if kname == 'skinny' else DP.LIN_TILED), name
                    got, gb = run_entry(L, e, xd, wd, bd, gd, rows, in_f, out_f, case['act'], case['slope'], case['gb'])
                    again, gb2 = run_entry(L, e, xd, wd, bd, gd, rows, in_f, out_f, case['act'], case['slope'], case['gb'])
                    assert np.array_equal(got, again), '%s: a second run differs' % name
                    family = 'dense_%s_%s' % (DP.ENTRY_NAMES[e], kname)
                    if e == DP.LINEAR_FWD and case['act'] in (DP.ACT_TANH, DP.ACT_SIGMOID):
                        family += '_tanh_sigmoid'
                    within(family, got, ref[keys[e]], ref[keys[e] + '_bound'], name)
                    if gb is not None:
                        assert np.array_equal(gb, gb2), '%s: the bias gradient of a second run differs' % name
                        within('dense_bias_grad_' + kname, gb, ref['gb'], ref['gb_bound'], name + ' gb')
                    results[(kname, nsub, e)] = got
    for e in ENTRIES:           # the two kernels agree within the sum of their bounds
        a, t = results[('skinny', 2, e)].astype(np.float64), results[('tiled', 2, e)].astype(np.float64)
        bound = 2.0 * ref[keys[e] + '_bound']
        assert (np.abs(a - t) <= bound).all(), '%s %s: skinny and tiled differ by more than both bounds' % (
            case['name'], DP.ENTRY_NAMES[e])


@pytest.mark.parametrize('k', DP.K_EDGES)
def test_dense_onehot_probe(L, k):
    """the contracted operand is the identity: every k position is read exactly once, so the result is the other operand (plus
    the bias as one fp32 add), bit for bit -- a chunk dropped or added twice at a wave, round or tile boundary is a wrong element"""
    eye = np.eye(k, dtype=np.float32)
    eyed = place(eye)
    rng = DP.rng_of('onehot_%d' % k)
    for e in ENTRIES:
        rows, in_f, out_f = DP.onehot_case(e, k)
        if e == DP.LINEAR_FWD:
            w, b = DP.f32(rng, (out_f, in_f)), DP.f32(rng, (out_f,))
            want = (torch.from_numpy(w).t() + torch.from_numpy(b)).numpy()
            xd, wd, bd, gd = eyed, place(w), place(b), None
        elif e == DP.LINEAR_BWD_DATA:
            w = DP.f32(rng, (out_f, in_f))
            want, xd, wd, bd, gd = w, None, place(w), None, eyed
        else:
            x = DP.f32(rng, (rows, in_f))
            want, xd, wd, bd, gd = x, place(x), None, None, eyed
        for kname, skinny in DP.KERNELS:
            for nsub in DP.NSUB_VALUES:
                with options({'linear_skinny': skinny, 'linear_nsub': nsub}):
                    got, gb = run_entry(L, e, xd, wd, bd, gd, rows, in_f, out_f, DP.ACT_NONE, 0.0, True)
                    same(got, want, 'one-hot K=%d %s %s nsub%d' % (k, DP.ENTRY_NAMES[e], kname, nsub))
                    if gb is not None:
                        same(gb, np.ones(out_f, dtype=np.float32), 'one-hot bias gradient K=%d %s' % (k, kname))


def test_linear_autograd_wiring(L):
    """ops.linear hands x, w, b and the activation-masked gy to the three entry points"""
    from scene_generation_amd import ops
    case = DP.DENSE_BY_NAME['act1_ragged']
    x, w, b, gy = DP.dense_inputs(case)
    ref = DP.dense_ref(case, x, w, b, gy)
    xt, wt, bt = [torch.from_numpy(a).to(DEV).requires_grad_() for a in (x, w, b)]
    y = ops.linear(xt, wt, bt, DP.ACT_RELU, 0.0)
    within('dense_autograd', y.detach().cpu().numpy(), ref['y'], ref['y_bound'], 'ops.linear forward')
    y.backward(torch.from_numpy(gy).to(DEV))
    mask = (y.detach().cpu().numpy() > 0).astype(np.float64)           # the mask of the forward under test
    g = gy.astype(np.float64) * mask
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    within('dense_autograd', xt.grad.cpu().numpy(), g @ w64, DP.gamma(case['out_f'] + 3) * (np.abs(g) @ np.abs(w64)), 'gx')
    within('dense_autograd', wt.grad.cpu().numpy(), g.T @ x64, DP.gamma(case['rows'] + 3) * (np.abs(g).T @ np.abs(x64)), 'gw')
    within('dense_autograd', bt.grad.cpu().numpy(), g.sum(0), DP.gamma(case['rows']) * np.abs(g).sum(0), 'gb')


# =============================================================================================
# pooling
# =============================================================================================
def linear_pair(L, family, taps, name, fwd, bwd, nc, exact_fwd=False, exact_bwd=False, extra_fwd=1, extra_bwd=0, xg=None):
    """a forward / adjoint pair of plane operators against its tap list.  fwd(xd, od) / bwd(gd, od) launch; the bounds are
    gamma(terms + extra) sum|terms| (extra: divisions), or equality for copies"""
    rng = DP.rng_of(family + name)
    x, g = xg if xg is not None else (DP.f32(rng, (nc, taps.n_in)), DP.f32(rng, (nc, taps.n_out)))
    if fwd is not None:
        o = outbuf(nc * taps.n_out)
        fwd(place(x), o)
        got = take(o, (nc, taps.n_out))
        if exact_fwd:
            same(got, taps.fwd(x).astype(np.float32), name + ' forward')
        else:
            within(family + '_fwd', got, taps.fwd(x), DP.gamma(taps.terms_out() + extra_fwd) * taps.abs_().fwd(np.abs(x)), name)
    if bwd is not None:
        o = outbuf(nc * taps.n_in)
        bwd(place(g), o)
        got = take(o, (nc, taps.n_in))
        if exact_bwd:
            same(got, taps.adj(g).astype(np.float32), name + ' adjoint')
        else:
            within(family + '_bwd', got, taps.adj(g), DP.gamma(taps.terms_in() + extra_bwd) * taps.abs_().adj(np.abs(g)), name)


@pytest.mark.parametrize('H,W', DP.AVGPOOL3S2_SHAPES)
def test_avgpool3s2(L, H, W):
    OH, OW, nc = (H - 1) // 2 + 1, (W - 1) // 2 + 1, DP.POOL_NC
    # forward: <= 9 terms and a division; backward: <= 4 quotients (one division and the adds behind it per term)
    linear_pair(L, 'avgpool3s2', DP.taps_avgpool3s2(H, W), '%dx%d' % (H, W),
                lambda xd, o: call(L, 'sg_avgpool3s2_fwd', ptr(xd), ptr(o), nc, H, W, OH, OW, stream()),
                lambda gd, o: call(L, 'sg_avgpool3s2_bwd', ptr(gd), ptr(o), nc, H, W, OH, OW, stream()), nc)


@pytest.mark.parametrize('H,W,k', DP.POOL2D_CASES)
def test_pool2d_avg(L, H, W, k):
    nc = DP.POOL_NC
    linear_pair(L, 'pool2d_avg', DP.taps_avgpool(H, W, k), '%dx%d k%d' % (H, W, k),
                lambda xd, o: call(L, 'sg_pool2d_fwd', ptr(xd), ptr(o), nc, H, W, k, 1, stream()),
                lambda gd, o: call(L, 'sg_pool2d_bwd', None, ptr(gd), ptr(o), nc, H, W, k, 1, stream()), nc)


def _maxpool(L, H, W, k, fwd, bwd, name):
    nc = DP.POOL_NC
    rng = DP.rng_of('gpu_max_' + name)
    x = DP.tie_values(rng, (nc, H, W))
    y, arg = DP.maxpool_ref(x, k)
    gy = DP.f32(rng, y.shape)
    xd = place(x)
    o = outbuf(y.size)
    fwd(xd, o)
    same(take(o, y.shape), y, name + ' forward')
    o = outbuf(x.size)
    bwd(xd, place(gy), o)
    same(take(o, x.shape), DP.maxpool_bwd_ref(arg, gy, H, W), name + ' gradient: the first maximum takes it')


@pytest.mark.parametrize('H,W', DP.MAXPOOL2_SHAPES)
def test_maxpool2(L, H, W):
    nc = DP.POOL_NC
    _maxpool(L, H, W, 2, lambda xd, o: call(L, 'sg_maxpool2_fwd', ptr(xd), ptr(o), nc, H, W, stream()),
             lambda xd, gd, o: call(L, 'sg_maxpool2_bwd', ptr(xd), ptr(gd), ptr(o), nc, H, W, stream()), 'maxpool2 %dx%d' % (H, W))


@pytest.mark.parametrize('H,W,k', DP.POOL2D_CASES)
def test_pool2d_max(L, H, W, k):
    nc = DP.POOL_NC
    _maxpool(L, H, W, k, lambda xd, o: call(L, 'sg_pool2d_fwd', ptr(xd), ptr(o), nc, H, W, k, 0, stream()),
             lambda xd, gd, o: call(L, 'sg_pool2d_bwd', ptr(xd), ptr(gd), ptr(o), nc, H, W, k, 0, stream()),
             'pool2d %dx%d k%d' % (H, W, k))


@pytest.mark.parametrize('NC,HW', DP.GAP_CASES)
def test_gap(L, NC, HW):
    linear_pair(L, 'gap', DP.taps_gap(HW), 'NC%d HW%d' % (NC, HW),
                lambda xd, o: call(L, 'sg_gap_fwd', ptr(xd), ptr(o), NC, HW, stream()),
                lambda gd, o: call(L, 'sg_gap_bwd', ptr(gd), ptr(o), NC, HW, stream()), NC, extra_bwd=0)


# =============================================================================================
# padding, upsampling, copies
# =============================================================================================
@pytest.mark.parametrize('H,W', DP.UPSAMPLE2_SHAPES)
def test_upsample2(L, H, W):
    linear_pair(L, 'upsample2', DP.taps_upsample2(H, W), '%dx%d' % (H, W),
                lambda xd, o: call(L, 'sg_upsample2_fwd', ptr(xd), ptr(o), 3, H, W, stream()), None, 3, exact_fwd=True)


@pytest.mark.parametrize('H,W,pad', DP.REFLECT_PAD_CASES)
def test_reflect_pad(L, H, W, pad):
    linear_pair(L, 'reflect_pad', DP.taps_reflect_pad(H, W, pad), '%dx%d p%d' % (H, W, pad),
                lambda xd, o: call(L, 'sg_reflect_pad_fwd', ptr(xd), ptr(o), 3, H, W, pad, stream()), None, 3, exact_fwd=True)


@pytest.mark.parametrize('H,W,pad', DP.REPLICATE_PAD_CASES)
def test_replicate_pad(L, H, W, pad):
    linear_pair(L, 'replicate_pad', DP.taps_replicate_pad(H, W, pad), '%dx%d p%d' % (H, W, pad),
                lambda xd, o: call(L, 'sg_replicate_pad_fwd', ptr(xd), ptr(o), 3, H, W, pad, stream()),
                lambda gd, o: call(L, 'sg_replicate_pad_bwd', ptr(gd), ptr(o), 3, H, W, pad, stream()), 3, exact_fwd=True)


@pytest.mark.parametrize('NC,H,W,pad,ups', DP.PAD_UPSAMPLE_CASES)
def test_pad_upsample_bwd(L, NC, H, W, pad, ups):
    taps = DP.taps_pad_upsample(H, W, pad, ups)
    rng = DP.rng_of('pu_%d_%d_%d_%d_%d' % (NC, H, W, pad, ups))
    g = DP.f32(rng, (NC, taps.n_out))
    if NC > 100:              # the planes on both sides of a launch boundary must not look alike
        g += np.arange(NC, dtype=np.float32)[:, None] % 7
    linear_pair(L, 'pad_upsample', taps, 'NC%d %dx%d p%d u%d' % (NC, H, W, pad, ups), None,
                lambda gd, o: call(L, 'sg_pad_upsample_bwd', ptr(gd), ptr(o), NC, H, W, pad, ups, stream()), NC, xg=(None, g))


@pytest.mark.parametrize('N,Ca,Cb,HW', DP.CONCAT_CASES)
def test_concat_channels(L, N, Ca, Cb, HW):
    rng = DP.rng_of('concat')
    a, b = DP.f32(rng, (N, Ca, HW)), DP.f32(rng, (N, Cb, HW))
    o = outbuf(N * (Ca + Cb) * HW)
    call(L, 'sg_concat_channels', ptr(place(a)), ptr(place(b)), ptr(o), N, Ca, Cb, HW, stream())
    same(take(o, (N, Ca + Cb, HW)), np.concatenate([a, b], 1), 'concat')


@pytest.mark.parametrize('M,C1,C2,R', DP.COND_SPLIT_CASES)
def test_cond_conv_split_merge(L, M, C1, C2, R):
    taps = DP.taps_cond_split(M, C1, C2, R)
    n1, n = M * C1 * R, taps.n_out
    rng = DP.rng_of('split_%d_%d_%d_%d' % (M, C1, C2, R))
    w, g = DP.f32(rng, (1, taps.n_in)), DP.f32(rng, (1, n))
    o1, o2 = outbuf(n1), outbuf(n - n1)
    call(L, 'sg_cond_conv_split_w', ptr(place(w)), ptr(o1), ptr(o2), M, C1, C2, R, stream())
    same(np.concatenate([take(o1, (n1,)), take(o2, (n - n1,))]), taps.fwd(w)[0].astype(np.float32), 'split')
    g1, g2 = place(g[0, :n1]), place(g[0, n1:])
    for use1, use2 in ((True, True), (False, True), (True, False), (False, False)):       # a null source reads as zeros
        gm = g.copy()
        if not use1:
            gm[0, :n1] = 0
        if not use2:
            gm[0, n1:] = 0
        o = outbuf(taps.n_in)
        call(L, 'sg_cond_conv_merge_w', ptr(g1) if use1 else None, ptr(g2) if use2 else None, ptr(o), M, C1, C2, R, stream())
        same(take(o, (taps.n_in,)), taps.adj(gm)[0].astype(np.float32), 'merge %s %s' % (use1, use2))


@pytest.mark.parametrize('KS', (1, 3, 4))
def test_cond_conv_bias_act_and_window_sums(L, KS):
    for idx, (ks, stride, pad, NM, ohw) in enumerate(c for c in DP.COND_WINDOW_CASES if c[0] == KS):
        OH, OW, H, W = DP.cond_window_geometry(KS, stride, pad, ohw)
        taps = DP.taps_window(OH, OW, H, W, KS, stride, pad)
        name = 'KS%d s%d p%d NM%d %dx%d' % (KS, stride, pad, NM, OH, OW)
        rng = DP.rng_of('window_' + name)
        y, p, g = DP.f32(rng, (NM, OH * OW)), DP.f32(rng, (NM, KS * KS)), DP.f32(rng, (NM, OH * OW))
        act, slope = DP.ACTS[idx % 5], DP.ACT_SLOPES[idx % 2]
        # bias_act, in place: window sum (terms adds), the add of y, the activation
        o = outbuf(NM * OH * OW)
        o[:-1].copy_(torch.from_numpy(y).reshape(-1))
        call(L, 'sg_cond_conv_bias_act', ptr(o), ptr(place(p)), NM, OH, OW, H, W, KS, stride, pad, act, slope, stream())
        pre = y.astype(np.float64) + taps.fwd(p)
        ref = DP.act_ref(pre, act, slope)
        bound = DP.ACT_LIPSCHITZ[act] * DP.gamma(taps.terms_out() + 2) * (np.abs(y) + taps.fwd(np.abs(p)))
        if act in (DP.ACT_TANH, DP.ACT_SIGMOID):
            bound = bound + 1e-6 * np.maximum(1.0, np.abs(ref))
        within('cond_bias_act', take(o, (NM, OH * OW)), ref, bound, name + ' act%d' % act)
        # window sums: every tap the sum of the outputs it reaches
        o = outbuf(NM * KS * KS)
        call(L, 'sg_cond_conv_window_sums', ptr(place(g)), ptr(o), NM, OH, OW, H, W, KS, stride, pad, stream())
        within('cond_window_sums', take(o, (NM, KS * KS)), taps.adj(g), DP.gamma(np.maximum(taps.terms_in(), 1)) * taps.adj(np.abs(g)),
               name)


@pytest.mark.parametrize('Cout,Cin', DP.FOLD_CASES)
def test_upconv3_fold_unfold(L, Cout, Cin):
    taps = DP.taps_upconv3_fold(Cout, Cin)
    rng = DP.rng_of('gpu_fold_%d_%d' % (Cout, Cin))
    w, gwt = DP.f32(rng, (1, taps.n_in)), DP.f32(rng, (1, taps.n_out))
    o = outbuf(taps.n_out)
    call(L, 'sg_upconv3_fold_weights', ptr(place(w)), ptr(o), Cout, Cin, stream())
    within('upconv3_fold', take(o, (1, taps.n_out)), taps.fwd(w), DP.gamma(taps.terms_out()) * taps.fwd(np.abs(w)), 'fold')
    o = outbuf(taps.n_in)
    call(L, 'sg_upconv3_unfold_wgrad', ptr(place(gwt)), ptr(o), Cout, Cin, stream())
    got = take(o, (Cout, Cin, 3, 3))
    same(got, DP.unfold_fp32(gwt, Cout, Cin), 'unfold: (a + b) + (c + d)')
    within('upconv3_unfold', got.reshape(1, -1), taps.adj(gwt), DP.gamma(taps.terms_in()) * taps.adj(np.abs(gwt)), 'unfold')


# =============================================================================================
# pointwise
# =============================================================================================
def _act_fp32(x, act, slope):
    s = np.float32(slope)
    if act == DP.ACT_RELU:
        return np.where(x > 0, x, np.float32(0))
    if act == DP.ACT_LEAKY:
        return np.where(x > 0, x, x * s).astype(np.float32)
    return x


@pytest.mark.parametrize('act', DP.ACTS)
def test_act_fwd_bwd(L, act):
    for slope in DP.ACT_SLOPES:
        for n in DP.ACT_NS:
            name = 'act%d slope %g n%d' % (act, slope, n)
            x, gy = DP.act_inputs(n, 'gpu'), DP.f32(DP.rng_of('actgy%d' % n), (n,))
            o = outbuf(n)
            call(L, 'sg_act_fwd', ptr(place(x)), ptr(o), n, act, slope, stream())
            y = take(o, (n,))
            if n:
                assert np.isfinite(y).all(), name
            if act in (DP.ACT_TANH, DP.ACT_SIGMOID):
                close_noted('act_tanh_sigmoid_fwd', y, DP.act_ref(x, act, slope), 1e-6, name)
                lo = -1.0 if act == DP.ACT_TANH else 0.0
                assert ((y >= lo) & (y <= 1.0)).all(), '%s: outside [%g, 1]' % (name, lo)       # +-90 saturate, finite
            else:
                same(y, _act_fp32(x, act, slope), name)
            yin = DP.act_ref(x, act, slope).astype(np.float32)           # backward from a given OUTPUT
            o = outbuf(n)
            call(L, 'sg_act_bwd', ptr(place(yin)), ptr(place(gy)), ptr(o), n, act, slope, stream())
            gx = take(o, (n,))
            if act in (DP.ACT_TANH, DP.ACT_SIGMOID):
                close_noted('act_tanh_sigmoid_bwd', gx, DP.act_bwd_ref(yin, gy, act, slope), 1e-5, name + ' bwd')
            else:
                d = {DP.ACT_RELU: np.where(yin > 0, 1, 0), DP.ACT_LEAKY: np.where(yin > 0, np.float32(1), np.float32(slope))}.get(
                    act, np.ones(n))
                same(gx, gy * d.astype(np.float32), name + ' bwd')


@pytest.mark.parametrize('n', DP.EWISE_NS)
def test_fill_scale_add_mul(L, n):
    rng = DP.rng_of('ewise%d' % n)
    a, b = DP.f32(rng, (n,)), DP.f32(rng, (n,))
    alpha = np.float32(0.37)
    o = outbuf(n)
    call(L, 'sg_fill', ptr(o), float(alpha), n, stream())
    same(take(o, (n,)), np.full(n, alpha), 'fill')
    o = outbuf(n)
    o[:-1].copy_(torch.from_numpy(a))
    call(L, 'sg_scale', ptr(o), float(alpha), n, stream())
    same(take(o, (n,)), a * alpha, 'scale')
    o = outbuf(n)
    call(L, 'sg_add', ptr(place(a)), ptr(place(b)), ptr(o), n, stream())
    same(take(o, (n,)), a + b, 'add')
    o = outbuf(n)
    call(L, 'sg_mul', ptr(place(a)), ptr(place(b)), float(alpha), ptr(o), n, stream())
    same(take(o, (n,)), (a * b) * alpha, 'mul')


@pytest.mark.parametrize('n,oy,ox', DP.AXPY_CASES)
def test_axpy_and_add_clear(L, n, oy, ox):
    rng = DP.rng_of('axpy_%d_%d_%d' % (n, oy, ox))
    y, x = DP.f32(rng, (n,)), DP.f32(rng, (n,))
    alpha = np.float32(-1.7)
    name = 'n%d y+%d x+%d' % (n, oy, ox)
    y64, x64 = y.astype(np.float64), x.astype(np.float64)
    # y + alpha x may be contracted to an fma: two roundings at most
    yo = outbuf(n, oy)
    yo[:-1].copy_(torch.from_numpy(y))
    xd = place(x, ox)
    call(L, 'sg_axpy', ptr(yo), ptr(xd), float(alpha), n, stream())
    within('axpy', take(yo, (n,)), y64 + np.float64(alpha) * x64, DP.gamma(2) * (np.abs(y64) + np.abs(np.float64(alpha) * x64)), name)
    same(xd.cpu().numpy()[:n], x, 'axpy leaves x alone')
    yo = outbuf(n, oy)
    yo[:-1].copy_(torch.from_numpy(y))
    xo = outbuf(n, ox)
    xo[:-1].copy_(torch.from_numpy(x))
    call(L, 'sg_add_clear', ptr(yo), ptr(xo), n, stream())
    within('add_clear', take(yo, (n,)), y64 + x64, DP.gamma(2) * (np.abs(y64) + np.abs(x64)), name)
    same(take(xo, (n,)), np.zeros(n), 'add_clear leaves x all zero')


def test_zero_length_calls_touch_nothing(L):
    g = torch.full((1,), GUARD, dtype=torch.float32, device=DEV)
    other = torch.full((1,), GUARD, dtype=torch.float32, device=DEV)
    s, p = stream(), ptr(other)
    for rc in (L.sg_act_fwd(ptr(g), ptr(g), 0, DP.ACT_TANH, 0.0, s), L.sg_act_bwd(ptr(g), ptr(g), ptr(g), 0, DP.ACT_RELU, 0.0, s),
               L.sg_fill(ptr(g), 1.0, 0, s), L.sg_scale(ptr(g), 2.0, 0, s), L.sg_add(ptr(g), ptr(g), ptr(g), 0, s),
               L.sg_mul(ptr(g), ptr(g), 2.0, ptr(g), 0, s), L.sg_axpy(ptr(g), p, 2.0, 0, s), L.sg_add_clear(ptr(g), p, 0, s),
               L.sg_pad_upsample_bwd(ptr(g), ptr(g), 0, 4, 4, 1, 1, s), L.sg_pad_upsample_bwd(ptr(g), ptr(g), 3, 0, 4, 1, 2, s),
               L.sg_cond_conv_bias_act(ptr(g), p, 0, 2, 2, 2, 2, 3, 1, 1, DP.ACT_RELU, 0.0, s),
               L.sg_cond_conv_window_sums(p, ptr(g), 0, 2, 2, 2, 2, 3, 1, 1, s)):
        assert rc == 0
    torch.cuda.synchronize()
    assert float(g.cpu()[0]) == GUARD and float(other.cpu()[0]) == GUARD
