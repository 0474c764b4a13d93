"""The object-accuracy classifier on the GPU (csrc/classifier.hip, ops/classifier.py, scene_generation_amd/accuracy.py).

Exact kernels (max-pool, relu(a + b), SGD, classify record) are compared bit for bit with the NumPy restatements of
tests/accuracy_ref.py.  Float sums (convolutions, blocks, whole networks) are compared with a float64 CPU run of the plain
torch.nn restatement; the bound is FACTOR = 16 times the error torch's own float32 CPU run of the same restatement makes on the same
inputs (never below 2^-24 of the tensor's largest magnitude: half a spacing, what rounding the float64 reference to float32 costs).
Errors are max |a - ref| / max |ref| per tensor.  The worst ratio per family goes to accuracy_margins.json in the suite's output
directory.  The tree only: no reference checkout."""
import copy
import random

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import accuracy_ref as R
import sampling_helpers as SH
from gpu_harness import Margins, N, margins_fixture
from conftest import skip_random_init
from scene_generation_amd import accuracy as A
from scene_generation_amd import ops, sample
from scene_generation_amd.model import Model
from scene_generation_amd.optim import FusedSGD
from scene_generation_amd.synthetic import make_batch, make_sampling_vocab

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 16.0
FACTORS = {'fold': 8.0, 'sgd_steps': 8.0}                     # families whose factor is halved (worst observed ratio under 1/8 of 16: profiles/accuracy_test_margins.md)
FLOOR = 2.0 ** -24
MARGINS = Margins()
_write_margins = margins_fixture(lambda: MARGINS.dump_yardstick('accuracy_margins.json', FACTORS, FACTOR))
CLS_KINDS = ('maxpool3s2', 'add_relu', 'bn_fold', 'sgd', 'classify_stats')


@pytest.fixture(scope='module', autouse=True)
def _fold_on():
    """the eval fast path is what this module tests: switched on for its tests whatever the shipped default, restored afterwards"""
    keep, A.ResNet.fold_batchnorm = A.ResNet.fold_batchnorm, True
    yield
    A.ResNet.fold_batchnorm = keep


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def offset_copy(a, off=1):
    """a device copy of ``a`` that starts ``off`` elements into its allocation (4 bytes past a 16-byte boundary for fp32) and is
    followed by one guard element -> (view, whole buffer, guard value)"""
    a = np.ascontiguousarray(a)
    guard = np.array(-777, a.dtype)
    buf = torch.from_numpy(np.concatenate([np.full(off, guard, a.dtype), a.reshape(-1), np.full(1, guard, a.dtype)])).to(DEV)
    return buf[off:off + a.size].view(a.shape), buf, guard


def check(family, name, got, ref64, ref32):
    """|got - ref64| <= factor * max(|ref32 - ref64|, 2^-24 max|ref64|), in max norm over the tensor; factor = the family's"""
    MARGINS.yardstick(family, name, got, ref64, ref32, FACTORS, FACTOR, FLOOR)


# =====================================================================================================================================
# 1. kernels through the C ABI
# =====================================================================================================================================
def _pool_inputs(H, W, NC, kind, rs):
    x = rs.randn(NC, H, W).astype(np.float32)
    if kind == 'negative':
        x = -np.abs(x) - 1
    elif kind == 'ties':
        x = np.round(x).astype(np.float32)
    elif kind == 'nan':
        x[0, H // 2, W // 2] = np.nan
        x[-1, 0, 0] = np.nan
        x[NC // 2, H - 1, W - 1] = np.nan
    return x


@pytest.mark.parametrize('NC', [1, 130])
@pytest.mark.parametrize('HW', [(1, 1), (2, 3), (7, 7), (8, 5), (13, 14)])
def test_maxpool3s2_kernels(HW, NC):
    H, W = HW
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rs = np.random.RandomState(H * 100 + W + NC)
    for kind in ('random', 'negative', 'ties', 'nan'):
        x = _pool_inputs(H, W, NC, kind, rs)
        gy = rs.randn(NC, OH, OW).astype(np.float32)
        want_y, want_gx = R.maxpool3s2_ref(x), R.maxpool3s2_bwd_ref(x, gy)
        if kind == 'negative':
            assert (want_y < 0).all()
        for off in (0, 1):                                   # aligned and offset base pointers; a guard word behind every output
            tx, _, _ = offset_copy(x, off)
            tgy, _, _ = offset_copy(gy, off)
            outs = []
            for _ in range(2):
                y, ybuf, g = offset_copy(np.zeros((NC, OH, OW), np.float32), off)
                gx, gbuf, _ = offset_copy(np.zeros((NC, H, W), np.float32), off)
                ops._call('sg_maxpool3s2_fwd', tx.data_ptr(), y.data_ptr(), NC, H, W, OH, OW, ops._stream())
                ops._call('sg_maxpool3s2_bwd', tx.data_ptr(), tgy.data_ptr(), gx.data_ptr(), NC, H, W, OH, OW, ops._stream())
                assert float(ybuf[-1]) == g and float(gbuf[-1]) == g and (off == 0 or (float(ybuf[0]) == g and float(gbuf[0]) == g))
                outs.append((N(y), N(gx)))
            assert np.array_equal(outs[0][0], want_y, equal_nan=True), (kind, off)
            assert np.array_equal(outs[0][1], want_gx, equal_nan=True), (kind, off)
            assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()


def test_maxpool3s2_autograd_and_module():
    from scene_generation_amd import layers
    rs = np.random.RandomState(3)
    x = rs.randn(2, 5, 9, 12).astype(np.float32)
    tx = T(x).requires_grad_(True)
    y = layers.MaxPool3s2()(tx)
    cx = torch.from_numpy(x).requires_grad_(True)
    cy = F.max_pool2d(cx, 3, stride=2, padding=1)
    g = torch.from_numpy(rs.randn(*cy.shape).astype(np.float32))
    y.backward(g.to(DEV))
    cy.backward(g)
    assert torch.equal(y.cpu(), cy) and torch.equal(tx.grad.cpu(), cx.grad)
    with pytest.raises(NotImplementedError):
        layers.MaxPool2d(3, stride=2)                        # the general module keeps refusing stride != kernel


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1027])
def test_add_relu_kernel(n):
    rs = np.random.RandomState(n)
    a, b = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    if n > 2:
        a[1], b[2] = np.nan, -0.0
        a[2] = 0.0
    want = R.add_relu_ref(a, b)
    for off in (0, 1):
        ta, _, _ = offset_copy(a, off)
        tb, _, _ = offset_copy(b, off)
        res = []
        for _ in range(2):
            y, ybuf, g = offset_copy(np.full(n, 5, np.float32), off)
            ops._call('sg_add_relu_fwd', ta.data_ptr(), tb.data_ptr(), y.data_ptr(), n, ops._stream())
            assert float(ybuf[-1]) == g
            res.append(N(y))
        assert np.array_equal(res[0], want, equal_nan=True), off
        assert res[0].tobytes() == res[1].tobytes()
    # autograd: one relu mask, the gradient of both operands
    ta, tb = T(a).requires_grad_(True), T(b).requires_grad_(True)
    y = ops.add_relu(ta, tb)
    gy = T(rs.randn(n).astype(np.float32))
    y.backward(gy)
    mask = torch.from_numpy((want > 0).astype(np.float32))
    assert torch.equal(ta.grad.cpu(), gy.cpu() * mask) and torch.equal(tb.grad.cpu(), ta.grad.cpu())


@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (5, 3, 7, 7), (64, 33, 3, 3), (130, 256, 1, 1)])
def test_bn_fold_kernel(shape):
    """against float64: w' is one product of w with s = gamma / sqrt(var + eps) (three roundings: sum, root / quotient, product), b' a
    product and a difference; bound 4 spacings of the result's largest operand (2^-21 relative)"""
    rs = np.random.RandomState(shape[0])
    Cout = shape[0]
    w = rs.randn(*shape).astype(np.float32)
    gamma, beta, mean = [rs.randn(Cout).astype(np.float32) for _ in range(3)]
    var = (rs.rand(Cout) + 0.05).astype(np.float32)
    want_w, want_b = R.bn_fold_ref(w, gamma, beta, mean, var, 1e-5)
    res = []
    for _ in range(2):
        gw, gb = ops.bn_fold(T(w), T(gamma), T(beta), T(mean), T(var), 1e-5)
        res.append((N(gw), N(gb)))
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()
    s = np.abs(gamma.astype(np.float64)) / np.sqrt(var.astype(np.float64) + 1e-5)
    ew = np.abs(res[0][0] - want_w) / np.maximum(np.abs(want_w), 1e-30)
    eb = np.abs(res[0][1] - want_b) / np.maximum(np.maximum(np.abs(beta), np.abs(mean) * s), 1e-30)
    print('bn_fold %s: w %.2e b %.2e (bound %.2e)' % (shape, ew.max(), eb.max(), 2.0 ** -21))
    assert ew.max() <= 2.0 ** -21 and eb.max() <= 2.0 ** -21


def _ulps_of_operands(a, b, scale):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float((d / np.spacing(np.maximum(np.abs(scale), np.float32(1e-30)).astype(np.float32)).astype(np.float64)).max())


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1027])
def test_sgd_kernel(n):
    """bit-equal to the separately rounded fp32 restatement over first and later steps, grad_scale != 1 and a changed lr; three plain
    steps within 2 ulp of torch.optim.SGD on the CPU.  DEVIATION from "within 2 ulp" read as spacings of the RESULT: the ulp is
    the spacing at the largest of |p|, |lr * buf| and |p - lr * buf|, per step, each step starting from torch's own state.
    p - lr * buf cancels, and torch's CPU kernel fuses the product into the subtraction, so its result differs from any separately
    rounded step by up to hundreds of spacings of a small result (212 observed at n = 1027) and by at most one spacing of the
    operands.  The bit-equal comparison above is the sharp check."""
    rs = np.random.RandomState(n)
    p0 = rs.randn(n).astype(np.float32)
    for off in (0, 1):
        p, pbuf, g0 = offset_copy(p0, off)
        buf, bbuf, _ = offset_copy(np.full(n, 123.0, np.float32), off)     # stale values: the first step must not read them
        rp, rb = p0.copy(), np.zeros(n, np.float32)
        for step, (lr, scale) in enumerate([(0.05, 1.0), (0.05, 0.25), (0.005, 1.0), (0.005, 3.0)]):
            g = rs.randn(n).astype(np.float32)
            tg, _, _ = offset_copy(g, off)
            ops._call('sg_sgd_momentum_step', p.data_ptr(), tg.data_ptr(), buf.data_ptr(), n, lr, 0.9, 1 if step == 0 else 0, scale,
                      ops._stream())
            rp, rb = R.sgd_ref(rp, g, rb, lr, 0.9, step == 0, scale)
            assert N(p).tobytes() == rp.tobytes() and N(buf).tobytes() == rb.tobytes(), (off, step)
            assert float(pbuf[-1]) == g0 and float(bbuf[-1]) == g0
    # against torch.optim.SGD, one step at a time from torch's own state
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([tp], lr=0.05, momentum=0.9)
    worst = 0.0
    for step in range(3):
        g = rs.randn(n).astype(np.float32)
        p_before = tp.detach().numpy().copy()
        b_before = opt.state[tp]['momentum_buffer'].numpy().copy() if step else np.zeros(n, np.float32)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, buf = T(p_before), T(b_before)
        ops.sgd_momentum_step(p, T(g), buf, 0.05, 0.9, step == 0)
        assert np.array_equal(N(buf), opt.state[tp]['momentum_buffer'].numpy())
        scale = np.maximum(np.maximum(np.abs(p_before), np.abs(np.float32(0.05) * N(buf))), np.abs(N(p)))
        worst = max(worst, _ulps_of_operands(N(p), tp.detach().numpy(), scale))
    print('n=%d: %.2f ulp from torch.optim.SGD' % (n, worst))
    assert worst <= 2


@pytest.mark.parametrize('classes', [1, 2, 172, 1000])
@pytest.mark.parametrize('rows', [1, 3, 257])
def test_classify_stats_kernel(rows, classes):
    rs = np.random.RandomState(rows * 1000 + classes)
    logits = rs.randn(rows, classes).astype(np.float32)
    if classes > 1:
        logits[0, :] = np.round(logits[0, :])                    # ties: the first maximum
        logits[rows // 2, classes // 2:] = logits[rows // 2].max() + 1          # a run of equal maxima
        logits[-1, classes - 1] = np.nan                         # a NaN row: the NaN is the maximum
        if rows > 2:
            logits[1, [0, classes - 1]] = np.nan                 # two NaNs: the first
    target = rs.randint(0, max(classes, 2), size=rows).astype(np.int64)
    target[::3] = R.classify_ref(logits, target, -1)[0][::3]     # some rows correct
    target[rows // 2] = 0                                        # an ignored row under ignore_label = 0
    want_preds = R.classify_ref(logits, target, -1)[0]
    assert want_preds.tolist() == torch.max(torch.from_numpy(logits), 1)[1].tolist()
    tl, _, _ = offset_copy(logits, 1)
    for ignore in (0, -1):
        want = R.classify_ref(logits, target, ignore)[1]
        acc = ops.new_classify_record(DEV)
        _, preds = ops.classify_stats(tl, T(target), ignore, acc, want_preds=True)
        assert np.array_equal(N(preds), want_preds)
        assert acc.tolist() == list(want)
        ops.classify_stats(T(logits), T(target), ignore, acc)                    # a second call accumulates; no preds asked for
        assert acc.tolist() == [2 * v for v in want]
    pred_guard, pbuf, g = offset_copy(np.zeros(rows, np.int64), 1)
    acc = ops.new_classify_record(DEV)
    ops._call('sg_classify_stats', tl.data_ptr(), T(target).data_ptr(), rows, classes, -1, pred_guard.data_ptr(), acc.data_ptr(),
              ops._stream())
    assert int(pbuf[-1]) == int(g) and int(pbuf[0]) == int(g) and np.array_equal(N(pred_guard), want_preds)


def test_profiler_kinds():
    names = set(ops.prof_read())
    assert set(CLS_KINDS) <= names
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        x = torch.randn(2, 3, 8, 8, device=DEV)
        ops.add_relu(ops.maxpool3s2(x), ops.maxpool3s2(x))
        ops.classify_stats(torch.randn(4, 5, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV))
        prof = ops.prof_read()
    finally:
        ops.prof_enable(False)
    assert [prof[k]['launches'] for k in CLS_KINDS] == [2, 1, 0, 0, 1]


# =====================================================================================================================================
# 2. blocks in training mode
# =====================================================================================================================================
def _randomise(mod, g, stats=True):
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                if stats:
                    m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                    m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))


BLOCKS = [('basic', 64, 64, 1, 4, 14), ('basic', 64, 128, 2, 4, 14), ('bottleneck', 256, 64, 1, 4, 14), ('bottleneck', 256, 128, 2, 4, 14),
          ('bottleneck', 128, 64, 2, 3, 7), ('basic', 128, 128, 1, 2, 16)]


def _make_block(kind, inplanes, planes, stride, ours):
    exp = 1 if kind == 'basic' else 4
    need_ds = stride != 1 or inplanes != planes * exp
    if ours:
        from scene_generation_amd import layers
        ds = nn.Sequential(A._conv(inplanes, planes * exp, 1, stride), layers.BatchNorm2d(planes * exp)) if need_ds else None
        return (A.BasicBlock if kind == 'basic' else A.Bottleneck)(inplanes, planes, stride, ds)
    ds = R.ref_downsample(inplanes, planes * exp, stride) if need_ds else None
    return (R.RefBasicBlock if kind == 'basic' else R.RefBottleneck)(inplanes, planes, stride, ds)


def _run_ref(ref, x, gy, dtype, train):
    m = copy.deepcopy(ref).to(dtype).train(train)
    xx = x.to(dtype).clone().requires_grad_(True)
    y = m(xx)
    y.backward(gy.to(dtype))
    return y.detach(), xx.grad, {k: p.grad for k, p in m.named_parameters()}, m


@pytest.mark.parametrize('case', BLOCKS, ids=lambda c: '%s_%d_%d_s%d_n%d_%d' % c)
def test_block_training_mode(case):
    kind, inplanes, planes, stride, n, hw = case
    g = torch.Generator().manual_seed(hw * 1000 + inplanes + planes)
    ref = _make_block(kind, inplanes, planes, stride, ours=False)
    _randomise(ref, g)
    blk = _make_block(kind, inplanes, planes, stride, ours=True)
    blk.load_state_dict(ref.state_dict())
    blk = blk.to(DEV).train(True)
    x = torch.randn(n, inplanes, hw, hw, generator=g)
    oh = (hw - 1) // stride + 1
    gy = torch.randn(n, planes * (1 if kind == 'basic' else 4), oh, oh, generator=g)
    y64, gx64, gp64, _ = _run_ref(ref, x, gy, torch.float64, True)
    y32, gx32, gp32, _ = _run_ref(ref, x, gy, torch.float32, True)
    if case == BLOCKS[-1]:                                       # the Winograd route: 2 * 8 * 8 = 128 tiles, 128 channels
        d = ops._conv_desc(n, 128, 0, hw, hw, 128, 3, 1, 1, False, 1, hw, hw)
        assert ops.WINOGRAD and ops._q(d, 'sg_conv2d_wino_supported')
    tx = x.to(DEV).requires_grad_(True)
    y = blk(tx)
    y.backward(gy.to(DEV))
    tag = '%s %d->%d s%d' % (kind, inplanes, planes, stride)
    check('block', tag + ' y', y, y64, y32)
    check('block', tag + ' gx', tx.grad, gx64, gx32)
    for k, p in blk.named_parameters():
        check('block', tag + ' ' + k, p.grad, gp64[k], gp32[k])


# =====================================================================================================================================
# 3. every distinct convolution of ResNet-18 / 50 / 101 at 224, alone
# =====================================================================================================================================
def _all_descs():
    out = []
    for name in ('resnet18', 'resnet50', 'resnet101'):
        for d in A.conv_descs(name, 224):
            if d not in out:
                out.append(d)
    return out


DESCS = [(2,) + d for d in _all_descs()] + [(32, 128, 128, 3, 1, 28)]


@pytest.mark.parametrize('case', DESCS, ids=lambda c: 'n%d_c%d_m%d_k%d_s%d_h%d' % c)
def test_conv_desc(case):
    n, cin, cout, ks, stride, h = case
    g = torch.Generator().manual_seed(cin * 7 + cout * 3 + ks + stride + h)
    x = torch.randn(n, cin, h, h, generator=g)
    w = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
    oh = (h + 2 * (ks // 2) - ks) // stride + 1
    gy = torch.randn(n, cout, oh, oh, generator=g)
    refs = {}
    for dt in (torch.float64, torch.float32):
        xx, ww = x.to(dt).clone().requires_grad_(True), w.to(dt).clone().requires_grad_(True)
        y = F.conv2d(xx, ww, None, stride, ks // 2)
        y.backward(gy.to(dt))
        refs[dt] = (y.detach(), xx.grad, ww.grad)
    if n == 32:
        d = ops._conv_desc(n, cin, 0, h, h, cout, 3, 1, 1, False, 1, h, h)
        assert ops.WINOGRAD and ops._q(d, 'sg_conv2d_wino_supported')
    tx, tw = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    ty = ops.conv2d(tx, tw, None, stride=stride, pad=ks // 2)
    ty.backward(gy.to(DEV))
    tag = 'N%d %d->%d k%d s%d @%d' % case
    fam = 'conv_wino' if n == 32 else 'conv'
    check(fam, tag + ' fwd', ty, refs[torch.float64][0], refs[torch.float32][0])
    check(fam, tag + ' dgrad', tx.grad, refs[torch.float64][1], refs[torch.float32][1])
    check(fam, tag + ' wgrad', tw.grad, refs[torch.float64][2], refs[torch.float32][2])


def test_winograd_route_at_the_scoring_shapes():
    """which 3x3 stride-1 convs of a 224 x 224 chunk qualify for the Winograd route (even planes, >= 128 channels in multiples of
    128, N * OH/2 * OW/2 a multiple of 128): with 64 crops only the 128-channel convs on 28 x 28; the 256-channel convs on 14 x 14
    need 128 crops; the 512-channel convs on the odd 7 x 7 plane never do"""
    def wino(n, c, h):
        return bool(ops._q(ops._conv_desc(n, c, 0, h, h, c, 3, 1, 1, False, 1, h, h), 'sg_conv2d_wino_supported'))
    assert ops.WINOGRAD
    assert [wino(64, 64, 56), wino(64, 128, 28), wino(64, 256, 14), wino(64, 512, 7)] == [False, True, False, False]
    assert [wino(128, 128, 28), wino(128, 256, 14), wino(128, 512, 7)] == [True, True, False]
    assert not wino(63, 128, 28) and not wino(8, 128, 28)            # a ragged last chunk


# =====================================================================================================================================
# 4. whole networks
# =====================================================================================================================================
def _net_pair(name, n_class, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    ref = R.RefResNet(name, n_class)
    for m in ref.modules():                                      # torchvision's init, as the code under test draws it
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
    _randomise(ref, g)
    with skip_random_init():
        net = A._build(name, n_class)
    net.load_state_dict(ref.state_dict())
    return ref, net.to(DEV), g


@pytest.fixture(scope='module', params=['resnet18', 'resnet50'])
def eval_case(request):
    """the eval-mode references of one network, computed once: logits and every parameter gradient in float64 and float32"""
    name = request.param
    ref, net, g = _net_pair(name, 172, 18 if name == 'resnet18' else 50)
    x = torch.randn(8, 3, 56, 56, generator=g)
    gy = torch.randn(8, 172, generator=g)
    y64, _, gp64, _ = _run_ref(ref, x, gy, torch.float64, False)
    y32, _, gp32, _ = _run_ref(ref, x, gy, torch.float32, False)
    return dict(name=name, ref=ref, net=net, x=x, gy=gy, y64=y64, y32=y32, gp64=gp64, gp32=gp32)


def test_network_eval_logits_and_gradients(eval_case):
    c = eval_case
    net = c['net'].eval()
    for p in net.parameters():
        p.requires_grad = True
        p.grad = None
    y = net(c['x'].to(DEV))
    y.backward(c['gy'].to(DEV))
    check('net_eval', c['name'] + ' logits', y, c['y64'], c['y32'])
    for k, p in net.named_parameters():
        check('net_eval', c['name'] + ' ' + k, p.grad, c['gp64'][k], c['gp32'][k])


def test_network_eval_folded_against_unfolded(eval_case):
    c = eval_case
    net = c['net'].eval()
    x = c['x'].to(DEV)
    ops.prof_enable(True)
    try:
        with torch.no_grad():
            ops.prof_reset()
            folded = net(x)
            prof_f = ops.prof_read()
            A.ResNet.fold_batchnorm = False
            try:
                ops.prof_reset()
                plain = net(x)
                prof_p = ops.prof_read()
            finally:
                A.ResNet.fold_batchnorm = True
            ops.prof_reset()
            again = net(x)                                       # the cached fold: no fold launch, the same bits
            prof_c = ops.prof_read()
    finally:
        ops.prof_enable(False)
    n_bn = sum(isinstance(m, nn.BatchNorm2d) for m in net.modules())
    assert prof_f['batchnorm']['launches'] == 0 and prof_f['bn_fold']['launches'] == n_bn
    assert prof_p['batchnorm']['launches'] >= n_bn and prof_p['bn_fold']['launches'] == 0
    assert prof_c['bn_fold']['launches'] == 0 and torch.equal(again, folded)
    check('fold', c['name'] + ' folded logits', folded, c['y64'], c['y32'])
    check('fold', c['name'] + ' unfolded logits', plain, c['y64'], c['y32'])
    # the cache follows the weights: a write through torch, train(), load_state_dict()
    with torch.no_grad():
        net.bn1.weight.mul_(2.0)
        changed = net(x)
        net.bn1.weight.mul_(0.5)
        assert not torch.equal(changed, folded) and torch.equal(net(x), folded)
    net.train(True)
    assert not net._fold_cache
    net.eval()
    with torch.no_grad():
        assert torch.equal(net(x), folded)


def test_resnet101_eval_forward():
    ref, net, g = _net_pair('resnet101', 172, 101)
    x = torch.randn(4, 3, 56, 56, generator=g)
    with torch.no_grad():
        y64 = copy.deepcopy(ref).double().eval()(x.double())
        y32 = ref.eval()(x)
        check('net_eval', 'resnet101 folded logits', net.eval()(x.to(DEV)), y64, y32)


@pytest.mark.parametrize('name', ['resnet18', 'resnet50'])
def test_network_training_mode(name):
    """logits, running statistics and the fc gradients (whole-network gradients in training mode are noise already on the CPU)"""
    ref, net, g = _net_pair(name, 172, 7)
    x = torch.randn(8, 3, 56, 56, generator=g)
    gy = torch.randn(8, 172, generator=g)
    y64, _, gp64, m64 = _run_ref(ref, x, gy, torch.float64, True)
    y32, _, gp32, m32 = _run_ref(ref, x, gy, torch.float32, True)
    net.train(True)
    y = net(x.to(DEV))
    y.backward(gy.to(DEV))
    check('net_train', name + ' logits', y, y64, y32)
    for k in ('fc.weight', 'fc.bias'):
        check('net_train', name + ' ' + k, dict(net.named_parameters())[k].grad, gp64[k], gp32[k])
    sd, sd64, sd32 = net.state_dict(), m64.state_dict(), m32.state_dict()
    for k in sd:
        if k.endswith(('running_mean', 'running_var')):
            check('net_train', name + ' ' + k, sd[k], sd64[k], sd32[k])
        elif k.endswith('num_batches_tracked'):
            assert int(sd[k]) == 1


def test_two_sgd_steps_under_the_freeze_rule(capsys):
    g = torch.Generator().manual_seed(11)
    with skip_random_init():
        net = A.all_pretrained_models(172, name='resnet18')
    ref = R.RefResNet('resnet18', 172)
    torch.manual_seed(3)
    for m in ref.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
    _randomise(ref, g)
    net.load_state_dict(ref.state_dict())
    net = net.to(DEV).train(True)
    frozen = [k for k, p in net.named_parameters() if not p.requires_grad]
    assert frozen and all(k.startswith(('conv1.', 'bn1.', 'layer1.')) for k in frozen)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    xs = [torch.randn(8, 3, 56, 56, generator=g) for _ in range(2)]
    labels = [torch.randint(0, 172, (8,), generator=g) for _ in range(2)]
    opt = FusedSGD([p for p in net.parameters() if p.requires_grad], lr=0.001, momentum=0.9)
    calls0 = ops.CALLS[0]
    for x, t in zip(xs, labels):
        opt.zero_grad()
        ops.cross_entropy(net(x.to(DEV)), t.to(DEV)).backward()
        c = ops.CALLS[0]
        opt.step()
        assert ops.CALLS[0] == c + 1                             # one launch
    assert ops.CALLS[0] > calls0
    refs = {}
    for dt in (torch.float64, torch.float32):
        m = copy.deepcopy(ref).to(dt).train(True)
        for k, p in m.named_parameters():
            p.requires_grad = k not in frozen
        o = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.001, momentum=0.9)
        for x, t in zip(xs, labels):
            o.zero_grad()
            F.cross_entropy(m(x.to(dt)), t).backward()
            o.step()
        refs[dt] = m.state_dict()
    after = net.state_dict()
    for k in frozen:
        assert torch.equal(after[k], before[k]), k               # bit-unchanged
    for k in after:
        if k.startswith(('bn1.', 'layer1.')) and k.endswith(('running_mean', 'running_var')):
            assert not torch.equal(after[k], before[k]), k        # the frozen BatchNorms still ran in training mode
    for k, p in net.named_parameters():
        if k not in frozen:
            assert not torch.equal(after[k], before[k]), k
            check('sgd_steps', k, after[k], refs[torch.float64][k], refs[torch.float32][k])
    sd = opt.state_dict()
    assert set(sd['state'][0]) == {'momentum_buffer'} and sd['param_groups'][0]['momentum'] == 0.9
    assert len(sd['state']) == len(opt.fp.params) and sd['param_groups'][0]['params'] == list(range(len(opt.fp.params)))
    # a step taken while in eval mode: the cached fold sees the kernel's write (the step bumps the parameters' version counters)
    net.eval()
    x0 = xs[0].to(DEV)
    with torch.no_grad():
        a = net(x0)
        assert net._fold_cache
    opt.zero_grad()
    opt.step()                                                   # a zero gradient: the momentum still moves every parameter
    with torch.no_grad():
        b = net(x0)
    assert not torch.equal(a, b)
    opt.param_groups[0]['lr'] = 0.5
    assert opt.lr == 0.5
    with pytest.raises(NotImplementedError):
        opt.zero_grad(set_to_none=True)


# =====================================================================================================================================
# 5. AccuracyMeter, Sampler, command line
# =====================================================================================================================================
@pytest.fixture(scope='module')
def classifier():
    torch.manual_seed(21)
    net = A.resnet18(12)
    _randomise(net, torch.Generator().manual_seed(22))
    with torch.no_grad():
        net.fc.bias[0] = -100.0                                  # never predicts the __image__ class, whose rows are not counted
    return net.to(DEV).eval()


def _meter_batch():
    b = make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=SH.C, num_preds=7, num_attributes=35, seed=321)
    return b


def test_accuracy_meter_against_the_reference_loop(classifier):
    b = _meter_batch()
    imgs, boxes, o2i = b.imgs.to(DEV), b.boxes.to(DEV), b.obj_to_img.to(DEV)
    meter = A.AccuracyMeter(classifier, input_shape=56, crop_chunk=64)
    logits = torch.cat(meter.logits(imgs, boxes, o2i))
    top2 = logits.topk(2, 1)[0]
    margin = float(((top2[:, 0] - top2[:, 1]) / logits.abs().max()).min())
    print('smallest top-2 gap / max |logit| = %.3e' % margin)
    assert margin > 1e-4                                         # a clear margin: the chunk size cannot flip a prediction
    preds = logits.argmax(1).cpu()
    objs = b.objs.clone()
    real = (objs != 0).nonzero().flatten()
    objs[real[::2]] = preds[real[::2]].clamp(min=1)              # half the real objects labelled with their prediction
    corrects = real_objects_count = 0
    for pred, label in zip(preds, objs):                         # sample_images.py:236-239
        if label.item() != 0:
            real_objects_count += 1
            corrects += 1 if pred.item() == label.item() else 0
    assert 0 < corrects and real_objects_count < objs.numel()
    for chunk in (3, 64):
        meter = A.AccuracyMeter(classifier, input_shape=56, crop_chunk=chunk)
        meter.update(imgs, boxes, o2i, objs.to(DEV))
        s = meter.summary()
        assert s == {'accuracy': corrects / real_objects_count, 'correct': corrects, 'counted': real_objects_count}, chunk
        meter.update(imgs, boxes, o2i, objs.to(DEV))              # accumulates
        assert meter.summary()['counted'] == 2 * real_objects_count
    assert A.AccuracyMeter(classifier).summary()['counted'] == 0


def test_accuracy_cli_train_and_score(tmp_path, capsys):
    """both subcommands of python -m scene_generation_amd.accuracy on a resnet18 at 56 x 56: the synthetic loaders, the FusedSGD +
    StepLR wiring, the save name, a file load_model reads back, and the score path through sample.build_model"""
    from trainer_helpers import _batch, _run, _trainer
    path = A.main(['train', '--model_name', 'resnet18', '--epochs', '2', '--batch_size', '2', '--input_shape', '56', '--image_size', '32',
                   '--n_class', '12', '--synthetic_batches', '2', '--save_loc', str(tmp_path)])
    out = capsys.readouterr()
    assert path == str(tmp_path / 'resnet18_12_classes.pth') and 'WITHOUT ImageNet weights' in out.err
    assert out.out.count('train Loss: ') == 2 and out.out.count('val Loss: ') == 2 and 'Epoch 1/1' in out.out
    losses = [float(v) for v in __import__('re').findall(r'Loss: ([\d.]+|nan)', out.out)]
    assert len(losses) == 4 and all(np.isfinite(losses))
    sd = torch.load(path, map_location='cpu')
    assert sd['fc.weight'].shape == (12, 512) and not any(v.is_cuda for v in sd.values())
    tr, ck, args = _trainer(tmp_path / 'train')
    _run(tr, _batch(), range(1))
    ckpt = tr.save_checkpoint(ck, 1, args, 0)
    res = A.main(['score', '--model', path, '--model_name', 'resnet18', '--checkpoint', ckpt, '--input_shape', '56', '--crop_chunk', '4',
                  '--batch_size', '3', '--num_samples', '3', '--use_gt_textures', '1', '--use_gt_boxes', '1', '--use_gt_masks', '1'])
    text = capsys.readouterr().out
    assert res['counted'] > 0 and 0.0 <= res['accuracy'] <= 1.0 and 'Accuracy {}'.format(res['accuracy']) in text


def _sampling_model():
    m = SH.small_model(Model, make_sampling_vocab(SH.C, 7, SH.A)).to(DEV)
    m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    return m


def test_sampler_with_meter_keeps_one_host_read(classifier, monkeypatch):
    m, b = _sampling_model(), _meter_batch()
    plain = sample.Sampler(m).sample_batch(b, use_gt_textures=True)
    reads = []
    for name in ('tolist', 'item', 'cpu', 'numpy'):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    for use_gt_boxes in (False, True):
        meter = A.AccuracyMeter(classifier, input_shape=56, crop_chunk=4)
        s = sample.Sampler(m, accuracy=meter)
        s.sample_batch(b, use_gt_textures=True, use_gt_boxes=use_gt_boxes)           # warm-up
        del reads[:]
        out = s.sample_batch(b, use_gt_textures=True, use_gt_boxes=use_gt_boxes)
        assert reads == ['tolist'], reads
        if not use_gt_boxes:
            assert torch.equal(out.images, plain.images) and torch.equal(out.boxes_pred, plain.boxes_pred)
        got = s.accuracy_summary()
        assert got['counted'] == 2 * int((b.objs != 0).sum())
    assert sample.Sampler(m).accuracy_summary() is None


def test_sample_cli_prints_accuracy(classifier, tmp_path, capsys):
    from trainer_helpers import _batch, _run, _trainer
    tr, ck, args = _trainer(tmp_path / 'train')
    _run(tr, _batch(), range(1))
    path = tr.save_checkpoint(ck, 1, args, 0)
    clf = str(tmp_path / 'resnet18_12_classes.pth')
    torch.save({'module.' + k: v.cpu() for k, v in classifier.state_dict().items()}, clf)
    base = ['--checkpoint', path, '--use_gt_boxes', '1', '--use_gt_masks', '1', '--use_gt_textures', '1', '--batch_size', '3',
            '--num_samples', '3']
    capsys.readouterr()
    random.seed(0)
    res0 = sample.main(base + ['--output_dir', str(tmp_path / 'a')])
    out0 = capsys.readouterr().out
    random.seed(0)
    res1 = sample.main(base + ['--output_dir', str(tmp_path / 'b'), '--accuracy_model_path', clf, '--accuracy_model_name', 'resnet18',
                               '--accuracy_input_shape', '56'])
    out1 = capsys.readouterr().out
    assert 'Accuracy' not in out0 and 'accuracy' not in res0
    lines0, lines1 = out0.splitlines(), out1.splitlines()
    acc_lines = [l for l in lines1 if l.startswith('Accuracy ')]
    assert len(acc_lines) == 1 and lines1.index(acc_lines[0]) > max(i for i, l in enumerate(lines1) if l.startswith('r0.3 '))
    assert [l for l in lines1 if l not in acc_lines] == lines0     # with the flag absent every output is what it was
    assert res1['accuracy']['counted'] > 0 and float(acc_lines[0].split()[1]) == res1['accuracy']['accuracy']
    for p0, p1 in zip(res0['paths'], res1['paths']):
        assert open(p0, 'rb').read() == open(p1, 'rb').read()
    # a path that is no file: no meter, no line (sample_images.py:181)
    sample.main(base + ['--output_dir', str(tmp_path / 'c'), '--accuracy_model_path', str(tmp_path / 'missing.pth')])
    assert 'Accuracy' not in capsys.readouterr().out


