"""Every InstanceNorm / BatchNorm / channel-sum launch plan and every scalar-loss, multi-loss and cross-entropy path against a
float64 reference of the same operation (the shape tables are tests/norm_cases.py; tests/test_norm_dispatch_cpu.py shows they
reach every plan the dispatch can choose).  Tolerances follow close() of gpu_harness.py and are no looser than its
test_instance_norm / test_batch_norm: y 2e-5, gradients 1e-4."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import norm_cases as NC
from oracle import sg_oracle as O
from gpu_harness import close
from gpu_harness import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SLOPE = 0.2


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=_gen(seed), dtype=torch.float64).mul(hi - lo).add(lo).float()


def close_rel(a, b, tol, name=''):
    """close() on both operands divided by max|b|: a bound relative to the tensor's own magnitude (gradients of means are ~1/n)"""
    m = float(b.detach().abs().max()) if b.numel() else 0.0
    m = m if m > 0 else 1.0
    close(a.detach().double().cpu() / m, b.detach().double().cpu() / m, tol, name)


def _act64(y, act):
    return F.relu(y) if act == 1 else (F.leaky_relu(y, SLOPE) if act == 2 else y)


# =============================================================================================
# InstanceNorm
# =============================================================================================
def sign_gapped(N, C, HW, seed, offset):
    """planes that are permutations of c +- (0.05 + k d): no normalised value within 1e-3 of the activation kink (the reference
    backward then uses its own derivative and cannot disagree with the kernel's mask), c uniform in offset + [-1, 1]"""
    g = _gen(seed)
    d = 2.0 / HW
    for _ in range(40):
        k = torch.arange(HW, dtype=torch.float64)
        v = (0.05 + k * d) * torch.where(k % 2 == 0, 1.0, -1.0)
        perm = torch.argsort(torch.rand(N * C, HW, generator=g), dim=1)
        c = torch.rand(N * C, 1, generator=g, dtype=torch.float64) * 2 - 1 + offset
        x = (c + v[perm]).float()
        if HW == 1:
            return x.view(N, C, 1, HW)
        xd = x.double()
        z = (xd - xd.mean(1, keepdim=True)) / (xd.var(1, unbiased=False, keepdim=True) + 1e-5).sqrt()
        if float(z.abs().min()) >= 1e-3:
            return x
        d *= 1.37
    raise AssertionError('no sign-gapped plane of %d elements' % HW)


def _instnorm_ref(x, gy, sk, act):
    xr = x.double().requires_grad_()
    mu = xr.mean((2, 3), keepdim=True)                    # (F.instance_norm refuses planes of one element)
    yr = _act64((xr - mu) / ((xr - mu).pow(2).mean((2, 3), keepdim=True) + 1e-5).sqrt(), act)
    if sk is not None:
        yr = yr + sk.double()
    yr.backward(gy.double())
    return yr.detach(), xr.grad


def _on_device(t, aligned):
    """t on the device, 16-byte aligned or through a one-float storage offset (a leaf that requires grad)"""
    if aligned:
        out = t.to(DEV)
        assert out.data_ptr() % 16 == 0
    else:
        buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
        out = buf[1:1 + t.numel()].view(t.shape)
        out.copy_(t)
        assert out.data_ptr() % 16 == 4
    return out.detach().requires_grad_()


def _run_instnorm(hip, x, gy, sk, act, aligned):
    xg = _on_device(x, aligned)
    sg = sk.to(DEV) if sk is not None else None
    yg = hip.instance_norm(xg, skip=sg, act=act, slope=SLOPE)
    yg.backward(gy.to(DEV))
    return yg.detach(), xg.grad


@pytest.mark.parametrize('idx', range(len(NC.INSTNORM_CASES)))
def test_instance_norm_every_plan_vs_fp64(hip, idx):
    from scene_generation_amd import _hip
    N, C, H, W, offset = NC.INSTNORM_CASES[idx]
    HW = H * W
    act, with_skip = idx % 3, idx % 2 == 0
    x = sign_gapped(N, C, HW, 700 + idx, offset).view(N, C, H, W)
    gy = rnd((N, C, H, W), 800 + idx)
    sk = rnd((N, C, H, W), 900 + idx) if with_skip else None
    yr, gxr = _instnorm_ref(x, gy, sk, act)
    for reg in NC.INSTNORM_REG_VALUES:
        with NC.option('instnorm_reg', reg):
            for aligned in (True, False):
                plan = (NC.instnorm_plan(_hip.lib(), 0, HW, aligned), NC.instnorm_plan(_hip.lib(), 1, HW, aligned))
                yg, gxg = _run_instnorm(hip, x, gy, sk, act, aligned)
                tag = 'HW %d reg %d %s act %d plan %s' % (HW, reg, 'aligned' if aligned else 'offset', act, plan)
                close(yg, yr, 2e-5, 'y ' + tag)
                close(gxg, gxr, 1e-4, 'gx ' + tag)


@pytest.mark.parametrize('HW', [1, 3, 64, 100, 1024, 1600, 16384, 20000, 65536])
def test_instance_norm_constant_planes(hip, HW):
    """constant planes: y = 0 (exactly when the plane's sum is exact, 1.5) and a finite gradient through rstd = 1/sqrt(eps)"""
    N, C = 2, 3
    gy = rnd((N, C, 1, HW), 41)
    for c in (1.5, -0.3):
        x = torch.full((N, C, 1, HW), c)
        yr, gxr = _instnorm_ref(x, gy, None, 0)
        for reg in NC.INSTNORM_REG_VALUES:
            with NC.option('instnorm_reg', reg):
                for aligned in (True, False):
                    yg, gxg = _run_instnorm(hip, x, gy, None, 0, aligned)
                    tag = 'c %g HW %d reg %d aligned %d' % (c, HW, reg, aligned)
                    assert torch.isfinite(gxg).all(), tag
                    if c == 1.5:
                        assert float(yg.abs().max()) == 0.0, tag
                        close(gxg, gxr, 1e-4, 'gx ' + tag)
                    else:
                        assert float(yg.abs().max()) <= 1e-3, tag


# =============================================================================================
# BatchNorm
# =============================================================================================
@pytest.mark.parametrize('idx', range(len(NC.BATCHNORM_CASES)))
def test_batch_norm_every_plan_vs_fp64(hip, idx):
    from scene_generation_amd.layers import BatchNorm1d, BatchNorm2d
    shape, blocks = NC.BATCHNORM_CASES[idx]
    C = shape[1]
    act = idx % 3 if int(torch.tensor(shape).prod()) < 100000 else 0        # (no activation kink among millions of values)
    one_d = len(shape) == 2
    ref = (nn.BatchNorm1d(C) if one_d else nn.BatchNorm2d(C)).double()
    mine = (BatchNorm1d(C) if one_d else BatchNorm2d(C))
    with torch.no_grad():
        mine.weight.copy_(rnd((C,), 61, 0.25, 1.75))
        mine.bias.copy_(rnd((C,), 62, -0.2, 0.2))
        ref.weight.copy_(mine.weight.double())
        ref.bias.copy_(mine.bias.double())
    mine = mine.to(DEV)
    with NC.option('bn_blocks', blocks):
        for step in range(4):
            training = step < 3                                          # three training steps, then eval
            ref.train(training)
            mine.train(training)
            x = rnd(shape, 1000 * idx + 10 * step, -2.0, 2.6)
            gy = rnd(shape, 1000 * idx + 10 * step + 1)
            ref.zero_grad()
            mine.zero_grad()
            xr = x.double().requires_grad_()
            yr = _act64(ref(xr), act)
            yr.backward(gy.double())
            xg = x.to(DEV).requires_grad_()
            yg = mine(xg, act=act, slope=SLOPE)
            yg.backward(gy.to(DEV))
            tag = '%s step %d training %d' % (shape, step, training)
            close(yg, yr, 2e-5, 'y ' + tag)
            close(xg.grad, xr.grad, 1e-4, 'gx ' + tag)
            close(mine.weight.grad, ref.weight.grad, 1e-4, 'ggamma ' + tag)
            close(mine.bias.grad, ref.bias.grad, 1e-4, 'gbeta ' + tag)
            close(mine.running_mean, ref.running_mean, 1e-5, 'running_mean ' + tag)
            close(mine.running_var, ref.running_var, 1e-5, 'running_var ' + tag)
            assert int(mine.num_batches_tracked) == int(ref.num_batches_tracked) == min(step + 1, 3)


# =============================================================================================
# channel_sum (conv bias gradients), through the C ABI
# =============================================================================================
def _channel_sum(g, N, C, HW, with_ws):
    from scene_generation_amd import _hip
    L = _hip.lib()
    out = torch.full((C,), float('nan'), device=DEV)
    wsb = L.sg_channel_sum_ws_bytes(C) if with_ws else 0
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
    rc = L.sg_channel_sum(ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(out.data_ptr()), N, C, HW,
                          ctypes.c_void_p(ws.data_ptr()) if with_ws else None, wsb, torch.cuda.current_stream().cuda_stream)
    _hip.check(rc, 'sg_channel_sum')
    return out


@pytest.mark.parametrize('case', NC.CHANNEL_SUM_CASES)
def test_channel_sum_every_plan_vs_fp64(hip, case):
    N, C, HW, with_ws = case
    g = rnd((N, C, HW), 71 + N + C + HW, -1.0, 1.5)
    out = _channel_sum(g.to(DEV), N, C, HW, with_ws).cpu().double()
    gd = g.double()
    ref = gd.sum((0, 2))
    bound = 2e-6 * gd.abs().sum((0, 2))                 # |error| per channel relative to sum |g| of that channel
    err = (out - ref).abs()
    assert torch.isfinite(out).all()
    assert bool((err <= bound).all()), 'channel %d: error %.3e, bound %.3e' % (int((err / bound).argmax()),
                                                                              float(err.max()), float(bound.max()))


# =============================================================================================
# scalar losses
# =============================================================================================
LOSS_N = [1, 7, 2048, 2049, 4194305]


def _loss_inputs(kind, n, seed):
    from scene_generation_amd.ops import _core as K
    if kind == K.LOSS_BCE_PROB_CONST:
        return rnd((n,), seed, 1e-3, 1 - 1e-3), None
    a = rnd((n,), seed, -3.0, 3.0)
    b = rnd((n,), seed + 1, -3.0, 3.0) if kind in (K.LOSS_MSE, K.LOSS_L1) else None
    return a, b


def _loss_ref64(kind, a, b, t):
    """the float64 form of the oracle / torch formula of each kind, summed (the kernels' scale multiplies outside)"""
    from scene_generation_amd.ops import _core as K
    if kind == K.LOSS_MSE_CONST:
        return ((a - t) ** 2).sum()
    if kind == K.LOSS_MSE:
        return ((a - b) ** 2).sum()
    if kind == K.LOSS_L1:
        return (a - b).abs().sum()
    if kind == K.LOSS_BCE_CONST:
        return O.bce_loss(a, torch.full_like(a, t)) * a.numel()
    if kind == K.LOSS_MEAN:
        return a.sum()
    if kind == K.LOSS_MSE_SIGMOID_CONST:
        return ((a.sigmoid() - t) ** 2).sum()
    assert kind == K.LOSS_BCE_PROB_CONST
    return F.binary_cross_entropy(a, torch.full_like(a, t), reduction='sum')


def _loss_kinds():
    from scene_generation_amd.ops import _core as K
    return [K.LOSS_MSE_CONST, K.LOSS_MSE, K.LOSS_L1, K.LOSS_BCE_CONST, K.LOSS_MEAN, K.LOSS_MSE_SIGMOID_CONST,
            K.LOSS_BCE_PROB_CONST]


def _scalar_loss(kind, a, b, t, scale, gout):
    """-> (loss, d loss / d a) through ScalarLossFn (sg_loss_fwd / sg_loss_bwd)"""
    from scene_generation_amd.ops.losses import ScalarLossFn
    ag = a.to(DEV).requires_grad_()
    lg = ScalarLossFn.apply(ag, None if b is None else b.to(DEV), kind, float(t), float(scale))
    lg.backward(torch.tensor(float(gout), device=DEV))
    return lg.detach(), ag.grad


@pytest.mark.parametrize('n', LOSS_N)
def test_scalar_losses_every_kind_vs_fp64(hip, n):
    for i, kind in enumerate(_loss_kinds()):
        a, b = _loss_inputs(kind, n, 130 + 7 * i)
        t = (0.0, 1.0, 0.7)[(i + n) % 3]
        scale = 1.0 / n                                            # what the ops wrappers pass: the mean
        lg, ga = _scalar_loss(kind, a, b, t, scale, float(n))     # gout n: gradients of the sum, O(1) per element
        ar = a.double().requires_grad_()
        lr = _loss_ref64(kind, ar, None if b is None else b.double(), t)
        lr.backward()
        sc = float(torch.tensor(scale, dtype=torch.float32))
        close(lg, lr.detach() * sc, 1e-5, 'loss kind %d n %d' % (kind, n))
        close_rel(ga, ar.grad * (float(n) * sc), 1e-5, 'grad kind %d n %d' % (kind, n))


def _edge(kind, vals, t, b=None):
    a = torch.tensor(vals, dtype=torch.float32)
    lg, ga = _scalar_loss(kind, a, b, t, 1.0, 1.0)
    ar = a.double().requires_grad_()
    lr = _loss_ref64(kind, ar, None if b is None else b.double(), t)
    lr.backward()
    return lg.cpu().double(), ga.cpu().double(), lr.detach(), ar.grad


def test_bce_logits_gradient_at_zero_matches_the_oracle(hip):
    """bce_logits_const at a logit of exactly 0: the oracle's formula under autograd (clamp(min=0) passes the gradient at 0,
    |x| does not) gives 1 - t -- the contract every loss here is held to (the function's own derivative there is 0.5 - t)"""
    from scene_generation_amd.ops import _core as K
    for t in (0.0, 1.0, 0.3):
        lg, ga, lr, gr = _edge(K.LOSS_BCE_CONST, [0.0, 30.0, -30.0, 100.0, -100.0], t)
        assert float(ga[0]) == pytest.approx(1.0 - t, abs=1e-7), (t, ga)
        assert float(gr[0]) == pytest.approx(1.0 - t, abs=1e-12)
        assert torch.allclose(ga, gr, rtol=1e-6, atol=1e-7), (t, ga, gr)
        assert float(lg) == pytest.approx(float(lr), rel=1e-6)


def test_bce_prob_gradient_clamps_like_torch(hip):
    """GANLoss(use_lsgan=False): torch's BCELoss backward is (a - t) / max(a (1 - a), 1e-12) -- also where a is within 1e-12 of
    0 or 1 (a = 0, t = 1: -1e12, not 0; a = 1e-30: -1e12, not -1e30)"""
    from scene_generation_amd.ops import _core as K
    vals = [0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24, 0.5]
    for t in (1.0, 0.0, 0.25):
        lg, ga, lr, gr = _edge(K.LOSS_BCE_PROB_CONST, vals, t)
        assert torch.isfinite(ga).all()
        assert torch.allclose(ga, gr, rtol=1e-6, atol=0.0), (t, ga, gr)
        assert float(lg) == pytest.approx(float(lr), rel=1e-6)
    _, ga, _, _ = _edge(K.LOSS_BCE_PROB_CONST, [0.0, 1e-30], 1.0)
    assert float(ga[0]) == pytest.approx(-1e12, rel=1e-6) and float(ga[1]) == pytest.approx(-1e12, rel=1e-6)


def test_loss_edge_inputs(hip):
    from scene_generation_amd.ops import _core as K
    lg, ga, lr, gr = _edge(K.LOSS_MSE_SIGMOID_CONST, [100.0, -100.0], 1.0)
    assert torch.isfinite(ga).all() and float(ga.abs().max()) <= 1e-30
    assert float(lg) == pytest.approx(float(lr), abs=1e-7)
    b = torch.tensor([0.5, -2.0, 0.0, 3.0])
    lg, ga, lr, gr = _edge(K.LOSS_L1, [0.5, -2.0, 0.0, 3.0], 0.0, b)          # a == b: loss 0, gradient 0 (sign(0))
    assert float(lg) == 0.0 and float(ga.abs().max()) == 0.0 and float(gr.abs().max()) == 0.0


# =============================================================================================
# multi_loss: one launch for many terms, bit-identical to per-term ScalarLossFn + ops.weighted_sum
# =============================================================================================
MULTI_SIZES = [1, 7, 255, 2048, 2049, 100000, 33, 4194305, 513, 64, 3]


def _multi_terms(kind, nterms, seed):
    from scene_generation_amd.ops import _core as K
    sizes = [MULTI_SIZES[(i * 5 + nterms) % len(MULTI_SIZES)] for i in range(nterms)]
    if nterms >= 11 and 4194305 not in sizes:
        sizes[3] = 4194305
    if nterms < 11:
        sizes = [min(s, 100000) for s in sizes]
    a, b = [], []
    for i, n in enumerate(sizes):
        ai, bi = _loss_inputs(kind, n, seed + 3 * i)
        a.append(ai)
        b.append(bi)
    weights = [(0.0 if i % 7 == 3 else (-0.5 - 0.1 * i if i % 4 == 1 else 0.25 + 0.05 * i)) for i in range(nterms)]
    targets = [(0.0, 1.0, 0.6)[i % 3] for i in range(nterms)]
    grad = [i % 3 != 2 for i in range(nterms)]                       # some terms do not require grad: null gradient pointers
    pair = kind in (K.LOSS_MSE, K.LOSS_L1)
    return a, (b if pair else None), weights, targets, grad


@pytest.mark.parametrize('nterms,kind_name,mean', [(1, 'LOSS_L1', True), (2, 'LOSS_MSE_CONST', False), (11, 'LOSS_L1', True),
                                                   (11, 'LOSS_BCE_CONST', False), (32, 'LOSS_MSE', True),
                                                   (32, 'LOSS_BCE_PROB_CONST', True), (33, 'LOSS_L1', False),
                                                   (33, 'LOSS_MSE_SIGMOID_CONST', True)])
def test_multi_loss_vs_fp64_and_per_term_path(hip, nterms, kind_name, mean):
    from scene_generation_amd.ops import _core as K
    from scene_generation_amd.ops.losses import ScalarLossFn, multi_loss, weighted_sum
    kind = getattr(K, kind_name)
    a, b, weights, targets, grad = _multi_terms(kind, nterms, 5000 + nterms)
    dev_a = [t.to(DEV).requires_grad_(g) for t, g in zip(a, grad)]
    dev_b = None if b is None else [t.to(DEV) for t in b]
    total = multi_loss(kind, dev_a, dev_b, targets, weights, mean)
    total.backward()
    # float64
    ra = [t.double().requires_grad_(g) for t, g in zip(a, grad)]
    ref = sum(w * _loss_ref64(kind, x, None if b is None else b[i].double(), targets[i]) *
              (float(torch.tensor(1.0 / x.numel(), dtype=torch.float32)) if mean else 1.0)
              for i, (x, w) in enumerate(zip(ra, weights)))
    ref.backward()
    close(total, ref.detach(), 1e-5, 'multi_loss %s %d' % (kind_name, nterms))
    for i, (x, r) in enumerate(zip(dev_a, ra)):
        if not grad[i]:
            assert x.grad is None
            continue
        if weights[i] == 0.0:
            assert float(x.grad.abs().max()) == 0.0
            continue
        close_rel(x.grad, r.grad, 1e-5, 'multi_loss %s term %d grad' % (kind_name, i))
    if nterms > 32:
        return
    # bitwise: ScalarLossFn per term, then ops.weighted_sum
    dev_a2 = [t.detach().clone().requires_grad_(g) for t, g in zip(dev_a, grad)]
    terms = [ScalarLossFn.apply(x, None if dev_b is None else dev_b[i], kind, float(targets[i]),
                                (1.0 / x.numel()) if mean else 1.0) for i, x in enumerate(dev_a2)]
    total2 = weighted_sum(terms, weights)
    total2.backward()
    assert torch.equal(total.detach(), total2.detach()), (float(total), float(total2))
    for i, (x, y) in enumerate(zip(dev_a, dev_a2)):
        assert (x.grad is None) == (y.grad is None)
        if x.grad is not None:
            assert torch.equal(x.grad, y.grad), 'term %d gradient differs from the per-term path' % i


# =============================================================================================
# cross-entropy
# =============================================================================================
@pytest.mark.parametrize('rows', [1, 5, 1056])
@pytest.mark.parametrize('classes', [1, 63, 64, 65, 179, 1000])
def test_cross_entropy_vs_fp64(hip, rows, classes):
    logits = rnd((rows, classes), 17 * rows + classes, -80.0, 80.0)
    target = torch.tensor([0 if r % 2 == 0 else classes - 1 for r in range(rows)], dtype=torch.int64)
    lr = logits.double().requires_grad_()
    ref = -F.log_softmax(lr, 1).gather(1, target.view(-1, 1)).mean()
    ref.backward()
    lg = logits.to(DEV).requires_grad_()
    out = hip.cross_entropy(lg, target.to(DEV))
    out.backward()
    close(out, ref.detach(), 1e-5, 'ce %dx%d' % (rows, classes))
    close_rel(lg.grad, lr.grad, 1e-5, 'ce grad %dx%d' % (rows, classes))


# =============================================================================================
# last_block: the one-launch finish of the two-stage reductions is bit-identical to the two-kernel form
# =============================================================================================
def test_last_block_is_bitwise_the_two_kernel_form(hip):
    from scene_generation_amd.layers import BatchNorm2d
    from scene_generation_amd.ops import _core as K
    from scene_generation_amd.ops.losses import multi_loss
    a_big, b_big = rnd((4194305,), 3), rnd((4194305,), 4)
    mt = _multi_terms(K.LOSS_L1, 11, 77)
    bn_x = [rnd((8, 16, 31, 31), 5, -2, 3), rnd((4, 3, 32, 32), 6, -2, 3), rnd((64, 3, 9, 9), 7, -2, 3)]
    results = {}
    for lb in (0, 7):
        with NC.option('last_block', lb):
            r = []
            for n in (7, 2049, 4194305):
                lg, ga = _scalar_loss(K.LOSS_L1, a_big[:n], b_big[:n], 0.0, 1.0 / n, 1.0)
                r += [lg, ga]
            a, b, w, t, g = mt
            dev_a = [x.to(DEV).requires_grad_() for x in a]
            tot = multi_loss(K.LOSS_L1, dev_a, [x.to(DEV) for x in b], t, w, True)
            tot.backward()
            r += [tot.detach()] + [x.grad for x in dev_a]
            for x in bn_x:
                m = BatchNorm2d(x.shape[1]).to(DEV)
                xg = x.to(DEV).requires_grad_()
                y = m(xg, act=1)
                y.backward(torch.ones_like(y))
                r += [y.detach(), xg.grad, m.weight.grad, m.bias.grad, m.running_mean, m.running_var]
            for (N, C, HW, ws) in NC.CHANNEL_SUM_CASES:
                r.append(_channel_sum(rnd((N, C, HW), N + C).to(DEV), N, C, HW, ws))
            torch.cuda.synchronize()
            results[lb] = [x.detach().cpu() for x in r]
    assert len(results[0]) == len(results[7])
    for i, (u, v) in enumerate(zip(results[0], results[7])):
        assert torch.equal(u, v), 'result %d differs between last_block 0 and 7' % i
