"""LPIPS as a training loss on the GPU (csrc/lpips.hip sg_lpips_layer_bwd / sg_lpips_input_bwd, ops/lpips.py, lpips.LPIPSLoss,
Trainer(lpips_loss=...)).

Float results -- the gradient of one tap, the loss and its gradient with respect to the pictures, the Trainer's ``g_lpips`` -- are
compared with a float64 CPU run of the plain torch restatement (tests/lpips_loss_ref.py: autograd of ``lpips_ref.layer_ref``); the
bound is the family's factor times the error torch's own float32 CPU autograd makes on the same inputs, never below 2^-24 of the
reference's largest magnitude, in max norm over every element (profiles/lpips_test_margins.md has the convention).  At a pixel of all
zeros autograd gives NaN, so there the references are the float64 and float32 NumPy closed forms.  The scaling layer's backward, the
gradient of d(x, x), repeats, offset operands and the forward of ``LpipsDistanceFn`` are compared bit for bit.  The worst ratio per
family goes to lpips_loss_margins.json in the suite's output directory.

Worst ratios measured on an MI355X with every family at the factor 16 (profiles/lpips_loss_test_margins.md): layer_bwd 1.72,
zero_pixel 0.52, loss_value 1.56, trainer 0.10 -- under 2, halved to 8; tiny_pixel 2.29 and loss_grad 2.28 stay at 16."""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

import lpips_loss_ref as R
import lpips_ref as LR
import trainer_helpers as TH
from gpu_harness import L, _release_operands  # noqa: F401  (fixtures)
from gpu_harness import Margins, bits, call, margins_fixture, outbuf, place, place_fenced, ptr, same_bits, stream, taken
from scene_generation_amd import lpips as LP
from scene_generation_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 16.0
# families whose worst observed ratio is under 2 (profiles/lpips_loss_test_margins.md): their factor is halved to 8
FACTORS = {k: 8.0 for k in ('layer_bwd', 'zero_pixel', 'loss_value', 'trainer')}
FLOOR = 2.0 ** -24
MARGINS = Margins()
_write_margins = margins_fixture(lambda: MARGINS.dump_yardstick('lpips_loss_margins.json', FACTORS, FACTOR))


def check(family, name, got, ref64, ref32):
    """|got - ref64| <= factor * max(|ref32 - ref64|, 2^-24 max|ref64|), in max norm over the tensor; factor = the family's"""
    MARGINS.yardstick(family, name, got, ref64, ref32, FACTORS, FACTOR, FLOOR)


def _pd(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_double))


def _raw_bwd(L, f0, f1, w, gout, off=0, fenced=False):
    """sg_lpips_layer_bwd through the C ABI on operands ``off`` floats past a 16-byte boundary (``fenced``: NaN around every input),
    into a pre-filled result with a guard word behind it -> numpy [P, C, HW]; every element written, the guard intact"""
    P, C, HW = f0.shape
    put = place_fenced if fenced else place
    a, b = put(f0.numpy(), off), put(f1.numpy(), off)
    ww = None if w is None else put(w.numpy(), off)
    g = gout.to(DEV)
    o = outbuf(P * C * HW, off)
    call(L, 'sg_lpips_layer_bwd', ptr(a), ptr(b), ptr(ww), _pd(g), P, C, HW, R.EPS, ptr(o), stream())
    return taken(o, (P, C, HW), 'sg_lpips_layer_bwd %s' % ((P, C, HW),))


# =====================================================================================================================================
# 1. the gradient of one tap
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _layer_refs(shape):
    f0, f1, w, gout = R.layer_inputs(shape)
    refs = {key: (R.layer_grad_autograd(f0, f1, ww, gout, torch.float64), R.layer_grad_autograd(f0, f1, ww, gout, torch.float32))
            for key, ww in (('w', w), ('ones', None))}
    return f0, f1, w, gout, refs


@pytest.mark.parametrize('case', R.LAYER_BWD, ids=lambda c: '%dx%dx%d' % c[0])
def test_lpips_layer_bwd(L, case):
    shape, why = case
    f0, f1, w, gout, refs = _layer_refs(shape)
    t0, t1, tw, tg = f0.to(DEV), f1.to(DEV), w.to(DEV), gout.to(DEV)
    for key, ww, hw in (('w', tw, w), ('ones', None, None)):
        r64, r32 = refs[key]
        assert float(r64.abs().max()) > 0 or shape[1] == 1                           # (C = 1: its one weight is one of the zeros)
        got = ops.lpips_layer_bwd(t0, t1, ww, tg)
        assert got.dtype == torch.float32 and got.shape == t0.shape
        check('layer_bwd', '%s %s' % (shape, key), got, r64, r32)
        g = got.cpu().numpy()
        same_bits(ops.lpips_layer_bwd(t0, t1, ww, tg).cpu().numpy(), g, 'a second run')
        # operands and result one element off a 16-byte boundary, NaN around the inputs, a guard behind the result: the same bits
        same_bits(_raw_bwd(L, f0, f1, hw, gout, off=1), g, 'offset operands')
        same_bits(_raw_bwd(L, f0, f1, hw, gout, off=0, fenced=True), g, 'fenced operands')
        # the same features on both sides: t = 0 by construction, the gradient is +0 in every bit
        zero = ops.lpips_layer_bwd(t0, t0.clone(), ww, tg)
        assert not bits(zero.cpu().numpy()).any()
    # a 4-D tap, the shape the loss hands over
    if shape[2] % 4 == 0 and shape[2] >= 4:
        got4 = ops.lpips_layer_bwd(t0.view(shape[0], shape[1], 4, -1), t1.view(shape[0], shape[1], 4, -1), tw, tg)
        assert got4.shape == (shape[0], shape[1], 4, shape[2] // 4)
        assert torch.equal(got4.reshape(shape), ops.lpips_layer_bwd(t0, t1, tw, tg))


@pytest.mark.parametrize('shape', [(2, 65, 35), (1, 520, 9), (4, 64, 4096)], ids=lambda s: '%dx%dx%d' % s)
def test_zero_and_tiny_pixels(shape):
    """a pixel of f0 set to 0 gets the finite closed form (autograd: NaN); a pixel scaled to 1e-15 -- n0 ~ 1e-14, n0 * s0^2 ~ 1e-34
    -- stays finite and accurate.  Both on their own: their gradients are ~1e10 times the others'"""
    P, C, HW = shape
    f0, f1, w, gout = R.layer_inputs(shape)
    jz, jt = HW // 3, HW - 1                                       # (the tiny pixel sits in the last, possibly partial, tile)
    f0 = f0.clone()
    f0[:, :, jz] = 0
    f0[:, :, jt] *= 1e-15
    assert float(f0[:, :, jt].pow(2).sum(1).sqrt().min()) > 1.2e-38 * 1e10
    got = ops.lpips_layer_bwd(f0.to(DEV), f1.to(DEV), w.to(DEV), gout.to(DEV)).cpu()
    assert bool(torch.isfinite(got).all())
    c64 = R.layer_grad_closed(f0.numpy(), f1.numpy(), w.numpy(), gout.numpy(), np.float64)
    c32 = R.layer_grad_closed(f0.numpy(), f1.numpy(), w.numpy(), gout.numpy(), np.float32)
    assert np.isfinite(c32).all() and np.abs(c64[:, :, jz]).max() > 1e5
    check('zero_pixel', '%s pixel %d' % (shape, jz), got[:, :, jz], c64[:, :, jz], c32[:, :, jz])
    # the tiny pixel has a norm: autograd answers (float32 autograd included, which is the yardstick)
    keep = [j for j in range(HW) if j != jz]
    a64 = R.layer_grad_autograd(f0[:, :, keep], f1[:, :, keep], w, gout * (len(keep) / HW), torch.float64)
    a32 = R.layer_grad_autograd(f0[:, :, keep], f1[:, :, keep], w, gout * (len(keep) / HW), torch.float32)
    k = keep.index(jt)
    assert bool(torch.isfinite(a64).all()) and float(a64[:, :, k].abs().max()) > 1e5
    check('tiny_pixel', '%s pixel %d' % (shape, jt), got[:, :, jt], a64[:, :, k], a32[:, :, k])
    rest = [j for j in keep if j != jt]
    idx = [keep.index(j) for j in rest]
    check('layer_bwd', '%s beside a zero and a tiny pixel' % (shape,), got[:, :, rest], a64[:, :, idx], a32[:, :, idx])


def test_lpips_layer_bwd_empty_and_rejects(L):
    before = ops.CALLS[0]
    e = torch.zeros(0, 4, 3, device=DEV)
    got = ops.lpips_layer_bwd(e, e, None, torch.zeros(0, dtype=torch.float64, device=DEV))
    assert tuple(got.shape) == (0, 4, 3) and ops.CALLS[0] == before + 1                # P == 0: the entry point returns before a launch
    a, g = torch.zeros(2, 4, 3, device=DEV), torch.ones(2, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match='lpips_layer_bwd'):
        ops.lpips_layer_bwd(a, torch.zeros(2, 4, 2, device=DEV), None, g)
    with pytest.raises(ValueError, match='lpips_layer_bwd'):
        ops.lpips_layer_bwd(a, a, torch.zeros(5, device=DEV), g)
    with pytest.raises(ValueError, match='lpips_layer_bwd'):
        ops.lpips_layer_bwd(a, a, None, torch.ones(2, device=DEV))                     # a float32 gradient
    with pytest.raises(ValueError, match='lpips_layer_bwd'):
        ops.lpips_layer_bwd(a, a, None, torch.ones(3, dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError, match='lpips_layer_bwd'):
        ops.lpips_layer_bwd(a.double(), a.double(), None, g)
    with pytest.raises(RuntimeError, match='sg_lpips_layer_bwd'):
        ops.lpips_layer_bwd(a, a, None, g, eps=-1.0)
    # the entry point's own messages, on device operands
    o = torch.zeros(24, device=DEV)
    odd = torch.zeros(3, dtype=torch.float32, device=DEV)[1:]                           # 4 bytes past an 8-byte boundary
    for args, msg in (((ptr(a), ptr(a), None, _pd(g), 2, 4, 3, 1e-10, None, stream()), 'null operand'),
                      ((ptr(a), None, None, _pd(g), 2, 4, 3, 1e-10, ptr(o), stream()), 'null operand'),
                      ((ptr(a), ptr(a), None, None, 2, 4, 3, 1e-10, ptr(o), stream()), 'null operand'),
                      ((ptr(a), ptr(a), None, _pd(g), 2, 0, 3, 1e-10, ptr(o), stream()), 'bad sizes'),
                      ((ptr(a), ptr(a), None, _pd(g), 1 << 20, 1 << 10, 4, 1e-10, ptr(o), stream()), 'bad sizes'),
                      ((ptr(a), ptr(a), None, _pd(g), 2, 4, 3, -1e-10, ptr(o), stream()), 'eps must not be negative'),
                      ((ptr(a), ptr(a), None, _pd(odd), 2, 4, 3, 1e-10, ptr(o), stream()), '8-byte aligned')):
        assert L.sg_lpips_layer_bwd(*args) < 0
        err = L.sg_last_error_string().decode()
        assert 'sg_lpips_layer_bwd' in err and msg in err, (msg, err)
    torch.cuda.synchronize()
    assert not bool(o.any())                                                            # nothing was launched


# =====================================================================================================================================
# 2. the scaling layer's backward
# =====================================================================================================================================
@pytest.mark.parametrize('shape', R.INPUT_BWD)
def test_lpips_input_bwd_bit_exact(shape):
    rs = np.random.RandomState(sum(shape))
    gy = (rs.randn(*shape) * 10.0 ** rs.randint(-6, 3, shape)).astype(np.float32)
    gy.reshape(-1)[:2] = (0.0, -1.0)
    got = ops.lpips_input_bwd(torch.from_numpy(gy).to(DEV))
    assert got.dtype == torch.float32 and np.array_equal(bits(got.cpu().numpy()), bits(R.input_bwd_np(gy)))
    x = torch.from_numpy((rs.rand(*shape) * 2 - 1).astype(np.float32)).to(DEV).requires_grad_(True)
    y = ops.LpipsInputFn.apply(x)
    assert torch.equal(y, ops.lpips_input(x.detach()))
    y.backward(torch.from_numpy(gy).to(DEV))
    assert torch.equal(x.grad, got)
    with pytest.raises(TypeError):
        ops.lpips_input_bwd(torch.zeros(1, 3, 2, 2, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        ops.lpips_input_bwd(torch.zeros(1, 4, 2, 2, device=DEV))
    assert tuple(ops.lpips_input_bwd(torch.zeros(0, 3, 2, 2, device=DEV)).shape) == (0, 3, 2, 2)


# =====================================================================================================================================
# 3. the distance as an autograd function, the loss
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _weights():
    return LR.random_backbone('vgg', 22), LR.random_lins('vgg', 23)


@pytest.mark.parametrize('weighted', [True, False], ids=['lin', 'unweighted'])
def test_distance_fn_forward_is_lpips_forward(weighted):
    sd, lins = _weights()
    lp = LP.LPIPS('vgg', backbone_weights=sd, lin_weights=LR.lin_state_dict(lins) if weighted else None, device=DEV)
    x0, x1 = R.pictures(2, 32, 7).to(DEV), R.pictures(2, 32, 8).to(DEV)
    want = lp(x0, x1)
    taps = lp.net(ops.lpips_input(torch.cat([x0, x1])))                              # the taps LPIPS.forward takes of these pictures
    fx = [t[:2].clone().requires_grad_(True) for t in taps]
    fy = [t[2:] for t in taps]
    got = ops.LpipsDistanceFn.apply(ops.LPIPS_EPS, *fx, *fy, *[lp.lin(k) for k in range(5)])
    assert got.dtype == torch.float64 and got.requires_grad and float(want.min()) > 0
    assert got.detach().cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    # its backward is one lpips_layer_bwd per tap on the incoming float64 gradient; nothing for targets and weights
    gout = torch.tensor([0.75, -1.5], dtype=torch.float64, device=DEV)
    before = ops.CALLS[0]
    got.backward(gout)
    assert ops.CALLS[0] == before + 5
    for k in range(5):
        assert torch.equal(fx[k].grad, ops.lpips_layer_bwd(fx[k].detach(), fy[k], lp.lin(k), gout))
        assert fy[k].grad is None


@functools.lru_cache(maxsize=None)
def _loss_case(input, weighted):
    sd, lins = _weights()
    x, y = R.pictures(2, 32, 7), R.pictures(2, 32, 8)
    if input == 'imagenet':
        x, y = R.imagenet_normalize(x), R.imagenet_normalize(y)
    ww = lins if weighted else None
    return x, y, R.loss_ref(sd, ww, x, y, torch.float64, input), R.loss_ref(sd, ww, x, y, torch.float32, input)


@pytest.mark.parametrize('weighted', [True, False], ids=['lin', 'unweighted'])
@pytest.mark.parametrize('input', ['imagenet', 'unit'])
def test_lpips_loss_value_and_gradient(input, weighted, capsys):
    sd, lins = _weights()
    x, y, (v64, g64), (v32, g32) = _loss_case(input, weighted)
    m = LP.LPIPSLoss(backbone_weights=sd, lin_weights=LR.lin_state_dict(lins) if weighted else None, input=input, device=DEV)
    assert ('DO NOT COMPARE' in capsys.readouterr().err) == (not weighted)
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    loss = m(xd, yd)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad and float(v64) > 1e-3
    loss.backward()
    tag = '%s %s' % (input, 'lin' if weighted else 'w = 1')
    check('loss_value', tag, loss.detach(), v64, v32)
    assert float(g64.abs().max()) > 0
    check('loss_grad', tag, xd.grad, g64, g32)
    assert yd.grad is None and all(p.grad is None and not p.requires_grad for p in m.parameters())
    # the same pictures again: the same bits, value and gradient
    x2 = x.to(DEV).requires_grad_(True)
    l2 = m(x2, y.to(DEV))
    l2.backward()
    assert torch.equal(l2, loss) and torch.equal(x2.grad, xd.grad)
    # a picture against itself: exactly 0, with a gradient of exactly 0
    x3 = x.to(DEV).requires_grad_(True)
    l3 = m(x3, x.to(DEV))
    l3.backward()
    assert float(l3) == 0.0 and not bool(x3.grad.any())
    # under no_grad nothing is recorded
    with torch.no_grad():
        assert torch.equal(m(xd, yd), loss) and not m(xd, yd).requires_grad
    with pytest.raises(ValueError, match='LPIPSLoss'):
        m(xd, yd[:1])


# =====================================================================================================================================
# 4. the Trainer's switch
# =====================================================================================================================================
def _one_step(tr, batch):
    random.seed(0)
    out = tr.step(batch, use_gt=TH.USE_GT[0])
    torch.cuda.synchronize()
    return out, dict(tr.generator_losses.items())


def test_trainer_with_the_lpips_term(monkeypatch):
    monkeypatch.delenv('SG_LPIPS_LOSS', raising=False)
    sd, lins = _weights()
    batch = TH._batch()
    on, _, _ = TH._trainer(lpips_loss={'weight': 0.5, 'backbone': sd, 'lin': LR.lin_state_dict(lins)})
    plain, _, _ = TH._trainer()
    off, _, _ = TH._trainer(lpips_loss=False)
    assert plain.criterionLPIPS is None and off.criterionLPIPS is None and isinstance(on.criterionLPIPS, LP.LPIPSLoss)
    p0 = on.optimizer.fp.flat.clone()
    assert torch.equal(p0, plain.optimizer.fp.flat)
    out_on, l_on = _one_step(on, batch)
    out_plain, l_plain = _one_step(plain, batch)
    _, l_off = _one_step(off, batch)
    # off: the losses and every parameter after the step are those of a Trainer built without the argument
    assert 'g_lpips' not in l_plain and l_off == l_plain and list(l_off) == list(l_plain)
    for (_, a), (_, b) in zip(off.named_optimizers(), plain.named_optimizers()):
        assert torch.equal(a.fp.flat, b.fp.flat) and torch.equal(a.exp_avg, b.exp_avg)
    # on: the term sits next to the others, which are the plain run's (the forward is the same)
    assert set(l_on) == set(l_plain) | {'g_lpips'} and torch.equal(out_on[0], out_plain[0])
    assert all(l_on[k] == l_plain[k] for k in l_plain if k != 'total_loss')
    imgs_pred, imgs = out_on[0].detach(), batch[0]
    direct = on.criterionLPIPS(imgs_pred, imgs)
    assert l_on['g_lpips'] == 0.5 * float(direct) > 0
    v64, _ = R.loss_ref(sd, lins, imgs_pred.cpu(), imgs.cpu(), torch.float64)
    v32, _ = R.loss_ref(sd, lins, imgs_pred.cpu(), imgs.cpu(), torch.float32)
    check('trainer', 'g_lpips of one step', torch.tensor(l_on['g_lpips'], dtype=torch.float64), 0.5 * v64, 0.5 * v32.double())
    assert abs(l_on['total_loss'] - (l_plain['total_loss'] + l_on['g_lpips'])) <= 1e-5 * abs(l_on['total_loss'])
    # the generator's gradient and step differ; the backbone took no gradient and moved nowhere
    assert not torch.equal(on.optimizer.fp.grad, plain.optimizer.fp.grad) and bool(torch.isfinite(on.optimizer.fp.grad).all())
    assert not torch.equal(on.optimizer.fp.flat, plain.optimizer.fp.flat)
    assert all(p.grad is None for p in on.criterionLPIPS.parameters())
    assert torch.equal(on.criterionLPIPS.net.state_dict()['features.0.weight'].cpu(), sd['features.0.weight'])
