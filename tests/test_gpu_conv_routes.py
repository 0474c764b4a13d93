"""Which C-ABI entry points one forward and one backward of every conv / dense operator issues, in order, at the smallest shape
that reaches each kernel route -- and, so that a matching trace with the wrong buffer written cannot pass, the outputs and
gradients against torch in fp64 at the tolerance tests/test_gpu_parity.py uses for the operator.

The parameters are plain tensors (no FusedAdam sinks), so no sg_axpy appears.  The expected lists are written out literally."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from gpu_harness import close
from tools_det import det

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'gpu tests need a device'
    from scene_generation_amd import ops, _hip
    _hip.lib()
    return ops


@contextlib.contextmanager
def recording(ops):
    """the names of the C-ABI calls issued inside the block (ops._call wrapped: the ops namespace hands the wrapper to every
    operator module; the calls still go through)"""
    names, real = [], ops._call

    def recorder(name, *args):
        names.append(name)
        return real(name, *args)
    ops._call = recorder
    try:
        yield names
    finally:
        ops._call = real


ACTS = {0: lambda t: t, 1: F.relu, 2: lambda t: F.leaky_relu(t, 0.2)}


def ref_backward(ypre, yg, gy, act):
    """fp64 reference backward from the pre-activation ``ypre``.  (Leaky)ReLU: with the derivative mask of the GPU result ``yg``,
    after checking that every unit the two masks disagree on is within the forward tolerance of the kink (a unit at rounding
    distance from 0 may sit on either side in two correct implementations)."""
    if act == 0:
        ypre.backward(gy.double())
        return
    lo = 0.0 if act == 1 else 0.2
    one, low = torch.tensor(1.0, dtype=torch.float64), torch.tensor(lo, dtype=torch.float64)
    dg = torch.where(yg.detach().cpu() > 0, one, low)
    flipped = dg != torch.where(ypre.detach() > 0, one, low)
    assert float(ypre.detach()[flipped].abs().max() if flipped.any() else 0.0) <= 3e-5 * max(1.0, float(ypre.detach().abs().max()))
    ypre.backward(gy.double() * dg)


def conv_ref(x, w, b, stride=1, pad=0, reflect=False, ups=1):
    if ups == 2:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    if reflect:
        return F.conv2d(F.pad(x, (pad,) * 4, mode='reflect'), w, b, stride=stride)
    return F.conv2d(x, w, b, stride=stride, padding=pad)


def leaves(*ts):
    return [t.double().requires_grad_() for t in ts], [t.to(DEV).requires_grad_() for t in ts]


# id: (N, C1, H, Cout, KS, pad, reflect, act, hint, forward calls, backward calls)
CONV2D = {
    'generic': (1, 3, 4, 8, 3, 1, False, 0, None, ['sg_conv2d_fwd'], ['sg_conv2d_dgrad', 'sg_conv2d_wgrad']),
    'generic_reflect': (1, 3, 4, 8, 3, 1, True, 0, None, ['sg_conv2d_fwd'], ['sg_conv2d_dgrad_folded', 'sg_conv2d_wgrad']),
    'generic_relu': (1, 3, 4, 8, 3, 1, False, 1, None, ['sg_conv2d_fwd'], ['sg_act_bwd', 'sg_conv2d_dgrad', 'sg_conv2d_wgrad']),
    'sparse': (1, 8, 4, 8, 3, 1, False, 0, 'sparse', ['sg_conv2d_fwd_sparse'], ['sg_conv2d_dgrad', 'sg_conv2d_wgrad_sparse']),
    'head': (1, 16, 4, 1, 1, 0, False, 0, None, ['sg_conv2d_head_fwd'],
             ['sg_conv2d_head_dgrad', 'sg_conv2d_head_wgrad', 'sg_channel_sum']),
    'smallm': (1, 3, 4, 3, 7, 3, True, 0, None, ['sg_conv2d_smallm_fwd'],
               ['sg_conv2d_dgrad', 'sg_pad_upsample_bwd', 'sg_conv2d_smallm_wgrad', 'sg_channel_sum']),
    'wino': (2, 128, 16, 128, 3, 1, True, 0, None, ['sg_conv2d_wino_fwd'],
             ['sg_conv2d_wino_dgrad', 'sg_conv2d_wino_wgrad', 'sg_channel_sum']),
    # the hint keeps the Winograd data gradient (full channel range only) out; the weight gradient stays, without saved operands
    'wino_grad_from': (2, 128, 16, 128, 3, 1, True, 0, 'grad_from', ['sg_conv2d_wino_fwd'],
                       ['sg_conv2d_dgrad_folded', 'sg_conv2d_wino_wgrad', 'sg_channel_sum']),
    'wino24': (1, 128, 31, 128, 4, 2, False, 0, None, ['sg_conv2d_wino24_fwd'],
               ['sg_conv2d_wino24_dgrad', 'sg_conv2d_wino24_wgrad', 'sg_channel_sum']),
}
GRAD_FROM = 64


@pytest.mark.parametrize('case', sorted(CONV2D))
def test_conv2d_route_calls(ops, case):
    N, C1, H, Cout, KS, pad, reflect, act, hint, fwd_calls, bwd_calls = CONV2D[case]
    x, w, b = det((N, C1, H, H), 711), det((Cout, C1, KS, KS), 712, 0.2), det((Cout,), 713, 0.2)
    if hint == 'sparse':        # channels 1 and 5 listed: every other one is zero, as the hint promises
        x[:, [0, 2, 3, 4, 6, 7]] = 0
    (xr, wr, br), (xg, wg, bg) = leaves(x, w, b)
    ypre = conv_ref(xr, wr, br, 1, pad, reflect)
    gy = det(tuple(ypre.shape), 714)
    gyd = gy.to(DEV)
    try:
        if hint == 'sparse':
            ops.set_hints(xg, sparse=(torch.tensor([[1, 5]] * N, dtype=torch.int32, device=DEV),
                                      torch.full((N,), 2, dtype=torch.int32, device=DEV)))
        elif hint == 'grad_from':
            ops.set_hints(xg, grad_from=GRAD_FROM)
        with recording(ops) as fwd:
            yg = ops.conv2d(xg, wg, bg, stride=1, pad=pad, reflect=reflect, act=act, slope=0.2)
        with recording(ops) as bwd:
            yg.backward(gyd)
    finally:
        ops.clear_hints()
    assert fwd == fwd_calls
    assert bwd == bwd_calls
    ref_backward(ypre, yg, gy, act)
    close(yg, ACTS[act](ypre).detach().float(), 3e-5, 'y')
    if hint == 'grad_from':      # nobody needs d/dx of the constant channels: zeros there
        assert not xg.grad[:, :GRAD_FROM].any()
        close(xg.grad[:, GRAD_FROM:], xr.grad[:, GRAD_FROM:].float(), 5e-5, 'gx')
    else:
        close(xg.grad, xr.grad.float(), 5e-5, 'gx')
    close(wg.grad, wr.grad.float(), 5e-5, 'gw')
    close(bg.grad, br.grad.float(), 5e-5, 'gb')


@pytest.mark.parametrize('case,dgrad', [('generic', 'sg_conv2d_dgrad'), ('head', 'sg_conv2d_head_dgrad')])
def test_bias_only_backward_calls(ops, case, dgrad):
    """the weight under skip_param_grads: the data gradient, then ONE sg_channel_sum; no weight gradient is computed or returned"""
    N, C1, H, Cout, KS, pad, reflect, act = CONV2D[case][:8]
    x, w, b = det((N, C1, H, H), 721), det((Cout, C1, KS, KS), 722, 0.2), det((Cout,), 723, 0.2)
    (xr, wr, br), (xg, wg, bg) = leaves(x, w, b)
    yr = conv_ref(xr, wr, br, 1, pad, reflect)
    gy = det(tuple(yr.shape), 724)
    gyd = gy.to(DEV)
    yg = ops.conv2d(xg, wg, bg, stride=1, pad=pad, reflect=reflect)
    with ops.skip_param_grads([wg]), recording(ops) as bwd:
        yg.backward(gyd)
    assert bwd == [dgrad, 'sg_channel_sum']
    assert wg.grad is None
    yr.backward(gy.double())
    close(xg.grad, xr.grad.float(), 5e-5, 'gx')
    close(bg.grad, br.grad.float(), 5e-5, 'gb')


def test_conv_instnorm_calls(ops):
    N, C, H = 4, 128, 16
    x, w, b = det((N, C, H, H), 731), det((C, C, 3, 3), 732, 0.1), det((C,), 733, 0.2)
    assert ops.conv_instnorm_fusable(torch.empty(N, C, H, H, device=DEV), w, 1, 1, 0)
    (xr, wr, br), (xg, wg, bg) = leaves(x, w, b)
    yr = F.instance_norm(conv_ref(xr, wr, br, 1, 1, True), eps=1e-5)
    gy = det(tuple(yr.shape), 734)
    gyd = gy.to(DEV)
    with recording(ops) as fwd:
        yg = ops.conv2d_instnorm(xg, wg, bg, eps=1e-5)
    with recording(ops) as bwd:
        yg.backward(gyd)
    assert fwd == ['sg_conv2d_wino_fwd_instnorm']
    assert bwd == ['sg_conv2d_wino_dgrad_instnorm', 'sg_conv2d_wino_wgrad']
    yr.backward(gy.double())
    close(yg, yr.detach().float(), 5e-5, 'out')
    close(xg.grad, xr.grad.float(), 1e-4, 'gx')
    close(wg.grad, wr.grad.float(), 1e-4, 'gw')
    # the conv bias is followed by a mean subtraction: its gradient is rounding noise around 0 in every implementation
    assert float(bg.grad.abs().max()) <= 1e-3 * float(gy.abs().sum(dim=(0, 2, 3)).max())


def test_conv_transpose2d_calls(ops):
    x, w, b = det((2, 16, 8, 8), 741), det((16, 8, 3, 3), 742, 0.2), det((8,), 743, 0.2)
    (xr, wr, br), (xg, wg, bg) = leaves(x, w, b)
    yr = F.conv_transpose2d(xr, wr, br, stride=2, padding=1, output_padding=1)
    gy = det(tuple(yr.shape), 744)
    gyd = gy.to(DEV)
    with recording(ops) as fwd:
        yg = ops.conv_transpose2d(xg, wg, bg, stride=2, pad=1, out_pad=1)
    with recording(ops) as bwd:
        yg.backward(gyd)
    assert fwd == ['sg_convT2d_fwd']
    assert bwd == ['sg_convT2d_dgrad', 'sg_convT2d_wgrad']
    yr.backward(gy.double())
    close(yg, yr.detach().float(), 3e-5, 'y')
    close(xg.grad, xr.grad.float(), 5e-5, 'gx')
    close(wg.grad, wr.grad.float(), 5e-5, 'gw')
    close(bg.grad, br.grad.float(), 5e-5, 'gb')


def test_upconv3_calls(ops):
    """Interpolate(x2) + Conv3x3(pad 1) below the Winograd widths: the sub-pixel transposed-conv form"""
    x, w, b = det((1, 4, 5, 5), 751), det((6, 4, 3, 3), 752, 0.2), det((6,), 753, 0.2)
    (xr, wr, br), (xg, wg, bg) = leaves(x, w, b)
    yr = conv_ref(xr, wr, br, 1, 1, False, ups=2)
    gy = det(tuple(yr.shape), 754)
    gyd = gy.to(DEV)
    assert ops.UPCONV
    with recording(ops) as fwd:
        yg = ops.conv2d(xg, wg, bg, stride=1, pad=1, upsample=2)
    with recording(ops) as bwd:
        yg.backward(gyd)
    assert fwd == ['sg_upconv3_fold_weights', 'sg_convT2d_fwd']
    assert bwd == ['sg_convT2d_dgrad', 'sg_convT2d_wgrad', 'sg_upconv3_unfold_wgrad']
    yr.backward(gy.double())
    close(yg, yr.detach().float(), 3e-5, 'y')
    close(xg.grad, xr.grad.float(), 5e-5, 'gx')
    close(wg.grad, wr.grad.float(), 5e-5, 'gw')
    close(bg.grad, br.grad.float(), 5e-5, 'gb')


def test_cond_conv2d_calls(ops):
    """a per-sample row as second source of a zero-padded conv: the constant channels folded into a per-tap term"""
    N, C1, C2, H, Cout = 2, 6, 5, 5, 8
    x, cond = det((N, C1, H, H), 761), det((N, C2), 765)
    w, b = det((Cout, C1 + C2, 3, 3), 762, 0.2), det((Cout,), 763, 0.2)
    (xr, cr, wr, br), (xg, cg, wg, bg) = leaves(x, cond, w, b)
    yr = F.conv2d(torch.cat([xr, cr.view(N, C2, 1, 1).expand(-1, -1, H, H)], 1), wr, br, padding=1)
    gy = det(tuple(yr.shape), 764)
    gyd = gy.to(DEV)
    assert ops.COND_FOLD
    with recording(ops) as fwd:
        yg = ops.conv2d(xg, wg, bg, stride=1, pad=1, x2=cg)
    with recording(ops) as bwd:
        yg.backward(gyd)
    assert fwd == ['sg_cond_conv_split_w', 'sg_linear_fwd', 'sg_conv2d_fwd', 'sg_cond_conv_bias_act']
    assert bwd == ['sg_conv2d_dgrad', 'sg_cond_conv_window_sums', 'sg_linear_bwd_data', 'sg_conv2d_wgrad', 'sg_linear_bwd_weight',
                   'sg_cond_conv_merge_w']
    yr.backward(gy.double())
    close(yg, yr.detach().float(), 3e-5, 'y')
    close(xg.grad, xr.grad.float(), 5e-5, 'gx')
    close(cg.grad, cr.grad.float(), 5e-5, 'gcond')
    close(wg.grad, wr.grad.float(), 5e-5, 'gw')
    close(bg.grad, br.grad.float(), 5e-5, 'gb')


@pytest.mark.parametrize('skip_weight', [False, True])
def test_linear_calls(ops, skip_weight):
    x, w, b = det((9, 13), 771), det((7, 13), 772, 0.1), det((7,), 773, 0.1)
    (xr, wr, br), (xg, wg, bg) = leaves(x, w, b)
    ypre = F.linear(xr, wr, br)
    gy = det(tuple(ypre.shape), 774)
    gyd = gy.to(DEV)
    with recording(ops) as fwd:
        yg = ops.linear(xg, wg, bg, act=1)
    with contextlib.ExitStack() as stack:
        if skip_weight:
            stack.enter_context(ops.skip_param_grads([wg]))
        bwd = stack.enter_context(recording(ops))
        yg.backward(gyd)
    assert fwd == ['sg_linear_fwd']
    assert bwd == ['sg_act_bwd', 'sg_linear_bwd_data'] + (['sg_channel_sum'] if skip_weight else ['sg_linear_bwd_weight'])
    ref_backward(ypre, yg, gy, 1)
    close(yg, F.relu(ypre).detach().float(), 2e-5, 'y')
    close(xg.grad, xr.grad.float(), 2e-5, 'gx')
    close(bg.grad, br.grad.float(), 2e-5, 'gb')
    if skip_weight:
        assert wg.grad is None
    else:
        close(wg.grad, wr.grad.float(), 2e-5, 'gw')


def test_factored_layout_conv_calls(ops):
    """a conv over a layout given in factored form (planes x per-object vectors), fused LeakyReLU: per-image filters, the
    per-image-weight conv, and in the backward the activation, the per-image filter gradient, the bias sum and the filters' adjoint"""
    N, J, H, num_objs, R, Cout = 2, 2, 6, 5, 3, 8
    img_idx, plane_idx = [0, 0, 1], [0, 1, 0]
    objs = torch.tensor([1, 4, 2])
    Z, rep = det((N, J, H, H), 781).abs(), det((3, R), 782).abs()
    w, b = det((Cout, num_objs + R, 3, 3), 783, 0.2), det((Cout,), 784, 0.2)
    (wr, br), (wg, bg) = leaves(w, b)
    vecs = torch.cat([F.one_hot(objs, num_objs).double(), rep.double()], 1)
    dense = torch.zeros(N, num_objs + R, H, H, dtype=torch.float64)
    for o, (n, j) in enumerate(zip(img_idx, plane_idx)):
        dense[n] += vecs[o].view(-1, 1, 1) * Z[n, j].double()
    ypre = conv_ref(dense, wr, br, 1, 1, False)
    gy = det(tuple(ypre.shape), 785)
    gyd = gy.to(DEV)
    f = ops.FactoredLayout(Z.to(DEV), objs.to(DEV), rep.to(DEV), num_objs, torch.tensor(img_idx, device=DEV),
                           torch.tensor(plane_idx, device=DEV), [2, 1])
    f.lists(0)                        # (host-built index lists, copied once per layout: not part of the conv's calls)
    layout = torch.empty(N, num_objs + R, H, H, device=DEV)          # never read: the factored form stands for it
    assert ops.FACTORED_LAYOUT
    try:
        ops.set_hints(layout, factored=f)
        with recording(ops) as fwd:
            yg = ops.conv2d(layout, wg, bg, stride=1, pad=1, act=2, slope=0.2)
        with recording(ops) as bwd:
            yg.backward(gyd)
    finally:
        ops.clear_hints()
    assert fwd == ['sg_factored_weights_fwd', 'sg_conv2d_fwd_perimage']
    assert bwd == ['sg_act_bwd', 'sg_conv2d_wgrad_perimage', 'sg_channel_sum', 'sg_factored_weights_bwd']
    ref_backward(ypre, yg, gy, 2)
    close(yg, ACTS[2](ypre).detach().float(), 1e-4, 'y')
    close(wg.grad, wr.grad.float(), 1e-4, 'gw')
    close(bg.grad, br.grad.float(), 1e-4, 'gb')
