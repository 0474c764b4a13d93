"""The opt-in bf16 residual trunk on the GPU: sg_conv3x3r_bf16_* against a float64 reference on bf16-rounded operands, proof
that the operands really are rounded, determinism, hipGraph capture of a bf16-trunk GlobalGenerator, and a bf16 Trainer
against an fp32 one from the same state."""
import copy
import functools
import math
import random

import pytest
import torch
import torch.nn.functional as F

from scene_generation_amd import graphs, ops
from scene_generation_amd.args import parser
from scene_generation_amd.generators import GlobalGenerator
from scene_generation_amd.layers import InstanceNorm2d
from scene_generation_amd.synthetic import batch_to, fill_deterministic, make_batch, make_vocab
from scene_generation_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(2, 64, 8, 8), (3, 64, 5, 7), (2, 128, 2, 2), (4, 256, 8, 8), (8, 1024, 16, 16), (32, 1024, 8, 8)]


def _data(shape, seed=0):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C)
    b = torch.randn(C, generator=g) * 0.1
    gy = torch.randn(N, C, H, W, generator=g)
    return x, w, b, gy


def _reference(x, w, b, gy, rounded):
    """float64 forward + autograd on the CPU; ``rounded``: the operands of every product rounded to bf16 first"""
    r = (lambda t: t.to(torch.bfloat16).double()) if rounded else (lambda t: t.double())
    xr = r(x).requires_grad_(True)
    wr = r(w).requires_grad_(True)
    br = b.double().requires_grad_(True)
    y = F.conv2d(F.pad(xr, (1, 1, 1, 1), mode='reflect'), wr, br)
    # each backward GEMM multiplies gy with w (dgrad) or x (wgrad): with bf16 operands gy is rounded too (the bias gradient is
    # a plain fp32 sum of gy, not a product)
    gyr = r(gy)
    gx, gw = torch.autograd.grad(y, (xr, wr), gyr)
    return y.detach(), gx, gw, gy.double().sum((0, 2, 3))


@functools.lru_cache(maxsize=None)
def _case(shape):
    x, w, b, gy = _data(shape)
    return (x, w, b, gy), _reference(x, w, b, gy, True), _reference(x, w, b, gy, False)


def _gpu(x, w, b, gy):
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True)
    y = ops.conv3x3_reflect_bf16(xd, wd, bd)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return y.detach().cpu(), xd.grad.cpu(), wd.grad.cpu(), bd.grad.cpu()


def _rel(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_matches_rounded_fp64_reference(shape):
    (x, w, b, gy), ref, _ = _case(shape)
    assert ops.conv3x3_reflect_bf16_supported(x.to(DEV), w.to(DEV))
    got = _gpu(x, w, b, gy)
    for name, a, r in zip(('y', 'gx', 'gw', 'gb'), got, ref):
        assert a.shape == r.shape, name
        assert _rel(a, r) <= 1e-5, (name, _rel(a, r))


@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_operands_really_are_bf16(shape):
    """against the UNROUNDED fp64 reference the error is the bf16 operand rounding (~1e-3 relative per product), far above
    what the fp32 paths reach (<= 1e-5): this fails on any path that multiplies fp32 operands"""
    (x, w, b, gy), _, exact = _case(shape)
    got = _gpu(x, w, b, gy)
    for name, a, r in zip(('y', 'gx', 'gw'), got[:3], exact[:3]):
        assert _rel(a, r) > 1e-4, (name, _rel(a, r))


@pytest.mark.parametrize('shape', [(2, 64, 8, 8), (8, 1024, 16, 16), (32, 1024, 8, 8)])
def test_kernel_deterministic(shape):
    x, w, b, gy = _data(shape, seed=1)
    a, c = _gpu(x, w, b, gy), _gpu(x, w, b, gy)
    for name, u, v in zip(('y', 'gx', 'gw', 'gb'), a, c):
        assert torch.equal(u, v), name


def test_unsupported_shapes_rejected():
    w = torch.zeros(96, 96, 3, 3, device=DEV)
    assert not ops.conv3x3_reflect_bf16_supported(torch.zeros(2, 96, 8, 8, device=DEV), w)      # C % 64 != 0
    w = torch.zeros(64, 64, 3, 3, device=DEV)
    assert not ops.conv3x3_reflect_bf16_supported(torch.zeros(2, 64, 1, 8, device=DEV), w)      # H < 2
    with pytest.raises(ValueError):
        ops.conv3x3_reflect_bf16(torch.zeros(2, 64, 1, 8, device=DEV), w)


def _generator(ngf, n_down, seed=0):
    torch.manual_seed(seed)
    g = GlobalGenerator(5, 3, ngf=ngf, n_downsampling=n_down, n_blocks=9, norm_layer=InstanceNorm2d).to(DEV)
    fill_deterministic(g)
    return g


def test_generator_graph_replay_matches_eager():
    g = _generator(16, 2)                                  # trunk: 64 channels at 8x8
    g.set_trunk_precision('bf16')
    x = torch.randn(2, 5, 32, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    saved = graphs.ENABLED
    try:
        with torch.no_grad():
            graphs.ENABLED = False
            eager = g(x).clone()
            graphs.ENABLED = True
            outs = [g(x).clone() for _ in range(4)]        # 2 eager warm-ups, capture, replay
        torch.cuda.synchronize()
    finally:
        graphs.ENABLED = saved
    assert any(e for seg in g._tail for e in seg.entries.values()), 'no segment was captured'
    for o in outs:
        assert torch.equal(o, eager)
    assert g.trunk_paths() == ['bf16'] * 9
    with pytest.raises(RuntimeError):
        g.set_trunk_precision('fp32')
    # against the fp32 trunk the image differs, but only by the operand rounding
    f = _generator(16, 2)
    with torch.no_grad():
        ref = f(x)
    assert f.trunk_paths() == ['fp32'] * 9
    assert not torch.equal(ref, eager) and float((ref - eager).abs().max()) < 0.05


@pytest.mark.parametrize('N,size', [(32, 128), (8, 256)])
def test_generator_paths_at_benchmark_shapes(N, size):
    g = _generator(64, 4)                                  # trunk: 1024 channels at size / 16
    g.set_trunk_precision('bf16')
    x = torch.randn(N, 5, size, size, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        y = g(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    assert g.trunk_paths() == ['bf16'] * 9


ARGV = ['--image_size', '32,32', '--batch_size', '3', '--vgg_features_weight', '0', '--output_dir', '/tmp/o',
        '--n_downsample_global', '2', '--gconv_hidden_dim', '64', '--gconv_num_layers', '3', '--mask_size', '8',
        '--ndf', '8', '--ndf_mask', '8', '--crop_size', '16', '--d_obj_arch', 'C4-8-2,C4-16-2', '--pool_size', '2']


def _trainer(precision):
    args = parser.parse_args(ARGV)
    ck = {'model_kwargs': {}, 'd_obj_kwargs': {}, 'd_mask_kwargs': {}, 'd_img_kwargs': {}}
    tr = Trainer(args, make_vocab(12, 4, 35), checkpoint=ck, device=DEV, trunk_precision=precision)
    for m in (tr.model, tr.netD, tr.obj_discriminator, tr.mask_discriminator):
        if m is not None:
            fill_deterministic(m)
    tr.model.noise_override = torch.linspace(-1, 1, args.mask_noise_dim).view(1, -1)
    return tr, ck


def _trunk_grads(tr):
    """gradients of the trunk conv WEIGHTS (a conv bias ahead of InstanceNorm has a mathematically zero gradient: what either
    precision returns for it is rounding noise, ~1e-8, with no direction to compare)"""
    opt = tr.optimizer
    trunk = [p for m in tr.model.layout_to_image.model if type(m).__name__ == 'ResnetBlock'
             for n, p in m.named_parameters() if n.endswith('weight')]
    idx = {id(p): i for i, p in enumerate(opt.fp.params)}
    return [opt.scaled_grad(idx[id(p)]).double().flatten() for p in trunk]


def test_trainer_bf16_against_fp32():
    batch = batch_to(make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=12, num_preds=4, seed=100), DEV)
    t16, ck16 = _trainer('bf16')
    t32, ck32 = _trainer('fp32')
    assert ck16['model_kwargs'] == ck32['model_kwargs']
    random.seed(0)
    t32.step(batch, use_gt=True)
    torch.cuda.synchronize()
    l32, g32 = dict(t32.generator_losses.items()), _trunk_grads(t32)
    random.seed(0)
    t16.step(batch, use_gt=True)
    torch.cuda.synchronize()
    l16, g16 = dict(t16.generator_losses.items()), _trunk_grads(t16)
    assert t16.model.layout_to_image.trunk_paths() == ['bf16'] * 9
    assert t32.model.layout_to_image.trunk_paths() == ['fp32'] * 9
    assert set(l16) == set(l32)
    for k in l32:
        assert math.isfinite(l16[k]), k
        assert abs(l16[k] - l32[k]) <= 0.02 * max(abs(l32[k]), 1e-3), (k, l16[k], l32[k])
    # Measured on MI355X: cosine 0.980-0.986 for all 18 weights, flat over the depth (the last block, first in the backward, is
    # no better than the first), while an fp32 rerun is bitwise equal and the kernels match the fp64 reference on rounded
    # operands to 1e-5.  So it is the bf16 rounding of each weight gradient's own operands, amplified by cancellation: the
    # gradient reaching a conv through InstanceNorm is orthogonal per plane to the normalised conv output, so gW = sum gy x is
    # a small difference of large terms (here over only N*H*W = 192 pixels).  The bound keeps a margin under that measurement.
    for i, (a, b) in enumerate(zip(g16, g32)):
        cos = float(a @ b / (a.norm() * b.norm()).clamp_min(1e-30))
        assert cos >= 0.97, (i, cos)
    for s in range(4):
        random.seed(1 + s)
        t16.step(batch, use_gt=True)
    torch.cuda.synchronize()
    for k, v in t16.generator_losses.items():
        assert math.isfinite(v), k
    # the checkpointed model is the fp32 model's: same kwargs, same keys, loads into an fp32 Trainer
    sd = t16.model.state_dict()
    assert sorted(sd) == sorted(t32.model.state_dict())
    t32.model.load_state_dict(copy.deepcopy(sd))
    for k, v in t32.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
