"""LPIPS as a training loss without a GPU: the declarations and argument checks of the two new entry points, the closed form of the
tap gradient against float64 autograd, why the zero-norm rule exists (autograd gives NaN there, a ReLU in front drops whatever
arrives), the scaling layer as the ImageNet normalisation, SG_LPIPS_LOSS parsing and the Trainer's switch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_loss_ref as R
import lpips_ref as LR
from scene_generation_amd import _hip, ops
from scene_generation_amd import lpips as LP
from scene_generation_amd.args import parser
from scene_generation_amd.synthetic import make_vocab
from scene_generation_amd.trainer import Trainer

ARGV = ['--image_size', '32,32', '--batch_size', '2', '--vgg_features_weight', '0',
        '--n_downsample_global', '2', '--gconv_hidden_dim', '64', '--gconv_num_layers', '3', '--mask_size', '8',
        '--ndf', '8', '--ndf_mask', '8', '--crop_size', '16', '--d_obj_arch', 'C4-8-2,C4-16-2', '--pool_size', '2']


def test_header_declares_the_entry_points():
    restype, argtypes, argnames = _hip.PROTOS['sg_lpips_layer_bwd']
    assert argnames == ['f0', 'f1', 'w', 'gout', 'P', 'C', 'HW', 'eps', 'gf0', 'stream'] and restype == ctypes.c_int
    assert argtypes[3] == ctypes.POINTER(ctypes.c_double) and argtypes[7] == ctypes.c_float
    assert _hip.PROTOS['sg_lpips_input_bwd'][2] == ['gy', 'N', 'HW', 'gx', 'stream']
    for name in ('sg_lpips_layer_bwd', 'sg_lpips_input_bwd'):
        assert hasattr(_hip.lib(), name)
    for name in ('lpips_layer_bwd', 'lpips_input_bwd', 'LpipsDistanceFn', 'LpipsInputFn'):
        assert callable(getattr(ops, name))


def test_entry_points_reject_bad_arguments_before_any_launch():
    L = _hip.lib()
    buf = np.zeros(64, np.float64)
    pd = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    odd = ctypes.cast(buf.ctypes.data + 4, ctypes.POINTER(ctypes.c_double))
    x = np.zeros(64, np.float32).ctypes.data
    for args in ((None, x, None, pd, 1, 4, 4, 1e-10, x, None), (x, None, None, pd, 1, 4, 4, 1e-10, x, None),
                 (x, x, None, None, 1, 4, 4, 1e-10, x, None), (x, x, None, pd, 1, 4, 4, 1e-10, None, None),      # null operands
                 (x, x, None, pd, -1, 4, 4, 1e-10, x, None), (x, x, None, pd, 1, 0, 4, 1e-10, x, None),
                 (x, x, None, pd, 1, 4, 0, 1e-10, x, None), (x, x, None, pd, 1 << 20, 1 << 10, 4, 1e-10, x, None),  # sizes, 2^31
                 (x, x, None, pd, 1, 4, 4, -1.0, x, None),                                                    # eps < 0
                 (x, x, None, odd, 1, 4, 4, 1e-10, x, None)):                                                 # misaligned gout
        assert L.sg_lpips_layer_bwd(*args) < 0 and 'sg_lpips_layer_bwd' in _hip.last_error(), args
    assert L.sg_lpips_layer_bwd(None, None, None, None, 0, 4, 4, 1e-10, None, None) == 0                      # P == 0: nothing to do
    assert L.sg_lpips_input_bwd(None, 1, 4, x, None) < 0 and 'sg_lpips_input_bwd' in _hip.last_error()
    assert L.sg_lpips_input_bwd(x, 1, 4, None, None) < 0
    assert L.sg_lpips_input_bwd(x, 1, 0, x, None) < 0 and L.sg_lpips_input_bwd(x, -1, 4, x, None) < 0
    assert L.sg_lpips_input_bwd(None, 0, 4, None, None) == 0


def test_wrappers_have_no_cpu_fallback():
    f = torch.zeros(1, 4, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.lpips_layer_bwd(f, f, None, torch.zeros(1, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.lpips_input_bwd(torch.zeros(1, 3, 2, 2))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        LP.LPIPSLoss(device='cpu')(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))


# ---- the closed form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 5, 7), (2, 65, 35), (1, 520, 9)])
@pytest.mark.parametrize('weighted', [True, False])
def test_closed_form_is_the_float64_autograd(shape, weighted):
    f0, f1, w, gout = R.layer_inputs(shape)
    w = w if weighted else None
    auto = R.layer_grad_autograd(f0, f1, w, gout, torch.float64).numpy()
    closed = R.layer_grad_closed(f0.numpy(), f1.numpy(), None if w is None else w.numpy(), gout.numpy(), np.float64)
    scale = np.abs(auto).max()
    assert scale > 0 and np.abs(auto - closed).max() <= 1e-13 * scale                # (the issue's check found 6e-17 absolute)
    # ... and the float32 closed form is a float32 evaluation of it
    c32 = R.layer_grad_closed(f0.numpy(), f1.numpy(), None if w is None else w.numpy(), gout.numpy(), np.float32)
    assert c32.dtype == np.float32 and np.abs(c32 - closed).max() <= 64 * 2.0 ** -24 * scale
    # the same features on both sides: t = 0 and a gradient of exactly 0
    same = R.layer_grad_closed(f0.numpy(), f0.numpy(), None if w is None else w.numpy(), gout.numpy(), np.float32)
    assert not same.any()


def test_zero_pixel_autograd_is_nan_and_the_closed_form_is_finite():
    f0, f1, w, gout = R.layer_inputs((2, 5, 7))
    f0 = f0.clone()
    f0[:, :, 3] = 0
    auto = R.layer_grad_autograd(f0, f1, w, gout, torch.float64)
    assert bool(torch.isnan(auto[:, :, 3]).all())                                    # sqrt'(0) = inf, times 2 * 0: NaN
    keep = [j for j in range(7) if j != 3]
    assert bool(torch.isfinite(auto[:, :, keep]).all())
    for dt in (np.float64, np.float32):
        closed = R.layer_grad_closed(f0.numpy(), f1.numpy(), w.numpy(), gout.numpy(), dt)
        assert np.isfinite(closed).all()
        # there it is g_k / eps with t = -f1 / s1: the second term is defined as 0
        n1 = np.sqrt((f1[:, :, 3].double().numpy() ** 2).sum(1, keepdims=True))
        want = 2 * w.double().numpy() * (-f1[:, :, 3].double().numpy() / (n1 + R.EPS)) * (gout.numpy() / 7).reshape(2, 1) / R.EPS
        assert np.abs(closed[:, :, 3] - want).max() <= 16 * 2.0 ** -24 * np.abs(want).max() and np.abs(want).max() > 1e8
        assert np.abs(closed[:, :, keep] - auto.numpy()[:, :, keep]).max() <= 64 * 2.0 ** -24 * np.abs(auto.numpy()[:, :, keep]).max()


def test_through_a_relu_the_zero_pixel_gets_no_gradient():
    """the taps are ReLU outputs: a pixel whose channels are all 0 has every pre-activation <= 0, and the ReLU backward hands the
    pre-activation 0 whatever arrives -- given that it is finite, which is what the kernel's rule provides"""
    f0, f1, w, gout = R.layer_inputs((2, 5, 7))
    pre = f0.double().clone()
    pre[:, :, 3] = -torch.rand(2, 5, dtype=torch.float64) - 0.1
    pre[0, 1, 3] = 0.0                                                               # a pre-activation of exactly 0 included
    pre.requires_grad_(True)
    tap = F.relu(pre)
    assert not bool(tap[:, :, 3].any())
    closed = R.layer_grad_closed(tap.detach().numpy(), f1.numpy(), w.numpy(), gout.numpy(), np.float64)
    assert np.abs(closed[:, :, 3]).max() > 1e8                                       # something large does arrive
    tap.backward(torch.from_numpy(closed))
    assert not bool(pre.grad[:, :, 3].any()) and bool(torch.isfinite(pre.grad).all())
    # the library's own ReLU backward multiplies by 0 or 1 (sg_act_bwd): finite * 0 is 0 as well
    assert not (closed[:, :, 3] * 0.0).any()


def test_scaling_layer_is_the_imagenet_normalisation():
    mean, std = np.array(R.IMAGENET_MEAN), np.array(R.IMAGENET_STD)
    assert np.abs(np.array(LR.SHIFT) - (2 * mean - 1)).max() <= 3e-8 and np.abs(np.array(LR.SCALE) - 2 * std).max() <= 3e-8
    unit = R.pictures(2, 16, 5).double()
    assert float((LR.input_ref(unit) - R.imagenet_normalize(unit)).abs().max()) <= 1e-6
    # the input backward's restatement: one division by the channel's scale
    gy = np.random.RandomState(0).randn(2, 3, 4, 5).astype(np.float32)
    gx = R.input_bwd_np(gy)
    assert gx.dtype == np.float32 and np.array_equal(gx[:, 1], gy[:, 1] / np.float32(.448))
    a = torch.from_numpy(gy).double().requires_grad_(True)
    LR.input_ref(a).backward(torch.ones(2, 3, 4, 5, dtype=torch.float64))
    assert np.abs(R.input_bwd_np(np.ones((2, 3, 4, 5), np.float32)) - a.grad.numpy()).max() <= 2.0 ** -22


# ---- the switch -----------------------------------------------------------------------------------------------------------------------
def test_lpips_loss_parsing():
    off = {'backbone': None, 'lin': None}
    assert LP.check_lpips_loss(1) == dict(off, weight=1.0) and LP.check_lpips_loss('0.25') == dict(off, weight=0.25)
    assert LP.check_lpips_loss(' weight=1.5 , backbone=/w/vgg16.pth,lin=/w/vgg.pth ') == {
        'weight': 1.5, 'backbone': '/w/vgg16.pth', 'lin': '/w/vgg.pth'}
    assert LP.check_lpips_loss('weight=2,lin=/w/vgg.pth') == {'weight': 2.0, 'backbone': None, 'lin': '/w/vgg.pth'}
    assert LP.check_lpips_loss({'weight': 3, 'backbone': {'features.0.weight': 0}})['backbone'] == {'features.0.weight': 0}
    for bad in ('abc', '0', '-1', 'nan', 'inf', 'weight=1,weight=2', 'backbone=/w/a.pth', 'weight=1,net=alex', 'weight=', 'weight=1,,',
                'lin=/a,1.0'):
        with pytest.raises(ValueError, match='lpips_loss'):
            LP.check_lpips_loss(bad)
    for bad in (0, -2.0, float('nan'), True, None, {'backbone': 'x'}, {'weight': 1, 'lin': 3}, {'weight': 1, 'alex': 'x'}):
        with pytest.raises(ValueError, match='lpips_loss'):
            LP.check_lpips_loss(bad)
    assert LP.lpips_loss_from_env({}) is None and LP.lpips_loss_from_env({'SG_LPIPS_LOSS': '  '}) is None
    assert LP.lpips_loss_from_env({'SG_LPIPS_LOSS': '1.0'}) == dict(off, weight=1.0)
    assert LP.lpips_loss_from_env({'SG_LPIPS_LOSS': 'weight=1.0,backbone=B,lin=L'}) == {'weight': 1.0, 'backbone': 'B', 'lin': 'L'}
    for bad in ('on', 'weight=0', 'w=1'):
        with pytest.raises(ValueError, match='SG_LPIPS_LOSS'):
            LP.lpips_loss_from_env({'SG_LPIPS_LOSS': bad})


def _trainer(tmp_path, **kw):
    args = parser.parse_args(ARGV + ['--output_dir', str(tmp_path)])
    ck = {'model_kwargs': {}, 'd_obj_kwargs': {}, 'd_mask_kwargs': {}, 'd_img_kwargs': {}}
    return Trainer(args, make_vocab(12, 4, 35), checkpoint=ck, device='cpu', **kw), args


def test_trainer_switch(tmp_path, monkeypatch, capsys):
    monkeypatch.delenv('SG_LPIPS_LOSS', raising=False)
    before = set(vars(parser.parse_args(ARGV + ['--output_dir', str(tmp_path)])))
    tr, args = _trainer(tmp_path)
    assert tr.criterionLPIPS is None and tr._lpips_loss is None                       # off: no module is built
    assert not any(isinstance(m, LP.LPIPSLoss) for m in vars(tr).values())
    assert set(vars(args)) == before and not [k for k in vars(args) if 'lpips' in k]      # no flag
    assert 'LPIPS' not in capsys.readouterr().err
    g_params = sum(p.numel() for p in tr.optimizer.fp.params)

    sd, lins = LR.random_backbone('vgg', 3), LR.random_lins('vgg', 4)
    tr, _ = _trainer(tmp_path, lpips_loss={'weight': 0.5, 'backbone': sd, 'lin': LR.lin_state_dict(lins)})
    assert isinstance(tr.criterionLPIPS, LP.LPIPSLoss) and tr._lpips_loss['weight'] == 0.5 and tr.criterionLPIPS.input == 'imagenet'
    assert capsys.readouterr().err == ''                                             # both weight sets given: no warning
    assert torch.equal(tr.criterionLPIPS.lin(2), lins[2].reshape(-1))
    assert not any(p.requires_grad for p in tr.criterionLPIPS.parameters())
    assert sum(p.numel() for p in tr.optimizer.fp.params) == g_params                # the frozen network joins no optimiser
    assert tr.criterionVGG is None                                                   # independent of --vgg_features_weight

    tr, _ = _trainer(tmp_path, lpips_loss=2)
    err = capsys.readouterr().err
    assert tr._lpips_loss['weight'] == 2.0 and 'WITHOUT pretrained backbone' in err and 'DO NOT COMPARE' in err

    monkeypatch.setenv('SG_LPIPS_LOSS', '0.75')
    tr, _ = _trainer(tmp_path)
    assert tr._lpips_loss['weight'] == 0.75 and tr.criterionLPIPS is not None
    tr, _ = _trainer(tmp_path, lpips_loss=0.25)                                       # the argument wins over the variable
    assert tr._lpips_loss['weight'] == 0.25
    tr, _ = _trainer(tmp_path, lpips_loss=False)
    assert tr.criterionLPIPS is None
    path = str(tmp_path / 'vgg16.pth')
    torch.save(sd, path)
    monkeypatch.setenv('SG_LPIPS_LOSS', 'weight=1.5,backbone=%s' % path)
    tr, _ = _trainer(tmp_path)
    assert tr._lpips_loss == {'weight': 1.5, 'backbone': path, 'lin': None}
    assert torch.equal(tr.criterionLPIPS.net.state_dict()['features.28.weight'], sd['features.28.weight'])
    for bad in ('yes', 'weight=-1', 'lin=/x'):
        monkeypatch.setenv('SG_LPIPS_LOSS', bad)
        with pytest.raises(ValueError, match='SG_LPIPS_LOSS'):
            _trainer(tmp_path)
    with pytest.raises(ValueError, match='lpips_loss'):
        _trainer(tmp_path, lpips_loss={'gain': 1.0})
