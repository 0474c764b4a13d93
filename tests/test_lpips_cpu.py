"""The diversity score without a GPU: the declarations, the host-only plan query of the wide convolution, the weight loaders, the
restatement's own properties, the command line's file pairing and the sampler's random stream."""
import ctypes
import random

import numpy as np
import pytest
import torch

import lpips_ref as LR
from scene_generation_amd import _hip, ops, sample
from scene_generation_amd import lpips as LP

NEW = ('sg_conv2d_wide_plan', 'sg_conv2d_wide_ws_bytes', 'sg_conv2d_wide_fwd', 'sg_lpips_input', 'sg_lpips_layer_ws_bytes',
       'sg_lpips_layer')


def test_header_declares_the_entry_points():
    for name in NEW:
        assert name in _hip.PROTOS, name
    restype, argtypes, argnames = _hip.PROTOS['sg_lpips_layer']
    assert argnames == ['f0', 'f1', 'w', 'P', 'C', 'HW', 'eps', 'out', 'accumulate', 'ws', 'ws_bytes', 'stream']
    assert argtypes[7] == ctypes.POINTER(ctypes.c_double) and argtypes[6] == ctypes.c_float
    assert _hip.PROTOS['sg_conv2d_wide_fwd'][2] == _hip.PROTOS['sg_conv2d_rect_fwd'][2]          # the same contract
    assert _hip.PROTOS['sg_conv2d_wide_ws_bytes'][0] == ctypes.c_size_t and _hip.PROTOS['sg_lpips_layer_ws_bytes'][0] == ctypes.c_size_t
    for name in ('conv2d_wide', 'conv2d_wide_plan', 'lpips_input', 'lpips_layer'):
        assert callable(getattr(ops, name))


def test_wide_plan_accepts_and_rejects():
    # AlexNet's stem: K = 363 (no 16-byte weight rows), always 64 x 64 tiles, no split
    p = ops.conv2d_wide_plan(ops.rect_desc(2, 3, 35, 35, 64, 11, 11, 4, 2, 2))
    assert p == {'tile': ops.RECT_TILE_64X64, 'bm': 64, 'bn': 64, 'vec': 0, 'splits': 1, 'kchunk': 363}
    p = ops.conv2d_wide_plan(ops.rect_desc(2, 4, 29, 9, 65, 11, 3, 4, 0, 1))
    assert (p['tile'], p['vec']) == (ops.RECT_TILE_64X64, 1)                           # K = 132: 16-byte rows when the base allows
    assert ops.conv2d_wide_plan(ops.rect_desc(2, 4, 29, 9, 65, 11, 3, 4, 0, 1), False)['vec'] == 0
    assert ops.conv2d_wide_plan(ops.rect_desc(64, 3, 128, 128, 64, 11, 11, 4, 2, 2))['tile'] == ops.RECT_TILE_64X64      # never 64 x 128
    assert ops.conv2d_wide_plan(ops.rect_desc(1, 3, 9, 9, 4, 7, 7))['splits'] == 1    # what the rectangular entry point refuses
    assert ops.conv2d_wide_plan(ops.rect_desc(1, 3, 9, 9, 4, 3, 3, stride=3))['tile'] == ops.RECT_TILE_64X64
    # a long reduction over few pixels: the split plan of the rectangular entry point
    p = ops.conv2d_wide_plan(ops.rect_desc(1, 32, 12, 12, 64, 11, 11, 1, 5, 5))
    assert p['splits'] > 1 and p['kchunk'] % 16 == 0 and p['kchunk'] * p['splits'] >= 32 * 121
    bad = [ops.rect_desc(1, 3, 40, 40, 8, 12, 11),                                     # 12 x 11 taps
           ops.rect_desc(1, 3, 40, 40, 8, 11, 12),
           ops.rect_desc(1, 3, 40, 40, 8, 11, 11, stride=5),
           ops.rect_desc(1, 3, 40, 40, 8, 3, 3, 1, 3, 0),                              # pad >= kernel
           ops.rect_desc(1, 3, 40, 40, 8, 3, 3, 1, 0, 3),
           ops.sgRectDesc(1, 3, 40, 40, 8, 11, 11, 4, 2, 2, 10, 9, 0, 8)]              # OH is (40 + 4 - 11) / 4 + 1 = 9, not 10
    bad[-1]._ref = ctypes.byref(bad[-1])
    for d in bad:
        with pytest.raises(RuntimeError, match='sg_conv2d_wide_plan'):
            ops.conv2d_wide_plan(d)
        assert _hip.lib().sg_conv2d_wide_ws_bytes(d._ref) == 0


def test_rect_plan_keeps_its_range():
    with pytest.raises(RuntimeError):
        ops.conv2d_rect_plan(ops.rect_desc(1, 3, 9, 9, 4, 7, 7))       # 49 taps
    with pytest.raises(RuntimeError):
        ops.conv2d_rect_plan(ops.rect_desc(1, 3, 9, 9, 4, 3, 3, stride=3))
    with pytest.raises(RuntimeError):
        ops.conv2d_rect_plan(ops.rect_desc(2, 3, 35, 35, 64, 11, 11, 4, 2, 2))
    assert ops.conv2d_rect_plan(ops.rect_desc(2, 48, 7, 7, 64, 5, 5, 1, 2, 2))['tile'] == ops.RECT_TILE_64X64


def test_entry_points_reject_bad_arguments_before_any_launch():
    L = _hip.lib()
    buf = np.zeros(64, np.float64)
    pd = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    odd = ctypes.cast(buf.ctypes.data + 4, ctypes.POINTER(ctypes.c_double))
    x = np.zeros(64, np.float32).ctypes.data
    for args in ((None, x, None, 1, 4, 4, 1e-10, pd, 0, None, 0, None), (x, None, None, 1, 4, 4, 1e-10, pd, 0, None, 0, None),
                 (x, x, None, 1, 4, 4, 1e-10, None, 0, None, 0, None),                               # null operands
                 (x, x, None, -1, 4, 4, 1e-10, pd, 0, None, 0, None), (x, x, None, 1, 0, 4, 1e-10, pd, 0, None, 0, None),
                 (x, x, None, 1, 4, 0, 1e-10, pd, 0, None, 0, None), (x, x, None, 1 << 20, 1 << 10, 4, 1e-10, pd, 0, None, 0, None),
                 (x, x, None, 1, 4, 4, -1.0, pd, 0, None, 0, None),                                   # eps < 0
                 (x, x, None, 1, 4, 4, 1e-10, odd, 0, None, 0, None),                                 # misaligned out
                 (x, x, None, 1, 4, 4096, 1e-10, pd, 0, None, 0, None)):                              # tiles > 1 without a workspace
        assert L.sg_lpips_layer(*args) < 0 and 'sg_lpips_layer' in _hip.last_error(), args
    assert L.sg_lpips_layer(None, None, None, 0, 4, 4, 1e-10, None, 0, None, 0, None) == 0           # P == 0: nothing to do
    assert L.sg_lpips_layer_ws_bytes(1, 4, 4) == 0 and L.sg_lpips_layer_ws_bytes(3, 64, 4096) >= 3 * 64 * 8
    assert L.sg_lpips_layer_ws_bytes(-1, 4, 4) == 0
    assert L.sg_lpips_input(None, 0, 0, 1, 4, x, None) < 0 and 'sg_lpips_input' in _hip.last_error()
    assert L.sg_lpips_input(x, 0, 0, 1, 0, x, None) < 0
    assert L.sg_lpips_input(None, 1, 1, 0, 4, None, None) == 0
    d = ops.rect_desc(2, 3, 35, 35, 64, 11, 11, 4, 2, 2)
    assert L.sg_conv2d_wide_fwd(d._ref, x, x, None, x, 7, None, 0, None) < 0 and 'act' in _hip.last_error()
    assert L.sg_conv2d_wide_fwd(d._ref, None, x, None, x, 0, None, 0, None) < 0 and 'null' in _hip.last_error()
    bad = ops.rect_desc(1, 3, 40, 40, 8, 11, 11, stride=5)
    assert L.sg_conv2d_wide_fwd(bad._ref, x, x, None, x, 0, None, 0, None) < 0 and 'bad desc' in _hip.last_error()


def test_wrappers_have_no_cpu_fallback():
    x = torch.zeros(1, 3, 35, 35)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.conv2d_wide(x, torch.zeros(4, 3, 11, 11), stride=4, pad=(2, 2))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.lpips_input(x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.lpips_layer(torch.zeros(1, 4, 2), torch.zeros(1, 4, 2))


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_backbone_and_lin_key_forms_load(net, tmp_path, capsys):
    sd, lins = LR.random_backbone(net, 3), LR.random_lins(net, 4)
    cls = LP.AlexFeatures if net == 'alex' else LP.Vgg16Features
    own = cls()
    assert sorted(own.state_dict()) == sorted(k for k in sd if k.startswith('features.'))          # torchvision's keys
    own.load_backbone(sd)                                                                          # classifier.* ignored
    for k, v in own.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert not any(p.requires_grad for p in own.parameters())
    whole = LR.whole_module_state_dict(net, sd, lins)
    other = cls().load_backbone({'module.' + k: v for k, v in whole.items()})                      # net.slice<j>.<i>.*, DataParallel save
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(KeyError):
        cls().load_backbone(LR.lin_state_dict(lins))
    with pytest.raises(RuntimeError):                                                              # strict: a missing conv is an error
        cls().load_backbone({k: v for k, v in sd.items() if not k.startswith('features.0.')})
    # the lin forms, from mappings and from a file
    path = str(tmp_path / 'lin.pth')
    torch.save(LR.lin_state_dict(lins, 'lin'), path)
    for src in (LR.lin_state_dict(lins, 'lin'), LR.lin_state_dict(lins, 'lins'), whole, path):
        got = LP.load_lin_weights(src, LP.CHANNELS[net])
        assert [tuple(w.shape) for w in got] == [(c,) for c in LP.CHANNELS[net]]
        assert all(torch.equal(a, b.reshape(-1)) for a, b in zip(got, lins))
    neg = [w.clone() for w in lins]
    neg[2][0, 7, 0, 0] = -1e-6
    with pytest.raises(ValueError, match='negative'):
        LP.load_lin_weights(LR.lin_state_dict(neg), LP.CHANNELS[net])
    with pytest.raises(KeyError):
        LP.load_lin_weights({k: v for k, v in LR.lin_state_dict(lins).items() if not k.startswith('lin4')}, LP.CHANNELS[net])
    with pytest.raises(ValueError, match='channels'):
        LP.load_lin_weights(LR.lin_state_dict(LR.random_lins('vgg' if net == 'alex' else 'alex', 4)), LP.CHANNELS[net])
    # the whole-module form carries the backbone too; the unweighted form and the random backbone warn loudly
    m = LP.LPIPS(net, lin_weights=whole, device='cpu')
    assert capsys.readouterr().err == ''
    assert torch.equal(m.net.state_dict()['features.0.weight'], sd['features.0.weight']) and torch.equal(m.lin(4), lins[4].reshape(-1))
    m = LP.LPIPS(net, backbone_weights=sd, lin_weights=None, device='cpu')
    err = capsys.readouterr().err
    assert 'DO NOT COMPARE' in err and 'WITHOUT pretrained' not in err and m.lin(0) is None
    LP.LPIPS(net, device='cpu')
    assert 'WITHOUT pretrained backbone' in capsys.readouterr().err
    with pytest.raises(ValueError):
        LP.LPIPS('squeeze', device='cpu')


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_alex_tap_sizes():
    sd = LR.random_backbone('alex', 1)
    for size, want in ((35, (8, 3, 1, 1, 1)), (64, (15, 7, 3, 3, 3)), (67, (16, 7, 3, 3, 3))):
        taps = LR.alex_taps(sd, torch.zeros(1, 3, size, size))
        assert tuple(t.size(2) for t in taps) == want and tuple(t.size(1) for t in taps) == LR.CHANNELS['alex']
    taps = LR.vgg16_taps(LR.random_backbone('vgg', 1), torch.zeros(1, 3, 32, 32))
    assert [tuple(t.shape[1:]) for t in taps] == [(64, 32, 32), (128, 16, 16), (256, 8, 8), (512, 4, 4), (512, 2, 2)]


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_restatement_identity_symmetry_and_zero_pixels(dtype):
    sd, lins = LR.random_backbone('alex', 5), LR.random_lins('alex', 6)
    g = torch.Generator().manual_seed(7)
    a, b = torch.rand(2, 3, 35, 35, generator=g) * 2 - 1, torch.rand(2, 3, 35, 35, generator=g) * 2 - 1
    for w in (lins, None):
        assert torch.equal(LR.lpips_ref('alex', sd, w, a, a, dtype), torch.zeros(2, dtype=dtype))      # d(x, x) == 0 exactly
        ab, ba = LR.lpips_ref('alex', sd, w, a, b, dtype), LR.lpips_ref('alex', sd, w, b, a, dtype)
        assert torch.equal(ab, ba) and bool((ab > 0).all())                                          # (u - v)^2 == (v - u)^2 bit for bit
    f0 = torch.randn(2, 5, 4, generator=g).to(dtype)
    f1 = f0.clone()
    f1[:, :, 1] = 0                                                                                   # a pixel of all zeros: 0 / eps, no NaN
    d = LR.layer_ref(f0, f1)
    assert bool(torch.isfinite(d).all()) and torch.allclose(d, torch.full((2,), 0.25, dtype=dtype))   # |a - 0|^2 = 1 at one pixel of four
    z = torch.zeros(1, 5, 4, dtype=dtype)
    assert torch.equal(LR.layer_ref(z, z), torch.zeros(1, dtype=dtype))


def test_input_restatements_agree():
    rs = np.random.RandomState(0)
    u = rs.randint(0, 256, (2, 3, 5, 7)).astype(np.uint8)
    got = LR.input_ref_np(u)
    assert got.dtype == np.float32
    want = LR.input_ref(LR.uint8_to_unit(torch.from_numpy(u), torch.float64)).numpy()
    assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max()
    x = (rs.rand(2, 3, 5, 7) * 2 - 1).astype(np.float32)
    assert np.array_equal(LR.input_ref_np(x), LR.input_ref(torch.from_numpy(x)).numpy())


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_pairs_files_by_sorted_name(tmp_path):
    for d, names in (('a', ['b/2.png', '10.png', 'b/1.jpg', 'notes.txt']), ('b', ['z.png', 'y.png', 'x.png'])):
        for n in names:
            p = tmp_path / d / n
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_bytes(b'')
    pairs = LP.pair_files(str(tmp_path / 'a'), str(tmp_path / 'b'))
    rel = [(a[len(str(tmp_path / 'a')) + 1:], b[len(str(tmp_path / 'b')) + 1:]) for a, b in pairs]
    assert rel == [('10.png', 'x.png'), ('b/1.jpg', 'y.png'), ('b/2.png', 'z.png')]
    (tmp_path / 'b' / 'w.png').write_bytes(b'')
    with pytest.raises(SystemExit, match='do not pair up'):
        LP.pair_files(str(tmp_path / 'a'), str(tmp_path / 'b'))
    (tmp_path / 'c').mkdir()
    with pytest.raises(SystemExit, match='no images'):
        LP.pair_files(str(tmp_path / 'c'), str(tmp_path / 'b'))
    a = LP.build_parser().parse_args(['--dir0', 'A', '--dir1', 'B'])
    assert (a.net, a.backbone, a.lin, a.batch_size) == ('alex', None, None, 32)
    a = sample.make_parser().parse_args(['--checkpoint', 'c'])
    assert (a.diversity_backbone, a.diversity_lin, a.diversity_net) == (None, None, 'alex')


# ---- the sampler's random stream --------------------------------------------------------------------------------------------------------
class _StubModel(torch.nn.Module):
    num_objs = 4

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


class _StubDiversity(object):
    def __init__(self):
        self.calls = []

    def __call__(self, a, b):
        self.calls.append((a, b))


def _stub_sampler(monkeypatch, **kw):
    bank = {c: np.arange(5 * (c + 2), dtype=np.float64).reshape(c + 2, 5) for c in range(4)}      # 2..5 rows per class
    s = sample.Sampler(_StubModel(), features=bank, colors=torch.zeros(4, 3), **kw)
    seen = []

    def forward(fn, objs_h, o2i_h, want_layout_rgb, want_layout, objs, score=None, scored=True):
        seen.append(scored)
        return sample.SampleOut(torch.full((2, 4, 4, 3), len(seen), dtype=torch.uint8), torch.tensor([[0., 0, 1, 1]] * 5),
                                torch.zeros(5, 2, 2))
    monkeypatch.setattr(s, '_forward', forward)
    return s, seen


def _stub_batch():
    objs = torch.tensor([1, 3, 0, 2, 0])
    boxes = torch.tensor([[0., 0, 1, 1]] * 5)
    return (torch.zeros(2, 3, 4, 4), objs, boxes, torch.zeros(5, 2, 2), torch.zeros(0, 3, dtype=torch.int64),
            torch.tensor([0, 0, 0, 1, 1]), torch.zeros(0, dtype=torch.int64), torch.zeros(5, 35))


def _draws(objs, times=1):
    """the reference's draws: one ``random.randint(0, rows - 1)`` per object, in object order"""
    for _ in range(times):
        for c in objs:
            random.randint(0, c + 2 - 1)
    return random.getstate()


def test_sampler_random_stream(monkeypatch):
    s, seen = _stub_sampler(monkeypatch)
    random.seed(9)
    s.sample_batch(_stub_batch())
    state = random.getstate()
    random.seed(9)
    assert state == _draws([1, 3, 0, 2, 0]) and seen == [True]
    total = s.iou.clone()
    assert s.diversity is None and s.diversity_summary() is None
    with pytest.raises(ValueError, match='without a diversity scorer'):
        s.sample_pair(_stub_batch())
    assert random.getstate() == state                            # nothing drawn by the refused call
    random.seed(9)
    s.sample_batch(_stub_batch(), use_gt_textures=True)
    random.seed(9)
    assert random.getstate() == _draws([])                       # ground-truth textures draw nothing
    # a pair: twice the draws, the second forward unscored, the IoU counters fed once
    div = _StubDiversity()
    s2, seen2 = _stub_sampler(monkeypatch, diversity=div)
    random.seed(9)
    first, second = s2.sample_pair(_stub_batch())
    state2 = random.getstate()
    random.seed(9)
    assert state2 == _draws([1, 3, 0, 2, 0], times=2) and seen2 == [True, False]
    assert torch.equal(s2.iou, total) and len(div.calls) == 1
    assert div.calls[0][0] is first.images and div.calls[0][1] is second.images and int(second.images[0, 0, 0, 0]) == 2
    with pytest.raises(ValueError, match='nothing is random'):
        s2.sample_pair(_stub_batch(), use_gt_textures=True)
    assert len(div.calls) == 1 and seen2 == [True, False]
