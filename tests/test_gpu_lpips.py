"""The diversity score on the GPU (csrc/lpips.hip, ops/lpips.py, scene_generation_amd/lpips.py, Sampler.sample_pair).

The scaling layer is compared bit for bit with the NumPy float32 restatement of tests/lpips_ref.py.  Float results (the wide
convolution, one tap of the distance, the backbones' taps, whole distances, the sampler's diversity) are compared with a float64 CPU
run of the plain torch restatement; the bound is the family's factor (16 for a family not yet measured, 8 where the worst observed
ratio is under 2: profiles/lpips_test_margins.md) times the error torch's own float32 CPU run makes on the same inputs, never below
2^-24 of the tensor's largest magnitude, in max norm.  The worst ratio per family goes to lpips_margins.json in the suite's output
directory.

Worst ratios measured on an MI355X (profiles/lpips_test_margins.md): wide_conv 1.81, layer 1.32, alex_taps 1.59, lpips_alex 0.80,
lpips_vgg 0.90, diversity_e2e 0.48 -- every family is under 2 and runs at the factor 8."""
import functools
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as LR
import sampling_helpers as SH
from gpu_harness import Margins, margins_fixture
from conftest import skip_random_init
from scene_generation_amd import inception as I
from scene_generation_amd import lpips as LP
from scene_generation_amd import ops, sample
from scene_generation_amd.model import Model
from scene_generation_amd.synthetic import fill_deterministic, make_batch, make_sampling_vocab

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 16.0
# families whose worst observed ratio is under 2 (profiles/lpips_test_margins.md): their factor is halved to 8
FACTORS = {k: 8.0 for k in ('wide_conv', 'layer', 'alex_taps', 'lpips_alex', 'lpips_vgg', 'diversity_e2e')}
FLOOR = 2.0 ** -24
MARGINS = Margins()
_write_margins = margins_fixture(lambda: MARGINS.dump_yardstick('lpips_margins.json', FACTORS, FACTOR))
SENTINEL = -12345.0


def offset_copy(t, off=1):
    """a device copy of ``t`` that starts ``off`` elements into its allocation (4 bytes past a 16-byte boundary for float32)"""
    buf = torch.full((t.numel() + off + 1,), -777.0, dtype=t.dtype, device=DEV)
    buf[off:off + t.numel()] = t.reshape(-1).to(DEV)
    view = buf[off:off + t.numel()].view(t.shape)
    assert view.data_ptr() % 16 == (4 * off) % 16 and view.is_contiguous()
    return view


def check(family, name, got, ref64, ref32):
    """|got - ref64| <= factor * max(|ref32 - ref64|, 2^-24 max|ref64|), in max norm over the tensor; factor = the family's"""
    MARGINS.yardstick(family, name, got, ref64, ref32, FACTORS, FACTOR, FLOOR)


# =====================================================================================================================================
# 1. the wide convolution
# =====================================================================================================================================
#        name              N  C  Cout H   W   KH  KW  s  pH pW
WIDE = [('alex_stem_35', 2, 3, 64, 35, 35, 11, 11, 4, 2, 2),
        ('alex_stem_rect', 2, 3, 64, 43, 30, 11, 11, 4, 2, 2),          # 10 x 6 output
        ('one_window', 1, 3, 5, 7, 7, 11, 11, 4, 2, 2),                 # a single output whose border taps are all padding
        ('k11s1_pad5', 2, 2, 9, 6, 6, 11, 11, 1, 5, 5),
        ('k7s3', 2, 5, 33, 16, 13, 7, 7, 3, 3, 3),
        ('k11x3_vec', 2, 4, 65, 29, 9, 11, 3, 4, 0, 1)]                 # K = 132: 16-byte weight rows, a 64-row tile boundary


@functools.lru_cache(maxsize=None)
def _wide_refs(case):
    name, n, c, cout, h, w, kh, kw, s, ph, pw = case
    g = torch.Generator().manual_seed(sum(case[1:]) * 7 + kh)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(cout, c, kh, kw, generator=g) * (2.0 / (c * kh * kw)) ** 0.5
    b = 0.3 * torch.randn(cout, generator=g)
    refs = {}
    for dt in (torch.float64, torch.float32):
        raw = F.conv2d(x.to(dt), wt.to(dt), None, s, (ph, pw))
        lin = raw + b.to(dt).view(1, -1, 1, 1)
        refs[dt] = {'bias_relu': F.relu(lin), 'bias': lin, 'plain': raw}
    return x, wt, b, refs


@pytest.mark.parametrize('case', WIDE, ids=lambda c: c[0])
def test_conv2d_wide(case):
    name, n, c, cout, h, w, kh, kw, s, ph, pw = case
    x, wt, b, refs = _wide_refs(case)
    oh, ow = refs[torch.float64]['plain'].shape[2:]
    if name == 'alex_stem_rect':
        assert (oh, ow) == (10, 6)
    if name == 'one_window':
        assert (oh, ow) == (1, 1)
    plan = ops.conv2d_wide_plan(ops.rect_desc(n, c, h, w, cout, kh, kw, s, ph, pw))
    assert (plan['tile'], plan['splits']) == (ops.RECT_TILE_64X64, 1) and plan['vec'] == (1 if (c * kh * kw) % 4 == 0 else 0)
    tx, tw, tb = x.to(DEV), wt.to(DEV), b.to(DEV)
    for variant, bias, act in (('bias_relu', tb, ops.ACT_RELU), ('bias', tb, ops.ACT_NONE), ('plain', None, ops.ACT_NONE)):
        out = ops.conv2d_wide(tx, tw, bias, stride=s, pad=(ph, pw), act=act)
        assert torch.equal(out, ops.conv2d_wide(tx, tw, bias, stride=s, pad=(ph, pw), act=act))           # deterministic
        check('wide_conv', '%s %s' % (name, variant), out, refs[torch.float64][variant], refs[torch.float32][variant])


def test_conv2d_wide_channel_slice_and_offset_pointers():
    case = WIDE[5]                                               # K = 132: the aligned run takes 16-byte weight loads, the offset one cannot
    name, n, c, cout, h, w, kh, kw, s, ph, pw = case
    x, wt, b, refs = _wide_refs(case)
    r64, r32 = refs[torch.float64]['bias_relu'], refs[torch.float32]['bias_relu']
    oh, ow = r64.shape[2:]
    tx, tw, tb = x.to(DEV), wt.to(DEV), b.to(DEV)
    out = torch.full((n, cout + 8, oh, ow), SENTINEL, device=DEV)
    res = ops.conv2d_wide(tx, tw, tb, stride=s, pad=(ph, pw), act=ops.ACT_RELU, out=out, out_c0=3)
    assert res is out
    side = torch.cat([out[:, :3], out[:, 3 + cout:]], 1)
    assert side.size(1) == 8 and bool((side == SENTINEL).all())          # three guard channels before, five after: untouched
    check('wide_conv', name + ' slice', out[:, 3:3 + cout], r64, r32)
    assert torch.equal(out[:, 3:3 + cout], ops.conv2d_wide(tx, tw, tb, stride=s, pad=(ph, pw), act=ops.ACT_RELU))
    # weights, input, bias and output one element past a 16-byte boundary
    ox, ow_, ob = offset_copy(x), offset_copy(wt), offset_copy(b)
    oout = offset_copy(torch.full((n, cout, oh, ow), SENTINEL))
    ops.conv2d_wide(ox, ow_, ob, stride=s, pad=(ph, pw), act=ops.ACT_RELU, out=oout)
    check('wide_conv', name + ' offset pointers', oout, r64, r32)
    x2, wt2, b2, refs2 = _wide_refs(WIDE[0])
    got = ops.conv2d_wide(offset_copy(x2), offset_copy(wt2), offset_copy(b2), stride=4, pad=(2, 2), act=ops.ACT_RELU)
    check('wide_conv', 'alex_stem_35 offset pointers', got, refs2[torch.float64]['bias_relu'], refs2[torch.float32]['bias_relu'])


def test_conv2d_wide_rejects_what_the_plan_rejects():
    x = torch.zeros(1, 3, 40, 40, device=DEV)
    for wshape, stride, pad in (((8, 3, 12, 11), 1, (0, 0)), ((8, 3, 11, 12), 1, (0, 0)), ((8, 3, 11, 11), 5, (0, 0)),
                                ((8, 3, 3, 3), 1, (3, 0)), ((8, 3, 3, 3), 1, (0, 3))):
        with pytest.raises(RuntimeError, match='sg_conv2d_wide_fwd'):
            ops.conv2d_wide(x, torch.zeros(wshape, device=DEV), stride=stride, pad=pad)
    with pytest.raises(RuntimeError, match='sg_conv2d_wide_fwd'):                # a kernel larger than the padded plane
        ops.conv2d_wide(torch.zeros(1, 3, 4, 4, device=DEV), torch.zeros(8, 3, 11, 11, device=DEV), stride=4, pad=(2, 2))
    with pytest.raises(ValueError):
        ops.conv2d_wide(x, torch.zeros(8, 4, 11, 11, device=DEV))
    with pytest.raises(ValueError):
        ops.conv2d_wide(x, torch.zeros(8, 3, 11, 11, device=DEV), act=ops.ACT_TANH)
    with pytest.raises(RuntimeError):                                            # and the rectangular entry point keeps refusing the stem
        ops.conv2d_rect(x, torch.zeros(8, 3, 11, 11, device=DEV), stride=4, pad=(2, 2))


# =====================================================================================================================================
# 2. the scaling layer
# =====================================================================================================================================
@pytest.mark.parametrize('shape', [(1, 3, 1, 1), (2, 3, 5, 7), (3, 3, 33, 31)])
def test_lpips_input_bit_exact(shape):
    rs = np.random.RandomState(sum(shape))
    u = rs.randint(0, 256, shape).astype(np.uint8)
    u.reshape(-1)[:2] = (0, 255)
    x = (rs.rand(*shape) * 2 - 1).astype(np.float32)
    x.reshape(-1)[:3] = (-1.0, 1.0, 0.0)
    for src in (u, x):
        want = LR.input_ref_np(src)
        got = ops.lpips_input(torch.from_numpy(src).to(DEV))
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)
        nhwc = torch.from_numpy(np.ascontiguousarray(src.transpose(0, 2, 3, 1))).to(DEV)
        assert np.array_equal(ops.lpips_input(nhwc, channels_last=True).cpu().numpy(), want)
    with pytest.raises(TypeError):
        ops.lpips_input(torch.zeros(1, 3, 2, 2, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        ops.lpips_input(torch.zeros(1, 4, 2, 2, device=DEV))
    assert tuple(ops.lpips_input(torch.zeros(0, 3, 2, 2, device=DEV)).shape) == (0, 3, 2, 2)


# =====================================================================================================================================
# 3. one tap of the distance
# =====================================================================================================================================
# the issue's shapes, then the launch forms they do not reach: (4, 128, 4096) 64-pixel tiles with 32 channels a thread; (1, 530, 7)
# channels beyond the 32 registers of a thread (read twice)
LAYER = [(1, 1, 1), (2, 3, 5), (3, 64, 64), (2, 192, 9), (2, 384, 1), (2, 65, 961), (2, 512, 64), (1, 64, 16384), (4, 128, 4096),
         (1, 530, 7)]


@functools.lru_cache(maxsize=None)
def _layer_inputs(shape):
    P, C, HW = shape
    g = torch.Generator().manual_seed(P * 1000003 + C * 101 + HW)
    f0, f1 = F.relu(torch.randn(P, C, HW, generator=g)), F.relu(torch.randn(P, C, HW, generator=g) + 0.2)      # taps follow a ReLU
    if HW > 1:
        f0[:, :, HW // 2] = 0                                    # a pixel of all zeros on one side
        f1[:, :, HW - 1] = 0
        f0[:, :, HW - 1] = 0                                     # ... and on both
    w = torch.rand(C, generator=g)
    w[::5] = 0
    refs = {}
    for key, ww in (('w', w), ('ones', None)):
        refs[key] = (LR.layer_ref(f0.double(), f1.double(), None if ww is None else ww.double()), LR.layer_ref(f0, f1, ww))
    return f0, f1, w, refs


@pytest.mark.parametrize('shape', LAYER, ids=lambda s: '%dx%dx%d' % s)
def test_lpips_layer(shape):
    P, C, HW = shape
    f0, f1, w, refs = _layer_inputs(shape)
    t0, t1, tw = f0.to(DEV), f1.to(DEV), w.to(DEV)
    o0, o1, ow = offset_copy(f0), offset_copy(f1), offset_copy(w)
    for key, ww, oww in (('w', tw, ow), ('ones', None, None)):
        r64, r32 = refs[key]
        got = ops.lpips_layer(t0, t1, ww)
        assert got.dtype == torch.float64 and tuple(got.shape) == (P,)
        check('layer', '%s %s' % (shape, key), got, r64, r32)
        assert got.cpu().numpy().tobytes() == ops.lpips_layer(t0, t1, ww).cpu().numpy().tobytes()          # two runs, bit-identical
        assert torch.equal(ops.lpips_layer(o0, o1, oww), got)                                            # offset base pointers
        assert torch.equal(ops.lpips_layer(t0, t0, ww), torch.zeros(P, dtype=torch.float64, device=DEV))   # d(x, x) == 0.0 exactly
        assert torch.equal(ops.lpips_layer(t1, t0, ww), got)                                             # symmetric bit for bit
        preset = torch.arange(1, P + 1, dtype=torch.float64, device=DEV) * 0.125
        acc = preset.clone()
        assert ops.lpips_layer(t0, t1, ww, out=acc, accumulate=True) is acc
        assert torch.equal(acc, preset + got)                                                            # added on top of the preset value
        assert torch.equal(ops.lpips_layer(t0, t1, ww, out=acc), got)                                    # overwritten without accumulate
    z = torch.zeros(P, C, HW, device=DEV)
    assert torch.equal(ops.lpips_layer(z, z, tw), torch.zeros(P, dtype=torch.float64, device=DEV))        # 0 / (0 + eps): no NaN


def test_lpips_layer_empty_and_rejects():
    e = torch.zeros(0, 4, 3, device=DEV)
    assert tuple(ops.lpips_layer(e, e).shape) == (0,)                                                    # P == 0: nothing launched
    a = torch.zeros(2, 4, 3, device=DEV)
    with pytest.raises(ValueError):
        ops.lpips_layer(a, torch.zeros(2, 4, 2, device=DEV))
    with pytest.raises(ValueError):
        ops.lpips_layer(a, a, torch.zeros(5, device=DEV))
    with pytest.raises(ValueError):
        ops.lpips_layer(a, a, out=torch.zeros(2, device=DEV))
    with pytest.raises(ValueError):
        ops.lpips_layer(a, a, accumulate=True)
    with pytest.raises(TypeError):
        ops.lpips_layer(a.double(), a.double())
    # a view of a 4-D tap: the halves of one 2P forward
    t = torch.rand(4, 6, 3, 5, generator=torch.Generator().manual_seed(1))
    got = ops.lpips_layer(t.to(DEV)[:2], t.to(DEV)[2:])
    check('layer', 'halves of a 4-D tap', got, LR.layer_ref(t[:2].double(), t[2:].double()), LR.layer_ref(t[:2], t[2:]))


# =====================================================================================================================================
# 4. networks
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _weights(net):
    return LR.random_backbone(net, 21 if net == 'alex' else 22), LR.random_lins(net, 23)


@functools.lru_cache(maxsize=None)
def _lpips(net, weighted):
    sd, lins = _weights(net)
    return LP.LPIPS(net, backbone_weights=sd, lin_weights=LR.lin_state_dict(lins) if weighted else None, device=DEV)


def _pictures(P, size, seed, identical=None):
    """smooth random pictures in [-1, 1] (pure noise gives every pair nearly the same distance); pair ``identical`` repeats x0"""
    g = torch.Generator().manual_seed(seed)
    def draw():
        low = torch.rand(P, 3, 5, 5, generator=g) * 2 - 1
        return (0.8 * F.interpolate(low, size=(size, size), mode='bilinear', align_corners=False)
                + 0.2 * (torch.rand(P, 3, size, size, generator=g) * 2 - 1)).clamp(-1, 1)
    x0, x1 = draw(), draw()
    if identical is not None:
        x1[identical] = x0[identical]
    return x0, x1


@pytest.mark.parametrize('size', [35, 67])
def test_alex_features_taps(size):
    sd, _ = _weights('alex')
    net = LP.AlexFeatures().load_backbone(sd).to(DEV)
    x = LR.input_ref(_pictures(2, size, size)[0])
    t64, t32 = LR.alex_taps(sd, x.double()), LR.alex_taps(sd, x)
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        taps = net(x.to(DEV))
        prof = ops.prof_read()
    finally:
        ops.prof_enable(False)
    assert prof['wide_conv_t64']['launches'] == 1 and prof['inception_pool']['launches'] == 2
    assert sum(prof[k]['launches'] for k in ('rect_conv_t64', 'rect_conv_t32', 'rect_conv_t64x128')) == 4
    assert [t.size(2) for t in taps] == ([8, 3, 1, 1, 1] if size == 35 else [16, 7, 3, 3, 3])
    for k, t in enumerate(taps):
        assert float(t64[k].abs().max()) > 1e-3 and not t.requires_grad
        check('alex_taps', 'alex %d px tap %d' % (size, k), t, t64[k], t32[k])
    assert all(torch.equal(a, b) for a, b in zip(net(x.to(DEV)), taps))


@pytest.mark.parametrize('weighted', [True, False], ids=['lin', 'unweighted'])
@pytest.mark.parametrize('size', [35, 64, 128])
def test_lpips_alex(size, weighted):
    sd, lins = _weights('alex')
    x0, x1 = _pictures(3, size, 100 + size, identical=1)
    r64 = LR.lpips_ref('alex', sd, lins if weighted else None, x0, x1, torch.float64)
    r32 = LR.lpips_ref('alex', sd, lins if weighted else None, x0, x1, torch.float32)
    m = _lpips('alex', weighted)
    got = m(x0.to(DEV), x1.to(DEV))
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (3,)
    assert float(got[1]) == 0.0 and float(r64[1]) == 0.0 and float(got[0]) > 0 and float(got[2]) > 0      # the identical pair: exactly 0
    check('lpips_alex', 'alex %d px %s' % (size, 'lin' if weighted else 'w = 1'), got, r64, r32)
    assert torch.equal(m(x0.to(DEV), x1.to(DEV)), got) and torch.equal(m(x1.to(DEV), x0.to(DEV)), got)


@pytest.mark.parametrize('weighted', [True, False], ids=['lin', 'unweighted'])
def test_lpips_vgg(weighted):
    sd, lins = _weights('vgg')
    x0, x1 = _pictures(2, 32, 7)
    r64 = LR.lpips_ref('vgg', sd, lins if weighted else None, x0, x1, torch.float64)
    r32 = LR.lpips_ref('vgg', sd, lins if weighted else None, x0, x1, torch.float32)
    m = _lpips('vgg', weighted)
    got = m(x0.to(DEV), x1.to(DEV))
    check('lpips_vgg', 'vgg 32 px %s' % ('lin' if weighted else 'w = 1'), got, r64, r32)
    assert torch.equal(m(x0.to(DEV), x1.to(DEV)), got)
    assert torch.equal(m(x0.to(DEV), x0.to(DEV)), torch.zeros(2, dtype=torch.float64, device=DEV))
    if weighted:
        taps = m.net(LR.input_ref(x0).to(DEV))
        assert [tuple(t.shape[1:]) for t in taps] == [(64, 32, 32), (128, 16, 16), (256, 8, 8), (512, 4, 4), (512, 2, 2)]
        u0, u1 = ((x0 * 0.5 + 0.5) * 255).round().byte(), ((x1 * 0.5 + 0.5) * 255).round().byte()      # uint8 pictures, both layouts
        want = LR.lpips_ref('vgg', sd, lins, LR.uint8_to_unit(u0, torch.float64), LR.uint8_to_unit(u1, torch.float64), torch.float64)
        w32 = LR.lpips_ref('vgg', sd, lins, LR.uint8_to_unit(u0, torch.float32), LR.uint8_to_unit(u1, torch.float32), torch.float32)
        g8 = m(u0.to(DEV), u1.to(DEV))
        check('lpips_vgg', 'vgg 32 px uint8', g8, want, w32)
        nhwc = m(u0.permute(0, 2, 3, 1).contiguous().to(DEV), u1.permute(0, 2, 3, 1).contiguous().to(DEV), channels_last=True)
        assert torch.equal(nhwc, g8)


def test_diversity_scorer_grows_and_reads_once():
    m = _lpips('alex', True)
    d = LP.Diversity(m, batch_size=2)
    r = d.compute()
    assert r['pairs'] == 0 and np.isnan(r['mean']) and np.isnan(r['std'])
    x0, x1 = _pictures(5, 35, 3)
    caps = []
    for _ in range(4):
        d(x0.to(DEV), x1.to(DEV))
        caps.append(d.dist.numel())
    assert caps == [8, 16, 16, 32] and d.count == 20                      # chunks of 2, 2, 1 per call; doubled when full
    one = m(x0.to(DEV), x1.to(DEV)).cpu()
    r = d.compute()
    assert r['pairs'] == 20 and abs(r['mean'] - float(one.mean())) <= 1e-12 * abs(float(one.mean()))
    assert abs(r['std'] - float(one.std(unbiased=False))) <= 1e-9 * float(one.std(unbiased=False))      # population std
    d.clean()
    assert d.count == 0 and d.dist.numel() == 32


# =====================================================================================================================================
# 5. the sampler
# =====================================================================================================================================
def _sampling_model():
    m = SH.small_model(Model, make_sampling_vocab(SH.C, 7, SH.A)).to(DEV)
    m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    return m


def _batch(seed=321):
    return make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=SH.C, num_preds=7, num_attributes=35, seed=seed)


def test_sample_pair_end_to_end():
    from scene_generation_amd.fid import FrechetInceptionDistance
    sd, lins = _weights('alex')
    model, bank = _sampling_model(), SH.make_banks()[0]
    with skip_random_init():
        inc = I.InceptionV3(num_classes=I.FID_CLASSES, aux_logits=False, fid_variant=True)
    fill_deterministic(inc)
    inc = inc.to(DEV).eval()

    def scorers():
        f = FrechetInceptionDistance(weights=inc, resize=True, batch_size=4, device=DEV)
        return I.InceptionScore(batch_size=4, resize=True, weights=inc, device=DEV, fid=f), f

    sc_a, fid_a = scorers()
    div = LP.Diversity(_lpips('alex', True), batch_size=2)
    a = sample.Sampler(model, features=bank, colors=torch.arange(36.).view(12, 3), inception=sc_a, fid=fid_a, diversity=div)
    random.seed(11)
    states, pairs = [], []
    for seed in (321, 322):
        states.append(random.getstate())
        pairs.append(a.sample_pair(_batch(seed), use_gt_boxes=True, use_gt_masks=True))
    assert not torch.equal(pairs[0][0].images, pairs[0][1].images)                        # the second forward drew other bank rows
    # a plain run with the same seed: the same counts
    sc_b, fid_b = scorers()
    b = sample.Sampler(model, features=bank, colors=torch.arange(36.).view(12, 3), inception=sc_b, fid=fid_b)
    random.seed(11)
    first_b = b.sample_batch(_batch(321), use_gt_boxes=True, use_gt_masks=True)
    assert torch.equal(first_b.images, pairs[0][0].images)                                # the first forward is the plain forward
    b.sample_batch(_batch(322), use_gt_boxes=True, use_gt_masks=True)
    assert torch.equal(a.iou, b.iou) and a.iou_summary()['total_boxes'] == b.iou_summary()['total_boxes'] > 0
    assert (sc_a.count, fid_a.fake.count) == (sc_b.count, fid_b.fake.count) == (6, 6)
    # ... and, started from the random state each pair started from (a forward draws from ``random`` itself, for the model's
    # appearance pool, so the second forward moves the stream), the same scorer contents bit for bit: they saw the first forward only
    sc_c, fid_c = scorers()
    c = sample.Sampler(model, features=bank, colors=torch.arange(36.).view(12, 3), inception=sc_c, fid=fid_c)
    for seed, state, pair in zip((321, 322), states, pairs):
        random.setstate(state)
        assert torch.equal(c.sample_batch(_batch(seed), use_gt_boxes=True, use_gt_masks=True).images, pair[0].images)
    assert torch.equal(sc_a.probs[:6], sc_c.probs[:6]) and bool(torch.isfinite(sc_a.probs[:6]).all())
    assert torch.equal(fid_a.fake.sum, fid_c.fake.sum) and torch.equal(fid_a.fake.outer, fid_c.fake.outer)
    assert torch.equal(a.iou, c.iou)
    # the number: the float64 restatement on the very uint8 pictures the SampleOuts hold
    got = a.diversity_summary()
    assert got['pairs'] == 6 and b.diversity_summary() is None
    u0 = torch.cat([p[0].images for p in pairs]).cpu().permute(0, 3, 1, 2)
    u1 = torch.cat([p[1].images for p in pairs]).cpu().permute(0, 3, 1, 2)
    assert u0.dtype == torch.uint8 and tuple(u0.shape) == (6, 3, 32, 32)
    want = {}
    for dt in (torch.float64, torch.float32):
        d = LR.lpips_ref('alex', sd, lins, LR.uint8_to_unit(u0, dt), LR.uint8_to_unit(u1, dt), dt).double()
        want[dt] = (float(d.mean()), float(d.std(unbiased=False)))
    assert want[torch.float64][0] > 1e-4 and want[torch.float64][1] > 0                   # the two draws give different pictures
    scale = abs(want[torch.float64][0])
    for k, name in enumerate(('mean', 'std')):
        s64, s32 = want[torch.float64][k], want[torch.float32][k]
        e, yard = abs(got[name] - s64) / scale, max(abs(s32 - s64) / scale, FLOOR)
        ratio = e / yard
        MARGINS.note('diversity_e2e', ratio, name)
        print('diversity_e2e %-5s got %.12g  fp64 %.12g  fp32 %.12g  ratio %.3f' % (name, got[name], s64, s32, ratio))
        assert ratio <= FACTORS.get('diversity_e2e', FACTOR), (name, got[name], s64, s32)
    with pytest.raises(ValueError, match='nothing is random'):
        a.sample_pair(_batch(), use_gt_boxes=True, use_gt_masks=True, use_gt_textures=True)
    with pytest.raises(ValueError, match='without a diversity scorer'):
        b.sample_pair(_batch())


def test_sample_cli_prints_the_diversity_line(tmp_path, capsys):
    vocab = make_sampling_vocab(SH.C, SH.P, SH.A)
    kw = dict(image_size=(32, 32), gconv_hidden_dim=64, gconv_num_layers=3, mask_size=8, mlp_normalization='none',
              appearance_normalization='batch', activation='leakyrelu-0.2', n_downsample_global=2, use_attributes=True, pool_size=2)
    m = SH.small_model(Model, vocab)                             # (these widths; non-degenerate predicted boxes)
    ckpt, bank = str(tmp_path / 'ckpt.pt'), str(tmp_path / 'features_clustered_001.npy')
    torch.save({'model_kwargs': dict(vocab=vocab, **kw), 'model_state': m.state_dict()}, ckpt)
    np.save(bank, SH.make_banks()[0], allow_pickle=True)
    sd, lins = _weights('alex')
    backbone, lin = str(tmp_path / 'alexnet.pth'), str(tmp_path / 'alex_lin.pth')
    torch.save(sd, backbone)
    torch.save(LR.lin_state_dict(lins), lin)
    base = ['--checkpoint', ckpt, '--batch_size', '3', '--num_samples', '6', '--use_gt_boxes', '1', '--use_gt_masks', '1']
    random.seed(4)
    res0 = sample.main(base + ['--output_dir', str(tmp_path / 'a')])
    out0 = capsys.readouterr().out
    assert 'Diversity' not in out0 and 'diversity' not in res0
    random.seed(4)
    res1 = sample.main(base + ['--output_dir', str(tmp_path / 'b'), '--diversity_backbone', backbone, '--diversity_lin', lin])
    out1 = capsys.readouterr()
    line = [l for l in out1.out.splitlines() if l.startswith('Diversity ')]
    assert len(line) == 1 and 'DO NOT COMPARE' not in out1.err
    mean, std = [float(v) for v in line[0].split()[1:]]
    assert res1['diversity'] == {'mean': mean, 'std': std, 'pairs': 6} and mean > 0 and std >= 0
    assert len(res1['paths']) == 6 and res1['iou']['total_boxes'] == res0['iou']['total_boxes']
    with pytest.raises(ValueError, match='needs the bank'):
        sample.main(base + ['--output_dir', str(tmp_path / 'c'), '--diversity_backbone', backbone, '--use_gt_textures', '1'])
