"""The Inception score on the GPU (csrc/inception.hip, ops/inception.py, scene_generation_amd/inception.py).

Exact kernels (the two pools) are compared bit for bit with the NumPy restatements of tests/inception_ref.py.  Float results
(rectangular convolutions, resize, softmax, whole networks, the end-to-end score) are compared with a float64 CPU run of the plain
torch restatement; the bound is the family's factor (16, or 8 where the worst observed ratio is under 2: profiles/
inception_test_margins.md) times the error torch's own float32 CPU run makes on the same inputs, never below 2^-24 of the tensor's
largest magnitude.  Errors are max |a - ref| / max |ref| per tensor.  sg_inception_score is compared with the NumPy float64
restatement on the same float32 probabilities within 1e-9 relative: its float64 sums have at most 6.4e4 terms (about 7e-12
relative), times 100 of headroom for the log / exp.  The worst ratio per family goes to inception_margins.json in the suite's
output directory.  The tree only: no reference checkout."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R
import sampling_helpers as SH
from gpu_harness import Margins, N, margins_fixture
from conftest import skip_random_init
from scene_generation_amd import inception as I
from scene_generation_amd import ops, sample
from scene_generation_amd.model import Model

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 16.0
# families whose worst observed ratio is under 2 (profiles/inception_test_margins.md): their factor is halved to 8; score_e2e keeps 16
FACTORS = {k: 8.0 for k in ('rect_conv', 'avgpool', 'resize', 'softmax', 'net')}
FLOOR = 2.0 ** -24
MARGINS = Margins()
_write_margins = margins_fixture(lambda: MARGINS.dump_yardstick('inception_margins.json', FACTORS, FACTOR))
SCORE_RTOL = 1e-9


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


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
# 1. the rectangular convolution
# =====================================================================================================================================
#            name            N  C     Cout H   W    KH KW s  pH pW
RECT = [('1x7_every_row_pads', 2, 5, 7, 9, 6, 1, 7, 1, 0, 3),
        ('7x1_on_9x6', 2, 5, 7, 9, 6, 7, 1, 1, 3, 0),
        ('1x3_33to65', 2, 33, 65, 8, 8, 1, 3, 1, 0, 1),
        ('3x1_33to65', 2, 33, 65, 8, 8, 3, 1, 1, 1, 0),
        ('k3s2_17to8', 2, 12, 40, 17, 17, 3, 3, 2, 0, 0),
        ('k3s2_8x7', 2, 9, 33, 8, 7, 3, 3, 2, 0, 0),
        ('k5p2_48to64', 2, 48, 64, 7, 7, 5, 5, 1, 2, 2),
        ('k1_64to80', 2, 64, 80, 5, 5, 1, 1, 1, 0, 0),
        ('k3p1_K27', 2, 3, 32, 10, 7, 3, 3, 1, 1, 1),
        ('k3_32to32_vector_weights', 2, 32, 32, 9, 11, 3, 3, 1, 0, 0),
        ('k1_2048to192_split', 1, 2048, 192, 8, 8, 1, 1, 1, 0, 0),
        ('1x7_160_on_17', 2, 160, 160, 17, 17, 1, 7, 1, 0, 3),
        ('k1_4to64_on_224_wide_tile', 2, 4, 64, 224, 224, 1, 1, 1, 0, 0)]
EXTRA = 9                                                        # sentinel channels around the slice: 4 before, 5 after
SENTINEL = -12345.0
PLANS_RUN = {}                                                   # case name -> the plans test_conv2d_rect launched (aligned, offset weights)


def _rect_refs(case):
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


@pytest.mark.parametrize('case', RECT, ids=lambda c: c[0])
def test_conv2d_rect(case):
    name, n, c, cout, h, w, kh, kw, s, ph, pw = case
    x, wt, b, refs = _rect_refs(case)
    oh, ow = refs[torch.float64]['plain'].shape[2:]
    d = ops.rect_desc(n, c, h, w, cout, kh, kw, s, ph, pw, 4, cout + EXTRA)
    assert (d.OH, d.OW) == (oh, ow)
    plan, plan_off = ops.conv2d_rect_plan(d, True), ops.conv2d_rect_plan(d, False)
    print(name, 'plan', plan, 'unaligned weights', plan_off)
    if 'split' in name:
        assert plan['splits'] > 1 and plan_off['splits'] == plan['splits']      # K = 2048 over 64 pixels: the split plan
    if 'wide_tile' in name:
        assert plan['tile'] == ops.RECT_TILE_64X128
    tx, tw, tb = x.to(DEV), wt.to(DEV), b.to(DEV)
    kept = {}
    for variant, bias, act in (('bias_relu', tb, ops.ACT_RELU), ('bias', tb, ops.ACT_NONE), ('plain', None, ops.ACT_NONE)):
        runs = []
        for _ in range(2):
            out = torch.full((n, cout + EXTRA, oh, ow), SENTINEL, device=DEV)
            res = ops.conv2d_rect(tx, tw, bias, stride=s, pad=(ph, pw), act=act, out=out, out_c0=4)
            assert res is out
            runs.append(out)
        out = kept[variant] = runs[0]
        assert torch.equal(runs[0], runs[1])                     # deterministic
        side = torch.cat([out[:, :4], out[:, 4 + cout:]], 1)
        assert bool((side == SENTINEL).all()), '%s %s: a channel outside the slice was written' % (name, variant)
        check('rect_conv', '%s %s' % (name, variant), out[:, 4:4 + cout], refs[torch.float64][variant], refs[torch.float32][variant])
    # operands that start 4 bytes past a 16-byte boundary: the scalar weight loader; the guard elements stay
    ox, xbuf, g = offset_copy(x.numpy())
    ow_, wbuf, _ = offset_copy(wt.numpy())
    assert ox.data_ptr() % 16 == 4 and ow_.data_ptr() % 16 == 4
    out = torch.full((n, cout + EXTRA, oh, ow), SENTINEL, device=DEV)
    ops.conv2d_rect(ox, ow_, tb, stride=s, pad=(ph, pw), act=ops.ACT_RELU, out=out, out_c0=4)
    assert float(xbuf[0]) == g and float(xbuf[-1]) == g and float(wbuf[0]) == g and float(wbuf[-1]) == g
    assert bool((torch.cat([out[:, :4], out[:, 4 + cout:]], 1) == SENTINEL).all())
    check('rect_conv', name + ' offset operands', out[:, 4:4 + cout], refs[torch.float64]['bias_relu'], refs[torch.float32]['bias_relu'])
    # a fresh output (no slice)
    y = ops.conv2d_rect(tx, tw, tb, stride=s, pad=(ph, pw), act=ops.ACT_RELU)
    assert torch.equal(y, kept['bias_relu'][:, 4:4 + cout])
    PLANS_RUN[name] = (plan, plan_off)                           # both forms ran to the end


def test_conv2d_rect_cases_reach_every_plan():
    """the plans the cases of ``RECT`` take (a host query; ``test_conv2d_rect`` launches exactly these and records them) reach every
    tile, both weight loaders and the split and unsplit forms -- and every (tile, loader, split or not) combination the network takes
    at the scoring batch and at one image"""
    plans = [ops.conv2d_rect_plan(ops.rect_desc(c[1], c[2], c[4], c[5], c[3], c[6], c[7], c[8], c[9], c[10], 4, c[3] + EXTRA), a)
             for c in RECT for a in (True, False)]
    if PLANS_RUN:                                                # the parametrised cases ran in this session: what they launched is this list
        ran = [p for c in RECT if c[0] in PLANS_RUN for p in PLANS_RUN[c[0]]]
        assert len(PLANS_RUN) < len(RECT) or ran == plans
    assert {p['tile'] for p in plans} == set(ops.RECT_TILES)
    assert {p['vec'] for p in plans} == {0, 1}
    assert any(p['splits'] > 1 for p in plans) and any(p['splits'] == 1 for p in plans)
    assert {(p['bm'], p['bn']) for p in plans} == {(64, 64), (32, 128), (64, 128)}
    seen = {(p['tile'], p['vec'], p['splits'] > 1) for p in plans}
    for n in (32, 1):
        for u in I.conv_units(299, n):
            p = I.unit_plan(u)
            assert (p['tile'], p['vec'], p['splits'] > 1) in seen, (u, p)


def test_conv2d_rect_rejects():
    x = torch.zeros(1, 3, 9, 9, device=DEV)
    with pytest.raises(RuntimeError):
        ops.conv2d_rect(x, torch.zeros(4, 3, 7, 7, device=DEV))                       # 49 taps
    with pytest.raises(ValueError):
        ops.conv2d_rect(x, torch.zeros(4, 3, 3, 3, device=DEV), out=torch.zeros(1, 4, 9, 9, device=DEV))      # wrong plane
    with pytest.raises(ValueError):
        ops.conv2d_rect(x, torch.zeros(4, 3, 3, 3, device=DEV), out=torch.zeros(1, 5, 7, 7, device=DEV), out_c0=2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.conv2d_rect(x.cpu(), torch.zeros(4, 3, 3, 3))


# =====================================================================================================================================
# 2. pools, resize
# =====================================================================================================================================
@pytest.mark.parametrize('HW', [(7, 7), (8, 8), (35, 35), (9, 6)])
def test_maxpool3s2v(HW):
    H, W = HW
    rs = np.random.RandomState(H * 10 + W)
    for kind in ('random', 'negative', 'nan'):
        x = rs.randn(2, 5, H, W).astype(np.float32)
        if kind == 'negative':
            x = -np.abs(x) - 1
        if kind == 'nan':
            x[0, 1, H // 2, W // 2] = np.nan
            x[1, 4, 0, 0] = np.nan
        want = R.maxpool3s2v_ref(x)
        OH, OW = want.shape[2:]
        assert (OH, OW) == ((H - 3) // 2 + 1, (W - 3) // 2 + 1)
        if (H, W) == (8, 8):                                     # the last column and row are in no window
            x2 = x.copy()
            x2[..., 7] = 1e9
            x2[..., 7, :] = 1e9
            assert np.array_equal(R.maxpool3s2v_ref(x2), want, equal_nan=True)
        assert np.array_equal(want, F.max_pool2d(torch.from_numpy(x), 3, stride=2).numpy(), equal_nan=True)
        for off in (0, 1):
            tx, _, _ = offset_copy(x, off)
            out = torch.full((2, 5 + EXTRA, OH, OW), SENTINEL, device=DEV)
            assert ops.maxpool3s2v(tx, out, 4) is out
            assert np.array_equal(N(out[:, 4:9]), want, equal_nan=True), (kind, off)
            assert bool((torch.cat([out[:, :4], out[:, 9:]], 1) == SENTINEL).all())
        assert np.array_equal(N(ops.maxpool3s2v(T(x))), want, equal_nan=True)
    with pytest.raises(ValueError):
        ops.maxpool3s2v(torch.zeros(1, 1, 2, 5, device=DEV))


@pytest.mark.parametrize('HW', [(1, 1), (3, 3), (17, 17), (5, 8)])
def test_avgpool3s1(HW):
    H, W = HW
    rs = np.random.RandomState(H * 10 + W)
    x = rs.randn(2, 7, H, W).astype(np.float32)
    want32 = R.avgpool3s1_ref(x)                                 # the same taps in the same order, in float32
    t64 = torch.from_numpy(x).double()
    ref64, ref32 = F.avg_pool2d(t64, 3, stride=1, padding=1), F.avg_pool2d(torch.from_numpy(x), 3, stride=1, padding=1)
    for off in (0, 1):
        tx, _, _ = offset_copy(x, off)
        y = ops.avgpool3s1(tx)
        assert np.array_equal(N(y), want32), off
        check('avgpool', 'avgpool3s1 %dx%d' % HW, y, ref64, ref32)
    # count_include_pad=True: the divisor is 9 on the border too -- not the existing sg_avgpool3s2 convention
    excl = F.avg_pool2d(t64, 3, stride=1, padding=1, count_include_pad=False)
    border = torch.ones(H, W, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    got = ops.avgpool3s1(T(x)).double().cpu()
    assert float((got - excl)[..., border].abs().max()) > 1e-3
    if H > 2 and W > 2:
        assert float((got - excl)[..., ~border].abs().max()) < 1e-6
    if (H, W) == (1, 1):
        assert np.array_equal(N(ops.avgpool3s1(T(x))), x / np.float32(9))


@pytest.mark.parametrize('case', [(5, 7, 11, 13), (64, 64, 299, 299), (128, 128, 299, 299), (9, 9, 9, 9), (12, 10, 5, 4)],
                         ids=lambda c: '%dx%d_to_%dx%d' % c)
def test_resize_bilinear(case):
    H, W, OH, OW = case
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H + OW))
    ref64 = F.interpolate(x.double(), size=(OH, OW), mode='bilinear', align_corners=False)
    ref32 = F.interpolate(x, size=(OH, OW), mode='bilinear', align_corners=False)
    assert np.allclose(R.resize_bilinear_ref(x.numpy(), OH, OW), ref64.numpy(), rtol=0, atol=1e-13)
    for off in (0, 1):
        tx, _, _ = offset_copy(x.numpy(), off)
        y = ops.resize_bilinear(tx, (OH, OW))
        check('resize', 'resize %dx%d -> %dx%d off %d' % (H, W, OH, OW, off), y, ref64, ref32)
    if (H, W) == (OH, OW):
        assert torch.equal(ops.resize_bilinear(x.to(DEV), (OH, OW)).cpu(), x)          # the identity is exact


# =====================================================================================================================================
# 3. softmax rows and the score
# =====================================================================================================================================
@pytest.mark.parametrize('classes', [5, 1000])
def test_softmax_rows(classes):
    g = torch.Generator().manual_seed(classes)
    rows = 7
    logits = 4.0 * torch.randn(rows, classes, generator=g)
    logits[1, :] = -80.0
    logits[1, classes // 2] = 80.0                               # exp(-160) underflows: exact zeros around one exact one
    logits[2, ::2] = 80.0
    logits[2, 1::2] = -80.0
    ref64, ref32 = F.softmax(logits.double(), 1), F.softmax(logits, 1)
    assert np.allclose(R.softmax_ref(logits.numpy()), ref64.numpy(), rtol=1e-12, atol=0)
    cap, row0 = 16, 5
    for off in (0, 1):
        buf, whole, guard = offset_copy(np.full((cap, classes), SENTINEL, np.float32), off)
        tl, _, _ = offset_copy(logits.numpy(), off)
        outs = []
        for _ in range(2):
            assert ops.softmax_rows(tl, buf, row0) is buf
            outs.append(buf.clone())
        assert torch.equal(outs[0], outs[1])
        got = buf[row0:row0 + rows]
        check('softmax', 'softmax %d classes off %d' % (classes, off), got, ref64, ref32)
        assert bool((buf[:row0] == SENTINEL).all()) and bool((buf[row0 + rows:] == SENTINEL).all())
        assert float(whole[-1]) == guard
        zeros = ref32 == 0
        assert int(zeros[1].sum()) == classes - 1 and bool((got.cpu()[zeros] == 0).all())
        assert float(got[1, classes // 2]) == 1.0
        assert float((got.double().sum(1) - 1).abs().max()) < 1e-5
    with pytest.raises(RuntimeError):
        ops.softmax_rows(logits.to(DEV), torch.zeros(8, classes, device=DEV), 2)      # 2 + 7 rows do not fit 8


def _probs(n, classes, seed, zeros=True):
    rs = np.random.RandomState(seed)
    p = R.softmax_ref(3.0 * rs.randn(n, classes)).astype(np.float32)
    if zeros:
        p[::2, ::3] = 0.0
        p[1, :] = 0.0
        p[1, 2] = 1.0
    return p


def _close(a, b, rtol=SCORE_RTOL):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= rtol * abs(b)


@pytest.mark.parametrize('shape', [(13, 5), (40, 1000), (257, 1000)], ids=lambda s: '%dx%d' % s)
def test_inception_score_kernel(shape):
    n, classes = shape
    p = _probs(n, classes, n + classes)
    tp, _, _ = offset_copy(p, 1)
    for splits in (1, 5):
        want = R.inception_score_ref(p, splits)
        outs = [ops.inception_score(tp, n, splits) for _ in range(2)]
        assert outs[0].dtype == torch.float64 and tuple(outs[0].shape) == (2 + splits,)
        assert N(outs[0]).tobytes() == N(outs[1]).tobytes()
        got = outs[0].tolist()
        print('score %dx%d splits %d: %.15g +- %.15g (restatement %.15g +- %.15g)' % (n, classes, splits, got[0], got[1], want[0], want[1]))
        assert _close(got[0], want[0]), (got, want)
        assert abs(got[1] - want[1]) <= SCORE_RTOL * abs(want[1]), (got, want)
        assert all(_close(a, b) for a, b in zip(got[2:], want[2]))
    # rows beyond n are not read as part of the score; n = 13 with 5 splits drops rows 10..12
    if n == 13:
        a = ops.inception_score(T(p), 13, 5).tolist()
        b = ops.inception_score(T(p[:10]), 10, 5).tolist()
        assert a == b
        c = ops.inception_score(T(p), 10, 5).tolist()
        assert c == b
        few = ops.inception_score(T(p), 3, 5).tolist()             # n < splits: every part is empty
        assert all(np.isnan(v) for v in few)
        assert all(np.isnan(v) for v in ops.inception_score(T(p), 0, 1).tolist())
        one_hot = np.eye(5, dtype=np.float32)
        assert abs(ops.inception_score(T(one_hot), 5, 1).tolist()[0] - 5.0) < 1e-12


# =====================================================================================================================================
# 4. whole network
# =====================================================================================================================================
@pytest.fixture(scope='module')
def pair():
    """one seeded network, on the CPU as the plain restatement and on the device as the code under test"""
    ref = R.randomise(R.RefInception3(num_classes=1000), 299).eval()
    with skip_random_init():
        net = I.InceptionV3(num_classes=1000)
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, net.to(DEV)


def _net_refs(ref, x):
    with torch.no_grad():
        m64 = copy.deepcopy(ref).double()
        f64, f32 = m64.features(x.double()), ref.features(x)
        return f64, f32, m64.fc(f64), ref.fc(f32)


@pytest.mark.parametrize('size', [139, 299])
def test_network_features_and_logits(pair, size):
    ref, net = pair
    x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(size))
    f64, f32, l64, l32 = _net_refs(ref, x)
    assert float(f64.abs().max()) > 1e-3 and float(l64.std()) > 1e-3           # a live network, not a collapsed one
    tx = x.to(DEV)
    feats = net.features(tx)                                     # (folds the 94 units when the cache is empty)
    assert len(net._fold_cache) == 94
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        logits = net(tx)
        prof = ops.prof_read()
    finally:
        ops.prof_enable(False)
    # one launch per conv unit (plus the slab reductions of the split ones), 4 max-pools + 9 average pools, no BatchNorm pass, no fold
    assert sum(prof[k]['launches'] for k in ('rect_conv_t64', 'rect_conv_t32', 'rect_conv_t64x128')) == 94, prof
    assert prof['rect_reduce']['launches'] == sum(I.unit_plan(u)['splits'] > 1 for u in I.conv_units(size, 2))
    assert prof['inception_pool']['launches'] == 13 and prof['batchnorm']['launches'] == 0 and prof['bn_fold']['launches'] == 0
    assert tuple(feats.shape) == (2, 2048) and tuple(logits.shape) == (2, 1000) and not logits.requires_grad
    check('net', 'inception %d features' % size, feats, f64, f32)
    check('net', 'inception %d logits' % size, logits, l64, l32)
    assert torch.equal(net(tx), logits)                          # bit-identical from run to run
    if size == 139:
        grids = sorted({u['H'] for u in I.conv_units(139, 2) if u['name'].startswith('Mixed_')})
        assert grids == [3, 7, 15]
        # the fold cache follows a write through torch
        with torch.no_grad():
            net.Mixed_5b.branch1x1.bn.weight.mul_(2.0)
            changed = net(tx)
            net.Mixed_5b.branch1x1.bn.weight.mul_(0.5)
        assert not torch.equal(changed, logits) and torch.equal(net(tx), logits)


def test_inception_score_object_end_to_end(pair, capsys):
    """InceptionScore(resize=True) on 64 x 64 images against the restatement: resize, network, softmax and score in float64"""
    ref, net = pair
    # four images that differ in tint and gradient (pure noise images all land on nearly the same softmax row and a score of 1)
    noise = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(64)) * 2 - 1
    tint = torch.tensor([[1., 1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, 1]]).view(4, 3, 1, 1)
    ramp = torch.linspace(-1, 1, 64).view(1, 1, 1, 64) * torch.tensor([1., -1, 0.5, 0]).view(4, 1, 1, 1)
    x = (0.6 * tint + 0.3 * ramp + 0.1 * noise).clamp(-1, 1)
    want = {}
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            up = F.interpolate(x.to(dt), size=(299, 299), mode='bilinear', align_corners=False)
            p = F.softmax(copy.deepcopy(ref).to(dt)(up), 1).numpy()
            want[dt] = R.inception_score_ref(p, 2)
    scorer = I.InceptionScore(batch_size=3, resize=True, weights=net, device=DEV)
    assert 'WITHOUT pretrained weights' not in capsys.readouterr().err
    scorer(x)
    assert scorer.count == 4
    mean, std = scorer.compute_score(splits=2)
    assert isinstance(mean, float) and isinstance(std, float)
    assert want[torch.float64][0] > 1.01 and want[torch.float64][1] > 1e-3      # a score that moves with its inputs
    for name, got, k in (('mean', mean, 0), ('std', std, 1)):
        s64, s32 = want[torch.float64][k], want[torch.float32][k]
        scale = abs(want[torch.float64][0])
        e, yard = abs(got - s64) / scale, max(abs(s32 - s64) / scale, FLOOR)
        ratio = e / yard
        MARGINS.note('score_e2e', ratio, name)
        print('score_e2e  %-6s got %.9g  fp64 %.9g  fp32 %.9g  ratio %.3f' % (name, got, s64, s32, ratio))
        assert ratio <= FACTORS.get('score_e2e', FACTOR), (name, got, s64, s32)


@pytest.fixture(scope='module')
def scorer():
    """a random-weight scorer on small inputs (75 x 75 is the network's minimum): buffer bookkeeping, not accuracy"""
    return I.InceptionScore(batch_size=2, resize=False, weights=None, device=DEV)


def test_scorer_warns_grows_cleans_and_repeats(scorer, capsys):
    I.InceptionScore(batch_size=2, weights=None, device=DEV)
    err = capsys.readouterr().err
    assert 'WITHOUT pretrained weights' in err and 'MEANINGLESS' in err
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        I.InceptionScore(cuda=False)
    g = torch.Generator().manual_seed(5)
    imgs = [torch.rand(5, 3, 75, 75, generator=g) * 2 - 1 for _ in range(4)]

    def run():
        scorer.clean()
        caps = []
        for im in imgs:
            scorer(im.to(DEV))
            caps.append(scorer.probs.size(0))
        return caps, scorer.scores(5).clone(), scorer.probs[:scorer.count].clone()

    scorer.probs = None                                          # start from nothing: 8 rows, then doubled to 16 and 32
    caps, s1, p1 = run()
    assert caps == [8, 16, 16, 32] and scorer.count == 20
    caps2, s2, p2 = run()                                        # clean() keeps the buffer and starts over
    assert caps2 == [32, 32, 32, 32] and scorer.count == 20
    assert torch.equal(p1, p2) and N(s1).tobytes() == N(s2).tobytes()          # two identical runs: bit-identical scores
    assert float((p1.double().sum(1) - 1).abs().max()) < 1e-5
    # the rows survive the growth: against one pass over everything in chunks of the same size
    want = R.inception_score_ref(N(p1), 5)
    mean, std = scorer.compute_score(splits=5)
    assert _close(mean, want[0]) and abs(std - want[1]) <= SCORE_RTOL * abs(want[1])
    logits = torch.cat([scorer.inception_model(torch.cat(imgs)[a:a + 2].to(DEV)) for a in range(0, 20, 2)])
    assert float((F.softmax(logits, 1) - p1).abs().max()) < 1e-5
    scorer.clean()
    assert scorer.count == 0 and all(np.isnan(v) for v in scorer.compute_score(splits=1))


# =====================================================================================================================================
# 5. wiring: check_model and the Sampler
# =====================================================================================================================================
def _sampling_model():
    return SH.sampling_model(Model, DEV)


_batch = SH.sampling_batch


def test_check_model_with_the_scorer():
    from scene_generation_amd.evaluate import check_model
    m = _sampling_model().eval()
    sc = I.InceptionScore(batch_size=4, resize=True, weights=None, device=DEV)
    cfg = type('A', (), {'num_val_samples': 6})()
    loader = [_batch(1), _batch(2), _batch(3)]
    iou, mean, std, fid = check_model(cfg, loader, m, sc, use_gt=True)
    assert sc.count == 6 and fid is None and np.isfinite(iou)
    assert isinstance(mean, float) and isinstance(std, float) and np.isfinite(mean) and np.isfinite(std) and mean >= 1.0 - 1e-9
    again = check_model(cfg, loader, m, sc, use_gt=True)          # clean() at the start of every pass
    assert sc.count == 6 and again[1:3] == (mean, std)


def test_sampler_with_scorer_adds_one_host_read(monkeypatch):
    m, b = _sampling_model(), _batch()
    plain = sample.Sampler(m).sample_batch(b, use_gt_textures=True)
    sc = I.InceptionScore(batch_size=2, resize=True, weights=None, device=DEV)
    s = sample.Sampler(m, inception=sc)
    s.sample_batch(b, use_gt_textures=True)                        # warm-up (fold, buffer)
    sc.clean()
    reads = []
    for name in ('tolist', 'item', 'cpu', 'numpy'):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    sample.Sampler(m).sample_batch(b, use_gt_textures=True)
    base = list(reads)
    del reads[:]
    out = s.sample_batch(b, use_gt_textures=True)
    assert reads == base == ['tolist'], (reads, base)              # the scorer adds no read to a batch
    assert torch.equal(out.images, plain.images) and torch.equal(out.boxes_pred, plain.boxes_pred)
    del reads[:]
    got = s.inception_summary(splits=1)
    assert reads == ['tolist']                                     # exactly one more, at the summary
    assert got['images'] == 3 and got['splits'] == 1 and np.isfinite(got['mean']) and got['std'] == 0.0
    assert sample.Sampler(m).inception_summary() is None


def test_sample_cli_prints_the_inception_line(tmp_path, capsys):
    """``sample --inception_weights PATH``: the scorer is built from a saved state_dict, the result gains ``inception`` and exactly one
    ``Inception MEAN STD`` line is printed; with the flag absent every other output is what it was"""
    import random
    from trainer_helpers import _batch as ema_batch, _run, _trainer
    tr, ck, args = _trainer(tmp_path / 'train')
    _run(tr, ema_batch(), range(1))
    path = tr.save_checkpoint(ck, 1, args, 0)
    torch.manual_seed(3)
    weights = str(tmp_path / 'inception.pth')
    torch.save({'module.' + k: v for k, v in I.InceptionV3().state_dict().items()}, weights)
    base = ['--checkpoint', path, '--use_gt_boxes', '1', '--use_gt_masks', '1', '--use_gt_textures', '1', '--batch_size', '3',
            '--num_samples', '6']
    capsys.readouterr()
    random.seed(0)
    res0 = sample.main(base + ['--output_dir', str(tmp_path / 'a')])
    out0 = capsys.readouterr()
    random.seed(0)
    res1 = sample.main(base + ['--output_dir', str(tmp_path / 'b'), '--inception_weights', weights, '--inception_splits', '2'])
    out1 = capsys.readouterr()
    assert 'inception' not in res0 and 'Inception' not in out0.out
    assert 'WITHOUT pretrained weights' not in out1.err          # the file was loaded
    lines = [l for l in out1.out.splitlines() if l.startswith('Inception ')]
    assert len(lines) == 1 and [l for l in out1.out.splitlines() if l not in lines] == out0.out.splitlines()
    inc = res1['inception']
    assert inc['images'] == 6 and inc['splits'] == 2 and np.isfinite(inc['mean']) and np.isfinite(inc['std']) and inc['mean'] >= 1 - 1e-9
    assert lines[0] == 'Inception {} {}'.format(inc['mean'], inc['std'])
    for p0, p1 in zip(res0['paths'], res1['paths']):
        assert open(p0, 'rb').read() == open(p1, 'rb').read()
