"""The Frechet Inception Distance on the GPU (csrc/fid.hip, ops/fid.py, scene_generation_amd/fid.py, the FID form of
scene_generation_amd/inception.py).

* The moment update (f64 matrix cores) is compared EXACTLY on integer data -- a wrong f64 lane map, k tail or D tail moves whole
  entries -- and on ReLU-ed Gaussian data against the standard summation bound (the products of float32 values are exact in float64).
* The finalize is compared with np.mean / np.cov on data that lies on a 2^-10 grid: its sums and products are then exact in float64,
  so what is measured is the finalize alone (the summation order is the float-moments test's subject).
* The two pools are compared bit for bit with the NumPy restatements of tests/fid_ref.py.
* The FID form of the network follows the yardstick rule of tests/test_gpu_inception.py: error over the error of torch's own float32
  CPU run of the same restatement, floor 2^-24, factor 16 -- halved to 8 after the worst ratio was measured under 2 at 16
  (profiles/fid_test_margins.md).
* End to end, ``compute()`` is compared with the exact nuclear-norm distance of the same device features; the yardstick is the
  disagreement of the two host forms on those features, floored at 2^-50 (tr S1 + tr S2), the bound 64 x that.
The worst ratios go to fid_margins.json in the suite's output directory.  The tree only: no reference checkout."""
import copy

import numpy as np
import pytest
import torch

import fid_ref as FR
import inception_ref as R
import sampling_helpers as SH
from gpu_harness import METRIC_GUARD, Margins, N, _place, margins_fixture
from sampling_helpers import _images
from conftest import skip_random_init
from scene_generation_amd import fid as FID
from scene_generation_amd import inception as I
from scene_generation_amd import ops, sample
from scene_generation_amd.model import Model
from scene_generation_amd.synthetic import make_batch, make_sampling_vocab

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 16.0                    # the project's value for a family not yet measured
# both families measured under 2 on an MI355X at the factor 16 (profiles/fid_test_margins.md): halved to 8, that file's convention
FACTORS = {'fid_net': 8.0, 'plain_net': 8.0}
FLOOR = 2.0 ** -24
E2E_FACTOR, E2E_FLOOR = 64.0, 2.0 ** -50
U = 2.0 ** -53
GUARD = METRIC_GUARD
MARGINS = Margins()
_write_margins = margins_fixture(lambda: MARGINS.dump_yardstick('fid_margins.json', FACTORS, FACTOR))


# =====================================================================================================================================
# 1-4. the moments
# =====================================================================================================================================
#          rows / calls              D     ldx - D  element offset of x
SHAPES = [((1,), 16, 0, 0), ((3,), 16, 0, 0), ((4,), 48, 0, 0), ((5,), 100, 0, 1), ((37,), 100, 3, 0), ((64,), 2048, 0, 0),
          ((32, 32, 32, 32, 2), 2048, 0, 0)]
IDS = ['%s_x%d%s%s' % ('+'.join(map(str, s[0])), s[1], '_ldx%d' % (s[1] + s[2]) if s[2] else '', '_off4B' if s[3] else '') for s in SHAPES]


def _accumulate(chunks, D, extra=0, off=0):
    """feed the chunks to guarded moment buffers -> (sum, outer) as NumPy arrays; the guards must survive"""
    sbuf = torch.full((D + 2,), GUARD, dtype=torch.float64, device=DEV)
    obuf = torch.full((D * D + 2,), GUARD, dtype=torch.float64, device=DEV)
    s, o = sbuf[1:1 + D], obuf[1:1 + D * D].view(D, D)
    s.zero_()
    o.zero_()
    for c in chunks:
        ops.fid_moments_update(_place(c, extra, off), s, o)
    assert sbuf[0].item() == GUARD and sbuf[-1].item() == GUARD and obuf[0].item() == GUARD and obuf[-1].item() == GUARD
    return N(s), N(o)


def _split(x, calls):
    assert sum(calls) == x.shape[0]
    edges = np.cumsum((0,) + tuple(calls))
    return [x[a:b] for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_moments_exact_on_integers(shape):
    calls, D, extra, off = shape
    rs = np.random.RandomState(D + sum(calls))
    x = rs.randint(-8, 9, size=(sum(calls), D)).astype(np.float32)
    want_s, want_o = FR.int_moments(x)
    s, o = _accumulate(_split(x, calls), D, extra, off)
    assert np.array_equal(s, want_s.astype(np.float64))
    bad = np.triu(o != want_o.astype(np.float64))
    assert not bad.any(), 'outer: %d wrong entries of the upper triangle, first at %s' % (bad.sum(), np.argwhere(bad)[0])


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_moments_float_within_the_summation_bound(shape):
    """|outer - ref| <= 2 (rows + calls) 2^-53 sum_k |x_ki||x_kj|: each of the two float64 sums (ours, the reference's) makes at most
    rows + calls roundings of partial sums bounded by that total; sum likewise"""
    calls, D, extra, off = shape
    rs = np.random.RandomState(D + sum(calls) + 1)
    x = FR.relu_gauss(rs, sum(calls), D)
    want_s, want_o, abs_s, abs_o = FR.float_moments(x)
    s, o = _accumulate(_split(x, calls), D, extra, off)
    g = 2.0 * (sum(calls) + len(calls)) * U
    es, eo = np.abs(s - want_s), np.triu(np.abs(o - want_o))
    with np.errstate(invalid='ignore', divide='ignore'):
        worst = max(np.nanmax(np.where(abs_s > 0, es / (g * abs_s), 0)), np.nanmax(np.where(abs_o > 0, eo / (g * abs_o), 0)))
    print('float moments %s: worst share of the bound %.3f' % (shape, worst))
    assert (es <= g * abs_s).all() and (eo <= g * np.triu(abs_o)).all()


@pytest.mark.parametrize('shape', [(3, 16), (37, 100), (64, 2048)], ids=lambda s: '%dx%d' % s)
def test_finalize_against_numpy(shape):
    n, D = shape
    rs = np.random.RandomState(n + D)
    x = (np.round(FR.relu_gauss(rs, n, D) * 1024) / 1024).astype(np.float32)         # a 2^-10 grid: sums and products exact in float64
    want_s, want_o, _, _ = FR.float_moments(x)
    s, o = torch.zeros(D, dtype=torch.float64, device=DEV), torch.zeros(D, D, dtype=torch.float64, device=DEV)
    ops.fid_moments_update(torch.from_numpy(x).to(DEV), s, o)
    assert np.array_equal(N(s), want_s) and np.array_equal(np.triu(N(o)), np.triu(want_o))
    o[torch.tril(torch.ones(D, D, dtype=torch.bool, device=DEV), -1)] = float('nan')      # the lower triangle is never read
    mu, sigma = ops.fid_moments_finalize(s, o, n)
    assert mu.dtype == torch.float64 and tuple(mu.shape) == (D,) and tuple(sigma.shape) == (D, D)
    mu, sigma = N(mu), N(sigma)
    assert sigma.tobytes() == np.ascontiguousarray(sigma.T).tobytes()                  # symmetric bit for bit
    x64 = x.astype(np.float64)
    ref_mu, ref_sigma = np.mean(x64, axis=0), np.cov(x64, rowvar=False)
    assert (np.abs(mu - ref_mu) <= 2 * np.spacing(np.abs(ref_mu))).all()
    bound = (n + 4) * U * (np.abs(want_o) + np.abs(np.outer(want_s, want_s)) / n) / (n - 1)
    err = np.abs(sigma - ref_sigma)
    with np.errstate(invalid='ignore', divide='ignore'):
        print('finalize %dx%d: worst share of the bound %.3f' % (n, D, np.nanmax(np.where(bound > 0, err / bound, 0))))
    assert (err <= bound).all()
    flat = torch.empty(D + D * D, dtype=torch.float64, device=DEV)                     # into a caller's buffer: the same bits
    m2, s2 = ops.fid_moments_finalize(s, o, n, out=flat)
    assert m2.data_ptr() == flat.data_ptr() and N(s2).tobytes() == sigma.tobytes() and N(m2).tobytes() == mu.tobytes()
    with pytest.raises(RuntimeError, match='sg_fid_moments_finalize'):
        ops.fid_moments_finalize(s, o, 1)


def test_moments_deterministic_and_merge():
    rs = np.random.RandomState(9)
    D = 200
    x = rs.randint(-8, 9, size=(70, D)).astype(np.float32)
    xf = FR.relu_gauss(rs, 70, D)
    runs = [_accumulate(_split(xf, (32, 32, 6)), D) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and np.triu(runs[0][1]).tobytes() == np.triu(runs[1][1]).tobytes()
    a, b = FID.FeatureMoments(D, DEV), FID.FeatureMoments(D, DEV)
    for c in _split(x[:33], (32, 1)):
        a.update(torch.from_numpy(c).to(DEV))
    b.update(torch.from_numpy(x[33:]).to(DEV))
    assert (a.count, b.count) == (33, 37)
    assert a.merge(b) is a and a.count == 70
    want_s, want_o = FR.int_moments(x)
    assert np.array_equal(N(a.sum), want_s) and np.array_equal(np.triu(N(a.outer)), np.triu(want_o))
    mu, sigma = a.statistics()
    assert mu.dtype == np.float64 and np.allclose(mu, x.astype(np.float64).mean(0), rtol=1e-14, atol=1e-15)
    assert np.allclose(sigma, np.cov(x.astype(np.float64), rowvar=False), rtol=0, atol=1e-12)
    a.clean()
    assert a.count == 0 and float(a.sum.abs().sum()) == 0 and float(a.outer.abs().sum()) == 0
    with pytest.raises(ValueError):
        a.statistics()
    with pytest.raises(ValueError):
        a.merge(FID.FeatureMoments(D + 1, DEV))


def test_moment_operator_rejects():
    s, o = torch.zeros(8, dtype=torch.float64, device=DEV), torch.zeros(8, 8, dtype=torch.float64, device=DEV)
    x = torch.zeros(3, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.fid_moments_update(x, s, torch.zeros(8, 9, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        ops.fid_moments_update(x, s.float(), o)
    with pytest.raises(ValueError):
        ops.fid_moments_update(torch.zeros(3, 7, device=DEV), s, o)
    with pytest.raises(TypeError):
        ops.fid_moments_update(x.double(), s, o)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.fid_moments_update(x.cpu(), s, o)
    ops.fid_moments_update(torch.ones(8, 3, device=DEV).t(), s, o)                      # a transposed view is made contiguous
    ops.fid_moments_update(x[:0], s, o)                                                # no rows: nothing happens
    assert N(s).tolist() == [3.0] * 8 and float(o[0, 7]) == 3.0


# =====================================================================================================================================
# 5. the two pools
# =====================================================================================================================================
@pytest.mark.parametrize('HW', [(1, 1), (2, 3), (8, 8), (17, 17)], ids=lambda s: '%dx%d' % s)
def test_branch_pools_bit_exact(HW):
    H, W = HW
    rs = np.random.RandomState(H * 10 + W)
    x = rs.randn(2, 3, H, W).astype(np.float32)
    cases = {'random': x, 'neg_inf': x.copy(), 'nan': x.copy()}
    cases['neg_inf'][0, 1] = -np.inf                              # a whole plane of -inf: the maximum is -inf, not the padding's
    cases['neg_inf'][1, 2, H // 2, W // 2] = -np.inf
    cases['nan'][0, 0, H // 2, W // 2] = np.nan
    cases['nan'][1, 1, 0, 0] = np.nan
    for kind, a in cases.items():
        want = FR.maxpool3s1_ref(a)
        assert np.array_equal(want, torch.nn.functional.max_pool2d(torch.from_numpy(a), 3, stride=1, padding=1).numpy(), equal_nan=True)
        for off in (0, 1):
            buf = torch.from_numpy(np.concatenate([np.zeros(off, np.float32), a.reshape(-1)])).to(DEV)
            t = buf[off:].view(a.shape)
            assert np.array_equal(N(ops.maxpool3s1(t)), want, equal_nan=True), (kind, off)
            if kind == 'random':
                assert np.array_equal(N(ops.avgpool3s1x(t)), FR.avgpool3s1x_ref(a)), off
    if (H, W) == (1, 1):
        assert np.array_equal(N(ops.avgpool3s1x(torch.from_numpy(x).to(DEV))), x)      # one tap, divisor 1
    ref64 = torch.nn.functional.avg_pool2d(torch.from_numpy(x).double(), 3, stride=1, padding=1, count_include_pad=False).numpy()
    assert np.allclose(N(ops.avgpool3s1x(torch.from_numpy(x).to(DEV))), ref64, rtol=0, atol=1e-6)


# =====================================================================================================================================
# 6. the FID form of the network
# =====================================================================================================================================
def _check(family, name, got, ref64, ref32):
    MARGINS.yardstick(family, name, got, ref64, ref32, FACTORS, FACTOR, FLOOR)


@pytest.fixture(scope='module')
def fid_pair():
    ref = R.randomise(FR.RefFidInception3(num_classes=1008), 75).eval()
    with skip_random_init():
        net = I.InceptionV3(num_classes=1008, aux_logits=False, fid_variant=True)
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, net.to(DEV)


def test_fid_form_features_and_logits(fid_pair):
    ref, net = fid_pair
    x = torch.randn(2, 3, 75, 75, generator=torch.Generator().manual_seed(75))
    with torch.no_grad():
        m64 = copy.deepcopy(ref).double()
        f64, f32 = m64.features(x.double()), ref.features(x)
        l64, l32 = m64.fc(f64), ref.fc(f32)
    assert float(f64.abs().max()) > 1e-3 and float(l64.std()) > 1e-3
    tx = x.to(DEV)
    feats, logits = net.features(tx), net(tx)
    assert tuple(feats.shape) == (2, 2048) and tuple(logits.shape) == (2, 1008)
    _check('fid_net', 'fid inception 75 features', feats, f64, f32)
    _check('fid_net', 'fid inception 75 logits', logits, l64, l32)
    assert torch.equal(net(tx), logits)
    # fid_variant=False is the existing network: the default and the explicit flag agree bit for bit on the same weights, follow the
    # plain restatement (torchvision's pools), and differ from the FID form
    plain_ref = R.RefInception3(num_classes=1008, aux_logits=False)
    plain_ref.load_state_dict(ref.state_dict(), strict=True)
    plain_ref.eval()
    with skip_random_init():
        plain, explicit = I.InceptionV3(num_classes=1008, aux_logits=False), I.InceptionV3(1008, False, fid_variant=False)
    for m in (plain, explicit):
        m.load_state_dict(ref.state_dict(), strict=True)
        m.to(DEV)
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        lp = plain(tx)
        prof = ops.prof_read()
        ops.prof_reset()
        net(tx)
        prof_fid = ops.prof_read()
    finally:
        ops.prof_enable(False)
    assert torch.equal(lp, explicit(tx)) and not torch.equal(lp, logits)
    assert prof['inception_pool']['launches'] == prof_fid['inception_pool']['launches'] == 13       # the same launches, other pools
    with torch.no_grad():
        p64, p32 = copy.deepcopy(plain_ref).double()(x.double()), plain_ref(x)
    _check('plain_net', 'default pools, 1008 classes', lp, p64, p32)


# =====================================================================================================================================
# 7-9. the object, end to end and in its callers
# =====================================================================================================================================
@pytest.fixture(scope='module')
def fid_net():
    """the seeded random FID-form network ``FrechetInceptionDistance(weights=None)`` builds"""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        return I.InceptionV3(num_classes=1008, aux_logits=False, fid_variant=True).to(DEV)


def test_end_to_end_against_the_nuclear_norm(fid_net, capsys):
    f = FID.FrechetInceptionDistance(weights=None, resize=False, batch_size=8, device=DEV)
    err = capsys.readouterr().err
    assert 'WITHOUT pretrained weights' in err and 'MEANINGLESS' in err
    assert f.inception_model.fid_variant and f.needs_real
    assert all(torch.equal(a, b) for a, b in zip(f.inception_model.state_dict().values(), fid_net.state_dict().values()))
    real, fake = _images(24, 1).to(DEV), (_images(21, 2) * 0.8 + 0.1).to(DEV)
    with pytest.raises(ValueError, match='fake side'):
        f.compute()
    f.add_real(real)
    f(fake)                                                       # chunks of 8, 8 and a tail of 5
    assert (f.real.count, f.fake.count) == (24, 21)
    got = f.compute()
    assert isinstance(got, float) and not f.needs_real
    feats = [torch.cat([fid_net.features(x[a:a + 8]) for a in range(0, x.size(0), 8)]).cpu().numpy() for x in (real, fake)]
    want, scale = FR.fid_nuclear(*feats)
    host = FID.frechet_distance(*FR.stats(feats[0]), *FR.stats(feats[1]))
    yard = max(abs(host - want), E2E_FLOOR * scale)
    ratio = abs(got - want) / yard
    MARGINS.extra['fid_e2e'] = {'ratio_of_yardstick': ratio, 'bound': E2E_FACTOR, 'fid': got, 'nuclear': want, 'host_symmetric': host,
                                'trace_scale': scale}
    print('fid_e2e  got %.17g  nuclear %.17g  host symmetric form %.17g  scale %.6g  ratio %.3f' % (got, want, host, scale, ratio))
    assert want > 1e-6 * scale                                    # two sets that differ
    assert ratio <= E2E_FACTOR, (got, want, host, scale)
    # clean() clears the fake side only; the real side stays closed and is reused
    f.clean()
    assert f.fake.count == 0 and f.real.count == 24 and not f.needs_real
    with pytest.raises(ValueError, match='fake side'):
        f.compute()
    f.clean_real()
    assert f.needs_real and f.real.count == 0


def test_shared_forward_with_the_inception_score(fid_net):
    rs = np.random.RandomState(4)
    real_stats = FR.stats(FR.relu_gauss(rs, 40, 2048))
    imgs = _images(10, 3).to(DEV)
    f = FID.FrechetInceptionDistance(weights=fid_net, real_stats=real_stats, resize=False, batch_size=4, device=DEV)
    g = FID.FrechetInceptionDistance(weights=fid_net, real_stats=real_stats, resize=False, batch_size=4, device=DEV)
    assert not f.needs_real
    with pytest.raises(RuntimeError):
        f.add_real(imgs)
    plain = I.InceptionScore(batch_size=4, resize=False, weights=fid_net, device=DEV)
    shared = I.InceptionScore(batch_size=4, resize=False, weights=fid_net, device=DEV, fid=f)
    assert plain.fid is None and shared.fid is f
    plain(imgs)
    shared(imgs)
    g(imgs)
    assert torch.equal(plain.probs[:10], shared.probs[:10])
    assert plain.compute_score(splits=2) == shared.compute_score(splits=2)
    assert f.fake.count == g.fake.count == 10
    assert torch.equal(f.fake.sum, g.fake.sum) and torch.equal(torch.triu(f.fake.outer), torch.triu(g.fake.outer))
    a, b = f.compute(), g.compute()
    assert a == b and np.isfinite(a)


def _sampling_model():
    m = SH.small_model(Model, make_sampling_vocab(SH.C, 7, SH.A)).to(DEV)
    m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    return m


def _batch(seed=321):
    return make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=SH.C, num_preds=7, num_attributes=35, seed=seed)


def test_check_model_and_sampler_with_fid(fid_net):
    from scene_generation_amd.evaluate import check_model
    m = _sampling_model().eval()
    cfg = type('A', (), {'num_val_samples': 6})()
    loader = [_batch(1), _batch(2), _batch(3)]
    assert check_model(cfg, loader, m, None, use_gt=True)[3] is None
    f = FID.FrechetInceptionDistance(weights=fid_net, resize=True, batch_size=4, device=DEV)
    iou, mean, std, value = check_model(cfg, loader, m, None, use_gt=True, fid=f)
    assert mean is None and std is None and isinstance(value, float) and np.isfinite(value) and np.isfinite(iou)
    assert (f.real.count, f.fake.count) == (6, 6) and not f.needs_real
    # the manual computation: the same images through a second object, in the same chunks
    manual = FID.FrechetInceptionDistance(weights=fid_net, resize=True, batch_size=4, device=DEV)
    with torch.no_grad():
        for batch in loader[:2]:
            imgs, objs, boxes, masks, triples, obj_to_img, _, attributes = [t.to(DEV) for t in batch]
            out = m(imgs, objs, triples, obj_to_img, boxes_gt=boxes, masks_gt=masks, attributes=attributes, test_mode=True, use_gt_box=True)
            manual.add_real(imgs)
            manual(out[0])
    assert manual.compute() == value
    # a second pass through a scorer that shares its forward: the real side is reused, the fake side fed by the scorer alone
    sc = I.InceptionScore(batch_size=4, resize=True, weights=fid_net, device=DEV, fid=f)
    again = check_model(cfg, loader, m, sc, use_gt=True, fid=f)
    assert (f.real.count, f.fake.count, sc.count) == (6, 6, 6) and again[3] == value and np.isfinite(again[1])
    # the sampler feeds the fake side once per batch, through the scorer when they share a forward
    f.clean()
    s = sample.Sampler(m, inception=sc, fid=f)
    s.sample_batch(_batch(), use_gt_textures=True)
    assert f.fake.count == 3
    sample.Sampler(m, fid=f).sample_batch(_batch(), use_gt_textures=True)
    assert f.fake.count == 6
    got = s.fid_summary()
    assert got['images'] == 6 and np.isfinite(got['fid']) and sample.Sampler(m).fid_summary() is None


def test_cli_directories_and_statistics_file(tmp_path, capsys):
    Image = pytest.importorskip('PIL.Image')
    for name, seed in (('real', 5), ('fake', 6)):
        (tmp_path / name).mkdir()
        px = ((_images(3, seed, 40) * 0.5 + 0.5) * 255).round().byte().permute(0, 2, 3, 1).numpy()
        for i in range(3):
            Image.fromarray(px[i]).save(str(tmp_path / name / ('%d.png' % i)))
    stats = str(tmp_path / 'real.npz')
    a = FID.main(['--real', str(tmp_path / 'real'), '--fake', str(tmp_path / 'fake'), '--save_stats', stats, '--batch_size', '2'])
    out = capsys.readouterr()
    assert 'WITHOUT pretrained weights' in out.err and out.out.strip().splitlines()[-1] == 'FID {}'.format(a)
    with np.load(stats) as z:
        assert sorted(z.files) == ['mu', 'n', 'sigma'] and int(z['n']) == 3 and z['sigma'].shape == (2048, 2048)
    b = FID.main(['--real', stats, '--fake', str(tmp_path / 'fake'), '--batch_size', '2'])
    assert a == b and np.isfinite(a)
    with pytest.raises(SystemExit):
        FID.main(['--real', str(tmp_path / 'none'), '--fake', str(tmp_path / 'fake')])
