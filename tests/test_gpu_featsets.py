"""KID and precision / recall on the GPU (csrc/featsets.hip, ops/featsets.py, scene_generation_amd/featsets.py).

* Exact on integer data, bit for bit against the int64 oracle of tests/featsets_ref.py, every output between guard words: a wrong
  f64 lane map, gather, tile enumeration, diagonal rule, k tail or D tail moves whole entries.  The oracle's sum of |k| is asserted
  below 2^53, so exactness is meaningful.
* Float data (ReLU-ed Gaussian rows) against the derived summation bounds (tests/featsets_ref.py): kernel sums within
  2 u [(3 D + 9) + P] sum T^3, distances within 2 (D + 2) u (|a|^2 + |b|^2 + 2 sum|a_k b_k|), KID within the propagated bound,
  membership decisions exact outside the rounding band (at most 0.1 % of pairs may fall inside it).
* Behaviour: bit-identical repeats, the bank, the metrics object against the restatement on the same device features, the shared
  forward, check_model, the sampler and the command lines.
The worst share of each bound goes to featsets_margins.json in the suite's output directory (profiles/featsets_test_margins.md).
The tree only: no reference checkout."""
import numpy as np
import pytest
import torch

import featsets_ref as R
import sampling_helpers as SH
from gpu_harness import Margins, N, _guarded, _guards_ok, _place, margins_fixture
from sampling_helpers import _images
from scene_generation_amd import featsets as FS
from scene_generation_amd import fid as FID
from scene_generation_amd import inception as I
from scene_generation_amd import ops, sample
from scene_generation_amd.model import Model
from scene_generation_amd.synthetic import make_batch, make_sampling_vocab

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MARGINS = Margins()
_write_margins = margins_fixture(lambda: MARGINS.dump('featsets_margins.json', 'share_of_bound', empty=False))


def poly_sums(x, y, ix, iy, gamma, coef0, degree, extra=0, off=0):
    buf, out = _guarded((ix.shape[0], 3), torch.float64)
    got = ops.feat_poly_sums(_place(x, extra, off), _place(y, extra, off), ix, iy, gamma, coef0, degree, out=out)
    assert got is out and _guards_ok(buf)
    return N(out)


def knn_radius(x, k, extra=0, off=0):
    buf, out = _guarded((x.shape[0],), torch.float64)
    assert ops.feat_knn_radius(_place(x, extra, off), k, out=out) is out and _guards_ok(buf)
    return N(out)


def manifold_counts(a, r2, b, extra=0, off=0):
    cbuf, count = _guarded((b.shape[0],), torch.int32)
    mbuf, mind2 = _guarded((a.shape[0],), torch.float64)
    ops.feat_manifold_counts(_place(a, extra, off), torch.from_numpy(np.asarray(r2, np.float64)).to(DEV), _place(b, extra, off),
                             count=count, mind2=mind2)
    assert _guards_ok(cbuf) and _guards_ok(mbuf)
    return N(count), N(mind2)


# =====================================================================================================================================
# 1. exact on integer data
# =====================================================================================================================================
def _tables(rs, S, s, n, m):
    """tables that name row 0 and the last row, give one row two positions of a subset and repeat a row across subsets"""
    out = []
    for rows in (n, m):
        t = rs.randint(0, rows, size=(S, s)).astype(np.int32)
        t[0, 0], t[0, s - 1] = 0, rows - 1
        if s >= 3:
            t[0, 1] = t[0, 0]                       # the same row at two positions of one subset: both positions count
        elif S > 1:
            t[1, 1] = t[1, 0]
        if S > 1:
            t[S - 1, 0] = t[0, s - 1]               # a row that several subsets share
        out.append(t)
    return out


@pytest.mark.parametrize('D', [4, 6, 64, 70])
def test_poly_sums_exact_on_integers(D):
    rs = np.random.RandomState(D)
    worst = 0
    for s in (2, 5, 64, 65):
        for S in (1, 3):
            for n, m in ((s, s), (s, 130), (130, s), (130, 130)):
                x = rs.randint(-3, 4, size=(n, D)).astype(np.float32)
                y = rs.randint(-3, 4, size=(m, D)).astype(np.float32)
                ix, iy = _tables(rs, S, s, n, m)
                want, mass = R.poly_sums_int(x, y, ix, iy, 1, 1, 3)
                assert mass < 2 ** 53
                worst = max(worst, mass)
                pad = (3, 1) if (s, S) == (65, 3) else (0, 0)                   # a padded row stride, a base 4 bytes into a vector
                got = poly_sums(x, y, ix, iy, 1.0, 1.0, 3, *pad)
                assert np.array_equal(got, want.astype(np.float64)), (D, s, S, n, m, got, want)
    print('poly sums D=%d: largest sum of |k| %.3g (2^53 = %.3g)' % (D, worst, 2.0 ** 53))


def test_poly_sums_exact_on_integers_2048():
    rs = np.random.RandomState(2048)
    D, s = 2048, 70
    for S, (n, m) in ((1, (s, 130)), (3, (130, s))):
        x = rs.randint(-1, 3, size=(n, D)).astype(np.float32)
        y = rs.randint(-1, 3, size=(m, D)).astype(np.float32)
        ix, iy = _tables(rs, S, s, n, m)
        want, mass = R.poly_sums_int(x, y, ix, iy, 1, 1, 3)
        print('poly sums D=2048 s=70: sum of |k| %.3g (2^53 = %.3g)' % (mass, 2.0 ** 53))
        assert mass < 2 ** 53
        assert np.array_equal(poly_sums(x, y, ix, iy, 1.0, 1.0, 3), want.astype(np.float64))


@pytest.mark.parametrize('degree', [1, 2, 4])
def test_poly_sums_other_degrees(degree):
    rs = np.random.RandomState(degree)
    n, m, D, s, S = 130, 70, 6, 65, 3
    x = rs.randint(-2, 3, size=(n, D)).astype(np.float32)
    y = rs.randint(-2, 3, size=(m, D)).astype(np.float32)
    ix, iy = _tables(rs, S, s, n, m)
    want, mass = R.poly_sums_int(x, y, ix, iy, 2, -1, degree)                  # another gamma and a negative coef0 on the way
    assert mass < 2 ** 53
    assert np.array_equal(poly_sums(x, y, ix, iy, 2.0, -1.0, degree), want.astype(np.float64))


NS = (4, 63, 64, 65, 130)


@pytest.mark.parametrize('D', [6, 70])
def test_knn_radius_exact_on_integers(D):
    rs = np.random.RandomState(100 + D)
    for n in NS:
        x = rs.randint(-3, 4, size=(n, D)).astype(np.float32)
        if n >= 8:
            x[n // 2] = x[0]                        # duplicated rows: a distance of zero that is not the row itself
            x[n - 1] = x[1]
            x[n - 2] = x[1]
        d2 = R.dist2_int(x, x)
        for k in (1, 3, 8):
            if n <= k:
                continue
            want = R.knn_radius(d2, k)
            got = knn_radius(x, k, *((3, 1) if n == 65 else (0, 0)))
            assert np.array_equal(got, want.astype(np.float64)), (n, k, np.argwhere(got != want)[:4])
    with pytest.raises(ValueError, match='k \\+ 1'):
        ops.feat_knn_radius(torch.zeros(3, 4, device=DEV), 3)


@pytest.mark.parametrize('D', [6, 70])
def test_manifold_counts_exact_on_integers(D):
    rs = np.random.RandomState(200 + D)
    for n, m in ((4, 63), (63, 64), (64, 65), (65, 130), (130, 4), (130, 65)):
        a = rs.randint(-3, 4, size=(n, D)).astype(np.float32)
        b = rs.randint(-3, 4, size=(m, D)).astype(np.float32)
        b[0] = a[n - 1]                             # a query on a reference: d2 = 0 <= any radius
        r2 = R.knn_radius(R.dist2_int(a, a), 3)     # integer radii: d2 == r2 happens, and <= decides it exactly
        d2 = R.dist2_int(a, b)
        want_c, want_m = R.manifold_counts(d2, r2)
        assert (d2 == r2[:, None]).any() or D > 6
        got_c, got_m = manifold_counts(a, r2, b, *((3, 1) if n == 65 else (0, 0)))
        assert np.array_equal(got_c, want_c) and np.array_equal(got_m, want_m.astype(np.float64)), (n, m)


# =====================================================================================================================================
# 2. float data against the summation bounds
# =====================================================================================================================================
FLOAT_SHAPES = [(130, 97, 64), (65, 130, 70), (70, 65, 2048)]


@pytest.fixture(scope='module')
def float_sets():
    out = {}
    for n, m, D in FLOAT_SHAPES:
        x, y = R.relu_gauss(1, n, D), R.relu_gauss(2, m, D)
        out[(n, m, D)] = (x, y)
    return out


@pytest.mark.parametrize('shape', FLOAT_SHAPES, ids=lambda s: '%d_%d_%d' % s)
def test_poly_sums_and_kid_within_the_bound(shape, float_sets):
    n, m, D = shape
    x, y = float_sets[shape]
    s = min(n, m)
    ix, iy = R.draw_subsets(7, 3, s, n, m)
    want, bound = R.poly_sums_float(x, y, ix, iy, 1.0 / D, 1.0, 3)
    got = poly_sums(x, y, ix, iy, 1.0 / D, 1.0, 3)
    share = float((np.abs(got - want) / bound).max())
    print('poly sums %s: worst share of the bound %.4f' % (shape, share))
    MARGINS.note('poly_sums', share, '%d_%d_%d' % shape)
    assert (np.abs(got - want) <= bound).all()
    per = lambda sums: sums[:, 0] / (s * (s - 1.0)) + sums[:, 1] / (s * (s - 1.0)) - 2.0 * sums[:, 2] / (s * s)
    kb = R.kid_bound(bound, s)
    kshare = float((np.abs(per(got) - per(want)) / kb).max())
    print('kid %s: per-subset values %s, worst share of the propagated bound %.4f' % (shape, per(got), kshare))
    MARGINS.note('kid', kshare, '%d_%d_%d' % shape)
    assert (np.abs(per(got) - per(want)) <= kb).all()
    mean, std = FS.kid_from_sums(got, s)
    rmean, rstd = R.kid_from_sums(want, s)
    assert abs(mean - rmean) <= kb.max() and abs(std - rstd) <= 2 * kb.max()


@pytest.mark.parametrize('shape', FLOAT_SHAPES, ids=lambda s: '%d_%d_%d' % s)
def test_manifold_within_the_bound(shape, float_sets):
    n, m, D = shape
    x, y = float_sets[shape]
    k = 3
    dxx, bxx = R.dist2_float(x, x)
    dxy, bxy = R.dist2_float(x, y)
    want_r2 = R.knn_radius(dxx, k)
    got_r2 = knn_radius(x, k)
    rb = bxx.max(1)                                 # the k-th smallest moves by no more than the largest error of its row
    share = float((np.abs(got_r2 - want_r2) / rb).max())
    print('radii %s: worst share of the bound %.4f' % (shape, share))
    MARGINS.note('knn_radius', share, '%d_%d_%d' % shape)
    assert (np.abs(got_r2 - want_r2) <= rb).all()
    got_c, got_m = manifold_counts(x, got_r2, y)
    mshare = float((np.abs(got_m - dxy.min(1)) / bxy.max(1)).max())
    print('nearest query %s: worst share of the bound %.4f' % (shape, mshare))
    MARGINS.note('mind2', mshare, '%d_%d_%d' % shape)
    assert (np.abs(got_m - dxy.min(1)) <= bxy.max(1)).all()
    gap = np.abs(dxy - want_r2[:, None])
    band = gap <= 2.0 * (bxy + rb[:, None])         # pairs the rounding may decide either way, the radius's own error counted
    print('membership %s: %d of %d pairs inside the band; smallest gap %.3g against a band of up to %.3g; precision %.3f'
          % (shape, band.sum(), band.size, gap.min(), (2.0 * (bxy + rb[:, None])).max(), float((got_c > 0).mean())))
    assert band.sum() <= 1e-3 * band.size
    sure = (dxy <= want_r2[:, None]) & ~band
    lo, hi = sure.sum(0), sure.sum(0) + band.sum(0)
    assert ((got_c >= lo) & (got_c <= hi)).all()
    assert 0 < (got_c > 0).sum() < m                # neither all outside nor all inside


# =====================================================================================================================================
# 3. behaviour
# =====================================================================================================================================
def test_outputs_repeat_bit_for_bit(float_sets):
    x, y = float_sets[(130, 97, 64)]
    ix, iy = R.draw_subsets(3, 4, 90, 130, 97)
    tx, ty = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    runs = []
    for _ in range(2):
        sums = ops.feat_poly_sums(tx, ty, ix, iy, 1.0 / 64, 1.0, 3)
        r2 = ops.feat_knn_radius(tx, 3)
        count, mind2 = ops.feat_manifold_counts(tx, r2, ty)
        runs.append(b''.join(N(t).tobytes() for t in (sums, r2, count, mind2)))
    assert runs[0] == runs[1]


def test_wrapper_refuses_an_index_outside_the_set():
    x = torch.zeros(5, 4, device=DEV)
    good = np.zeros((1, 2), np.int32)
    calls = ops.CALLS[0]
    for bad in (np.array([[0, 5]], np.int32), np.array([[-1, 0]], np.int32)):
        with pytest.raises(ValueError, match='outside'):
            ops.feat_poly_sums(x, x, bad, good, 1.0, 1.0, 3)
        with pytest.raises(ValueError, match='outside'):
            ops.feat_poly_sums(x, x, good, bad, 1.0, 1.0, 3)
    with pytest.raises(ValueError):
        ops.feat_poly_sums(x, x, torch.zeros(1, 2, dtype=torch.int32, device=DEV), good, 1.0, 1.0, 3)      # device tables are not checked: refused
    with pytest.raises(ValueError):
        ops.feat_poly_sums(x, x, good, good, 1.0, 1.0, 5)
    assert ops.CALLS[0] == calls                    # nothing was launched


def test_feature_bank_merge_equals_one_bank(tmp_path):
    rs = np.random.RandomState(5)
    rows = torch.from_numpy(rs.randn(70, 16).astype(np.float32)).to(DEV)
    one, a, b = FS.FeatureBank(16, DEV, capacity=8), FS.FeatureBank(16, DEV, capacity=8), FS.FeatureBank(16, DEV)
    for lo, hi in ((0, 32), (32, 33), (33, 70)):
        one.update(rows[lo:hi])
    a.update(rows[:33])
    b.update(rows[33:])
    assert a.merge(b) is a and a.count == one.count == 70 and torch.equal(a.rows(), one.rows()) and torch.equal(one.rows(), rows)
    assert one.buf.size(0) == 128 and one.rows().data_ptr() == one.buf.data_ptr()
    path = str(tmp_path / 'bank.npy')
    one.save(path)
    assert torch.equal(FS.FeatureBank.load(path, DEV).rows(), rows)
    assert torch.equal(ops.feat_knn_radius(a.rows(), 3), ops.feat_knn_radius(rows, 3))


@pytest.fixture(scope='module')
def fid_net():
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        return I.InceptionV3(num_classes=1008, aux_logits=False, fid_variant=True).to(DEV)


def _against_the_restatement(res, real, fake, k, subsets, size, seed):
    want, info = R.metrics(real, fake, k=k, subsets=subsets, size=size, seed=seed)
    print('metrics: got %s\n         want %s\n         %s' % (res, want, info))
    assert sorted(res) == sorted(['kid_mean', 'kid_std', 'kid_subset_size', 'precision', 'recall', 'density', 'coverage', 'real', 'fake'])
    assert (res['real'], res['fake'], res['kid_subset_size']) == (want['real'], want['fake'], want['kid_subset_size'])
    assert abs(res['kid_mean'] - want['kid_mean']) <= info['kid_bound'] and abs(res['kid_std'] - want['kid_std']) <= 2 * info['kid_bound']
    n, m = real.shape[0], fake.shape[0]
    assert abs(res['precision'] - want['precision']) <= info['band_precision'] / m
    assert abs(res['recall'] - want['recall']) <= info['band_recall'] / n
    assert abs(res['density'] - want['density']) <= info['band_precision'] / (k * m) + 1e-15
    assert abs(res['coverage'] - want['coverage']) <= info['band_precision'] / n
    return want


def test_metrics_object_on_images_equals_the_restatement(fid_net, capsys):
    sets = FS.FeatureSetMetrics(weights=fid_net, k=3, kid_subsets=4, kid_subset_size=1000, seed=2, resize=False, batch_size=8, device=DEV)
    assert sets.inception_model is None and sets.needs_real and sets.dim == 2048
    real, fake = _images(24, 1).to(DEV), (_images(21, 2) * 0.8 + 0.1).to(DEV)
    sets.add_real(real)
    sets(fake)
    assert (sets.real.count, sets.fake.count) == (24, 21) and sets.inception_model is fid_net
    res = sets.compute()
    assert res['kid_subset_size'] == 21 and not sets.needs_real
    feats = [torch.cat([fid_net.features(x[a:a + 8]) for a in range(0, x.size(0), 8)]) for x in (real, fake)]
    assert torch.equal(sets.real.rows(), feats[0]) and torch.equal(sets.fake.rows(), feats[1])
    _against_the_restatement(res, N(feats[0]), N(feats[1]), 3, 4, 1000, 2)
    r2 = sets._real_r2
    assert sets.compute() == res and sets._real_r2 is r2                            # the same bits; the real radii were kept
    sets.clean()
    assert sets.fake.count == 0 and sets.real.count == 24 and sets._real_r2 is r2
    sets.add_real(real[:3])
    assert sets._real_r2 is None and sets.real.count == 27                          # a changed real side drops them
    with pytest.raises(ValueError, match='fake side'):
        sets.compute()
    # one subset of the full size: the full-set estimator
    full = FS.FeatureSetMetrics(real_features=N(feats[0])[:21], kid_subsets=1, kid_subset_size=21, device=DEV)
    full.add_features(feats[1])
    one = full.compute()
    idx = np.arange(21, dtype=np.int32)[None]
    sums, bound = R.poly_sums_float(N(feats[0])[:21], N(feats[1]), idx, idx, 1.0 / 2048, 1.0, 3)
    assert one['kid_std'] == 0.0 and abs(one['kid_mean'] - R.kid_from_sums(sums, 21)[0]) <= R.kid_bound(bound, 21).max()


def test_shared_forward_through_fid_and_the_inception_score(fid_net):
    imgs, real = _images(10, 3).to(DEV), _images(9, 4).to(DEV)
    sets = FS.FeatureSetMetrics(weights=fid_net, kid_subsets=2, resize=False, batch_size=4, device=DEV)
    f = FID.FrechetInceptionDistance(weights=fid_net, resize=False, batch_size=4, device=DEV, sets=sets)
    g = FID.FrechetInceptionDistance(weights=fid_net, resize=False, batch_size=4, device=DEV)
    plain = I.InceptionScore(batch_size=4, resize=False, weights=fid_net, device=DEV)
    shared = I.InceptionScore(batch_size=4, resize=False, weights=fid_net, device=DEV, fid=f)
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        plain(imgs)
        p0 = ops.prof_read()
        ops.prof_reset()
        shared(imgs)
        p1 = ops.prof_read()
    finally:
        ops.prof_enable(False)
    conv = lambda p: sum(v['launches'] for name, v in p.items() if name.startswith('rect_conv'))
    assert conv(p0) == conv(p1) > 0                                                 # one forward, not two
    assert torch.equal(plain.probs[:10], shared.probs[:10])                         # logits bit-identical to the unattached run
    assert f.fake.count == 10 and sets.fake.count == 10 and sets.inception_model is None
    g(imgs)
    assert torch.equal(f.fake.sum, g.fake.sum) and torch.equal(torch.triu(f.fake.outer), torch.triu(g.fake.outer))
    f.add_real(real)
    g.add_real(real)
    assert sets.real.count == 9 and f.real.count == 9
    assert f.compute() == g.compute()
    feats = [torch.cat([fid_net.features(x[a:a + 4]) for a in range(0, x.size(0), 4)]) for x in (real, imgs)]
    assert torch.equal(sets.real.rows(), feats[0]) and torch.equal(sets.fake.rows(), feats[1])
    _against_the_restatement(f.sets.compute(), N(feats[0]), N(feats[1]), 3, 2, 1000, 0)
    f.clean()
    assert sets.fake.count == 0 and sets.real.count == 9
    f.clean_real()
    assert sets.real.count == 0 and sets.needs_real


def _sampling_model():
    m = SH.small_model(Model, make_sampling_vocab(SH.C, 7, SH.A)).to(DEV)
    m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    return m


def _batch(seed=321):
    return make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=SH.C, num_preds=7, num_attributes=35, seed=seed)


def test_check_model_and_sampler_fill_the_attached_object(fid_net):
    from scene_generation_amd.evaluate import check_model
    m = _sampling_model().eval()
    cfg = type('A', (), {'num_val_samples': 6})()
    loader = [_batch(1), _batch(2), _batch(3)]
    sets = FS.FeatureSetMetrics(weights=fid_net, kid_subsets=3, seed=1, resize=True, batch_size=4, device=DEV)
    f = FID.FrechetInceptionDistance(weights=fid_net, resize=True, batch_size=4, device=DEV, sets=sets)
    plain = FID.FrechetInceptionDistance(weights=fid_net, resize=True, batch_size=4, device=DEV)
    value = check_model(cfg, loader, m, None, use_gt=True, fid=f)[3]
    assert value == check_model(cfg, loader, m, None, use_gt=True, fid=plain)[3]     # the distance is what it was
    assert (sets.real.count, sets.fake.count) == (6, 6)
    first = f.sets.compute()
    assert first['real'] == first['fake'] == first['kid_subset_size'] == 6 and all(np.isfinite(v) for v in first.values())
    assert 0.0 <= first['precision'] <= 1.0 and 0.0 <= first['recall'] <= 1.0 and 0.0 <= first['coverage'] <= 1.0
    _against_the_restatement(first, N(sets.real.rows()), N(sets.fake.rows()), 3, 3, 1000, 1)
    # the second pass, through a scorer that shares its forward: the fake side is cleared and refilled, the real side reused
    r2 = sets._real_r2
    sc = I.InceptionScore(batch_size=4, resize=True, weights=fid_net, device=DEV, fid=f)
    again = check_model(cfg, loader, m, sc, use_gt=True, fid=f)
    assert again[3] == value and (sets.real.count, sets.fake.count, sc.count) == (6, 6, 6) and sets._real_r2 is r2
    assert f.sets.compute() == first
    # the sampler: through the distance, through the scorer in the distance's place, and on its own
    f.clean()
    s = sample.Sampler(m, inception=sc, fid=f, sets=sets)
    s.sample_batch(_batch(), use_gt_textures=True)
    assert (f.fake.count, sets.fake.count) == (3, 3)
    sample.Sampler(m, fid=f, sets=sets).sample_batch(_batch(), use_gt_textures=True)
    assert (f.fake.count, sets.fake.count) == (6, 6)
    lone = FS.FeatureSetMetrics(weights=fid_net, real_features=N(sets.real.rows()), kid_subsets=3, seed=1, resize=True, batch_size=4,
                                device=DEV)
    via = I.InceptionScore(batch_size=4, resize=True, weights=fid_net, device=DEV, fid=lone)
    s2 = sample.Sampler(m, inception=via, sets=lone)
    s2.sample_batch(_batch(), use_gt_textures=True)
    s3 = sample.Sampler(m, sets=lone)
    s3.sample_batch(_batch(), use_gt_textures=True)
    assert lone.fake.count == 6 and torch.equal(lone.fake.rows(), sets.fake.rows())
    got = s.featsets_summary()
    assert got == s2.featsets_summary() and got['fake'] == 6 and sample.Sampler(m).featsets_summary() is None


def test_command_lines(tmp_path, capsys):
    Image = pytest.importorskip('PIL.Image')
    for name, seed in (('real', 5), ('fake', 6)):
        (tmp_path / name).mkdir()
        px = ((_images(5, seed, 40) * 0.5 + 0.5) * 255).round().byte().permute(0, 2, 3, 1).numpy()
        for i in range(5):
            Image.fromarray(px[i]).save(str(tmp_path / name / ('%d.png' % i)))
    real_npy, fid_npy, stats = str(tmp_path / 'real.npy'), str(tmp_path / 'real_fid.npy'), str(tmp_path / 'real.npz')
    argv = ['--fake', str(tmp_path / 'fake'), '--batch_size', '2', '--kid_subsets', '3', '--seed', '1']
    a = FS.main(['--real', str(tmp_path / 'real'), '--save_real', real_npy] + argv)
    out = capsys.readouterr()
    assert 'WITHOUT pretrained weights' in out.err
    assert out.out.strip().splitlines()[-3:] == FS.format_lines(a)
    assert out.out.strip().splitlines()[-3].split()[0] == 'KID' and len(out.out.strip().splitlines()[-3].split()) == 3
    assert out.out.strip().splitlines()[-2].split()[0::2] == ['Precision', 'Recall']
    assert out.out.strip().splitlines()[-1].split()[0::2] == ['Density', 'Coverage']
    rows = np.load(real_npy)
    assert rows.dtype == np.float32 and rows.shape == (5, 2048) and a['real'] == a['fake'] == a['kid_subset_size'] == 5
    b = FS.main(['--real', real_npy] + argv)                                        # the saved real side: the same numbers
    assert a == b
    fake_npy = str(tmp_path / 'fake.npy')
    FS.main(['--real', real_npy, '--save_real', str(tmp_path / 'copy.npy')] + argv)
    assert np.array_equal(np.load(str(tmp_path / 'copy.npy')), rows)
    # python -m scene_generation_amd.fid --save_features writes the same rows, next to its statistics
    capsys.readouterr()
    FID.main(['--real', str(tmp_path / 'real'), '--fake', str(tmp_path / 'fake'), '--save_stats', stats, '--save_features', fid_npy,
              '--batch_size', '2'])
    assert np.array_equal(np.load(fid_npy), rows)
    # features on both sides: no network is built
    sets = FS.FeatureSetMetrics(real_features=real_npy, batch_size=2, device=DEV)
    FID._feed_dir(sets, str(tmp_path / 'fake'), 2)                                  # the chunks the command line feeds
    np.save(fake_npy, N(sets.fake.rows()))
    capsys.readouterr()
    c = FS.main(['--real', real_npy, '--fake', fake_npy, '--kid_subsets', '3', '--seed', '1'])
    assert 'WITHOUT pretrained weights' not in capsys.readouterr().err and c == a


def test_sample_cli_prints_the_three_lines(tmp_path, capsys):
    import random
    from trainer_helpers import _batch as ema_batch, _run, _trainer
    tr, ck, args = _trainer(tmp_path / 'train')
    _run(tr, ema_batch(), range(1))
    path = tr.save_checkpoint(ck, 1, args, 0)
    torch.manual_seed(3)
    weights, real_npy, stats = str(tmp_path / 'inception.pth'), str(tmp_path / 'real.npy'), str(tmp_path / 'real.npz')
    net = I.InceptionV3(num_classes=1008, aux_logits=False, fid_variant=True)
    torch.save(net.state_dict(), weights)
    rows = N(net.to(DEV).features(_images(7, 8).to(DEV)))
    np.save(real_npy, rows)
    np.savez(stats, mu=rows.astype(np.float64).mean(0), sigma=np.cov(rows.astype(np.float64), rowvar=False))
    base = ['--checkpoint', path, '--use_gt_boxes', '1', '--use_gt_masks', '1', '--use_gt_textures', '1', '--batch_size', '3',
            '--num_samples', '6', '--inception_weights', weights]
    capsys.readouterr()
    random.seed(0)
    res0 = sample.main(base + ['--output_dir', str(tmp_path / 'a')])
    out0 = capsys.readouterr()
    random.seed(0)
    res1 = sample.main(base + ['--output_dir', str(tmp_path / 'b'), '--real_features', real_npy])
    out1 = capsys.readouterr()
    random.seed(0)
    res2 = sample.main(base + ['--output_dir', str(tmp_path / 'c'), '--real_features', real_npy, '--fid_stats', stats])
    out2 = capsys.readouterr()
    assert 'featsets' not in res0 and 'KID' not in out0.out
    new = FS.format_lines(res1['featsets'])
    assert [l for l in out1.out.splitlines() if l not in new] == out0.out.splitlines() and out1.out.splitlines()[-3:] == new
    assert res1['featsets']['real'] == 7 and res1['featsets']['fake'] == 6 and res1['inception'] == res0['inception']
    assert res2['featsets'] == res1['featsets'] and np.isfinite(res2['fid']['fid']) and res2['inception'] == res0['inception']
    assert [l for l in out2.out.splitlines() if l.startswith(('KID ', 'Precision ', 'Density '))] == new
    with pytest.raises(ValueError, match='--real_features needs --inception_weights'):
        sample.main(['--checkpoint', path, '--output_dir', str(tmp_path / 'd'), '--real_features', real_npy])
