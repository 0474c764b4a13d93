"""FID-infinity on the GPU (csrc/fidinf.hip, ops/fidinf.py, scene_generation_amd/fidinf.py).

* ``sg_fidinf_grams`` against the float64 restatement of tests/fidinf_ref.py within the DERIVED summation bounds
  |P - P_ref| <= 2 gamma_{D+2} |Z||Z|^T and |G - G_ref| <= 2 gamma_{2D+4} |Z||Sigma||Z|^T, entry by entry, between guard words; exact
  symmetry; bit-identical repeats; a padded row stride and a base one float into its allocation.
* ``sg_fidinf_subset_terms`` on ragged subsets (2, 3, 16, 17 and 37 of 37 rows) within the bound derived the same way, exact symmetry
  of every block, and poison outside the blocks untouched.
* End to end against the restatement's Gram-form pipeline and against the existing D x D route (``FeatureMoments`` +
  ``frechet_distance``) at the margin measured for the two reference forms (tests/test_fidinf_cpu.py).
* The shared forward, the command line and ``sample --fid_infinity 1``.
The worst share of each bound goes to fidinf_margins.json in the suite's output directory (profiles/fidinf_test_margins.md).
The tree only: no reference checkout."""
import numpy as np
import pytest
import torch

import fidinf_ref as R
from fidinf_ref import REL, _Net
from gpu_harness import METRIC_GUARD, Margins, N, _guarded, _guards_ok, _place, margins_fixture
from sampling_helpers import _images
from scene_generation_amd import featsets as FS
from scene_generation_amd import fid as FID
from scene_generation_amd import fidinf as FI
from scene_generation_amd import inception as I
from scene_generation_amd import ops, sample

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = METRIC_GUARD
MARGINS = Margins()
_write_margins = margins_fixture(lambda: MARGINS.dump('fidinf_margins.json', 'share_of_bound', empty=False))


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _inputs(n, D):
    """pooled-like rows, and the mean (near 0.4) and numpy.cov of OTHER such rows"""
    x = R.pooled_like(1000 * n + D, n, D)
    mu, sigma = R.stats(R.pooled_like(7 + D, max(2 * D, 16), D))
    return x, mu, sigma


def grams(x, mu, sigma, extra=0, off=0):
    n = x.shape[0]
    pbuf, P = _guarded((n, n))
    gbuf, G = _guarded((n, n))
    got = ops.fidinf_grams(_place(x, extra, off), _dev64(mu), _dev64(sigma), P=P, G=G)
    assert got[0] is P and got[1] is G and _guards_ok(pbuf) and _guards_ok(gbuf)
    return P, G


# =====================================================================================================================================
# 1. the Gram matrices
# =====================================================================================================================================
GRAM_CASES = [(2, 1, 0, 0), (17, 70, 0, 0), (37, 64, 0, 0), (65, 256, 3, 1), (130, 2048, 0, 0)]


@pytest.mark.parametrize('n,D,extra,off', GRAM_CASES, ids=lambda v: str(v))
def test_grams_within_the_derived_bound(n, D, extra, off):
    x, mu, sigma = _inputs(n, D)
    assert 0.2 < mu.mean() < 0.7 and (x >= 0).all()
    Z, Pr, Gr = R.grams(x, mu, sigma)
    bP, bG = R.gram_bounds(Z, sigma)
    P, G = grams(x, mu, sigma, extra, off)
    P, G = N(P), N(G)
    assert np.isfinite(P).all() and np.isfinite(G).all() and not (P == GUARD).any() and not (G == GUARD).any()
    sp, sg = float((np.abs(P - Pr) / bP).max()), float((np.abs(G - Gr) / bG).max())
    print('grams n=%d D=%d: worst share of the bound P %.4f G %.4f' % (n, D, sp, sg))
    MARGINS.note('grams_P', sp, '%d_%d' % (n, D))
    MARGINS.note('grams_G', sg, '%d_%d' % (n, D))
    assert (np.abs(P - Pr) <= bP).all() and (np.abs(G - Gr) <= bG).all()
    assert np.array_equal(P, P.T) and np.array_equal(G, G.T)                        # bit for bit
    P2, G2 = grams(x, mu, sigma, extra, off)
    assert np.array_equal(N(P2), P) and np.array_equal(N(G2), G)                    # the same call, the same bits


def test_grams_take_sigma_as_given():
    """Y = Z sigma, not Z sigma^T: an unsymmetric sigma tells them apart (and a wrong operand orientation in the tile)"""
    x, mu, sigma = _inputs(37, 70)
    sigma = sigma + np.triu(np.random.RandomState(3).randn(70, 70), 1) * 0.05
    Z, Pr, Gr = R.grams(x, mu, sigma)
    _, bG = R.gram_bounds(Z, sigma)
    _, G = grams(x, mu, sigma)
    assert (np.abs((Z @ sigma.T) @ Z.T - Gr) > 4 * bG).any()                         # the test can tell
    upper = np.triu(np.ones((37, 37), bool))                                        # the entries i <= j are the computed ones
    assert (np.abs(N(G) - Gr) <= bG)[upper].all()


def test_grams_wrapper_refuses():
    x = torch.zeros(5, 8, device=DEV)
    mu, sigma = torch.zeros(8, dtype=torch.float64, device=DEV), torch.zeros(8, 8, dtype=torch.float64, device=DEV)
    calls = ops.CALLS[0]
    for bad in (lambda: ops.fidinf_grams(x[:1], mu, sigma), lambda: ops.fidinf_grams(x, mu[:7], sigma),
                lambda: ops.fidinf_grams(x, mu, sigma.float()), lambda: ops.fidinf_grams(x, mu.cpu(), sigma),
                lambda: ops.fidinf_grams(x, mu, sigma.t()),          # not contiguous
                lambda: ops.fidinf_grams(x, mu, sigma, P=torch.zeros(5, 4, dtype=torch.float64, device=DEV))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.fidinf_grams(x.double(), mu, sigma)
    assert ops.CALLS[0] == calls                    # nothing was launched


# =====================================================================================================================================
# 2. the subset terms
# =====================================================================================================================================
def test_subset_terms_on_ragged_subsets():
    n, sizes = 37, np.array([2, 3, 16, 17, 37], np.int32)
    x, mu, sigma = _inputs(n, 64)
    P, G = grams(x, mu, sigma)
    rs = np.random.RandomState(11)
    idx = np.zeros((5, 37), np.int32)
    for q, s in enumerate(sizes):
        idx[q, :s] = rs.permutation(n)[:s]
    idx[0, :2] = (n - 1, 0)                         # the last row and the first
    Ph, Gh = N(P), N(G)
    want_sums, want_M = R.subset_terms(Ph, Gh, idx, sizes)          # on the device's own P and G: the terms alone are under test
    zero = np.zeros_like(Ph)
    bsums, bM = R.subset_terms_bounds(Ph, Gh, zero, zero, idx, sizes)
    mbuf, M = _guarded((5, 37, 37))
    M.fill_(GUARD)                                  # poison everywhere: what lies outside a block must stay
    sbuf, sums = _guarded((5, 2))
    got = ops.fidinf_subset_terms(P, G, idx, sizes, M=M, sums=sums)
    assert got[0] is M and got[1] is sums and _guards_ok(mbuf) and _guards_ok(sbuf)
    Mh, sh = N(M), N(sums)
    share = float((np.abs(sh - want_sums) / bsums).max())
    print('subset sums: worst share of the bound %.4f' % share)
    MARGINS.note('subset_sums', share, '37')
    assert (np.abs(sh - want_sums) <= bsums).all()
    for q, s in enumerate(sizes):
        block = Mh[q, :s, :s]
        mshare = float((np.abs(block - want_M[q]) / bM[q]).max())
        print('M block of %d rows: worst share of the bound %.4f' % (s, mshare))
        MARGINS.note('subset_M', mshare, str(int(s)))
        assert (np.abs(block - want_M[q]) <= bM[q]).all()
        assert np.array_equal(block, block.T)                                       # bit for bit
        outside = np.ones((37, 37), bool)
        outside[:s, :s] = False
        assert (Mh[q][outside] == GUARD).all() and not (block == GUARD).any()
    M2, sums2 = ops.fidinf_subset_terms(P, G, idx, sizes)
    for q, s in enumerate(sizes):
        assert np.array_equal(N(M2)[q, :s, :s], Mh[q, :s, :s])
    assert np.array_equal(N(sums2), sh)


def test_subset_terms_wrapper_refuses():
    P = torch.zeros(6, 6, dtype=torch.float64, device=DEV)
    good, sz = np.zeros((2, 4), np.int32), np.array([2, 4], np.int32)
    calls = ops.CALLS[0]
    bad = [lambda: ops.fidinf_subset_terms(P, P, np.array([[0, 6, 0, 0], [0, 0, 0, 0]], np.int32), sz),       # an index outside the set
           lambda: ops.fidinf_subset_terms(P, P, np.array([[0, -1, 0, 0], [0, 0, 0, 0]], np.int32), sz),
           lambda: ops.fidinf_subset_terms(P, P, good, np.array([1, 4], np.int32)),                            # sizes outside 2 .. smax
           lambda: ops.fidinf_subset_terms(P, P, good, np.array([2, 5], np.int32)),
           lambda: ops.fidinf_subset_terms(P, P, good, np.array([2], np.int32)),
           lambda: ops.fidinf_subset_terms(P, P, torch.zeros(2, 4, dtype=torch.int32, device=DEV), sz),        # device tables cannot be checked
           lambda: ops.fidinf_subset_terms(P, P.float(), good, sz),
           lambda: ops.fidinf_subset_terms(P[:, :5], P, good, sz)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert ops.CALLS[0] == calls                    # nothing was launched


# =====================================================================================================================================
# 3. end to end
# =====================================================================================================================================
@pytest.fixture(scope='module')
def case64():
    c = R.case(64, 400, 4000)
    c['want'] = R.pipeline_gram(c['fake'], c['mu'], c['sigma'])
    return c


def test_fid_infinity_against_the_restatement_and_the_dxd_route(case64):
    c, want = case64, case64['want']
    rows = torch.from_numpy(c['fake']).to(DEV)
    res = FI.fid_infinity(rows, c['mu'], c['sigma'])
    assert sorted(res) == ['fid', 'fid_inf', 'fids', 'images', 'sizes', 'slope']
    assert res['sizes'] == want['sizes'].tolist() and res['images'] == 400 and len(res['fids']) == 15 and res['fid'] == res['fids'][-1]
    rel = np.abs(np.array(res['fids']) - want['fids']) / np.abs(want['fids'])
    rel_inf = abs(res['fid_inf'] - want['fid_inf']) / abs(want['fid_inf'])
    print('fid_infinity D=64 N=400: subset FIDs %.3g relative, FID_inf %.3g relative (%.6f against %.6f); bound %.3g'
          % (rel.max(), rel_inf, res['fid_inf'], want['fid_inf'], REL))
    # the cross-check between the new route and the existing one: the moments of the same rows, then the D x D distance
    mom = FID.FeatureMoments(64, DEV)
    mom.update(rows)
    mu2, sigma2 = mom.statistics()
    dxd = FID.frechet_distance(c['mu'], c['sigma'], mu2, sigma2)
    rel_dxd = abs(res['fid'] - dxd) / abs(dxd)
    print('FID_N: the Gram route %.12f, FeatureMoments + frechet_distance %.12f, %.3g relative' % (res['fid'], dxd, rel_dxd))
    MARGINS.note('fid_infinity_fids', float(rel.max() / REL), '64_400')
    MARGINS.note('fid_infinity_intercept', float(rel_inf / REL), '64_400')
    MARGINS.note('fid_n_against_dxd', float(rel_dxd / REL), '64_400')
    assert (rel <= REL).all() and rel_inf <= REL and rel_dxd <= REL
    assert FI.fid_infinity(rows, c['mu'], c['sigma']) == res                        # the same bits
    other = FI.fid_infinity(rows, c['mu'], c['sigma'], seed=1)
    assert other['fid'] == res['fid'] and other['fids'][0] != res['fids'][0]        # the full set is the identity; the draws differ
    few = FI.fid_infinity(rows, c['mu'], c['sigma'], num_points=4, min_size=100)
    assert few['sizes'] == [100, 200, 300, 400] and few['fid'] == res['fid']
    with pytest.raises(ValueError, match='max_rows'):
        FI.fid_infinity(rows, c['mu'], c['sigma'], max_rows=399)


def test_subsets_are_chunked_under_the_memory_limit(case64, monkeypatch):
    rows = torch.from_numpy(case64['fake']).to(DEV)
    whole = FI.fid_infinity(rows, case64['mu'], case64['sigma'])
    calls = []
    real = ops.fidinf_subset_terms
    monkeypatch.setattr(FI, 'M_BYTES_MAX', 3 * 400 * 400 * 8)
    monkeypatch.setattr(ops, 'fidinf_subset_terms', lambda P, G, idx, sizes: (calls.append(idx.shape), real(P, G, idx, sizes))[1])
    assert FI.fid_infinity(rows, case64['mu'], case64['sigma']) == whole
    assert len(calls) > 3 and all(S * s * s * 8 <= 3 * 400 * 400 * 8 for S, s in calls) and sum(S for S, _ in calls) == 15


def test_shared_forward_fixed_and_open_real_side(case64):
    c = case64
    rows = torch.from_numpy(c['fake']).to(DEV)
    stats = (c['mu'], c['sigma'])
    want = FI.fid_infinity(rows, *stats)
    tap = FI.FIDInfinity(real_stats=stats, dim=64, device=DEV)
    f = FID.FrechetInceptionDistance(weights=_Net(64), real_stats=stats, device=DEV, sets=tap)
    for lo, hi in ((0, 130), (130, 131), (131, 400)):
        f.add_features(rows[lo:hi])
    assert tap.fake.count == f.fake.count == 400 and torch.equal(tap.fake.rows(), rows)
    assert f.sets.compute() == want and not tap.needs_real
    assert abs(f.compute() - want['fid']) <= REL * want['fid']                      # the distance itself, by its own route
    f.clean()
    assert tap.fake.count == 0
    # an open real side: the statistics are the object's own moments of the real rows
    real = torch.from_numpy(R.draw(5, R.population(10, 64), 300)).to(DEV)
    tap2 = FI.FIDInfinity(dim=64, device=DEV)
    g = FID.FrechetInceptionDistance(weights=_Net(64), device=DEV, sets=tap2)
    for lo, hi in ((0, 7), (7, 300)):
        g.real.update(real[lo:hi])                  # (what add_real does with the features of a batch of images)
        g.sets.add_real_features(real[lo:hi])
    for lo, hi in ((0, 1), (1, 399), (399, 400)):
        g.add_features(rows[lo:hi])
    mom = FID.FeatureMoments(64, DEV)
    for lo, hi in ((0, 7), (7, 300)):               # (the same calls: the moments round once per call)
        mom.update(real[lo:hi])
    assert tap2.needs_real
    got = g.sets.compute()
    assert got == FI.fid_infinity(rows, *mom.statistics()) and not tap2.needs_real
    assert abs(g.compute() - got['fid']) <= REL * got['fid']
    g.clean_real()
    assert tap2.real.count == 0 and tap2.needs_real and tap2.fake.count == 400
    with pytest.raises(ValueError, match='real side holds 0 rows'):
        tap2.compute()
    # then: KID and precision / recall behind the tap, one feed
    sets = FS.FeatureSetMetrics(real_features=N(real), kid_subsets=2, device=DEV, dim=64)
    both = FI.FIDInfinity(real_stats=stats, dim=64, device=DEV, then=sets)
    h = FID.FrechetInceptionDistance(weights=_Net(64), real_stats=stats, device=DEV, sets=both)
    h.add_features(rows)
    lone = FS.FeatureSetMetrics(real_features=N(real), kid_subsets=2, device=DEV, dim=64)
    lone.add_features(rows)
    assert both.compute() == want and sets.compute() == lone.compute()


# =====================================================================================================================================
# 4. the command lines
# =====================================================================================================================================
def test_command_line(tmp_path, capsys):
    Image = pytest.importorskip('PIL.Image')
    for name, seed, n in (('real', 5, 8), ('fake', 6, 6)):
        (tmp_path / name).mkdir()
        px = ((_images(n, seed, 40) * 0.5 + 0.5) * 255).round().byte().permute(0, 2, 3, 1).numpy()
        for i in range(n):
            Image.fromarray(px[i]).save(str(tmp_path / name / ('%d.png' % i)))
    stats, fake_npy = str(tmp_path / 'real.npz'), str(tmp_path / 'fake.npy')
    capsys.readouterr()
    plain = FID.main(['--real', str(tmp_path / 'real'), '--fake', str(tmp_path / 'fake'), '--save_stats', stats, '--batch_size', '2'])
    capsys.readouterr()
    a = FI.main(['--real', str(tmp_path / 'real'), '--fake', str(tmp_path / 'fake'), '--batch_size', '2'])
    out = capsys.readouterr()
    assert 'WITHOUT pretrained weights' in out.err
    assert out.out.strip().splitlines()[-2:] == FI.format_lines(a) == ['FID_inf {}'.format(a['fid_inf']), 'FID_N {} N 6'.format(a['fid'])]
    assert a['sizes'] == [3, 4, 5, 6] and a['images'] == 6 and np.isfinite(a['fid_inf'])
    # the full-set value is the FID command's number.  (Plumbing only: with 6 and 8 rows of 2048 dimensions either route may keep one
    # eigenvalue of rounding noise, ~2^-52 of the largest, whose square root is ~1.5e-8 of its; the tight comparison is the end-to-end test)
    assert abs(a['fid'] - plain) <= 1e-6 * abs(plain)
    b = FI.main(['--real', stats, '--fake', str(tmp_path / 'fake'), '--batch_size', '2'])      # the saved statistics: the same numbers
    assert b == a
    # features on the fake side, statistics on the real one: no network is built
    bank = FS.FeatureSetMetrics(real_features=np.zeros((1, 2048), np.float32), batch_size=2, device=DEV)
    FID._feed_dir(bank, str(tmp_path / 'fake'), 2)
    np.save(fake_npy, N(bank.fake.rows()))
    capsys.readouterr()
    c = FI.main(['--real', stats, '--fake', fake_npy, '--seed', '0'])
    assert 'WITHOUT pretrained weights' not in capsys.readouterr().err and c == a
    d = FI.main(['--real', stats, '--fake', fake_npy, '--num_points', '2', '--min_size', '4'])
    assert d['sizes'] == [4, 6] and d['fid'] == a['fid']


def test_sample_cli_prints_the_line_after_fid(tmp_path, capsys):
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
            '--num_samples', '6', '--inception_weights', weights, '--fid_stats', stats]
    runs = []
    for k, extra in enumerate(([], ['--fid_infinity', '1'], ['--fid_infinity', '1', '--real_features', real_npy])):
        capsys.readouterr()
        random.seed(0)
        res = sample.main(base + ['--output_dir', str(tmp_path / ('out%d' % k))] + extra)
        runs.append((res, capsys.readouterr().out.splitlines()))
    (res0, out0), (res1, out1), (res2, out2) = runs
    assert 'fid_inf' not in res0 and not any(l.startswith('FID_inf') for l in out0)              # 0 is the default
    at = [i for i, l in enumerate(out1) if l.startswith('FID ')]
    assert len(at) == 1 and out1[at[0] + 1] == 'FID_inf {}'.format(res1['fid_inf']['fid_inf'])      # directly after the FID line
    assert out1[:at[0] + 1] + out1[at[0] + 2:] == out0                              # and nothing else changed
    assert res1['fid'] == res0['fid'] and res1['inception'] == res0['inception']
    inf = res1['fid_inf']
    assert inf['images'] == 6 and inf['sizes'] == [3, 4, 5, 6] and np.isfinite(inf['fid_inf'])
    assert abs(inf['fid'] - res1['fid']['fid']) <= 1e-6 * abs(inf['fid'])            # (plumbing: see test_command_line)
    # with --real_features the FeatureSetMetrics hangs behind the tap: fed once, by the same forward
    assert res2['fid_inf'] == inf and res2['featsets']['fake'] == 6 and res2['featsets']['real'] == 7
    new = FS.format_lines(res2['featsets'])
    assert [l for l in out2 if l not in new] == out1 and out2[-3:] == new
    with pytest.raises(ValueError, match='--fid_infinity needs --fid_stats'):
        sample.main(['--checkpoint', path, '--output_dir', str(tmp_path / 'd'), '--inception_weights', weights, '--fid_infinity', '1'])
    assert not (tmp_path / 'd').exists()
