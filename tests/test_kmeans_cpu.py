"""Host side of the appearance bank (no GPU): tests/kmeans_ref.py pinned to scikit-learn's Lloyd, the deterministic ordering of the
centres, the bank files and the two command lines."""
import os

import numpy as np
import pytest

import kmeans_ref as KR
from scene_generation_amd import bank, sample


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_ref_lloyd_matches_sklearn(seed):
    """same explicit init, tol = 0, algorithm = 'lloyd': centres agree to 1e-12, with and without empty-cluster events"""
    cluster = pytest.importorskip('sklearn.cluster')
    K, D = 10, 32
    rs = np.random.RandomState(seed)
    x, off = KR.segmented(rs, KR.class_sizes(rs, K), K, D)
    events = 0
    for c in range(len(off) - 1):
        xc = x[off[c]:off[c + 1]]
        if not len(xc):
            assert KR.lloyd(xc, xc[:0])['n_iter'] == 0
            continue
        k = min(len(xc), K)
        init = xc[:k].copy()
        got = KR.lloyd(xc, init, tol=0.0)
        events += got['events']
        km = cluster.KMeans(n_clusters=k, init=init, n_init=1, algorithm='lloyd', tol=0, max_iter=300).fit(xc)
        assert np.abs(got['centers'] - km.cluster_centers_).max() <= 1e-12, (seed, c)
        assert got['counts'].sum() == len(xc) and (got['counts'] > 0).all()
        assert abs(got['inertia'] - km.inertia_) <= 1e-9 * max(1.0, km.inertia_)
    assert (events > 0) == (seed in (0, 1, 3)), 'seeds 0, 1 and 3 are the ones with empty-cluster events'


def test_ref_relocate_rule():
    lab = np.array([0, 0, 0, 1, 0])
    m = np.array([1.0, 5.0, 5.0, 9.0, 2.0])
    # centre 2 is empty: row 3 is alone in centre 1 (not a candidate); rows 1 and 2 tie: the lower row goes
    assert KR.relocate(lab, m, 3).tolist() == [0, 2, 0, 1, 0]
    # two empty centres, ascending: the farthest row first
    assert KR.relocate(np.zeros(5, dtype=np.int64), m, 3).tolist() == [0, 2, 0, 1, 0]


def test_ref_pp_round():
    rs = np.random.RandomState(5)
    x = rs.randn(50, 4)
    first, _ = KR.pp_round(x, None, 0.5)
    assert first == 25
    pick, m = KR.pp_round(x, None, 0.3, prev=first, first=True)
    cum = np.cumsum(m)
    assert m[first] == 0 and pick != first and cum[pick] > 0.3 * cum[-1] and (pick == 0 or cum[pick - 1] <= 0.3 * cum[-1])


def test_order_centers_pc1():
    rs = np.random.RandomState(3)
    c = rs.randn(17, 32)
    got, order = bank.order_centers(c, 'pc1', return_order=True)
    assert sorted(order.tolist()) == list(range(17)) and np.array_equal(got, c[order])
    perm = rs.permutation(17)
    assert np.array_equal(bank.order_centers(c[perm]), got), 'invariant to a permutation of the input rows'
    assert np.array_equal(bank.order_centers(-c), -got[::-1]), '-centers: the same order reversed'
    assert np.array_equal(bank.order_centers(c, 'none'), c)
    assert bank.order_centers(c[:1]).shape == (1, 32) and bank.order_centers(c[:0]).shape == (0, 32)
    assert bank.order_centers(c.astype(np.float32)).dtype == np.float64
    with pytest.raises(ValueError):
        bank.order_centers(c, 'umap')


def _toy_bank():
    rs = np.random.RandomState(11)
    feats = {0: rs.rand(150, 8), 1: rs.rand(4, 8), 2: np.zeros((0, 8)), 3: rs.rand(1, 8)}
    b = {'features': feats}
    for k in (100, 10, 1):
        b[k] = {c: v[:min(len(v), k)].astype(np.float32) for c, v in feats.items() if len(v)}
    return b


def test_save_bank_round_trip(tmp_path):
    b = _toy_bank()
    paths = bank.save_bank(b, str(tmp_path / 'out'))
    assert sorted(os.path.basename(p) for p in paths) == ['features.npy', 'features_clustered_001.npy', 'features_clustered_010.npy',
                                                          'features_clustered_100.npy']
    for key, name in [('features', 'features.npy'), (100, 'features_clustered_100.npy'), (10, 'features_clustered_010.npy'),
                      (1, 'features_clustered_001.npy')]:
        d = np.load(str(tmp_path / 'out' / name), allow_pickle=True).item()
        assert isinstance(d, dict) and all(type(c) is int for c in d)
        assert all(v.dtype == np.float64 and v.ndim == 2 and v.shape[1] == 8 for v in d.values())
        assert sorted(d) == ([0, 1, 2, 3] if key == 'features' else [0, 1, 3])
        for c, v in d.items():
            assert np.array_equal(v, np.asarray(b[key][c], dtype=np.float64))
            if key != 'features':
                assert v.shape[0] == min(b['features'][c].shape[0], key), 'a class with fewer rows than K gets k_c = n_c rows'
    assert d[0].shape == (1, 8)


def test_sample_load_features_reads_the_001_file(tmp_path):
    b = _toy_bank()
    bank.save_bank(b, str(tmp_path))
    args = sample.make_parser().parse_args(['--checkpoint', str(tmp_path / 'ckpt.pt')])
    got = sample.load_features(args)
    assert sorted(got) == [0, 1, 3] and all(v.shape == (1, 8) for v in got.values())
    assert np.array_equal(got[1], np.asarray(b[1][1], dtype=np.float64))
    many, one = sample.load_bank(str(tmp_path))
    assert many[0].shape == (100, 8) and one[0].shape == (1, 8)
    with pytest.raises(ValueError, match='No features file'):
        sample.load_bank(str(tmp_path / 'nowhere'))


def test_parsers():
    a = bank.make_parser().parse_args(['--checkpoint', 'x.pt'])
    assert (a.weights, a.output_dir, a.n_clusters, a.seed, a.n_init, a.order, a.model_mode) == \
        ('model', None, (100, 10, 1), 0, 1, 'pc1', 'eval')
    assert a.num_samples > 0 and a.batch_size > 0
    b = bank.make_parser().parse_args(['--checkpoint', 'x.pt', '--n_clusters', '50,5', '--weights', 'ema_best', '--order', 'tsne',
                                       '--n_init', '3', '--seed', '7', '--output_dir', 'o'])
    assert (b.n_clusters, b.weights, b.order, b.n_init, b.seed, b.output_dir) == ((50, 5), 'ema_best', 'tsne', 3, 7, 'o')
    s = sample.make_parser().parse_args(['--checkpoint', 'x.pt'])
    assert s.bank is None and s.features is None
    assert sample.make_parser().parse_args(['--checkpoint', 'x.pt', '--bank', 'd']).bank == 'd'
    assert bank.bank_file(100) == 'features_clustered_100.npy' and bank.bank_file(10) == 'features_clustered_010.npy'
    assert bank.bank_file(1) == 'features_clustered_001.npy' and bank.bank_file('features') == 'features.npy'


def test_draw_uniforms_is_the_seeded_table():
    u = bank.draw_uniforms(4, 2, 3, 5)
    assert u.shape == (2, 3, 5) and u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(u, bank.draw_uniforms(4, 2, 3, 5)) and not np.array_equal(u, bank.draw_uniforms(5, 2, 3, 5))
    assert np.array_equal(u[0], bank.draw_uniforms(4, 1, 3, 5)[0]), 'restart 0 of n_init = 2 is the run with n_init = 1'
