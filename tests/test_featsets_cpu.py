"""KID and precision / recall without a GPU: the argument errors of the three C entry points, the host estimators against the
restatement of tests/featsets_ref.py, the subset tables, the clamp and the row-count errors, the feature bank on a CPU device, the
command lines, and ``FrechetInceptionDistance(sets=None)`` being what it was."""
import ctypes

import numpy as np
import pytest
import torch

import featsets_ref as R
from scene_generation_amd import _hip, featsets, fid, ops, sample

NEW = ('sg_feat_poly_sums_ws_bytes', 'sg_feat_poly_sums', 'sg_feat_knn_radius_ws_bytes', 'sg_feat_knn_radius',
       'sg_feat_manifold_counts_ws_bytes', 'sg_feat_manifold_counts')


def test_prototypes_and_wrappers():
    for name in NEW:
        assert name in _hip.PROTOS and hasattr(_hip.lib(), name), name
    restype, argtypes, argnames = _hip.PROTOS['sg_feat_poly_sums']
    assert argnames == ['x', 'n', 'ldx', 'y', 'm', 'ldy', 'D', 'ix', 'iy', 'S', 's', 'gamma', 'coef0', 'degree', 'out', 'ws', 'ws_bytes',
                        'stream']
    assert argtypes[11] == argtypes[12] == ctypes.c_double and argtypes[14] == ctypes.POINTER(ctypes.c_double)
    assert all(_hip.PROTOS[n][0] == ctypes.c_size_t for n in NEW if n.endswith('_ws_bytes'))
    for name in ('feat_poly_sums', 'feat_knn_radius', 'feat_manifold_counts'):
        assert callable(getattr(ops, name))


def test_entry_points_reject_bad_arguments():
    """negative codes with the function's name, before anything touches a device; zero work returns 0 without a look at the pointers"""
    L = _hip.lib()
    buf = np.zeros(4096, np.float64)
    pd = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    odd = ctypes.cast(buf.ctypes.data + 4, ctypes.POINTER(ctypes.c_double))
    v, vodd, vhalf = buf.ctypes.data, buf.ctypes.data + 4, buf.ctypes.data + 2
    big = 1 << 15
    poly = L.sg_feat_poly_sums
    good = (v, 4, 4, v, 4, 4, 4, v, v, 1, 2, 1.0, 1.0, 3, pd, v, big, None)

    def swap(args, **kw):
        names = _hip.PROTOS[swap.fn][2]
        return tuple(kw.get(n, a) for n, a in zip(names, args))

    swap.fn = 'sg_feat_poly_sums'
    bad = [swap(good, x=None), swap(good, y=None), swap(good, ix=None), swap(good, iy=None), swap(good, out=None), swap(good, ws=None),
           swap(good, x=vhalf), swap(good, y=vhalf), swap(good, ix=vhalf), swap(good, iy=vhalf), swap(good, out=odd), swap(good, ws=vodd),
           swap(good, ldx=3), swap(good, ldy=3), swap(good, n=0), swap(good, m=0), swap(good, D=0), swap(good, s=0), swap(good, S=-1),
           swap(good, degree=0), swap(good, degree=5), swap(good, ws_bytes=8)]
    for args in bad:
        assert poly(*args) < 0 and 'sg_feat_poly_sums' in _hip.last_error(), args
    assert poly(*swap(good, S=0, x=None, y=None, ix=None, iy=None, out=None, ws=None, ws_bytes=0)) == 0
    assert 'degree' in (poly(*swap(good, degree=5)), _hip.last_error())[1]

    knn = L.sg_feat_knn_radius
    swap.fn = 'sg_feat_knn_radius'
    good = (v, 9, 4, 4, 3, pd, v, big, None)
    bad = [swap(good, x=None), swap(good, r2=None), swap(good, ws=None), swap(good, x=vhalf), swap(good, r2=odd), swap(good, ws=vodd),
           swap(good, ldx=3), swap(good, D=0), swap(good, n=-1), swap(good, k=0), swap(good, k=9), swap(good, n=3), swap(good, ws_bytes=8)]
    for args in bad:
        assert knn(*args) < 0 and 'sg_feat_knn_radius' in _hip.last_error(), args
    assert knn(*swap(good, n=0, x=None, r2=None, ws=None, ws_bytes=0)) == 0
    assert 'k=3' in (knn(*swap(good, n=3)), _hip.last_error())[1]                 # k needs k + 1 rows

    cnt = L.sg_feat_manifold_counts
    swap.fn = 'sg_feat_manifold_counts'
    good = (v, 5, 4, pd, v, 6, 4, 4, v, pd, v, big, None)
    bad = [swap(good, a=None), swap(good, r2=None), swap(good, b=None), swap(good, count=None), swap(good, mind2=None), swap(good, ws=None),
           swap(good, a=vhalf), swap(good, b=vhalf), swap(good, count=vhalf), swap(good, r2=odd), swap(good, mind2=odd), swap(good, ws=vodd),
           swap(good, lda=3), swap(good, ldb=3), swap(good, D=0), swap(good, n=-1), swap(good, m=-1), swap(good, ws_bytes=8)]
    for args in bad:
        assert cnt(*args) < 0 and 'sg_feat_manifold_counts' in _hip.last_error(), args
    for zero in (dict(n=0), dict(m=0)):
        assert cnt(*swap(good, a=None, r2=None, b=None, count=None, mind2=None, ws=None, ws_bytes=0, **zero)) == 0
    # the workspace queries: what the three calls split their work into
    assert L.sg_feat_poly_sums_ws_bytes(3, 65) == 3 * (2 * 3 + 4) * 8 and L.sg_feat_poly_sums_ws_bytes(0, 5) == 0
    assert L.sg_feat_knn_radius_ws_bytes(1000) >= (1000 + 16 * 4 * 8 * 1000) * 8 and L.sg_feat_knn_radius_ws_bytes(0) == 0
    assert L.sg_feat_manifold_counts_ws_bytes(5, 6) == 11 * 8


def test_wrappers_refuse_before_a_launch():
    x = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.feat_knn_radius(x, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.feat_poly_sums(x, x, np.zeros((1, 2), np.int32), np.zeros((1, 2), np.int32), 1.0, 1.0, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.feat_manifold_counts(x, torch.zeros(4, dtype=torch.float64), x)


def test_kid_from_sums_against_the_restatement():
    rs = np.random.RandomState(0)
    for S, s in ((1, 2), (5, 7), (100, 1000)):
        sums = rs.rand(S, 3) * s * s * 3.0
        got, want = featsets.kid_from_sums(sums, s), R.kid_from_sums(sums, s)
        assert all(isinstance(v, float) for v in got)
        assert abs(got[0] - want[0]) <= 4 * np.spacing(np.abs(sums).max() / s) and abs(got[1] - want[1]) <= 1e-12 * (1 + want[1])
    assert featsets.kid_from_sums(np.array([[6.0, 2.0, 9.0]]), 3) == (6.0 / 6 + 2.0 / 6 - 2.0, 0.0)
    # two identical sets, full size, from the float restatement of the sums: the estimate of a zero distance is below zero by the
    # diagonal's share, never the biased estimator's 0
    x = R.relu_gauss(1, 9, 16)
    idx = np.arange(9, dtype=np.int32)[None]
    sums, _ = R.poly_sums_float(x, x, idx, idx, 1.0 / 16, 1.0, 3)
    assert featsets.kid_from_sums(sums, 9)[0] < 0
    with pytest.raises(ValueError):
        featsets.kid_from_sums(np.zeros((1, 3)), 1)


def test_manifold_metrics_against_the_restatement():
    rs = np.random.RandomState(3)
    for n, m, k in ((5, 7, 1), (130, 97, 3), (40, 40, 8)):
        cf, cr, cov = rs.randint(0, 4, m), rs.randint(0, 3, n), rs.rand(n) < 0.5
        got, want = featsets.manifold_metrics(cf.astype(np.int32), cr.astype(np.int32), cov, k), R.prdc(cf, cr, cov, k)
        assert sorted(got) == ['coverage', 'density', 'precision', 'recall']
        assert all(isinstance(got[key], float) and abs(got[key] - want[key]) <= 1e-15 for key in got), (got, want)
    one = featsets.manifold_metrics(np.array([0, 2, 5, 0]), np.array([1, 0]), np.array([True, False]), 3)
    assert one == {'precision': 0.5, 'recall': 0.5, 'density': 7.0 / 12.0, 'coverage': 0.5}


def test_subset_tables():
    a = featsets.draw_subsets(5, 7, 30, 100, 40)
    b = featsets.draw_subsets(5, 7, 30, 100, 40)
    c = featsets.draw_subsets(6, 7, 30, 100, 40)
    want = R.draw_subsets(5, 7, 30, 100, 40)
    for t, w, hi in zip(a, want, (100, 40)):
        assert t.dtype == np.int32 and t.shape == (7, 30) and t.min() >= 0 and t.max() < hi and np.array_equal(t, w)
        assert all(len(set(row.tolist())) == 30 for row in t)                     # no repeats within a subset
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(a[0], c[0])
    full = featsets.draw_subsets(0, 1, 40, 40, 40)
    assert sorted(full[0][0].tolist()) == list(range(40))                         # one subset of the full size: every row once
    with pytest.raises(ValueError):
        featsets.draw_subsets(0, 3, 41, 100, 40)


def _bank_rows(rs, n, d=8):
    return torch.from_numpy(rs.randn(n, d).astype(np.float32))


def test_feature_bank_on_a_cpu_device(tmp_path):
    rs = np.random.RandomState(8)
    chunks = [_bank_rows(rs, n) for n in (3, 1, 6, 20)]
    bank = featsets.FeatureBank(8, 'cpu', capacity=4)
    for c in chunks:
        bank.update(c)
    assert bank.count == 30 and bank.buf.size(0) == 32 and tuple(bank.rows().shape) == (30, 8)      # 4 -> 8 -> 16 -> 32
    assert torch.equal(bank.rows(), torch.cat(chunks))
    a, b = featsets.FeatureBank(8, 'cpu', capacity=2), featsets.FeatureBank(8, 'cpu')
    a.update(chunks[0]), a.update(chunks[1]), b.update(chunks[2]), b.update(chunks[3])
    assert a.merge(b) is a and a.count == 30 and torch.equal(a.rows(), bank.rows()) and b.count == 26
    path = str(tmp_path / 'feats.npy')
    bank.save(path)
    raw = np.load(path)
    assert raw.dtype == np.float32 and raw.shape == (30, 8) and np.array_equal(raw, bank.rows().numpy())
    back = featsets.FeatureBank.load(path, 'cpu')
    assert back.dim == 8 and back.count == 30 and torch.equal(back.rows(), bank.rows())
    bank.clean()
    assert bank.count == 0 and tuple(bank.rows().shape) == (0, 8)
    with pytest.raises(ValueError):
        bank.update(torch.zeros(2, 9))
    with pytest.raises(TypeError):
        bank.update(torch.zeros(2, 8, dtype=torch.float64))
    with pytest.raises(ValueError):
        bank.merge(featsets.FeatureBank(9, 'cpu'))
    np.save(path, np.zeros(5, np.float32))
    with pytest.raises(ValueError):
        featsets.load_features(path)


def test_metrics_object_clamp_and_row_errors(tmp_path):
    rs = np.random.RandomState(9)
    m = featsets.FeatureSetMetrics(device='cpu', dim=8, k=3, kid_subset_size=1000)
    assert m.inception_model is None and m.needs_real and not m.real_fixed          # no network until images arrive
    with pytest.raises(ValueError, match='real side holds 0 rows'):
        m.compute()
    m.add_real_features(_bank_rows(rs, 12))
    m.add_features(_bank_rows(rs, 1))
    with pytest.raises(ValueError, match='fake side holds 1 rows.*at least 2'):
        m.compute()
    m.add_features(_bank_rows(rs, 2))
    with pytest.raises(ValueError, match=r'fake side holds 3 rows.*k \+ 1 = 4'):
        m.compute()
    m.add_features(_bank_rows(rs, 4))
    assert m.subset_size() == 7                                                     # clamped to the smaller side
    m.kid_subset_size = 5
    assert m.subset_size() == 5
    m.clean()
    assert m.fake.count == 0 and m.real.count == 12 and m.needs_real
    m.clean_real()
    assert m.real.count == 0
    for bad in (dict(k=0), dict(k=9), dict(kid_subsets=0), dict(kid_subset_size=1)):
        with pytest.raises(ValueError):
            featsets.FeatureSetMetrics(device='cpu', dim=8, **bad)
    # a fixed real side: from an array or a file; it takes no more rows
    rows = rs.randn(6, 8).astype(np.float32)
    path = str(tmp_path / 'real.npy')
    np.save(path, rows)
    for src in (rows, path, torch.from_numpy(rows)):
        f = featsets.FeatureSetMetrics(device='cpu', dim=8, real_features=src)
        assert f.real_fixed and not f.needs_real and f.real.count == 6 and np.array_equal(f.real.rows().numpy(), rows)
        with pytest.raises(RuntimeError):
            f.add_real_features(_bank_rows(rs, 2))
        with pytest.raises(RuntimeError):
            f.clean_real()
    with pytest.raises(ValueError):
        featsets.FeatureSetMetrics(device='cpu', dim=9, real_features=rows)


def test_cli_parsers():
    a = featsets.build_parser().parse_args(['--weights', 'w.pth', '--real', 'r.npy', '--fake', 'dir'])
    assert (a.weights, a.real, a.fake, a.save_real, a.k, a.kid_subsets, a.kid_subset_size, a.seed) == ('w.pth', 'r.npy', 'dir', None, 3, 100,
                                                                                                    1000, 0)
    b = featsets.build_parser().parse_args(['--real', 'a', '--fake', 'b', '--save_real', 'o.npy', '--k', '5', '--kid_subsets', '7',
                                            '--kid_subset_size', '50', '--seed', '4'])
    assert (b.save_real, b.k, b.kid_subsets, b.kid_subset_size, b.seed) == ('o.npy', 5, 7, 50, 4)
    with pytest.raises(SystemExit):
        featsets.build_parser().parse_args(['--real', 'x'])
    assert fid.build_parser().parse_args(['--real', 'a', '--fake', 'b']).save_features is None
    assert fid.build_parser().parse_args(['--real', 'a', '--fake', 'b', '--save_features', 'f.npy']).save_features == 'f.npy'
    with pytest.raises(SystemExit, match='--save_features needs'):
        fid.main(['--real', 'stats.npz', '--fake', 'b', '--save_features', 'f.npy'])
    assert sample.make_parser().parse_args(['--checkpoint', 'c']).real_features is None
    assert sample.make_parser().parse_args(['--checkpoint', 'c', '--real_features', 'r.npy']).real_features == 'r.npy'
    lines = featsets.format_lines({'kid_mean': 0.5, 'kid_std': 0.25, 'precision': 1.0, 'recall': 0.0, 'density': 2.0, 'coverage': 0.75})
    assert lines == ['KID 0.5 0.25', 'Precision 1.0 Recall 0.0', 'Density 2.0 Coverage 0.75']


def test_sample_real_features_needs_inception_weights(tmp_path):
    args = sample.make_parser().parse_args(['--checkpoint', 'none', '--real_features', 'r.npy'])
    with pytest.raises(ValueError, match='--real_features needs --inception_weights'):
        sample.run_model(args, None, str(tmp_path / 'out'))
    assert not (tmp_path / 'out').exists()                                          # refused before any work


class _Net(torch.nn.Module):
    """stands in for an InceptionV3 where only ``fc.in_features`` is read"""

    def __init__(self, dim=8):
        super().__init__()
        self.fc = torch.nn.Linear(dim, 2)


def test_fid_without_sets_is_what_it_was():
    stats = (np.zeros(8), np.eye(8))
    f = fid.FrechetInceptionDistance(weights=_Net(), real_stats=stats, device='cpu')
    assert f.sets is None
    assert sorted(vars(f)) == sorted(['resize', 'batch_size', 'device', 'inception_model', 'fake', 'real', '_real_stats', '_real_open',
                                      '_root', 'sets'])
    assert f.real is None and not f.needs_real and f.fake.count == 0 and f.resize is True and f.batch_size == 32
    g = fid.FrechetInceptionDistance(weights=_Net(), device='cpu')
    assert g.sets is None and g.needs_real and g.real.count == 0 and g._root is None and g._real_stats is None
    import inspect
    sig = inspect.signature(fid.FrechetInceptionDistance.__init__)
    assert list(sig.parameters)[1:] == ['weights', 'real_stats', 'resize', 'batch_size', 'device', 'sets'] and sig.parameters['sets'].default is None


def test_fid_with_sets_attachment_rules():
    rows = np.random.RandomState(1).randn(6, 8).astype(np.float32)
    stats = (np.zeros(8), np.eye(8))
    open_sets = featsets.FeatureSetMetrics(device='cpu', dim=8)
    fixed_sets = featsets.FeatureSetMetrics(device='cpu', dim=8, real_features=rows)
    with pytest.raises(ValueError, match='needs real_features='):
        fid.FrechetInceptionDistance(weights=_Net(), real_stats=stats, device='cpu', sets=open_sets)
    with pytest.raises(ValueError, match='real_features'):
        fid.FrechetInceptionDistance(weights=_Net(), device='cpu', sets=fixed_sets)
    with pytest.raises(ValueError, match='dimensions'):
        fid.FrechetInceptionDistance(weights=_Net(), device='cpu', sets=featsets.FeatureSetMetrics(device='cpu', dim=9))
    f = fid.FrechetInceptionDistance(weights=_Net(), real_stats=stats, device='cpu', sets=fixed_sets)
    assert f.sets is fixed_sets
    g = fid.FrechetInceptionDistance(weights=_Net(), device='cpu', sets=open_sets)
    open_sets.add_features(torch.zeros(3, 8))
    open_sets.add_real_features(torch.zeros(2, 8))
    g.fake.count = 3                                   # (the moments themselves need the device: only the bookkeeping is checked here)
    g.clean()
    assert open_sets.fake.count == 0 and open_sets.real.count == 2
    g.clean_real()
    assert open_sets.real.count == 0 and open_sets.needs_real
