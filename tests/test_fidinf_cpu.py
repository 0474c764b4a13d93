"""FID-infinity without a GPU: the host logic (sizes, subset tables, the line), the Gram form of the Frechet distance against the D x D
form of tests/fidinf_ref.py, the estimator's bias against a closed-form truth, the tap protocol on a CPU device, the argument errors of
the two C entry points and the command-line parsers."""
import ctypes

import numpy as np
import pytest
import torch

import fidinf_ref as R
from fidinf_ref import REL, _Net
from scene_generation_amd import _hip, featsets, fid, fidinf, ops, sample

NEW = ('sg_fidinf_grams_ws_bytes', 'sg_fidinf_grams', 'sg_fidinf_subset_terms_ws_bytes', 'sg_fidinf_subset_terms')


# ---- host logic -----------------------------------------------------------------------------------------------------------------------
def test_draw_sizes():
    s = fidinf.draw_sizes(400)
    assert np.array_equal(s, R.sizes_of(400)) and s[0] == 200 and s[-1] == 400 and len(s) == 15 and np.all(np.diff(s) > 0)
    assert np.array_equal(fidinf.draw_sizes(1000, 15, 100), R.sizes_of(1000, 15, 100))
    few = fidinf.draw_sizes(10, 15)                 # 5 .. 10 in 15 steps: duplicates go
    assert few.tolist() == [5, 6, 7, 8, 9, 10]
    assert fidinf.draw_sizes(5, 2, 2).tolist() == [2, 5]
    for bad in ((3, 15, 1), (2, 15, None), (10, 15, 10), (10, 1, 5), (10, 15, 11)):      # min_size < 2 (twice), one size, one point, min > n
        with pytest.raises(ValueError):
            fidinf.draw_sizes(*bad)


def test_draw_subsets():
    sizes = fidinf.draw_sizes(40, 6)
    a, sa = fidinf.draw_subsets(3, sizes, 40)
    b, _ = fidinf.draw_subsets(3, sizes, 40)
    c, _ = fidinf.draw_subsets(4, sizes, 40)
    assert a.dtype == np.int32 and sa.dtype == np.int32 and a.shape == (len(sizes), 40) and np.array_equal(sa, sizes)
    assert np.array_equal(a, b) and not np.array_equal(a, c) and np.array_equal(a, R.tables(3, sizes, 40))
    for q, s in enumerate(sizes):
        row = a[q, :s]
        assert len(set(row.tolist())) == s and row.min() >= 0 and row.max() < 40 and not a[q, s:].any()      # no repeats; zero padding
    assert np.array_equal(a[-1], np.arange(40))                                     # the full subset: the identity order
    assert not np.array_equal(a[0, :sizes[0]], np.arange(sizes[0]))
    for bad in ([1, 5], [5, 41], []):
        with pytest.raises(ValueError):
            fidinf.draw_subsets(0, bad, 40)


def test_extrapolate_returns_an_exact_line():
    sizes = np.array([200, 250, 300, 400])
    c, m = fidinf.extrapolate(sizes, 3.25 + 480.0 / sizes)
    assert abs(c - 3.25) <= 1e-13 and abs(m - 480.0) <= 1e-10
    c, m = fidinf.extrapolate([2, 4], [5.0, 4.0])
    assert abs(c - 3.0) <= 1e-14 and abs(m - 4.0) <= 1e-14
    want = R.line(sizes, [7.0, 6.5, 6.1, 5.9])
    got = fidinf.extrapolate(sizes, [7.0, 6.5, 6.1, 5.9])
    assert abs(got[0] - want[0]) <= 1e-12 and abs(got[1] - want[1]) <= 1e-9
    for bad in (([5], [1.0]), ([5, 5], [1.0, 2.0]), ([5, 6], [1.0])):
        with pytest.raises(ValueError):
            fidinf.extrapolate(*bad)


# ---- the Gram form against the D x D form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,N,n_real', [(64, 400, 4000), (256, 200, 1000)])
def test_gram_form_equals_the_dxd_form(D, N, n_real):
    c = R.case(D, N, n_real)
    sizes = R.sizes_of(N)
    assert len(sizes) == 15
    idx = R.tables(0, sizes, N)
    want = R.subset_fids_dxd(c['fake'], c['mu'], c['sigma'], idx, sizes)
    _, P, G = R.grams(c['fake'], c['mu'], c['sigma'])
    sums, Ms = R.subset_terms(P, G, idx, sizes)
    tr = float(np.trace(c['sigma']))
    got = np.array([fidinf.fid_from_terms(sums[q], Ms[q], int(s), tr) for q, s in enumerate(sizes)])
    ref_pair = np.abs(R.subset_fids_gram(c['fake'], c['mu'], c['sigma'], idx, sizes) - want) / np.abs(want)
    rel = np.abs(got - want) / np.abs(want)
    print('D=%d N=%d: fid_from_terms against the D x D form %.3g relative; the two reference forms %.3g; bound %.3g'
          % (D, N, rel.max(), ref_pair.max(), REL))
    assert isinstance(fidinf.fid_from_terms(sums[0], Ms[0], int(sizes[0]), tr), float)
    assert (rel <= REL).all()
    with pytest.raises(ValueError):
        fidinf.fid_from_terms(sums[0], Ms[1], int(sizes[0]), tr)


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_extrapolation_beats_the_full_set_value(seed):
    """a property of the estimator: against the closed-form distance of the fake POPULATION to the sample real statistics, the
    intercept is more than 4 x closer than the FID of all N rows (the reference alone: ratios 0.008 .. 0.14 on these inputs)"""
    c = R.case(64, 400, 4000, seed)
    sizes = fidinf.draw_sizes(400, 15, 400 // 2)
    idx, sizes = fidinf.draw_subsets(seed, sizes, 400)
    _, P, G = R.grams(c['fake'], c['mu'], c['sigma'])
    sums, Ms = R.subset_terms(P, G, idx, sizes)
    tr = float(np.trace(c['sigma']))
    fids = [fidinf.fid_from_terms(sums[q], Ms[q], int(s), tr) for q, s in enumerate(sizes)]
    fid_inf, slope = fidinf.extrapolate(sizes, fids)
    err_inf, err_n = abs(fid_inf - c['truth']), abs(fids[-1] - c['truth'])
    print('seed %d: truth %.4f FID_N %.4f FID_inf %.4f ratio %.4f' % (seed, c['truth'], fids[-1], fid_inf, err_inf / err_n))
    assert slope > 0 and err_inf < err_n / 4


# ---- the tap protocol -----------------------------------------------------------------------------------------------------------------
class _Log(object):
    """a ``then`` that records every call"""

    def __init__(self, dim=8, real_fixed=False):
        self.dim, self.real_fixed, self.calls = dim, real_fixed, []

    def add_features(self, f):
        self.calls.append(('add_features', tuple(f.shape)))

    def add_real_features(self, f):
        self.calls.append(('add_real_features', tuple(f.shape)))

    def clean(self):
        self.calls.append(('clean',))

    def clean_real(self):
        self.calls.append(('clean_real',))


def test_tap_protocol_on_a_cpu_device(tmp_path):
    stats = (np.zeros(8), np.eye(8))
    fixed, opened = fidinf.FIDInfinity(real_stats=stats, dim=8, device='cpu'), fidinf.FIDInfinity(dim=8, device='cpu')
    assert fixed.real_fixed and not fixed.needs_real and fixed.real is None and fixed.dim == 8
    assert not opened.real_fixed and opened.needs_real and opened.real.count == 0
    path = str(tmp_path / 'stats.npz')
    np.savez(path, mu=stats[0], sigma=stats[1])
    assert fidinf.FIDInfinity(real_stats=path, dim=8, device='cpu').real_fixed
    with pytest.raises(ValueError, match='dimensions'):
        fidinf.FIDInfinity(real_stats=stats, dim=9, device='cpu')
    # the attachment rule of FrechetInceptionDistance, as it stands: fixed goes with real_stats, open with add_real
    assert fid.FrechetInceptionDistance(weights=_Net(), real_stats=stats, device='cpu', sets=fixed).sets is fixed
    g = fid.FrechetInceptionDistance(weights=_Net(), device='cpu', sets=opened)
    assert g.sets is opened
    with pytest.raises(ValueError, match='needs real_features='):
        fid.FrechetInceptionDistance(weights=_Net(), real_stats=stats, device='cpu', sets=opened)
    with pytest.raises(ValueError, match='real_features'):
        fid.FrechetInceptionDistance(weights=_Net(), device='cpu', sets=fixed)
    with pytest.raises(ValueError, match='dimensions'):
        fid.FrechetInceptionDistance(weights=_Net(), device='cpu', sets=fidinf.FIDInfinity(dim=9, device='cpu'))
    # then: dimensions and the state of the real side must match; every call is forwarded
    with pytest.raises(ValueError, match='dimensions'):
        fidinf.FIDInfinity(dim=8, device='cpu', then=_Log(9))
    with pytest.raises(ValueError, match='fix both'):
        fidinf.FIDInfinity(dim=8, device='cpu', then=_Log(8, real_fixed=True))
    with pytest.raises(ValueError, match='fix both'):
        fidinf.FIDInfinity(real_stats=stats, dim=8, device='cpu', then=_Log(8))
    log = _Log()
    t = fidinf.FIDInfinity(dim=8, device='cpu', then=log)
    t.add_features(torch.zeros(3, 8))
    t.real.update = lambda f: setattr(t.real, 'count', t.real.count + f.size(0))     # (the moments need the device: bookkeeping only)
    t.add_real_features(torch.zeros(2, 8))
    assert t.fake.count == 3 and t.real.count == 2
    t.clean()
    assert t.fake.count == 0 and t.real.count == 2
    t.add_features(torch.ones(4, 8))
    t.clean_real()
    assert t.real.count == 0 and t.fake.count == 4 and t.needs_real
    assert log.calls == [('add_features', (3, 8)), ('add_real_features', (2, 8)), ('clean',), ('add_features', (4, 8)), ('clean_real',)]
    # a real FeatureSetMetrics behind a fixed real side, driven through FrechetInceptionDistance's own clean
    rows = np.random.RandomState(1).randn(6, 8).astype(np.float32)
    sets = featsets.FeatureSetMetrics(device='cpu', dim=8, real_features=rows)
    both = fidinf.FIDInfinity(real_stats=stats, dim=8, device='cpu', then=sets)
    f = fid.FrechetInceptionDistance(weights=_Net(), real_stats=stats, device='cpu', sets=both)
    both.add_features(torch.zeros(5, 8))
    assert both.fake.count == 5 and sets.fake.count == 5
    f.clean()
    assert both.fake.count == 0 and sets.fake.count == 0 and sets.real.count == 6
    for call in (lambda: both.add_real_features(torch.zeros(2, 8)), both.clean_real):
        with pytest.raises(RuntimeError, match='fixed by real_stats'):
            call()
    with pytest.raises(ValueError, match='fake side holds 0 rows'):
        both.compute()
    with pytest.raises(ValueError, match='real side holds 0 rows'):
        (lambda o: (o.add_features(torch.zeros(3, 8)), o.compute()))(fidinf.FIDInfinity(dim=8, device='cpu'))


def test_sampler_sees_a_sets_object_behind_the_tap():
    stats = (np.zeros(8), np.eye(8))
    sets = featsets.FeatureSetMetrics(device='cpu', dim=8, real_features=np.zeros((3, 8), np.float32))
    tap = fidinf.FIDInfinity(real_stats=stats, dim=8, device='cpu', then=sets)
    f = fid.FrechetInceptionDistance(weights=_Net(), real_stats=stats, device='cpu', sets=tap)
    probe = sample.Sampler.__new__(sample.Sampler)
    probe.fid, probe.inception, probe.sets = f, None, sets
    assert probe._sets_shared()                      # fed by the forward of fid through the tap: not a second time
    probe.fid = fid.FrechetInceptionDistance(weights=_Net(), real_stats=stats, device='cpu', sets=sets)
    assert probe._sets_shared()
    probe.fid = fid.FrechetInceptionDistance(weights=_Net(), real_stats=stats, device='cpu')
    assert not probe._sets_shared()
    probe.fid, probe.inception = None, type('S', (), {'fid': tap})()
    assert probe._sets_shared()


def test_too_many_rows_name_plain_fid():
    with pytest.raises(ValueError, match='max_rows = 4.*FrechetInceptionDistance'):
        fidinf.fid_infinity(torch.zeros(5, 8), np.zeros(8), np.eye(8), max_rows=4)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_wrappers():
    for name in NEW:
        assert name in _hip.PROTOS and hasattr(_hip.lib(), name), name
    pd = ctypes.POINTER(ctypes.c_double)
    restype, argtypes, argnames = _hip.PROTOS['sg_fidinf_grams']
    assert argnames == ['x', 'n', 'D', 'ldx', 'mu', 'sigma', 'P', 'G', 'ws', 'ws_bytes', 'stream'] and argtypes[4:8] == [pd] * 4
    restype, argtypes, argnames = _hip.PROTOS['sg_fidinf_subset_terms']
    assert argnames == ['P', 'G', 'n', 'idx', 'sizes', 'S', 'smax', 'M', 'sums', 'ws', 'ws_bytes', 'stream']
    assert argtypes[:2] == [pd] * 2 and argtypes[7:9] == [pd] * 2
    assert all(_hip.PROTOS[n][0] == ctypes.c_size_t for n in NEW if n.endswith('_ws_bytes'))
    assert callable(ops.fidinf_grams) and callable(ops.fidinf_subset_terms)


def test_entry_points_reject_bad_arguments():
    """negative codes that name the function, before anything touches a device (the library loads without one)"""
    L = _hip.lib()
    buf = np.zeros(1 << 15, np.float64)
    pd = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    odd = ctypes.cast(buf.ctypes.data + 4, ctypes.POINTER(ctypes.c_double))
    v, vodd, vhalf = buf.ctypes.data, buf.ctypes.data + 4, buf.ctypes.data + 2
    big = 1 << 15

    def swap(fn, args, **kw):
        return tuple(kw.get(n, a) for n, a in zip(_hip.PROTOS[fn][2], args))

    grams = L.sg_fidinf_grams
    good = (v, 5, 4, 4, pd, pd, pd, pd, v, big, None)
    bad = [dict(x=None), dict(mu=None), dict(sigma=None), dict(P=None), dict(G=None), dict(ws=None), dict(x=vhalf), dict(mu=odd),
           dict(sigma=odd), dict(P=odd), dict(G=odd), dict(ws=vodd), dict(D=0), dict(n=1), dict(n=0), dict(n=-3), dict(ldx=3),
           dict(ws_bytes=16 * 5 * 4 - 1), dict(ws_bytes=0)]
    for kw in bad:
        assert grams(*swap('sg_fidinf_grams', good, **kw)) < 0 and 'sg_fidinf_grams' in _hip.last_error(), kw
    assert 'n >= 2' in (grams(*swap('sg_fidinf_grams', good, n=1)), _hip.last_error())[1]
    assert L.sg_fidinf_grams_ws_bytes(1000, 2048) == 16 * 1000 * 2048 and L.sg_fidinf_grams_ws_bytes(0, 5) == 0
    assert L.sg_fidinf_grams_ws_bytes(4096, 1 << 20) == 16 * 4096 * (1 << 20)          # beyond 2^32: size_t arithmetic

    terms = L.sg_fidinf_subset_terms
    good = (pd, pd, 9, v, v, 3, 5, pd, pd, v, big, None)
    bad = [dict(P=None), dict(G=None), dict(idx=None), dict(sizes=None), dict(M=None), dict(sums=None), dict(ws=None), dict(P=odd),
           dict(G=odd), dict(M=odd), dict(sums=odd), dict(ws=vodd), dict(idx=vhalf), dict(sizes=vhalf), dict(n=1), dict(S=-1),
           dict(smax=1), dict(smax=0), dict(ws_bytes=8 * (3 * 3 * 5 + 3) - 1)]
    for kw in bad:
        assert terms(*swap('sg_fidinf_subset_terms', good, **kw)) < 0 and 'sg_fidinf_subset_terms' in _hip.last_error(), kw
    assert terms(*swap('sg_fidinf_subset_terms', good, S=0, P=None, G=None, idx=None, sizes=None, M=None, sums=None, ws=None,
                       ws_bytes=0)) == 0
    assert L.sg_fidinf_subset_terms_ws_bytes(3, 5) == 8 * (3 * 3 * 5 + 3) and L.sg_fidinf_subset_terms_ws_bytes(0, 5) == 0


def test_wrappers_refuse_before_a_launch():
    x = torch.zeros(4, 8)
    calls = ops.CALLS[0]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.fidinf_grams(x, torch.zeros(8, dtype=torch.float64), torch.zeros(8, 8, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.fidinf_subset_terms(torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64), np.zeros((1, 2), np.int32),
                                np.array([2], np.int32))
    assert ops.CALLS[0] == calls


# ---- parsers ----------------------------------------------------------------------------------------------------------------------------
def test_cli_parsers():
    a = fidinf.build_parser().parse_args(['--weights', 'w.pth', '--real', 'r.npz', '--fake', 'dir'])
    assert (a.weights, a.real, a.fake, a.num_points, a.min_size, a.seed, a.image_size) == ('w.pth', 'r.npz', 'dir', 15, None, 0, None)
    b = fidinf.build_parser().parse_args(['--real', 'a', '--fake', 'b.npy', '--num_points', '7', '--min_size', '50', '--seed', '4',
                                          '--image_size', '64,64'])
    assert (b.num_points, b.min_size, b.seed, b.image_size) == (7, 50, 4, (64, 64))
    with pytest.raises(SystemExit):
        fidinf.build_parser().parse_args(['--real', 'x'])
    assert fidinf.format_lines({'fid_inf': 1.5, 'fid': 2.25, 'images': 7}) == ['FID_inf 1.5', 'FID_N 2.25 N 7']
    assert sample.make_parser().parse_args(['--checkpoint', 'c']).fid_infinity is False
    assert sample.make_parser().parse_args(['--checkpoint', 'c', '--fid_infinity', '1']).fid_infinity is True


def test_sample_fid_infinity_needs_fid_stats(tmp_path):
    args = sample.make_parser().parse_args(['--checkpoint', 'none', '--fid_infinity', '1', '--inception_weights', 'w.pth'])
    with pytest.raises(ValueError, match='--fid_infinity needs --fid_stats'):
        sample.run_model(args, None, str(tmp_path / 'out'))
    assert not (tmp_path / 'out').exists()          # refused before any work


@pytest.mark.parametrize('count,match', [(3, 'draw_sizes'), (4097, 'max_rows = 4096')])
def test_sample_fid_infinity_refuses_an_impossible_count_at_once(tmp_path, count, match):
    """the synthetic generator makes exactly --num_samples pictures: a count FID-infinity cannot take is refused before the first one"""
    args = sample.make_parser().parse_args(['--checkpoint', 'none', '--fid_infinity', '1', '--inception_weights', 'w.pth', '--fid_stats',
                                            's.npz', '--num_samples', str(count)])
    with pytest.raises(ValueError, match=match):
        sample.run_model(args, None, str(tmp_path / 'out'))
    assert not (tmp_path / 'out').exists()
    fidinf.check_count(4)
    fidinf.check_count(4096)
    with pytest.raises(ValueError):
        fidinf.check_count(4097)
    with pytest.raises(ValueError):
        fidinf.check_count(10, max_rows=9)
