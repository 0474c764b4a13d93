"""IS-infinity without a GPU: the float64 restatement of tests/isinf_ref.py against the direct form of the score, the host's share of
scene_generation_amd/isinf.py (subset tables, repeats, the two lines) driven by the restatement's subset scores, the property that
justifies the feature (the intercepts lie closer to the large-sample score than the plain score does), the argument errors of the
two C entry points and the parsers."""
import ctypes

import numpy as np
import pytest
import torch

import isinf_ref as R
from scene_generation_amd import _hip, inception, isinf, ops, sample
from scene_generation_amd.fidinf import draw_sizes, draw_subsets, extrapolate

NEW = ('sg_isinf_row_terms', 'sg_isinf_subset_scores_ws_bytes', 'sg_isinf_subset_scores')
RPW = _hip.CONST['SG_ISINF_ROWS_PER_WG']


def host_is_infinity(p, **knobs):
    """``isinf.is_infinity`` with the device's two calls replaced by the restatement"""
    idx, tsizes, point, sizes = isinf.draw_tables(p.shape[0], **knobs)
    out, _ = R.subset_scores(p, idx, tsizes)
    return isinf.from_scores(sizes, point, out, p.shape[0])


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def test_the_host_share_is_fidinfs_own():
    assert isinf.draw_sizes is draw_sizes and isinf.draw_subsets is draw_subsets and isinf.extrapolate is extrapolate


def test_extrapolate_recovers_an_exact_line():
    sizes = np.array([512, 600, 777, 1024])
    c, m = isinf.extrapolate(sizes, 44.0 - 2200.0 / sizes)
    assert abs(c - 44.0) <= 1e-12 and abs(m + 2200.0) <= 1e-8
    want = R.line(sizes, [40.0, 41.0, 41.5, 42.5])
    got = isinf.extrapolate(sizes, [40.0, 41.0, 41.5, 42.5])
    assert abs(got[0] - want[0]) <= 1e-11 and abs(got[1] - want[1]) <= 1e-8


def test_reference_at_all_rows_is_the_direct_score():
    """exp(mean KL) the way scripts/inception_score.py computes one split, against H / n - T: the same number in float64"""
    for seed, n, C in ((0, 300, 1000), (1, 64, 10), (2, 129, 1008)):
        p = R.rows(seed, n, C, 0.02 if C >= 1000 else 0.5)
        p[3] *= 0.5                                  # a row whose sum is not 1: both forms normalise it
        p[5, ::2] = 0.0                              # exact zeros
        out, parts = R.subset_scores(p, np.arange(n, dtype=np.int32)[None], [n])
        want = R.direct_score(p)
        bound = R.score_bound(want, *parts[0], C)
        print('n=%d C=%d: H / n - T form %.15g, direct form %.15g, %.3g of the bound' % (n, C, out[0, 1], want, abs(out[0, 1] - want) / bound))
        assert abs(out[0, 1] - want) <= bound and abs(out[0, 0] - np.log(want)) <= R.log_score_bound(*parts[0], C) + 4 * R.U


def test_identical_rows_score_one_at_every_size():
    p = np.tile(R.rows(4, 1, 50, 0.5), (40, 1))
    res = host_is_infinity(p, num_points=6)
    assert res['sizes'] == draw_sizes(40, 6).tolist() and len(res['scores']) == len(res['sizes'])
    assert np.allclose(res['scores'], 1.0, rtol=0, atol=1e-13)
    assert abs(res['is_inf'] - 1.0) <= 1e-12 and abs(res['is_inf_log'] - 1.0) <= 1e-12 and abs(res['is'] - 1.0) <= 1e-13


def test_one_class_gives_exactly_one():
    p = np.random.RandomState(0).rand(12, 1).astype(np.float32) + 0.5
    res = host_is_infinity(p, num_points=4)
    assert res['scores'] == [1.0] * len(res['sizes']) and res['is'] == 1.0 and res['is_inf'] == 1.0 and res['is_inf_log'] == 1.0
    assert res['slope'] == 0.0 and res['images'] == 12


def test_a_zero_row_contributes_nothing_but_counts():
    p = R.rows(5, 9, 10, 0.5)
    p[4] = 0.0
    out, parts = R.subset_scores(p, np.arange(9, dtype=np.int32)[None], [9])
    s, h = R.row_terms(p)
    assert s[4] == 0.0 and h[4] == 0.0 and parts[0][2] == 9
    rest = np.delete(p, 4, 0).astype(np.float64)
    rest_h = np.delete(h, 4).sum()
    ph = rest / rest.sum(1, keepdims=True)
    want = rest_h / 9 - ((ph.sum(0) / 9) * np.log(rest.sum(0) / rest.sum())).sum()      # the other rows' sums over all NINE
    assert abs(out[0, 0] - want) <= 1e-14 and np.isfinite(out).all()


# ---- repeats and the tables -------------------------------------------------------------------------------------------------------------
def test_draw_tables_repeats_and_the_full_set_once():
    n = 40
    sizes = draw_sizes(n, 6)
    idx, tsizes, point, got_sizes = isinf.draw_tables(n, 6, seed=3)
    want_idx, want_sizes = draw_subsets(3, sizes, n)
    assert np.array_equal(got_sizes, sizes) and np.array_equal(idx, want_idx) and np.array_equal(tsizes, want_sizes)
    assert idx.dtype == np.int32 and tsizes.dtype == np.int32 and point.tolist() == list(range(len(sizes)))
    idx3, tsizes3, point3, _ = isinf.draw_tables(n, 6, seed=3, repeats=3)
    P = len(sizes)
    assert idx3.shape == (3 * (P - 1) + 1, n) and tsizes3.shape == (3 * (P - 1) + 1,)
    assert np.array_equal(idx3[:P], idx) and np.array_equal(tsizes3[:P], tsizes)            # the first draw is the single draw
    assert np.bincount(point3).tolist() == [3] * (P - 1) + [1]                              # the full set once
    assert (tsizes3 == n).sum() == 1 and np.array_equal(idx3[P - 1], np.arange(n))
    assert np.array_equal(tsizes3, sizes[point3])
    for k in range(P - 1):                           # three different draws of each size, each without repeats and in range
        rows_k = [tuple(idx3[s, :tsizes3[s]]) for s in np.flatnonzero(point3 == k)]
        assert len(set(rows_k)) == 3 and all(len(set(r)) == len(r) and min(r) >= 0 and max(r) < n for r in rows_k)
    assert np.array_equal(isinf.draw_tables(n, 6, seed=3, repeats=3)[0], idx3)
    assert not np.array_equal(isinf.draw_tables(n, 6, seed=4, repeats=3)[0], idx3)
    with pytest.raises(ValueError, match='repeats'):
        isinf.draw_tables(n, 6, repeats=0)
    # every size equal to n cannot happen (draw_sizes needs two); min_size == n - 1 leaves one size below n
    assert np.bincount(isinf.draw_tables(5, 2, 4, repeats=2)[2]).tolist() == [2, 1]


def test_from_scores_averages_the_repeats_before_the_fit():
    sizes = np.array([4, 6, 8])
    point = np.array([0, 1, 2, 0, 1])
    out = np.array([[np.log(2.0), 2.0], [np.log(3.0), 3.0], [np.log(5.0), 5.0], [np.log(4.0), 4.0], [np.log(3.5), 3.5]])
    res = isinf.from_scores(sizes, point, out, 8)
    assert res['scores'] == [3.0, 3.25, 5.0] and res['is'] == 5.0 and res['images'] == 8 and res['sizes'] == [4, 6, 8]
    c, m = extrapolate(sizes, [3.0, 3.25, 5.0])
    assert res['is_inf'] == c and res['slope'] == m
    logs = [(np.log(2.0) + np.log(4.0)) / 2, (np.log(3.0) + np.log(3.5)) / 2, np.log(5.0)]
    assert abs(res['is_inf_log'] - np.exp(extrapolate(sizes, logs)[0])) <= 1e-14
    assert sorted(res) == ['images', 'is', 'is_inf', 'is_inf_log', 'scores', 'sizes', 'slope']
    with pytest.raises(ValueError, match='results'):
        isinf.from_scores(sizes, point, out[:4], 8)


@pytest.mark.parametrize('repeats', [1, 3])
def test_host_pipeline_equals_the_restated_one(repeats):
    p = R.rows(7, 60, 100, 0.1)
    got = host_is_infinity(p, num_points=5, seed=2, repeats=repeats)
    want = R.pipeline(p, 5, None, 2, repeats)
    assert got['sizes'] == want['sizes'].tolist()
    assert np.allclose(got['scores'], want['scores'], rtol=1e-13, atol=0)
    for k in ('is', 'is_inf', 'is_inf_log', 'slope'):
        assert abs(got[k] - want[k]) <= 1e-10 * abs(want[k]), k
    if repeats == 3:
        assert got['is'] == host_is_infinity(p, num_points=5, seed=2)['is']                  # the full set: computed once, not averaged


# ---- the property that justifies the feature --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def truth():
    """the score of 61 440 rows of the generator, chunk by chunk"""
    return R.large_sample_score(15 * 4096, 1000)


@pytest.mark.parametrize('seed', range(8))
def test_intercepts_beat_the_plain_score(truth, seed):
    """C = 1000, n = 1024: the plain score lies 3.5 % .. 6.3 % below the large-sample score, both intercepts within 2.4 % of it (the
    restatement alone, on this generator and these seeds)"""
    p = R.rows(seed, 1024, 1000)
    res = host_is_infinity(p)
    e_n, e_inf, e_log = abs(res['is'] / truth - 1), abs(res['is_inf'] / truth - 1), abs(res['is_inf_log'] / truth - 1)
    print('seed %d: truth %.4f IS_N %.4f (%.2f %%) IS_inf %.4f (%.2f %%) IS_inf_log %.4f (%.2f %%)'
          % (seed, truth, res['is'], 100 * e_n, res['is_inf'], 100 * e_inf, res['is_inf_log'], 100 * e_log))
    assert len(res['sizes']) == 15 and res['sizes'][0] == 512 and res['sizes'][-1] == 1024 and res['slope'] < 0
    assert e_inf < e_n and e_log < e_n


# ---- argument errors --------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    for bad in (3, 2, 0):
        with pytest.raises(ValueError, match='draw_sizes'):
            isinf.check_count(bad)
    isinf.check_count(4)
    isinf.check_count(50000)                         # no row cap
    with pytest.raises(ValueError, match='draw_sizes'):
        isinf.check_count(100, min_size=101)
    with pytest.raises(ValueError, match='softmax rows'):
        isinf.is_infinity(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match='softmax rows'):
        isinf.is_infinity(torch.zeros(4))
    with pytest.raises(ValueError, match='draw_sizes'):
        isinf.is_infinity(torch.zeros(3, 5))         # too few rows: refused on the host, before a launch
    with pytest.raises(TypeError, match='InceptionScore'):
        isinf.ISInfinity(object())
    assert isinf.format_lines({'is_inf': 1.5, 'is': 1.25, 'images': 7}) == ['IS_inf 1.5', 'IS_N 1.25 N 7']


def test_wrappers_refuse_before_a_launch():
    calls = ops.CALLS[0]
    p = torch.zeros(4, 8)
    d = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.isinf_row_terms(p)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.isinf_subset_scores(p, d, d, np.zeros((1, 2), np.int32), np.array([2], np.int32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        isinf.is_infinity(torch.full((8, 4), 0.25))
    assert ops.CALLS[0] == calls and ops.ISINF_ROWS_PER_WG == RPW


def test_isinfinity_reads_the_scorers_rows(monkeypatch):
    seen = []
    monkeypatch.setattr(isinf, 'is_infinity', lambda rows, *knobs: (seen.append((rows, knobs)), {'is_inf': 2.0})[1])
    scorer = type('S', (), {'rows': lambda self: 'the rows'})()
    assert isinf.ISInfinity(scorer, num_points=7, min_size=5, seed=3, repeats=2).compute() == {'is_inf': 2.0}
    assert seen == [('the rows', (7, 5, 3, 2))]
    # InceptionScore.rows(): the view probs[:count], empty before the first batch
    s = inception.InceptionScore.__new__(inception.InceptionScore)
    torch.nn.Module.__init__(s)
    s.classes, s.device, s.probs, s.count = 6, torch.device('cpu'), None, 0
    assert tuple(s.rows().shape) == (0, 6) and s.rows().dtype == torch.float32
    s.probs, s.count = torch.arange(24, dtype=torch.float32).view(4, 6), 3
    assert torch.equal(s.rows(), s.probs[:3]) and s.rows().data_ptr() == s.probs.data_ptr()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_prototypes_constants_and_kinds():
    for name in NEW:
        assert name in _hip.PROTOS and hasattr(_hip.lib(), name), name
    pd = ctypes.POINTER(ctypes.c_double)
    restype, argtypes, argnames = _hip.PROTOS['sg_isinf_row_terms']
    assert argnames == ['probs', 'n', 'classes', 'ldp', 'rs', 'h', 'stream'] and argtypes[4:6] == [pd] * 2
    restype, argtypes, argnames = _hip.PROTOS['sg_isinf_subset_scores']
    assert argnames == ['probs', 'n', 'classes', 'ldp', 'rs', 'h', 'idx', 'sizes', 'S', 'smax', 'out', 'ws', 'ws_bytes', 'stream']
    assert argtypes[4:6] == [pd] * 2 and argtypes[10] == pd
    assert _hip.PROTOS['sg_isinf_subset_scores_ws_bytes'][0] == ctypes.c_size_t
    assert _hip.PROTOS['sg_isinf_subset_scores_ws_bytes'][2] == ['S', 'smax', 'classes']
    assert RPW >= 1 and callable(ops.isinf_row_terms) and callable(ops.isinf_subset_scores)
    lib = _hip.lib()
    kinds = [lib.sg_prof_kind_name(i).decode() for i in range(lib.sg_prof_num_kinds())]
    assert 'isinf_row_terms' in kinds and 'isinf_subset_scores' in kinds


def test_entry_points_reject_bad_arguments():
    """negative codes that name the function, before anything touches a device (the library loads without one)"""
    L = _hip.lib()
    buf = np.zeros(1 << 15, np.float64)
    pd = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    odd = ctypes.cast(buf.ctypes.data + 4, ctypes.POINTER(ctypes.c_double))
    v, vodd, vhalf = buf.ctypes.data, buf.ctypes.data + 4, buf.ctypes.data + 2
    big = 1 << 18

    def swap(fn, args, **kw):
        return tuple(kw.get(n, a) for n, a in zip(_hip.PROTOS[fn][2], args))

    terms = L.sg_isinf_row_terms
    good = (v, 5, 4, 4, pd, pd, None)
    bad = [dict(probs=None), dict(rs=None), dict(h=None), dict(probs=vhalf), dict(rs=odd), dict(h=odd), dict(n=0), dict(n=-2),
           dict(classes=0), dict(ldp=3)]
    for kw in bad:
        assert terms(*swap('sg_isinf_row_terms', good, **kw)) < 0 and 'sg_isinf_row_terms' in _hip.last_error(), kw

    need = L.sg_isinf_subset_scores_ws_bytes
    slots = lambda S, smax, C: 8 * S * ((smax + RPW - 1) // RPW + 1) * (2 * C + 1)
    assert need(3, 5, 4) == slots(3, 5, 4) and need(15, 1000, 1000) == slots(15, 1000, 1000)
    assert need(1, RPW, 7) == slots(1, RPW, 7) and need(1, RPW + 1, 7) == slots(1, RPW + 1, 7)
    assert need(0, 5, 4) == 0 and need(3, 0, 4) == 0 and need(3, 5, 0) == 0
    assert need(15, 50000, 1008) == slots(15, 50000, 1008)
    assert need(1 << 20, 1 << 20, 1008) == slots(1 << 20, 1 << 20, 1008)             # beyond 2^32: size_t arithmetic

    scores = L.sg_isinf_subset_scores
    good = (v, 9, 4, 4, pd, pd, v, v, 3, 5, pd, v, big, None)
    bad = [dict(probs=None), dict(rs=None), dict(h=None), dict(idx=None), dict(sizes=None), dict(out=None), dict(ws=None),
           dict(probs=vhalf), dict(rs=odd), dict(h=odd), dict(out=odd), dict(ws=vodd), dict(idx=vhalf), dict(sizes=vhalf), dict(n=0),
           dict(classes=0), dict(ldp=3), dict(S=-1), dict(smax=1), dict(smax=0), dict(ws_bytes=slots(3, 5, 4) - 1), dict(ws_bytes=0)]
    for kw in bad:
        assert scores(*swap('sg_isinf_subset_scores', good, **kw)) < 0 and 'sg_isinf_subset_scores' in _hip.last_error(), kw
    assert 'workspace' in (scores(*swap('sg_isinf_subset_scores', good, ws_bytes=8)), _hip.last_error())[1]
    assert scores(*swap('sg_isinf_subset_scores', good, S=0, probs=None, rs=None, h=None, idx=None, sizes=None, out=None, ws=None,
                        ws_bytes=0)) == 0


# ---- parsers ----------------------------------------------------------------------------------------------------------------------------
def test_cli_parsers():
    a = isinf.build_parser().parse_args(['--weights', 'w.pth', '--dir', 'd'])
    assert (a.weights, a.dir, a.probs, a.num_points, a.min_size, a.seed, a.repeats, a.image_size) == ('w.pth', 'd', None, 15, None, 0, 1, None)
    b = isinf.build_parser().parse_args(['--probs', 'p.npy', '--num_points', '7', '--min_size', '50', '--seed', '4', '--repeats', '3',
                                         '--image_size', '64,64', '--resize_filter', 'bicubic'])
    assert (b.probs, b.dir, b.num_points, b.min_size, b.seed, b.repeats, b.image_size, b.resize_filter) == ('p.npy', None, 7, 50, 4, 3, (64, 64),
                                                                                                          'bicubic')
    for bad in ([], ['--dir', 'd', '--probs', 'p.npy']):
        with pytest.raises(SystemExit):
            isinf.build_parser().parse_args(bad)
    assert inception.build_parser().parse_args(['--dir', 'd']).save_probs is None
    assert inception.build_parser().parse_args(['--dir', 'd', '--save_probs', 'o.npy']).save_probs == 'o.npy'
    assert sample.make_parser().parse_args(['--checkpoint', 'c']).is_infinity is False
    assert sample.make_parser().parse_args(['--checkpoint', 'c', '--is_infinity', '1']).is_infinity is True


def test_load_probs(tmp_path):
    path = str(tmp_path / 'p.npy')
    np.save(path, np.full((3, 4), 0.25))
    got = isinf.load_probs(path)
    assert got.dtype == np.float32 and got.shape == (3, 4) and got.flags['C_CONTIGUOUS']
    np.save(path, np.zeros(5))
    with pytest.raises(ValueError, match='softmax rows'):
        isinf.load_probs(path)
    np.save(path, np.zeros((3, 4), np.int64))
    with pytest.raises(ValueError, match='softmax rows'):
        isinf.load_probs(path)


def test_sample_is_infinity_needs_the_network_and_enough_pictures(tmp_path):
    args = sample.make_parser().parse_args(['--checkpoint', 'none', '--is_infinity', '1'])
    with pytest.raises(ValueError, match='--is_infinity needs --inception_weights'):
        sample.run_model(args, None, str(tmp_path / 'out'))
    args = sample.make_parser().parse_args(['--checkpoint', 'none', '--is_infinity', '1', '--inception_weights', 'w.pth', '--num_samples', '3'])
    with pytest.raises(ValueError, match='draw_sizes'):                              # refused before the first picture
        sample.run_model(args, None, str(tmp_path / 'out'))
    assert not (tmp_path / 'out').exists()
