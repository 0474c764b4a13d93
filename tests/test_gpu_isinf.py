"""IS-infinity on the GPU (csrc/isinf.hip, ops/isinf.py, scene_generation_amd/isinf.py).

* ``sg_isinf_row_terms`` against the float64 restatement of tests/isinf_ref.py within the DERIVED bounds of its docstring, between guard
  words: 37 rows of 1, 10, 1000 and 1008 classes, a padded row stride and a base one float into its allocation, rows with exact zeros,
  one all-zero row, rows whose sum is not 1.
* ``sg_isinf_subset_scores`` on ragged subsets around R = SG_ISINF_ROWS_PER_WG (2, 3, R - 1, R, R + 1 and 2 R + 1 of 2 R + 1 rows, one in
  identity order; S = 7 and S = 1) within the derived bound on the log score, over both loaders (16-byte and 4-byte), a ragged last
  column vector and two column tiles; bit-identical repeats; poison beyond ``out`` and the queried workspace untouched; negative codes
  with nothing written.
* The full-set point against ``InceptionScore.scores(1)``: two independent kernels for one definition, within the same bound.
* End to end against the restated pipeline, through a scorer fed by a stand-in network, ``check_model``, the two command lines and
  ``sample --is_infinity 1``.
The worst share of each bound goes to isinf_margins.json in the suite's output directory (profiles/isinf_test_margins.md).
The tree only: no reference checkout."""
import ctypes

import numpy as np
import pytest
import torch

import isinf_ref as R
from fidinf_ref import _Net
from gpu_harness import Margins, N, _guarded, _guards_ok, _place, margins_fixture
from sampling_helpers import _images
from scene_generation_amd import _hip
from scene_generation_amd import inception as I
from scene_generation_amd import isinf as II
from scene_generation_amd import ops, sample

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POISON = -777.0
RPW = _hip.CONST['SG_ISINF_ROWS_PER_WG']
MARGINS = Margins()
_write_margins = margins_fixture(lambda: MARGINS.dump('isinf_margins.json', 'share_of_bound', empty=False))


def _share(err, bound):
    """the largest err / bound; a zero bound (an exact value) allows a zero error only"""
    err, bound = np.atleast_1d(err), np.atleast_1d(bound)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _rows(n, C, seed):
    """test rows: exact zeros in some, one all-zero row, rows whose sum is 0.5 and 3"""
    p = R.rows(seed, n, C, 0.02 if C >= 1000 else 0.5)
    p[1, ::3] = 0.0
    p[n // 2] = 0.0
    p[2] *= 0.5
    p[n - 1] *= 3.0
    return p


# =====================================================================================================================================
# 1. the row terms
# =====================================================================================================================================
@pytest.mark.parametrize('extra,off', [(0, 0), (3, 1)], ids=['tight', 'padded_off1'])
@pytest.mark.parametrize('C', [1, 10, 1000, 1008])
def test_row_terms_within_the_derived_bound(C, extra, off):
    n = 37
    p = _rows(n, C, 100 + C)
    want_s, want_h = R.row_terms(p)
    bs, bh = R.row_bounds(want_s, want_h, C)
    sbuf, rs = _guarded((n,), fill=POISON)
    hbuf, h = _guarded((n,), fill=POISON)
    view = _place(p, extra, off)
    got = ops.isinf_row_terms(view, rs=rs, h=h)
    assert got[0] is rs and got[1] is h and _guards_ok(sbuf, POISON) and _guards_ok(hbuf, POISON)
    s, hh = N(rs), N(h)
    assert np.isfinite(s).all() and np.isfinite(hh).all() and s[n // 2] == 0.0 and hh[n // 2] == 0.0      # the all-zero row: exact zeros
    share_s, share_h = _share(np.abs(s - want_s), bs), _share(np.abs(hh - want_h), bh)
    print('row terms C=%d extra=%d off=%d: worst share of the bound s %.4f h %.4f' % (C, extra, off, share_s, share_h))
    MARGINS.note('row_sums', share_s, '%d_%d_%d' % (C, extra, off))
    MARGINS.note('row_entropies', share_h, '%d_%d_%d' % (C, extra, off))
    assert share_s <= 1.0 and share_h <= 1.0
    rs2, h2 = ops.isinf_row_terms(view)
    assert np.array_equal(N(rs2), s) and np.array_equal(N(h2), hh)                   # the same call, the same bits


# =====================================================================================================================================
# 2. the subset scores
# =====================================================================================================================================
def _ragged_tables(n, seed):
    """sizes 2, 3, R - 1, R, R + 1, 2 R + 1 (drawn) and 2 R + 1 (identity) of n = 2 R + 1 rows"""
    assert n == 2 * RPW + 1
    sizes = np.array([2, 3, RPW - 1, RPW, RPW + 1, n, n], np.int32)
    rs = np.random.RandomState(seed)
    idx = np.zeros((7, n), np.int32)
    for q, s in enumerate(sizes[:6]):
        idx[q, :s] = rs.permutation(n)[:s]
    idx[0, :2] = (n - 1, 0)                          # the last row and the first
    idx[6] = np.arange(n)
    return idx, sizes


# (C, extra, off): 4-byte loader (stride not a multiple of 4; base off by one float), 16-byte loader with a ragged last vector,
# tight 1000 and 1008, two column tiles with a ragged last vector
SUBSET_CASES = [(10, 0, 0), (10, 2, 0), (1000, 0, 0), (1000, 3, 1), (1008, 0, 0), (1030, 2, 0)]


@pytest.mark.parametrize('C,extra,off', SUBSET_CASES, ids=lambda v: str(v))
def test_subset_scores_on_ragged_subsets(C, extra, off):
    n = 2 * RPW + 1
    p = _rows(n, C, 200 + C)
    idx, sizes = _ragged_tables(n, C)
    want, parts = R.subset_scores(p, idx, sizes)
    view = _place(p, extra, off)
    assert (view.data_ptr() % 16 == 0 and view.stride(0) % 4 == 0) == ((C, extra, off) not in ((10, 0, 0), (1000, 3, 1)))
    rs, h = ops.isinf_row_terms(view)
    obuf = torch.full((7 + 2, 2), POISON, dtype=torch.float64, device=DEV)          # two rows beyond S
    got = ops.isinf_subset_scores(view, rs, h, idx, sizes, out=obuf[:7])
    assert got.data_ptr() == obuf.data_ptr() and (obuf[7:] == POISON).all().item()
    out = N(got)
    assert np.isfinite(out).all()
    for q, s in enumerate(sizes):
        bl, bs = R.log_score_bound(*parts[q], C), R.score_bound(want[q, 1], *parts[q], C)
        sl, ss = abs(out[q, 0] - want[q, 0]) / bl, abs(out[q, 1] - want[q, 1]) / bs
        print('subset of %d rows, C=%d: log score %.15g (%.4f of the bound %.3g), score %.4f of its bound' % (s, C, out[q, 0], sl, bl, ss))
        MARGINS.note('subset_log_score', sl, '%d_%d_%d_%d' % (C, extra, off, s))
        MARGINS.note('subset_score', ss, '%d_%d_%d_%d' % (C, extra, off, s))
        assert sl <= 1.0 and ss <= 1.0
    again = ops.isinf_subset_scores(view, rs, h, idx, sizes)
    assert np.array_equal(N(again), out)                                            # the same call, the same bits
    # S = 1: every subset alone gives the bits it had among the seven (its chunks and its finishing workgroup are its own)
    for q in (0, 3, 4, 6):
        one = ops.isinf_subset_scores(view, rs, h, idx[q:q + 1, :max(int(sizes[q]), 2)], sizes[q:q + 1])
        assert np.array_equal(N(one)[0], out[q]), q


def _raw(view, rs, h, didx, dsz, S, smax, out, ws, ws_bytes, **over):
    """the entry point itself, on device tables"""
    n, C = view.shape
    a = dict(probs=view.data_ptr(), n=n, classes=C, ldp=view.stride(0), rs=ops._pd(rs), h=ops._pd(h), idx=didx.data_ptr(),
             sizes=dsz.data_ptr(), S=S, smax=smax, out=ops._pd(out), ws=ws.data_ptr(), ws_bytes=ws_bytes, stream=ops._stream())
    a.update({k[:-1]: v for k, v in over.items()})          # (overrides are spelled with a trailing underscore: rs_=None)
    return _hip.lib().sg_isinf_subset_scores(*[a[k] for k in _hip.PROTOS['sg_isinf_subset_scores'][2]])


def test_workspace_tail_bad_arguments_and_table_entries_outside_the_set():
    n, C = 2 * RPW + 1, 10
    p = _rows(n, C, 7)
    idx, sizes = _ragged_tables(n, 3)
    view = _place(p, 2, 0)
    rs, h = ops.isinf_row_terms(view)
    need = int(_hip.lib().sg_isinf_subset_scores_ws_bytes(7, n, C))
    assert need == 8 * 7 * ((n + RPW - 1) // RPW + 1) * (2 * C + 1)
    ws = torch.full((need // 8 + 16,), POISON, dtype=torch.float64, device=DEV)
    out = torch.full((9, 2), POISON, dtype=torch.float64, device=DEV)
    didx, dsz = torch.from_numpy(idx).to(DEV), torch.from_numpy(sizes).to(DEV)
    # every bad argument: a negative code, nothing launched, nothing written
    odd = lambda t: ctypes.cast(t.data_ptr() + 4, ctypes.POINTER(ctypes.c_double))
    bad = [dict(probs=None), dict(rs=None), dict(h=None), dict(idx=None), dict(sizes=None), dict(out=None), dict(ws=None),
           dict(probs=view.data_ptr() + 2), dict(rs=odd(rs)), dict(h=odd(h)), dict(out=odd(out)), dict(ws=ws.data_ptr() + 4),
           dict(idx=didx.data_ptr() + 2), dict(sizes=dsz.data_ptr() + 2), dict(n=0), dict(classes=0), dict(ldp=C - 1), dict(S=-1),
           dict(smax=1), dict(ws_bytes=need - 1)]
    for kw in bad:
        assert _raw(view, rs, h, didx, dsz, 7, n, out, ws, need, **{k + '_': v for k, v in kw.items()}) < 0 and 'sg_isinf_subset_scores' in _hip.last_error(), kw
    for kw in (dict(probs=None), dict(rs=None), dict(h=odd(h)), dict(n=0), dict(classes=0), dict(ldp=C - 1)):
        a = dict(probs=view.data_ptr(), n=n, classes=C, ldp=view.stride(0), rs=ops._pd(rs), h=ops._pd(h), stream=ops._stream())
        a.update(kw)
        assert _hip.lib().sg_isinf_row_terms(*[a[k] for k in _hip.PROTOS['sg_isinf_row_terms'][2]]) < 0, kw
    torch.cuda.synchronize()
    assert (ws == POISON).all().item() and (out == POISON).all().item()
    assert _raw(view, rs, h, didx, dsz, 0, n, out, ws, 0, probs_=None, rs_=None, h_=None, idx_=None, sizes_=None, out_=None, ws_=None) == 0
    # the call itself: the queried bytes are enough, what lies beyond them and beyond S rows of out stays
    assert _raw(view, rs, h, didx, dsz, 7, n, out, ws, need) == 0
    first = N(out)
    assert (ws[need // 8:] == POISON).all().item() and (first[7:] == POISON).all() and np.isfinite(first[:7]).all()
    assert np.array_equal(first[:7], N(ops.isinf_subset_scores(view, rs, h, idx, sizes)))
    # entries outside [0, n) read as rows that contribute nothing (the restatement: an appended all-zero row); a size is clamped to
    # [0, smax] and below 2 both outputs are NaN
    wild = idx.copy()
    wild[1, 1], wild[4, 0], wild[4, RPW] = -1, n, 2 ** 31 - 1
    wsz = sizes.copy()
    wsz[0], wsz[2], wsz[5] = 1, -5, n + 1000
    ref_p = np.concatenate([p, np.zeros((1, C), np.float32)])
    ref_idx = np.where((wild < 0) | (wild >= n), n, wild)
    ref_sz = np.clip(wsz, 0, n)
    want, parts = R.subset_scores(ref_p, ref_idx[[1, 3, 4, 5, 6]], ref_sz[[1, 3, 4, 5, 6]])
    assert _raw(view, rs, h, torch.from_numpy(wild).to(DEV), torch.from_numpy(wsz).to(DEV), 7, n, out, ws, need) == 0
    got = N(out)
    assert np.isnan(got[[0, 2]]).all() and (got[7:] == POISON).all()
    for k, q in enumerate([1, 3, 4, 5, 6]):
        assert abs(got[q, 0] - want[k, 0]) <= R.log_score_bound(*parts[k], C), q
    assert np.array_equal(got[[3, 5, 6]], first[[3, 5, 6]])                          # (5: a size beyond smax is all of its table row)
    assert not np.array_equal(got[4], first[4])


def test_wrappers_refuse():
    p = torch.full((6, 8), 0.125, device=DEV)
    rs, h = ops.isinf_row_terms(p)
    good, sz = np.zeros((2, 4), np.int32), np.array([2, 4], np.int32)
    good[1] = (0, 1, 2, 3)
    calls = ops.CALLS[0]
    bad = [lambda: ops.isinf_subset_scores(p, rs, h, np.array([[0, 6, 0, 0], [0, 0, 0, 0]], np.int32), sz),       # an index outside the set
           lambda: ops.isinf_subset_scores(p, rs, h, np.array([[0, -1, 0, 0], [0, 0, 0, 0]], np.int32), sz),
           lambda: ops.isinf_subset_scores(p, rs, h, good, np.array([1, 4], np.int32)),                            # sizes outside 2 .. smax
           lambda: ops.isinf_subset_scores(p, rs, h, good, np.array([2, 5], np.int32)),
           lambda: ops.isinf_subset_scores(p, rs, h, good, np.array([2], np.int32)),
           lambda: ops.isinf_subset_scores(p, rs, h, good[:, :1], np.array([1, 1], np.int32)),                     # smax < 2
           lambda: ops.isinf_subset_scores(p, rs, h, torch.zeros(2, 4, dtype=torch.int32, device=DEV), sz),        # device tables cannot be checked
           lambda: ops.isinf_subset_scores(p, rs.float(), h, good, sz),
           lambda: ops.isinf_subset_scores(p, rs[:5], h, good, sz),
           lambda: ops.isinf_subset_scores(p, rs, h.cpu(), good, sz),
           lambda: ops.isinf_subset_scores(p, rs, h, good, sz, out=torch.zeros(2, 3, dtype=torch.float64, device=DEV)),
           lambda: ops.isinf_row_terms(p, rs=torch.zeros(5, dtype=torch.float64, device=DEV)),
           lambda: ops.isinf_row_terms(p[:0])]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        ops.isinf_row_terms(p.double())
    assert ops.CALLS[0] == calls                    # nothing was launched
    assert tuple(ops.isinf_subset_scores(p, rs, h, np.zeros((0, 4), np.int32), np.zeros(0, np.int32)).shape) == (0, 2)
    out = N(ops.isinf_subset_scores(p, rs, h, good, sz))
    assert np.abs(out[:, 0]).max() <= 1e-14 and np.abs(out[:, 1] - 1).max() <= 1e-14              # identical rows: score 1


# =====================================================================================================================================
# 3. end to end
# =====================================================================================================================================
class _Stand(_Net):
    """the stand-in network with what an ``InceptionScore`` calls: ``features`` (the first ``dim`` values of the flattened image) and
    an ``fc`` to 1000 classes"""

    def __init__(self, dim=64, classes=1000):
        super().__init__(dim)
        g = torch.Generator().manual_seed(11)
        self.fc = torch.nn.Linear(dim, classes)
        with torch.no_grad():
            self.fc.weight.copy_(torch.randn(classes, dim, generator=g) * 0.6)
            self.fc.bias.zero_()
        self.dim = dim

    def features(self, x):
        return x.flatten(1)[:, :self.dim].contiguous()


@pytest.fixture(scope='module')
def scored():
    """a scorer fed 300 pictures in chunks of 32, the host copy of its rows and their restated row terms"""
    scorer = I.InceptionScore(batch_size=32, resize=False, weights=_Stand(), device=DEV)
    g = torch.Generator().manual_seed(5)
    imgs = torch.randn(300, 3, 8, 8, generator=g)
    scorer(imgs[:130])
    scorer(imgs[130:])
    p = N(scorer.rows())
    return scorer, p, R.row_terms(p)


def _full_parts(p):
    n = p.shape[0]
    _, parts = R.subset_scores(p, np.arange(n, dtype=np.int32)[None], [n])
    return parts[0]


def test_rows_accessor_and_the_full_set_against_the_existing_score(scored):
    scorer, p, _ = scored
    assert scorer.count == 300 and tuple(scorer.rows().shape) == (300, 1000) and scorer.rows().data_ptr() == scorer.probs.data_ptr()
    assert scorer.probs.size(0) > 300 and abs(p.sum(1) - 1).max() < 1e-5
    res = II.is_infinity(scorer.rows())
    existing = scorer.scores(1)[0].item()
    H, T, n = _full_parts(p)
    bound = R.score_bound(existing, H, T, n, 1000)
    share = abs(res['is'] - existing) / bound
    print('IS of all 300 rows: the subset kernels %.15g, sg_inception_score %.15g, %.4f of the bound %.3g' % (res['is'], existing, share, bound))
    MARGINS.note('full_set_against_inception_score', share, '300_1000')
    assert share <= 1.0
    assert res['is'] > 5.0                           # a peaked, varied set of rows: the test can tell a score from 1


@pytest.mark.parametrize('points,repeats', [(15, 1), (15, 3), (2, 1), (2, 3)])
def test_is_infinity_against_the_restated_pipeline(scored, points, repeats):
    scorer, p, terms = scored
    idx, tsizes, point, sizes = II.draw_tables(300, points, None, 0, repeats)
    want_out, parts = R.subset_scores(p, idx, tsizes, terms)
    want = II.from_scores(sizes, point, want_out, 300)
    whole = R.pipeline(p, points, None, 0, repeats)                                  # the restatement of the host's share as well
    assert want['sizes'] == whole['sizes'].tolist() and abs(want['is_inf'] - whole['is_inf']) <= 1e-10 * abs(whole['is_inf'])
    assert abs(want['is_inf_log'] - whole['is_inf_log']) <= 1e-10 * whole['is_inf_log']
    res = II.is_infinity(scorer.rows(), num_points=points, repeats=repeats)
    assert sorted(res) == ['images', 'is', 'is_inf', 'is_inf_log', 'scores', 'sizes', 'slope']
    assert res['sizes'] == want['sizes'] and res['images'] == 300 and len(res['scores']) == len(res['sizes']) == points
    assert res['is'] == res['scores'][-1]
    rs, h = ops.isinf_row_terms(scorer.rows())
    dev_out = N(ops.isinf_subset_scores(scorer.rows(), rs, h, idx, tsizes))
    assert res == II.from_scores(sizes, point, dev_out, 300)                         # the function is these two calls and the host's share
    # every subset within its own derived bound; a point is the mean of its subsets, so within the largest of theirs
    bl = np.array([R.log_score_bound(*parts[k], 1000) for k in range(len(tsizes))])
    bs = np.array([R.score_bound(want_out[k, 1], *parts[k], 1000) for k in range(len(tsizes))])
    share = max(_share(np.abs(dev_out[:, 0] - want_out[:, 0]), bl), _share(np.abs(dev_out[:, 1] - want_out[:, 1]), bs))
    pl = np.array([bl[point == k].max() for k in range(points)])
    ps = np.array([bs[point == k].max() for k in range(points)])
    assert (np.abs(np.array(res['scores']) - want['scores']) <= ps).all()
    # an intercept is a linear map of the points, intercept = sum_k coef_k y_k: it moves by at most sum_k |coef_k| bound_k
    x = 1.0 / sizes
    coef = 1.0 / len(x) - x.mean() * (x - x.mean()) / ((x - x.mean()) ** 2).sum()
    b_inf, b_log = float((np.abs(coef) * ps).sum()), float((np.abs(coef) * pl).sum())
    s_inf = abs(res['is_inf'] - want['is_inf']) / (b_inf + 8 * R.U * np.abs(coef).sum() * max(want['scores']))
    s_log = abs(np.log(res['is_inf_log']) - np.log(want['is_inf_log'])) / (b_log + 8 * R.U * np.abs(coef).sum() * np.log(max(want['scores'])))
    print('is_infinity points=%d repeats=%d: subsets within %.4f of their bounds, IS_inf %.12g (%.4f of its bound), IS_inf_log %.12g (%.4f)'
          % (points, repeats, share, res['is_inf'], s_inf, res['is_inf_log'], s_log))
    MARGINS.note('is_infinity_subsets', share, '%d_%d' % (points, repeats))
    MARGINS.note('is_infinity_intercept', s_inf, '%d_%d' % (points, repeats))
    MARGINS.note('is_infinity_log_intercept', s_log, '%d_%d' % (points, repeats))
    assert share <= 1.0 and s_inf <= 1.0 and s_log <= 1.0
    assert II.is_infinity(scorer.rows(), num_points=points, repeats=repeats) == res  # the same bits
    if repeats == 3:
        assert res['is'] == II.is_infinity(scorer.rows(), num_points=points)['is']   # the full set: once, not averaged
    other = II.is_infinity(scorer.rows(), num_points=points, repeats=repeats, seed=1)
    assert other['is'] == res['is'] and other['scores'][0] != res['scores'][0]


def test_one_host_read(scored, monkeypatch):
    scorer = scored[0]
    reads = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda t, *a, **k: (reads.append(tuple(t.shape)), real(t, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, 'item', lambda t: reads.append('item'))
    monkeypatch.setattr(torch.Tensor, 'tolist', lambda t: reads.append('tolist'))
    II.ISInfinity(scorer, repeats=2).compute()
    assert reads == [(2 * 14 + 1, 2)]


def test_isinfinity_after_check_model():
    from scene_generation_amd.evaluate import check_model
    from scene_generation_amd.model import Model
    from sampling_helpers import sampling_batch as _batch, sampling_model
    m = sampling_model(Model, DEV).eval()
    sc = I.InceptionScore(batch_size=4, resize=True, weights=None, device=DEV)
    cfg = type('A', (), {'num_val_samples': 6})()
    loader = [_batch(1), _batch(2), _batch(3)]
    result = check_model(cfg, loader, m, sc, use_gt=True)
    assert len(result) == 4 and sc.count == 6 and result[3] is None                 # the signature and the return value are what they were
    res = II.ISInfinity(sc).compute()
    assert res['images'] == 6 and res['sizes'] == [3, 4, 5, 6] and np.isfinite(res['is_inf']) and np.isfinite(res['is_inf_log'])
    p = N(sc.rows())
    want = R.pipeline(p)
    H, T, n = _full_parts(p)
    assert abs(res['is'] - want['is']) <= R.score_bound(want['is'], H, T, n, p.shape[1])
    assert abs(res['is'] - sc.scores(1)[0].item()) <= R.score_bound(want['is'], H, T, n, p.shape[1])
    assert check_model(cfg, loader, m, sc, use_gt=True)[1:3] == result[1:3] and II.ISInfinity(sc).compute() == res


# =====================================================================================================================================
# 4. the command lines
# =====================================================================================================================================
def test_command_lines_and_the_probs_round_trip(tmp_path, capsys):
    Image = pytest.importorskip('PIL.Image')
    (tmp_path / 'pics').mkdir()
    px = ((_images(6, 6, 40) * 0.5 + 0.5) * 255).round().byte().permute(0, 2, 3, 1).numpy()
    for i in range(6):
        Image.fromarray(px[i]).save(str(tmp_path / 'pics' / ('%d.png' % i)))
    probs = str(tmp_path / 'probs.npy')
    capsys.readouterr()
    mean, _ = I.main(['--dir', str(tmp_path / 'pics'), '--batch_size', '2', '--splits', '1', '--save_probs', probs])
    capsys.readouterr()
    rows = np.load(probs)
    assert rows.shape == (6, 1000) and rows.dtype == np.float32
    a = II.main(['--dir', str(tmp_path / 'pics'), '--batch_size', '2'])
    out = capsys.readouterr()
    assert 'WITHOUT pretrained weights' in out.err
    assert out.out.strip().splitlines()[-2:] == II.format_lines(a) == ['IS_inf {}'.format(a['is_inf']), 'IS_N {} N 6'.format(a['is'])]
    assert a['sizes'] == [3, 4, 5, 6] and a['images'] == 6 and np.isfinite(a['is_inf'])
    H, T, n = _full_parts(rows)
    assert abs(a['is'] - mean) <= R.score_bound(mean, H, T, n, 1000)                # the full-set value is the score command's number
    # the saved rows: the same numbers, and no network is built
    b = II.main(['--probs', probs])
    out = capsys.readouterr()
    assert 'WITHOUT pretrained weights' not in out.err and b == a and out.out.strip().splitlines() == II.format_lines(a)
    c = II.main(['--probs', probs, '--num_points', '2', '--min_size', '4', '--repeats', '2', '--seed', '3'])
    assert c['sizes'] == [4, 6] and c['is'] == a['is']


def test_sample_cli_prints_the_line_after_the_inception_line(tmp_path, capsys):
    import random
    from trainer_helpers import _batch as ema_batch, _run, _trainer
    tr, ck, args = _trainer(tmp_path / 'train')
    _run(tr, ema_batch(), range(1))
    path = tr.save_checkpoint(ck, 1, args, 0)
    torch.manual_seed(3)
    weights = str(tmp_path / 'inception.pth')
    torch.save(I.InceptionV3().state_dict(), weights)
    base = ['--checkpoint', path, '--use_gt_boxes', '1', '--use_gt_masks', '1', '--use_gt_textures', '1', '--batch_size', '3',
            '--num_samples', '6', '--inception_weights', weights, '--inception_splits', '1']
    runs = []
    for k, extra in enumerate(([], ['--is_infinity', '1'])):
        capsys.readouterr()
        random.seed(0)
        res = sample.main(base + ['--output_dir', str(tmp_path / ('out%d' % k))] + extra)
        runs.append((res, capsys.readouterr().out.splitlines()))
    (res0, out0), (res1, out1) = runs
    assert 'is_inf' not in res0 and not any(l.startswith('IS_inf') for l in out0)                # 0 is the default
    at = [i for i, l in enumerate(out1) if l.startswith('Inception ')]
    assert len(at) == 1 and out1[at[0] + 1] == 'IS_inf {}'.format(res1['is_inf']['is_inf'])        # directly after the Inception line
    assert out1[:at[0] + 1] + out1[at[0] + 2:] == out0                              # and nothing else changed
    assert res1['inception'] == res0['inception']
    inf = res1['is_inf']
    assert inf['images'] == 6 and inf['sizes'] == [3, 4, 5, 6] and np.isfinite(inf['is_inf'])
    assert abs(inf['is'] - res1['inception']['mean']) <= 1e-9 * inf['is']            # (plumbing; the tight comparison is in section 3)
    # a count that gives no two subset sizes is refused before the first picture
    with pytest.raises(ValueError, match='draw_sizes'):
        sample.main(base[:11] + ['3'] + base[12:] + ['--output_dir', str(tmp_path / 'short'), '--is_infinity', '1'])
    assert not (tmp_path / 'short').exists()
