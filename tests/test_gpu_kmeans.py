"""The appearance bank on the GPU: the four k-means kernels against the float64 restatement of tests/kmeans_ref.py with derived
tolerances (eps = 2^-23), the Lloyd loop (converged parity, fixed point, determinism, k = 1), bank.encode against
evaluate.encode_features, the command lines end to end and the launch profile of a bank build.  The tree only: no reference
checkout."""
import json
import math
import os

import numpy as np
import pytest
import torch

import kmeans_ref as KR
from gpu_harness import _dump
from scene_generation_amd import bank, ops, sample
from scene_generation_amd.model import Model
from scene_generation_amd.synthetic import fill_deterministic, make_batch, make_sampling_vocab, make_vocab

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = KR.EPS
PARITY = {}
KM_KINDS = {'kmeans_assign', 'kmeans_update', 'kmeans_relocate', 'kmeans_pp'}


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _record(key, value):
    PARITY[key] = max(PARITY.get(key, 0.0), float(value))


def _sizes(K, P=20000):
    s = [0, 1, max(K - 3, 0), K, 3000, 7000]
    return s + [P - sum(s)]


def _data(kind, K, D, seed, sizes=None):
    """(x float32 [P, D], offsets int64 [C + 1]): the reference works on the SAME fp32 numbers, widened to fp64"""
    rs = np.random.RandomState(seed)
    x, off = KR.segmented(rs, sizes or _sizes(K), K, D, kind)
    return x.astype(np.float32), off, rs


def _perturbed_centers(x, off, K, rs, scale=0.1):
    """centres = perturbed rows of the class (its first k_c rows of the block)"""
    C, D = len(off) - 1, x.shape[1]
    cen = np.zeros((C, K, D), dtype=np.float32)
    for c in range(C):
        n = off[c + 1] - off[c]
        k = min(n, K)
        if k:
            rows = off[c] + rs.choice(n, k, replace=False)
            cen[c, :k] = x[rows] + scale * rs.randn(k, D).astype(np.float32)
    return cen


def _two_nearest(x64, c64, chunk=256):
    """per row: (best index, best d2, second index, second d2) in fp64, a tie to the lowest index"""
    n, k = len(x64), len(c64)
    j1, d1, j2, d2 = np.zeros(n, np.int64), np.zeros(n), np.full(n, -1, np.int64), np.full(n, np.inf)
    for a in range(0, n, chunk):
        d = KR.dist2(x64[a:a + chunk], c64)
        idx = np.arange(len(d))
        b = d.argmin(1)
        j1[a:a + chunk], d1[a:a + chunk] = b, d[idx, b]
        if k > 1:
            d[idx, b] = np.inf
            s = d.argmin(1)
            j2[a:a + chunk], d2[a:a + chunk] = s, d[idx, s]
    return j1, d1, j2, d2


def _assign_dev(x, off, cen, prev=None, state=None):
    plan = ops.kmeans_plan(T(off, torch.int32))
    C, K = cen.shape[0], cen.shape[1]
    labels = torch.full((1, plan.P), -1, dtype=torch.int32, device=DEV) if prev is None else prev.clone()
    mind2 = torch.zeros(1, plan.P, device=DEV)
    changed = torch.zeros(1, C, dtype=torch.int32, device=DEV)
    acount = torch.zeros(1, C, K, dtype=torch.int32, device=DEV)
    ops.kmeans_assign(T(x), plan, T(cen).unsqueeze(0).contiguous(), labels, mind2, changed, acount, state)
    return plan, labels, mind2, changed, acount


def _check_labels(x, off, cen, lab, md=None, tag=''):
    """labels against the fp64 argmin outside the tie band, one of the two nearest inside it, at most 1 % of the rows banded;
    -> boolean mask of the banded rows"""
    banded = np.zeros(len(x), dtype=bool)
    for c in range(len(off) - 1):
        a, b = off[c], off[c + 1]
        k = min(b - a, cen.shape[1])
        if not k:
            continue
        x64, c64 = x[a:b].astype(np.float64), cen[c, :k].astype(np.float64)
        j1, d1, j2, d2 = _two_nearest(x64, c64)
        band = KR.tie_band(x64, c64)
        inb = (d2 - d1) <= band
        banded[a:b] = inb
        got = lab[a:b]
        assert ((got >= 0) & (got < k)).all(), (tag, c)
        assert (got[~inb] == j1[~inb]).all(), (tag, c, int((got[~inb] != j1[~inb]).sum()))
        assert ((got[inb] == j1[inb]) | (got[inb] == j2[inb])).all(), (tag, c)
        if md is not None:
            err = np.abs(md[a:b].astype(np.float64) - d1)
            assert (err <= band).all(), (tag, c, float((err / band).max()))
            _record('assign: max |mind2 - fp64| / bound', (err / band).max())
    frac = banded.mean() if len(x) else 0.0
    _record('assign: largest share of rows in the tie band', frac)
    assert frac <= 0.01, (tag, frac)
    return banded


# ---- assign --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 10, 100])
@pytest.mark.parametrize('D', [8, 32, 128])
@pytest.mark.parametrize('kind', ['noise', 'relu', 'blobs'])
def test_assign_one_step(kind, D, K):
    x, off, rs = _data(kind, K, D, seed=1000 + 7 * D + K)
    cen = _perturbed_centers(x, off, K, rs)
    plan, labels, mind2, changed, acount = _assign_dev(x, off, cen)
    lab, md = N(labels[0]), N(mind2[0])
    _check_labels(x, off, cen, lab, md, tag='%s D=%d K=%d' % (kind, D, K))
    sizes = np.diff(off)
    assert np.array_equal(N(changed[0]), sizes), 'every label differs from the initial -1'
    for c in range(len(sizes)):
        assert np.array_equal(N(acount[0, c]), np.bincount(lab[off[c]:off[c + 1]], minlength=K)), c
    # the same centres again: nothing changes, same bits
    _, labels2, mind22, changed2, _ = _assign_dev(x, off, cen, prev=labels)
    assert torch.equal(labels2, labels) and torch.equal(mind22, mind2) and int(changed2.abs().sum()) == 0


def test_assign_tie_goes_to_the_lowest_index_and_ranges_are_checked():
    x = np.zeros((5, 8), dtype=np.float32)
    x[:, 0] = [0, 1, 2, 3, 4]
    cen = np.zeros((1, 4, 8), dtype=np.float32)
    cen[0, :, 0] = [3, 1, 1, 3]                       # centres 1 = 2 and 0 = 3 coincide; row 2 is equally far from all
    _, labels, mind2, _, _ = _assign_dev(x, np.array([0, 5]), cen)
    assert N(labels[0]).tolist() == [1, 1, 0, 0, 0] and N(mind2[0]).tolist() == [1, 0, 1, 0, 1]
    with pytest.raises(RuntimeError, match='the MI355X HIP path has no CPU fallback'):
        ops.kmeans_plan(torch.tensor([0, 5], dtype=torch.int32))
    with pytest.raises(RuntimeError, match='D=129'):
        _assign_dev(np.zeros((5, 129), dtype=np.float32), np.array([0, 5]), np.zeros((1, 2, 129), dtype=np.float32))
    with pytest.raises(RuntimeError, match='K=257'):
        _assign_dev(np.zeros((5, 8), dtype=np.float32), np.array([0, 5]), np.zeros((1, 257, 8), dtype=np.float32))
    # the documented upper corner works: D = 128, K = 256 (and a D that is no multiple of 4)
    for D, K in [(128, 256), (30, 7)]:
        xs, off, rs = _data('noise', K, D, seed=5, sizes=[300, 0, 1500])
        cs = _perturbed_centers(xs, off, K, rs)
        _, lab, md, _, _ = _assign_dev(xs, off, cs)
        _check_labels(xs, off, cs, N(lab[0]), N(md[0]), tag='D=%d K=%d' % (D, K))


# ---- update --------------------------------------------------------------------------------------------------------------------------
def _update_dev(x, off, lab, md, cen_old, **kw):
    plan = ops.kmeans_plan(T(off, torch.int32))
    C, K, D = cen_old.shape
    cen = T(cen_old).unsqueeze(0).contiguous()
    counts = torch.zeros(1, C, K, dtype=torch.int32, device=DEV)
    inertia, shift = torch.zeros(1, C, device=DEV), torch.zeros(1, C, device=DEV)
    ops.kmeans_update(T(x), plan, T(lab, torch.int32).unsqueeze(0).contiguous(), T(md).unsqueeze(0).contiguous(), cen, counts,
                      inertia, shift, **kw)
    return cen, counts, inertia, shift


def _check_centers(x, off, lab, cen_dev, cen_old, tag=''):
    """every centre within (n_j - 1) eps mean_i |x_i| per component of the fp64 mean (the worst case of ANY fp32 summation order);
    a centre without rows keeps its value"""
    for c in range(len(off) - 1):
        a, b = off[c], off[c + 1]
        k = min(b - a, cen_old.shape[1])
        x64 = x[a:b].astype(np.float64)
        for j in range(k):
            rows = x64[lab[a:b] == j]
            if not len(rows):
                assert np.array_equal(cen_dev[c, j], cen_old[c, j]), (tag, c, j)
                continue
            bound = (len(rows) - 1) * EPS * np.abs(rows).mean(0)
            err = np.abs(cen_dev[c, j].astype(np.float64) - rows.mean(0))
            assert (err <= bound).all(), (tag, c, j, len(rows), float(err.max()))
            if len(rows) > 1 and bound.min() > 0:
                _record('update: max |centre - fp64 mean| / bound', (err / bound).max())
                _record('update: max |centre - fp64 mean|', err.max())


@pytest.mark.parametrize('K,D,kind', [(100, 32, 'relu'), (10, 32, 'blobs'), (100, 128, 'noise'), (1, 8, 'noise'), (10, 30, 'relu')])
def test_update_given_labels(K, D, kind):
    x, off, rs = _data(kind, K, D, seed=77 + K + D)
    cen_old = _perturbed_centers(x, off, K, rs)
    _, labels, mind2, _, _ = _assign_dev(x, off, cen_old)
    lab, md = N(labels[0]).copy(), N(mind2[0])
    big = len(off) - 2                                  # leave two centres of the largest class without rows
    if K >= 10:
        seg = lab[off[big]:off[big + 1]]
        seg[seg == 2] = 3
        seg[seg == 5] = 0
    cen, counts, inertia, shift = _update_dev(x, off, lab, md, cen_old)
    cen = N(cen[0])
    _check_centers(x, off, lab, cen, cen_old, tag='%s D=%d K=%d' % (kind, D, K))
    for c in range(len(off) - 1):
        seg = lab[off[c]:off[c + 1]]
        assert np.array_equal(N(counts[0, c]), np.bincount(seg, minlength=K)), 'counts are exact'
        want = md[off[c]:off[c + 1]].astype(np.float64).sum()
        n_c = len(seg)
        assert abs(float(inertia[0, c]) - want) <= n_c * EPS * want, (c, float(inertia[0, c]), want)
        if want > 0:
            _record('update: max inertia error / (n_c eps inertia)', abs(float(inertia[0, c]) - want) / (n_c * EPS * want))
        sh = ((cen[c].astype(np.float64) - cen_old[c].astype(np.float64)) ** 2).sum()
        assert abs(float(shift[0, c]) - sh) <= 1e-4 * max(sh, 1e-30)
    # bit-identical from run to run
    cen2, counts2, inertia2, shift2 = _update_dev(x, off, lab, md, cen_old)
    assert np.array_equal(N(cen2[0]), cen) and torch.equal(inertia2, inertia) and torch.equal(shift2, shift)


# ---- relocate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 3])
def test_relocate_full_iteration(seed):
    """the blob inputs whose first-k initialisation runs into empty centres: the iteration in which the reference meets the event,
    on the device"""
    K, D = 10, 32
    rs = np.random.RandomState(seed)
    x, off = KR.segmented(rs, KR.class_sizes(rs, K), K, D)
    x = x.astype(np.float32)
    C = len(off) - 1
    cen0 = np.zeros((C, K, D), dtype=np.float32)
    event_classes = []
    for c in range(C):
        xc = x[off[c]:off[c + 1]].astype(np.float64)
        k = min(len(xc), K)
        if not k:
            continue
        trace = []
        KR.lloyd(xc, xc[:k].copy(), trace=trace)
        pick = trace[0]
        for cen in trace:
            if (np.bincount(KR.assign(xc, cen)[0], minlength=k) == 0).any():
                pick = cen
                event_classes.append(c)
                break
        cen0[c, :k] = pick.astype(np.float32)
    assert event_classes, 'no empty-cluster event in this input'
    plan, labels, mind2, changed, acount = _assign_dev(x, off, cen0)
    empties = [(N(acount[0, c, :min(off[c + 1] - off[c], K)]) == 0).sum() for c in range(C)]
    assert all(empties[c] > 0 for c in event_classes)
    banded = _check_labels(x, off, cen0, N(labels[0]), N(mind2[0]), tag='relocate seed %d' % seed)
    ops.kmeans_relocate(plan, labels, mind2, acount)
    cen = T(cen0).unsqueeze(0).contiguous()
    counts = torch.zeros(1, C, K, dtype=torch.int32, device=DEV)
    inertia, shift = torch.zeros(1, C, device=DEV), torch.zeros(1, C, device=DEV)
    ops.kmeans_update(T(x), plan, labels, mind2, cen, counts, inertia, shift, acount=acount)
    assert int(acount.abs().sum()) == 0, 'the update clears the counters of the assign'
    lab, checked = N(labels[0]), 0
    for c in range(C):
        a, b = off[c], off[c + 1]
        k = min(b - a, K)
        if not k:
            continue
        xc, cc = x[a:b].astype(np.float64), cen0[c, :k].astype(np.float64)
        rl, rm = KR.assign(xc, cc)
        rl = KR.relocate(rl, rm, k)
        free = ~banded[a:b]
        assert (lab[a:b][free] == rl[free]).all(), c
        assert (N(counts[0, c, :k]) > 0).all(), 'no centre is left without rows'
        if (lab[a:b] == rl).all():
            _check_centers(xc.astype(np.float32), np.array([0, b - a]), rl, N(cen[0, c:c + 1]), cen0[c:c + 1], tag='relocate')
            checked += c in event_classes
    assert checked > 0


# ---- k-means++ -----------------------------------------------------------------------------------------------------------------------
def _pp_rounds(x, off, u, K):
    plan = ops.kmeans_plan(T(off, torch.int32))
    C, D = len(off) - 1, x.shape[1]
    xt, ut = T(x), T(u).reshape(1, C, K).contiguous()
    cen = torch.zeros(1, C, K, D, device=DEV)
    mind2 = torch.zeros(1, plan.P, device=DEV)
    picks = torch.full((1, C, K), -1, dtype=torch.int32, device=DEV)
    snaps = []
    for t in range(K):
        ops.kmeans_pp_step(xt, plan, ut, cen, mind2, picks, t)
        snaps.append(mind2[0].clone())
    return N(picks[0]), [N(s) for s in snaps], N(cen[0])


@pytest.mark.parametrize('K,D,kind', [(10, 32, 'blobs'), (100, 32, 'noise'), (10, 128, 'relu'), (16, 30, 'noise')])
def test_kmeans_pp_rounds(K, D, kind):
    x, off, rs = _data(kind, K, D, seed=300 + K + D, sizes=[0, 1, max(K - 3, 1), K, 700, 2600])
    C = len(off) - 1
    u = bank.draw_uniforms(9, 1, C, K)[0]
    picks, snaps, cen = _pp_rounds(x, off, u, K)
    for c in range(C):
        a, b = off[c], off[c + 1]
        n = b - a
        k = min(n, K)
        x64 = x[a:b].astype(np.float64)
        assert (picks[c, k:] == -1).all()
        if not k:
            continue
        p = picks[c, :k]
        assert ((p >= 0) & (p < n)).all(), 'every pick is a row of its own class'
        assert np.array_equal(cen[c, :k], x[a:b][p]), 'the centre is the picked row'
        assert p[0] == min(int(np.float32(u[c, 0]) * np.float32(n)), n - 1)
        if len(np.unique(x64, axis=0)) >= k:
            assert len(set(p.tolist())) == k, 'distinct rows give distinct picks'
        ref = None
        for t in range(1, k):
            m = snaps[t][a:b].astype(np.float64)
            d = ((x64 - x64[p[t - 1]]) ** 2).sum(1)
            ref = d if ref is None else np.minimum(ref, d)
            tol = 4 * (D + 3) * EPS * ((x64 ** 2).sum(1) + (x64[p[:t]] ** 2).sum(1).max())
            assert (np.abs(m - ref) <= tol).all(), (c, t)
            assert (m[p[:t]] == 0).all(), 'a chosen row is at distance zero'
            cum = np.cumsum(m)
            total = cum[-1]
            bnd = n * EPS * total
            target = float(u[c, t]) * total
            i = p[t]
            assert (cum[i - 1] if i else 0.0) - bnd <= target <= cum[i] + bnd, (c, t, i)
    picks2, _, _ = _pp_rounds(x, off, u, K)
    assert np.array_equal(picks, picks2), 'the same table of uniforms gives the same picks'


# ---- the Lloyd loop ------------------------------------------------------------------------------------------------------------------
def _first_k_init(x, off, K):
    C = len(off) - 1
    init = np.zeros((C, K, x.shape[1]), dtype=np.float32)
    for c in range(C):
        k = min(off[c + 1] - off[c], K)
        init[c, :k] = x[off[c]:off[c] + k]
    return init


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_converged_parity_blobs(seed):
    K, D = 10, 32
    rs = np.random.RandomState(seed)
    x, off = KR.segmented(rs, KR.class_sizes(rs, K), K, D)
    x = x.astype(np.float32)
    init = _first_k_init(x, off, K)
    res = bank.kmeans_segmented(T(x), T(off, torch.int32), K, init=T(init), tol=0.0)
    lab, cen, n_iter, counts, inertia = N(res.labels), N(res.centers), N(res.n_iter), N(res.counts), N(res.inertia)
    assert N(res.k).tolist() == [min(int(n), K) for n in np.diff(off)]
    banded_total = 0
    for c in range(len(off) - 1):
        a, b = off[c], off[c + 1]
        k = min(b - a, K)
        xc = x[a:b].astype(np.float64)
        trace = []
        ref = KR.lloyd(xc, init[c, :k].astype(np.float64), tol=0.0, trace=trace)
        assert n_iter[c] == ref['n_iter'], (c, n_iter[c], ref['n_iter'])
        if not k:
            continue
        inb = np.zeros(b - a, dtype=bool)
        for cc in trace:                                  # union of the per-iteration bands
            _, d1, _, d2 = _two_nearest(xc, cc)
            inb |= (d2 - d1) <= KR.tie_band(xc, cc)
        banded_total += int(inb.sum())
        assert (lab[a:b][~inb] == ref['labels'][~inb]).all(), c
        assert np.array_equal(counts[c], np.bincount(lab[a:b], minlength=K))
        if (lab[a:b] == ref['labels']).all():
            _check_centers(x[a:b], np.array([0, b - a]), ref['labels'], cen[c:c + 1], np.full((1, K, D), np.nan, np.float32),
                           tag='converged')
            assert abs(inertia[c] - ref['inertia']) <= max(1e-4 * ref['inertia'], 1e-30)
    assert banded_total <= 0.01 * len(x)


@pytest.mark.parametrize('kind,K,D', [('noise', 100, 32), ('relu', 10, 32), ('noise', 10, 128)])
def test_fixed_point_hard_data(kind, K, D):
    """k-means++ and Lloyd to the end on data without structure: one fp64 step from the returned centres changes no label outside
    the tie band.  (No quality threshold: fp32 and fp64 trajectories of 10+ iterations may end in different optima.)"""
    x, off, _ = _data(kind, K, D, seed=4242 + K, sizes=[0, 1, max(K - 3, 1), K, 1500, 5000])
    res = bank.kmeans_segmented(T(x), T(off, torch.int32), K, seed=3)
    lab, cen, n_iter = N(res.labels), N(res.centers), N(res.n_iter)
    _check_labels(x, off, cen, lab, tag='fixed point %s' % kind)
    sizes = np.diff(off)
    assert (n_iter[sizes > 0] >= 1).all() and (n_iter <= 300).all() and n_iter[sizes == 0].tolist() == [0]
    _record('fixed point: most iterations of a class', n_iter.max())
    for c in range(len(sizes)):
        assert np.array_equal(N(res.counts[c]), np.bincount(lab[off[c]:off[c + 1]], minlength=K))
    assert res.host_reads <= math.ceil(res.iterations_issued / bank.HOST_STRIDE)


def _same(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ('centers', 'labels', 'inertia', 'n_iter', 'counts'))


def test_determinism_and_independence_of_the_other_classes():
    K, D = 10, 32
    x, off, rs = _data('relu', K, D, seed=99, sizes=[40, 0, 2500, 7, 1300, 1])
    C = len(off) - 1
    u = bank.draw_uniforms(5, 3, C, K)
    xt, ot = T(x), T(off, torch.int32)
    a = bank.kmeans_segmented(xt, ot, K, u=u[:1])
    b = bank.kmeans_segmented(xt, ot, K, u=u[:1])
    assert _same(a, b), 'two runs are bit-identical'
    assert _same(a, bank.kmeans_segmented(xt, ot, K, seed=5)), 'u defaults to the table of the seed'
    # the classes in another order
    perm = [4, 2, 5, 0, 3, 1]
    xp = np.concatenate([x[off[c]:off[c + 1]] for c in perm], 0)
    offp = np.concatenate([[0], np.cumsum([off[c + 1] - off[c] for c in perm])])
    p = bank.kmeans_segmented(T(xp), T(offp, torch.int32), K, u=u[:1, perm])
    for i, c in enumerate(perm):
        assert torch.equal(p.centers[i], a.centers[c]) and torch.equal(p.inertia[i], a.inertia[c])
        assert torch.equal(p.n_iter[i], a.n_iter[c]) and torch.equal(p.counts[i], a.counts[c])
        assert torch.equal(p.labels[offp[i]:offp[i + 1]], a.labels[off[c]:off[c + 1]])
    # a class on its own
    for c in (2, 3):
        s = bank.kmeans_segmented(T(x[off[c]:off[c + 1]]), T(np.array([0, off[c + 1] - off[c]]), torch.int32), K, u=u[:1, c:c + 1])
        assert torch.equal(s.centers[0], a.centers[c]) and torch.equal(s.labels, a.labels[off[c]:off[c + 1]])
        assert torch.equal(s.inertia[0], a.inertia[c]) and torch.equal(s.n_iter[0], a.n_iter[c])
    # n_init = 3 against three separate runs with the same rows of u
    multi = bank.kmeans_segmented(xt, ot, K, n_init=3, u=u)
    singles = [bank.kmeans_segmented(xt, ot, K, u=u[r:r + 1]) for r in range(3)]
    inert = torch.stack([s.inertia for s in singles])
    assert torch.equal(multi.inertia, inert.min(0).values)
    for c in range(C):
        r = int(np.argmin(N(inert[:, c])))                # numpy: the first of equals
        assert torch.equal(multi.centers[c], singles[r].centers[c]) and torch.equal(multi.n_iter[c], singles[r].n_iter[c])
        assert torch.equal(multi.labels[off[c]:off[c + 1]], singles[r].labels[off[c]:off[c + 1]])
        assert torch.equal(multi.counts[c], singles[r].counts[c])
    assert _same(multi, bank.kmeans_segmented(xt, ot, K, n_init=3, seed=5))


def test_k_equals_one():
    x, off, _ = _data('relu', 1, 32, seed=8, sizes=[0, 1, 5, 3000, 1025])
    res = bank.kmeans_segmented(T(x), T(off, torch.int32), 1)
    sizes = np.diff(off)
    assert N(res.n_iter).tolist() == [0, 1, 1, 1, 1], 'one centre: the first update is the answer'
    lab = np.zeros(len(x), dtype=np.int64)
    assert np.array_equal(N(res.labels), lab)
    _check_centers(x, off, lab, N(res.centers), np.full((len(sizes), 1, 32), np.nan, np.float32), tag='k=1')
    for c in range(len(sizes)):
        xc = x[off[c]:off[c + 1]].astype(np.float64)
        want = ((xc - xc.mean(0)) ** 2).sum() if len(xc) else 0.0
        assert abs(float(res.inertia[c]) - want) <= 1e-4 * want + 1e-30


# ---- the bank ------------------------------------------------------------------------------------------------------------------------
KW = dict(image_size=(32, 32), gconv_hidden_dim=32, gconv_num_layers=2, mask_size=8, n_downsample_global=1,
          appearance_normalization='batch', activation='leakyrelu-0.2', use_attributes=True, pool_size=2, rep_size=8)


def _eval_model(vocab=None):
    m = Model(vocab or make_vocab(12, 4, 35), **KW).to(DEV)
    fill_deterministic(m)
    m.eval()
    return m


def test_bank_encode_equals_encode_features():
    """the model, vocabulary and batch of test_eval_hooks_feature_bank_and_check_model"""
    from scene_generation_amd.evaluate import encode_features
    m = _eval_model()
    b = make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=12, num_preds=4, seed=33)
    b2 = make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=12, num_preds=4, seed=34)
    for loader in ([b], [b, b2]):
        want = encode_features(m, loader, object_size=64)
        x, offsets = bank.encode(m, loader, object_size=64)
        assert x.dtype == torch.float32 and x.is_cuda and offsets.dtype == torch.int32 and offsets.is_cuda
        hist = np.bincount(np.concatenate([N(d.objs) for d in loader]), minlength=12)
        assert np.array_equal(N(offsets), np.concatenate([[0], np.cumsum(hist)]))
        off = N(offsets)
        for c in range(12):
            assert torch.equal(x[off[c]:off[c + 1]].cpu(), torch.from_numpy(want[c].astype(np.float32))), c
    x3, _ = bank.encode(m, [b, b2], object_size=64, max_objects=1)
    assert x3.size(0) == b.objs.numel()


def _checkpoint(tmp_path):
    vocab = make_sampling_vocab(12, 4, 35)
    m = _eval_model(vocab)
    path = str(tmp_path / 'ckpt.pt')
    torch.save({'model_kwargs': dict(vocab=vocab, **KW), 'model_state': m.state_dict()}, path)
    return path


def test_train_bank_sample_end_to_end(tmp_path):
    path = _checkpoint(tmp_path)
    out = str(tmp_path / 'pictures')
    sample_argv = ['--checkpoint', path, '--output_dir', out, '--batch_size', '8', '--num_samples', '8', '--use_gt_textures', '0']
    with pytest.raises(ValueError, match='No features file'):
        sample.main(sample_argv)
    res = bank.main(['--checkpoint', path, '--batch_size', '8', '--num_samples', '64'])
    names = ['features.npy', 'features_clustered_100.npy', 'features_clustered_010.npy', 'features_clustered_001.npy']
    assert sorted(os.path.basename(p) for p in res['paths']) == sorted(names)
    files = {n: np.load(str(tmp_path / n), allow_pickle=True).item() for n in names}
    feats = files['features.npy']
    assert sorted(feats) == list(range(12)) and all(v.dtype == np.float64 and v.shape[1] == 8 for v in feats.values())
    live = sorted(c for c, v in feats.items() if v.shape[0])
    assert len(live) >= 6 and sum(v.shape[0] for v in feats.values()) > 200
    for n, k in zip(names[1:], (100, 10, 1)):
        d = files[n]
        assert sorted(d) == live
        for c in live:
            assert d[c].dtype == np.float64 and d[c].shape == (min(feats[c].shape[0], k), 8) and np.isfinite(d[c]).all()
    for c in live:                                       # k = 1: the class mean
        assert np.abs(files[names[3]][c][0] - feats[c].mean(0)).max() <= 1e-5 * (1 + np.abs(feats[c]).max())
    assert [r['k'] for r in res['report']] == [100, 10, 1] and all(r['classes'] == len(live) for r in res['report'])
    # the same sampling call now finds its bank
    got = sample.main(sample_argv)
    assert len(got['paths']) == 8 and all(os.path.isfile(p) for p in got['paths'])
    # scene graphs with --bank: feature number -1 -> row 0 of the _001 file, 3 -> row 3 of the _100 file
    rich = [c for c in live if c and files[names[1]][c].shape[0] >= 4][:2]
    assert len(rich) == 2
    graph = {'objects': ['obj%d' % rich[0], 'obj%d' % rich[1]], 'relationships': [[0, 'left of', 1]], 'features': [-1, 3]}
    gpath = str(tmp_path / 'graphs.json')
    with open(gpath, 'w') as f:
        json.dump([graph], f)
    args = sample.make_parser().parse_args(['--checkpoint', path])
    m = sample.build_model(args, torch.load(path, map_location='cpu', weights_only=False), DEV)
    m.features, m.features_one = sample.load_bank(str(tmp_path))
    objs, _, _, _, fts = m.encode_scene_graphs(sample.load_scene_graphs(gpath))
    assert objs.tolist() == [rich[0], rich[1], 0]
    assert np.array_equal(N(fts[0]), files[names[3]][rich[0]][0].astype(np.float32))
    assert np.array_equal(N(fts[1]), files[names[1]][rich[1]][3].astype(np.float32))
    assert np.array_equal(N(fts[2]), files[names[3]][0][0].astype(np.float32))
    out2 = str(tmp_path / 'from_graphs')
    got = sample.main(['--checkpoint', path, '--output_dir', out2, '--scene_graphs', gpath, '--bank', str(tmp_path)])
    assert len(got['paths']) == 1 and os.path.isfile(got['paths'][0])


def _kinds(prof):
    return {k for k, v in prof.items() if v['launches'] > 0}


def test_bank_build_launch_profile():
    """the launches of a bank build: the crop / encoder / MLP kernels of the encode, then nothing but the k-means kernels; the
    convergence flags are read at most once per HOST_STRIDE iterations"""
    m = _eval_model()
    loader = [make_batch(N=8, size=32, mask_size=8, num_objs=12, num_preds=4, seed=50 + i) for i in range(6)]
    bank.build_bank(m, loader, n_clusters=(10, 1))                      # warm-up outside the profile
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        x, offsets = bank.encode(m, loader)
        enc = ops.prof_read()
        ops.prof_reset()
        res = bank.kmeans_segmented(x, offsets, 10, seed=1)
        km = ops.prof_read()
        ops.prof_reset()
        report = []
        bank.build_bank(m, loader, n_clusters=(10, 1), seed=1, report=report)
        whole = ops.prof_read()
    finally:
        ops.prof_enable(False)
    assert _kinds(enc) and not (_kinds(enc) & KM_KINDS)
    assert _kinds(km) == KM_KINDS, 'between the seeding and the last Lloyd iteration only the k-means kernels run'
    it = res.iterations_issued
    assert it >= int(res.n_iter.max()) and it % bank.HOST_STRIDE == 0 or it == 300
    assert km['kmeans_pp']['launches'] == 10 and km['kmeans_relocate']['launches'] == it
    assert km['kmeans_assign']['launches'] == it + 2 and km['kmeans_update']['launches'] == it + 3    # + final pass, + tolerance
    assert res.host_reads == it // bank.HOST_STRIDE, 'one read of the flags per HOST_STRIDE iterations, none in between'
    assert _kinds(whole) == _kinds(enc) | KM_KINDS
    for k in _kinds(enc):
        assert whole[k]['launches'] == enc[k]['launches'], k
    assert [r['k'] for r in report] == [10, 1] and report[0]['host_reads'] == res.host_reads


def test_write_parity_record():
    """the largest observed errors of the tests above -> kmeans_parity.json in the suite's output directory (a record, not a check)"""
    assert PARITY
    _dump('kmeans_parity.json', PARITY)
