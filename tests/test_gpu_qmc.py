"""Quasi-random inputs on the GPU (csrc/qmc.hip, ops/qmc.py, scene_generation_amd/qmc.py, the model's and the sampler's opt-in paths).

* ``sg_sobol_points``: ``torch.equal`` to the restatement of tests/qmc_ref.py (pinned to torch's SobolEngine by test_qmc_cpu.py) for
  n in {1, 2, 63, 64, 65, 257}, D in {1, 3, 70, 160}, ld = D and D + 3, first in {0, 1, 2^20 - 3, 2^30 - n}, scrambled and plain
  tables, between guard words, the padding columns untouched; every negative code with ``out`` still poisoned; two draws of a stream
  equal one draw of the sum; the (0, 6, D)-net property of the first two blocks of 64 scrambled points, in integers.
* ``sg_qmc_unpack``: pick and u exact; noise within ONE float32 ulp of float32(scipy.special.ndtri(cell centre)) -- derived, not
  measured: the fp64 inverse is accurate far below half a float32 ulp, so its rounding is the reference's float32 or its
  neighbour.  The share of exact matches goes to qmc_margins.json in the suite's output directory.
* ``sg_bank_draw``: row_idx exact and rows ``torch.equal`` to the bank's, classes of 1, 3, 100 and no rows, rep = 32 (16-byte copies),
  6 (8-byte), 5 and a misaligned base (4-byte), classes outside the table and pick = -1, between guard words.
* the model's per-image noise and tensor features, the sampler with ``quasi_random`` and the command line.
The tree only: no reference checkout."""
import os
import random

import numpy as np
import pytest
import torch

import qmc_ref as R
import sampling_helpers as SH
from gpu_harness import _dump, _guarded, margins_fixture
from scene_generation_amd import _hip, attributes, ops, qmc, sample, scenegraph
from scene_generation_amd.model import Model
from scene_generation_amd.synthetic import batch_to, make_batch, make_sampling_vocab

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POISON = -777
G = 16                                      # guard words on each side
MARGINS = {}
_write_margins = margins_fixture(lambda: MARGINS and _dump('qmc_margins.json', MARGINS))
_TABLES = {}
E = {k: _hip.CONST['SG_QMC_ERR_' + k] for k in ('NULL', 'DIMS', 'LD', 'RANGE', 'COUNT')}


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _tables(D, scramble, seed=5):
    """(dirs, shift) int64 on the host and int32 on the device, once per case"""
    key = (D, scramble, seed)
    if key not in _TABLES:
        dirs, shift = R.tables(D, scramble, seed)
        _TABLES[key] = (dirs, shift, T(dirs, torch.int32), T(shift, torch.int32))
    return _TABLES[key]


def _raw(name, **a):
    """the entry point itself -> its return code"""
    a.setdefault('stream', ops._stream())
    return getattr(_hip.lib(), name)(*[a[k] for k in _hip.PROTOS[name][2]])


# =====================================================================================================================================
# 1. the points
# =====================================================================================================================================
@pytest.mark.parametrize('scramble', [False, True], ids=['plain', 'scrambled'])
@pytest.mark.parametrize('D', [1, 3, 70, 160])
def test_sobol_points_equal_the_restatement(D, scramble):
    dirs, shift, ddirs, dshift = _tables(D, scramble)
    for n in (1, 2, 63, 64, 65, 257):
        for first in (0, 1, 2 ** 20 - 3, 2 ** 30 - n):
            want = R.points(dirs, shift, first, n)
            for ld in (D, D + 3):
                buf, out = _guarded((n, ld), torch.int32, POISON, G)
                assert _raw('sg_sobol_points', dirs=ddirs.data_ptr(), shift=dshift.data_ptr(), out=out.data_ptr(), first=first, n=n, D=D,
                            ld=ld) == 0
                expect = np.full((n, ld), POISON, np.int64)
                expect[:, :D] = want
                expect = np.concatenate([np.full(G, POISON), expect.ravel(), np.full(G, POISON)])
                assert torch.equal(buf.cpu(), torch.from_numpy(expect).to(torch.int32)), (n, first, ld)       # values, padding, guards
            got = ops.sg_sobol_points(ddirs, dshift, first, n, ld=D + 3)                # the wrapper: a fresh tensor, a view when padded
            assert got.dtype == torch.int32 and tuple(got.shape) == (n, D) and got.stride(0) == D + 3
            assert torch.equal(got.cpu(), torch.from_numpy(want).to(torch.int32))
    assert tuple(ops.sg_sobol_points(ddirs, dshift, 7, 0).shape) == (0, D)


def test_sobol_points_negative_codes_write_nothing():
    D = 3
    _, _, ddirs, dshift = _tables(D, True)
    buf, out = _guarded((4, D), torch.int32, POISON, G)
    good = dict(dirs=ddirs.data_ptr(), shift=dshift.data_ptr(), out=out.data_ptr(), first=0, n=4, D=D, ld=D)
    seen = set()
    for kw, code in ((dict(dirs=None), 'NULL'), (dict(shift=None), 'NULL'), (dict(out=None), 'NULL'), (dict(D=0), 'DIMS'),
                     (dict(D=_hip.CONST['SG_QMC_MAX_DIMS'] + 1, ld=1 << 20), 'DIMS'), (dict(ld=D - 1), 'LD'), (dict(first=-1), 'RANGE'),
                     (dict(first=2 ** 30 - 3), 'RANGE'), (dict(first=2 ** 30 + 1, n=0), 'RANGE'), (dict(n=-1), 'COUNT')):
        assert _raw('sg_sobol_points', **dict(good, **kw)) == E[code] and 'sg_sobol_points' in _hip.last_error(), kw
        seen.add(E[code])
    assert len(seen) == 5 and all(c < 0 for c in seen)
    assert _raw('sg_sobol_points', **dict(good, n=0, dirs=None, shift=None, out=None)) == 0            # nothing to write: success
    torch.cuda.synchronize()
    assert (buf == POISON).all().item()
    for bad, match in ((dict(dirs=ddirs.to(torch.int64)), 'dirs must be int32'), (dict(dirs=ddirs[:, :29].contiguous()), r'dirs must be \[\*, 30\]'),
                       (dict(dirs=ddirs.t().contiguous().t()), 'dirs must be contiguous'), (dict(shift=dshift[:2]), r'shift must be \[3\]'),
                       (dict(shift=dshift.cpu()), 'shift is on cpu'), (dict(first=-1), 'first and n'), (dict(n=-1), 'first and n'),
                       (dict(first=2 ** 30, n=1), 'first and n'), (dict(ld=2), 'ld = 2')):
        a = dict(dirs=ddirs, shift=dshift, first=0, n=4, ld=None)
        a.update(bad)
        with pytest.raises(ValueError, match=match):
            ops.sg_sobol_points(a['dirs'], a['shift'], a['first'], a['n'], ld=a['ld'])


@pytest.mark.parametrize('scramble', [False, True], ids=['plain', 'scrambled'])
def test_stream_draws_are_a_cut_of_one_sequence(scramble):
    dirs, shift, _, _ = _tables(70, scramble, 11)
    s = qmc.SobolStream(70, scramble=scramble, seed=11, device=DEV)
    a, b = s.draw(37), s.draw(220)
    assert s.position == 257 and a.dtype == torch.int32 and a.is_cuda and tuple(b.shape) == (220, 70)
    whole = s.reset().draw(257)
    assert torch.equal(torch.cat([a, b]), whole) and torch.equal(whole.cpu(), torch.from_numpy(R.points(dirs, shift, 0, 257)).to(torch.int32))
    assert tuple(s.draw(0).shape) == (0, 70) and s.position == 257
    s.reset().fast_forward(2 ** 20 - 3)
    assert torch.equal(s.draw(9).cpu(), torch.from_numpy(R.points(dirs, shift, 2 ** 20 - 3, 9)).to(torch.int32)) and s.position == 2 ** 20 + 6
    s.reset().fast_forward(2 ** 30 - 2)
    assert tuple(s.draw(2).shape) == (2, 70)                            # the last two points
    with pytest.raises(ValueError, match='leaves the sequence'):
        s.draw(1)


def test_net_property_on_the_device():
    """a scrambled Sobol sequence is a (0, m, 1)-net in base 2 in every coordinate: the top 6 bits of points [64 b, 64 b + 64) are
    a permutation of 0..63 -- exact, in integers, computed on the device"""
    s = qmc.SobolStream(160, scramble=True, seed=3, device=DEV)
    x = s.draw(128)
    want = torch.arange(64, dtype=torch.int32, device=DEV).view(64, 1).expand(64, 160)
    for b in range(2):
        top = x[64 * b:64 * b + 64] >> 24
        assert torch.equal(torch.sort(top, dim=0)[0], want), b


# =====================================================================================================================================
# 2. the unpacking
# =====================================================================================================================================
def _within_one_ulp(got, want64, name, case):
    """got (fp32) is float32(want64) or one of its two neighbours; records the share of exact matches"""
    ref = want64.astype(np.float32)
    lo, hi = np.nextafter(ref, np.float32(-np.inf)), np.nextafter(ref, np.float32(np.inf))
    assert np.isfinite(got).all() and ((got >= lo) & (got <= hi)).all(), case
    share = float((got == ref).mean())
    print('%s %s: %d values, %.4f of them the reference\'s float32 itself' % (name, case, got.size, share))
    if share < MARGINS.get(name, {'share_exact': 2.0})['share_exact']:
        MARGINS[name] = {'share_exact': share, 'case': case, 'values': int(got.size), 'bound_ulp': 1}


COUNTS = (0, 1, 2, 4, 3)                     # objects per image; max_objects = 4


@pytest.mark.parametrize('pad', [0, 3], ids=['tight', 'padded'])
def test_unpack_equals_the_restatement(pad):
    noise_dim, J, N = 64, 4, 5
    D = noise_dim + 3 * J
    _, _, ddirs, dshift = _tables(D, True, 21)
    pts = ops.sg_sobol_points(ddirs, dshift, 1000, N, ld=D + pad)
    o2i_h = [n for n, k in enumerate(COUNTS) for _ in range(k)]
    o2i = T(np.array(o2i_h, np.int64))
    seg = ops.segment_offsets(o2i, N)
    noise, pick, u = ops.sg_qmc_unpack(pts, o2i, seg, noise_dim, J)
    assert noise.dtype == torch.float32 and pick.dtype == torch.int32 and u.dtype == torch.float32
    assert tuple(noise.shape) == (N, noise_dim) and tuple(pick.shape) == (10,) and tuple(u.shape) == (10, 2)
    wn, wp, wu = R.unpack(pts.cpu().numpy(), o2i_h, noise_dim, J)
    assert (wp >= 0).all() and np.array_equal(pick.cpu().numpy(), wp)
    assert np.array_equal(u.cpu().numpy().astype(np.float64), wu) and (u < 1).all().item() and (u >= 0).all().item()
    _within_one_ulp(noise.cpu().numpy(), wn, 'noise', 'batch_pad%d' % pad)
    again = ops.sg_qmc_unpack(pts, o2i, seg, noise_dim, J)
    assert all(torch.equal(a, b) for a, b in zip(again, (noise, pick, u)))              # the same call, the same bits


def test_unpack_noise_over_many_points_and_the_extremes():
    _, _, ddirs, dshift = _tables(160, True, 21)
    pts = ops.sg_sobol_points(ddirs, dshift, 0, 257)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    seg = lambda N: torch.zeros(N + 1, dtype=torch.int32, device=DEV)       # no objects: every image's segment is empty
    noise, pick, u = ops.sg_qmc_unpack(pts, none, seg(257), 160, 0)
    assert pick.numel() == 0 and tuple(u.shape) == (0, 2)
    _within_one_ulp(noise.cpu().numpy(), R.unpack(pts.cpu().numpy(), [], 160, 0)[0], 'noise', '257x160')
    # hand-made points: the first and the last cell, the two around 1/2
    hand = T(np.array([[0, 2 ** 30 - 1, 2 ** 29 - 1, 2 ** 29]], np.int32))
    noise = ops.sg_qmc_unpack(hand, none, seg(1), 4, 0)[0].cpu().numpy()
    assert np.isfinite(noise).all() and abs(noise[0, 0] + 6.1208) < 1e-4 and abs(noise[0, 1] - 6.1208) < 1e-4
    assert -2e-9 < noise[0, 2] < 0 < noise[0, 3] < 2e-9
    _within_one_ulp(noise, R.unpack(hand.cpu().numpy(), [], 4, 0)[0], 'noise', 'extremes')


def test_unpack_object_limit_and_bad_arguments():
    noise_dim, J = 6, 4
    q = qmc.QuasiRandomInputs(noise_dim, max_objects=J, seed=2, device=DEV)
    o2i_h = [0, 0, 0, 0, 0, 1]                                  # image 0: max_objects + 1 objects
    o2i = T(np.array(o2i_h, np.int64))
    seg = ops.segment_offsets(o2i, 2)
    with pytest.raises(ValueError, match='image 0 has more than 4 objects'):
        q.draw(o2i, seg, 2, obj_to_img_host=o2i_h)
    assert q.position == 0                                      # raised before the draw
    noise, pick, u = q.draw(o2i, seg, 2)                        # no host list: the object past the limit reads as "no draw"
    assert q.position == 2
    pts = R.points(*R.tables(q.dimension, True, 2), 0, 2)
    wn, wp, wu = R.unpack(pts, o2i_h, noise_dim, J)
    assert wp[4] == -1 and (wp[[0, 1, 2, 3, 5]] >= 0).all() and np.array_equal(pick.cpu().numpy(), wp)
    assert np.array_equal(u.cpu().numpy().astype(np.float64), wu) and not wu[4].any()
    # an object of no image of the call
    far = T(np.array([0, 1, 7], np.int64))
    p2 = ops.sg_qmc_unpack(T(pts, torch.int32), far, ops.segment_offsets(far[:2], 2), noise_dim, J)[1]
    assert p2[2].item() == -1 and p2[0].item() == wp[0]
    # every negative code, the outputs still poisoned
    dp = T(pts, torch.int32)
    nb, nz = _guarded((2, noise_dim), torch.float32, POISON, G)
    pb, pk = _guarded((6,), torch.int32, POISON, G)
    ub, uu = _guarded((6, 2), torch.float32, POISON, G)
    good = dict(points=dp.data_ptr(), ld=q.dimension, obj_to_img=o2i.data_ptr(), seg_off=seg.data_ptr(), noise=nz.data_ptr(),
                pick=pk.data_ptr(), u=uu.data_ptr(), N=2, O=6, noise_dim=noise_dim, max_objects=J)
    for kw, code in ((dict(points=None), 'NULL'), (dict(obj_to_img=None), 'NULL'), (dict(seg_off=None), 'NULL'), (dict(noise=None), 'NULL'),
                     (dict(pick=None), 'NULL'), (dict(u=None), 'NULL'), (dict(noise_dim=-1), 'DIMS'), (dict(max_objects=-1), 'DIMS'),
                     (dict(noise_dim=0, max_objects=0), 'DIMS'), (dict(ld=q.dimension - 1), 'LD'), (dict(N=-1), 'COUNT'), (dict(O=-1), 'COUNT')):
        assert _raw('sg_qmc_unpack', **dict(good, **kw)) == E[code] and 'sg_qmc_unpack' in _hip.last_error(), kw
    torch.cuda.synchronize()
    assert all((b == POISON).all().item() for b in (nb, pb, ub))
    assert _raw('sg_qmc_unpack', **good) == 0                   # and the call itself between the guards
    assert all((b[:G] == POISON).all().item() and (b[-G:] == POISON).all().item() for b in (nb, pb, ub))
    assert torch.equal(pk, pick) and torch.equal(uu, u) and torch.equal(nz, noise)
    for bad, match in ((dict(points=dp.to(torch.int64)), 'points must be int32'), (dict(points=dp[:, :17]), 'points has 17 columns'),
                       (dict(points=dp.t().contiguous().t()), 'contiguous rows'), (dict(obj_to_img=o2i.to(torch.int32)), 'obj_to_img must be int64'),
                       (dict(seg_off=seg[:2]), r'seg_off must be \[3\]'), (dict(seg_off=seg.to(torch.int64)), 'seg_off must be int32'),
                       (dict(obj_to_img=o2i.cpu()), 'obj_to_img is on cpu'), (dict(max_objects=-1), 'max_objects = -1')):
        a = dict(points=dp, obj_to_img=o2i, seg_off=seg, noise_dim=noise_dim, max_objects=J)
        a.update(bad)
        with pytest.raises(ValueError, match=match):
            ops.sg_qmc_unpack(a['points'], a['obj_to_img'], a['seg_off'], a['noise_dim'], a['max_objects'])


# =====================================================================================================================================
# 3. the bank draw
# =====================================================================================================================================
# (rep, floats the outputs' and the bank's base is moved by): 16-byte, 8-byte and 4-byte copies, the last also from a base no wider load could take
@pytest.mark.parametrize('rep,off', [(32, 0), (6, 0), (5, 0), (32, 1)], ids=lambda v: str(v))
def test_bank_draw_equals_the_restatement(rep, off):
    rs = np.random.RandomState(rep + off)
    feats = {1: rs.rand(1, rep), 2: rs.rand(3, rep), 4: rs.rand(100, rep)}          # classes 0 and 3: no rows
    b = qmc.DeviceBank.from_dict(feats, 5, DEV)
    assert b.class_off.tolist() == [0, 0, 1, 4, 4, 104] and b.rep == rep
    bank = b.bank
    if off:                                                     # the same rows from a base that is only 4-byte aligned
        moved = torch.empty(bank.numel() + off, dtype=torch.float32, device=DEV)
        bank = moved[off:].view_as(bank).copy_(b.bank)
        assert bank.data_ptr() % 8 == 4
    picks = [0, 2 ** 30 - 1] + rs.randint(0, 2 ** 30, size=6).tolist()
    objs = [c for c in (1, 2, 4) for _ in picks] + [0, 3, -1, 5, 1 << 40, 4, 2]
    pick = picks * 3 + [5, 5, 5, 5, 5, -1, -1]
    O = len(objs)
    want_rows, want_idx = R.bank_draw(bank.cpu().numpy(), b.class_off.cpu().numpy(), objs, pick)
    assert want_idx[:8].tolist() == [0] * 8 and want_idx[8:10].tolist() == [0, 2] and want_idx[16:18].tolist() == [0, 99]
    assert (want_idx[-7:] == -1).all() and not want_rows[-7:].any() and (want_idx[:-7] >= 0).all()
    dobjs, dpick = T(np.array(objs, np.int64)), T(np.array(pick, np.int32))
    rbuf = torch.full((O * rep + 2 * G + off,), float(POISON), dtype=torch.float32, device=DEV)
    rows = rbuf[G + off:G + off + O * rep].view(O, rep)
    ibuf, idx = _guarded((O,), torch.int32, POISON, G)
    assert _raw('sg_bank_draw', bank=bank.data_ptr(), class_off=b.class_off.data_ptr(), objs=dobjs.data_ptr(), pick=dpick.data_ptr(),
                row_idx=idx.data_ptr(), rows=rows.data_ptr(), O=O, C=5, rep=rep, R=104) == 0
    assert np.array_equal(idx.cpu().numpy(), want_idx) and torch.equal(rows.cpu(), torch.from_numpy(want_rows))
    assert (ibuf[:G] == POISON).all().item() and (ibuf[-G:] == POISON).all().item()
    assert (rbuf[:G + off] == POISON).all().item() and (rbuf[-G:] == POISON).all().item()
    got_rows, got_idx = b.draw(dobjs, dpick)                    # the public call: fresh tensors, the same values
    assert torch.equal(got_rows, rows) and torch.equal(got_idx, idx) and got_rows.data_ptr() != rows.data_ptr()
    sel = got_idx >= 0
    assert torch.equal(got_rows[sel], b.bank[(b.class_off[dobjs[sel]] + got_idx[sel])])
    with pytest.raises(ValueError, match='No features for class 0'):
        b.draw(dobjs, dpick, objs_host=[c if abs(c) < 100 else 99 for c in objs])
    ok = [1, 2, 4, 4]
    r4, i4 = b.draw(T(np.array(ok, np.int64)), T(np.array([7, 2 ** 29, 0, 2 ** 30 - 1], np.int32)), objs_host=ok)
    assert i4.tolist() == [0, 1, 0, 99] and torch.equal(r4[3], b.bank[103])
    # a table that points past the bank forms no address
    short = dict(bank=bank.data_ptr(), class_off=b.class_off.data_ptr(), objs=dobjs.data_ptr(), pick=dpick.data_ptr(), row_idx=idx.data_ptr(),
                 rows=rows.data_ptr(), O=O, C=5, rep=rep, R=4)
    assert _raw('sg_bank_draw', **short) == 0
    assert (idx[16:24] == -1).all().item() and not rows[16:24].any().item() and np.array_equal(idx[:16].cpu().numpy(), want_idx[:16])


def test_bank_draw_negative_codes_and_bad_arguments():
    b = qmc.DeviceBank.from_dict({0: np.ones((2, 4)), 1: np.ones((3, 4))}, 2, DEV)
    objs, pick = T(np.array([0, 1, 1], np.int64)), T(np.array([1, 2, 3], np.int32))
    rbuf, rows = _guarded((3, 4), torch.float32, POISON, G)
    ibuf, idx = _guarded((3,), torch.int32, POISON, G)
    good = dict(bank=b.bank.data_ptr(), class_off=b.class_off.data_ptr(), objs=objs.data_ptr(), pick=pick.data_ptr(), row_idx=idx.data_ptr(),
                rows=rows.data_ptr(), O=3, C=2, rep=4, R=5)
    for kw, code in ((dict(bank=None), 'NULL'), (dict(class_off=None), 'NULL'), (dict(objs=None), 'NULL'), (dict(pick=None), 'NULL'),
                     (dict(row_idx=None), 'NULL'), (dict(rows=None), 'NULL'), (dict(C=0), 'DIMS'), (dict(rep=0), 'DIMS'), (dict(O=-1), 'COUNT'),
                     (dict(R=-1), 'COUNT')):
        assert _raw('sg_bank_draw', **dict(good, **kw)) == E[code] and 'sg_bank_draw' in _hip.last_error(), kw
    assert _raw('sg_bank_draw', **dict(good, O=0, objs=None, pick=None, row_idx=None, rows=None)) == 0
    torch.cuda.synchronize()
    assert (rbuf == POISON).all().item() and (ibuf == POISON).all().item()
    for bad, match in ((dict(bank=b.bank.double()), 'bank must be float32'), (dict(bank=b.bank[0]), r'bank must be \[\*, \*\]'),
                       (dict(bank=b.bank[:, :2]), 'bank must be contiguous'), (dict(class_off=b.class_off.to(torch.int32)), 'class_off must be int64'),
                       (dict(class_off=b.class_off[:1]), 'C \\+ 1 >= 2'), (dict(objs=objs.to(torch.int32)), 'objs must be int64'),
                       (dict(pick=pick.to(torch.int64)), 'pick must be int32'), (dict(pick=pick[:2]), r'pick must be \[3\]'),
                       (dict(objs=objs.cpu()), 'objs is on cpu')):
        a = dict(bank=b.bank, class_off=b.class_off, objs=objs, pick=pick)
        a.update(bad)
        with pytest.raises(ValueError, match=match):
            ops.sg_bank_draw(a['bank'], a['class_off'], a['objs'], a['pick'])


# =====================================================================================================================================
# 4. the model
# =====================================================================================================================================
def _model():
    m = SH.small_model(Model, make_sampling_vocab(SH.C, 7, SH.A)).to(DEV)
    m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    return m


def _batch(seed=321):
    b = make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=SH.C, num_preds=7, num_attributes=35, seed=seed)
    return scenegraph.regraph(b, seed=1)


def _stats():
    rs = np.random.RandomState(8)
    counts = rs.randint(0, 30, size=(SH.C, 35)).astype(np.int64)
    counts[0] = 0
    return attributes.AttributeStats(SH.C, device=DEV, counts=counts)


def _run(m, dev, features, seed=0):
    """a test-mode forward on predicted boxes and masks -> its tensors (the draws of ``random`` pinned)"""
    random.seed(seed)
    with torch.no_grad():
        out = m(dev.imgs, dev.objs, dev.triples, dev.obj_to_img, attributes=dev.attributes, test_mode=True, features=features)
    return [t for t in out if t is not None]


def _bank_rows(dev, seed=4):
    many = SH.make_banks()[0]
    rs = np.random.RandomState(seed)
    return np.stack([many[c][rs.randint(0, 100)] for c in dev.objs.tolist()]).astype(np.float32)


def test_model_noise_one_row_per_image():
    m = _model()
    dev = batch_to(_batch(), DEV)
    O, N = dev.objs.numel(), 3
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(N, 64, generator=g).to(DEV)
    obj_vecs = torch.randn(O, 128, generator=g).to(DEV)
    row = m.noise_override.to(DEV)
    parent = ops.concat_cols(obj_vecs, row.expand(O, 64))       # what _mask_vecs was before it knew obj_to_img
    assert torch.equal(m._mask_vecs(obj_vecs, O, dev.obj_to_img), parent) and torch.equal(m._mask_vecs(obj_vecs, O), parent)
    m.noise_override = noise
    got = m._mask_vecs(obj_vecs, O, dev.obj_to_img)
    assert torch.equal(got[:, 128:], noise[dev.obj_to_img]) and torch.equal(got[:, :128], obj_vecs)
    with pytest.raises(ValueError, match='needs obj_to_img'):
        m._mask_vecs(obj_vecs, O)
    # the whole forward: N copies of one row are that row
    feats = list(torch.from_numpy(_bank_rows(dev)).to(DEV).unbind(0))
    m.noise_override = row.cpu()
    one = _run(m, dev, feats)
    m.noise_override = row.expand(N, 64).contiguous()
    many = _run(m, dev, feats)
    assert len(one) == len(many) >= 4 and all(torch.equal(a, b) for a, b in zip(one, many))
    m.noise_override = noise                                    # and different rows give another picture
    assert not torch.equal(_run(m, dev, feats)[0], one[0])


def test_model_features_as_one_tensor():
    m = _model()
    dev = batch_to(_batch(), DEV)
    rows = torch.from_numpy(_bank_rows(dev)).to(DEV)
    as_list = _run(m, dev, list(rows.unbind(0)))
    as_tensor = _run(m, dev, rows)
    assert len(as_list) == len(as_tensor) >= 4 and all(torch.equal(a, b) for a, b in zip(as_list, as_tensor))
    with_none = list(rows.unbind(0))
    with_none[1] = None                                         # the list form keeps its None entries: repr_net's row there
    assert not torch.equal(_run(m, dev, with_none)[0], as_list[0])
    for bad, match in ((rows[:, :31], 'must be'), (rows[:-1], 'must be'), (rows.cpu(), 'float tensor on'), (rows.to(torch.int32), 'float tensor on')):
        with pytest.raises(ValueError, match=match):
            _run(m, dev, bad)


# =====================================================================================================================================
# 5. the sampler and the command line
# =====================================================================================================================================
def _sampler(m, seed, **kw):
    return sample.Sampler(m, features=SH.make_banks()[0], quasi_random=qmc.QuasiRandomInputs(64, max_objects=8, seed=seed, device=DEV), **kw)


def test_sampler_repeats_with_the_seed_and_follows_the_restatement():
    m, stats = _model(), _stats()
    batches = [_batch(321), _batch(322)]
    runs = {}
    for tag, seed in (('a', 6), ('b', 6), ('c', 7)):
        s = _sampler(m, seed, attribute_stats=stats, sample_attributes=True)
        outs, draws = [], []
        for b in batches:
            random.seed(tag)                                    # whatever the pseudo-random stream holds
            outs.append(s.sample_batch(b))
            draws.append(s.last_draws)
        runs[tag] = (outs, draws, s)
    for x, y in zip(runs['a'][0], runs['b'][0]):
        assert torch.equal(x.images, y.images) and torch.equal(x.boxes_pred, y.boxes_pred) and torch.equal(x.masks_pred, y.masks_pred)
    assert not torch.equal(runs['a'][0][0].images, runs['c'][0][0].images)
    assert not torch.equal(runs['a'][0][0].images, runs['a'][0][1].images)
    assert m.noise_override.shape == (1, 64)                    # restored after every forward
    # call k consumed the points [k N, (k + 1) N)
    s = runs['a'][2]
    assert s.quasi_random.position == 6 and s.quasi_random.dimension == 64 + 24
    dirs, shift = R.tables(88, True, 6)
    bank = s._device_bank
    for k, b in enumerate(batches):
        noise, pick, u, row_idx = runs['a'][1][k]
        wn, wp, wu = R.unpack(R.points(dirs, shift, 3 * k, 3), b.obj_to_img.tolist(), 64, 8)
        assert np.array_equal(pick.cpu().numpy(), wp) and np.array_equal(u.cpu().numpy().astype(np.float64), wu)
        _within_one_ulp(noise.cpu().numpy(), wn, 'noise', 'sampler_call%d' % k)
        want_idx = R.bank_draw(bank.bank.cpu().numpy(), bank.class_off.cpu().numpy(), b.objs.tolist(), wp)[1]
        assert np.array_equal(row_idx.cpu().numpy(), want_idx) and (want_idx >= 0).all()
    # the attribute block the forward saw is the draw with the stream's uniforms
    seen = []
    real = m.forward

    def spy(*a, **k):
        seen.append((k['attributes'].clone(), k['features'], m.noise_override))
        return real(*a, **k)
    m.forward = spy
    try:
        s2 = _sampler(m, 6, attribute_stats=stats, sample_attributes=True)
        s2.sample_batch(batches[0])
    finally:
        del m.forward
    dev = [t.to(DEV) for t in batches[0]]
    noise, pick, u, row_idx = s2.last_draws
    want = attributes.sample_attributes(dev[1], dev[4], dev[5], stats, given=torch.zeros_like(dev[7]), u=u, triple_to_img=dev[6])[0]
    assert torch.equal(seen[0][0], want) and torch.is_tensor(seen[0][1]) and tuple(seen[0][1].shape) == (dev[1].numel(), 32)
    assert seen[0][2] is noise and torch.equal(noise, runs['a'][1][0][0])
    assert torch.equal(seen[0][1], bank.bank[(bank.class_off[dev[1]] + row_idx)])
    # ground-truth textures: the bank columns are skipped
    s3 = _sampler(m, 6)
    s3.sample_batch(batches[0], use_gt_textures=True)
    assert s3.last_draws[3] is None and s3._device_bank is None and torch.equal(s3.last_draws[1], pick)
    # an image over the limit raises before anything is drawn
    s4 = sample.Sampler(m, features=SH.make_banks()[0], quasi_random=qmc.QuasiRandomInputs(64, max_objects=2, seed=1, device=DEV))
    with pytest.raises(ValueError, match='more than 2 objects'):
        s4.sample_batch(batches[0])
    assert s4.quasi_random.position == 0
    with pytest.raises(ValueError, match='No features file'):
        sample.Sampler(m, quasi_random=qmc.QuasiRandomInputs(64, max_objects=8, device=DEV)).sample_batch(batches[0])
    with pytest.raises(ValueError, match='mask noise has 64'):
        sample.Sampler(m, features=SH.make_banks()[0], quasi_random=qmc.QuasiRandomInputs(32, max_objects=8, device=DEV)).sample_batch(batches[0])


def test_sample_pair_and_json_leave_the_scored_stream_alone():
    m, stats = _model(), _stats()
    b = _batch()
    pairs = []
    s = _sampler(m, 6, attribute_stats=stats, sample_attributes=True, diversity=lambda x, y: pairs.append((x, y)))
    first, second = s.sample_pair(b)
    assert s.quasi_random.position == 3 and s._quasi_pair.position == 3 and s._quasi_pair.seed == 7           # N, not 2 N
    assert len(pairs) == 1 and pairs[0][0] is first.images and not torch.equal(first.images, second.images)
    alone = _sampler(m, 6, attribute_stats=stats, sample_attributes=True).sample_batch(b)
    assert torch.equal(alone.images, first.images)              # the scored forward is the one a plain call runs
    s.sample_pair(b)
    assert s.quasi_random.position == 6 and s._quasi_pair.position == 6
    # scene graphs: noise and attribute columns from the stream, the bank rows by the graphs' own feature numbers
    outs = []
    for _ in range(2):
        sj = _sampler(m, 9, attribute_stats=stats, sample_attributes=True)
        outs.append(sj.sample_json(SH.scene_graphs()))
        assert sj.quasi_random.position == 2 and sj.last_draws[3] is None and tuple(sj.last_draws[0].shape) == (2, 64)
    assert torch.equal(outs[0].images, outs[1].images)
    assert not torch.equal(outs[0].images, _sampler(m, 10, attribute_stats=stats, sample_attributes=True).sample_json(SH.scene_graphs()).images)


def test_sampler_without_quasi_random_draws_as_the_host_loop_always_did():
    m = _model()
    b = _batch()
    many = SH.make_banks()[0]
    seen = []
    real = m.forward

    def spy(*a, **k):
        seen.append(k['features'])
        return real(*a, **k)
    m.forward = spy
    try:
        s = sample.Sampler(m, features=many)
        random.seed(0)
        s.sample_batch(b)
    finally:
        del m.forward
    random.seed(0)
    want = []
    for c in b.objs.tolist():                                   # sample_images.py: one randint per object, in object order
        want.append(many[c][random.randint(0, many[c].shape[0] - 1), :])
    assert isinstance(seen[0], list) and len(seen[0]) == len(want)
    assert torch.equal(torch.stack(seen[0]).cpu(), torch.from_numpy(np.stack(want).astype(np.float32)))
    assert s.quasi_random is None and s.last_draws is None and s._device_bank is None and s._quasi_pair is None


# the arguments of SH.small_model, whose pictures depend on their inputs (its box_net override travels in the state dict)
KW = dict(image_size=(32, 32), gconv_hidden_dim=64, gconv_num_layers=3, mask_size=8, mlp_normalization='none',
          appearance_normalization='batch', activation='leakyrelu-0.2', n_downsample_global=2, use_attributes=True, pool_size=2)


def test_command_line_repeats_byte_for_byte(tmp_path):
    vocab = make_sampling_vocab(SH.C, 7, SH.A)
    ckpt = str(tmp_path / 'ckpt.pt')
    torch.save({'model_kwargs': dict(vocab=vocab, **KW), 'model_state': _model().state_dict()}, ckpt)
    bank = str(tmp_path / 'bank.npy')
    np.save(bank, SH.make_banks()[0], allow_pickle=True)
    base = ['--checkpoint', ckpt, '--features', bank, '--num_samples', '5', '--batch_size', '3', '--quasi_random', '1']
    files = {}
    for tag, extra in (('a', []), ('b', []), ('c', ['--qmc_seed', '1'])):
        random.seed(tag)
        torch.manual_seed(len(files))
        res = sample.main(base + extra + ['--output_dir', str(tmp_path / tag)])
        assert len(res['paths']) == 5 and all(os.path.isfile(p) for p in res['paths'])
        files[tag] = [open(p, 'rb').read() for p in res['paths']]
    assert files['a'] == files['b'] and len(set(files['a'])) == 5           # byte for byte, and five different pictures
    assert all(x != y for x, y in zip(files['a'], files['c']))               # another scrambling: other pictures
    with pytest.raises(ValueError, match='more than 1 objects'):
        sample.main(base + ['--qmc_max_objects', '1', '--output_dir', str(tmp_path / 'd')])
