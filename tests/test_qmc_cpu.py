"""Quasi-random inputs, host side (scene_generation_amd/qmc.py, ops/qmc.py, include/sg2im_hip.h): the restated Sobol formula of
tests/qmc_ref.py against torch.quasirandom.SobolEngine -- which pins the reference the GPU tests compare the kernels with -- the
packing of the appearance bank, the column layout of a point, every bad argument of the three public classes and of the entry
points (negative codes before any launch), the operators' argument checks that need no device, and the parser's flags."""
import ctypes

import numpy as np
import pytest
import torch
from torch.quasirandom import SobolEngine

import qmc_ref as R
from scene_generation_amd import _hip, ops, qmc, sample

DIMS = (1, 3, 70, 160)
SEED = 5


def _ints(draw):
    """the 30-bit integers of a float64 draw of the engine (exact: a float64 holds x * 2^-30)"""
    v = draw.numpy() * 2.0 ** 30
    assert (v == np.floor(v)).all()
    return v.astype(np.int64)


# ---- the formula ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scramble', [False, True], ids=['plain', 'scrambled'])
@pytest.mark.parametrize('D', DIMS)
def test_restated_formula_equals_the_engine(D, scramble):
    dirs, shift = R.tables(D, scramble, SEED)
    assert dirs.shape == (D, 30) and shift.shape == (D,) and dirs.max() < 2 ** 30 and 0 <= shift.min() and shift.max() < 2 ** 30
    assert scramble or (shift == 0).all()
    e = SobolEngine(D, scramble=scramble, seed=SEED)
    got = np.concatenate([_ints(e.draw(137, dtype=torch.float64)), _ints(e.draw(163, dtype=torch.float64))])       # two draw calls
    want = R.points(dirs, shift, 0, 300)
    assert (want >= 0).all() and (want < 2 ** 30).all()
    assert np.array_equal(got[1:], want[1:])
    # point 0: the shift itself.  The engine keeps its first point as a float32 (``_first_point``), i.e. rounded to 24 bits when scrambled
    assert np.array_equal(want[0], e.shift.numpy())
    if scramble:
        assert np.array_equal(got[0], (np.float32(1.0) * (want[0] * 2.0 ** -30).astype(np.float32)).astype(np.float64) * 2.0 ** 30)
    else:
        assert np.array_equal(got[0], want[0]) and (want[0] == 0).all()
    # after a skip that ends three points before bit 20 of the point number first sets
    f = SobolEngine(D, scramble=scramble, seed=SEED)
    f.fast_forward(2 ** 20 - 3)
    assert np.array_equal(_ints(f.draw(9, dtype=torch.float64)), R.points(dirs, shift, 2 ** 20 - 3, 9))
    # every point stands alone: a run of the sequence is the same rows wherever it is cut
    assert np.array_equal(R.points(dirs, shift, 257, 43), want[257:])


def test_the_last_points_of_the_sequence():
    dirs, shift = R.tables(3, True, SEED)
    x = R.points(dirs, shift, 2 ** 30 - 4, 4)
    assert x.shape == (4, 3) and (x >= 0).all() and (x < 2 ** 30).all()
    with pytest.raises(AssertionError):
        R.points(dirs, shift, 2 ** 30 - 4, 5)


def test_unpack_restatement_ranges():
    x = np.array([[0, 2 ** 30 - 1, 2 ** 29, 63, 64, 2 ** 30 - 1]], np.int64)
    noise, pick, u = R.unpack(x, [0], 3, 1)
    assert np.isfinite(noise).all() and abs(noise[0, 0] + 6.1208) < 1e-3 and abs(noise[0, 1] - 6.1208) < 1e-3 and noise[0, 0] == -noise[0, 1]
    assert abs(noise[0, 2] - 2.0 ** -31 * np.sqrt(2 * np.pi)) < 1e-18      # the centre of the cell right of 1/2: the slope there is sqrt(2 pi)
    assert pick.tolist() == [63] and u.tolist() == [[2.0 ** -24, 1.0 - 2.0 ** -24]]
    assert (u.astype(np.float32).astype(np.float64) == u).all() and (u < 1).all()


# ---- DeviceBank ----------------------------------------------------------------------------------------------------------------------
def test_device_bank_packing():
    rs = np.random.RandomState(0)
    feats = {4: rs.rand(3, 5), 1: rs.rand(1, 5), 2: rs.rand(100, 5).astype(np.float32)}          # classes 0 and 3 missing, order shuffled
    b = qmc.DeviceBank.from_dict(feats, 6, device='cpu')
    assert b.bank.dtype == torch.float32 and tuple(b.bank.shape) == (104, 5) and b.rep == 5 and b.num_classes == 6
    assert b.class_off.dtype == torch.int64 and b.class_off.tolist() == [0, 0, 1, 101, 101, 104, 104]
    assert b.rows_per_class == [0, 1, 100, 0, 3, 0]
    for c, a in feats.items():
        lo = b.class_off[c].item()
        assert np.array_equal(b.bank[lo:lo + a.shape[0]].numpy(), a.astype(np.float32))
    objs = torch.tensor([1, 3, 2])
    with pytest.raises(ValueError, match='No features for class 3'):
        b.draw(objs, torch.zeros(3, dtype=torch.int32), objs_host=[1, 3, 2])
    with pytest.raises(ValueError, match='No features for class 6'):
        b.draw(objs, torch.zeros(3, dtype=torch.int32), objs_host=[1, 6, 2])
    with pytest.raises(ValueError, match='objs_host has 2 entries for 3'):
        b.draw(objs, torch.zeros(3, dtype=torch.int32), objs_host=[1, 2])
    # the restatement on the packed bank
    rows, idx = R.bank_draw(b.bank.numpy(), b.class_off.numpy(), [2, 2, 4, 4, 1, 0, 7, 2], [0, 2 ** 30 - 1, 2 ** 29, 2 ** 30 - 1, 12345, 5, 5, -1])
    assert idx.tolist() == [0, 99, 1, 2, 0, -1, -1, -1]
    assert np.array_equal(rows[1], b.bank[100].numpy()) and np.array_equal(rows[3], b.bank[103].numpy()) and not rows[5:].any()


@pytest.mark.parametrize('features,num_classes,match', [
    ([1, 2], 3, 'non-empty dictionary'), ({}, 3, 'non-empty dictionary'), ({0: np.zeros((2, 4))}, 0, 'num_classes'),
    ({0: np.zeros((2, 4))}, 2.0, 'num_classes'), ({3: np.zeros((2, 4))}, 3, 'holds the class 3'), ({-1: np.zeros((2, 4))}, 3, 'holds the class -1'),
    ({'a': np.zeros((2, 4))}, 3, 'holds the class'), ({0: np.zeros((2, 4)), 1: np.zeros((2, 5))}, 3, r'features\[1\] must be \[rows, 4\]'),
    ({0: np.zeros(4)}, 3, r'features\[0\] must be'), ({0: np.zeros((2, 0))}, 3, r'features\[0\] must be')])
def test_device_bank_bad_arguments(features, num_classes, match):
    with pytest.raises(ValueError, match=match):
        qmc.DeviceBank.from_dict(features, num_classes, device='cpu')


# ---- SobolStream / QuasiRandomInputs ------------------------------------------------------------------------------------------------
def test_stream_tables_and_position():
    s = qmc.SobolStream(70, seed=SEED, device='cpu')
    dirs, shift = R.tables(70, True, SEED)
    assert s.dirs.dtype == torch.int32 and s.shift.dtype == torch.int32 and s.scramble and s.dimension == 70
    assert np.array_equal(s.dirs.numpy(), dirs) and np.array_equal(s.shift.numpy(), shift)
    assert not qmc.SobolStream(3, scramble=False, device='cpu').shift.any()
    assert s.position == 0 and s.fast_forward(10) is s and s.position == 10 and s.fast_forward(0).position == 10
    assert s.fast_forward(2 ** 30 - 10).position == 2 ** 30 == qmc.POINTS
    with pytest.raises(ValueError, match='leaves the sequence'):
        s.draw(1)                                               # raises before anything is launched
    with pytest.raises(ValueError, match='leaves the sequence'):
        s.fast_forward(1)
    assert s.reset() is s and s.position == 0
    assert qmc.MAXBIT == 30 == SobolEngine.MAXBIT and 4096 <= qmc.MAX_DIMS <= SobolEngine.MAXDIM


@pytest.mark.parametrize('kw,match', [
    (dict(dimension=0), 'dimension'), (dict(dimension=qmc.MAX_DIMS + 1), 'dimension'), (dict(dimension=2.0), 'dimension'),
    (dict(dimension=True), 'dimension'), (dict(dimension=2, seed='a'), 'seed'), (dict(dimension=2, seed=1.5), 'seed')])
def test_stream_bad_arguments(kw, match):
    with pytest.raises(ValueError, match=match):
        qmc.SobolStream(device='cpu', **kw)


@pytest.mark.parametrize('n', [-1, 1.0, None, True])
def test_stream_bad_counts(n):
    s = qmc.SobolStream(2, device='cpu')
    with pytest.raises(ValueError, match='n must be a non-negative integer'):
        s.draw(n)
    with pytest.raises(ValueError, match='n must be a non-negative integer'):
        s.fast_forward(n)
    assert s.position == 0


def test_inputs_dimension_layout():
    q = qmc.QuasiRandomInputs(64, device='cpu')
    assert (q.noise_dim, q.max_objects, q.seed, q.dimension, q.position) == (64, 32, 0, 160, 0)
    assert q.stream.dimension == 160 and q.stream.scramble and q.stream.seed == 0
    q = qmc.QuasiRandomInputs(5, max_objects=4, seed=9, device='cpu')
    assert q.dimension == 17 and q.stream.seed == 9
    assert [q.columns(j) for j in range(4)] == [(5, 6, 7), (8, 9, 10), (11, 12, 13), (14, 15, 16)]
    for slot in (-1, 4):
        with pytest.raises(ValueError, match='slot'):
            q.columns(slot)
    assert qmc.QuasiRandomInputs(0, max_objects=1, device='cpu').dimension == 3
    q.check_image_sizes([0, 0, 0, 0, 2, 2, 2, 2])
    with pytest.raises(ValueError, match='image 2 has more than 4 objects'):
        q.check_image_sizes([0, 1, 2, 2, 2, 2, 2])
    o2i = torch.tensor([0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match='image 0 has more than 4 objects'):          # before anything is launched or drawn
        q.draw(o2i, torch.tensor([0, 5], dtype=torch.int32), 1, obj_to_img_host=[0] * 5)
    with pytest.raises(ValueError, match='obj_to_img_host has 4 entries for 5'):
        q.draw(o2i, torch.tensor([0, 5], dtype=torch.int32), 1, obj_to_img_host=[0] * 4)
    for N in (-1, 1.5):
        with pytest.raises(ValueError, match='N must be'):
            q.draw(o2i, torch.tensor([0, 5], dtype=torch.int32), N)
    q.stream.fast_forward(2 ** 30 - 1)
    with pytest.raises(ValueError, match='leaves the sequence'):
        q.draw(o2i[:2], torch.tensor([0, 1, 2], dtype=torch.int32), 2, obj_to_img_host=[0, 1])
    assert q.position == 2 ** 30 - 1


@pytest.mark.parametrize('kw,match', [
    (dict(noise_dim=-1), 'noise_dim'), (dict(noise_dim=1.0), 'noise_dim'), (dict(noise_dim=4, max_objects=0), 'max_objects'),
    (dict(noise_dim=4, max_objects=2.0), 'max_objects'), (dict(noise_dim=4, seed='x'), 'seed'), (dict(noise_dim=4, seed=None), 'seed'),
    (dict(noise_dim=qmc.MAX_DIMS, max_objects=1), 'dimensions')])
def test_inputs_bad_arguments(kw, match):
    with pytest.raises(ValueError, match=match):
        qmc.QuasiRandomInputs(device='cpu', **kw)


# ---- operators and entry points ------------------------------------------------------------------------------------------------------
def test_operators_name_the_host_tensor():
    """a CPU tensor is refused by name (there is no fallback); nothing is launched"""
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(ValueError, match='dirs is on cpu'):
        ops.sg_sobol_points(i32(2, 30), i32(2), 0, 1)
    with pytest.raises(ValueError, match='dirs must be a tensor'):
        ops.sg_sobol_points(None, i32(2), 0, 1)
    with pytest.raises(ValueError, match='points is on cpu'):
        ops.sg_qmc_unpack(i32(1, 4), torch.zeros(1, dtype=torch.int64), i32(2), 1, 1)
    with pytest.raises(ValueError, match='noise_dim = -1'):
        ops.sg_qmc_unpack(i32(1, 4), torch.zeros(1, dtype=torch.int64), i32(2), -1, 1)
    with pytest.raises(ValueError, match='bank is on cpu'):
        ops.sg_bank_draw(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), i32(1))


def test_header_binds_the_entry_points():
    for name in ('sg_sobol_points', 'sg_qmc_unpack', 'sg_bank_draw'):
        assert name in _hip.PROTOS and _hip.PROTOS[name][0] == ctypes.c_int and _hip.PROTOS[name][2][-1] == 'stream'
        assert hasattr(_hip.lib(), name)
    assert _hip.PROTOS['sg_sobol_points'][2] == ['dirs', 'shift', 'out', 'first', 'n', 'D', 'ld', 'stream']
    assert _hip.PROTOS['sg_sobol_points'][1][3:5] == [ctypes.c_int64, ctypes.c_int64]
    assert _hip.CONST['SG_QMC_MAXBIT'] == 30 and _hip.CONST['SG_QMC_MAX_DIMS'] >= 4096
    codes = [_hip.CONST['SG_QMC_ERR_' + k] for k in ('NULL', 'DIMS', 'LD', 'RANGE', 'COUNT')]
    assert all(c < 0 for c in codes) and len(set(codes + [-1, _hip.CONST['SG_ERR_INDEX']])) == 7


def test_entry_points_refuse_bad_arguments_with_distinct_codes():
    """host memory stands in for the operands: a refused call launches nothing and touches none of it"""
    L, E = _hip.lib(), {k: _hip.CONST['SG_QMC_ERR_' + k] for k in ('NULL', 'DIMS', 'LD', 'RANGE', 'COUNT')}
    buf = (ctypes.c_char * 4096)(*([0x5a] * 4096))
    p = ctypes.cast(buf, ctypes.c_void_p)

    def run(name, good, **kw):
        a = dict(good, **kw)
        rc = getattr(L, name)(*[a[k] for k in _hip.PROTOS[name][2]])
        assert rc == 0 or name in _hip.last_error(), (name, kw)
        return rc

    good = dict(dirs=p, shift=p, out=p, first=0, n=4, D=3, ld=3, stream=None)
    for kw, code in ((dict(dirs=None), 'NULL'), (dict(shift=None), 'NULL'), (dict(out=None), 'NULL'), (dict(D=0), 'DIMS'),
                     (dict(D=_hip.CONST['SG_QMC_MAX_DIMS'] + 1, ld=1 << 20), 'DIMS'), (dict(ld=2), 'LD'), (dict(first=-1), 'RANGE'),
                     (dict(first=2 ** 30 - 3), 'RANGE'), (dict(first=2 ** 30 + 1, n=0), 'RANGE'), (dict(first=2 ** 62, n=2 ** 62), 'RANGE'),
                     (dict(n=-1), 'COUNT')):
        assert run('sg_sobol_points', good, **kw) == E[code], kw
    assert run('sg_sobol_points', good, n=0, dirs=None, shift=None, out=None) == 0
    assert run('sg_sobol_points', good, n=0, first=2 ** 30, dirs=None, shift=None, out=None) == 0

    good = dict(points=p, ld=11, obj_to_img=p, seg_off=p, noise=p, pick=p, u=p, N=2, O=3, noise_dim=5, max_objects=2, stream=None)
    for kw, code in ((dict(points=None), 'NULL'), (dict(obj_to_img=None), 'NULL'), (dict(seg_off=None), 'NULL'), (dict(noise=None), 'NULL'),
                     (dict(pick=None), 'NULL'), (dict(u=None), 'NULL'), (dict(noise_dim=-1), 'DIMS'), (dict(max_objects=-1), 'DIMS'),
                     (dict(noise_dim=0, max_objects=0), 'DIMS'), (dict(max_objects=8000, ld=1 << 20), 'DIMS'), (dict(ld=10), 'LD'),
                     (dict(N=-1), 'COUNT'), (dict(O=-1), 'COUNT'), (dict(N=2 ** 30, noise_dim=4), 'COUNT')):
        assert run('sg_qmc_unpack', good, **kw) == E[code], kw
    assert run('sg_qmc_unpack', good, N=0, O=0, points=None, obj_to_img=None, seg_off=None, noise=None, pick=None, u=None) == 0

    good = dict(bank=p, class_off=p, objs=p, pick=p, row_idx=p, rows=p, O=3, C=2, rep=4, R=5, stream=None)
    for kw, code in ((dict(bank=None), 'NULL'), (dict(class_off=None), 'NULL'), (dict(objs=None), 'NULL'), (dict(pick=None), 'NULL'),
                     (dict(row_idx=None), 'NULL'), (dict(rows=None), 'NULL'), (dict(C=0), 'DIMS'), (dict(rep=0), 'DIMS'), (dict(O=-1), 'COUNT'),
                     (dict(R=-1), 'COUNT'), (dict(O=2 ** 30, rep=2), 'COUNT')):
        assert run('sg_bank_draw', good, **kw) == E[code], kw
    assert run('sg_bank_draw', good, O=0, bank=None, class_off=None, objs=None, pick=None, row_idx=None, rows=None) == 0
    assert bytes(buf) == b'\x5a' * 4096


# ---- command line --------------------------------------------------------------------------------------------------------------------
def test_parser_flags():
    a = sample.make_parser().parse_args(['--checkpoint', 'c'])
    assert a.quasi_random is False and a.qmc_seed == 0 and a.qmc_max_objects == 32
    a = sample.make_parser().parse_args(['--checkpoint', 'c', '--quasi_random', '1', '--qmc_seed', '7', '--qmc_max_objects', '12'])
    assert a.quasi_random is True and a.qmc_seed == 7 and a.qmc_max_objects == 12
    assert sample.Sampler.__init__.__defaults__[-1] is None          # quasi_random: off unless handed in
