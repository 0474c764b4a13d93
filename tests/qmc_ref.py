"""Plain-numpy restatement, in int64 / float64, of the three definitions of the quasi-random inputs (include/sg2im_hip.h:
sg_sobol_points, sg_qmc_unpack, sg_bank_draw), shared by tests/test_qmc_cpu.py -- which pins ``points`` to
torch.quasirandom.SobolEngine -- and tests/test_gpu_qmc.py.  Host only."""
import numpy as np

MAXBIT = 30


def tables(D, scramble, seed=0):
    """(dirs [D, 30], shift [D]) int64 of a torch.quasirandom.SobolEngine"""
    from torch.quasirandom import SobolEngine
    e = SobolEngine(D, scramble=scramble, seed=seed)
    return e.sobolstate.numpy().astype(np.int64), e.shift.numpy().astype(np.int64)


def points(dirs, shift, first, n):
    """x [n, D] int64: x(i, d) = shift[d] ^ XOR over the set bits b of g of dirs[d][b], g = k ^ (k >> 1), k = first + i"""
    dirs, shift = np.asarray(dirs, np.int64), np.asarray(shift, np.int64)
    assert first >= 0 and n >= 0 and first + n <= 1 << MAXBIT
    k = first + np.arange(n, dtype=np.int64)
    g = k ^ (k >> 1)
    x = np.broadcast_to(shift[None, :], (n, shift.size)).copy()
    for b in range(MAXBIT):
        x ^= np.where(((g >> b) & 1)[:, None] == 1, dirs[None, :, b], 0)
    return x


def cell_centres(x):
    """the argument of the inverse normal CDF, float64 (exact: x + 0.5 has 31 bits)"""
    return (np.asarray(x, np.int64).astype(np.float64) + 0.5) * 2.0 ** -MAXBIT


def unpack(pts, obj_to_img, noise_dim, max_objects):
    """-> (noise float64 [N, noise_dim] = ndtri of the cell centres, unrounded; pick int64 [O]; u float64 [O, 2], each exactly an
    fp32 value) of the points [N, >= noise_dim + 3 * max_objects]; objects of sorted obj_to_img in slots past max_objects, or of an
    image outside [0, N): pick -1, u 0"""
    from scipy.special import ndtri
    pts = np.asarray(pts, np.int64)
    o2i = np.asarray(obj_to_img, np.int64)
    N, O = pts.shape[0], o2i.size
    noise = ndtri(cell_centres(pts[:, :noise_dim]))
    seg = np.searchsorted(o2i, np.arange(N + 1))
    pick, u = np.full(O, -1, np.int64), np.zeros((O, 2), np.float64)
    for o in range(O):
        n = int(o2i[o])
        if not 0 <= n < N:
            continue
        j = o - int(seg[n])
        if 0 <= j < max_objects:
            c = noise_dim + 3 * j
            pick[o] = pts[n, c]
            u[o] = (pts[n, c + 1:c + 3] >> 6).astype(np.float64) * 2.0 ** -24
    return noise, pick, u


def bank_draw(bank, class_off, objs, pick):
    """-> (rows [O, rep] of bank's dtype, row_idx int64 [O]): idx = (pick * rows_c) >> 30 within the class; -1 and zeros for a class
    outside the table or without rows and for a pick outside [0, 2^30)"""
    bank, off = np.asarray(bank), np.asarray(class_off, np.int64)
    C, O = off.size - 1, len(objs)
    rows, row_idx = np.zeros((O, bank.shape[1]), bank.dtype), np.full(O, -1, np.int64)
    for o in range(O):
        c, p = int(objs[o]), int(pick[o])
        if not 0 <= c < C or not 0 <= p < 1 << MAXBIT:
            continue
        n = int(off[c + 1] - off[c])
        if n <= 0:
            continue
        idx = (p * n) >> MAXBIT
        row_idx[o] = idx
        rows[o] = bank[int(off[c]) + idx]
    return rows, row_idx
