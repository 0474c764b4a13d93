"""Statistics of all pairs of retained feature rows (csrc/featsets.hip): the polynomial-kernel sums of the Kernel Inception Distance,
the k-NN radii and the membership pass of improved precision / recall and density / coverage, all on the f64 matrix cores.  No
wrapper synchronises.  (Part of scene_generation_amd.ops: see ops/__init__.py.)"""
import ctypes

import numpy as np
import torch

from ._core import _L, _call, _dev, _p, _stream, workspace

_PD = ctypes.POINTER(ctypes.c_double)
KNN_MAX = 8
POLY_DEGREE_MAX = 4


def _pd(t):
    return ctypes.cast(t.data_ptr(), _PD)


def _rows(x, who, D=None):
    """float32 feature rows [rows, D] on the device, unit column stride, row stride >= D -> (x, rows, D, ld)"""
    _dev(x, who)
    if x.dtype != torch.float32:
        raise TypeError('%s must be float32, got %s' % (who, x.dtype))
    if x.dim() != 2 or (D is not None and x.size(1) != D):
        raise ValueError('%s: feature rows [rows, %s], got %s' % (who, 'D' if D is None else D, tuple(x.shape)))
    rows, D = x.size(0), x.size(1)
    if (D > 1 and x.stride(1) != 1) or (rows > 1 and x.stride(0) < D):
        x = x.contiguous()
    return x, rows, D, (x.stride(0) if rows > 1 else D)


def _out(out, shape, dtype, device, who):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise ValueError('%s must be a contiguous %s tensor %s on %s, got %s %s on %s'
                         % (who, dtype, tuple(shape), device, out.dtype, tuple(out.shape), out.device))
    return out


def _table(t, rows, who):
    """a host index table [S, s] -> contiguous int32 NumPy array, every entry checked against [0, rows) (free here: no device
    synchronisation)"""
    if isinstance(t, torch.Tensor):
        if t.is_cuda:
            raise ValueError('%s: the index tables are host arrays (they are range-checked before the upload)' % who)
        t = t.numpy()
    t = np.asarray(t)
    if t.ndim != 2 or t.shape[1] < 1 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError('%s: an integer table [S, s] with s >= 1, got %s %s' % (who, t.dtype, t.shape))
    if t.size and (int(t.min()) < 0 or int(t.max()) >= rows):
        raise ValueError('%s: indices span [%d, %d], outside the %d rows of the set' % (who, int(t.min()), int(t.max()), rows))
    return np.ascontiguousarray(t, dtype=np.int32)


def feat_poly_sums(x, y, ix, iy, gamma, coef0, degree, out=None):
    """-> out [S, 3] float64 on the device: per subset q, sum_{i != j} k(x_ix[q,i], x_ix[q,j]), sum_{i != j} k(y_.., y_..) and
    sum_{i, j} k(x_.., y_..) with k(a, b) = (gamma a.b + coef0)^degree (degree 1..4).  ``x`` [n, D], ``y`` [m, D] float32 on the
    device; ``ix``, ``iy`` HOST integer tables [S, s], range-checked here (ValueError, nothing is launched) and then uploaded."""
    x, n, D, ldx = _rows(x, 'feat_poly_sums x')
    y, m, _, ldy = _rows(y, 'feat_poly_sums y', D)
    if x.device != y.device:
        raise ValueError('feat_poly_sums: x on %s and y on %s' % (x.device, y.device))
    if n < 1 or m < 1:
        raise ValueError('feat_poly_sums: empty feature set (%d and %d rows)' % (n, m))
    if not 1 <= int(degree) <= POLY_DEGREE_MAX:
        raise ValueError('feat_poly_sums: degree %r is outside 1..%d' % (degree, POLY_DEGREE_MAX))
    tx, ty = _table(ix, n, 'feat_poly_sums ix'), _table(iy, m, 'feat_poly_sums iy')
    if tx.shape != ty.shape:
        raise ValueError('feat_poly_sums: tables of %s and %s' % (tx.shape, ty.shape))
    S, s = tx.shape
    out = _out(out, (S, 3), torch.float64, x.device, 'feat_poly_sums out')
    if S == 0:
        return out
    dx, dy = torch.from_numpy(tx).to(x.device), torch.from_numpy(ty).to(x.device)
    nbytes = int(_L().sg_feat_poly_sums_ws_bytes(S, s))
    ws = workspace(nbytes, x.device)
    _call('sg_feat_poly_sums', _p(x), n, ldx, _p(y), m, ldy, D, _p(dx), _p(dy), S, s, float(gamma), float(coef0), int(degree), _pd(out),
          _p(ws), nbytes, _stream())
    return out


def feat_knn_radius(x, k, out=None):
    """-> r2 [n] float64 on the device: the k-th smallest squared distance from each row of ``x`` [n, D] to the OTHER rows (by
    index: duplicate rows count), 1 <= k <= 8, k < n"""
    x, n, D, ldx = _rows(x, 'feat_knn_radius x')
    k = int(k)
    if not 1 <= k <= KNN_MAX or k >= n:
        raise ValueError('feat_knn_radius: k = %d needs 1 <= k <= %d and at least k + 1 = %d rows, got %d' % (k, KNN_MAX, k + 1, n))
    out = _out(out, (n,), torch.float64, x.device, 'feat_knn_radius out')
    nbytes = int(_L().sg_feat_knn_radius_ws_bytes(n))
    ws = workspace(nbytes, x.device)
    _call('sg_feat_knn_radius', _p(x), n, D, ldx, k, _pd(out), _p(ws), nbytes, _stream())
    return out


def feat_manifold_counts(a, r2, b, count=None, mind2=None):
    """references ``a`` [n, D] with radii ``r2`` [n] (float64), queries ``b`` [m, D] -> (count [m] int32: the number of reference
    balls each query lies in, mind2 [n] float64: each reference's squared distance to its nearest query), on the device"""
    a, n, D, lda = _rows(a, 'feat_manifold_counts a')
    b, m, _, ldb = _rows(b, 'feat_manifold_counts b', D)
    if n < 1 or m < 1:
        raise ValueError('feat_manifold_counts: empty feature set (%d references, %d queries)' % (n, m))
    if (not r2.is_cuda or r2.dtype != torch.float64 or tuple(r2.shape) != (n,) or not r2.is_contiguous() or r2.device != a.device
            or b.device != a.device):
        raise ValueError('feat_manifold_counts: r2 must be a contiguous float64 tensor [%d] on %s, b on the same device' % (n, a.device))
    count = _out(count, (m,), torch.int32, a.device, 'feat_manifold_counts count')
    mind2 = _out(mind2, (n,), torch.float64, a.device, 'feat_manifold_counts mind2')
    nbytes = int(_L().sg_feat_manifold_counts_ws_bytes(n, m))
    ws = workspace(nbytes, a.device)
    _call('sg_feat_manifold_counts', _p(a), n, lda, _pd(r2), _p(b), m, ldb, D, _p(count), _pd(mind2), _p(ws), nbytes, _stream())
    return count, mind2
