"""FID-infinity's own operators (csrc/fidinf.hip): the two Gram matrices of the shifted fake rows on the f64 matrix cores, and the
per-subset terms every subset's Frechet distance is made of.  No wrapper synchronises.  (Part of scene_generation_amd.ops: see
ops/__init__.py.)"""
import numpy as np
import torch

from ._core import _L, _call, _dev, _p, _stream, workspace
from .featsets import _out, _pd, _rows, _table


def _f64(t, shape, device, who):
    """a contiguous float64 device tensor of ``shape`` on ``device``"""
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
            or t.device != device):
        raise ValueError('%s must be a contiguous float64 tensor %s on %s, got %s' % (
            who, tuple(shape), device, '%s %s on %s' % (t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor) else type(t)))
    return t


def fidinf_grams(x, mu, sigma, P=None, G=None):
    """-> (P, G) float64 [n, n] on the device: P = Z Z^T and G = Z sigma Z^T with Z = double(x) - mu.  ``x`` float32 [n, D] on the
    device (n >= 2; a row stride >= D is taken as it is), ``mu`` [D] and ``sigma`` [D, D] contiguous float64 on the same device.
    Both results equal their transposes bit for bit, and the same call gives the same bits."""
    x, n, D, ldx = _rows(x, 'fidinf_grams x')
    if n < 2:
        raise ValueError('fidinf_grams: a covariance needs at least 2 rows, got %d' % n)
    mu = _f64(mu, (D,), x.device, 'fidinf_grams mu')
    sigma = _f64(sigma, (D, D), x.device, 'fidinf_grams sigma')
    P = _out(P, (n, n), torch.float64, x.device, 'fidinf_grams P')
    G = _out(G, (n, n), torch.float64, x.device, 'fidinf_grams G')
    nbytes = int(_L().sg_fidinf_grams_ws_bytes(n, D))
    ws = workspace(nbytes, x.device)
    _call('sg_fidinf_grams', _p(x), n, D, ldx, _pd(mu), _pd(sigma), _pd(P), _pd(G), _p(ws), nbytes, _stream())
    return P, G


def fidinf_subset_terms(P, G, idx, sizes, M=None, sums=None):
    """-> (M [S, smax, smax], sums [S, 2]) float64 on the device.  ``P``, ``G``: the results of ``fidinf_grams``; ``idx`` a HOST integer
    table [S, smax] whose row q holds ``sizes[q]`` row numbers (the rest of the row is never read; pad it with 0), ``sizes`` HOST
    integers [S] in 2 .. smax -- both range-checked here (ValueError, nothing is launched) and then uploaded.  sums[q] = (sum_i P_ii, sum_ij P_ij) over
    the subset; the leading sizes[q] x sizes[q] block of M[q] is the doubly centred G of the subset over sizes[q] - 1, symmetric bit for
    bit; the entries outside the block are NOT written."""
    _dev(P, 'fidinf_subset_terms P')
    if P.dim() != 2 or P.size(0) != P.size(1) or P.size(0) < 2:
        raise ValueError('fidinf_subset_terms: P must be a square matrix of at least 2 rows, got %s' % (tuple(P.shape),))
    n = P.size(0)
    P = _f64(P, (n, n), P.device, 'fidinf_subset_terms P')
    G = _f64(G, (n, n), P.device, 'fidinf_subset_terms G')
    tab = _table(idx, n, 'fidinf_subset_terms idx')          # the whole table, the padding past a subset's size included
    S, smax = tab.shape
    if isinstance(sizes, torch.Tensor):
        if sizes.is_cuda:
            raise ValueError('fidinf_subset_terms sizes: a host array (it is range-checked before the upload)')
        sizes = sizes.numpy()
    sz = np.asarray(sizes)
    if sz.shape != (S,) or not np.issubdtype(sz.dtype, np.integer):
        raise ValueError('fidinf_subset_terms sizes: host integers [%d], got %s %s' % (S, sz.dtype, sz.shape))
    if smax < 2 or (S and (int(sz.min()) < 2 or int(sz.max()) > smax)):
        raise ValueError('fidinf_subset_terms sizes: subsets of %s rows in a table of smax = %d columns; each needs 2 .. smax'
                         % ('%d .. %d' % (int(sz.min()), int(sz.max())) if S else 'no', smax))
    M = _out(M, (S, smax, smax), torch.float64, P.device, 'fidinf_subset_terms M')
    sums = _out(sums, (S, 2), torch.float64, P.device, 'fidinf_subset_terms sums')
    if S == 0:
        return M, sums
    dtab = torch.from_numpy(tab).to(P.device)
    dsz = torch.from_numpy(np.ascontiguousarray(sz, dtype=np.int32)).to(P.device)
    nbytes = int(_L().sg_fidinf_subset_terms_ws_bytes(S, smax))
    ws = workspace(nbytes, P.device)
    _call('sg_fidinf_subset_terms', _pd(P), _pd(G), n, _p(dtab), _p(dsz), S, smax, _pd(M), _pd(sums), _p(ws), nbytes, _stream())
    return M, sums
