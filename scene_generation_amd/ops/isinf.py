"""IS-infinity's own operators (csrc/isinf.hip): the per-row sums and entropies of the stored softmax rows, and the Inception score of
every subset of them by one gathered column reduction.  No wrapper synchronises.  (Part of scene_generation_amd.ops: see
ops/__init__.py.)"""
import numpy as np
import torch

from .._hip import CONST
from ._core import _L, _call, _p, _stream, workspace
from .featsets import _out, _pd, _rows, _table
from .fidinf import _f64

ISINF_ROWS_PER_WG = CONST['SG_ISINF_ROWS_PER_WG']


def isinf_row_terms(probs, rs=None, h=None):
    """-> (rs, h) float64 [n] on the device: rs[i] = the float64 sum of row i of ``probs`` (float32 [n, classes] on the device, n >= 1;
    a row stride >= classes is taken as it is), h[i] = sum_j ph log ph with ph = double(p) / rs[i], a term whose ph is not > 0 being 0.
    The same call gives the same bits."""
    probs, n, classes, ldp = _rows(probs, 'isinf_row_terms probs')
    if n < 1 or classes < 1:
        raise ValueError('isinf_row_terms: probs [n >= 1, classes >= 1], got %s' % (tuple(probs.shape),))
    rs = _out(rs, (n,), torch.float64, probs.device, 'isinf_row_terms rs')
    h = _out(h, (n,), torch.float64, probs.device, 'isinf_row_terms h')
    _call('sg_isinf_row_terms', _p(probs), n, classes, ldp, _pd(rs), _pd(h), _stream())
    return rs, h


def isinf_subset_scores(probs, rs, h, idx, sizes, out=None):
    """-> out [S, 2] float64 on the device: {log score, score} of every subset.  ``probs`` as above, ``rs`` and ``h`` the results of
    ``isinf_row_terms`` on it; ``idx`` a HOST integer table [S, smax] whose row q holds ``sizes[q]`` row numbers (the rest of the row is
    never read; pad it with 0), ``sizes`` HOST integers [S] in 2 .. smax -- the pair ``fidinf.draw_subsets`` returns, both range-checked
    here (ValueError, nothing is launched) and then uploaded.  A subset of all rows in identity order is ``ops.inception_score`` with
    one split, up to the order of the sums.  The same call gives the same bits."""
    probs, n, classes, ldp = _rows(probs, 'isinf_subset_scores probs')
    if n < 1 or classes < 1:
        raise ValueError('isinf_subset_scores: probs [n >= 1, classes >= 1], got %s' % (tuple(probs.shape),))
    rs = _f64(rs, (n,), probs.device, 'isinf_subset_scores rs')
    h = _f64(h, (n,), probs.device, 'isinf_subset_scores h')
    tab = _table(idx, n, 'isinf_subset_scores idx')          # the whole table, the padding past a subset's size included
    S, smax = tab.shape
    if isinstance(sizes, torch.Tensor):
        if sizes.is_cuda:
            raise ValueError('isinf_subset_scores sizes: a host array (it is range-checked before the upload)')
        sizes = sizes.numpy()
    sz = np.asarray(sizes)
    if sz.shape != (S,) or not np.issubdtype(sz.dtype, np.integer):
        raise ValueError('isinf_subset_scores sizes: host integers [%d], got %s %s' % (S, sz.dtype, sz.shape))
    if smax < 2 or (S and (int(sz.min()) < 2 or int(sz.max()) > smax)):
        raise ValueError('isinf_subset_scores sizes: subsets of %s rows in a table of smax = %d columns; each needs 2 .. smax'
                         % ('%d .. %d' % (int(sz.min()), int(sz.max())) if S else 'no', smax))
    out = _out(out, (S, 2), torch.float64, probs.device, 'isinf_subset_scores out')
    if S == 0:
        return out
    dtab = torch.from_numpy(tab).to(probs.device)
    dsz = torch.from_numpy(np.ascontiguousarray(sz, dtype=np.int32)).to(probs.device)
    nbytes = int(_L().sg_isinf_subset_scores_ws_bytes(S, smax, classes))
    ws = workspace(nbytes, probs.device)
    _call('sg_isinf_subset_scores', _p(probs), n, classes, ldp, _pd(rs), _pd(h), _p(dtab), _p(dsz), S, smax, _pd(out), _p(ws), nbytes,
          _stream())
    return out
