"""FID-infinity (Chong & Forsyth, CVPR 2020): the Frechet Inception Distance extrapolated to an infinite number of generated images.

    python -m scene_generation_amd.fidinf --weights W --real DIR|STATS.npz --fake DIR|FEATS.npy [--num_points 15] [--min_size n]
                                          [--seed 0] [--batch_size 32] [--image_size H,W [--resize_filter bilinear|bicubic]]
        -> FID_inf x / FID_N y N n

The FID of N generated images over-estimates the distance by a term that is close to linear in 1 / N.  FID-infinity evaluates the FID
on subsets of several sizes n, fits a line in 1 / n and reports its intercept.  Every subset of a validation pass has fewer rows than
the features have dimensions, and there the whole computation lives on the n x n side.  With Z = X - 1 mu_r^T (the fake rows shifted
by the real mean), H = I - 1 1^T / n and S the rows of a subset:

* the non-zero eigenvalues of Sigma_r Sigma_S are those of M_S = H G_SS H / (n - 1), G = Z Sigma_r Z^T, a positive semi-definite
  n x n matrix: tr (Sigma_r Sigma_S)^1/2 = sum sqrt(lambda_i(M_S));
* tr Sigma_S = (sum_i P_ii - sum_ij P_ij / n) / (n - 1) and |mean_S - mu_r|^2 = sum_ij P_ij / n^2 over the subset, P = Z Z^T.

So ``ops.fidinf_grams`` computes P and G ONCE for all the rows (f64 matrix cores), ``ops.fidinf_subset_terms`` gathers and centres
each subset's block, and the host takes ``numpy.linalg.eigvalsh`` of one n_q x n_q matrix per subset -- a symmetric eigenproblem of
at most ``max_rows`` = 4096 rows is not worth a device solver.  No D x D matrix is decomposed anywhere, and the result is exact for the
rank-deficient covariances such subsets always have.  Only ``compute()`` / ``fid_infinity`` synchronise; they read back one n_q x n_q
matrix and two numbers per subset, never a feature row.

* The route is for N <= ``max_rows`` rows (the M blocks grow as N^2); beyond that the bias it removes is small and plain FID
  (fid.py) is the tool.
* IS-infinity, the paper's companion for the Inception score, is ``isinf.py``; it uses ``draw_sizes``, ``draw_subsets`` and
  ``extrapolate`` of this module.  The paper's Sobol sampling of the generator's input is NOT built.
* ``FIDInfinity`` speaks the protocol ``FrechetInceptionDistance(sets=...)`` and ``InceptionScore(fid=...)`` drive, and forwards every
  call to an optional ``FeatureSetMetrics`` (``then``), so FID, FID-infinity, KID and precision / recall hang on one Inception forward.
"""
import argparse

import numpy as np
import torch

from . import ops
from .featsets import FeatureBank, load_features
from .fid import FeatureMoments, _truncate, load_statistics
from .imageprep import _feed_dir, add_arguments

__all__ = ['FIDInfinity', 'draw_sizes', 'draw_subsets', 'fid_from_terms', 'extrapolate', 'fid_infinity', 'check_count', 'main']

M_BYTES_MAX = 1 << 30            # the M blocks of one ops.fidinf_subset_terms call


# ---- the host's share -----------------------------------------------------------------------------------------------------------------
def draw_sizes(n_fake, num_points=15, min_size=None):
    """the subset sizes: ``numpy.linspace(min_size, n_fake, num_points).astype(int)`` without duplicates, ascending, the last one
    ``n_fake``.  ``min_size`` defaults to ``n_fake // 2``: with every n below the feature dimension the FID bends away from a line in
    1 / n at small n, and the upper half bends least (the paper's n_fake / 10 .. n_fake belongs to n > D)."""
    n_fake, num_points = int(n_fake), int(num_points)
    min_size = n_fake // 2 if min_size is None else int(min_size)
    if min_size < 2 or min_size > n_fake or num_points < 2:
        raise ValueError('draw_sizes: %d points from min_size = %d to %d rows; needs 2 <= min_size <= rows and at least 2 points'
                         % (num_points, min_size, n_fake))
    sizes = np.unique(np.linspace(min_size, n_fake, num_points).astype(int))
    if sizes.size < 2:
        raise ValueError('draw_sizes: %d .. %d rows give %d distinct size; a line needs 2' % (min_size, n_fake, sizes.size))
    return sizes


def draw_subsets(seed, sizes, n_fake):
    """(idx int32 [S, max(sizes)], sizes int32 [S]): row q holds ``sizes[q]`` distinct rows of the fake set, padded with 0 -- the prefix
    of a fresh permutation from ``numpy.random.RandomState(seed)`` per size, in the order of ``sizes``; a subset of all ``n_fake`` rows
    is the identity order and draws nothing.  On the host, before the first launch."""
    sizes = np.asarray(sizes).astype(np.int32).reshape(-1)
    if sizes.size < 1 or int(sizes.min()) < 2 or int(sizes.max()) > n_fake:
        raise ValueError('draw_subsets: subsets of %s rows from %d' % (sizes.tolist(), n_fake))
    rs = np.random.RandomState(seed)
    idx = np.zeros((sizes.size, int(sizes.max())), np.int32)
    for q, s in enumerate(sizes.tolist()):
        idx[q, :s] = np.arange(n_fake, dtype=np.int32) if s == n_fake else rs.permutation(n_fake)[:s]
    return idx, sizes


def fid_from_terms(sums_q, M_q, n_q, trace_sigma_r):
    """the Frechet distance of one subset to the real statistics, float64 on the host: ``sums_q`` = (sum_i P_ii, sum_ij P_ij),
    ``M_q`` = H G_SS H / (n_q - 1) [n_q, n_q], ``trace_sigma_r`` = tr Sigma_r.
    |mean_S - mu_r|^2 + tr Sigma_r + tr Sigma_S - 2 sum sqrt(lambda_i(M_q)), the eigenvalues truncated as in ``fid.frechet_distance``."""
    n = float(n_q)
    diag, total = float(sums_q[0]), float(sums_q[1])
    M_q = np.asarray(M_q, np.float64)
    if M_q.shape != (int(n_q), int(n_q)) or n_q < 2:
        raise ValueError('fid_from_terms: M %s for a subset of %d rows (at least 2)' % (M_q.shape, n_q))
    lam = _truncate(np.linalg.eigvalsh(M_q))
    mean_term = total / (n * n)
    trace_s = (diag - total / n) / (n - 1.0)
    return float(mean_term + float(trace_sigma_r) + trace_s - 2.0 * np.sqrt(lam).sum())


def extrapolate(sizes, fids):
    """(intercept, slope) of the ordinary least-squares line fid = intercept + slope / n, float64"""
    x = 1.0 / np.asarray(sizes, np.float64).reshape(-1)
    y = np.asarray(fids, np.float64).reshape(-1)
    if x.size != y.size or x.size < 2 or np.unique(x).size < 2:
        raise ValueError('extrapolate: a line needs 2 distinct sizes, got %d sizes and %d values' % (x.size, y.size))
    xm, ym = x.mean(), y.mean()
    slope = float(((x - xm) * (y - ym)).sum() / ((x - xm) ** 2).sum())
    return float(ym - slope * xm), slope


def _chunks(sizes, limit):
    """ascending ``sizes`` cut into runs [a, b) whose M blocks (b - a) * sizes[b - 1]^2 * 8 bytes stay within ``limit`` (one subset at
    least)"""
    a = 0
    while a < len(sizes):
        b = a + 1
        while b < len(sizes) and (b + 1 - a) * int(sizes[b]) ** 2 * 8 <= limit:
            b += 1
        yield a, b
        a = b


def _check_rows(n, max_rows):
    if n > max_rows:
        raise ValueError('fid_infinity: %d rows; the n x n route is for at most max_rows = %d (beyond that the bias of plain FID is '
                         'small: use fid.FrechetInceptionDistance)' % (n, max_rows))


def check_count(n_fake, num_points=15, min_size=None, max_rows=4096):
    """ValueError when ``fid_infinity`` would refuse ``n_fake`` rows (too many for the route, or too few for two subset sizes): for a
    caller that knows the count before it starts the work"""
    _check_rows(int(n_fake), max_rows)
    draw_sizes(n_fake, num_points, min_size)


def _on_device(fake_rows, dmu, dsigma, trace_r, num_points, min_size, seed, max_rows):
    """``fid_infinity`` with the real statistics already on the device as float64 tensors and tr Sigma_r on the host"""
    n = int(fake_rows.size(0))
    _check_rows(n, max_rows)
    idx, sizes = draw_subsets(seed, draw_sizes(n, num_points, min_size), n)           # on the host, before the first launch
    P, G = ops.fidinf_grams(fake_rows, dmu, dsigma)
    fids = []
    for a, b in _chunks(sizes, M_BYTES_MAX):
        smax = int(sizes[b - 1])
        M, sums = ops.fidinf_subset_terms(P, G, idx[a:b, :smax], sizes[a:b])
        host = sums.cpu().numpy()                                                     # the read-back: 2 numbers and one block per subset
        for q in range(b - a):
            s = int(sizes[a + q])
            fids.append(fid_from_terms(host[q], M[q, :s, :s].cpu().numpy(), s, trace_r))
    intercept, slope = extrapolate(sizes, fids)
    return {'fid_inf': intercept, 'fid': fids[-1], 'slope': slope, 'sizes': [int(s) for s in sizes], 'fids': fids, 'images': n}


def fid_infinity(fake_rows, mu, sigma, num_points=15, min_size=None, seed=0, max_rows=4096):
    """{'fid_inf', 'fid', 'slope', 'sizes', 'fids', 'images'}: the FID of ``fake_rows`` (float32 [N, D] on the device:
    ``FeatureBank.rows()``) to the real statistics ``mu`` [D], ``sigma`` [D, D] (float64 on the host) on ``num_points`` subset sizes
    from ``min_size`` to N (``draw_sizes`` / ``draw_subsets`` with ``seed``), and the intercept of their line in 1 / n.  'fid' is the
    value of all N rows, the last point; 'sizes' and 'fids' are lists.  More than ``max_rows`` rows: ValueError."""
    _check_rows(int(fake_rows.size(0)), max_rows)
    mu = np.ascontiguousarray(np.asarray(mu, np.float64).reshape(-1))
    sigma = np.ascontiguousarray(np.asarray(sigma, np.float64))
    dev = fake_rows.device
    return _on_device(fake_rows, torch.from_numpy(mu).to(dev), torch.from_numpy(sigma).to(dev), float(np.trace(sigma)), num_points,
                      min_size, seed, max_rows)


# ---- the object -----------------------------------------------------------------------------------------------------------------------
class FIDInfinity(object):
    """FID-infinity on pooled Inception features, fed by the forward of another metric: the ``sets`` of a
    ``FrechetInceptionDistance`` or the ``fid`` of an ``InceptionScore``.

    ``real_stats``: an ``.npz`` path or a ``(mu, sigma)`` pair that fixes the real side (``real_fixed``); None: the real side is its own
    ``FeatureMoments``, fed through ``add_real_features``.  Fake rows go to a ``FeatureBank``.  ``then``: a ``FeatureSetMetrics`` (or
    anything of this protocol) every call is forwarded to; its real side must be fixed exactly when this one is.
    ``add_features(f)`` / ``add_real_features(f)`` add rows, ``clean()`` clears the fake side, ``clean_real()`` the real one;
    ``compute()`` -> the dict of ``fid_infinity``.  No call but ``compute()`` synchronises."""

    def __init__(self, real_stats=None, dim=2048, device='cuda', num_points=15, min_size=None, seed=0, then=None):
        self.dim, self.device = int(dim), torch.device(device)
        self.num_points, self.min_size, self.seed, self.then = int(num_points), min_size, seed, then
        self.fake = FeatureBank(self.dim, self.device)
        self.real, self._stats, self._stats_dev, self._real_open = None, None, None, False
        if real_stats is not None:
            mu, sigma = load_statistics(real_stats) if isinstance(real_stats, str) else real_stats
            mu, sigma = np.asarray(mu, np.float64).reshape(-1), np.asarray(sigma, np.float64)
            if mu.size != self.dim or sigma.shape != (self.dim, self.dim):
                raise ValueError('FIDInfinity: real statistics of %d dimensions for features of %d' % (mu.size, self.dim))
            self._stats = (mu, sigma)
        else:
            self.real = FeatureMoments(self.dim, self.device)
            self._real_open = True
        if then is not None:
            if then.dim != self.dim:
                raise ValueError('FIDInfinity: then keeps features of %d dimensions, this object %d' % (then.dim, self.dim))
            if bool(then.real_fixed) != self.real_fixed:
                raise ValueError('FIDInfinity: the real side here is %s but that of then is %s; fix both (real_stats= and '
                                 'real_features=) or neither' % (('open', 'fixed')[self.real_fixed], ('open', 'fixed')[bool(then.real_fixed)]))

    # ---- feeding ------------------------------------------------------------------------------------------------------------------------
    @property
    def real_fixed(self):
        """the real side was given by ``real_stats`` and takes no rows"""
        return self.real is None

    @property
    def needs_real(self):
        return self._real_open

    def add_features(self, feats):
        """pooled features [rows, dim] of fake images"""
        self.fake.update(feats)
        if self.then is not None:
            self.then.add_features(feats)

    def add_real_features(self, feats):
        """pooled features [rows, dim] of real images"""
        if self.real is None:
            raise RuntimeError('FIDInfinity.add_real_features: the real side is fixed by real_stats')
        self._stats, self._stats_dev = None, None
        self.real.update(feats)
        if self.then is not None:
            self.then.add_real_features(feats)

    def clean(self):
        self.fake.clean()
        if self.then is not None:
            self.then.clean()

    def clean_real(self):
        if self.real is None:
            raise RuntimeError('FIDInfinity.clean_real: the real side is fixed by real_stats')
        self.real.clean()
        self._stats, self._stats_dev, self._real_open = None, None, True
        if self.then is not None:
            self.then.clean_real()

    # ---- the numbers --------------------------------------------------------------------------------------------------------------------
    def real_statistics(self):
        if self._stats is None:
            if self.real.count < 2:
                raise ValueError('FIDInfinity: the real side holds %d rows; a covariance needs at least 2' % self.real.count)
            self._stats = self.real.statistics()
        return self._stats

    def compute(self, max_rows=4096):
        if self.fake.count < 2:
            raise ValueError('FIDInfinity: the fake side holds %d rows; a covariance needs at least 2' % self.fake.count)
        mu, sigma = self.real_statistics()
        self._real_open = False
        if self._stats_dev is None:         # the real statistics do not change between evaluations: their device copy is kept
            self._stats_dev = (torch.from_numpy(np.ascontiguousarray(mu)).to(self.device),
                               torch.from_numpy(np.ascontiguousarray(sigma)).to(self.device), float(np.trace(sigma)))
        dmu, dsigma, trace_r = self._stats_dev
        return _on_device(self.fake.rows(), dmu, dsigma, trace_r, self.num_points, self.min_size, self.seed, max_rows)


def format_lines(res):
    """the two lines every front end ends with"""
    return ['FID_inf {}'.format(res['fid_inf']), 'FID_N {} N {}'.format(res['fid'], res['images'])]


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog='python -m scene_generation_amd.fidinf',
                                description='FID-infinity: the Frechet Inception Distance of a set of images extrapolated to an infinite '
                                'number of them (for at most 4096 images)')
    p.add_argument('--weights', default=None, type=str, help='state_dict file of the Inception network (never downloaded); needed for '
                   'a directory of images; only pt_inception-2015-12-05-*.pth gives numbers comparable with published ones')
    p.add_argument('--real', required=True, type=str, help='a directory of images, or an .npz with mu and sigma')
    p.add_argument('--fake', required=True, type=str, help='a directory of images, or an .npy of features [N, dim]')
    p.add_argument('--num_points', default=15, type=int, help='subset sizes on the line')
    p.add_argument('--min_size', default=None, type=int, help='smallest subset (default: half the fake images)')
    p.add_argument('--seed', default=0, type=int)
    p.add_argument('--batch_size', default=32, type=int)
    p.add_argument('--device', default='cuda', type=str)
    return add_arguments(p)


def main(argv=None):
    args = build_parser().parse_args(argv)
    stats = args.real if args.real.lower().endswith('.npz') else None
    fake_npy = args.fake.lower().endswith('.npy')
    knobs = dict(num_points=args.num_points, min_size=args.min_size, seed=args.seed, device=args.device)
    if stats is not None and fake_npy:      # statistics and features: no network is built
        mu, sigma = load_statistics(stats)
        inf = FIDInfinity(real_stats=(mu, sigma), dim=mu.size, **knobs)
    else:
        from .fid import FrechetInceptionDistance
        from .inception import inception_network
        net = inception_network(args.weights, torch.device(args.device), 'FIDInfinity', True, 'distances are MEANINGLESS as FIDs')
        inf = FIDInfinity(real_stats=stats, dim=net.fc.in_features, **knobs)
        fid = FrechetInceptionDistance(weights=net, real_stats=stats, resize=True, batch_size=args.batch_size, device=args.device, sets=inf)
        prep = dict(image_size=args.image_size, resize_filter=args.resize_filter, device=fid.device)
        if stats is None:
            _feed_dir(fid.add_real, args.real, args.batch_size, **prep)
        if not fake_npy:
            _feed_dir(fid, args.fake, args.batch_size, **prep)
    if fake_npy:
        inf.add_features(torch.from_numpy(load_features(args.fake)).to(inf.device))
    res = inf.compute()
    for line in format_lines(res):
        print(line)
    return res


if __name__ == '__main__':
    main()
