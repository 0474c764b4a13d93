"""Kernel Inception Distance and improved precision / recall (with density / coverage) on device-resident Inception features.

    python -m scene_generation_amd.featsets --weights W --real DIR|FEATS.npy --fake DIR|FEATS.npy [--save_real OUT.npy] [--k 3]
                                            [--kid_subsets 100] [--kid_subset_size 1000] [--seed 0]
        -> KID mean std / Precision p Recall r / Density d Coverage c

FID (fid.py) keeps no feature, and at the ~1000 images of a validation pass it is strongly biased and needs a truncated form to be
defined at all.  These are the numbers made for that sample size, and they are statistics of all pairs of feature ROWS, so the rows
are kept -- on the device:

* ``FeatureBank``: float32 rows [N, dim] in a device buffer that doubles when full; ``update`` is one copy and no synchronisation.
* KID (Binkowski et al. 2018): the unbiased MMD^2 estimate with k(a, b) = (a.b / D + 1)^3 over ``kid_subsets`` subsets of
  ``kid_subset_size`` rows of each side, reported as mean and std over the subsets.  The subsets are drawn on the host before the
  first launch; ``ops.feat_poly_sums`` gathers the rows through the tables and returns three sums per subset; ``kid_from_sums`` is the
  host's float64 arithmetic on those 3 S numbers.
* Improved precision / recall (Kynkaanniemi et al. 2019, k = 3) and density / coverage (Naeem et al. 2020): ``ops.feat_knn_radius``
  gives each row's squared distance to its k-th nearest other row; ``ops.feat_manifold_counts`` counts, per query, the reference balls
  that hold it, and finds each reference's nearest query.  One pass with the real side as reference gives precision, density and
  coverage; one with the fake side as reference gives recall.
* Only ``compute()`` synchronises: it reads back the [S, 3] sums, two count vectors and one vector of flags, never a feature.
* ``FrechetInceptionDistance(sets=...)`` hands the pooled features it computes to a ``FeatureSetMetrics`` too (one Inception forward
  for every number); ``check_model(fid=f)`` then fills it and the caller reads ``f.sets.compute()``.
"""
import argparse

import numpy as np
import torch

from . import ops
from .evalkit import grow_rows
from .imageprep import _feed_dir, add_arguments
from .inception import inception_network, pooled_features

__all__ = ['FeatureBank', 'FeatureSetMetrics', 'draw_subsets', 'kid_from_sums', 'manifold_metrics', 'load_features', 'main']

KID_DEGREE, KID_COEF0 = 3, 1.0


class FeatureBank(object):
    """float32 feature rows [count, dim] on ``device``, in a buffer that doubles when full"""

    def __init__(self, dim=2048, device='cuda', capacity=1024):
        self.dim, self.device = int(dim), torch.device(device)
        self.buf = torch.empty(max(int(capacity), 1), self.dim, dtype=torch.float32, device=self.device)
        self.count = 0

    def clean(self):
        self.count = 0

    def update(self, feats):
        """append the rows of ``feats`` (float32 [rows, dim]): one copy, no synchronisation"""
        if feats.dim() != 2 or feats.size(1) != self.dim:
            raise ValueError('FeatureBank.update: rows of %d dimensions, got %s' % (self.dim, tuple(feats.shape)))
        if feats.dtype != torch.float32:
            raise TypeError('FeatureBank.update: features must be float32, got %s' % feats.dtype)
        rows = int(feats.size(0))
        self.buf = grow_rows(self.buf, self.count, rows, 1, (self.dim,), torch.float32, self.device)     # (the capacity is never 0)
        self.buf[self.count:self.count + rows].copy_(feats.detach())
        self.count += rows

    def merge(self, other):
        """append another bank's rows (the building block of a gather across ranks)"""
        if other.dim != self.dim:
            raise ValueError('FeatureBank.merge: %d against %d dimensions' % (other.dim, self.dim))
        self.update(other.rows().to(self.device))
        return self

    def rows(self):
        """the rows held, a view [count, dim] of the buffer"""
        return self.buf[:self.count]

    def save(self, path):
        """``.npy``, float32 [count, dim] (a read-back: for the real side's file, not part of an evaluation)"""
        with open(path, 'wb') as f:
            np.save(f, self.rows().cpu().numpy())

    @classmethod
    def load(cls, path, device='cuda'):
        feats = load_features(path)
        bank = cls(feats.shape[1], device, capacity=max(feats.shape[0], 1))
        bank.update(torch.from_numpy(feats).to(bank.device))
        return bank


def load_features(path):
    """float32 [N, dim] of an ``.npy`` file (``FeatureBank.save``)"""
    feats = np.load(path)
    if feats.ndim != 2 or not np.issubdtype(feats.dtype, np.floating):
        raise ValueError('%s: %s %s is not a [N, dim] array of features' % (path, feats.dtype, feats.shape))
    return np.ascontiguousarray(feats, dtype=np.float32)


# ---- the host's share -----------------------------------------------------------------------------------------------------------------
def draw_subsets(seed, subsets, size, n_real, n_fake):
    """(ix [subsets, size], iy [subsets, size]) int32: per subset ``size`` distinct rows of each side, drawn from
    ``numpy.random.RandomState(seed)`` in the order real, fake, real, ... -- on the host, before the first launch"""
    if size < 1 or size > min(n_real, n_fake) or subsets < 1:
        raise ValueError('draw_subsets: %d subsets of %d rows from %d and %d' % (subsets, size, n_real, n_fake))
    rs = np.random.RandomState(seed)
    ix, iy = np.empty((subsets, size), np.int32), np.empty((subsets, size), np.int32)
    for q in range(subsets):
        ix[q] = rs.permutation(n_real)[:size]
        iy[q] = rs.permutation(n_fake)[:size]
    return ix, iy


def kid_from_sums(sums, size):
    """(mean, std) over subsets of Sxx / (s (s - 1)) + Syy / (s (s - 1)) - 2 Sxy / s^2, float64; ``sums`` [S, 3] = (Sxx, Syy, Sxy)
    with the diagonal left out of the first two.  std is the population form (numpy.std), 0 for one subset."""
    sums = np.asarray(sums, np.float64).reshape(-1, 3)
    s = float(size)
    if size < 2:
        raise ValueError('kid_from_sums: the unbiased estimate needs subsets of at least 2 rows, got %d' % size)
    per = sums[:, 0] / (s * (s - 1.0)) + sums[:, 1] / (s * (s - 1.0)) - 2.0 * sums[:, 2] / (s * s)
    return float(per.mean()), float(per.std())


def manifold_metrics(count_fake, count_real, covered, k):
    """{'precision', 'recall', 'density', 'coverage'} from ``count_fake`` [m] (real balls holding each fake row), ``count_real`` [n]
    (fake balls holding each real row) and ``covered`` [n] (a fake row lies in the real row's ball)"""
    count_fake, count_real, covered = np.asarray(count_fake), np.asarray(count_real), np.asarray(covered)
    return {'precision': float((count_fake > 0).mean()), 'recall': float((count_real > 0).mean()),
            'density': float(count_fake.astype(np.float64).sum() / (float(k) * count_fake.size)), 'coverage': float(covered.astype(bool).mean())}


# ---- the object -----------------------------------------------------------------------------------------------------------------------
class FeatureSetMetrics(object):
    """KID and precision / recall / density / coverage between a real and a fake set of images, on the pooled Inception features.

    ``weights``: as ``FrechetInceptionDistance``; the network is built on first use by ``__call__`` / ``add_real`` only -- an object fed
    through ``add_features`` / ``add_real_features`` (attached to a ``FrechetInceptionDistance(sets=...)``) never builds one.
    ``real_features``: an ``.npy`` path, an array or a tensor [N, dim] that fixes the real side; None: fed through ``add_real``.

    The feeding surface is ``FrechetInceptionDistance``'s: ``__call__(imgs)`` / ``add_features(f)`` add to the fake side,
    ``add_real(imgs)`` / ``add_real_features(f)`` to the real one, ``clean()`` clears the fake side, ``clean_real()`` the real one,
    ``needs_real`` says whether the real side is still open (the first ``compute()`` closes it).  ``compute()`` -> dict; no other call
    synchronises.  The real side's radii are kept until the real side changes."""

    def __init__(self, weights=None, real_features=None, k=3, kid_subsets=100, kid_subset_size=1000, seed=0, resize=True, batch_size=32,
                 device=None, dim=None):
        assert batch_size > 0
        if not 1 <= int(k) <= ops.KNN_MAX:
            raise ValueError('FeatureSetMetrics: k = %r is outside 1..%d' % (k, ops.KNN_MAX))
        if int(kid_subsets) < 1 or int(kid_subset_size) < 2:
            raise ValueError('FeatureSetMetrics: kid_subsets >= 1 and kid_subset_size >= 2, got %r and %r' % (kid_subsets, kid_subset_size))
        self.k, self.kid_subsets, self.kid_subset_size, self.seed = int(k), int(kid_subsets), int(kid_subset_size), seed
        self.resize, self.batch_size, self.device = resize, batch_size, torch.device(device if device is not None else 'cuda')
        self._weights, self.inception_model = weights, None
        if isinstance(weights, torch.nn.Module):
            dim = weights.fc.in_features
        self.dim = int(dim) if dim is not None else 2048
        self.fake = FeatureBank(self.dim, self.device)
        self._real_fixed, self._real_open, self._real_r2 = False, True, None
        if real_features is not None:
            if isinstance(real_features, str):
                real_features = load_features(real_features)
            feats = torch.as_tensor(real_features)
            if feats.dim() != 2 or feats.size(1) != self.dim:
                raise ValueError('FeatureSetMetrics: real features %s for features of %d dimensions' % (tuple(feats.shape), self.dim))
            self.real = FeatureBank(self.dim, self.device, capacity=max(int(feats.size(0)), 1))
            self.real.update(feats.to(self.device, torch.float32))
            self._real_fixed, self._real_open = True, False
        else:
            self.real = FeatureBank(self.dim, self.device)

    # ---- feeding ------------------------------------------------------------------------------------------------------------------------
    @property
    def needs_real(self):
        return self._real_open

    @property
    def real_fixed(self):
        """the real side was given by ``real_features`` and takes no more rows"""
        return self._real_fixed

    def _network(self):
        if self.inception_model is None:
            net = inception_network(self._weights, self.device, 'FeatureSetMetrics', True,
                                    'numbers are MEANINGLESS as KID / precision / recall')
            if net.fc.in_features != self.dim:
                raise ValueError('FeatureSetMetrics: a network of %d features for banks of %d' % (net.fc.in_features, self.dim))
            self.inception_model = net
        return self.inception_model

    def _features(self, imgs):
        return pooled_features(self._network(), imgs, self.batch_size, self.resize, self.device)

    def add_features(self, feats):
        """pooled features [rows, dim] of fake images"""
        self.fake.update(feats)

    def add_real_features(self, feats):
        """pooled features [rows, dim] of real images"""
        if self._real_fixed:
            raise RuntimeError('FeatureSetMetrics.add_real_features: the real side is fixed by real_features')
        self._real_r2 = None
        self.real.update(feats)

    def __call__(self, imgs):
        for f in self._features(imgs):
            self.fake.update(f)

    def add_real(self, imgs):
        if self._real_fixed:
            raise RuntimeError('FeatureSetMetrics.add_real: the real side is fixed by real_features')
        for f in self._features(imgs):
            self.add_real_features(f)

    def clean(self):
        self.fake.clean()

    def clean_real(self):
        if self._real_fixed:
            raise RuntimeError('FeatureSetMetrics.clean_real: the real side is fixed by real_features')
        self.real.clean()
        self._real_r2, self._real_open = None, True

    # ---- the numbers --------------------------------------------------------------------------------------------------------------------
    def _check_counts(self):
        need = max(self.k + 1, 2)
        for name, bank in (('real', self.real), ('fake', self.fake)):
            if bank.count < 2:
                raise ValueError('FeatureSetMetrics: the %s side holds %d rows; KID needs at least 2' % (name, bank.count))
            if bank.count < need:
                raise ValueError('FeatureSetMetrics: the %s side holds %d rows; the k = %d nearest-neighbour radius needs at least '
                                 'k + 1 = %d' % (name, bank.count, self.k, self.k + 1))

    def subset_size(self):
        """``kid_subset_size`` clamped to the smaller side"""
        return min(self.kid_subset_size, self.real.count, self.fake.count)

    def real_radii(self):
        if self._real_r2 is None:           # the real side does not change between evaluations: its radii are kept
            self._real_r2 = ops.feat_knn_radius(self.real.rows(), self.k)
        return self._real_r2

    def compute(self):
        self._check_counts()
        n, m = self.real.count, self.fake.count
        size = self.subset_size()
        ix, iy = draw_subsets(self.seed, self.kid_subsets, size, n, m)          # on the host, before the first launch
        real, fake = self.real.rows(), self.fake.rows()
        sums = ops.feat_poly_sums(real, fake, ix, iy, 1.0 / self.dim, KID_COEF0, KID_DEGREE)
        r2_real = self.real_radii()
        r2_fake = ops.feat_knn_radius(fake, self.k)
        count_fake, mind2_real = ops.feat_manifold_counts(real, r2_real, fake)      # precision, density, coverage
        count_real, _ = ops.feat_manifold_counts(fake, r2_fake, real)               # recall
        covered = mind2_real <= r2_real
        self._real_open = False
        mean, std = kid_from_sums(sums.cpu().numpy(), size)                         # the read-back: 3 S doubles, two counts, n flags
        out = {'kid_mean': mean, 'kid_std': std, 'kid_subset_size': size}
        out.update(manifold_metrics(count_fake.cpu().numpy(), count_real.cpu().numpy(), covered.cpu().numpy(), self.k))
        out.update(real=n, fake=m)
        return out


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def format_lines(res):
    """the three lines every front end prints"""
    return ['KID {} {}'.format(res['kid_mean'], res['kid_std']), 'Precision {} Recall {}'.format(res['precision'], res['recall']),
            'Density {} Coverage {}'.format(res['density'], res['coverage'])]


def build_parser():
    p = argparse.ArgumentParser(prog='python -m scene_generation_amd.featsets',
                                description='Kernel Inception Distance and precision / recall / density / coverage between two sets of '
                                'images or of saved Inception features')
    p.add_argument('--weights', default=None, type=str, help='state_dict file of the Inception network (never downloaded); needed '
                   'for a directory of images; only pt_inception-2015-12-05-*.pth gives numbers comparable with published ones')
    p.add_argument('--real', required=True, type=str, help='a directory of images, or an .npy of features [N, dim]')
    p.add_argument('--fake', required=True, type=str, help='a directory of images, or an .npy of features [N, dim]')
    p.add_argument('--save_real', default=None, type=str, help='write the features of --real to this .npy')
    p.add_argument('--k', default=3, type=int, help='neighbour of the manifold radius')
    p.add_argument('--kid_subsets', default=100, type=int)
    p.add_argument('--kid_subset_size', default=1000, type=int)
    p.add_argument('--seed', default=0, type=int)
    p.add_argument('--batch_size', default=32, type=int)
    p.add_argument('--device', default='cuda', type=str)
    return add_arguments(p)


def main(argv=None):
    args = build_parser().parse_args(argv)
    real_npy, fake_npy = args.real.lower().endswith('.npy'), args.fake.lower().endswith('.npy')
    sets = FeatureSetMetrics(weights=args.weights, real_features=args.real if real_npy else None, k=args.k,
                             kid_subsets=args.kid_subsets, kid_subset_size=args.kid_subset_size, seed=args.seed, resize=True,
                             batch_size=args.batch_size, device=args.device)
    prep = dict(image_size=args.image_size, resize_filter=args.resize_filter, device=sets.device)
    if not real_npy:
        _feed_dir(sets.add_real, args.real, args.batch_size, **prep)
    if args.save_real:
        sets.real.save(args.save_real)
    if fake_npy:
        sets.add_features(torch.from_numpy(load_features(args.fake)).to(sets.device))
    else:
        _feed_dir(sets, args.fake, args.batch_size, **prep)
    res = sets.compute()
    for line in format_lines(res):
        print(line)
    return res


if __name__ == '__main__':
    main()
