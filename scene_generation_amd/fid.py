"""The Frechet Inception Distance: the fourth value of ``evaluate.check_model`` (the reference leaves it None, train.py:81).

    python -m scene_generation_amd.fid --weights W --real DIR|STATS.npz --fake DIR [--save_stats OUT.npz] [--save_features OUT.npy]
                                       [--batch_size 32] [--image_size H,W [--resize_filter bilinear|bicubic]]   -> FID x

* ``FeatureMoments``: count, sum and the upper triangle of the outer-product sum of feature rows, float64, on the device
  (sg_fid_moments_update on the f64 matrix cores: one launch per batch, no feature is kept or read back).  ``statistics()`` is one
  finalize launch and one device-to-host copy of ``(mu, sigma)``.  8 D^2 + 8 D bytes per side: 32 MB at D = 2048.
* ``frechet_distance``: |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2 on the host in float64, the trace term by the symmetric
  form with rank truncation, so that it is right for the rank-deficient covariances an evaluation over ~1000 images of 2048
  dimensions always has.
* ``FrechetInceptionDistance``: the object ``check_model``, ``Sampler`` and ``InceptionScore(fid=...)`` drive.
* Published FIDs come from ONE network: the TF-ported pt_inception-2015-12-05 weights in the FID form of ``InceptionV3``
  (``load_inception`` recognises the file by its 1008 classes).  Any other weights give a distance, not a number that compares with
  a paper's.  Nothing is ever downloaded: ``weights`` is a local file.
"""
import argparse

import numpy as np
import torch

from . import ops
from .featsets import FeatureBank
from .imageprep import _feed_dir, add_arguments
from .inception import inception_network, pooled_features

__all__ = ['FeatureMoments', 'FrechetInceptionDistance', 'frechet_distance', 'load_statistics', 'main']


class FeatureMoments(object):
    """raw float64 moments of feature rows [*, dim] on ``device``: ``count`` (a host int), ``sum`` [dim], ``outer`` [dim, dim] (its
    upper triangle; the lower one is unspecified).  No shift: moments of two accumulators add (``merge``)."""

    def __init__(self, dim=2048, device='cuda'):
        self.dim, self.device = int(dim), torch.device(device)
        self.sum = torch.zeros(self.dim, dtype=torch.float64, device=self.device)
        self.outer = torch.zeros(self.dim, self.dim, dtype=torch.float64, device=self.device)
        self.count = 0

    def clean(self):
        self.sum.zero_()
        self.outer.zero_()
        self.count = 0

    def update(self, feats):
        """add the rows of ``feats`` (float32 [rows, dim], on the device): one launch, no synchronisation"""
        ops.fid_moments_update(feats, self.sum, self.outer)
        self.count += int(feats.size(0))

    def merge(self, other):
        """add another accumulator's rows (the building block of a reduction across ranks)"""
        if other.dim != self.dim:
            raise ValueError('FeatureMoments.merge: %d against %d dimensions' % (other.dim, self.dim))
        self.sum += other.sum.to(self.device)
        self.outer += other.outer.to(self.device)
        self.count += other.count
        return self

    def statistics(self):
        """-> (mu [dim], sigma [dim, dim]) float64 NumPy arrays: one finalize launch and the one device-to-host copy"""
        if self.count < 2:
            raise ValueError('FeatureMoments.statistics: a covariance needs at least 2 rows, got %d' % self.count)
        flat = torch.empty(self.dim + self.dim * self.dim, dtype=torch.float64, device=self.device)
        ops.fid_moments_finalize(self.sum, self.outer, self.count, out=flat)
        host = flat.cpu().numpy()
        return host[:self.dim], host[self.dim:].reshape(self.dim, self.dim)

    def save(self, path):
        """``.npz`` with ``mu`` and ``sigma`` (the layout of pytorch-fid's precomputed statistics) and the row count ``n``"""
        mu, sigma = self.statistics()
        np.savez(path, mu=mu, sigma=sigma, n=np.int64(self.count))


def load_statistics(path):
    """(mu, sigma) float64 of an ``.npz`` that holds ``mu`` and ``sigma`` (``FeatureMoments.save``, or pytorch-fid's files)"""
    with np.load(path) as f:
        mu, sigma = np.asarray(f['mu'], np.float64), np.asarray(f['sigma'], np.float64)
    if mu.ndim != 1 or sigma.shape != (mu.size, mu.size):
        raise ValueError('%s: mu %s and sigma %s are not a mean and its covariance' % (path, mu.shape, sigma.shape))
    return mu, sigma


# ---- the distance ---------------------------------------------------------------------------------------------------------------------
def _truncate(lam):
    """eigenvalues at or below D * 2^-52 * lambda_max are rounding noise of a rank-deficient matrix: zero (their square roots, D of
    them, would otherwise add ~1e-8 of the trace)"""
    top = lam.max() if lam.size else 0.0
    return np.where(lam > lam.size * 2.0 ** -52 * top, lam, 0.0)


def psd_sqrt(sigma):
    """R = V diag(sqrt(lambda)) V^T of a symmetric positive semi-definite matrix, its eigenvalues truncated (``_truncate``)"""
    lam, V = np.linalg.eigh(np.asarray(sigma, np.float64))
    return (V * np.sqrt(_truncate(lam))) @ V.T


def _trace_sqrt_product(R1, sigma2):
    """tr (S1 S2)^1/2 = sum of the square roots of the eigenvalues of sym(R1 S2 R1), R1 = S1^1/2"""
    M = R1 @ np.asarray(sigma2, np.float64) @ R1
    lam = _truncate(np.linalg.eigvalsh(0.5 * (M + M.T)))
    return float(np.sqrt(lam).sum())


def frechet_distance(mu1, sigma1, mu2, sigma2, root1=None):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2 in float64 on the host.  The trace term: eigh(S1), eigenvalues
    <= D 2^-52 lambda_max set to zero, R = V diag(sqrt(lambda)) V^T, M = sym(R S2 R), eigvalsh(M), the same truncation, the sum of
    the square roots -- exact for rank-deficient covariances, where an unsymmetric matrix square root is not.  ``root1``: R of S1
    when the caller has it (``psd_sqrt``)."""
    mu1, mu2 = np.asarray(mu1, np.float64).reshape(-1), np.asarray(mu2, np.float64).reshape(-1)
    sigma1, sigma2 = np.asarray(sigma1, np.float64), np.asarray(sigma2, np.float64)
    D = mu1.size
    if mu2.size != D or sigma1.shape != (D, D) or sigma2.shape != (D, D):
        raise ValueError('frechet_distance: mu %s / %s and sigma %s / %s do not belong together'
                         % (mu1.shape, mu2.shape, sigma1.shape, sigma2.shape))
    R = root1 if root1 is not None else psd_sqrt(sigma1)
    d = mu1 - mu2
    return float(d @ d + np.trace(sigma1) + np.trace(sigma2) - 2.0 * _trace_sqrt_product(R, sigma2))


class FrechetInceptionDistance(object):
    """FID between a real and a fake set of images [N, 3, H, W] (resized to 299 x 299 on the device with ``resize``).  Both sets must
    arrive in the same normalisation; none is applied here.

    ``weights``: as ``InceptionScore`` -- a ``state_dict`` path (``load_inception``; the pt_inception file gives the FID form), an
    ``InceptionV3``, or None for ``inception.DEFAULT_WEIGHTS`` and, failing that, a seeded random network and a loud warning.
    ``real_stats``: an ``.npz`` path or a ``(mu, sigma)`` pair; None: the real side is accumulated through ``add_real``.

    ``__call__(imgs)`` adds to the fake side (``add_features(f)`` takes pooled features directly: ``InceptionScore(fid=...)``);
    ``clean()`` clears the fake side only, ``clean_real()`` the real one; ``needs_real`` says whether the real side still has to be
    fed (an accumulated real side is closed by the first ``compute()``: a validation pass feeds it once and later passes reuse it);
    ``compute()`` -> float.  No call but ``compute()`` synchronises.

    ``sets``: a ``featsets.FeatureSetMetrics`` (None: off, and nothing below runs).  Every pooled feature row this object sees is then
    also handed to it -- fake rows through ``add_features`` / ``__call__``, real rows through ``add_real`` -- so KID and precision /
    recall share this object's Inception forward; ``clean`` and ``clean_real`` clear its sides too.  The caller reads
    ``fid.sets.compute()``.  With ``real_stats`` the real rows never pass through here: the attached object must then hold its own
    (``FeatureSetMetrics(real_features=...)``)."""

    def __init__(self, weights=None, real_stats=None, resize=True, batch_size=32, device=None, sets=None):
        assert batch_size > 0
        self.sets = sets
        self.resize, self.batch_size, self.device = resize, batch_size, torch.device(device if device is not None else 'cuda')
        self.inception_model = inception_network(weights, self.device, 'FrechetInceptionDistance', True,
                                                 'distances are MEANINGLESS as FIDs')
        dim = self.inception_model.fc.in_features
        self.fake = FeatureMoments(dim, self.device)
        self.real, self._real_stats, self._real_open, self._root = None, None, False, None
        if real_stats is not None:
            mu, sigma = load_statistics(real_stats) if isinstance(real_stats, str) else real_stats
            mu, sigma = np.asarray(mu, np.float64).reshape(-1), np.asarray(sigma, np.float64)
            if mu.size != dim or sigma.shape != (dim, dim):
                raise ValueError('FrechetInceptionDistance: real statistics of %d dimensions for features of %d' % (mu.size, dim))
            self._real_stats = (mu, sigma)
        else:
            self.real = FeatureMoments(dim, self.device)
            self._real_open = True
        if sets is not None:
            if sets.dim != dim:
                raise ValueError('FrechetInceptionDistance: sets keeps features of %d dimensions, the network gives %d' % (sets.dim, dim))
            if (real_stats is not None) != bool(sets.real_fixed):
                raise ValueError('FrechetInceptionDistance: real_stats fixes the real side, so the attached FeatureSetMetrics needs '
                                 'real_features= (the rows the statistics were made of) -- and only then' if real_stats is not None else
                                 'FrechetInceptionDistance: the attached FeatureSetMetrics has real_features= but the real side here '
                                 'is fed through add_real; give real_stats= as well, or leave real_features out')

    # ---- feeding ------------------------------------------------------------------------------------------------------------------------
    @property
    def needs_real(self):
        return self._real_open

    def _features(self, imgs):
        return pooled_features(self.inception_model, imgs, self.batch_size, self.resize, self.device)

    def add_features(self, feats):
        """pooled features [rows, dim] of fake images (the entry ``InceptionScore(fid=...)`` uses)"""
        self.fake.update(feats)
        if self.sets is not None:
            self.sets.add_features(feats)

    def __call__(self, imgs):
        for f in self._features(imgs):
            self.add_features(f)

    def add_real(self, imgs):
        if self.real is None:
            raise RuntimeError('FrechetInceptionDistance.add_real: the real side is fixed by real_stats')
        self._real_stats, self._root = None, None
        for f in self._features(imgs):
            self.real.update(f)
            if self.sets is not None:
                self.sets.add_real_features(f)

    def clean(self):
        self.fake.clean()
        if self.sets is not None:
            self.sets.clean()

    def clean_real(self):
        if self.real is None:
            raise RuntimeError('FrechetInceptionDistance.clean_real: the real side is fixed by real_stats')
        self.real.clean()
        self._real_stats, self._root, self._real_open = None, None, True
        if self.sets is not None:
            self.sets.clean_real()

    # ---- the number ---------------------------------------------------------------------------------------------------------------------
    def real_statistics(self):
        if self._real_stats is None:
            if self.real.count < 2:
                raise ValueError('FrechetInceptionDistance: the real side holds %d rows; a covariance needs at least 2' % self.real.count)
            self._real_stats = self.real.statistics()
        return self._real_stats

    def compute(self):
        if self.fake.count < 2:
            raise ValueError('FrechetInceptionDistance: the fake side holds %d rows; a covariance needs at least 2' % self.fake.count)
        mu1, sigma1 = self.real_statistics()
        self._real_open = False
        if self._root is None:              # the real statistics do not change between evaluations: their square root is kept
            self._root = psd_sqrt(sigma1)
        mu2, sigma2 = self.fake.statistics()
        return frechet_distance(mu1, sigma1, mu2, sigma2, root1=self._root)


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog='python -m scene_generation_amd.fid',
                                description='Frechet Inception Distance between two sets of images (resized to 299 x 299 on the device)')
    p.add_argument('--weights', default=None, type=str, help='state_dict file of the Inception network (never downloaded); only '
                   'pt_inception-2015-12-05-*.pth gives numbers comparable with published FIDs')
    p.add_argument('--real', required=True, type=str, help='a directory of images, or an .npz with mu and sigma')
    p.add_argument('--fake', required=True, type=str, help='a directory of images')
    p.add_argument('--save_stats', default=None, type=str, help='write the statistics of --real (a directory) to this .npz')
    p.add_argument('--save_features', default=None, type=str, help='write the pooled features of --real (a directory) to this .npy: '
                   'the real side of python -m scene_generation_amd.featsets and of sample --real_features')
    p.add_argument('--batch_size', default=32, type=int)
    p.add_argument('--device', default='cuda', type=str)
    return add_arguments(p)


def main(argv=None):
    args = build_parser().parse_args(argv)
    stats = args.real if args.real.lower().endswith('.npz') else None
    if stats is not None and args.save_stats:
        raise SystemExit('--save_stats needs --real to be a directory of images')
    if stats is not None and args.save_features:
        raise SystemExit('--save_features needs --real to be a directory of images')
    fid = FrechetInceptionDistance(weights=args.weights, real_stats=stats, resize=True, batch_size=args.batch_size, device=args.device)
    prep = dict(image_size=args.image_size, resize_filter=args.resize_filter, device=fid.device)
    if stats is None:
        feed_real = fid.add_real
        if args.save_features:          # the rows are kept only on request: a plain run holds moments alone
            bank = FeatureBank(fid.fake.dim, fid.device)

            def feed_real(imgs):
                for f in fid._features(imgs):
                    fid.real.update(f)
                    bank.update(f)
        _feed_dir(feed_real, args.real, args.batch_size, **prep)
        if args.save_stats:
            fid.real.save(args.save_stats)
        if args.save_features:
            bank.save(args.save_features)
    _feed_dir(fid, args.fake, args.batch_size, **prep)
    value = fid.compute()
    print('FID {}'.format(value))
    return value


if __name__ == '__main__':
    main()
