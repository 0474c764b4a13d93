"""IS-infinity (Chong & Forsyth, CVPR 2020): the Inception score extrapolated to an infinite number of generated images.

    python -m scene_generation_amd.isinf --weights W --dir DIR | --probs FILE.npy [--num_points 15] [--min_size n] [--seed 0]
                                         [--repeats 1] [--batch_size 32] [--image_size H,W [--resize_filter bilinear|bicubic]]
        -> IS_inf x / IS_N y N n

The Inception score of N images under-estimates the score of the generator: the plug-in entropy of the class marginal is biased by a
term that goes like (classes - 1) / (2 N), and a validation pass has N ~ 1000 images against 1000 classes -- several per cent, more
than the differences between the checkpoints the score is asked to rank.  IS-infinity evaluates the score on subsets of several sizes
n, fits a line in 1 / n and reports its intercept.

Everything it needs is what ``InceptionScore`` already holds on the device, the softmax rows.  ``ops.isinf_row_terms`` makes one pass
over them (each row's float64 sum and its entropy term), ``ops.isinf_subset_scores`` computes the score of every subset in one call --
a column reduction that gathers the rows through the subset table, with no gathered copy -- and the host reads back two numbers per
subset, once.  The definition is that of ``ops.inception_score`` with one split, so the full-set point is the existing score up to the
order of the sums.

* ``is_inf`` is the intercept of the line fitted to the scores (the paper's figure), ``is_inf_log`` the exponential of the intercept
  of the line fitted to the LOG scores: the leading bias of the plug-in entropy is exactly linear in 1 / n there.
* There is no row cap: nothing here is n x n (``fidinf`` has one because its Gram matrices are).
* The subset sizes and tables are those of ``fidinf`` (``draw_sizes``, ``draw_subsets``), the line is its ``extrapolate``.  The paper
  draws its sizes with Sobol points; that is NOT built, the sizes are evenly spaced.
* ``ISInfinity(scorer)`` wraps an ``InceptionScore``: after ``evaluate.check_model(...)`` has fed it, ``ISInfinity(scorer).compute()``
  is the extrapolated figure of that validation pass.
"""
import argparse

import numpy as np
import torch

from . import ops
from .fidinf import draw_sizes, draw_subsets, extrapolate
from .imageprep import _feed_dir, add_arguments

__all__ = ['ISInfinity', 'draw_tables', 'from_scores', 'is_infinity', 'check_count', 'format_lines', 'main']


# ---- the host's share -----------------------------------------------------------------------------------------------------------------
def draw_tables(n, num_points=15, min_size=None, seed=0, repeats=1):
    """(idx int32 [S, n], table_sizes int32 [S], point int [S], sizes): the subsets of one evaluation.  ``sizes`` are
    ``fidinf.draw_sizes(n, num_points, min_size)``; every size below ``n`` gets ``repeats`` subsets (``fidinf.draw_subsets`` under
    ``seed`` for the first, under ``[seed, r]`` for repeat r >= 1), the full set -- the identity order, nothing to draw -- one.  Row s
    of the table belongs to ``sizes[point[s]]``; the rows of the first draw come first, in the order of ``sizes``, so ``repeats=1`` is
    exactly the pair ``draw_subsets`` returns.

    ``min_size`` defaults to ``n // 2``: below n ~ classes the score's curve in 1 / n bends away from the line (classes that no row of
    a small subset supports drop out of the marginal's entropy altogether, a bias no term in 1 / n describes), and the upper half
    bends least -- the same choice, for the same kind of reason, as ``fidinf`` makes for n below the feature dimension."""
    n, repeats = int(n), int(repeats)
    if repeats < 1:
        raise ValueError('draw_tables: repeats = %d; at least 1' % repeats)
    sizes = draw_sizes(n, num_points, min_size)
    idx, tsz = draw_subsets(seed, sizes, n)
    tables, tsizes, point = [idx], [tsz], [np.arange(sizes.size)]
    below = np.flatnonzero(sizes < n)
    for r in range(1, repeats):
        if below.size:
            more, msz = draw_subsets([seed, r], sizes[below], n)
            pad = np.zeros((more.shape[0], n), np.int32)
            pad[:, :more.shape[1]] = more
            tables.append(pad)
            tsizes.append(msz)
            point.append(below)
    return np.concatenate(tables), np.concatenate(tsizes).astype(np.int32), np.concatenate(point), sizes


def from_scores(sizes, point, out, n):
    """the result dict from the read-back ``out`` [S, 2] = {log score, score} of the subsets of ``draw_tables``: per size the mean of
    its subsets' scores (and of their log scores), then the two lines"""
    out = np.asarray(out, np.float64).reshape(-1, 2)
    sizes, point = np.asarray(sizes), np.asarray(point)
    if out.shape[0] != point.size:
        raise ValueError('from_scores: %d results for %d subsets' % (out.shape[0], point.size))
    count = np.bincount(point, minlength=sizes.size).astype(np.float64)
    logs = np.bincount(point, weights=out[:, 0], minlength=sizes.size) / count
    scores = np.bincount(point, weights=out[:, 1], minlength=sizes.size) / count
    last = np.flatnonzero(point == sizes.size - 1)
    if sizes[-1] == n and last.size == 1:                   # the full set is one subset: its score as it was computed, no averaging
        logs[-1], scores[-1] = out[last[0]]
    intercept, slope = extrapolate(sizes, scores)
    log_intercept, _ = extrapolate(sizes, logs)
    return {'is_inf': intercept, 'is_inf_log': float(np.exp(log_intercept)), 'is': float(scores[-1]), 'slope': slope,
            'sizes': [int(s) for s in sizes], 'scores': [float(s) for s in scores], 'images': int(n)}


def check_count(n, num_points=15, min_size=None):
    """ValueError when ``is_infinity`` would refuse ``n`` rows (too few for two subset sizes): for a caller that knows the count
    before it starts the work"""
    draw_sizes(n, num_points, min_size)


def is_infinity(probs, num_points=15, min_size=None, seed=0, repeats=1):
    """{'is_inf', 'is_inf_log', 'is', 'slope', 'sizes', 'scores', 'images'}: the Inception score of ``probs`` (float32 [N, classes]
    softmax rows on the device: ``InceptionScore.rows()``) on ``num_points`` subset sizes from ``min_size`` (default N // 2, see
    ``draw_tables``) to N, and the intercepts of their lines in 1 / n.  'is_inf' is the intercept of the scores' line and 'slope' its
    slope; 'is_inf_log' is exp of the intercept of the log scores' line; 'is' is the score of all N rows, the last point; 'sizes' and
    'scores' are lists.  ``repeats`` > 1 draws that many subsets per size below N and averages their scores before the fit; the full
    set is computed once.  Any number of rows.  One host read: the [S, 2] result."""
    if not isinstance(probs, torch.Tensor) or probs.dim() != 2:
        raise ValueError('is_infinity: softmax rows [N, classes], got %s' % (tuple(probs.shape) if isinstance(probs, torch.Tensor)
                                                                              else type(probs),))
    n = int(probs.size(0))
    idx, tsizes, point, sizes = draw_tables(n, num_points, min_size, seed, repeats)          # on the host, before the first launch
    rs, h = ops.isinf_row_terms(probs)
    out = ops.isinf_subset_scores(probs, rs, h, idx, tsizes)
    return from_scores(sizes, point, out.cpu().numpy(), n)                                   # the read-back


# ---- the object -----------------------------------------------------------------------------------------------------------------------
class ISInfinity(object):
    """IS-infinity on the softmax rows an ``inception.InceptionScore`` holds: ``ISInfinity(scorer, **knobs).compute()`` -> the dict of
    ``is_infinity`` over ``scorer.rows()``.  The knobs are those of ``is_infinity`` (num_points, min_size, seed, repeats).  Nothing is
    copied and the scorer is not changed; only ``compute()`` synchronises."""

    def __init__(self, scorer, num_points=15, min_size=None, seed=0, repeats=1):
        if not callable(getattr(scorer, 'rows', None)):
            raise TypeError('ISInfinity: an inception.InceptionScore (anything with rows()), got %s' % type(scorer).__name__)
        self.scorer, self.num_points, self.min_size, self.seed, self.repeats = scorer, int(num_points), min_size, seed, int(repeats)

    def compute(self):
        return is_infinity(self.scorer.rows(), self.num_points, self.min_size, self.seed, self.repeats)


def format_lines(res):
    """the two lines every front end ends with"""
    return ['IS_inf {}'.format(res['is_inf']), 'IS_N {} N {}'.format(res['is'], res['images'])]


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def load_probs(path):
    """float32 [N, classes] from the .npy ``python -m scene_generation_amd.inception --save_probs`` writes"""
    rows = np.load(path, allow_pickle=False)
    if rows.ndim != 2 or rows.shape[1] < 1 or not np.issubdtype(rows.dtype, np.floating):
        raise ValueError('%s: softmax rows [N, classes] of a floating type, got %s %s' % (path, rows.dtype, rows.shape))
    return np.ascontiguousarray(rows, dtype=np.float32)


def build_parser():
    p = argparse.ArgumentParser(prog='python -m scene_generation_amd.isinf',
                                description='IS-infinity: the Inception score of a set of images extrapolated to an infinite number of '
                                'them')
    p.add_argument('--weights', default=None, type=str, help='state_dict file of torchvision\'s inception_v3 (never downloaded); needed '
                   'for --dir')
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument('--dir', default=None, type=str, help='a directory of images (resized to 299 x 299 on the device)')
    src.add_argument('--probs', default=None, type=str, help='an .npy of softmax rows [N, classes] (python -m '
                     'scene_generation_amd.inception --save_probs): no network is built')
    p.add_argument('--num_points', default=15, type=int, help='subset sizes on the line')
    p.add_argument('--min_size', default=None, type=int, help='smallest subset (default: half the images)')
    p.add_argument('--seed', default=0, type=int)
    p.add_argument('--repeats', default=1, type=int, help='subsets drawn per size below N; their scores are averaged')
    p.add_argument('--batch_size', default=32, type=int)
    p.add_argument('--device', default='cuda', type=str)
    return add_arguments(p)


def main(argv=None):
    args = build_parser().parse_args(argv)
    knobs = dict(num_points=args.num_points, min_size=args.min_size, seed=args.seed, repeats=args.repeats)
    if args.probs is not None:
        res = is_infinity(torch.from_numpy(load_probs(args.probs)).to(args.device), **knobs)
    else:
        from .inception import InceptionScore, find_images
        if not find_images(args.dir):               # said before a network is built
            raise SystemExit('no images under %s' % args.dir)
        scorer = InceptionScore(batch_size=args.batch_size, resize=True, weights=args.weights, device=args.device)
        _feed_dir(scorer, args.dir, args.batch_size, image_size=args.image_size, resize_filter=args.resize_filter, device=scorer.device)
        res = ISInfinity(scorer, **knobs).compute()
    for line in format_lines(res):
        print(line)
    return res


if __name__ == '__main__':
    main()
