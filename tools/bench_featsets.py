"""Benchmark of the feature-set metrics' own work (scene_generation_amd/featsets.py, csrc/featsets.hip) on cuda:0, at D = 2048.

* ``poly_sums``: one ``ops.feat_poly_sums`` of ``--subsets`` x ``--subset_size`` subsets (the table upload included: it is what
  ``FeatureSetMetrics.compute`` issues) at n = m = 1000 and 5000.  Algorithmic FLOPs: 2 D (s (s + 1) + s^2) per subset -- the
  symmetric sums over the upper triangle, the cross sum over the square.
* ``knn_radius`` (2 D n^2) and ``manifold_counts`` (2 D n m) at the same two sizes, k = 3.
* Next to each: its share of the Inception forward of the same number of images (n + m for the pair figures, n for the radii), from
  the ``features_forward_299`` record of profiles/fid_bench.jsonl, the ratio to the one f64 rate measured in this tree
  (``moments_update`` of the same file), and the time of the NumPy float64 restatement on this host's CPUs (the threads NumPy's BLAS
  is given: ``host_threads``).  The restatement of the kernel sums is timed over ``--numpy_subsets`` subsets and scaled to all of
  them (recorded as such).

The method is tools/bench_fid.py's: warmed up, the median of ``--blocks`` blocks of at least ``--seconds`` each by the host clock
around a device synchronise, with the spread, the same launches between two device events next to it, the clocks the driver reports
before and after.  Nothing is asserted.  One JSON line per figure, appended to profiles/featsets_bench.jsonl (or --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from scene_generation_amd import featsets as FS  # noqa: E402
from scene_generation_amd import ops  # noqa: E402
from tools.benchkit import emit, host_ms, measure, require_device  # noqa: E402

DEV = 'cuda:0'


def fid_bench_figures(path):
    """(images per second of the Inception forward, f64 GFLOP/s of sg_fid_moments_update) from profiles/fid_bench.jsonl, or Nones"""
    ips, gf = None, None
    if os.path.isfile(path):
        for line in open(path):
            rec = json.loads(line)
            if rec.get('figure') == 'features_forward_299':
                ips = rec['images_per_s']
            if rec.get('figure') == 'moments_update':
                gf = rec['f64_gflops']
    return ips, gf


def numpy_poly_sums(x, y, ix, iy, gamma, coef0):
    out = np.empty((ix.shape[0], 3))
    for q in range(ix.shape[0]):
        a, b = x[ix[q]], y[iy[q]]
        kxx, kyy, kxy = ((gamma * g + coef0) ** 3 for g in (a @ a.T, b @ b.T, a @ b.T))
        out[q] = kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum()
    return out


def numpy_dist2(a, b):
    return np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T), 0.0)


def numpy_knn_radius(x, k):
    d = numpy_dist2(x, x)
    np.fill_diagonal(d, np.inf)
    return np.partition(d, k - 1, axis=1)[:, k - 1]


def numpy_manifold_counts(a, r2, b):
    d = numpy_dist2(a, b)
    return (d <= r2[:, None]).sum(0), d.min(1)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--dim', type=int, default=2048)
    p.add_argument('--sizes', type=int, nargs='+', default=[1000, 5000])
    p.add_argument('--subsets', type=int, default=100)
    p.add_argument('--subset_size', type=int, default=1000)
    p.add_argument('--numpy_subsets', type=int, default=5)
    p.add_argument('--k', type=int, default=3)
    p.add_argument('--seconds', type=float, default=0.5)
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--fid_bench', default=os.path.join(ROOT, 'profiles', 'fid_bench.jsonl'))
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'featsets_bench.jsonl'))
    args = p.parse_args(argv)
    require_device()
    D, k = args.dim, args.k
    ips, ref_gflops = fid_bench_figures(args.fid_bench)
    base = {'device': torch.cuda.get_device_name(0), 'dim': D, 'host_threads': torch.get_num_threads(), 'numpy': np.__version__,
            'inception_images_per_s': ips, 'fid_moments_f64_gflops': ref_gflops}

    def derived(ms, flops, images, numpy_ms):
        gf = flops / (ms * 1e-3) / 1e9
        return {'alg_flops': flops, 'f64_gflops': gf, 'ratio_to_fid_moments_rate': gf / ref_gflops if ref_gflops else None,
                'share_of_inception_forward': ms / (images / ips * 1e3) if ips else None, 'numpy_f64_ms': numpy_ms,
                'numpy_over_device': numpy_ms / ms}

    g = torch.Generator(device=DEV).manual_seed(1)
    for n in args.sizes:
        x = torch.relu(torch.randn(n, D, device=DEV, generator=g))
        y = torch.relu(torch.randn(n, D, device=DEV, generator=g) * 1.1 + 0.1)
        hx, hy = x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
        s = min(args.subset_size, n)
        ix, iy = FS.draw_subsets(0, args.subsets, s, n, n)
        r = measure(lambda: ops.feat_poly_sums(x, y, ix, iy, 1.0 / D, 1.0, 3), args.seconds, args.blocks, clocks=True)
        q = min(args.numpy_subsets, args.subsets)
        np_ms = host_ms(lambda: numpy_poly_sums(hx, hy, ix[:q], iy[:q], 1.0 / D, 1.0))[0] * args.subsets / q
        emit(args.out, dict(base, figure='poly_sums', n=n, m=n, subsets=args.subsets, subset_size=s, numpy_subsets_timed=q,
                            **derived(r['ms'], 2.0 * D * args.subsets * (s * (s + 1.0) + s * s), 2 * n, np_ms), **r))

        r = measure(lambda: ops.feat_knn_radius(x, k), args.seconds, args.blocks, clocks=True)
        np_ms = host_ms(lambda: numpy_knn_radius(hx, k))[0]
        emit(args.out, dict(base, figure='knn_radius', n=n, k=k, **derived(r['ms'], 2.0 * D * n * n, n, np_ms), **r))

        r2 = ops.feat_knn_radius(x, k)
        hr2 = r2.cpu().numpy()
        r = measure(lambda: ops.feat_manifold_counts(x, r2, y), args.seconds, args.blocks, clocks=True)
        np_ms = host_ms(lambda: numpy_manifold_counts(hx, hr2, hy))[0]
        emit(args.out, dict(base, figure='manifold_counts', n=n, m=n, k=k, **derived(r['ms'], 2.0 * D * n * n, 2 * n, np_ms), **r))

    # the whole of compute() at the validation pass's size, as a user meets it (host clock, the read-back included)
    n = args.sizes[0]
    sets = FS.FeatureSetMetrics(real_features=torch.relu(torch.randn(n, D, device=DEV, generator=g)), k=k, kid_subsets=args.subsets,
                                kid_subset_size=args.subset_size, device=DEV, dim=D)
    sets.add_features(torch.relu(torch.randn(n, D, device=DEV, generator=g) * 1.1 + 0.1))
    sets.compute()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = sets.compute()
        times.append((time.perf_counter() - t0) * 1e3)
    emit(args.out, dict(base, figure='compute', n=n, m=n, k=k, subsets=args.subsets, subset_size=min(args.subset_size, n),
                        compute_ms=sorted(times)[1], share_of_inception_forward=sorted(times)[1] / (2 * n / ips * 1e3) if ips else None,
                        result=res))


if __name__ == '__main__':
    main()
