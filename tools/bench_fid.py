"""Benchmark of the Frechet Inception Distance's own work (scene_generation_amd/fid.py, csrc/fid.hip) on cuda:0.

* ``moments_update``: one ``sg_fid_moments_update`` of ``--batch`` x 2048 features into the 2048 x 2048 float64 moments, with the
  bytes the algorithm moves (the read-modify-write of the upper triangle) over its time.
* ``moments_finalize``: one ``sg_fid_moments_finalize`` at 2048.
* ``statistics_and_distance``: the device-to-host copy of (mu, sigma) and ``frechet_distance`` on the host, the real side's square
  root cached as ``FrechetInceptionDistance`` caches it, and once without the cache.
* ``features_forward_299``: for scale, ``InceptionV3.features`` (the FID form) of ``--batch`` images at 299 x 299, and the update's
  share of it.

Every device figure: warmed up, then the median of ``--blocks`` blocks of at least ``--seconds`` each by the host clock around a
device synchronise, with the spread, and next to it the same launches between two device events; the shader and memory clocks the
driver reports are read before and after (sysfs, read only; null where the host does not show them).  Nothing is asserted.  One JSON
line per figure, appended to profiles/fid_bench.jsonl (or --out).  Random weights (the arithmetic does not depend on them)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from scene_generation_amd import fid as FID  # noqa: E402
from scene_generation_amd import inception as I  # noqa: E402
from scene_generation_amd import ops  # noqa: E402
from tools.benchkit import clocks, emit, measure, require_device  # noqa: E402

DEV = 'cuda:0'


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=32)
    p.add_argument('--dim', type=int, default=2048)
    p.add_argument('--seconds', type=float, default=0.5)
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--rows', type=int, default=256, help='rows per side of the distance that is timed')
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fid_bench.jsonl'))
    args = p.parse_args(argv)
    require_device()
    D = args.dim
    base = {'device': torch.cuda.get_device_name(0), 'batch': args.batch, 'dim': D}

    g = torch.Generator(device=DEV).manual_seed(1)
    mom = FID.FeatureMoments(D, DEV)
    x = torch.relu(torch.randn(args.batch, D, device=DEV, generator=g))
    tri_bytes = 16.0 * (D * (D + 1) / 2)                            # the upper triangle read and written, 8 bytes each way
    r = measure(lambda: ops.fid_moments_update(x, mom.sum, mom.outer), args.seconds, args.blocks, clocks=True)
    update_ms = r['ms']
    emit(args.out, dict(base, figure='moments_update', rows=args.batch, alg_bytes=tri_bytes + 4.0 * args.batch * D,
                        alg_gbytes_per_s=(tri_bytes + 4.0 * args.batch * D) / (r['ms'] * 1e-3) / 1e9,
                        f64_gflops=2.0 * args.batch * D * (D + 1) / 2 / (r['ms'] * 1e-3) / 1e9, **r))

    # moments of two sides for the finalize and the distance
    sides = []
    for k in range(2):
        m = FID.FeatureMoments(D, DEV)
        for a in range(0, args.rows, args.batch):
            m.update(torch.relu(torch.randn(min(args.batch, args.rows - a), D, device=DEV, generator=g) * (1.0 + 0.1 * k) + 0.1 * k))
        sides.append(m)
    flat = torch.empty(D + D * D, dtype=torch.float64, device=DEV)
    r = measure(lambda: ops.fid_moments_finalize(sides[0].sum, sides[0].outer, sides[0].count, out=flat), args.seconds, args.blocks,
                clocks=True)
    emit(args.out, dict(base, figure='moments_finalize', n=sides[0].count, alg_bytes=12.0 * D * D,
                        alg_gbytes_per_s=12.0 * D * D / (r['ms'] * 1e-3) / 1e9, **r))

    # the host part: copy + distance (host clock; the copy ends in a synchronise)
    mu1, s1 = sides[0].statistics()
    t0 = time.perf_counter()
    root = FID.psd_sqrt(s1)
    root_s = time.perf_counter() - t0
    copies, cached = [], []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mu2, s2 = sides[1].statistics()
        t1 = time.perf_counter()
        value = FID.frechet_distance(mu1, s1, mu2, s2, root1=root)
        t2 = time.perf_counter()
        copies.append((t1 - t0) * 1e3)
        cached.append((t2 - t1) * 1e3)
    t0 = time.perf_counter()
    cold = FID.frechet_distance(mu1, s1, mu2, s2)
    cold_ms = (time.perf_counter() - t0) * 1e3
    emit(args.out, dict(base, figure='statistics_and_distance', rows_per_side=args.rows, fid=value, fid_without_cached_root=cold,
                        finalize_and_copy_ms=statistics.median(copies), distance_cached_root_ms=statistics.median(cached),
                        distance_cold_ms=cold_ms, real_root_once_ms=root_s * 1e3, host_threads=torch.get_num_threads(),
                        numpy=np.__version__, clocks=clocks()))

    # for scale: the forward the update sits next to
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        net = I.InceptionV3(num_classes=I.FID_CLASSES, aux_logits=False, fid_variant=True).to(DEV)
    imgs = torch.rand(args.batch, 3, 299, 299, device=DEV) * 2 - 1
    r = measure(lambda: net.features(imgs), args.seconds, args.blocks, clocks=True)
    emit(args.out, dict(base, figure='features_forward_299', images_per_s=args.batch / (r['ms'] * 1e-3),
                        update_share_of_forward=update_ms / r['ms'], **r))


if __name__ == '__main__':
    main()
