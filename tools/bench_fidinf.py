"""Benchmark of FID-infinity (scene_generation_amd/fidinf.py, csrc/fidinf.hip) on cuda:0 at the validation pass's shape: N = 1000
fake rows of D = 2048 dimensions, 15 subset sizes.  One JSON line, appended to profiles/fidinf_bench.jsonl (or --out):

* ``fid_infinity_ms``: the wall time of ``fidinf.fid_infinity`` as a user meets it (host clock: the two kernels, the read-back of one
  n_q x n_q block per subset and the host's ``eigvalsh`` of each), the median of ``--runs`` runs after one warm-up.
* ``parent_route_ms``: the same 15 subset FIDs by the route the tree had before: per subset the rows gathered on the device,
  ``FeatureMoments`` over them, ``statistics()`` and ``frechet_distance`` against the real statistics, the square root of the real
  covariance computed once and handed to every call (as ``FrechetInceptionDistance`` keeps it) and counted.  One run.
* ``grams`` / ``subset_terms``: the device time of the two entry points (tools/bench_fid.py's method: the median of blocks by the host
  clock around a synchronise, the same launches between two device events next to it).  The f64 rate of the first is that of the
  FLOPs it EXECUTES, ``2 * 64 * 64 * D`` per 64 x 64 tile over the tiles of Y and the upper tile pairs of P and G -- the count
  tools/bench_fid.py uses for ``sg_fid_moments_update`` (the triangle), so the two rates compare; the FLOPs of the full squares
  (``alg_flops``) are recorded next to it.
* ``max_rel_difference``: the largest relative difference between the two routes' 15 values.

The one condition: the new route must be faster than the parent's at this shape (asserted at the end, after the line is written)."""
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
from scene_generation_amd import fidinf as FI  # noqa: E402
from scene_generation_amd import ops  # noqa: E402
from tools.benchkit import emit, measure, require_device  # noqa: E402

DEV = 'cuda:0'


def parent_route(rows, mu, sigma, idx, sizes):
    """the subset FIDs through the D x D moments and two 2048 x 2048 eigen-decompositions each (one of them shared)"""
    root = FID.psd_sqrt(sigma)
    out = []
    for q, s in enumerate(sizes):
        mom = FID.FeatureMoments(rows.size(1), rows.device)
        mom.update(rows[torch.from_numpy(idx[q, :s].astype(np.int64)).to(rows.device)])
        mu2, sigma2 = mom.statistics()
        out.append(FID.frechet_distance(mu, sigma, mu2, sigma2, root1=root))
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--rows', type=int, default=1000)
    p.add_argument('--real_rows', type=int, default=5000)
    p.add_argument('--dim', type=int, default=2048)
    p.add_argument('--num_points', type=int, default=15)
    p.add_argument('--runs', type=int, default=3)
    p.add_argument('--seconds', type=float, default=0.5)
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fidinf_bench.jsonl'))
    args = p.parse_args(argv)
    require_device()
    N, D = args.rows, args.dim
    g = torch.Generator(device=DEV).manual_seed(1)
    real = FID.FeatureMoments(D, DEV)
    for a in range(0, args.real_rows, 500):
        real.update(torch.relu(torch.randn(min(500, args.real_rows - a), D, device=DEV, generator=g)))
    mu, sigma = real.statistics()
    rows = torch.relu(torch.randn(N, D, device=DEV, generator=g) * 1.1 + 0.1)

    FI.fid_infinity(rows, mu, sigma, num_points=args.num_points)                    # warm-up: the workspace, the BLAS threads
    torch.cuda.synchronize()
    times = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        res = FI.fid_infinity(rows, mu, sigma, num_points=args.num_points)
        times.append((time.perf_counter() - t0) * 1e3)

    idx, sizes = FI.draw_subsets(0, FI.draw_sizes(N, args.num_points), N)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parent = parent_route(rows, mu, sigma, idx, sizes)
    parent_ms = (time.perf_counter() - t0) * 1e3
    diff = float(np.max(np.abs(np.array(parent) - np.array(res['fids'])) / np.abs(np.array(parent))))

    dmu, dsigma = torch.from_numpy(mu.copy()).to(DEV), torch.from_numpy(sigma.copy()).to(DEV)
    P, G = ops.fidinf_grams(rows, dmu, dsigma)
    rg = measure(lambda: ops.fidinf_grams(rows, dmu, dsigma, P=P, G=G), args.seconds, args.blocks, clocks=True)
    didx, dsz = idx, sizes
    M, sums = ops.fidinf_subset_terms(P, G, didx, dsz)
    rt = measure(lambda: ops.fidinf_subset_terms(P, G, didx, dsz, M=M, sums=sums), args.seconds, args.blocks,
                 clocks=True)                                       # (the table upload included)
    flops = 2.0 * N * D * D + 2.0 * 2.0 * N * N * D             # Y, then P and G over the full square
    nt, ntd = (N + 63) // 64, (D + 63) // 64
    done = 2.0 * 64 * 64 * D * (nt * ntd + 2 * (nt * (nt + 1) // 2))      # what the kernels execute: whole tiles, the upper pairs only
    rec = {'figure': 'fid_infinity', 'device': torch.cuda.get_device_name(0), 'rows': N, 'dim': D, 'num_points': len(sizes),
           'sizes': [int(s) for s in sizes], 'host_threads': torch.get_num_threads(), 'numpy': np.__version__,
           'fid_infinity_ms': statistics.median(times), 'fid_infinity_runs_ms': times, 'parent_route_ms': parent_ms,
           'parent_over_new': parent_ms / statistics.median(times), 'max_rel_difference': diff, 'fid_inf': res['fid_inf'],
           'fid_n': res['fid'], 'subset_terms': rt,
           'grams': dict(rg, alg_flops=flops, executed_flops=done, f64_gflops=done / (rg['ms'] * 1e-3) / 1e9)}
    emit(args.out, rec)
    assert rec['fid_infinity_ms'] < parent_ms, 'the n x n route (%.0f ms) is not faster than the D x D route (%.0f ms)' % (
        rec['fid_infinity_ms'], parent_ms)


if __name__ == '__main__':
    main()
