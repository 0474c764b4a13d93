"""Benchmark of IS-infinity (scene_generation_amd/isinf.py, csrc/isinf.hip) on cuda:0 at the two shapes it has to serve: N = 1000
softmax rows (a validation pass) and N = 50 000 (the paper's setting), 1000 classes, 15 subset sizes.  One JSON line per shape,
appended to profiles/isinf_bench.jsonl (or --out):

* ``is_infinity_ms``: the wall time of ``isinf.is_infinity`` as a user meets it (host clock: the subset tables drawn on the host, their
  upload, the two entry points and the read-back of the [S, 2] result), the median of ``--runs`` runs after one warm-up.
* ``row_terms`` / ``subset_scores``: the device time of the two entry points on tables that are already on the device
  (tools/bench_fid.py's method: the median of blocks by the host clock around a synchronise, the same launches between two device
  events next to it).  ``bytes_read`` = (N + sum n_q) * classes * 4, the rows the two read, and ``gbytes_per_s`` that over the sum of
  the two times.  ``subset_scores_wrapper`` is ``ops.isinf_subset_scores`` itself: the host check of the tables and their upload included.
* ``torch_ms``: in the same run, the plain torch-on-device formulation of the same numbers -- the float64 rows, their normalised form
  and entropies computed once, then per subset ``index_select`` of both and float64 tensor ops, one read-back of the stacked result --
  the baseline; one warm-up, then the median of ``--runs`` runs.
* ``max_rel_difference``: the largest relative difference between the two routes' log scores.
Nothing is asserted: no ratio is fixed; both times are recorded."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from scene_generation_amd import _hip  # noqa: E402
from scene_generation_amd import isinf as II  # noqa: E402
from scene_generation_amd import ops  # noqa: E402
from tools.benchkit import emit, host_ms, measure, require_device  # noqa: E402

DEV = 'cuda:0'


def torch_route(probs, didx, sizes):
    """[S, 2] on the host by tensor ops alone"""
    p = probs.double()
    ph = p / p.sum(1, keepdim=True)
    h = torch.where(ph > 0, ph * torch.log(ph), torch.zeros_like(ph)).sum(1)
    out = []
    for q, nq in enumerate(sizes):
        t = didx[q, :nq]
        rows = ph.index_select(0, t)
        mh = torch.where(rows > 0, rows, torch.zeros_like(rows)).sum(0) / nq
        col = p.index_select(0, t).sum(0)
        qh = col / col.sum()
        T = torch.where(mh > 0, mh * torch.log(qh), torch.zeros_like(mh)).sum()
        ls = h.index_select(0, t).sum() / nq - T
        out.append(torch.stack((ls, torch.exp(ls))))
    return torch.stack(out).cpu().numpy()


def wall(fn, runs):
    """-> (the last result, host ms of each of ``runs`` calls, a synchronise included), after one warm-up: the workspace, the allocator"""
    fn()
    timed = [host_ms(fn, sync=True) for _ in range(runs)]
    return timed[-1][1], [ms for ms, _ in timed]


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--rows', type=int, nargs='+', default=[1000, 50000])
    p.add_argument('--classes', type=int, default=1000)
    p.add_argument('--num_points', type=int, default=15)
    p.add_argument('--runs', type=int, default=5)
    p.add_argument('--seconds', type=float, default=0.3)
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'isinf_bench.jsonl'))
    args = p.parse_args(argv)
    require_device()
    C = args.classes
    for n in args.rows:
        g = torch.Generator(device=DEV).manual_seed(1)
        probs = torch.softmax(torch.randn(n, C, device=DEV, generator=g) * 3.0, dim=1)
        res, times = wall(lambda: II.is_infinity(probs, num_points=args.num_points), args.runs)

        idx, sizes, _, _ = II.draw_tables(n, args.num_points)
        S, smax = idx.shape
        didx, dsz = torch.from_numpy(idx).to(DEV), torch.from_numpy(sizes).to(DEV)
        rs, h = ops.isinf_row_terms(probs)
        out = torch.empty(S, 2, dtype=torch.float64, device=DEV)
        nbytes = int(_hip.lib().sg_isinf_subset_scores_ws_bytes(S, smax, C))
        ws = ops.workspace(nbytes, probs.device)
        rr = measure(lambda: ops.isinf_row_terms(probs, rs=rs, h=h), args.seconds, args.blocks, clocks=True)
        rk = measure(lambda: ops._call('sg_isinf_subset_scores', ops._p(probs), n, C, probs.stride(0), ops._pd(rs), ops._pd(h), ops._p(didx),
                                       ops._p(dsz), S, smax, ops._pd(out), ops._p(ws), nbytes, ops._stream()),
                     args.seconds, args.blocks, clocks=True)
        rw = measure(lambda: ops.isinf_subset_scores(probs, rs, h, idx, sizes, out=out), args.seconds, args.blocks, clocks=True)
        mine = out.cpu().numpy()

        long_idx = didx.long()
        theirs, torch_times = wall(lambda: torch_route(probs, long_idx, sizes.tolist()), args.runs)
        diff = float(np.max(np.abs(theirs[:, 0] - mine[:, 0]) / np.abs(theirs[:, 0])))

        bytes_read = (n + int(sizes.sum())) * C * 4.0
        kernels_ms = rr['ms'] + rk['ms']
        rec = {'figure': 'is_infinity', 'device': torch.cuda.get_device_name(0), 'rows': n, 'classes': C, 'num_points': int(S),
               'sizes': [int(s) for s in sizes], 'rows_per_wg': _hip.CONST['SG_ISINF_ROWS_PER_WG'], 'workspace_bytes': nbytes,
               'is_infinity_ms': statistics.median(times), 'is_infinity_runs_ms': times, 'torch_ms': statistics.median(torch_times),
               'torch_runs_ms': torch_times, 'torch_over_is_infinity': statistics.median(torch_times) / statistics.median(times),
               'max_rel_difference': diff, 'is_inf': res['is_inf'], 'is_inf_log': res['is_inf_log'], 'is_n': res['is'],
               'row_terms': rr, 'subset_scores': rk, 'subset_scores_wrapper': rw, 'bytes_read': bytes_read, 'kernels_ms': kernels_ms,
               'gbytes_per_s': bytes_read / (kernels_ms * 1e-3) / 1e9}
        emit(args.out, rec)


if __name__ == '__main__':
    main()
