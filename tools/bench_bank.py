"""Benchmark of the appearance bank's segmented k-means (scene_generation_amd/bank.py, csrc/kmeans.hip) on cuda:0.

Shape: a COCO-sized synthetic bank -- P = 400 000 rows, C = 184 classes with a long-tailed size distribution (the largest class
about 10 % of P, the last ten classes below 100 rows), D = 32, K = 100 / 10 / 1; the two kernels once more at D = 128.

* per launch: sg_kmeans_assign and sg_kmeans_update with every class running, warmed up, a timed block is >= ``--seconds`` of
  back-to-back launches between two device events, a figure is the median of ``--blocks`` blocks with their spread.  Bytes are the
  ALGORITHMIC bytes (x once per launch, labels / mind2 once, the centres once per tile), given as a share of the 8.0 TB/s HBM peak;
  FLOPs are 3 P K D (subtract, multiply, add) against the 157.3 TFLOP/s fp32 vector peak (which assumes packed FMAs: the kernel's
  subtract + FMA pairs can reach 3/4 of it at best).  The bound that applies is the larger of the two least times.
* the whole build: the three clusterings (k-means++ seeding, Lloyd to convergence, final pass) of ``bank.cluster_bank``; the host
  stride of the convergence check against its two neighbours, alternating in one process.
* scikit-learn's KMeans(n_init=1) over the same classes on the same box's CPUs when it is importable.

One JSON line per figure, appended to profiles/bank_bench.jsonl (or --out)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from scene_generation_amd import bank, ops  # noqa: E402
from tools.benchkit import device_block, emit, host_ms, require_device  # noqa: E402

HBM_PEAK_GBS, FP32_VALU_TFLOPS = 8000.0, 157.3
DEV = 'cuda:0'


def class_sizes(P, C, small=10):
    """long tail: sizes ~ rank^-0.8 (the largest about 10 % of P), the last ``small`` classes 5 .. 95 rows"""
    tail = [5 + 10 * i for i in range(small)]
    w = 1.0 / np.arange(1, C - small + 1) ** 0.8
    big = np.maximum(100, np.floor(w / w.sum() * (P - sum(tail)))).astype(np.int64)
    big[0] += P - sum(tail) - big.sum()
    return [int(v) for v in big] + tail


def make_bank(P, C, D, seed=0):
    """post-ReLU-like rows around 30 blobs per class: (x fp32 [P, D] on the device, offsets int32 [C + 1], sizes)"""
    rs = np.random.RandomState(seed)
    sizes = class_sizes(P, C)
    parts = []
    for n in sizes:
        means = rs.randn(30, D) * 1.5 + 0.5
        parts.append(np.maximum(means[rs.randint(0, 30, n)] + rs.randn(n, D), 0.0).astype(np.float32))
    x = torch.from_numpy(np.concatenate(parts, 0)).to(DEV)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(DEV)
    return x, off, sizes


def bench_kernels(a, x, off, K):
    P, D = x.shape
    plan = ops.kmeans_plan(off)
    C = plan.C
    res = bank.kmeans_segmented(x, off, K, max_iter=2, tol=0.0)            # realistic centres and labels: two Lloyd iterations
    cen = res.centers.unsqueeze(0).contiguous()
    labels, mind2 = res.labels.unsqueeze(0).contiguous(), torch.zeros(1, P, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    changed, acount, counts = torch.zeros(1, C, **i32), torch.zeros(1, C, K, **i32), torch.zeros(1, C, K, **i32)
    inertia, shift = torch.zeros(1, C, device=DEV), torch.zeros(1, C, device=DEV)
    cen2 = cen.clone()
    cases = [
        ('kmeans_assign', lambda: ops.kmeans_assign(x, plan, cen, labels, mind2, changed, acount),
         P * (4.0 * D + 12.0) + plan.T * K * D * 4.0, 3.0 * P * K * D),
        ('kmeans_update', lambda: ops.kmeans_update(x, plan, labels, mind2, cen2, counts, inertia, shift),
         P * (4.0 * D + 8.0) + 2.0 * plan.T * K * (D + 1) * 4.0 + C * K * D * 8.0, 1.0 * P * D),
    ]
    for name, fn, nbytes, flops in cases:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        blocks = [device_block(lambda i: fn(), a.seconds)[0] for _ in range(a.blocks)]
        med = statistics.median(blocks)
        gbs, tf = nbytes / (med * 1e-3) / 1e9, flops / (med * 1e-3) / 1e12
        t_mem, t_alu = nbytes / (HBM_PEAK_GBS * 1e9), flops / (FP32_VALU_TFLOPS * 1e12)
        emit(a.out, {'figure': 'kernel', 'kernel': name, 'P': P, 'C': C, 'D': D, 'K': K, 'tiles': plan.T, 'us': round(med * 1e3, 2),
                     'spread_us': round((max(blocks) - min(blocks)) * 1e3, 2), 'alg_bytes': int(nbytes), 'GBps': round(gbs, 1),
                     'frac_of_hbm_peak': round(gbs / HBM_PEAK_GBS, 4), 'flops': int(flops), 'TFLOPs': round(tf, 2),
                     'frac_of_fp32_valu_peak': round(tf / FP32_VALU_TFLOPS, 4), 'bound': 'memory' if t_mem >= t_alu else 'fp32 VALU',
                     'least_us': round(max(t_mem, t_alu) * 1e6, 2), 'frac_of_bound': round(max(t_mem, t_alu) * 1e3 / med, 4)})


def bench_build(a, x, off):
    bank.cluster_bank(x, off, (100, 10, 1))                                  # warm-up of every shape
    runs, report = [], None
    for _ in range(a.blocks):
        rep = []
        ms, _ = host_ms(lambda: bank.cluster_bank(x, off, (100, 10, 1), order='none', report=rep), sync=True)
        runs.append(ms)
        report = rep
    emit(a.out, {'figure': 'build', 'P': x.size(0), 'D': x.size(1), 'ms': round(statistics.median(runs), 2),
                 'spread_ms': round(max(runs) - min(runs), 2), 'runs_ms': [round(r, 2) for r in runs], 'host_stride': bank.HOST_STRIDE,
                 'per_k': [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()} for r in report]})
    strides = [max(1, bank.HOST_STRIDE // 2), bank.HOST_STRIDE, bank.HOST_STRIDE * 2]
    times = {s: [] for s in strides}
    for _ in range(a.blocks):                                                 # alternating in one process
        for s in strides:
            ms, res = host_ms(lambda: bank.kmeans_segmented(x, off, 100, host_stride=s), sync=True)
            times[s].append(ms)
    for s in strides:
        emit(a.out, {'figure': 'host_stride', 'stride': s, 'K': 100, 'ms': round(statistics.median(times[s]), 2),
                     'spread_ms': round(max(times[s]) - min(times[s]), 2), 'runs_ms': [round(r, 2) for r in times[s]]})


def bench_sklearn(a, x, off, sizes):
    try:
        from sklearn.cluster import KMeans
    except ImportError:
        emit(a.out, {'figure': 'sklearn', 'available': False})
        return
    xs, o = x.cpu().numpy().astype(np.float64), np.concatenate([[0], np.cumsum(sizes)])
    per_k = {}
    for k in (100, 10, 1):
        t0 = time.perf_counter()
        for c, n in enumerate(sizes):
            if n:
                KMeans(n_clusters=min(n, k), n_init=1, random_state=0).fit(xs[o[c]:o[c + 1]])
        per_k[k] = round(time.perf_counter() - t0, 3)
    emit(a.out, {'figure': 'sklearn', 'available': True, 'cpus': len(os.sched_getaffinity(0)), 'seconds_per_k': per_k,
                 'seconds': round(sum(per_k.values()), 3), 'omp_num_threads': os.environ.get('OMP_NUM_THREADS')})


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bank_bench.jsonl'))
    p.add_argument('--rows', type=int, default=400000)
    p.add_argument('--classes', type=int, default=184)
    p.add_argument('--seconds', type=float, default=0.5, help='timed work per block of a kernel alone')
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--sklearn', type=int, default=1)
    a = p.parse_args()
    require_device()
    prop = torch.cuda.get_device_properties(0)
    emit(a.out, {'figure': 'run', 'time': time.strftime('%Y-%m-%d %H:%M:%S'), 'device': prop.name, 'CUs': prop.multi_processor_count,
                 'clock_rate_khz': getattr(prop, 'clock_rate', None), 'memory_clock_rate_khz': getattr(prop, 'memory_clock_rate', None),
                 'seconds': a.seconds, 'blocks': a.blocks, 'rows': a.rows, 'classes': a.classes})
    x, off, sizes = make_bank(a.rows, a.classes, 32)
    emit(a.out, {'figure': 'shape', 'P': int(x.size(0)), 'C': len(sizes), 'largest': max(sizes), 'smallest': min(sizes),
                 'below_100': sum(1 for s in sizes if s < 100)})
    for K in (100, 10, 1):
        bench_kernels(a, x, off, K)
    x128, off128, _ = make_bank(a.rows, a.classes, 128, seed=1)
    bench_kernels(a, x128, off128, 100)
    del x128
    bench_build(a, x, off)
    if a.sklearn:
        bench_sklearn(a, x, off, sizes)


if __name__ == '__main__':
    main()
