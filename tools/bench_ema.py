"""Micro-benchmark of the generator's Adam step with and without the fused parameter EMA: sg_adam_step (28 B/param) against
sg_adam_step_ema (36 B/param), plus the standalone sg_ema_update (12 B/param), over one flat buffer of the size of the generator's
FlatParams at BASELINE configs[1] (128x128, reference default widths; the Model is built on the meta device to count it).  HIP
events on the launch stream, median of 7 runs of 10 back-to-back launches after warm-up.  One JSON line per kernel.
Usage: python tools/bench_ema.py"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from scene_generation_amd import ops
from tools.benchkit import emit, event_runs, generator_flat_numel, require_device


def main():
    require_device()
    dev = torch.device('cuda:0')
    params, n = generator_flat_numel()
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=g)
    grad = torch.randn(n, device=dev, generator=g)
    m = torch.randn(n, device=dev, generator=g) * 0.1
    v = torch.rand(n, device=dev, generator=g) * 0.01
    e = p.clone()
    # lr 0: the timed launches leave p where it is (the traffic is the same)
    kernels = {
        'sg_adam_step': (28, lambda: ops.adam_step(p, grad, m, v, 0.0, 0.5, 0.999, 1e-8, 10)),
        'sg_adam_step_ema': (36, lambda: ops.adam_step_ema(p, grad, m, v, e, 0.0, 0.5, 0.999, 1e-8, 10, 1.0, 1.0 - 0.999)),
        'sg_ema_update': (12, lambda: ops.ema_update(e, p, 1.0 - 0.999)),
    }
    for name, (bpp, fn) in kernels.items():
        us = [ms * 1e3 for ms in event_runs(fn, 10, 7, 3)]
        med, best = statistics.median(us), min(us)
        emit(None, {'kernel': name, 'params': params, 'flat_numel': n, 'bytes_per_param': bpp, 'us_median': round(med, 1),
                    'us_min': round(best, 1), 'tb_per_s': round(bpp * n / (med * 1e-6) / 1e12, 2)})


if __name__ == '__main__':
    main()
