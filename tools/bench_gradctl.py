"""Micro-benchmark of the gradient control of the fused Adam step: sg_grad_norm (one read of the gradient, 4 B/param) and
sg_adam_step_ctl against sg_adam_step (28 B/param), over one flat buffer of the size of the generator's FlatParams at BASELINE
configs[1] (tools/bench_ema.py's buffer).  HIP events on the launch stream, 7 runs of 10 back-to-back launches after warm-up;
each line carries the median, the fastest and the slowest run: their spread is the allowance the comparison gets.  The last line
states the two comparisons.  One JSON line each.
Usage: python tools/bench_gradctl.py"""
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
    ctl, ws = ops.grad_ctl_alloc(dev)
    ops.grad_norm(grad, ctl, ws, 1.0, 0.0)
    norm = ops.grad_ctl_read(ctl)['norm']
    # lr 0: the timed launches leave p where it is (the traffic is the same); the record clips at half the norm
    kernels = {
        'sg_adam_step': (28, lambda: ops.adam_step(p, grad, m, v, 0.0, 0.5, 0.999, 1e-8, 10)),
        'sg_adam_step_ctl': (28, lambda: ops.adam_step_ctl(p, grad, m, v, ctl, 0.0, 0.5, 0.999, 1e-8, 10)),
        'sg_grad_norm': (4, lambda: ops.grad_norm(grad, ctl, ws, 1.0, 0.5 * norm)),
        # once more, after the others: the order of the runs is not what separates them
        'sg_adam_step (again)': (28, lambda: ops.adam_step(p, grad, m, v, 0.0, 0.5, 0.999, 1e-8, 10)),
    }
    res = {}
    for name, (bpp, fn) in kernels.items():
        us = [ms * 1e3 for ms in event_runs(fn, 10, 7, 3)]
        med, best, worst = statistics.median(us), min(us), max(us)
        res[name] = r = {'kernel': name, 'params': params, 'flat_numel': n, 'bytes_per_param': bpp, 'us_median': round(med, 1),
                         'us_min': round(best, 1), 'us_max': round(worst, 1),
                         'tb_per_s': round(bpp * n / (med * 1e-6) / 1e12, 3),
                         'tb_per_s_spread': [round(bpp * n / (worst * 1e-6) / 1e12, 3), round(bpp * n / (best * 1e-6) / 1e12, 3)]}
        emit(None, r)
    adam = [res['sg_adam_step'], res['sg_adam_step (again)']]
    lo = min(a['tb_per_s_spread'][0] for a in adam)
    slowest = max(a['us_max'] for a in adam)
    emit(None, {
        'yardstick': 'sg_adam_step in this run', 'adam_tb_per_s': [a['tb_per_s'] for a in adam], 'adam_tb_per_s_slowest_run': lo,
        'grad_norm_tb_per_s': res['sg_grad_norm']['tb_per_s'], 'grad_norm_reaches_adam_rate': res['sg_grad_norm']['tb_per_s'] >= lo,
        'adam_ctl_us_median': res['sg_adam_step_ctl']['us_median'], 'adam_us_slowest_run': slowest,
        'adam_ctl_inside_adam_spread': res['sg_adam_step_ctl']['us_median'] <= slowest})


if __name__ == '__main__':
    main()
