"""Micro-benchmark of one ResnetBlock conv (ReflectionPad2d(1) + Conv2d(1024, 1024, 3)) on the bf16-operand path
(sg_conv3x3r_bf16_fwd / _dgrad / _wgrad) next to the fp32 Winograd path of the same conv (sg_conv2d_wino_fwd / _dgrad / _wgrad),
at the trunk shapes of BASELINE configs[1] (N 32, 8x8) and the per-GPU shape of configs[3] (N 8, 16x16).  HIP events on the
launch stream, median of 7 runs of 20 back-to-back calls after warm-up.  One JSON line per (shape, path, direction).
Usage: python tools/bench_bf16_trunk.py"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from scene_generation_amd import ops
from scene_generation_amd.ops._core import _call, _conv_desc, _p, _q, _stream, workspace
from tools.benchkit import emit, event_runs, require_device

PEAK_BF16 = 2.5e15
SHAPES = [('configs[1]', 32, 1024, 8, 8), ('configs[3]', 8, 1024, 16, 16)]


def main():
    require_device()
    dev = torch.device('cuda:0')
    for name, N, C, H, W in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(N, C, H, W, device=dev, generator=g)
        w = torch.randn(C, C, 3, 3, device=dev, generator=g) / 96.0
        b = torch.randn(C, device=dev, generator=g)
        gy = torch.randn(N, C, H, W, device=dev, generator=g)
        y, gx, gw = torch.empty_like(x), torch.empty_like(x), torch.empty_like(w)
        gb = torch.empty_like(b)
        d = _conv_desc(N, C, 0, H, W, C, 3, 1, 1, True, 1, H, W, 0, 0)
        s = _stream()
        flop = 2.0 * N * H * W * C * C * 9
        bws = _q(d, 'sg_conv3x3r_bf16_ws_bytes')
        bw = workspace(bws, dev)
        wws = _q(d, 'sg_conv2d_wino_ws_bytes')
        paths = {
            'bf16': {
                'fwd': lambda: _call('sg_conv3x3r_bf16_fwd', d._ref, _p(x), _p(w), _p(b), _p(y), _p(bw), bws, s),
                'dgrad': lambda: _call('sg_conv3x3r_bf16_dgrad', d._ref, _p(gy), _p(w), _p(gx), _p(bw), bws, s),
                'wgrad': lambda: _call('sg_conv3x3r_bf16_wgrad', d._ref, _p(gy), _p(x), _p(gw), _p(gb), _p(bw), bws, s),
            },
        }
        if _q(d, 'sg_conv2d_wino_supported'):
            ww = workspace(max(wws, bws), dev)        # (one cache entry per stream: sized for both paths up front)
            bw = ww
            paths['fp32_winograd'] = {
                'fwd': lambda: _call('sg_conv2d_wino_fwd', d._ref, _p(x), _p(w), _p(b), _p(y), 0, 0.0, None, None, _p(ww),
                                     wws, s),
                'dgrad': lambda: _call('sg_conv2d_wino_dgrad', d._ref, _p(gy), _p(w), _p(gx), None, None, _p(ww), wws, s),
                'wgrad': lambda: _call('sg_conv2d_wino_wgrad', d._ref, _p(gy), _p(x), _p(gw), None, None, _p(ww), wws, s),
            }
        for path, fns in paths.items():
            for direction, fn in fns.items():
                us = [ms * 1e3 for ms in event_runs(fn, 20, 7, 3)]
                med, best = statistics.median(us), min(us)
                emit(None, {'shape': name, 'N': N, 'C': C, 'H': H, 'W': W, 'path': path, 'dir': direction,
                                  'us_median': round(med, 1), 'us_min': round(best, 1),
                                  'direct_tflops': round(flop / (med * 1e-6) / 1e12, 1),
                                  'frac_bf16_peak': round(flop / (med * 1e-6) / PEAK_BF16, 3)})


if __name__ == '__main__':
    main()
