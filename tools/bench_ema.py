"""Micro-benchmark of the generator's Adam step with and without the fused parameter EMA: sg_adam_step (28 B/param) against
sg_adam_step_ema (36 B/param), plus the standalone sg_ema_update (12 B/param), over one flat buffer of the size of the generator's
FlatParams at BASELINE configs[1] (128x128, reference default widths; the Model is built on the meta device to count it).  HIP
events on the launch stream, median of 7 runs of 10 back-to-back launches after warm-up.  One JSON line per kernel.
Usage: python tools/bench_ema.py"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from scene_generation_amd import ops
from scene_generation_amd.args import parser
from scene_generation_amd.model import Model
from scene_generation_amd.optim import FlatParams
from scene_generation_amd.synthetic import make_vocab


def timeit(fn, n=10, reps=7):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / n * 1e3)
    return statistics.median(ts), min(ts)


def generator_flat_numel():
    args = parser.parse_args(['--image_size', '128,128', '--output_dir', '/tmp/o'])
    kw = {'vocab': make_vocab(), 'image_size': args.image_size, 'embedding_dim': args.embedding_dim,
          'gconv_dim': args.gconv_dim, 'gconv_hidden_dim': args.gconv_hidden_dim, 'gconv_num_layers': args.gconv_num_layers,
          'mlp_normalization': args.mlp_normalization, 'appearance_normalization': args.appearance_normalization,
          'activation': args.activation, 'mask_size': args.mask_size, 'n_downsample_global': args.n_downsample_global,
          'box_dim': args.box_dim, 'use_attributes': args.use_attributes, 'box_noise_dim': args.box_noise_dim,
          'mask_noise_dim': args.mask_noise_dim, 'pool_size': args.pool_size, 'rep_size': args.rep_size}
    with torch.device('meta'):
        ps = list(Model(**kw).parameters())
    a = FlatParams.ALIGN
    return sum(p.numel() for p in ps), sum((p.numel() + a - 1) // a * a for p in ps)


def main():
    torch.cuda.set_device(0)
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
        med, best = timeit(fn)
        print(json.dumps({'kernel': name, 'params': params, 'flat_numel': n, 'bytes_per_param': bpp,
                          'us_median': round(med, 1), 'us_min': round(best, 1),
                          'tb_per_s': round(bpp * n / (med * 1e-6) / 1e12, 2)}), flush=True)


if __name__ == '__main__':
    main()
