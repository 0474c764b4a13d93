"""Benchmark of the diversity score's own work (scene_generation_amd/lpips.py, csrc/lpips.hip) on cuda:0.

* ``wide_conv_alex_stem``: ``sg_conv2d_wide_fwd`` at AlexNet's stem (11 x 11 stride 4, 3 -> 64) for 64 images of 128 x 128 (the 2P
  forward of 32 pairs): ms and the share of the 157.3 TFLOP/s f32 MFMA peak.
* ``lpips_layer``: ``sg_lpips_layer`` at each of the ten tap shapes (alex and vgg at 128 px, P = 32): ms and algorithmic GB/s (both
  feature maps read once: 8 P C HW bytes) with its share of the 8 TB/s HBM peak, and -- the yardstick -- the same arithmetic written
  in plain torch device ops on the same tensors, what a straight port of the package runs, timed in the same run.
* ``lpips_call``: a whole ``LPIPS`` call per backbone, P = 32 pairs at 128 x 128.
* ``sample_pair``: ``Sampler.sample_pair`` against ``Sampler.sample_batch`` on one batch of a full-size generator, the cost a
  diversity evaluation adds to sampling.

Every figure: warmed up, then the median of ``--blocks`` blocks of at least ``--seconds`` each by the host clock around a device
synchronise, with the spread, and next to it the same launches between two device events; the shader and memory clocks the driver
reports are read before and after (sysfs, read only; null where the host does not show them).  Nothing is asserted.  One JSON line
per figure, appended to profiles/lpips_bench.jsonl (or --out).  Random weights (the arithmetic does not depend on them)."""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from scene_generation_amd import lpips as LP  # noqa: E402
from scene_generation_amd import ops  # noqa: E402
from tools.benchkit import emit, measure, require_device  # noqa: E402

DEV = 'cuda:0'
MFMA_F32_TFLOPS = 157.3
HBM_TBYTES_PER_S = 8.0
# (C, side of the tap) at 128 x 128
TAPS = {'alex': ((64, 31), (192, 15), (384, 7), (256, 7), (256, 7)), 'vgg': ((64, 128), (128, 64), (256, 32), (512, 16), (512, 8))}


def torch_layer(f0, f1, w, eps=1e-10):
    """one tap in plain torch device ops, as the package writes it (normalize_tensor, difference, square, 1 x 1 conv, spatial mean)"""
    n0 = torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True))
    n1 = torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True))
    d = (f0 / (n0 + eps) - f1 / (n1 + eps)) ** 2
    return (d * w.view(1, -1, 1, 1)).sum(1, keepdim=True).mean([2, 3]).view(-1)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--pairs', type=int, default=32)
    p.add_argument('--size', type=int, default=128)
    p.add_argument('--seconds', type=float, default=0.3)
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--skip_sampler', type=int, default=0)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lpips_bench.jsonl'))
    args = p.parse_args(argv)
    require_device()
    P, S = args.pairs, args.size
    base = {'device': torch.cuda.get_device_name(0), 'pairs': P, 'size': S}
    g = torch.Generator(device=DEV).manual_seed(1)

    # the stem
    x = torch.randn(2 * P, 3, S, S, device=DEV, generator=g)
    w = torch.randn(64, 3, 11, 11, device=DEV, generator=g) * 0.05
    b = torch.randn(64, device=DEV, generator=g) * 0.05
    y = ops.conv2d_wide(x, w, b, stride=4, pad=(2, 2), act=ops.ACT_RELU)
    r = measure(lambda: ops.conv2d_wide(x, w, b, stride=4, pad=(2, 2), act=ops.ACT_RELU, out=y), args.seconds, args.blocks, clocks=True)
    flops = 2.0 * 64 * 363 * 2 * P * y.size(2) * y.size(3)
    tf = flops / (r['ms'] * 1e-3) / 1e12
    emit(args.out, dict(base, figure='wide_conv_alex_stem', images=2 * P, out_side=y.size(2), flops=flops, tflops=tf,
                        share_of_f32_mfma_peak=tf / MFMA_F32_TFLOPS, plan=ops.conv2d_wide_plan(ops.rect_desc(2 * P, 3, S, S, 64, 11, 11, 4, 2, 2)),
                        **r))

    # the ten taps (sizes given for 128 px; other sizes scale the sides)
    for net, taps in TAPS.items():
        for k, (C, side) in enumerate(taps):
            side = max(1, side * S // 128)
            f = torch.relu(torch.randn(2 * P, C, side, side, device=DEV, generator=g))
            wk = torch.rand(C, device=DEV, generator=g)
            out = torch.empty(P, dtype=torch.float64, device=DEV)
            f0, f1 = f[:P], f[P:]
            r = measure(lambda: ops.lpips_layer(f0, f1, wk, out=out), args.seconds, args.blocks, clocks=True)
            rt = measure(lambda: torch_layer(f0, f1, wk), args.seconds, args.blocks, clocks=True)
            nbytes = 8.0 * P * C * side * side
            gbs = nbytes / (r['ms'] * 1e-3) / 1e9
            dev = float((out.float() - torch_layer(f0, f1, wk)).abs().max() / out.abs().max())
            emit(args.out, dict(base, figure='lpips_layer', net=net, tap=k, C=C, HW=side * side, alg_bytes=nbytes, alg_gbytes_per_s=gbs,
                                share_of_hbm_peak=gbs / (HBM_TBYTES_PER_S * 1e3), torch_ops_ms=rt['ms'], torch_ops_spread=rt['spread'],
                                torch_ops_device_events_ms=rt['device_events_ms'], speedup_over_torch_ops=rt['ms'] / r['ms'],
                                rel_dev_from_torch_ops=dev, **r))

    # a whole call per backbone
    x0 = torch.rand(P, 3, S, S, device=DEV, generator=g) * 2 - 1
    x1 = torch.rand(P, 3, S, S, device=DEV, generator=g) * 2 - 1
    models = {}
    for net in ('alex', 'vgg'):
        m = models[net] = LP.LPIPS(net, device=DEV)
        for k, C in enumerate(m.net.channels):
            setattr(m, 'lin%d' % k, torch.rand(C, device=DEV, generator=g))
        r = measure(lambda: m(x0, x1), args.seconds, args.blocks, clocks=True)
        emit(args.out, dict(base, figure='lpips_call', net=net, pairs_per_s=P / (r['ms'] * 1e-3), **r))

    # what sample_pair adds to a sampling batch
    if not args.skip_sampler:
        import numpy as np
        from scene_generation_amd import sample
        from scene_generation_amd.model import Model
        from scene_generation_amd.synthetic import batch_to, fill_deterministic, make_batch, make_vocab
        model = Model(make_vocab(), image_size=(S, S), use_attributes=True, appearance_normalization='batch',
                      activation='leakyrelu-0.2')
        fill_deterministic(model)
        model = model.to(DEV).eval()
        model.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
        rs = np.random.RandomState(0)
        bank = {c: rs.rand(100, model.rep_size) for c in range(model.num_objs)}
        batch = batch_to(make_batch(N=P, min_objs=3, max_objs=8, size=S, seed=2000), DEV)
        plain = sample.Sampler(model, features=bank)
        paired = sample.Sampler(model, features=bank, diversity=LP.Diversity(models['alex'], batch_size=P))
        random.seed(0)
        rb = measure(lambda: plain.sample_batch(batch), args.seconds, args.blocks, clocks=True)
        rp = measure(lambda: paired.sample_pair(batch), args.seconds, args.blocks, clocks=True)
        emit(args.out, dict(base, figure='sample_pair', net='alex', sample_batch_ms=rb['ms'], sample_batch_spread=rb['spread'],
                            added_ms=rp['ms'] - rb['ms'], added_share_of_sample_batch=(rp['ms'] - rb['ms']) / rb['ms'], **rp))


if __name__ == '__main__':
    main()
