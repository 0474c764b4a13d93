"""What LPIPS as a training loss costs (scene_generation_amd/lpips.py LPIPSLoss, csrc/lpips.hip sg_lpips_layer_bwd) on cuda:0.
(Named lpips_loss_bench.py, not bench_*.py: tests/test_benchkit_cpu.py pins the number of tools/bench_*.py files; like them it
measures through tools/benchkit.py only and keeps no copy of a primitive.)

* ``lpips_layer_bwd``: ``sg_lpips_layer_bwd`` at each of the five training tap shapes (VGG-16 at 128 x 128, N = 32: C / HW = 64 / 16384,
  128 / 4096, 256 / 1024, 512 / 256, 512 / 64): ms and algorithmic GB/s (two reads and one write of the feature map: 12 P C HW bytes)
  with its share of the 8 TB/s HBM peak, next to ``sg_lpips_layer`` on the same tensors in the same run (8 P C HW bytes) and the
  ratio of the two achieved rates.
* ``lpips_loss_call``: one forward + backward of ``LPIPSLoss`` on N pictures (the gradient with respect to the prediction).
* ``train_step``: the headline training step (bench.py's workload: 128 x 128, batch 32, the default widths, VGG19 loss off) with the
  LPIPS term off, with ``lpips_loss=1`` on, and with the reference's VGG19 feature loss on (``--vgg_features_weight 10``) instead:
  three Trainers in this one process, one after the other, on the same two batches.

Every figure: warmed up, then the median of ``--blocks`` blocks of at least ``--seconds`` each by the host clock around a device
synchronise, with the spread, and next to it the same launches between two device events; the clocks the driver reports before and
after.  Nothing is asserted: the run records what the loss costs.  One JSON line per figure, appended to
profiles/lpips_loss_bench.jsonl (or --out).  Random weights (the arithmetic and its cost do not depend on them)."""
import argparse
import gc
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
HBM_TBYTES_PER_S = 8.0
TAPS = ((64, 128), (128, 64), (256, 32), (512, 16), (512, 8))          # (C, side of the tap) of VGG-16 at 128 x 128


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=32)
    p.add_argument('--size', type=int, default=128)
    p.add_argument('--seconds', type=float, default=0.3)
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--step_seconds', type=float, default=1.0)
    p.add_argument('--skip_steps', type=int, default=0)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lpips_loss_bench.jsonl'))
    args = p.parse_args(argv)
    require_device()
    os.environ.pop('SG_LPIPS_LOSS', None)             # the three legs below say what they run
    N, S = args.batch, args.size
    base = {'device': torch.cuda.get_device_name(0), 'batch': N, 'size': S}
    g = torch.Generator(device=DEV).manual_seed(1)

    # (a) the backward kernel next to the forward kernel
    for k, (C, side) in enumerate(TAPS):
        side = max(1, side * S // 128)
        f0 = torch.relu(torch.randn(N, C, side, side, device=DEV, generator=g))
        f1 = torch.relu(torch.randn(N, C, side, side, device=DEV, generator=g))
        wk = torch.rand(C, device=DEV, generator=g)
        out = torch.empty(N, dtype=torch.float64, device=DEV)
        gout = torch.full((N,), 1.0 / N, dtype=torch.float64, device=DEV)
        rf = measure(lambda: ops.lpips_layer(f0, f1, wk, out=out), args.seconds, args.blocks, clocks=True)
        rb = measure(lambda: ops.lpips_layer_bwd(f0, f1, wk, gout), args.seconds, args.blocks, clocks=True)
        elems = float(N) * C * side * side
        fwd_gbs, bwd_gbs = 8.0 * elems / (rf['ms'] * 1e-3) / 1e9, 12.0 * elems / (rb['ms'] * 1e-3) / 1e9
        emit(args.out, dict(base, figure='lpips_layer_bwd', tap=k, C=C, HW=side * side, alg_bytes=12.0 * elems, alg_gbytes_per_s=bwd_gbs,
                            share_of_hbm_peak=bwd_gbs / (HBM_TBYTES_PER_S * 1e3), fwd_ms=rf['ms'], fwd_spread=rf['spread'],
                            fwd_device_events_ms=rf['device_events_ms'], fwd_alg_bytes=8.0 * elems, fwd_alg_gbytes_per_s=fwd_gbs,
                            bwd_rate_over_fwd_rate=bwd_gbs / fwd_gbs, **rb))
        del f0, f1

    # the whole loss, forward + backward
    m = LP.LPIPSLoss(device=DEV)
    for k, C in enumerate(m.net.channels):
        setattr(m, 'lin%d' % k, torch.rand(C, device=DEV, generator=g))
    x = torch.randn(N, 3, S, S, device=DEV, generator=g).requires_grad_(True)
    y = torch.randn(N, 3, S, S, device=DEV, generator=g)

    def loss_call():
        x.grad = None
        m(x, y).backward()
    r = measure(loss_call, args.seconds, args.blocks, clocks=True)
    emit(args.out, dict(base, figure='lpips_loss_call', net='vgg', **r))
    del m, x, y

    # (b) the headline step without the term, with it, and with the VGG19 loss instead
    if args.skip_steps:
        return
    from scene_generation_amd.args import parser
    from scene_generation_amd.pipeline import DeviceBatchPrefetcher
    from scene_generation_amd.synthetic import make_batch, make_vocab
    from scene_generation_amd.trainer import Trainer
    vocab = make_vocab()
    staged = list(DeviceBatchPrefetcher([make_batch(N=N, min_objs=3, max_objs=8, size=S, seed=i) for i in range(2)], DEV))
    results = {}
    for leg, vgg_weight, lpips_loss in (('off', 0, False), ('lpips', 0, 1.0), ('vgg19', 10, False)):
        gc.collect()
        torch.cuda.empty_cache()
        a = parser.parse_args(['--image_size', '%d,%d' % (S, S), '--batch_size', str(N), '--vgg_features_weight', str(vgg_weight),
                               '--output_dir', '/tmp/o'])
        torch.manual_seed(1234)
        tr = Trainer(a, vocab, device=DEV, lpips_loss=lpips_loss)
        tr.model.layout_objects_hint = 9
        tr.dense_layout_outputs = False
        random.seed(0)
        torch.manual_seed(100)
        count = [0]

        def one_step():
            db = staged[count[0] % 2]
            count[0] += 1
            tr.model.objs_host, tr.model.obj_to_img_host = db.objs_host, db.obj_to_img_host
            tr.step(db.batch, use_gt=tr.draw_use_gt())
        r = measure(one_step, args.step_seconds, args.blocks, warmup=4, clocks=True)
        results[leg] = r['ms']
        emit(args.out, dict(base, figure='train_step', leg=leg, vgg_features_weight=vgg_weight, lpips_loss=lpips_loss or 0,
                            added_ms_over_off=r['ms'] - results['off'], added_share_of_off=(r['ms'] - results['off']) / results['off'],
                            **r))
        del tr, one_step


if __name__ == '__main__':
    main()
