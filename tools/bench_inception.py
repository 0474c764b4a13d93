"""Benchmark of the Inception score (scene_generation_amd/inception.py, csrc/inception.hip) on cuda:0.

* ``score``: images per second of ``InceptionScore(resize=True)`` fed ``--batch`` images of ``--size`` x ``--size`` (resize to 299,
  Inception-v3, softmax rows into the device buffer), with the whole-forward TFLOP/s (2 FLOP per multiply-add of the 94 conv units and
  the dense layer) as a share of the 157.3 TFLOP/s f32 MFMA peak -- a whole-program rate, not a kernel's share.
* ``class``: one profiled pass through the library's own per-kind event timers (not the end-to-end figure: the timers serialise the
  launches), summed per geometry class of the conv units -- stem, 1x1, 3x3, 5x5, 1x7 / 7x1, 1x3 / 3x1 on each grid -- with each class's
  FLOPs over its time as a share of the f32 MFMA peak (median of ``--blocks`` rounds of 10 launches per unit, with the spread of the
  rounds); and the time of the pools / resize / softmax kinds.
* ``plans``: which launch plan (tile, weight loader, k-chunks) each of the 94 conv units takes at this batch.
* ``check_model``: one ``evaluate.check_model`` pass over ``--num_val_samples`` synthetic validation images with and without the scorer,
  the two variants alternating block by block.

Every timed figure: warmed up, then the median of ``--blocks`` blocks of at least ``--seconds`` each, with their spread.  One JSON
line per figure, appended to profiles/inception_bench.jsonl (or --out).  Random weights (the arithmetic does not depend on them)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from scene_generation_amd import inception as I  # noqa: E402
from scene_generation_amd import ops  # noqa: E402
from tools.benchkit import emit, measure, profiled, require_device, timed_block  # noqa: E402

MFMA_F32_TFLOPS = 157.3
DEV = 'cuda:0'


def unit_flops(u):
    return 2.0 * u['N'] * u['Cout'] * u['OH'] * u['OW'] * u['C'] * u['KH'] * u['KW']


def unit_class(u):
    blk = u['name'].split('.')[0]
    if not blk.startswith('Mixed_'):
        return 'stem %dx%d s%d @%d' % (u['KH'], u['KW'], u['stride'], u['H'])
    return '%dx%d s%d @%d' % (u['KH'], u['KW'], u['stride'], u['H'])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=32)
    p.add_argument('--size', type=int, default=128)
    p.add_argument('--seconds', type=float, default=1.0)
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--num_val_samples', type=int, default=64)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'inception_bench.jsonl'))
    args = p.parse_args(argv)
    require_device()
    base = {'device': torch.cuda.get_device_name(0), 'batch': args.batch, 'size': args.size}

    scorer = I.InceptionScore(batch_size=args.batch, resize=True, weights=None, device=DEV)
    net = scorer.inception_model
    imgs = torch.rand(args.batch, 3, args.size, args.size, device=DEV) * 2 - 1
    units = I.conv_units(299, args.batch)
    flops = sum(unit_flops(u) for u in units) + 2.0 * args.batch * 2048 * net.fc.out_features

    # ---- plans ---------------------------------------------------------------------------------------------------------------------
    plans = [dict(name=u['name'], K=u['C'] * u['KH'] * u['KW'], M=u['Cout'], pixels=u['N'] * u['OH'] * u['OW'],
                  tile=ops.RECT_TILES[pl['tile']], vec=pl['vec'], splits=pl['splits'], kchunk=pl['kchunk'])
             for u, pl in ((u, I.unit_plan(u)) for u in units)]
    emit(args.out, dict(base, figure='plans', units=len(plans), plans=plans))

    # ---- images per second -----------------------------------------------------------------------------------------------------------
    def feed():
        scorer.clean()
        scorer(imgs)
    r = measure(feed, args.seconds, args.blocks, warmup=2)
    tf = flops / (r['ms'] * 1e-3) / 1e12
    emit(args.out, dict(base, figure='score', images_per_s=args.batch / (r['ms'] * 1e-3), gflop_per_image=flops / args.batch / 1e9,
                        tflops_whole_forward=tf, share_of_f32_mfma_peak_whole_forward=tf / MFMA_F32_TFLOPS, **r))
    x299 = ops.resize_bilinear(imgs, (299, 299))
    r = measure(lambda: net(x299), args.seconds, args.blocks, warmup=2)
    tf = flops / (r['ms'] * 1e-3) / 1e12
    emit(args.out, dict(base, figure='network_forward_299', images_per_s=args.batch / (r['ms'] * 1e-3), tflops_whole_forward=tf,
                        share_of_f32_mfma_peak_whole_forward=tf / MFMA_F32_TFLOPS, **r))
    probs = scorer.probs
    n = min(probs.size(0), 4 * args.batch)
    probs[:n] = torch.softmax(torch.randn(n, probs.size(1), device=DEV), 1)
    r = measure(lambda: ops.inception_score(probs, n, 5), args.seconds, args.blocks, warmup=2)
    emit(args.out, dict(base, figure='inception_score_kernel', rows=n, splits=5, **r))

    # ---- per geometry class: one conv unit at a time between the library's event timers ---------------------------------------------
    classes = {}

    def per_class_then_one_pass():
        for u in units:
            g = torch.Generator(device=DEV).manual_seed(1)
            x = torch.randn(u['N'], u['C'], u['H'], u['W'], device=DEV, generator=g)
            w = torch.randn(u['Cout'], u['C'], u['KH'], u['KW'], device=DEV, generator=g) * 0.05
            b = torch.zeros(u['Cout'], device=DEV)
            out = torch.empty(u['N'], u['out_ctot'], u['OH'], u['OW'], device=DEV)

            def run():
                ops.conv2d_rect(x, w, b, stride=u['stride'], pad=(u['padH'], u['padW']), act=ops.ACT_RELU, out=out, out_c0=u['out_c0'])
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            reps, rounds = 10, []
            for _ in range(args.blocks):                            # ``blocks`` rounds of 10 launches: the median round, and the spread
                ops.prof_reset()
                for _ in range(reps):
                    run()
                prof = ops.prof_read()
                rounds.append(sum(prof[k]['ms'] for k in ('rect_conv_t64', 'rect_conv_t32', 'rect_conv_t64x128', 'rect_reduce')) / reps)
            c = classes.setdefault(unit_class(u), {'units': 0, 'ms': 0.0, 'lo': 0.0, 'hi': 0.0, 'flops': 0.0})
            c['units'] += 1
            c['ms'] += statistics.median(rounds)
            c['lo'] += min(rounds)
            c['hi'] += max(rounds)
            c['flops'] += unit_flops(u)
        # the other kinds over one whole pass: what is read when this returns
        ops.prof_reset()
        scorer.clean()
        scorer(imgs)
    prof, _ = profiled(per_class_then_one_pass)
    total_ms = sum(c['ms'] for c in classes.values())
    for name, c in sorted(classes.items()):
        tf = c['flops'] / (c['ms'] * 1e-3) / 1e12
        emit(args.out, dict(base, figure='class', geometry=name, units=c['units'], kernel_ms=c['ms'], gflop=c['flops'] / 1e9,
                            tflops=tf, share_of_f32_mfma_peak=tf / MFMA_F32_TFLOPS, share_of_conv_time=c['ms'] / total_ms,
                            spread=(c['hi'] - c['lo']) / c['ms'], rounds=args.blocks, launches_per_round=10))
    emit(args.out, dict(base, figure='conv_kernels_total', kernel_ms=total_ms,
                        tflops=sum(c['flops'] for c in classes.values()) / (total_ms * 1e-3) / 1e12,
                        share_of_f32_mfma_peak=sum(c['flops'] for c in classes.values()) / (total_ms * 1e-3) / 1e12 / MFMA_F32_TFLOPS))
    emit(args.out, dict(base, figure='other_kinds_one_pass',
                        kinds={k: {'ms': v['ms'], 'launches': v['launches']} for k, v in prof.items()
                               if v['launches'] and not k.startswith('rect_conv')}))

    # ---- check_model with and without the scorer ---------------------------------------------------------------------------------------
    from scene_generation_amd.evaluate import check_model
    from scene_generation_amd.model import Model
    from scene_generation_amd.synthetic import make_batch, make_vocab
    vocab = make_vocab(12, 4, 35)
    model = Model(vocab, image_size=(args.size, args.size), gconv_hidden_dim=128, gconv_num_layers=5, mask_size=16, n_downsample_global=4,
                  appearance_normalization='batch', activation='leakyrelu-0.2', use_attributes=True, pool_size=2, rep_size=32).to(DEV).eval()
    nb = max(1, args.num_val_samples // args.batch)
    loader = [make_batch(N=args.batch, min_objs=3, max_objs=8, size=args.size, mask_size=16, num_objs=12, num_preds=4, seed=50 + i)
              for i in range(nb)]
    cfg = type('A', (), {'num_val_samples': nb * args.batch})()
    sc = I.InceptionScore(batch_size=args.batch, resize=True, weights=net, device=DEV)
    variants = {'with': lambda: check_model(cfg, loader, model, sc, True), 'without': lambda: check_model(cfg, loader, model, None, True)}
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    blocks = {'with': [], 'without': []}
    for _ in range(args.blocks):                                    # the two variants alternate, block by block
        for name, fn in variants.items():
            blocks[name].append(timed_block(fn, args.seconds)[0])
    med = {k: statistics.median(v) for k, v in blocks.items()}
    emit(args.out, dict(base, figure='check_model', num_val_samples=nb * args.batch, with_scorer_ms=med['with'],
                        without_scorer_ms=med['without'], with_scorer_blocks_ms=blocks['with'], without_scorer_blocks_ms=blocks['without'],
                        with_scorer_spread=(max(blocks['with']) - min(blocks['with'])) / med['with'],
                        without_scorer_spread=(max(blocks['without']) - min(blocks['without'])) / med['without'],
                        scorer_ms_per_image=(med['with'] - med['without']) / (nb * args.batch)))


if __name__ == '__main__':
    main()
