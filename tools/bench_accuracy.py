"""Benchmark of the object-accuracy classifier (scene_generation_amd/accuracy.py, csrc/classifier.hip) on cuda:0.

* ResNet-101 (``--model``) at 224 x 224 with 64-crop chunks: the eval forward with the BatchNorms folded into the convolutions, the
  plain eval forward, one training step under the reference's freeze rule (forward, cross-entropy, backward, FusedSGD), and the
  scoring of one sampled batch's crops through ``AccuracyMeter`` against the reference's bookkeeping (argmax + two ``.item()`` per
  object, scripts/sample_images.py:233-239) on the same network.  Forward figures carry TFLOP/s (2 FLOP per multiply-add of the
  convolutions and the dense layer) as a share of the 157.3 TFLOP/s f32 MFMA peak; the folded forward also carries the library's
  time per kernel kind from one profiled pass.
* the new kernels alone on ``--elements`` floats (the max-pool on the stem's 64 x 112 x 112 planes of a chunk): algorithmic bytes
  over time as a share of the 8.0 TB/s HBM peak, between two device events.

Every figure: warmed up, then the median of ``--blocks`` blocks of at least ``--seconds`` each, with their spread.  One JSON line
per figure, appended to profiles/accuracy_bench.jsonl (or --out)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from scene_generation_amd import accuracy, layers, ops  # noqa: E402
from scene_generation_amd.optim import FusedSGD  # noqa: E402
from tools.benchkit import emit, measure, profiled, require_device  # noqa: E402

HBM_PEAK_GBS, MFMA_F32_TFLOPS = 8000.0, 157.3
DEV = 'cuda:0'


def forward_flops(model, x):
    """2 * multiply-adds of every convolution and the dense layer in one forward of ``x``"""
    total, hooks = [0], []

    def conv_hook(m, inp, out):
        total[0] += 2 * out.numel() * m.in_channels * m.kernel_size[0] * m.kernel_size[1]

    def fc_hook(m, inp, out):
        total[0] += 2 * out.numel() * m.in_features
    for m in model.modules():
        if isinstance(m, layers.Conv2d):
            hooks.append(m.register_forward_hook(conv_hook))
        elif isinstance(m, layers.Linear):
            hooks.append(m.register_forward_hook(fc_hook))
    A = accuracy.ResNet
    keep, A.fold_batchnorm = A.fold_batchnorm, False         # the plain form calls the modules the hooks sit on
    try:
        with torch.no_grad():
            model(x)
    finally:
        A.fold_batchnorm = keep
        for h in hooks:
            h.remove()
    return total[0]


def kinds_of(fn):
    """the library's time per kernel kind in one profiled call (events around every launch: the sum exceeds the unprofiled time)"""
    prof, _ = profiled(fn)
    return {k: {'launches': v['launches'], 'ms': round(v['ms'], 4), 'TFLOPs': round(v['flops'] / v['ms'] / 1e9, 2) if v['ms'] else 0.0}
            for k, v in prof.items() if v['launches']}


def bench_network(args):
    torch.manual_seed(0)
    S, B = args.input_shape, args.chunk
    x = torch.randn(B, 3, S, S, device=DEV)
    labels = torch.randint(0, 172, (B,), device=DEV)
    base = {'model': args.model, 'input': S, 'chunk': B, 'classes': 172}

    model = accuracy.all_pretrained_models(172, name=args.model).to(DEV)
    model.eval()
    flops = forward_flops(model, x)

    def fwd():
        with torch.no_grad():
            return model(x)

    keep_fold = accuracy.ResNet.fold_batchnorm
    for fold in (True, False):
        accuracy.ResNet.fold_batchnorm = fold
        try:
            rec = dict(base, bench='eval_forward_folded' if fold else 'eval_forward_unfolded', flops=flops, clock='device events')
            rec.update(measure(fwd, args.seconds, args.blocks, warmup=2, device_events=True))
            rec['TFLOPs'] = flops / rec['ms'] / 1e9
            rec['share_of_f32_mfma_peak'] = rec['TFLOPs'] / MFMA_F32_TFLOPS
            rec['ms_per_crop'] = rec['ms'] / B
            rec['kinds'] = kinds_of(fwd)
            emit(args.out, rec)
        finally:
            accuracy.ResNet.fold_batchnorm = keep_fold
    accuracy.ResNet.fold_batchnorm = True
    for other in [int(c) for c in args.other_chunks.split(',') if c]:       # the chunk size picks the route of the 3x3 convs
        xo = torch.randn(other, 3, S, S, device=DEV)

        def fwd_other():
            with torch.no_grad():
                return model(xo)
        rec = dict(base, bench='eval_forward_folded', chunk=other, flops=flops * other // B, clock='device events')
        rec.update(measure(fwd_other, args.seconds, args.blocks, warmup=2, device_events=True))
        rec['TFLOPs'] = rec['flops'] / rec['ms'] / 1e9
        rec['share_of_f32_mfma_peak'] = rec['TFLOPs'] / MFMA_F32_TFLOPS
        rec['ms_per_crop'] = rec['ms'] / other
        rec['kinds'] = kinds_of(fwd_other)
        emit(args.out, rec)
        del xo
    accuracy.ResNet.fold_batchnorm = keep_fold

    # scoring one sampled batch's worth of crops: the meter against the reference's per-object bookkeeping
    O = args.objects
    imgs = torch.randn(32, 3, 128, 128, device=DEV)
    xy = torch.rand(O, 2, device=DEV) * 0.5
    boxes = torch.cat([xy, xy + 0.2 + 0.3 * torch.rand(O, 2, device=DEV)], 1).contiguous()
    o2i = torch.arange(O, device=DEV) * 32 // O
    objs = torch.randint(0, 172, (O,), device=DEV)
    meter = accuracy.AccuracyMeter(model, S, B)

    def score_meter():
        meter.update(imgs, boxes, o2i, objs)

    def score_reference():
        corrects = real = 0
        for out, a in zip(meter.logits(imgs, boxes, o2i), range(0, O, B)):
            _, preds = torch.max(out, 1)
            for pred, label in zip(preds, objs[a:a + out.size(0)]):
                if label.item() != 0:
                    real += 1
                    corrects += 1 if pred.item() == label.item() else 0
        return corrects, real

    for name, fn in (('score_meter', score_meter), ('score_item_loop', score_reference)):
        rec = dict(base, bench=name, objects=O, clock='host, ends in a synchronise')
        rec.update(measure(fn, args.seconds, args.blocks, warmup=2))
        emit(args.out, rec)

    # one training step under the freeze rule
    model.train(True)
    opt = FusedSGD([p for p in model.parameters() if p.requires_grad], lr=0.001, momentum=0.9)

    def step():
        opt.zero_grad()
        ops.cross_entropy(model(x), labels).backward()
        opt.step()

    rec = dict(base, bench='train_step_freeze_rule', clock='device events', trainable=int(opt.fp.numel),
               frozen_stages=model.frozen_stages())
    rec.update(measure(step, args.seconds, args.blocks, warmup=2, device_events=True))
    emit(args.out, rec)


def bench_kernels(args):
    n = args.elements
    a, b, y = (torch.randn(n, device=DEV) for _ in range(3))
    figures = [('add_relu', lambda: ops._call('sg_add_relu_fwd', a.data_ptr(), b.data_ptr(), y.data_ptr(), n, ops._stream()), 12 * n)]
    p, g, buf = (torch.randn(n, device=DEV) for _ in range(3))
    figures.append(('sgd_momentum_step', lambda: ops.sgd_momentum_step(p, g, buf, 1e-3, 0.9, False), 20 * n))
    NC, H = args.chunk * 64, 112
    xin = torch.randn(NC, H, H, device=DEV)
    yout = torch.empty(NC, H // 2, H // 2, device=DEV)
    gxin = torch.empty_like(xin)
    figures.append(('maxpool3s2_fwd', lambda: ops._call('sg_maxpool3s2_fwd', xin.data_ptr(), yout.data_ptr(), NC, H, H, H // 2, H // 2,
                                                        ops._stream()), 4 * (xin.numel() + yout.numel())))
    figures.append(('maxpool3s2_bwd', lambda: ops._call('sg_maxpool3s2_bwd', xin.data_ptr(), yout.data_ptr(), gxin.data_ptr(), NC, H, H,
                                                        H // 2, H // 2, ops._stream()), 4 * (2 * xin.numel() + yout.numel())))
    w = torch.randn(2048, 1024, 1, 1, device=DEV)
    vecs = [torch.rand(2048, device=DEV) + 0.5 for _ in range(4)]
    figures.append(('bn_fold', lambda: ops.bn_fold(w, vecs[0], vecs[1], vecs[2], vecs[3], 1e-5), 8 * w.numel()))
    logits = torch.randn(1024, 172, device=DEV)
    target = torch.randint(0, 172, (1024,), device=DEV)
    acc = ops.new_classify_record(DEV)
    figures.append(('classify_stats', lambda: ops.classify_stats(logits, target, 0, acc), 4 * logits.numel() + 8 * 1024))
    for name, fn, nbytes in figures:
        rec = {'bench': 'kernel_' + name, 'bytes': nbytes, 'clock': 'device events'}
        rec.update(measure(fn, args.seconds, args.blocks, warmup=2, device_events=True))
        rec['GBs'] = nbytes / rec['ms'] / 1e6
        rec['share_of_hbm_peak'] = rec['GBs'] / HBM_PEAK_GBS
        emit(args.out, rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'accuracy_bench.jsonl'))
    ap.add_argument('--model', default='resnet101')
    ap.add_argument('--input_shape', type=int, default=224)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--other_chunks', default='128', help='further chunk sizes for the folded eval forward (comma list)')
    ap.add_argument('--objects', type=int, default=200, help='objects of the scored batch (configuration c2 has about 200)')
    ap.add_argument('--elements', type=int, default=1 << 26)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--skip', default='', help='comma list of: network, kernels')
    args = ap.parse_args()
    require_device()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if 'kernels' not in args.skip:
        bench_kernels(args)
    if 'network' not in args.skip:
        bench_network(args)


if __name__ == '__main__':
    main()
