"""Benchmark of the sampling path (scene_generation_amd/sample.py) on cuda:0.

* ``Sampler.sample_batch`` (ground-truth boxes, masks and textures; reference default widths, nine residual blocks) at N = 1, 8, 32
  of configs[1] (128 x 128, <= 8 objects per image) and N = 8 at 256 x 256 (<= 16 objects), with the factored test-mode layout ON
  and OFF **alternating in one process**: every shape and mode is warmed up first, a timed block is >= 1 s of back-to-back calls
  between two device events, a figure is the median of five blocks (on, off, on, off, ...) with their spread.  "off" -- the dense
  layout through the channel-sparse stem -- is the behaviour before the sampling path existed, i.e. the baseline.
* the three sampling kernels alone: time per call over the ALGORITHMIC bytes (functions of the shapes, below), as a share of the
  8.0 TB/s HBM peak and of the 6.29 TB/s a float4 copy reaches on this part.  Buffers rotate through a set larger than the
  Infinity Cache.

One JSON line per figure, appended to profiles/sample_bench.jsonl (or --out)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

from scene_generation_amd import ops, sample  # noqa: E402
from scene_generation_amd.model import Model  # noqa: E402
from scene_generation_amd.synthetic import batch_to, fill_deterministic, make_batch, make_vocab  # noqa: E402
from tools.benchkit import device_block, emit, require_device  # noqa: E402

HBM_PEAK_GBS, HBM_COPY_GBS = 8000.0, 6290.0
DEV = 'cuda:0'


# ---- algorithmic bytes -----------------------------------------------------------------------------------------------------------
def planes_bytes(N, J, H, W, O, D, M, i64):
    """Z + winner + value written once; masks, boxes, vecs read once (the mass / order launches re-read masks from cache)"""
    return 4.0 * N * (J + 2) * H * W + (8.0 if i64 else 4.0) * O * M * M + 4.0 * O * (D + 4)


def dense_bytes(N, D, H, W):
    return 4.0 * N * D * H * W


def deprocess_bytes(N, C, H, W, rescale, f32, u8):
    """the image read once per launch (twice with rescale: min / max, then convert), outputs written once"""
    return N * C * H * W * ((8.0 if rescale else 4.0) + (4.0 if f32 else 0.0) + (1.0 if u8 else 0.0))


def layout_rgb_bytes(N, H, W):
    """winner + value read by both launches, three colour planes written"""
    return N * H * W * (2 * 8.0 + 12.0)


def bench_sampler(a):
    from conftest import skip_random_init
    shapes = [(1, 128, 8), (8, 128, 8), (32, 128, 8), (8, 256, 16)]
    for N, S, max_objs in shapes:
        with skip_random_init():
            m = Model(make_vocab(), image_size=(S, S), use_attributes=True, appearance_normalization='batch',
                      activation='leakyrelu-0.2')
        fill_deterministic(m)
        m = m.eval().to(DEV)
        m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
        batch = batch_to(make_batch(N=N, min_objs=3, max_objs=max_objs, size=S, seed=2000), DEV)
        samplers = {mode: sample.Sampler(m, factored=(mode == 'on')) for mode in ('on', 'off')}
        flags = dict(use_gt_boxes=True, use_gt_masks=True, use_gt_textures=True, use_gt_attr=True)
        for mode in ('on', 'off'):                               # warm-up of every shape and mode (graph capture, plan caches)
            for _ in range(3):
                samplers[mode].sample_batch(batch, **flags)
        torch.cuda.synchronize()
        blocks = {'on': [], 'off': []}
        for _ in range(a.blocks):
            for mode in ('on', 'off'):
                blocks[mode].append(device_block(lambda i: samplers[mode].sample_batch(batch, **flags), a.seconds)[0])
        for mode in ('on', 'off'):
            med = statistics.median(blocks[mode])
            emit(a.out, {'figure': 'sample_batch', 'N': N, 'size': S, 'max_objs': max_objs, 'factored': mode, 'ms_per_batch': round(med, 4),
                         'images_per_s': round(1e3 * N / med, 1), 'blocks_ms': [round(b, 4) for b in blocks[mode]],
                         'spread_ms': round(max(blocks[mode]) - min(blocks[mode]), 4)})
        on, off = statistics.median(blocks['on']), statistics.median(blocks['off'])
        spread = max(max(blocks[k]) - min(blocks[k]) for k in blocks)
        emit(a.out, {'figure': 'sample_batch_ab', 'N': N, 'size': S, 'off_over_on': round(off / on, 4), 'delta_ms': round(off - on, 4),
                     'spread_ms': round(spread, 4), 'faster_by_more_than_spread': bool(off - on > spread)})
        del m, samplers, batch
        torch.cuda.empty_cache()


def bench_kernels(a):
    for N, S, max_objs in [(1, 128, 8), (8, 128, 8), (32, 128, 8), (8, 256, 16)]:
        b = make_batch(N=N, min_objs=3, max_objs=max_objs, size=S, seed=2000)
        O_, M, D = b.objs.numel(), b.masks.size(1), 172 + 32
        counts, plane = [0] * N, []
        for i in b.obj_to_img.tolist():
            plane.append(counts[i])
            counts[i] += 1
        J = max(counts)
        g = torch.Generator().manual_seed(1)
        vecs = torch.cat([torch.eye(172)[b.objs], torch.rand(O_, 32, generator=g)], 1).to(DEV)
        boxes, masks, o2i = b.boxes.to(DEV), b.masks.to(DEV), b.obj_to_img.to(DEV)
        pidx = torch.tensor(plane, dtype=torch.int64, device=DEV)
        objs = b.objs.to(DEV)
        colors = torch.randint(0, 256, [172, 3], generator=g).float().to(DEV)
        seg = ops.segment_offsets(o2i, N)
        nbuf = max(2, min(16, int(600e6 / (N * 3 * S * S * 4)) + 1))
        imgs = [torch.randn(N, 3, S, S, device=DEV) for _ in range(nbuf)]
        with torch.no_grad():
            Z, winner, value = ops.masks_to_layout_test_planes(vecs, boxes, masks, seg, pidx, N, J, S, S, False)
        cases = [
            ('layout_test_planes', lambda i: ops.masks_to_layout_test_planes(vecs, boxes, masks, seg, pidx, N, J, S, S, False),
             planes_bytes(N, J, S, S, O_, D, M, True)),
            ('layout_test_dense', lambda i: ops.masks_to_layout_test(vecs, boxes, masks, seg, N, S, S, False), dense_bytes(N, D, S, S)),
            ('deprocess_u8', lambda i: ops.deprocess_images(imgs[i % nbuf]), deprocess_bytes(N, 3, S, S, True, False, True)),
            ('deprocess_f32', lambda i: ops.deprocess_images(imgs[i % nbuf], uint8=False, float32=True),
             deprocess_bytes(N, 3, S, S, True, True, False)),
            ('layout_rgb', lambda i: ops.layout_rgb(winner, value, objs, colors), layout_rgb_bytes(N, S, S)),
        ]
        with torch.no_grad():
            for name, fn, nbytes in cases:
                for i in range(3):
                    fn(i)
                torch.cuda.synchronize()
                blocks = [device_block(fn, a.kernel_seconds)[0] for _ in range(a.blocks)]
                med = statistics.median(blocks)
                gbs = nbytes / (med * 1e-3) / 1e9
                emit(a.out, {'figure': 'kernel', 'kernel': name, 'N': N, 'size': S, 'J': J, 'O': O_, 'us': round(med * 1e3, 2),
                             'alg_bytes': int(nbytes), 'GBps': round(gbs, 1), 'frac_of_hbm_peak': round(gbs / HBM_PEAK_GBS, 4),
                             'frac_of_copy_rate': round(gbs / HBM_COPY_GBS, 4),
                             'spread_us': round((max(blocks) - min(blocks)) * 1e3, 2)})


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sample_bench.jsonl'))
    p.add_argument('--seconds', type=float, default=1.0, help='timed work per block of sample_batch')
    p.add_argument('--kernel_seconds', type=float, default=1.0, help='timed work per block of a kernel alone')
    p.add_argument('--blocks', type=int, default=5)
    p.add_argument('--only', default='', choices=['', 'sampler', 'kernels'])
    a = p.parse_args()
    require_device()
    emit(a.out, {'figure': 'run', 'time': time.strftime('%Y-%m-%d %H:%M:%S'), 'device': torch.cuda.get_device_name(0),
                 'seconds': a.seconds, 'kernel_seconds': a.kernel_seconds, 'blocks': a.blocks})
    if a.only in ('', 'kernels'):
        bench_kernels(a)
    if a.only in ('', 'sampler'):
        bench_sampler(a)


if __name__ == '__main__':
    main()
