"""Benchmark of the quasi-random inputs (scene_generation_amd/qmc.py, csrc/qmc.hip) on cuda:0, at 32 images / 200 objects.

* the call time of the three launches -- ``sg_sobol_points`` (32 points of 160 dimensions), ``sg_qmc_unpack``, ``sg_bank_draw`` (200
  rows of 32 floats out of a bank of 172 classes x 100 rows) -- each between two device events around back-to-back calls, and the three
  together through ``QuasiRandomInputs.draw`` + ``DeviceBank.draw`` on the host clock around calls that end in a synchronise.  The
  kernels move a few kilobytes: the figures are launch floors, not shares of a peak.
* the time ``Sampler.sample_batch`` spends IN FRONT OF the forward -- from its entry to the call of the model -- with ``quasi_random``
  off (the host loop over the bank: one ``random.randint`` and one numpy row per object, a stack, an upload, an unbind) and on (three
  launches), on the host clock, and the whole call on device events.  The same sampler class, the same batch, one process, the two
  modes alternating block by block.

Every time: warmed up, then the median of ``--blocks`` blocks of at least ``--seconds`` each, with their spread, clocks as found.
One JSON line per figure, appended to profiles/qmc_bench.jsonl (or --out)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from scene_generation_amd import ops, qmc, sample  # noqa: E402
from scene_generation_amd.model import Model  # noqa: E402
from scene_generation_amd.synthetic import batch_to, fill_deterministic, make_batch, make_vocab  # noqa: E402
from tools.benchkit import emit, measure, require_device, summary, timed_block  # noqa: E402

DEV = 'cuda:0'
N, C, ROWS, REP, NOISE, SLOTS = 32, 172, 100, 32, 64, 32


def make_bank(seed=0):
    rs = np.random.RandomState(seed)
    return {c: rs.rand(ROWS, REP).astype(np.float32) for c in range(C)}


def the_batch():
    """32 images, 200 objects (4..7 real objects per image and its __image__ object): the first seed that gives exactly 200"""
    for seed in range(200):
        b = make_batch(N=N, min_objs=4, max_objs=7, size=128, seed=3000 + seed)
        if b.objs.numel() == 200:
            return b
    raise SystemExit('no synthetic batch of 200 objects among 200 seeds')


def bench_calls(args, batch):
    b = batch_to(batch, DEV)
    O = b.objs.numel()
    q = qmc.QuasiRandomInputs(NOISE, max_objects=SLOTS, seed=0, device=DEV)
    bank = qmc.DeviceBank.from_dict(make_bank(), C, DEV)
    seg = ops.segment_offsets(b.obj_to_img, N)
    o2i_h, objs_h = batch.obj_to_img.tolist(), batch.objs.tolist()
    points = q.stream.draw(N)
    noise, pick, u = ops.sg_qmc_unpack(points, b.obj_to_img, seg, NOISE, SLOTS)
    base = {'N': N, 'O': O, 'dimensions': q.dimension, 'bank_rows': C * ROWS, 'rep': REP}
    for name, fn in (('sg_sobol_points', lambda: ops.sg_sobol_points(q.stream.dirs, q.stream.shift, 0, N)),
                     ('sg_qmc_unpack', lambda: ops.sg_qmc_unpack(points, b.obj_to_img, seg, NOISE, SLOTS)),
                     ('sg_bank_draw', lambda: ops.sg_bank_draw(bank.bank, bank.class_off, b.objs, pick))):
        rec = dict(base, bench=name, clock='device events')
        rec.update(measure(fn, args.seconds, args.blocks, device_events=True))
        emit(args.out, rec)

    def three():
        q.stream.reset()
        _, p, _ = q.draw(b.obj_to_img, seg, N, obj_to_img_host=o2i_h)
        return bank.draw(b.objs, p, objs_host=objs_h)

    rec = dict(base, bench='draw_and_bank_draw', clock='host, ends in a synchronise')
    rec.update(measure(three, args.seconds, args.blocks))
    emit(args.out, rec)


class _Stop(Exception):
    pass


def bench_front(args, batch):
    """sample_batch up to the call of the model: the model raises at once, so the time is the sampler's own work in front of it"""
    from conftest import skip_random_init
    with skip_random_init():
        m = Model(make_vocab(), image_size=(128, 128), use_attributes=True, appearance_normalization='batch', activation='leakyrelu-0.2')
    fill_deterministic(m)
    m = m.eval().to(DEV)
    m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    feats = make_bank()
    dev = batch_to(batch, DEV)
    samplers = {'off': sample.Sampler(m, features=feats),
                'on': sample.Sampler(m, features=feats, quasi_random=qmc.QuasiRandomInputs(NOISE, max_objects=SLOTS, seed=0, device=DEV))}
    real = m.forward

    def stop(*a, **k):
        raise _Stop()

    def front(mode):
        def run():
            samplers[mode].quasi_random and samplers[mode].quasi_random.stream.reset()
            try:
                samplers[mode].sample_batch(dev)
            except _Stop:
                pass
        return run

    def whole(mode):
        def run():
            samplers[mode].quasi_random and samplers[mode].quasi_random.stream.reset()
            samplers[mode].sample_batch(dev)
        return run

    for label, make, events, hook in (('sample_batch_front', front, False, stop), ('sample_batch', whole, True, None)):
        if hook is not None:
            m.forward = hook
        try:
            for mode in samplers:
                for _ in range(3):
                    make(mode)()
            torch.cuda.synchronize()
            blocks = {'off': [], 'on': []}
            for _ in range(args.blocks):                      # alternating, so that a drift of the clocks hits both alike
                for mode in ('off', 'on'):
                    blocks[mode].append(timed_block(make(mode), args.seconds)[1 if events else 0])
        finally:
            if hook is not None:
                del m.forward
        assert m.forward.__func__ is real.__func__
        for mode in ('off', 'on'):
            rec = {'bench': label, 'quasi_random': mode, 'N': N, 'O': dev.objs.numel(), 'size': 128,
                   'clock': 'device events' if events else 'host, ends in a synchronise'}
            rec.update(summary(blocks[mode]))
            emit(args.out, rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'qmc_bench.jsonl'))
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--seconds', type=float, default=0.5)
    ap.add_argument('--only', default='', choices=['', 'calls', 'front'])
    args = ap.parse_args()
    require_device()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    emit(args.out, {'bench': 'run', 'time': time.strftime('%Y-%m-%d %H:%M:%S'), 'device': torch.cuda.get_device_name(0),
                    'seconds': args.seconds, 'blocks': args.blocks})
    batch = the_batch()
    if args.only in ('', 'calls'):
        bench_calls(args, batch)
    if args.only in ('', 'front'):
        bench_front(args, batch)


if __name__ == '__main__':
    main()
