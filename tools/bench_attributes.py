"""Benchmark of the attribute sampler (scene_generation_amd/attributes.py, csrc/attributes.hip) on cuda:0.

* one ``sample_attributes`` call (uniforms uploaded beforehand, host list of obj_to_img given: no synchronisation inside) on the
  batches of configurations c2 (N = 32, 3..8 objects, one relation per object) and c5 (N = 32, 32 objects, 96 triples per image),
  their graphs derived from their own boxes and masks: call time on the host clock around back-to-back calls that end in a device
  synchronise, the launch alone between two device events, and the numpy restatement of tests/attributes_ref.py on the same input,
  for scale.  One wavefront per image walks its triples serially, so the launch is latency, not bandwidth: no share of a peak.
* ``Sampler.sample_batch`` at N = 32 / 128 x 128 (reference default widths, predicted boxes and masks) with the option on and
  off, alternating in one process; images per second.
* the attribute-agreement fractions of ``graph_metrics`` (how often the predicted layout lands in the sampled size bucket /
  location cell) under both size rules.  The weights are the deterministic fill, not a trained model: the fractions say that the
  pipeline runs end to end, not how good a trained model is.

Every time: warmed up, then the median of ``--blocks`` blocks of at least ``--seconds`` each, with their spread, clocks as found.
One JSON line per figure, appended to profiles/attributes_bench.jsonl (or --out)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

from scene_generation_amd import attributes, ops, sample, scenegraph  # noqa: E402
from scene_generation_amd.model import Model  # noqa: E402
from scene_generation_amd.synthetic import CONFIGS, batch_to, fill_deterministic, make_batch, make_config_batch, make_vocab  # noqa: E402
from tools.benchkit import emit, measure, require_device, timed_block  # noqa: E402

DEV = 'cuda:0'


def bench_call(name, args):
    import attributes_ref
    cfg = CONFIGS[name]
    host = scenegraph.regraph(make_config_batch(name, seed=0), seed=0, pairs_per_obj=cfg['spatial_per_obj'])
    b = batch_to(host, DEV)
    stats = attributes.AttributeStats(172, device=DEV).update(b.objs, b.attributes)
    O, T = b.objs.numel(), b.triples.size(0)
    o2i_h = host.obj_to_img.tolist()
    u_h = attributes.draw_uniforms(0, O)
    u = torch.from_numpy(u_h).to(DEV)

    def call():
        return attributes.sample_attributes(b.objs, b.triples, b.obj_to_img, stats, u=u, triple_to_img=b.triple_to_img,
                                            obj_to_img_host=o2i_h)

    def launch():
        return ops.sg_sample_attributes(b.objs, b.obj_to_img, b.triples, b.triple_to_img, stats.counts, u, cfg['N'])

    base = {'config': name, 'N': cfg['N'], 'O': O, 'T': T, 'triples_per_image': T / cfg['N']}
    rec = dict(base, bench='sample_attributes', clock='host, ends in a synchronise')
    rec.update(measure(call, args.seconds, args.blocks))
    emit(args.out, rec)
    rec = dict(base, bench='sg_sample_attributes', clock='device events')
    rec.update(measure(launch, args.seconds, args.blocks, device_events=True))
    emit(args.out, rec)
    counts = stats.counts.cpu().numpy()
    np_in = [t.numpy() for t in (host.objs, host.obj_to_img, host.triples, host.triple_to_img)]
    times = []
    for _ in range(args.blocks):
        t0 = time.perf_counter()
        want = attributes_ref.sample(np_in[0], np_in[1], np_in[2], np_in[3], counts, u_h, None, cfg['N'], 10, 5)
        times.append((time.perf_counter() - t0) * 1e3)
    got = call()
    same = bool((got[1].cpu().numpy() == want[0]).all() and (got[2].cpu().numpy() == want[1]).all())
    med = statistics.median(times)
    emit(args.out, dict(base, bench='numpy_restatement', clock='host', ms=med, spread=(max(times) - min(times)) / med, blocks_ms=times,
                        equals_device=same))


def bench_sampler(args):
    from conftest import skip_random_init
    N, S = 32, 128
    with skip_random_init():
        m = Model(make_vocab(), image_size=(S, S), use_attributes=True, appearance_normalization='batch', activation='leakyrelu-0.2')
    fill_deterministic(m)
    m = m.eval().to(DEV)
    m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    batches = [scenegraph.regraph(make_batch(N=N, min_objs=3, max_objs=8, size=S, seed=2000 + k), seed=k) for k in range(4)]
    stats = attributes.build_stats(batches, 172, device=DEV)
    batch = batch_to(batches[0], DEV)
    flags = dict(use_gt_textures=True)
    samplers = {'on': sample.Sampler(m, attribute_stats=stats, sample_attributes=True), 'off': sample.Sampler(m)}
    for mode in samplers:
        for _ in range(3):
            samplers[mode].sample_batch(batch, **flags)
    torch.cuda.synchronize()
    blocks = {'on': [], 'off': []}
    for _ in range(args.blocks):
        for mode in ('on', 'off'):
            blocks[mode].append(timed_block(lambda: samplers[mode].sample_batch(batch, **flags), args.seconds)[1])
    for mode in ('on', 'off'):
        med = statistics.median(blocks[mode])
        emit(args.out, {'bench': 'sample_batch', 'N': N, 'size': S, 'sample_attributes': mode, 'ms_per_batch': med,
                        'images_per_s': 1e3 * N / med, 'blocks_ms': blocks[mode], 'spread': (max(blocks[mode]) - min(blocks[mode])) / med,
                        'clock': 'device events'})
    for rule in attributes.SIZE_RULES:
        s = sample.Sampler(m, attribute_stats=stats, sample_attributes=True, attribute_size_rule=rule, graph_metrics=True)
        for b in batches:
            s.sample_batch(b, **flags)
        g = s.graph_summary()
        emit(args.out, {'bench': 'attribute_agreement', 'size_rule': rule, 'images': N * len(batches), 'size_acc': g['size_acc'],
                        'loc_acc': g['loc_acc'], 'rel_acc': g['rel_acc'], 'weights': 'deterministic fill (untrained)'})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attributes_bench.jsonl'))
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--seconds', type=float, default=0.5)
    ap.add_argument('--configs', default='c2,c5')
    ap.add_argument('--only', default='', choices=['', 'calls', 'sampler'])
    args = ap.parse_args()
    require_device()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    emit(args.out, {'bench': 'run', 'time': time.strftime('%Y-%m-%d %H:%M:%S'), 'device': torch.cuda.get_device_name(0),
                    'seconds': args.seconds, 'blocks': args.blocks})
    if args.only in ('', 'calls'):
        for name in [c for c in args.configs.split(',') if c]:
            bench_call(name, args)
    if args.only in ('', 'sampler'):
        bench_sampler(args)


if __name__ == '__main__':
    main()
