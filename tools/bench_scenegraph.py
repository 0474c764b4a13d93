"""Benchmark of the scene-graph derivation (scene_generation_amd/scenegraph.py, csrc/scenegraph.hip) on cuda:0.

* ``graph_from_layout`` (host list of obj_to_img given: no synchronisation inside) and the agreement pair (centroids, triple
  agreement, attribute agreement) on the batches of configurations c2 (N = 32, 3..8 objects, one partner per object) and c5
  (N = 32, 32 objects, two partners): call time, launches and C-ABI calls per call.  A call here is mostly host work and launch
  latency -- the kernels move a few MB -- so the time is a host clock around back-to-back calls that end in a device
  synchronise, not a share of any peak.
* one dataset-sized pass of ``object_centers``: O = 100 000 masks of 32 x 32 int64 (0.82 GB), between two device events.  Bytes are
  the ALGORITHMIC bytes (every mask once, boxes in, centres and counts out), given as a share of the 8.0 TB/s HBM peak; the integer
  work (about twelve vector operations per element) is set against the 78.6 T lane-operations/s of the vector ALUs (256 CUs x 128
  lanes x 2.4 GHz), and the bound that applies is the larger of the two least times.

Every figure: warmed up, then the median of ``--blocks`` blocks of at least ``--seconds`` each, with their spread.  One JSON line
per figure, appended to profiles/scenegraph_bench.jsonl (or --out)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from scene_generation_amd import ops, scenegraph  # noqa: E402
from scene_generation_amd.synthetic import CONFIGS, batch_to, make_config_batch  # noqa: E402
from tools.benchkit import emit, measure, profiled, require_device  # noqa: E402

HBM_PEAK_GBS, VALU_LANE_TOPS, OPS_PER_ELEMENT = 8000.0, 78.6, 12.0
DEV = 'cuda:0'


def launches_of(fn):
    """(kernel launches of the library by kind, C-ABI calls) of one call"""
    prof, calls = profiled(fn)
    return {k: v['launches'] for k, v in prof.items() if v['launches']}, calls


def bench_batch(name, args):
    cfg = CONFIGS[name]
    r = cfg['spatial_per_obj']
    b = batch_to(make_config_batch(name, seed=0), DEV)
    o2i_h, objs_h = b.obj_to_img.tolist(), b.objs.tolist()
    O = b.objs.numel()
    u = torch.from_numpy(scenegraph.draw_uniforms(0, O, r)).to(DEV)

    def derive():
        return scenegraph.graph_from_layout(b.objs, b.boxes, b.masks, b.obj_to_img, pairs_per_obj=r, u=u, obj_to_img_host=o2i_h,
                                            objs_host=objs_h)

    triples, _, attributes = derive()
    counts = scenegraph.new_counts(7, DEV)

    def agree():
        centers = scenegraph.object_centers(b.boxes, b.masks)
        scenegraph.triple_agreement(triples, b.boxes, centers=centers, counts=counts)
        scenegraph.attribute_agreement(attributes, b.boxes, centers=centers, counts=counts)

    for what, fn in (('graph_from_layout', derive), ('agreement', agree)):
        launches, calls = launches_of(fn)
        rec = {'bench': what, 'config': name, 'N': cfg['N'], 'O': O, 'T': int(triples.size(0)), 'M': int(b.masks.size(1)),
               'pairs_per_obj': r, 'launches': launches, 'abi_calls': calls, 'clock': 'host, ends in a synchronise'}
        rec.update(measure(fn, args.seconds, args.blocks))
        emit(args.out, rec)


def bench_dataset_pass(args):
    O, M = args.objects, 32
    g = torch.Generator(device=DEV).manual_seed(0)
    masks = (torch.rand(O, M, M, device=DEV, generator=g) < 0.6).long()
    xy = torch.rand(O, 2, device=DEV, generator=g) * 0.5
    boxes = torch.cat([xy, xy + 0.1 + 0.4 * torch.rand(O, 2, device=DEV, generator=g)], 1).contiguous()
    nbytes = O * (M * M * 8 + 16 + 8 + 4)
    rec = {'bench': 'object_centers', 'O': O, 'M': M, 'dtype': 'int64', 'bytes': nbytes, 'clock': 'device events'}
    rec.update(measure(lambda: ops.sg_object_centers(boxes, masks), args.seconds, args.blocks, device_events=True))
    t_mem, t_alu = nbytes / (HBM_PEAK_GBS * 1e9) * 1e3, O * M * M * OPS_PER_ELEMENT / (VALU_LANE_TOPS * 1e12) * 1e3
    rec.update({'GBs': nbytes / rec['ms'] / 1e6, 'share_of_hbm_peak': t_mem / rec['ms'], 'least_ms_memory': t_mem,
                'least_ms_valu': t_alu, 'bound': 'memory' if t_mem >= t_alu else 'integer VALU',
                'share_of_bound': max(t_mem, t_alu) / rec['ms']})
    emit(args.out, rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scenegraph_bench.jsonl'))
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--seconds', type=float, default=0.5)
    ap.add_argument('--objects', type=int, default=100000, help='masks of the dataset-sized pass')
    ap.add_argument('--configs', default='c2,c5')
    args = ap.parse_args()
    require_device()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in [c for c in args.configs.split(',') if c]:
        bench_batch(name, args)
    bench_dataset_pass(args)


if __name__ == '__main__':
    main()
