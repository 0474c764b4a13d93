"""The appearance bank, built on the GPU (surface of the reference's scripts/encode_features.py):

    python -m scene_generation_amd.bank --checkpoint CKPT.pt [--weights ema] [--output_dir DIR] [--n_clusters 100,10,1]

writes ``features.npy`` and ``features_clustered_{100,010,001}.npy`` next to the checkpoint, where ``scene_generation_amd.sample``
(and a reference checkout) looks for them.

* ``encode``: ``repr_net(image_encoder(crop))`` of every object of a loader; rows and class ids stay on the device and are sorted by
  class once with a stable sort -> (x [P, D] fp32, offsets [C + 1] int32).
* ``kmeans_segmented``: Lloyd's k-means of EVERY class in the same launches (csrc/kmeans.hip), in fp32, seeded by plain k-means++
  with one trial per round from a table of uniforms drawn on the host (NOT scikit-learn's greedy variant with 2 + log k trials),
  empty clusters relocated by scikit-learn's rule, convergence kept per class on the device and read by the host every
  ``HOST_STRIDE`` iterations.  Deterministic: the same inputs and seed give the same bits, and a class's result does not depend
  on the other classes.
* ``order_centers``: the reference sorts a class's centres along an (unseeded) 1-D t-SNE so that the GUI's appearance slider
  moves smoothly; the default here is the projection on the first principal axis, which is deterministic.
* ``build_bank`` / ``save_bank`` / ``run`` / the command line.
``evaluate.encode_features`` / ``evaluate.cluster_features`` (the host / scikit-learn forms) stay as they are."""
import argparse
import os
import time

import numpy as np
import torch

from . import ops
from .bilinear import crop_bbox_batch
from .utils import int_tuple

# The host reads the per-class ``state`` flags once every HOST_STRIDE Lloyd iterations (one small device-to-host copy and the
# synchronisation that goes with it).  Iterations issued after the last class finished cost three launches whose workgroups exit
# at once.  Measured on MI355X (tools/bench_bank.py; 400 000 rows, 184 classes, K = 100, median of five runs
# alternating in one process): 13.21 / 12.97 / 12.85 ms for a stride of 2 / 4 / 8 with spreads of 0.3 ms -- no difference beyond the
# spread, so the middle one stays (at most three idle iterations).
HOST_STRIDE = 4
FILES = {'features': 'features.npy', 100: 'features_clustered_100.npy', 10: 'features_clustered_010.npy', 1: 'features_clustered_001.npy'}


def bank_file(k):
    """file name of the bank with ``k`` centres per class (the reference's three, and the same pattern for any other k)"""
    return FILES[k] if k in FILES else 'features_clustered_%03d.npy' % k


class KMeansResult(object):
    """centers [C, K, D] fp32 (class c: its first k[c] rows), k [C], counts [C, K], labels [P], inertia [C], n_iter [C] on the device;
    ``host_reads``: device-to-host reads of the convergence flags; ``picks`` [C, K]: the seeding rows (k-means++ only)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def draw_uniforms(seed, n_init, C, K):
    """the table of uniforms of the k-means++ rounds: numpy.random.RandomState(seed).random_sample((n_init, C, K)) as fp32, kept
    below 1"""
    u = np.random.RandomState(seed).random_sample((n_init, C, K)).astype(np.float32)
    return np.minimum(u, np.float32(1.0 - 2.0 ** -24))


def kmeans_segmented(x, offsets, n_clusters, init='k-means++', seed=0, n_init=1, max_iter=300, tol=1e-4, u=None,
                     host_stride=None):
    """Lloyd's k-means of every class of x [P, D] (rows grouped by class, offsets [C + 1] int32) with up to ``n_clusters`` centres
    per class (a class with fewer rows gets one centre per row).  ``init``: 'k-means++' -- plain k-means++ with ONE trial per round
    (scikit-learn's default is the greedy variant: this one is the textbook algorithm), driven by the table ``u`` [n_init, C, K] of
    uniforms (default: ``draw_uniforms(seed, ...)``), or a tensor [C, K, D] of initial centres.  ``tol`` is scikit-learn's: a class
    stops when its squared centre shift is at most tol * (mean per-dimension variance of its rows), or when no label changed.  With
    ``n_init`` > 1 the restarts run as more problems of the same launches and the one with the lowest inertia is kept per class."""
    plan = ops.kmeans_plan(offsets)
    x = ops._f32(x, 'x')
    dev, P, C, K, D = x.device, plan.P, plan.C, int(n_clusters), x.size(1)
    explicit = torch.is_tensor(init)
    R = 1 if explicit else int(n_init)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    labels = torch.full((R, P), -1, **i32)
    mind2 = torch.zeros(R, P, **f32)
    changed, acount, counts = torch.zeros(R, C, **i32), torch.zeros(R, C, K, **i32), torch.zeros(R, C, K, **i32)
    state, n_iter = torch.zeros(R, C, **i32), torch.zeros(R, C, **i32)
    inertia, shift = torch.zeros(R, C, **f32), torch.zeros(R, C, **f32)
    sizes = torch.from_numpy(plan.sizes).to(dev)
    # scikit-learn's tolerance: tol * mean_d var_d(x) per class, from the kernels themselves (k = 1: mean, then the distances to it)
    tolvar = torch.zeros(C, **f32)
    if tol > 0 and P > 0:
        c1, l1 = torch.zeros(1, C, 1, D, **f32), torch.zeros(1, P, **i32)
        m1, n1, i1, s1 = torch.zeros(1, P, **f32), torch.zeros(1, C, 1, **i32), torch.zeros(1, C, **f32), torch.zeros(1, C, **f32)
        ch1, a1 = torch.zeros(1, C, **i32), torch.zeros(1, C, 1, **i32)
        ops.kmeans_update(x, plan, l1, m1, c1, n1, i1, s1)
        ops.kmeans_assign(x, plan, c1, l1, m1, ch1, a1)
        ops.kmeans_update(x, plan, l1, m1, c1, n1, i1, s1, final_pass=True)
        tolvar = (i1[0] / (sizes.clamp(min=1).to(torch.float32) * D) * float(tol)).contiguous()
    picks = None
    if explicit:
        centers = ops._f32(init, 'init').reshape(1, C, K, D).clone()
    else:
        if init != 'k-means++':
            raise ValueError("init must be 'k-means++' or a tensor [C, K, D]")
        if u is None:
            u = draw_uniforms(seed, R, C, K)
        u = torch.as_tensor(u, dtype=torch.float32).reshape(R, C, K).contiguous().to(dev)
        centers, picks = torch.zeros(R, C, K, D, **f32), torch.full((R, C, K), -1, **i32)
        for t in range(K):                                       # no host synchronisation: K launches back to back
            ops.kmeans_pp_step(x, plan, u, centers, mind2, picks, t)
    stride = int(host_stride or HOST_STRIDE)
    host_reads, issued = 0, 0
    for it in range(int(max_iter)):
        ops.kmeans_assign(x, plan, centers, labels, mind2, changed, acount, state)
        ops.kmeans_relocate(plan, labels, mind2, acount, state)
        ops.kmeans_update(x, plan, labels, mind2, centers, counts, inertia, shift, tolvar, state, n_iter, changed, acount)
        issued = it + 1
        if issued % stride == 0:
            host_reads += 1
            if state.cpu().numpy().all():                        # the loop's only device-to-host read: a plain copy, no kernel
                break
    # the classes that stopped on the centre shift (or on max_iter) get the labels and the inertia of their final centres
    ops.kmeans_assign(x, plan, centers, labels, mind2, changed, acount, state, final_pass=True)
    ops.kmeans_update(x, plan, labels, mind2, centers, counts, inertia, shift, tolvar, state, n_iter, changed, acount, final_pass=True)
    kc = sizes.clamp(max=K).to(torch.int32)
    if R > 1:
        # the FIRST restart with the lowest inertia (argmin leaves the choice among equals open)
        ridx = torch.arange(R, device=dev).unsqueeze(1).expand(R, C)
        best = torch.where(inertia == inertia.min(0).values, ridx, torch.full_like(ridx, R - 1)).min(0).values     # [C]
        cidx = torch.arange(C, device=dev)
        row_class = torch.repeat_interleave(cidx, sizes)
        labels = labels.gather(0, best[row_class].unsqueeze(0))[0]
        centers, counts, inertia, n_iter = centers[best, cidx], counts[best, cidx], inertia[best, cidx], n_iter[best, cidx]
        picks = picks[best, cidx] if picks is not None else None
    else:
        labels, centers, counts, inertia, n_iter = labels[0], centers[0], counts[0], inertia[0], n_iter[0]
        picks = picks[0] if picks is not None else None
    return KMeansResult(centers=centers, k=kc, counts=counts, labels=labels, inertia=inertia, n_iter=n_iter, picks=picks,
                        host_reads=host_reads, iterations_issued=issued, tolvar=tolvar)


def encode(model, loader, object_size=64, max_objects=None):
    """``repr_net(image_encoder(crop))`` of every object of ``loader`` (the calls of evaluate.encode_features), kept on the device:
    -> (x [P, D] fp32 sorted by class with a STABLE sort, so a class's rows keep loader order; offsets [C + 1] int32).  No
    device-to-host copy per batch.  The model is used in whatever mode it is in."""
    device = next(model.parameters()).device
    num_objs = len(model.vocab['object_to_idx'])
    feats, ids, count = [], [], 0
    with torch.no_grad():
        for data in loader:
            imgs, objs, boxes, obj_to_img = data[0].to(device), data[1].to(device), data[2].to(device), data[5].to(device)
            feats.append(model.repr_net(model.image_encoder(crop_bbox_batch(imgs, boxes, obj_to_img, object_size))).float())
            ids.append(objs)
            count += objs.numel()
            if max_objects is not None and count >= max_objects:
                break
    if not feats:
        return (torch.zeros(0, getattr(model, 'rep_size', 0), device=device),
                torch.zeros(num_objs + 1, dtype=torch.int32, device=device))
    x, ids = torch.cat(feats, 0), torch.cat(ids, 0)
    ids, order = torch.sort(ids, stable=True)
    offsets = torch.zeros(num_objs + 1, dtype=torch.int32, device=device)
    offsets[1:] = torch.cumsum(torch.bincount(ids, minlength=num_objs), 0).to(torch.int32)
    return x[order].contiguous(), offsets


def order_centers(centers, how='pc1', return_order=False):
    """A class's centres [k, D] sorted for the appearance slider.  'pc1' (default): by the projection on the first principal axis of
    the centres (fp64), the axis signed so that its component of largest magnitude is positive -- deterministic.  'tsne': along a
    1-D t-SNE like the reference (scikit-learn, imported here only; not reproducible).  'none': as they are."""
    c = np.asarray(centers, dtype=np.float64)
    k = c.shape[0]
    if how == 'none' or k <= 1:
        order = np.arange(k)
    elif how == 'pc1':
        z = c - c.mean(0)
        axis = np.linalg.svd(z, full_matrices=False)[2][0]
        if axis[np.argmax(np.abs(axis))] < 0:
            axis = -axis
        order = np.argsort(z @ axis, kind='stable')
    elif how == 'tsne':
        from sklearn.manifold import TSNE
        order = np.argsort(TSNE(n_components=1, perplexity=min(30.0, k - 1.0)).fit_transform(c).reshape(-1))
    else:
        raise ValueError("order must be 'pc1', 'tsne' or 'none'")
    return (c[order], order) if return_order else c[order]


def cluster_bank(x, offsets, n_clusters=(100, 10, 1), seed=0, n_init=1, order='pc1', max_iter=300, tol=1e-4, report=None):
    """the clustered dicts of a bank: {k: {label: float64 [k_c, D]}} for the classes that have rows"""
    sizes = np.diff(offsets.cpu().numpy())
    out = {}
    for k in n_clusters:
        t0 = time.time()
        res = kmeans_segmented(x, offsets, k, seed=seed, n_init=n_init, max_iter=max_iter, tol=tol)
        cen = res.centers.cpu().numpy()
        iters, inertia = res.n_iter.cpu().numpy(), res.inertia.cpu().numpy()
        out[k] = {int(c): order_centers(cen[c, :min(int(n), k)], order) for c, n in enumerate(sizes) if n > 0}
        if report is not None:
            live = sizes > 0
            report.append({'k': int(k), 'classes': int(live.sum()), 'max_iter': int(iters[live].max()) if live.any() else 0,
                           'mean_iter': float(iters[live].mean()) if live.any() else 0.0,
                           'inertia': float(inertia[live].astype(np.float64).sum()), 'seconds': time.time() - t0,
                           'host_reads': res.host_reads})
    return out


def build_bank(model, loader, n_clusters=(100, 10, 1), object_size=64, max_objects=None, seed=0, n_init=1, order='pc1',
               max_iter=300, tol=1e-4, report=None):
    """-> {'features': {label: float64 [n_c, D]} for EVERY label (empty arrays for classes without rows), k: {label: float64
    [k_c, D]} for every k of ``n_clusters`` and the classes with rows}: the reference's formats (float64 throughout, as
    encode_features.py:121,133 makes them)."""
    x, offsets = encode(model, loader, object_size, max_objects)
    off = offsets.cpu().numpy()
    rows = x.cpu().numpy().astype(np.float64)
    bank = {'features': {c: rows[off[c]:off[c + 1]] for c in range(len(off) - 1)}}
    bank.update(cluster_bank(x, offsets, n_clusters, seed, n_init, order, max_iter, tol, report))
    return bank


def save_bank(bank, directory):
    """features.npy and features_clustered_{100,010,001}.npy: pickled dicts that ``np.load(allow_pickle=True).item()`` reads;
    -> the paths written"""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for key, value in bank.items():
        path = os.path.join(directory, bank_file(key))
        np.save(path, {int(c): np.asarray(v, dtype=np.float64) for c, v in value.items()}, allow_pickle=True)
        paths.append(path)
    return paths


def run(args, checkpoint, loader=None, device='cuda'):
    """checkpoint -> bank files (``loader``: any iterable of collated batches; the synthetic generator when None)"""
    from .sample import build_model, synthetic_loader
    model = build_model(args, checkpoint, device)
    if loader is None:
        loader = synthetic_loader(model, args.batch_size, args.num_samples, checkpoint['model_kwargs'].get('mask_size', 32))
    out_dir = args.output_dir or os.path.dirname(os.path.abspath(args.checkpoint))
    report = []
    t0 = time.time()
    bank = build_bank(model, loader, tuple(args.n_clusters), seed=args.seed, n_init=args.n_init, order=args.order, report=report)
    rows = sum(v.shape[0] for v in bank['features'].values())
    print('encoded %d objects of %d classes' % (rows, sum(1 for v in bank['features'].values() if v.shape[0])))
    for rec in report:
        print('k = %(k)d: %(classes)d classes clustered, iterations max %(max_iter)d mean %(mean_iter).1f, '
              'total inertia %(inertia).6g, %(seconds).3f s' % rec)
    paths = save_bank(bank, out_dir)
    print('wrote %s in %.2f s' % (', '.join(os.path.basename(p) for p in paths), time.time() - t0))
    return {'paths': paths, 'report': report, 'bank': bank}


def make_parser():
    from .sample import WEIGHT_KEYS
    p = argparse.ArgumentParser(prog='python -m scene_generation_amd.bank', description=__doc__.split('\n')[0])
    p.add_argument('--checkpoint', required=True)
    p.add_argument('--weights', default='model', choices=sorted(WEIGHT_KEYS),
                   help='model_state / model_best_state / model_ema_state / model_ema_best_state of the checkpoint')
    p.add_argument('--output_dir', default=None, help="default: the checkpoint's directory, where the sampler looks")
    p.add_argument('--model_mode', default='eval', choices=['train', 'eval'])
    p.add_argument('--num_samples', default=1024, type=int, help='images from the synthetic generator when no loader is given')
    p.add_argument('--batch_size', default=24, type=int)
    p.add_argument('--n_clusters', default=(100, 10, 1), type=int_tuple)
    p.add_argument('--seed', default=0, type=int)
    p.add_argument('--n_init', default=1, type=int)
    p.add_argument('--order', default='pc1', choices=['pc1', 'tsne', 'none'])
    return p


def main(argv=None):
    args = make_parser().parse_args(argv)
    checkpoint = torch.load(args.checkpoint, map_location='cpu', weights_only=False)
    print('Loading model from ', args.checkpoint)
    return run(args, checkpoint)


if __name__ == '__main__':
    main()
