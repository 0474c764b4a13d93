#!/usr/bin/env python
"""Capture the scene-graph goldens from the REFERENCE implementation (needs a checkout of it; CPU only).

    python tools/make_golden_scenegraph.py --reference /path/to/reference

* tests/golden/scenegraph_coco.npz: what the reference's own ``CocoSceneGraphDataset.__getitem__`` + ``coco_collate_fn``
  (scene_generation/data/coco.py, run unmodified) return for a tiny COCO-format annotation file and PIL-written images in a
  temporary directory: 24 images of 1 to 8 objects, mask_size 16.  Only the third-party imports that are absent here are stubbed
  in ``sys.modules`` (pycocotools.mask, skimage.transform, torchvision.transforms), and ``seg_to_mask`` / ``imresize`` are patched
  to small numpy rasterisers -- polygon decoding and mask resizing are not what the golden pins; lines 323-416 are.
* tests/golden/scenegraph_gui.json: what ``json_to_scene_graph`` of scripts/gui/model.py returns for five layouts that between
  them hit all six predicates (imageio and scene_generation.vis stubbed, sys.argv set for its argument parser).

Before a fixture is written, the float64 restatement of tests/scenegraph_ref.py must reproduce it, and every decision in it must
be robust: each argument of a round() at least 1e-3 away from a half-integer, each | |dx| - |dy| | and each strict box comparison
at least 1e-3 wide.  A seed that misses is skipped for the next.  The device's decisions must then EQUAL the golden.
Only recorded inputs and outputs are written; no reference source travels."""
import argparse
import importlib.util
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
import PIL.Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'tests', 'golden')
MASK_SIZE, MARGIN = 16, 1e-3

import scenegraph_ref as R  # noqa: E402


def _module(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def install_stubs():
    """absent third-party modules only; everything of the reference itself is imported as it is"""
    class Compose(object):
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, img):                        # the pixels are not part of the golden
            return torch.zeros(3, 1, 1)

    class _Plain(object):
        def __init__(self, *a, **k):
            pass

    tr = _module('torchvision.transforms', Compose=Compose, ToTensor=_Plain, Normalize=_Plain)
    tv = _module('torchvision', transforms=tr)
    for sub in ('models', 'utils'):
        setattr(tv, sub, _module('torchvision.' + sub))
    _module('pycocotools.mask')
    _module('pycocotools', mask=sys.modules['pycocotools.mask'])
    _module('skimage.transform', resize=None)
    _module('skimage', transform=sys.modules['skimage.transform'])


def rasterise(seg, width, height):
    """stands in for seg_to_mask: ``seg`` = {'shape': 'ellipse' | 'rect' | 'none', 'box': [x, y, w, h] in pixels} -> uint8 (H, W)"""
    ys, xs = np.mgrid[0:int(height), 0:int(width)]
    x, y, w, h = seg['box']
    if seg['shape'] == 'none':
        return np.zeros((int(height), int(width)), np.uint8)
    if seg['shape'] == 'rect':
        return ((xs + 0.5 >= x) & (xs + 0.5 <= x + w) & (ys + 0.5 >= y) & (ys + 0.5 <= y + h)).astype(np.uint8)
    cx, cy = x + w / 2.0, y + h / 2.0
    return ((((xs + 0.5 - cx) / (w / 2.0)) ** 2 + ((ys + 0.5 - cy) / (h / 2.0)) ** 2) <= 1.0).astype(np.uint8)


def resize_nearest(img, shape, mode=None, anti_aliasing=None):
    """stands in for skimage.transform.resize: the value at the centre of every output cell"""
    H, W = img.shape
    rows = np.minimum(((np.arange(shape[0]) + 0.5) * H / shape[0]).astype(int), H - 1)
    cols = np.minimum(((np.arange(shape[1]) + 0.5) * W / shape[1]).astype(int), W - 1)
    return img[rows][:, cols]


def make_dataset_files(directory, rs):
    """24 images (64 x 48 ... 96 x 80 pixels) of 1..8 objects: the first three hold 1, 2 and 8; boxes partly nested, masks as
    ellipses, off-centre rectangles or nothing at all"""
    images, annotations = [], []
    counts = [1, 2, 8] + [int(rs.randint(1, 9)) for _ in range(21)]
    aid = 1
    for n, k in enumerate(counts):
        W, H = int(rs.choice([64, 80, 96])), int(rs.choice([48, 64, 80]))
        name = 'img%02d.png' % n
        PIL.Image.new('RGB', (W, H), (n * 9 % 256, 90, 160)).save(os.path.join(directory, name))
        images.append({'id': 100 + n, 'file_name': name, 'width': W, 'height': H})
        boxes = []
        for i in range(k):
            if i and rs.rand() < 0.3:                   # nested in an earlier box: inside / surrounding
                px, py, pw, ph = boxes[int(rs.randint(0, i))]
                w, h = pw * rs.uniform(0.5, 0.8), ph * rs.uniform(0.5, 0.8)
                x, y = px + (pw - w) * rs.uniform(0.2, 0.8), py + (ph - h) * rs.uniform(0.2, 0.8)
            else:
                w, h = W * rs.uniform(0.2, 0.7), H * rs.uniform(0.2, 0.7)
                x, y = (W - w) * rs.rand(), (H - h) * rs.rand()
            box = [float(x), float(y), float(w), float(h)]
            boxes.append(box)
            shape = ['ellipse', 'rect', 'rect', 'none'][int(rs.randint(0, 4))] if i else 'ellipse'
            part = box if shape != 'rect' else [box[0], box[1], box[2] * rs.uniform(0.3, 1.0), box[3] * rs.uniform(0.3, 1.0)]
            annotations.append({'id': aid, 'image_id': 100 + n, 'category_id': int(rs.randint(1, 7)), 'bbox': box,
                                'segmentation': {'shape': shape, 'box': [float(v) for v in part]}})
            aid += 1
    categories = [{'id': c, 'name': 'thing%d' % c} for c in range(1, 7)]
    path = os.path.join(directory, 'instances.json')
    with open(path, 'w') as f:
        json.dump({'images': images, 'annotations': annotations, 'categories': categories}, f)
    return path


def capture_coco(seed):
    from scene_generation.data import coco
    coco.seg_to_mask = rasterise
    coco.imresize = resize_nearest
    rs = np.random.RandomState(seed)
    with tempfile.TemporaryDirectory() as d:
        inst = make_dataset_files(d, rs)
        ds = coco.CocoSceneGraphDataset(d, inst, stuff_json=None, stuff_only=False, image_size=(32, 32), mask_size=MASK_SIZE,
                                        min_objects_per_image=1, max_objects_per_image=8)
        random.seed(seed)
        batch = coco.coco_collate_fn([ds[i] for i in range(len(ds))])
    _, objs, boxes, masks, triples, obj_to_img, triple_to_img, attributes = batch
    return dict(objs=objs.numpy(), boxes=boxes.numpy(), masks=masks.numpy().astype(np.uint8), triples=triples.numpy(),
                obj_to_img=obj_to_img.numpy(), triple_to_img=triple_to_img.numpy(), attributes=attributes.numpy())


def check_coco(g):
    """the restatement reproduces the capture, with room to spare at every decision; -> error text or None"""
    assert g['boxes'].dtype == np.float32 and g['attributes'].shape[1] == 35
    centers = R.centers_ref(g['boxes'], g['masks'])[0].astype(np.float32)
    _, _, hot = R.attributes_ref(g['boxes'], centers)
    if not np.array_equal(hot, g['attributes']):
        return 'attributes differ'
    spatial = g['triples'][g['triples'][:, 1] > 0]
    s, o = spatial[:, 0], spatial[:, 2]
    if not np.array_equal(R.predicates_ref(g['boxes'], centers, s, o), spatial[:, 1]):
        return 'predicates differ'
    if not np.array_equal(R.predicates_ref(g['boxes'], centers, s, o, R.angle_class_cmp), spatial[:, 1]):
        return 'comparison form differs'
    r, ang, box = R.margins(g['boxes'], centers, s, o)
    if min(r, ang, box) < MARGIN:
        return 'margins %.2e %.2e %.2e' % (r, ang, box)
    return None


GUI_LAYOUTS = [
    {'image_id': 1, 'objects': [
        {'text': 'sky-other', 'left': 0.0, 'top': 0.0, 'width': 1.0, 'height': 0.45, 'size': 9, 'location': 2, 'feature': -1},
        {'text': 'tree', 'left': 0.4, 'top': 0.1, 'width': 0.2, 'height': 0.2, 'size': 1, 'location': 7, 'feature': 3},
        {'text': 'grass', 'left': 0.0, 'top': 0.6, 'width': 1.0, 'height': 0.4, 'size': 8, 'location': 22, 'feature': -1}]},
    {'image_id': 2, 'objects': [
        {'text': 'person', 'left': 0.45, 'top': 0.45, 'width': 0.1, 'height': 0.12, 'size': 0, 'location': 12, 'feature': 5},
        {'text': 'building-other', 'left': 0.2, 'top': 0.2, 'width': 0.6, 'height': 0.6, 'size': 6, 'location': 12, 'feature': -1},
        {'text': 'car', 'left': 0.7, 'top': 0.55, 'width': 0.25, 'height': 0.15, 'size': 2, 'location': 14, 'feature': 40}]},
    {'image_id': 3, 'objects': [
        {'text': 'boat', 'left': 0.05, 'top': 0.5, 'width': 0.2, 'height': 0.1, 'size': 1, 'location': 10, 'feature': 0},
        {'text': 'sea', 'left': 0.6, 'top': 0.55, 'width': 0.3, 'height': 0.2, 'size': 3, 'location': 13, 'feature': -1},
        {'text': 'clouds', 'left': 0.55, 'top': 0.05, 'width': 0.3, 'height': 0.15, 'size': 2, 'location': 3, 'feature': 7},
        {'text': 'mountain', 'left': 0.1, 'top': 0.2, 'width': 0.3, 'height': 0.2, 'size': 2, 'location': 6, 'feature': -1}]},
    {'image_id': 4, 'objects': [
        {'text': 'dog', 'left': 0.3, 'top': 0.7, 'width': 0.15, 'height': 0.15, 'size': 1, 'location': 16, 'feature': 12},
        {'text': 'frisbee', 'left': 0.32, 'top': 0.2, 'width': 0.1, 'height': 0.08, 'size': 0, 'location': 6, 'feature': -1}]},
    {'image_id': 5, 'objects': [
        {'text': 'bench', 'left': 0.25, 'top': 0.4, 'width': 0.5, 'height': 0.3, 'size': 4, 'location': 12, 'feature': 9}]},
]


def capture_gui(reference):
    _module('imageio', imwrite=None)
    _module('scene_generation.vis')
    argv = sys.argv
    sys.argv = ['model.py', '--checkpoint', 'none']
    try:
        spec = importlib.util.spec_from_file_location('reference_gui_model', os.path.join(reference, 'scripts', 'gui', 'model.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return [mod.json_to_scene_graph(json.dumps(layout)) for layout in GUI_LAYOUTS]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', default=os.environ.get('SG_REFERENCE_DIR'), help='checkout of the reference implementation')
    ap.add_argument('--seed', type=int, default=0, help='first seed tried')
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(os.path.join(args.reference, 'scene_generation')):
        ap.error('--reference (or SG_REFERENCE_DIR) must name a checkout that holds scene_generation/')
    sys.path.insert(0, args.reference)
    install_stubs()

    for seed in range(args.seed, args.seed + 50):
        g = capture_coco(seed)
        why = check_coco(g)
        if why is None:
            break
        print('seed %d: %s -- next' % (seed, why))
    else:
        raise SystemExit('no seed gave a robust golden')
    preds = sorted(set(g['triples'][:, 1].tolist()))
    assert preds == list(range(7)), 'all predicates must occur: %s' % preds
    sizes = np.bincount(g['obj_to_img'])
    assert sizes.min() == 2 and 3 in sizes and (g['masks'].reshape(len(g['masks']), -1).sum(1) == 0).any()
    path = os.path.join(OUT, 'scenegraph_coco.npz')
    np.savez_compressed(path, seed=np.int64(seed), **g)
    print('scenegraph_coco.npz  seed %d  %d images, %d objects, %d triples  %.1f KB' %
          (seed, sizes.size, g['objs'].size, g['triples'].shape[0], os.path.getsize(path) / 1024))

    graphs = capture_gui(args.reference)
    used = {r[1] for gs in graphs for sg in gs for r in sg['relationships']}
    assert used == set(R.PRED_NAMES[1:]), 'the layouts must hit all six predicates: %s' % sorted(used)
    for layout, want in zip(GUI_LAYOUTS, graphs):
        assert R.gui_scene_graphs_ref(layout) == want, layout['image_id']
    path = os.path.join(OUT, 'scenegraph_gui.json')
    with open(path, 'w') as f:
        json.dump({'layouts': GUI_LAYOUTS, 'scene_graphs': graphs}, f, indent=1)
    print('scenegraph_gui.json  %d layouts  %.1f KB' % (len(graphs), os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
