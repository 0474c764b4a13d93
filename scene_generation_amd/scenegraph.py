"""Scene graphs from layouts, on the device, and how well a layout honours a graph.

The reference derives a scene graph from boxes and masks inside ``CocoSceneGraphDataset.__getitem__`` (data/coco.py:323-416), in
Python loops over objects: a mask centroid per object, from it the size and location attribute bits, and for a randomly drawn
partner one of six geometric predicates.  Here the same rules are launches over a collated batch (csrc/scenegraph.hip, exact rules
in include/sg2im_hip.h and DESIGN.md section 4e):

* ``object_centers`` / ``attributes_from_layout`` / ``predicates``: the three parts, usable on their own.
* ``graph_from_layout``: (triples, triple_to_img, attributes) of a batch in the collate order of coco.py:358-413,501-547, the
  partner draw driven by a table of uniforms drawn once on the host.  ``regraph`` applies it to a ``synthetic.Batch``, whose random
  predicates and attributes then agree with its own boxes and masks.
* ``triple_agreement`` / ``attribute_agreement`` / ``summary``: integer counters, accumulated on the device and read ONCE, of the
  triples (per predicate) and attribute bits that the geometry of a layout -- e.g. the boxes and masks a sampler predicted --
  agrees with.
* ``layout_json_to_scene_graphs``: the layouts a drawing front end sends (scripts/gui/model.py:111-180) to the scene-graph
  dictionaries ``Model.encode_scene_graphs`` takes.  Host only: a handful of objects.

Every object id is global (collated), every image ends with its ``__image__`` object, and nothing but ``summary`` (and
``graph_from_layout`` without a host copy of ``obj_to_img``) synchronises with the host."""
import json
import math

import numpy as np
import torch

from . import ops
from .utils import to_device_async

PREDICATES = ['__in_image__', 'left of', 'right of', 'above', 'below', 'inside', 'surrounding']      # coco.py:18,206
SIZE_LEN, GRID = 10, 5                                                                              # coco.py:25-26 (25 = 5 x 5 cells)


def object_centers(boxes, masks, return_count=False):
    """centers [O, 2] fp32: the mean box coordinate of the set mask elements (coco.py:326-341); an empty mask gives the box centre"""
    centers, count = ops.sg_object_centers(boxes, masks)
    return (centers, count) if return_count else centers


def attributes_from_layout(boxes, masks, size_len=SIZE_LEN, grid=GRID, centers=None):
    """-> (attributes [O, size_len + grid * grid] fp32 one-hot blocks, size_idx [O] int32, loc_idx [O] int32); coco.py:296,347"""
    if centers is None:
        centers = object_centers(boxes, masks)
    size_idx, loc_idx, block = ops.sg_object_attributes(boxes, centers, size_len, grid)
    return block, size_idx, loc_idx


def predicates(boxes, centers, s, o):
    """p [T] int64 (index into PREDICATES) of the pairs (s[t], o[t]) of global object ids; coco.py:368-385"""
    return ops.sg_pair_predicates(boxes, centers, s, o)


def draw_uniforms(seed, O, pairs_per_obj=1):
    """the table of the partner draw: numpy.random.RandomState(seed).random_sample((O, pairs_per_obj, 2)) as fp32, kept below 1"""
    u = np.random.RandomState(seed).random_sample((O, pairs_per_obj, 2)).astype(np.float32)
    return np.minimum(u, np.float32(1.0 - 2.0 ** -24))


def triple_offsets(seg_off, pairs_per_obj=1):
    """tri_off [N + 1] (host list) from the object offsets: an image with k real objects owns k __in_image__ triples and, when
    k >= 2, k * pairs_per_obj spatial ones (coco.py:359-361,409-413)"""
    off = [0]
    for a, b in zip(seg_off, seg_off[1:]):
        k = b - a - 1
        if k < 0:
            raise ValueError('every image needs at least its __image__ object')
        off.append(off[-1] + k + (k * pairs_per_obj if k >= 2 else 0))
    return off


def graph_from_layout(objs, boxes, masks, obj_to_img, pairs_per_obj=1, seed=0, u=None, obj_to_img_host=None, objs_host=None,
                      image_class=0, size_len=SIZE_LEN, grid=GRID):
    """-> (triples [T, 3] int64, triple_to_img [T] int64, attributes [O, size_len + grid * grid] fp32) derived from the layout.

    ``u`` [O, pairs_per_obj, 2]: uniforms in [0, 1) (numpy or tensor; default ``draw_uniforms(seed, ...)``), uploaded before the first
    launch; row o belongs to object o, so an image's graph does not depend on where the image stands in the batch.
    ``obj_to_img_host``: the host list of obj_to_img (DeviceBatchPrefetcher carries one).  Without it the call reads obj_to_img back
    once -- its only synchronisation.  With ``objs_host`` as well, an image whose last object is not ``image_class`` raises."""
    from .pipeline import segment_offsets
    dev = boxes.device
    ops._dev(boxes, 'boxes')
    O = boxes.size(0)
    if obj_to_img_host is None:
        obj_to_img_host = obj_to_img.tolist()                   # the documented read
    if len(obj_to_img_host) != O:
        raise ValueError('obj_to_img has %d entries for %d boxes' % (len(obj_to_img_host), O))
    N = obj_to_img_host[-1] + 1 if O else 0
    seg = segment_offsets(obj_to_img_host, N)
    if objs_host is not None:
        for n in range(N):
            if seg[n + 1] == seg[n] or objs_host[seg[n + 1] - 1] != image_class:
                raise ValueError('image %d does not end with the __image__ object (class %d)' % (n, image_class))
    tri = triple_offsets(seg, pairs_per_obj)
    if u is None:
        u = draw_uniforms(seed, O, pairs_per_obj)
    if not torch.is_tensor(u):
        u = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32))
    if tuple(u.shape) != (O, pairs_per_obj, 2):
        raise ValueError('u must be [%d, %d, 2], got %s' % (O, pairs_per_obj, tuple(u.shape)))
    u = to_device_async(u, dev) if not u.is_cuda else u
    offs = to_device_async(torch.tensor([seg, tri], dtype=torch.int32), dev)
    centers = object_centers(boxes, masks)
    attributes, _, _ = attributes_from_layout(boxes, masks, size_len, grid, centers=centers)
    triples, triple_to_img = ops.sg_draw_pairs(offs[0], offs[1], u, boxes, centers, tri[-1])
    return triples, triple_to_img, attributes


def regraph(batch, seed=0, pairs_per_obj=1):
    """a ``synthetic.Batch`` (host or device) with triples, triple_to_img and attributes replaced by the ones its own boxes and
    masks imply.  A host batch is computed on the current GPU and comes back on the host."""
    from .synthetic import Batch
    on_host = not batch.boxes.is_cuda
    dev = torch.device('cuda', torch.cuda.current_device()) if on_host else batch.boxes.device
    objs, boxes, masks, o2i = [t.to(dev) for t in (batch.objs, batch.boxes, batch.masks, batch.obj_to_img)]
    host = (batch.obj_to_img.tolist(), batch.objs.tolist()) if on_host else torch.stack((batch.obj_to_img, batch.objs)).tolist()
    triples, t2i, attributes = graph_from_layout(objs, boxes, masks, o2i, pairs_per_obj, seed, obj_to_img_host=host[0],
                                                 objs_host=host[1])
    if batch.attributes.size(1) != attributes.size(1):
        raise ValueError('the batch carries %d attribute bits, the derived block has %d' % (batch.attributes.size(1), attributes.size(1)))
    if on_host:
        triples, t2i, attributes = triples.cpu(), t2i.cpu(), attributes.cpu()
    return Batch(batch.imgs, batch.objs, batch.boxes, batch.masks, triples, batch.obj_to_img, t2i, attributes)


# ---- agreement -------------------------------------------------------------------------------------------------------------------
def new_counts(num_preds, device):
    """the accumulator of both agreement calls: int64 [num_preds + 2, 2]; rows [:num_preds] per predicate (seen, agreeing), row
    num_preds the size bits, row num_preds + 1 the location bits"""
    return torch.zeros(num_preds + 2, 2, dtype=torch.int64, device=device)


def triple_agreement(triples, boxes, masks=None, centers=None, counts=None, num_preds=len(PREDICATES)):
    """adds, per predicate p >= 1, the triples seen and those whose predicate derived from (boxes, centers) equals p.  ``counts``:
    an accumulator of ``new_counts`` (returned; a fresh one when None)."""
    if centers is None:
        centers = object_centers(boxes, masks)
    if counts is None:
        counts = new_counts(num_preds, boxes.device)
    P = counts.size(0) - 2
    ops.sg_triple_agreement(triples, boxes, centers, P, counts=counts[:P])
    return counts


def attribute_agreement(attributes, boxes, masks=None, centers=None, counts=None, num_preds=len(PREDICATES), size_len=SIZE_LEN,
                        grid=GRID):
    """adds the objects whose given size (location) block has exactly one bit set and those whose bit is the one derived from
    (boxes, centers); rows without a bit -- attributes that were not specified -- count for nothing"""
    if centers is None:
        centers = object_centers(boxes, masks)
    if counts is None:
        counts = new_counts(num_preds, boxes.device)
    size_idx, loc_idx, _ = ops.sg_object_attributes(boxes, centers, size_len, grid, onehot=False)
    ops.sg_attribute_agreement(attributes, size_idx, loc_idx, size_len, grid, counts=counts[counts.size(0) - 2:])
    return counts


def summary(counts, vocab=None):
    """the ONE device-to-host read: {'rel_acc', 'rel_acc_by_pred': {name: (agree, seen)}, 'size_acc', 'loc_acc'} (NaN when nothing
    was seen)"""
    rows = counts.tolist()
    P = len(rows) - 2
    names = list((vocab or {}).get('pred_idx_to_name', PREDICATES))
    names += ['p%d' % i for i in range(len(names), P)]
    ratio = lambda a, n: a / n if n else float('nan')
    seen, agree = sum(r[0] for r in rows[1:P]), sum(r[1] for r in rows[1:P])
    return {'rel_acc': ratio(agree, seen), 'rel_acc_by_pred': {names[p]: (rows[p][1], rows[p][0]) for p in range(1, P)},
            'size_acc': ratio(rows[P][1], rows[P][0]), 'loc_acc': ratio(rows[P + 1][1], rows[P + 1][0])}


# ---- layouts of a drawing front end ----------------------------------------------------------------------------------------------
def layout_json_to_scene_graphs(text_or_dict):
    """scripts/gui/model.py:111-180: {'image_id', 'objects': [{'text', 'left', 'top', 'width', 'height', 'size', 'location',
    'feature'}, ...]} (a JSON string or the dictionary; a list of them gives one graph each) -> the list of scene-graph dictionaries
    of ``Model.encode_scene_graphs``.  Every object is related to the next one in the list.  As in the reference, inside /
    surrounding is decided on boxes of half-width (size + 1) / 20 around each object's centre, clipped to the image, while the
    angle is the one between the centres of the declared boxes."""
    scene = json.loads(text_or_dict) if isinstance(text_or_dict, str) else text_or_dict
    if isinstance(scene, (list, tuple)):
        return [g for one in scene for g in layout_json_to_scene_graphs(one)]
    if len(scene) == 0:
        return []
    objs = scene['objects']
    mean, margin_box = [], []
    for ob in objs:
        x0, y0 = ob['left'], ob['top']
        x1, y1 = ob['width'] + x0, ob['height'] + y0
        mx, my = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
        m = (ob['size'] + 1) / 10 / 2
        mean.append((mx, my))
        margin_box.append((max(0, mx - m), max(0, my - m), min(1, mx + m), min(1, my + m)))
    relationships = []
    for i in range(len(objs) - 1):
        sx0, sy0, sx1, sy1 = margin_box[i]
        ox0, oy0, ox1, oy1 = margin_box[i + 1]
        theta = math.atan2(mean[i][1] - mean[i + 1][1], mean[i][0] - mean[i + 1][0])
        if sx0 < ox0 and sx1 > ox1 and sy0 < oy0 and sy1 > oy1:
            p = 'surrounding'
        elif sx0 > ox0 and sx1 < ox1 and sy0 > oy0 and sy1 < oy1:
            p = 'inside'
        elif theta >= 3 * math.pi / 4 or theta <= -3 * math.pi / 4:
            p = 'left of'
        elif -3 * math.pi / 4 <= theta < -math.pi / 4:
            p = 'above'
        elif -math.pi / 4 <= theta < math.pi / 4:
            p = 'right of'
        else:
            p = 'below'
        relationships.append([i, p, i + 1])
    return [{'objects': [ob['text'] for ob in objs], 'relationships': relationships,
             'attributes': {'size': [ob['size'] for ob in objs], 'location': [ob['location'] for ob in objs]},
             'features': [ob['feature'] for ob in objs], 'image_id': scene['image_id']}]
