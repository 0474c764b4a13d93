"""Shared by tests/test_scenegraph_cpu.py, tests/test_gpu_scenegraph.py and tools/make_golden_scenegraph.py: a numpy float64 / pure
Python restatement of what csrc/scenegraph.hip computes (data/coco.py:323-416 of the reference), written the way the reference
writes it -- ``math.atan2`` thresholds, Python's ``round`` on doubles, loops over objects.  test_scenegraph_cpu.py pins it to the
outputs the reference itself produced (tests/golden/scenegraph_coco.npz, scenegraph_gui.json)."""
import json
import math

import numpy as np

PRED_NAMES = ['__in_image__', 'left of', 'right of', 'above', 'below', 'inside', 'surrounding']      # coco.py:18,206
F32 = np.float32


def mask_set(masks):
    """which elements count as set: an integer mask == 1 (coco.py:332), a float mask > 0.5"""
    masks = np.asarray(masks)
    return masks > F32(0.5) if masks.dtype.kind == 'f' else masks == 1


def centers_ref(boxes, masks):
    """-> (centers float64 [O, 2], not yet rounded to fp32; count int64 [O]).  The mean of linspace(x0, x1, M) over the set
    elements is x0 + (x1 - x0) * Sx / (count * (M - 1)) with Sx the sum of the set elements' column indices."""
    boxes = np.asarray(boxes, dtype=F32)
    sel = mask_set(masks)
    O, M = sel.shape[0], sel.shape[1]
    out, count = np.zeros((O, 2), np.float64), np.zeros(O, np.int64)
    for i in range(O):
        x0, y0, x1, y1 = boxes[i]
        rows, cols = np.nonzero(sel[i])
        c = count[i] = rows.size
        if c == 0:                                    # coco.py:335-337, in fp32 like the tensors there
            out[i] = float(F32(0.5) * (x0 + x1)), float(F32(0.5) * (y0 + y1))
        elif M == 1:
            out[i] = float(x0), float(y0)
        else:
            den = float(c) * float(M - 1)
            out[i, 0] = float(x0) + (float(x1) - float(x0)) * float(int(cols.sum())) / den
            out[i, 1] = float(y0) + (float(y1) - float(y0)) * float(int(rows.sum())) / den
    return out, count


def _clamp(v, hi):
    return min(max(int(v), 0), hi)


def size_arg(box, S=10):
    """the argument of round() of the size index: the box differences are taken in fp32 first"""
    box = np.asarray(box, dtype=F32)
    return float(S - 1) * float(box[2] - box[0]) * float(box[3] - box[1])


def loc_args(center, g=5):
    c = np.asarray(center, dtype=F32)
    return float(c[0]) * float(g - 1), float(c[1]) * float(g - 1)


def attributes_ref(boxes, centers, S=10, g=5):
    """-> (size_idx, loc_idx int64 [O], one-hot float32 [O, S + g * g]) from fp32 boxes and fp32 centres (coco.py:296,347)"""
    boxes, centers = np.asarray(boxes, dtype=F32), np.asarray(centers, dtype=F32)
    O = boxes.shape[0]
    si, li, hot = np.zeros(O, np.int64), np.zeros(O, np.int64), np.zeros((O, S + g * g), F32)
    for i in range(O):
        si[i] = _clamp(round(size_arg(boxes[i], S)), S - 1)
        ax, ay = loc_args(centers[i], g)
        li[i] = _clamp(round(ax), g - 1) + g * _clamp(round(ay), g - 1)
        hot[i, si[i]] = 1
        hot[i, S + li[i]] = 1
    return si, li, hot


def _nesting(bs, bo):
    sx0, sy0, sx1, sy1 = [F32(v) for v in bs]
    ox0, oy0, ox1, oy1 = [F32(v) for v in bo]
    if sx0 < ox0 and sx1 > ox1 and sy0 < oy0 and sy1 > oy1:
        return 6
    if sx0 > ox0 and sx1 < ox1 and sy0 > oy0 and sy1 < oy1:
        return 5
    return 0


def angle_class_atan2(dx, dy):
    """coco.py:372,378-385 on an fp32 difference"""
    theta = math.atan2(float(dy), float(dx))
    if theta >= 3 * math.pi / 4 or theta <= -3 * math.pi / 4:
        return 1
    if -3 * math.pi / 4 <= theta < -math.pi / 4:
        return 3
    if -math.pi / 4 <= theta < math.pi / 4:
        return 2
    return 4


def angle_class_cmp(dx, dy):
    """the comparison form the kernels use"""
    dx, dy = F32(dx), F32(dy)
    ax, ay = abs(dx), abs(dy)
    if dx < 0 and ay <= ax:
        return 1
    if dy < 0 and ay > ax:
        return 3
    if dy > 0 and ay >= ax:
        return 4
    return 2


def predicate_ref(boxes, centers, s, o, angle=angle_class_atan2):
    """coco.py:368-385 for one (subject, object) pair; fp32 boxes and centres, the difference taken in fp32 (coco.py:371)"""
    boxes, centers = np.asarray(boxes, dtype=F32), np.asarray(centers, dtype=F32)
    nest = _nesting(boxes[s], boxes[o])
    if nest:
        return nest
    d = centers[s] - centers[o]
    return angle(d[0], d[1])


def predicates_ref(boxes, centers, s, o, angle=angle_class_atan2):
    return np.array([predicate_ref(boxes, centers, int(a), int(b), angle) for a, b in zip(s, o)], np.int64)


def tie_table():
    """(dx, dy) fp32 pairs on and next to every threshold of the angle classes: the four diagonals, the four axes, zero, and the
    one-ulp neighbours of each diagonal at several magnitudes"""
    out = [(0.0, 0.0)]
    for m in (1.0, 0.25, 0.3, 1e-3, 3.0e-39, 7.5):
        m = F32(m)
        up, dn = np.nextafter(m, F32(np.inf)), np.nextafter(m, F32(0))
        for sx in (1, -1):
            for sy in (1, -1):
                for a, b in ((m, m), (m, up), (m, dn), (up, m), (dn, m)):
                    out.append((sx * a, sy * b))
        out += [(m, 0.0), (-m, 0.0), (0.0, m), (0.0, -m)]
    return [(F32(a), F32(b)) for a, b in out]


def triple_counts(seg_sizes, r):
    """triples per image for images of ``seg_sizes`` objects (the trailing __image__ included)"""
    return [(k - 1) + ((k - 1) * r if k - 1 >= 2 else 0) for k in seg_sizes]


def draw_pairs_ref(seg_sizes, u, boxes, centers, angle=angle_class_atan2):
    """coco.py:358-413 and the collate of coco.py:501-547 with the partner draw driven by u [O, r, 2]: real object i of an image
    with k real objects draws j = min(int(u0 * (k - 1)), k - 2), j += (j >= i) and is the subject when u1 > 0.5"""
    u = np.asarray(u, dtype=F32)
    r = u.shape[1]
    triples, t2i, base = [], [], 0
    for n, size in enumerate(seg_sizes):
        k = size - 1
        if k >= 2:
            for i in range(k):
                for q in range(r):
                    j = min(int(float(u[base + i, q, 0]) * (k - 1)), k - 2)
                    j += 1 if j >= i else 0
                    s, o = (i, j) if u[base + i, q, 1] > F32(0.5) else (j, i)
                    triples.append([base + s, predicate_ref(boxes, centers, base + s, base + o, angle), base + o])
                    t2i.append(n)
        for i in range(k):
            triples.append([base + i, 0, base + k])
            t2i.append(n)
        base += size
    return np.array(triples, np.int64).reshape(-1, 3), np.array(t2i, np.int64)


def triple_agreement_ref(triples, boxes, centers, P):
    counts = np.zeros((P, 2), np.int64)
    for s, p, o in np.asarray(triples).tolist():
        if 1 <= p < P:
            counts[p, 0] += 1
            counts[p, 1] += int(predicate_ref(boxes, centers, s, o) == p)
    return counts


def attribute_agreement_ref(attrs, size_idx, loc_idx, S=10, g=5):
    attrs = np.asarray(attrs)
    counts = np.zeros((2, 2), np.int64)
    for i in range(attrs.shape[0]):
        for b, (blk, idx) in enumerate(((attrs[i, :S], size_idx[i]), (attrs[i, S:S + g * g], loc_idx[i]))):
            on = np.nonzero(blk > 0.5)[0]
            if on.size == 1:
                counts[b, 0] += 1
                counts[b, 1] += int(on[0] == idx)
    return counts


def margins(boxes, centers, s, o, S=10, g=5):
    """how far the decisions of a set of objects and pairs are from flipping: (smallest distance of a round() argument from a
    half-integer, smallest | |dx| - |dy| | over the pairs decided by the angle, smallest gap of a strict box comparison)"""
    boxes, centers = np.asarray(boxes, dtype=F32), np.asarray(centers, dtype=F32)
    half = lambda v: abs((v % 1.0) - 0.5)
    r = min(min(half(size_arg(b, S)), *[half(a) for a in loc_args(c, g)]) for b, c in zip(boxes, centers))
    ang, box = np.inf, np.inf
    for a, b in zip(s, o):
        box = min(box, float(np.abs(boxes[a].astype(np.float64) - boxes[b].astype(np.float64)).min()))
        if not _nesting(boxes[a], boxes[b]):
            d = (centers[a] - centers[b]).astype(np.float64)
            ang = min(ang, abs(abs(d[0]) - abs(d[1])), abs(d[0]) if abs(d[1]) <= abs(d[0]) else abs(d[1]))
    return r, ang, box


def gui_scene_graphs_ref(text_or_dict):
    """scripts/gui/model.py:111-180: the inside / surrounding test on margin boxes built from ``size``, the angle between the
    declared boxes' centres, every object related to the next one"""
    scene = json.loads(text_or_dict) if isinstance(text_or_dict, str) else text_or_dict
    if len(scene) == 0:
        return []
    objs = scene['objects']

    def geometry(ob):
        x0, y0 = ob['left'], ob['top']
        x1, y1 = ob['width'] + x0, ob['height'] + y0
        mx, my = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
        m = (ob['size'] + 1) / 10 / 2
        return (mx, my), (max(0, mx - m), max(0, my - m), min(1, mx + m), min(1, my + m))

    rel = []
    for i in range(len(objs) - 1):
        (sx, sy), (sx0, sy0, sx1, sy1) = geometry(objs[i])
        (ox, oy), (ox0, oy0, ox1, oy1) = geometry(objs[i + 1])
        if sx0 < ox0 and sx1 > ox1 and sy0 < oy0 and sy1 > oy1:
            p = 6
        elif sx0 > ox0 and sx1 < ox1 and sy0 > oy0 and sy1 < oy1:
            p = 5
        else:
            theta = math.atan2(sy - oy, sx - ox)
            if theta >= 3 * math.pi / 4 or theta <= -3 * math.pi / 4:
                p = 1
            elif -3 * math.pi / 4 <= theta < -math.pi / 4:
                p = 3
            elif -math.pi / 4 <= theta < math.pi / 4:
                p = 2
            else:
                p = 4
        rel.append([i, PRED_NAMES[p], i + 1])
    return [{'objects': [ob['text'] for ob in objs], 'relationships': rel,
             'attributes': {'size': [ob['size'] for ob in objs], 'location': [ob['location'] for ob in objs]},
             'features': [ob['feature'] for ob in objs], 'image_id': scene['image_id']}]
