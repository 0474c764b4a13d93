"""Scene graphs from layouts on the GPU (csrc/scenegraph.hip through scene_generation_amd.scenegraph): the mask centroids against the
float64 restatement of tests/scenegraph_ref.py with a derived bound, every decision (size / location index, predicate) EXACTLY
against the restatement applied to the device's own fp32 centres, the goldens captured from the reference, graph_from_layout
against the driven partner draw, the agreement counters against host counts, and the sampler's opt-in graph metrics.  The tree
only: no reference checkout."""
import json
import os

import numpy as np
import pytest
import torch

import sampling_helpers as SH
import scenegraph_ref as R
from scene_generation_amd import ops, sample, scenegraph
from scene_generation_amd.model import Model
from scene_generation_amd.pipeline import validate_collated
from scene_generation_amd.synthetic import batch_to, make_batch, make_sampling_vocab

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SIZES = [2, 3, 9, 6, 8, 12]                 # objects per image, the trailing __image__ included: k = 1, k = 2, ... ; O = 40
SG_KINDS = ('scenegraph_centers', 'scenegraph_derive', 'scenegraph_agree')


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _boxes(rs, sizes=SIZES):
    """fp32 boxes of a batch of images of ``sizes`` objects: random, every third real object nested in its predecessor, the last
    of an image [0, 0, 1, 1]"""
    out = []
    for size in sizes:
        for i in range(size - 1):
            if i % 3 == 2:
                px0, py0, px1, py1 = out[-1]
                w, h = (px1 - px0) * rs.uniform(0.4, 0.8), (py1 - py0) * rs.uniform(0.4, 0.8)
                x0, y0 = px0 + (px1 - px0 - w) * rs.uniform(0.2, 0.8), py0 + (py1 - py0 - h) * rs.uniform(0.2, 0.8)
            else:
                w, h = rs.uniform(0.15, 0.6), rs.uniform(0.15, 0.6)
                x0, y0 = (1 - w) * rs.rand(), (1 - h) * rs.rand()
            out.append([x0, y0, x0 + w, y0 + h])
        out.append([0., 0., 1., 1.])
    return np.array(out, np.float32)


def _masks(rs, M, kind, sizes=SIZES):
    """[O, M, M] int64 0 / 1 (with stray 2s, which are not set) or fp32 in [0, 1] (with exact 0.5s, which are not set): random, then
    an empty mask, a full one and one pixel in each corner; every image's last mask all ones"""
    O = sum(sizes)
    if kind == 'i64':
        m = (rs.rand(O, M, M) < 0.6).astype(np.int64)
        m[rs.rand(O, M, M) < 0.05] = 2
    else:
        m = rs.rand(O, M, M).astype(np.float32)
        m[rs.rand(O, M, M) < 0.05] = 0.5
    one = 1 if kind == 'i64' else 0.75
    m[3] = 0
    m[4] = one
    for o, (r, c) in zip((5, 6, 8, 9), ((0, 0), (0, M - 1), (M - 1, 0), (M - 1, M - 1))):
        m[o] = 0
        m[o, r, c] = one
    for last in np.cumsum(sizes) - 1:
        m[last] = one
    return m


@pytest.fixture(scope='module')
def layout16():
    """the N = 6, O = 40 layout most tests share: boxes, int64 masks (M = 16), obj_to_img, device centres"""
    rs = np.random.RandomState(11)
    boxes, masks = _boxes(rs), _masks(rs, 16, 'i64')
    o2i = np.repeat(np.arange(len(SIZES)), SIZES)
    objs = rs.randint(1, 12, size=len(o2i))
    objs[np.cumsum(SIZES) - 1] = 0
    centers = scenegraph.object_centers(T(boxes), T(masks))
    return dict(boxes=boxes, masks=masks, o2i=o2i, objs=objs, centers=N(centers))


# ---- centres ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['i64', 'f32'])
@pytest.mark.parametrize('M', [1, 5, 16, 32, 64])
def test_object_centers(M, kind):
    """both launch plans (a wave per object up to M = 16, a workgroup per object above), 16-byte and element loads (M = 5: masks that
    start off a 16-byte boundary), several loads per thread (M = 64).  Bound: the fp64 value is rounded to fp32 once, and it lies
    inside the box, so the error is at most half an ulp of max(|x0|, |x1|) <= 2^-24 max(|x0|, |x1|); a factor two covers the
    order of evaluation in fp64."""
    rs = np.random.RandomState(100 + M)
    boxes, masks = _boxes(rs), _masks(rs, M, kind)
    want, want_count = R.centers_ref(boxes, masks)
    tb, tm = T(boxes), T(masks)
    got, count = scenegraph.object_centers(tb, tm, return_count=True)
    again, count2 = scenegraph.object_centers(tb, tm, return_count=True)
    assert got.dtype == torch.float32 and got.shape == (40, 2) and count.dtype == torch.int32
    assert torch.equal(got, again) and torch.equal(count, count2)
    assert np.array_equal(N(count), want_count)
    assert want_count[3] == 0 and want_count[4] == M * M and (want_count[[5, 6, 8, 9]] == 1).all()
    bound = 2.0 ** -23 * np.stack([np.abs(boxes[:, [0, 2]]).max(1), np.abs(boxes[:, [1, 3]]).max(1)], 1).astype(np.float64)
    err = np.abs(N(got).astype(np.float64) - want)
    print('M=%d %s: max err / bound = %.3f' % (M, kind, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), float((err - bound).max())
    # the corners of the box are hit exactly; the empty mask gives the fp32 box centre
    if M > 1:
        assert np.array_equal(N(got)[5], boxes[5, [0, 1]]) and np.array_equal(N(got)[9], boxes[9, [2, 3]])
    else:
        assert np.array_equal(N(got)[4], boxes[4, [0, 1]])
    assert np.array_equal(N(got)[3], np.float32(0.5) * (boxes[3, [0, 1]] + boxes[3, [2, 3]]))


@pytest.mark.parametrize('kind', ['i64', 'f32'])
@pytest.mark.parametrize('M', [16, 32])
def test_object_centers_unaligned_base(M, kind):
    """a mask tensor that starts one element off a 16-byte boundary takes the element loads and gives the same bits"""
    rs = np.random.RandomState(7)
    boxes, masks = _boxes(rs), _masks(rs, M, kind)
    tm = T(masks)
    flat = torch.empty(tm.numel() + 1, dtype=tm.dtype, device=DEV)
    shifted = flat[1:].view_as(tm)
    shifted.copy_(tm)
    assert tm.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    a = scenegraph.object_centers(T(boxes), tm, return_count=True)
    b = scenegraph.object_centers(T(boxes), shifted, return_count=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_object_centers_rejects_bad_input():
    boxes = torch.rand(3, 4, device=DEV)
    with pytest.raises(TypeError):
        scenegraph.object_centers(boxes, torch.ones(3, 4, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        scenegraph.object_centers(boxes, torch.ones(2, 4, 4, device=DEV))
    with pytest.raises(RuntimeError, match='M <= 256'):
        scenegraph.object_centers(boxes[:1], torch.ones(1, 257, 257, device=DEV))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        scenegraph.object_centers(boxes.cpu(), torch.ones(3, 4, 4))


# ---- decisions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,g', [(10, 5), (4, 3)])
def test_attribute_indices_equal_restatement(layout16, S, g):
    boxes, centers = layout16['boxes'], layout16['centers']
    si, li, hot = R.attributes_ref(boxes, centers, S, g)
    block, size_idx, loc_idx = scenegraph.attributes_from_layout(T(boxes), T(layout16['masks']), S, g)
    assert np.array_equal(N(size_idx), si) and np.array_equal(N(loc_idx), li)
    assert block.shape == (40, S + g * g) and np.array_equal(N(block), hot)
    if (S, g) == (10, 5):                                   # the __image__ rows need no special case
        last = np.cumsum(SIZES) - 1
        assert (si[last] == 9).all() and (li[last] == 12).all()
    block2, _, _ = scenegraph.attributes_from_layout(T(boxes), None, S, g, centers=T(centers))
    assert torch.equal(block, block2)


def test_attribute_rounding_is_half_to_even_and_clamped():
    """arguments that are exactly representable halves; products above S - 1 and centres outside [0, 1] are clamped"""
    boxes = np.array([[0, 0, 0.5, 0.25], [0, 0, 0.75, 0.5], [0, 0, 0.625, 1.0], [0, 0, 2, 2], [0.5, 0.5, 0.25, 1]], np.float32)
    centers = np.array([[0.125, 0.375], [0.625, 0.875], [0.5, 0.5], [1.5, -0.25], [0.124, 0.376]], np.float32)
    size_idx, loc_idx, _ = ops.sg_object_attributes(T(boxes), T(centers), 5, 5)
    si, li, _ = R.attributes_ref(boxes, centers, 5, 5)
    assert si.tolist() == [0, 2, 2, 4, 0] and li.tolist() == [0 + 5 * 2, 2 + 5 * 4, 2 + 5 * 2, 4 + 5 * 0, 0 + 5 * 2]
    assert N(size_idx).tolist() == si.tolist() and N(loc_idx).tolist() == li.tolist()


def test_predicates_equal_restatement(layout16):
    boxes, centers = layout16['boxes'], layout16['centers']
    rs = np.random.RandomState(3)
    s, o = rs.randint(0, 40, 400), rs.randint(0, 40, 400)
    nested = [(i, i - 1) for i in range(1, 40) if R._nesting(boxes[i], boxes[i - 1])]
    assert len(nested) >= 5
    s[:len(nested)], o[:len(nested)] = np.array(nested).T
    s[len(nested):2 * len(nested)], o[len(nested):2 * len(nested)] = np.array(nested).T[::-1]
    want = R.predicates_ref(boxes, centers, s, o)
    got = N(scenegraph.predicates(T(boxes), T(centers), T(s), T(o)))
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert set(want.tolist()) == {1, 2, 3, 4, 5, 6}
    bad = N(scenegraph.predicates(T(boxes), T(centers), T(np.array([0, 40, -1])), T(np.array([1, 1, 1]))))
    assert bad.tolist()[1:] == [-1, -1] and bad[0] == R.predicate_ref(boxes, centers, 0, 1)      # an id outside the batch: -1


def test_predicate_tie_table():
    """the table of tests/test_scenegraph_cpu.py through sg_pair_predicates: the subject's centre IS (dx, dy), the object's the
    origin, so the fp32 difference is exact; equal boxes, which are neither inside nor surrounding"""
    table = R.tie_table()
    n = len(table)
    centers = np.zeros((n + 1, 2), np.float32)
    centers[:n] = np.array(table, np.float32)
    boxes = np.tile(np.array([[0.2, 0.2, 0.8, 0.8]], np.float32), (n + 1, 1))
    s, o = np.arange(n), np.full(n, n)
    got = N(scenegraph.predicates(T(boxes), T(centers), T(s), T(o)))
    want = np.array([R.angle_class_atan2(dx, dy) for dx, dy in table])
    assert np.array_equal(got, want)
    assert got[0] == 2, 'dx = dy = 0 is right of'


def test_predicate_nesting_is_strict():
    boxes = np.array([[0.1, 0.1, 0.9, 0.9],      # 0 surrounds 1
                      [0.2, 0.2, 0.8, 0.8],
                      [0.1, 0.2, 0.8, 0.8],      # shares x0 with 0: not inside it
                      [0.2, 0.2, 0.8, 0.9],      # shares y1 with 0
                      [0.2, 0.2, 0.8, 0.8]], np.float32)     # equals 1
    centers = np.array([[0.5, 0.5], [0.5, 0.5], [0.3, 0.45], [0.6, 0.7], [0.5, 0.5]], np.float32)
    s = np.array([0, 1, 2, 0, 3, 0, 1, 4])
    o = np.array([1, 0, 0, 2, 0, 3, 4, 1])
    got = N(scenegraph.predicates(T(boxes), T(centers), T(s), T(o))).tolist()
    assert got == R.predicates_ref(boxes, centers, s, o).tolist()
    assert got[:2] == [6, 5] and got[2:] == [1, 2, 4, 3, 2, 2]


# ---- against the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('as_float', [False, True])
def test_reference_golden(as_float):
    g = dict(np.load(os.path.join(GOLDEN, 'scenegraph_coco.npz')))
    boxes = T(g['boxes'])
    masks = T(g['masks'], torch.float32 if as_float else torch.int64)
    centers = scenegraph.object_centers(boxes, masks)
    attributes, _, _ = scenegraph.attributes_from_layout(boxes, masks, centers=centers)
    assert np.array_equal(N(attributes), g['attributes'])
    tri = g['triples']
    spatial = tri[:, 1] > 0
    p = N(scenegraph.predicates(boxes, centers, T(tri[:, 0]), T(tri[:, 2])))
    assert np.array_equal(p[spatial], tri[spatial, 1])
    counts = N(scenegraph.triple_agreement(T(tri), boxes, centers=centers))
    assert np.array_equal(counts[1:7, 0], np.bincount(tri[:, 1], minlength=7)[1:]) and np.array_equal(counts[1:7, 0], counts[1:7, 1])
    counts = N(scenegraph.attribute_agreement(T(g['attributes']), boxes, centers=centers))
    assert counts[7:].tolist() == [[len(g['objs'])] * 2] * 2


# ---- graph_from_layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 2])
def test_graph_from_layout(layout16, r):
    L = layout16
    boxes, masks, o2i, objs = T(L['boxes']), T(L['masks']), T(L['o2i']), T(L['objs'])
    u = scenegraph.draw_uniforms(5, 40, r)
    want_tri, want_t2i = R.draw_pairs_ref(SIZES, u, L['boxes'], L['centers'])
    tri, t2i, attrs = scenegraph.graph_from_layout(objs, boxes, masks, o2i, pairs_per_obj=r, u=u, obj_to_img_host=L['o2i'].tolist(),
                                                   objs_host=L['objs'].tolist())
    assert tri.dtype == torch.int64 and t2i.dtype == torch.int64
    assert np.array_equal(N(tri), want_tri) and np.array_equal(N(t2i), want_t2i)
    assert np.array_equal(N(attrs), R.attributes_ref(L['boxes'], L['centers'])[2])
    # k = 1: only the __in_image__ triple; k = 2: two spatial triples per draw between the two objects
    assert N(tri)[N(t2i) == 0].tolist() == [[0, 0, 1]]
    two = N(tri)[N(t2i) == 1]
    assert len(two) == 2 * r + 2 and all(sorted((a, b)) == [2, 3] for a, _, b in two[:2 * r].tolist())
    imgs = torch.zeros(len(SIZES), 3, 4, 4, device=DEV)
    assert validate_collated((imgs, objs, boxes, masks, tri, o2i, t2i, attrs)) == L['o2i'].tolist()
    # seed -> the same table; no host list -> the documented read, the same graph
    tri2, t2i2, attrs2 = scenegraph.graph_from_layout(objs, boxes, masks, o2i, pairs_per_obj=r, seed=5)
    assert torch.equal(tri, tri2) and torch.equal(t2i, t2i2) and torch.equal(attrs, attrs2)
    tri3, _, _ = scenegraph.graph_from_layout(objs, boxes, masks, o2i, pairs_per_obj=r, seed=6)
    assert not torch.equal(tri, tri3)
    # an image's graph does not depend on its position in the batch: image 3 alone, with its rows of u
    a, b = sum(SIZES[:3]), sum(SIZES[:4])
    alone, t2i_a, attrs_a = scenegraph.graph_from_layout(objs[a:b], boxes[a:b].contiguous(), masks[a:b].contiguous(), o2i[a:b] - 3,
                                                         pairs_per_obj=r, u=u[a:b], obj_to_img_host=[0] * (b - a))
    among = N(tri)[N(t2i) == 3]
    among[:, [0, 2]] -= a
    assert np.array_equal(N(alone), among) and not N(t2i_a).any() and torch.equal(attrs_a, attrs[a:b])


def test_graph_from_layout_checks_the_image_object(layout16):
    L = layout16
    objs_h = L['objs'].tolist()
    objs_h[sum(SIZES[:2]) - 1] = 4
    with pytest.raises(ValueError, match='image 1 does not end with the __image__ object'):
        scenegraph.graph_from_layout(T(L['objs']), T(L['boxes']), T(L['masks']), T(L['o2i']), obj_to_img_host=L['o2i'].tolist(),
                                     objs_host=objs_h)
    with pytest.raises(ValueError, match='u must be'):
        scenegraph.graph_from_layout(T(L['objs']), T(L['boxes']), T(L['masks']), T(L['o2i']), u=np.zeros((40, 2, 2), np.float32))


# ---- agreement --------------------------------------------------------------------------------------------------------------------
def _synthetic(seed=3, N_=6):
    return make_batch(N=N_, min_objs=1, max_objs=8, size=32, mask_size=8, num_objs=12, num_preds=7, seed=seed)


def test_regraph_and_triple_agreement():
    b = _synthetic()
    for dev_batch in (False, True):
        rb = scenegraph.regraph(batch_to(b, DEV) if dev_batch else b, seed=2)
        assert rb.triples.is_cuda == dev_batch and rb.attributes.is_cuda == dev_batch
        assert rb.boxes is not None and torch.equal(rb.boxes.cpu(), b.boxes) and torch.equal(rb.masks.cpu(), b.masks)
        if not dev_batch:
            host = rb
    assert torch.equal(host.triples, rb.triples.cpu()) and torch.equal(host.attributes, rb.attributes.cpu())
    validate_collated(host)
    boxes, masks, tri = T(N(host.boxes)), T(N(host.masks)), T(N(host.triples))
    centers = scenegraph.object_centers(boxes, masks)
    counts = N(scenegraph.triple_agreement(tri, boxes, masks))
    assert counts.shape == (9, 2)
    seen = np.bincount(N(host.triples)[:, 1], minlength=7)
    assert counts[0].tolist() == [0, 0] and np.array_equal(counts[1:7, 0], seen[1:]) and np.array_equal(counts[1:7, 1], seen[1:])
    assert np.array_equal(counts[:7], R.triple_agreement_ref(N(host.triples), N(host.boxes), N(centers), 7))
    assert scenegraph.summary(T(counts))['rel_acc'] == 1.0
    # the counters accumulate
    twice = scenegraph.triple_agreement(tri, boxes, centers=centers, counts=T(counts))
    assert np.array_equal(N(twice), 2 * counts)
    # move the subject of a 'left of' triple to the far side of its partner: that triple, and whatever else hangs on the box, flips
    tl = N(host.triples)
    t = int(np.flatnonzero(tl[:, 1] == 1)[0])
    s, o = tl[t, 0], tl[t, 2]
    moved_boxes, moved_centers = N(host.boxes).copy(), N(centers).copy()
    shift = np.float32(2 * (moved_centers[o, 0] - moved_centers[s, 0]))
    moved_boxes[s, [0, 2]] += shift
    moved_centers[s, 0] += shift
    want = R.triple_agreement_ref(tl, moved_boxes, moved_centers, 7)
    got = N(scenegraph.triple_agreement(tri, T(moved_boxes), centers=T(moved_centers)))
    assert np.array_equal(got[:7], want) and np.array_equal(got[:7, 0], counts[:7, 0])
    assert got[1, 1] < counts[1, 1] and R.predicate_ref(moved_boxes, moved_centers, s, o) != 1


def test_attribute_agreement(layout16):
    L = layout16
    si, li, hot = R.attributes_ref(L['boxes'], L['centers'])
    given = hot.copy()
    given[0] = 0                                            # nothing specified: ignored
    given[1, :10] = 0                                       # only the location specified
    given[2, 10:] = 0
    given[5, (si[5] + 1) % 10] = 1                          # two size bits: not a one-hot block
    given[6, :10] = np.roll(given[6, :10], 1)               # a wrong size
    given[7, 10:] = np.roll(given[7, 10:], 3)               # a wrong location
    given[8] = np.float32(0.4) * given[8]                   # below the threshold: no bits
    want = R.attribute_agreement_ref(given, si, li)
    assert want.tolist() == [[40 - 4, 40 - 5], [40 - 3, 40 - 4]]
    counts = scenegraph.attribute_agreement(T(given), T(L['boxes']), T(L['masks']))
    assert N(counts)[:7].sum() == 0 and np.array_equal(N(counts)[7:], want)
    s = scenegraph.summary(counts)
    assert s['size_acc'] == 35 / 36 and s['loc_acc'] == 36 / 37 and np.isnan(s['rel_acc'])


# ---- sampler ----------------------------------------------------------------------------------------------------------------------
def _model():
    m = SH.small_model(Model, make_sampling_vocab(SH.C, 7, SH.A)).to(DEV)
    m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    return m


def _sample_batch():
    b = make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=SH.C, num_preds=7, num_attributes=35, seed=321)
    return scenegraph.regraph(b, seed=1)


def _library_summary(out, triples, attributes, vocab):
    counts = scenegraph.new_counts(7, DEV)
    scenegraph.triple_agreement(triples.to(DEV), out.boxes_pred, out.masks_pred, counts=counts)
    scenegraph.attribute_agreement(attributes.to(DEV), out.boxes_pred, out.masks_pred, counts=counts)
    return scenegraph.summary(counts, vocab)


def test_sampler_graph_metrics():
    m, b = _model(), _sample_batch()
    outs = {}
    for on in (False, True):
        s = sample.Sampler(m, colors=torch.arange(36.).view(12, 3), graph_metrics=on)
        o = s.sample_batch(b, use_gt_textures=True, want_layout_rgb=True)
        outs[on] = (s, o)
    off, on = outs[False][1], outs[True][1]
    for name in ('images', 'boxes_pred', 'masks_pred', 'layout_rgb'):
        assert torch.equal(getattr(off, name), getattr(on, name)), name
    assert outs[False][0].graph_summary() is None
    got = outs[True][0].graph_summary()
    want = _library_summary(on, b.triples, b.attributes, m.vocab)      # the batch's attributes, not the zeroed copy the model saw
    assert got == want and set(got) == {'rel_acc', 'rel_acc_by_pred', 'size_acc', 'loc_acc'}
    seen = np.bincount(N(b.triples)[:, 1], minlength=7)
    assert [got['rel_acc_by_pred'][n][1] for n in R.PRED_NAMES[1:]] == seen[1:].tolist()
    assert 0.0 <= got['rel_acc'] <= 1.0 and 0.0 <= got['size_acc'] <= 1.0
    # a second batch accumulates
    outs[True][0].sample_batch(b, use_gt_textures=True)
    again = outs[True][0].graph_summary()
    assert [v[1] for v in again['rel_acc_by_pred'].values()] == (2 * seen[1:]).tolist() and again['rel_acc'] == got['rel_acc']
    # scene graphs: the attributes the graph specified
    s = sample.Sampler(m, graph_metrics=True)
    sgs = SH.scene_graphs()
    o = s.sample_json(sgs)
    objs, triples, _, attributes, _ = m.encode_scene_graphs(SH.scene_graphs())
    assert s.graph_summary() == _library_summary(o, triples, attributes, m.vocab)


def test_sampler_graph_metrics_launches_and_host_reads(monkeypatch):
    """off: no scene-graph kernel runs; on: the centroids, the derived indices and the two counters -- and still ONE host read"""
    m, b = _model(), _sample_batch()
    reads = []
    for name in ('tolist', 'item', 'cpu', 'numpy'):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    profs = {}
    for on in (False, True):
        s = sample.Sampler(m, graph_metrics=on)
        s.sample_batch(b, use_gt_textures=True)                          # warm-up outside the profile
        ops.prof_enable(True)
        try:
            ops.prof_reset()
            del reads[:]
            s.sample_batch(b, use_gt_textures=True)
            n_reads = list(reads)
            profs[on] = ops.prof_read()
        finally:
            ops.prof_enable(False)
        assert n_reads == ['tolist'], n_reads
    assert [profs[False][k]['launches'] for k in SG_KINDS] == [0, 0, 0]
    assert [profs[True][k]['launches'] for k in SG_KINDS] == [1, 1, 2]
    for k in profs[False]:
        if k not in SG_KINDS:
            assert profs[True][k]['launches'] == profs[False][k]['launches'], k


KW = dict(image_size=(32, 32), gconv_hidden_dim=32, gconv_num_layers=2, mask_size=8, n_downsample_global=1,
          appearance_normalization='batch', activation='leakyrelu-0.2', use_attributes=True, pool_size=2, rep_size=8)


def test_command_line_layouts_and_consistent_graphs(tmp_path, capsys):
    from scene_generation_amd.synthetic import fill_deterministic
    vocab = make_sampling_vocab(12, 7, 35)
    m = Model(vocab, **KW).to(DEV)
    fill_deterministic(m)
    m.eval()
    ckpt = str(tmp_path / 'ckpt.pt')
    torch.save({'model_kwargs': dict(vocab=vocab, **KW), 'model_state': m.state_dict()}, ckpt)
    rs = np.random.RandomState(0)
    bank = {c: rs.rand(8, 8) for c in range(12)}
    np.save(str(tmp_path / 'bank.npy'), bank, allow_pickle=True)
    with open(os.path.join(GOLDEN, 'scenegraph_gui.json')) as f:
        layouts = json.load(f)['layouts']
    names = {}
    for layout in layouts:                                   # the front end's class names -> the test vocabulary's
        for ob in layout['objects']:
            ob['text'] = names.setdefault(ob['text'], 'obj%d' % (1 + len(names) % 11))
            ob['feature'] = min(ob['feature'], 2)
    lpath = str(tmp_path / 'layouts.json')
    with open(lpath, 'w') as f:
        json.dump(layouts, f)
    res = sample.main(['--checkpoint', ckpt, '--output_dir', str(tmp_path / 'a'), '--layouts', lpath, '--features',
                       str(tmp_path / 'bank.npy'), '--batch_size', '3', '--graph_metrics', '1'])
    assert len(res['paths']) == 5 and all(os.path.isfile(p) for p in res['paths'])
    nrel = sum(len(layout['objects']) - 1 for layout in layouts)
    assert sum(v[1] for v in res['graph']['rel_acc_by_pred'].values()) == nrel
    assert 'rel_acc' in capsys.readouterr().out
    res = sample.main(['--checkpoint', ckpt, '--output_dir', str(tmp_path / 'b'), '--num_samples', '6', '--batch_size', '3',
                       '--use_gt_textures', '1', '--consistent_graphs', '1', '--graph_metrics', '1'])
    assert len(res['paths']) == 6
    g = res['graph']
    batches = list(sample.synthetic_loader(m, 3, 6, 8))
    objects = sum(b.objs.numel() for b in batches)
    assert sum(v[1] for v in g['rel_acc_by_pred'].values()) == objects - 6      # one spatial triple per real object (3 or more an image)
    assert all(0 <= a <= n for a, n in g['rel_acc_by_pred'].values())
    assert 0.0 <= g['rel_acc'] <= 1.0 and 0.0 <= g['size_acc'] <= 1.0 and 0.0 <= g['loc_acc'] <= 1.0
    out = capsys.readouterr().out
    assert 'rel_acc %s' % g['rel_acc'] in out and 'size_acc %s' % g['size_acc'] in out and 'left of: ' in out
    res = sample.main(['--checkpoint', ckpt, '--output_dir', str(tmp_path / 'c'), '--num_samples', '3', '--batch_size', '3',
                       '--use_gt_textures', '1'])
    assert 'graph' not in res and 'rel_acc' not in capsys.readouterr().out
