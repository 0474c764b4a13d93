"""Scene graphs from layouts, the parts that need no GPU: the float64 restatement of tests/scenegraph_ref.py against what the reference
itself returned (tests/golden/scenegraph_coco.npz: CocoSceneGraphDataset.__getitem__ + coco_collate_fn; scenegraph_gui.json:
json_to_scene_graph), the comparison form of the angle classes against the atan2 form, the host-side pieces of
scene_generation_amd.scenegraph and the new command-line flags."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import scenegraph_ref as R
from scene_generation_amd import sample, scenegraph

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def coco():
    return dict(np.load(os.path.join(GOLDEN, 'scenegraph_coco.npz')))


@pytest.fixture(scope='module')
def gui():
    with open(os.path.join(GOLDEN, 'scenegraph_gui.json')) as f:
        return json.load(f)


def test_golden_covers_the_cases(coco):
    sizes = np.bincount(coco['obj_to_img'])
    assert sizes.size == 24 and sizes.min() == 2 and 3 in sizes and sizes.max() >= 8          # k = 1, k = 2, many real objects
    assert coco['masks'].shape[1:] == (16, 16) and coco['masks'].dtype == np.uint8
    assert sorted(set(coco['triples'][:, 1].tolist())) == list(range(7))
    empty = coco['masks'].reshape(len(coco['masks']), -1).sum(1) == 0
    assert empty.any(), 'an empty mask (coco.py:335-337) must be in the golden'


def test_restatement_reproduces_reference_attributes(coco):
    centers, count = R.centers_ref(coco['boxes'], coco['masks'])
    assert np.array_equal(count, coco['masks'].reshape(len(count), -1).sum(1))
    si, li, hot = R.attributes_ref(coco['boxes'], centers.astype(np.float32))
    assert np.array_equal(hot, coco['attributes'])
    last = np.flatnonzero(np.diff(coco['obj_to_img'], append=10 ** 6))                       # every image's __image__ row
    assert (si[last] == 9).all() and (li[last] == 12).all()


@pytest.mark.parametrize('angle', [R.angle_class_atan2, R.angle_class_cmp])
def test_restatement_reproduces_reference_triples(coco, angle):
    """given the (s, o) columns the reference drew, the predicate column; and the collate order around them"""
    centers = R.centers_ref(coco['boxes'], coco['masks'])[0].astype(np.float32)
    tri = coco['triples']
    assert np.array_equal(np.where(tri[:, 1] > 0, R.predicates_ref(coco['boxes'], centers, tri[:, 0], tri[:, 2], angle), 0), tri[:, 1])
    sizes = np.bincount(coco['obj_to_img']).tolist()
    assert np.bincount(coco['triple_to_img']).tolist() == R.triple_counts(sizes, 1)
    base = t = 0
    for n, size in enumerate(sizes):
        k = size - 1
        nsp = k if k >= 2 else 0
        rows = tri[t:t + nsp + k]
        assert (coco['triple_to_img'][t:t + nsp + k] == n).all()
        assert (rows[:nsp, 1] > 0).all() and ((rows[:nsp, [0, 2]] >= base) & (rows[:nsp, [0, 2]] < base + k)).all()
        for i in range(nsp):                               # real object i is one end of its triple, its partner is another object
            assert (base + i) in rows[i, [0, 2]] and rows[i, 0] != rows[i, 2]
        assert rows[nsp:].tolist() == [[base + i, 0, base + k] for i in range(k)]
        base, t = base + size, t + nsp + k
    assert t == len(tri)


def test_comparison_form_equals_atan2_form():
    table = R.tie_table()
    assert len(table) > 100
    for dx, dy in table:
        assert R.angle_class_cmp(dx, dy) == R.angle_class_atan2(dx, dy), (dx, dy)
    one = np.float32(1)
    assert [R.angle_class_cmp(a * one, b * one) for a, b in ((1, 1), (-1, 1), (-1, -1), (1, -1))] == [4, 1, 1, 2]
    assert [R.angle_class_cmp(a * one, b * one) for a, b in ((1, 0), (-1, 0), (0, 1), (0, -1), (0, 0))] == [2, 1, 4, 3, 2]
    rs = np.random.RandomState(5)
    d = (rs.rand(4000, 2).astype(np.float32) - np.float32(0.5)) * np.float32(2)
    d[::7, 1] = d[::7, 0]                                  # exact diagonals and anti-diagonals among random differences
    d[3::7, 1] = -d[3::7, 0]
    for dx, dy in d:
        assert R.angle_class_cmp(dx, dy) == R.angle_class_atan2(dx, dy), (dx, dy)


def test_draw_pairs_restatement_structure():
    """the driven partner draw: never the object itself, every partner reachable, subject chosen by the second uniform"""
    sizes = [4, 2, 3, 6]
    O = sum(sizes)
    rs = np.random.RandomState(2)
    boxes = rs.rand(O, 4).astype(np.float32)
    centers = rs.rand(O, 2).astype(np.float32)
    for r in (1, 2):
        u = scenegraph.draw_uniforms(7, O, r)
        assert u.shape == (O, r, 2) and u.dtype == np.float32 and u.max() < 1
        tri, t2i = R.draw_pairs_ref(sizes, u, boxes, centers)
        assert np.bincount(t2i).tolist() == R.triple_counts(sizes, r) == [3 + 3 * r, 1, 2 + 2 * r, 5 + 5 * r]
        seg = [0] + np.cumsum(sizes).tolist()
        assert scenegraph.triple_offsets(seg, r) == [0] + np.cumsum(R.triple_counts(sizes, r)).tolist()
        assert (tri[:, 0] != tri[:, 2]).all()
    # u0 sweeps the partners in order, skipping the object itself; u1 > 0.5 makes the object the subject
    u = np.zeros((4, 1, 2), np.float32)
    u[0] = [0.0, 0.9]
    u[1] = [0.0, 0.1]
    u[2] = [0.99, 0.9]
    tri, _ = R.draw_pairs_ref([4], u, boxes[:4], centers[:4])
    assert tri[:3, [0, 2]].tolist() == [[0, 1], [0, 1], [2, 1]]


def test_layout_json_to_scene_graphs_equals_reference(gui):
    assert len(gui['layouts']) == 5
    used = set()
    for layout, want in zip(gui['layouts'], gui['scene_graphs']):
        assert scenegraph.layout_json_to_scene_graphs(copy.deepcopy(layout)) == want
        assert scenegraph.layout_json_to_scene_graphs(json.dumps(layout)) == want
        assert R.gui_scene_graphs_ref(layout) == want
        used |= {r[1] for sg in want for r in sg['relationships']}
    assert used == set(scenegraph.PREDICATES[1:])
    both = scenegraph.layout_json_to_scene_graphs(gui['layouts'][:2])
    assert both == gui['scene_graphs'][0] + gui['scene_graphs'][1]
    assert scenegraph.layout_json_to_scene_graphs('{}') == []
    assert scenegraph.PREDICATES == R.PRED_NAMES


def test_load_layouts_feeds_the_scene_graph_path(gui, tmp_path):
    path = str(tmp_path / 'layouts.json')
    with open(path, 'w') as f:
        json.dump(gui['layouts'], f)
    sgs = sample.load_layouts(path)
    assert sgs == [g for gs in gui['scene_graphs'] for g in gs]


def test_summary_reads_the_counters():
    counts = torch.zeros(9, 2, dtype=torch.int64)
    counts[1] = torch.tensor([4, 3])
    counts[6] = torch.tensor([2, 2])
    counts[7] = torch.tensor([10, 5])
    got = scenegraph.summary(counts, {'pred_idx_to_name': R.PRED_NAMES})
    assert got['rel_acc'] == 5 / 6 and got['size_acc'] == 0.5 and np.isnan(got['loc_acc'])
    assert got['rel_acc_by_pred']['left of'] == (3, 4) and got['rel_acc_by_pred']['surrounding'] == (2, 2)
    assert list(got['rel_acc_by_pred']) == R.PRED_NAMES[1:]


def test_no_cpu_fallback():
    boxes, masks = torch.rand(3, 4), torch.ones(3, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        scenegraph.object_centers(boxes, masks)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        scenegraph.predicates(boxes, torch.rand(3, 2), torch.zeros(2, dtype=torch.int64), torch.ones(2, dtype=torch.int64))
    with pytest.raises(ValueError, match='at least its __image__'):
        scenegraph.triple_offsets([0, 0, 3])


def test_parser_accepts_the_new_flags():
    p = sample.make_parser()
    a = p.parse_args(['--checkpoint', 'c.pt'])
    assert a.layouts is None and a.consistent_graphs is False and a.graph_metrics is False
    a = p.parse_args(['--checkpoint', 'c.pt', '--layouts', 'l.json', '--consistent_graphs', '1', '--graph_metrics', '1'])
    assert a.layouts == 'l.json' and a.consistent_graphs is True and a.graph_metrics is True
