"""The host side of the sampling path (scene_generation_amd/sample.py, Model.encode_scene_graphs) against the reference's recorded
outputs (tests/golden/sample_*.npz, tools/make_golden_sampling.py), and the test helpers' restatements pinned to the same fixtures.
Runs without a GPU."""
import json

import pytest
import torch

import sampling_helpers as SH
from scene_generation_amd import sample
from scene_generation_amd.model import Model


def T(a):
    return torch.from_numpy(a)


@pytest.fixture(scope='module')
def model():
    return SH.small_model(Model)


def test_encode_scene_graphs_matches_reference(golden, model):
    g = golden('sample_encode')
    assert int(g['bank_seed']) == SH.BANK_SEED
    sgs = SH.scene_graphs()
    objs, triples, o2i, attributes, features = model.encode_scene_graphs(sgs)
    for got, key in ((objs, 'objs'), (triples, 'triples'), (o2i, 'obj_to_img'), (attributes, 'attributes')):
        want = T(g[key])
        assert got.dtype == want.dtype and torch.equal(got, want), key
    assert attributes.shape[1] == 35 and attributes[3, 9] == 1 and attributes[3, 22] == 1          # the __image__ row of graph 1
    assert isinstance(features, list) and len(features) == objs.numel()
    assert torch.equal(torch.stack(features), T(g['features'])) and features[0].dtype == torch.float32
    # the caller's dicts are appended to, exactly as recorded
    assert sgs == json.loads(str(g['mutated']))
    assert sgs[0]['objects'][-1] == '__image__' and sgs[0]['features'][-1] == 17
    assert sgs[1]['relationships'][-1] == [1, '__in_image__', 2]


def test_encode_scene_graphs_cumulative_zip_and_fix(model):
    """graph 2 (classes 2, 9, 0) is served from the banks of the classes at the START of the list (3, 5, 7) by default"""
    many, one = model.features, model.features_one
    _, _, _, _, feats = model.encode_scene_graphs(SH.scene_graphs())
    f32 = lambda a: torch.from_numpy(a).to(torch.float32)          # noqa: E731
    assert torch.equal(feats[0], f32(many[3][5])) and torch.equal(feats[1], f32(one[5][0]))
    assert torch.equal(feats[2], f32(many[7][99]))                  # 140 is clamped to row 99
    assert torch.equal(feats[3], f32(many[0][17]))                  # the image's own row: image_id
    assert torch.equal(feats[4], f32(one[3][0])) and torch.equal(feats[5], f32(many[5][99]))        # classes 3, 5: not 2, 9
    assert torch.equal(feats[6], f32(many[7][99]))                  # image_id 250 -> row 99 of class 7, not of class 0
    _, _, _, _, fixed = model.encode_scene_graphs(SH.scene_graphs(), fix_feature_classes=True)
    assert all(torch.equal(a, b) for a, b in zip(fixed[:4], feats[:4]))
    assert torch.equal(fixed[4], f32(one[2][0])) and torch.equal(fixed[5], f32(many[9][99])) and torch.equal(fixed[6], f32(many[0][99]))


def test_encode_scene_graphs_single_dict_and_errors(model):
    sg = SH.scene_graphs()[0]
    objs, triples, o2i, attributes, _ = model.encode_scene_graphs(sg)
    assert objs.tolist() == [3, 5, 7, 0] and o2i.tolist() == [0, 0, 0, 0] and triples.shape == (5, 3)
    bad = SH.scene_graphs()[0]
    bad['objects'][1] = 'unicorn'
    with pytest.raises(ValueError, match='unicorn'):
        model.encode_scene_graphs(bad)
    bad = SH.scene_graphs()[0]
    bad['relationships'][0][1] = 'orbiting'
    with pytest.raises(ValueError, match='orbiting'):
        model.encode_scene_graphs(bad)
    # the attributes the issue adds exist and default to the parent's behaviour
    fresh = Model(model.vocab, image_size=(32, 32), gconv_hidden_dim=64, gconv_num_layers=3, mask_size=8, n_downsample_global=2,
                  appearance_normalization='batch', activation='leakyrelu-0.2')
    assert fresh.features is None and fresh.features_one is None and fresh.factored_test_layout is False
    assert model.encode_scene_graphs(SH.scene_graphs()[0])[4] != []
    fresh_feats = fresh.encode_scene_graphs(SH.scene_graphs()[0])[4]
    assert fresh_feats == []                                        # no banks: an empty list, as in the reference


def test_iou_bookkeeping_matches_reference(golden):
    g = golden('sample_iou')
    pred, gt, o2i = SH.iou_inputs()
    tot = sample.iou_totals(pred, gt, o2i)
    s = sample.iou_summary(tot)
    assert s['total_boxes'] == int(g['total_boxes']) == 7            # 12 objects, 5 images: each loses its last object
    assert int(tot[1]) == int(g['bigger_05']) and int(tot[2]) == int(g['bigger_03'])
    want = float(g['iou_sum'])
    assert abs(float(tot[0]) - want) <= 1e-6 * abs(want)
    assert abs(s['avg_iou'] - want / 7) <= 1e-6 * want
    # a batch of one object keeps nothing
    one = sample.iou_totals(pred[:1], gt[:1], o2i[:1])
    assert one.tolist() == [0.0, 0.0, 0.0, 0.0]


def test_deprocess_restatement_is_the_reference(golden):
    g = golden('sample_deprocess')
    for tag, x in SH.deprocess_inputs().items():
        for key, rescale in (('_rescale', True), ('_plain', False)):
            got, want = SH.deprocess_ref(x, rescale), T(g[tag + key])
            assert got.shape == want.shape
            assert torch.equal(torch.isnan(got), torch.isnan(want))
            assert torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), tag + key
    a = T(g['a_rescale'])
    assert bool(torch.isnan(a[2]).all()) and float(a[0].min()) == 0.0 and float(a[0].max()) == 255.0
    u = SH.to_uint8_ref(a)
    assert u.shape == (4, 16, 20, 3) and u.dtype == torch.uint8 and int(u[2].max()) == 0 and int(u[0].max()) == 255


def test_layout_rgb_restatement_is_the_reference(golden):
    g = golden('sample_layout_rgb')
    vecs, boxes, masks, o2i, objs, colors, num_objs, H = SH.layout_rgb_inputs()
    got, want = SH.layout_rgb_ref(T(g['layout']), colors, num_objs), T(g['rgb'])
    assert got.shape == want.shape == (2, 3, H, H)
    assert float((got - want).abs().max()) <= 1e-4 and abs(float(want.max()) - 255.0) <= 1e-4


def test_cli_arguments():
    p = sample.make_parser()
    a = p.parse_args(['--checkpoint', 'c.pt'])
    assert (a.weights, a.output_dir, a.batch_size, a.image_size, a.scene_graphs) == ('model', 'output', 24, None, None)
    assert not (a.use_gt_boxes or a.use_gt_masks or a.use_gt_textures or a.use_gt_attr or a.save_layout or a.save_gt_imgs)
    assert a.factored is True and p.parse_args(['--checkpoint', 'c.pt', '--factored', '0']).factored is False
    a = p.parse_args(['--checkpoint', 'c.pt', '--weights', 'ema_best', '--use_gt_boxes', '1', '--use_gt_masks', '1',
                      '--save_layout', '1', '--batch_size', '4', '--image_size', '64,64', '--scene_graphs', 'g.json',
                      '--output_dir', 'o'])
    assert a.weights == 'ema_best' and a.use_gt_boxes and a.use_gt_masks and a.save_layout and a.batch_size == 4
    assert tuple(a.image_size) == (64, 64) and a.scene_graphs == 'g.json' and a.output_dir == 'o'
    with pytest.raises(SystemExit):
        p.parse_args(['--checkpoint', 'c.pt', '--weights', 'latest'])
    with pytest.raises(SystemExit):
        p.parse_args([])                                            # --checkpoint is required


def test_weights_selection():
    ck = {'model_state': {'w': 1}, 'model_best_state': {'w': 2}}
    assert sample.select_weights(ck, 'model') == {'w': 1} and sample.select_weights(ck, 'best') == {'w': 2}
    for which in ('ema', 'ema_best'):
        with pytest.raises(ValueError, match='no model_ema'):
            sample.select_weights(ck, which)
    ck.update(model_ema_state={'w': 3}, model_ema_best_state={'w': 4})
    assert sample.select_weights(ck, 'ema') == {'w': 3} and sample.select_weights(ck, 'ema_best') == {'w': 4}
    with pytest.raises(ValueError):
        sample.select_weights(ck, 'latest')
    with pytest.raises(ValueError, match='model_best_state'):
        sample.select_weights({'model_state': {}}, 'best')


def test_scene_graph_file_defaults(tmp_path):
    path = tmp_path / 'g.json'
    path.write_text(json.dumps({'objects': ['obj1', 'obj2'], 'relationships': [[0, 'left of', 1]]}))
    sgs = sample.load_scene_graphs(str(path))
    assert sgs == [{'objects': ['obj1', 'obj2'], 'relationships': [[0, 'left of', 1]], 'features': [-1, -1], 'image_id': -1,
                    'attributes': {'size': [], 'location': []}}]


def test_sample_module_is_part_of_the_overlay_and_shadows_nothing():
    import scene_generation_amd as pkg
    assert 'sample' in pkg._SUBMODULES and 'data' not in pkg._SUBMODULES
    import os
    assert not os.path.exists(os.path.join(os.path.dirname(pkg.__file__), 'data'))
