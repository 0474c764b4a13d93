"""The sampling path on the GPU: the factored test-mode compositing against the dense kernel (bit for bit) and the reference's
goldens, sg_deprocess_images and sg_layout_rgb against the reference's recorded outputs and the restatements of
tests/sampling_helpers.py, Model.forward_json / the factored test-mode forward against the goldens, and the Sampler (determinism,
EMA weights from a checkpoint, files written, which layout kernel ran).  Fixtures and the tree only: no reference checkout."""
import json
import os
import random

import numpy as np
import pytest
import torch

import sampling_helpers as SH
from scene_generation_amd import ops, sample
from scene_generation_amd.model import Model
from scene_generation_amd.synthetic import batch_to, fill_deterministic, make_batch, make_vocab
from gpu_harness import _dump, close
from tools_det import det

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = {}


def T(a):
    return torch.from_numpy(a)


def _planes_of(o2i):
    counts, plane = {}, []
    for i in o2i.tolist():
        plane.append(counts.get(i, 0))
        counts[i] = plane[-1] + 1
    return torch.tensor(plane, dtype=torch.int64), max(counts.values()), max(counts) + 1


def _planes_vs_dense(vecs, boxes, masks, o2i, H, W, avg):
    """-> (dense kernel output, reconstruction from the planes kernel), after the structural checks"""
    pidx, J, N = _planes_of(o2i)
    vecs, boxes, masks, o2i, pidx = [t.to(DEV) for t in (vecs, boxes, masks, o2i, pidx)]
    seg = ops.segment_offsets(o2i, N)
    with torch.no_grad():
        dense = ops.masks_to_layout_test(vecs, boxes, masks, seg, N, H, W, avg)
        Z, winner, value = ops.masks_to_layout_test_planes(vecs, boxes, masks, seg, pidx, N, J, H, W, avg)
        Z2, winner2, none = ops.masks_to_layout_test_planes(vecs, boxes, masks, seg, pidx, N, J, H, W, avg, want_value=False)
    torch.cuda.synchronize()
    assert Z.shape == (N, J, H, W) and winner.shape == (N, H, W) and winner.dtype == torch.int32 and none is None
    assert torch.equal(Z, Z2) and torch.equal(winner, winner2)
    won = winner >= 0
    w = winner.long().clamp(min=0)
    assert bool((o2i[w] == torch.arange(N, device=DEV).view(N, 1, 1))[won].all())        # a winner belongs to its image
    assert int((Z != 0).sum(1).max()) <= 1                                               # at most one non-zero plane per pixel
    assert bool((value[~won] == 0).all()) and bool((value[won] > 0).all())
    pick = torch.gather(Z, 1, pidx[w].unsqueeze(1)).squeeze(1)
    assert torch.equal(torch.where(won, pick, torch.zeros_like(pick)), value) and torch.equal(Z.sum(1), value)
    recon = (vecs[w] * value.unsqueeze(-1)) * won.unsqueeze(-1)                          # vecs[winner] * value through winner
    recon = recon.permute(0, 3, 1, 2).contiguous()
    assert torch.equal(recon, dense)
    return dense, recon


@pytest.mark.parametrize('case', ['demo_16', 'demo_64', 'i64_m32', 'f32_m16', 'f32_m8_avg', 'many'])
def test_planes_vs_dense_goldens(golden, case):
    g = golden('layout_test_' + case)
    dense, recon = _planes_vs_dense(T(g['vecs']), T(g['boxes']), T(g['masks']), T(g['obj_to_img']), int(g['H']), int(g['W']),
                                    bool(int(g['avg'])))
    close(recon, g['out'], 1e-5, 'factored test-mode layout')


SYNTH = {'32': dict(N=3, max_objs=4, size=32, mask_size=8, seed=321), '64': dict(N=4, max_objs=8, size=64, mask_size=16, seed=7),
         '128': dict(N=8, max_objs=8, size=128, mask_size=32, seed=11)}


@pytest.mark.parametrize('size', ['32', '64', '128'])
def test_planes_vs_dense_synthetic(size):
    """ground-truth boxes and masks of the synthetic generator: the visiting order matters (>= 10 % of the pixels are claimed by two
    or more objects), int64 and fp32 masks, 'avg' on and off, and a width that is not a multiple of 4"""
    b = make_batch(min_objs=2, num_objs=12, num_preds=4, num_attributes=35, **SYNTH[size])
    H = SYNTH[size]['size']
    O_ = b.objs.numel()
    vecs = det((O_, 12 + 8), 83) + 0.55
    pidx, J, N = _planes_of(b.obj_to_img)
    for W in (H, H - 2):
        seg = ops.segment_offsets(b.obj_to_img.to(DEV), N)
        S = ops.layout_planes(b.boxes.to(DEV), b.masks.to(DEV), seg, pidx.to(DEV), N, J, H, W)       # sampled mask per object
        contested = float(((S > 0.5).sum(1) >= 2).float().mean())
        print('size %s W %d: %.1f %% of the pixels claimed by two or more objects' % (size, W, 100 * contested))
        assert contested >= 0.10
        soft = torch.rand(b.masks.shape, generator=torch.Generator().manual_seed(6))      # every sampled value is rounded
        for masks in (b.masks, b.masks.float(), soft):
            for avg in (False, True):
                _planes_vs_dense(vecs, b.boxes, masks, b.obj_to_img, H, W, avg)


def _eq_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


def _check_deprocess(x, want_by_rescale=None):
    xd = x.to(DEV)
    for rescale in (True, False):
        f, u = ops.deprocess_images(xd, rescale=rescale, uint8=True, float32=True)
        u_only = ops.deprocess_images(xd, rescale=rescale)
        f_only = ops.deprocess_images(xd, rescale=rescale, uint8=False, float32=True)
        torch.cuda.synchronize()
        f, u = f.cpu(), u.cpu()
        N, C, H, W = x.shape
        assert f.shape == (N, C, H, W) and u.shape == (N, H, W, C) and u.dtype == torch.uint8
        assert _eq_nan(f, SH.deprocess_ref(x, rescale))
        if want_by_rescale is not None:
            assert _eq_nan(f, want_by_rescale[rescale])
        assert torch.equal(u, SH.to_uint8_ref(f)) and torch.equal(u_only.cpu(), u) and _eq_nan(f_only.cpu(), f)
    return f, u


def test_deprocess_fixture(golden):
    g = golden('sample_deprocess')
    for tag, x in SH.deprocess_inputs().items():
        _check_deprocess(x, {True: T(g[tag + '_rescale']), False: T(g[tag + '_plain'])})
    x = SH.deprocess_inputs()['a']
    f, u = ops.deprocess_images(x.to(DEV), rescale=True, uint8=True, float32=True)
    assert bool(torch.isnan(f[2]).all()) and int(u[2].max()) == 0            # the constant image: NaN / 0
    host = sample.imagenet_deprocess_batch(x.to(DEV))
    assert not host.is_cuda and _eq_nan(host, T(g['a_rescale']))


@pytest.mark.parametrize('shape', [(1, 3, 128, 128), (3, 3, 128, 128), (32, 3, 128, 128), (3, 3, 30, 50), (2, 1, 30, 50),
                                   (2, 5, 16, 20)])
def test_deprocess_random(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g) * 0.8
    x[0, 0, 0, :3] = torch.tensor([-3.0, 3.0, 0.0])[:min(3, shape[3])]       # values the clamp without rescale has to cut
    _check_deprocess(x)


def test_layout_rgb(golden):
    g = golden('sample_layout_rgb')
    vecs, boxes, masks, o2i, objs, colors, num_objs, H = SH.layout_rgb_inputs()
    pidx, J, N = _planes_of(o2i)
    dv = [t.to(DEV) for t in (vecs, boxes, masks, o2i, pidx, objs, colors)]
    seg = ops.segment_offsets(dv[3], N)
    with torch.no_grad():
        dense = ops.masks_to_layout_test(dv[0], dv[1], dv[2], seg, N, H, H, False)
        Z, winner, value = ops.masks_to_layout_test_planes(dv[0], dv[1], dv[2], seg, dv[4], N, J, H, H, False)
        rgb = ops.layout_rgb(winner, value, dv[5], dv[6]).cpu()
    assert rgb.shape == (N, 3, H, H)
    assert float((rgb - T(g['rgb'])).abs().max()) <= 1e-4
    assert float((rgb - SH.layout_rgb_ref(dense.cpu(), colors, num_objs)).abs().max()) <= 1e-4
    assert abs(float(rgb.max()) - 255.0) <= 1e-4 and float(rgb.min()) == 0.0
    # a width the vector form cannot take (H * W % 4 != 0)
    with torch.no_grad():
        dense = ops.masks_to_layout_test(dv[0], dv[1], dv[2], seg, N, 15, 13, False)
        Z, winner, value = ops.masks_to_layout_test_planes(dv[0], dv[1], dv[2], seg, dv[4], N, J, 15, 13, False)
        rgb = ops.layout_rgb(winner, value, dv[5], dv[6]).cpu()
    assert float((rgb - SH.layout_rgb_ref(dense.cpu(), colors, num_objs)).abs().max()) <= 1e-4


def _dev_stats(a, b):
    a, b = a.detach().float().cpu(), torch.as_tensor(b).float().cpu()
    return {'max_abs': float((a - b).abs().max()), 'max_ref': float(b.abs().max())}


def test_forward_json_golden(golden):
    g = golden('sample_forward_json')
    m = SH.small_model(Model).to(DEV)
    m.noise_override = T(g['noise']).to(DEV)
    for factored in (False, True):
        m.factored_test_layout = factored
        with torch.no_grad():
            out, objs = m.forward_json(SH.scene_graphs())
        assert out[3] is None and out[5] is None and torch.equal(objs.cpu(), T(g['objs']))
        ops.ensure_dense(out[4])
        tag = 'forward_json factored' if factored else 'forward_json dense'
        PARITY[tag] = _dev_stats(out[0], g['imgs_pred'])
        close(out[1], g['boxes_pred'], 2e-5, tag + ' boxes')
        close(out[2], g['masks_pred'], 2e-5, tag + ' masks')
        close(out[4], g['pred_layout'], 2e-5, tag + ' layout')
        close(out[0], g['imgs_pred'], 1e-4, tag + ' imgs')


def test_factored_test_mode_forward_golden(golden):
    from sampling_helpers import inference_model, inference_cases
    g = golden('model_test_mode')
    m, batch = inference_model(Model)
    m = m.to(DEV)
    imgs, objs, boxes, masks, triples, o2i, _, attributes = batch_to(batch, DEV)
    for tag, kw in inference_cases(batch, g):
        kw = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        m.noise_override = T(g[tag + '_noise']).to(DEV)
        outs = {}
        for factored in (False, True):
            m.factored_test_layout = factored
            with torch.no_grad():
                out = m(imgs, objs, triples, o2i, attributes=attributes, test_mode=True, **kw)
            assert out[3] is None and out[5] is None
            if factored:
                assert ops.hint(out[4], 'pending') is not None and ops.hint(out[4], 'factored') is not None
                winner, value = ops.hint(out[4], 'test_planes')
                assert winner.shape == value.shape == (3, 32, 32)
                ops.ensure_dense(out[4])
                assert ops.hint(out[4], 'pending') is None
            outs[factored] = [t.clone() for t in (out[0], out[1], out[2], out[4])]
        on, off = outs[True], outs[False]
        assert torch.equal(on[3], off[3])                         # the same kernel fills the dense layout
        assert torch.equal(on[1], off[1]) and torch.equal(on[2], off[2])
        PARITY['model_test_mode %s dense' % tag] = _dev_stats(off[0], g[tag + '_imgs_pred'])
        PARITY['model_test_mode %s factored' % tag] = _dev_stats(on[0], g[tag + '_imgs_pred'])
        PARITY['model_test_mode %s factored vs dense' % tag] = _dev_stats(on[0], off[0])
        close(on[1], g[tag + '_boxes_pred'], 2e-5, tag + ' boxes')
        close(on[2], g[tag + '_masks_pred'], 2e-5, tag + ' masks')
        close(on[3], g[tag + '_pred_layout'], 2e-5, tag + ' layout')
        close(on[0], g[tag + '_imgs_pred'], 1e-4, tag + ' imgs (factored)')


def test_factored_vs_dense_full_size():
    """128 x 128, N = 8, nine residual blocks: the factored stem against the dense one"""
    from conftest import skip_random_init
    with skip_random_init():
        m = Model(make_vocab(12, 4, 35), image_size=(128, 128), mask_size=32, use_attributes=True, n_blocks_global=9,
                  appearance_normalization='batch', activation='leakyrelu-0.2')
    fill_deterministic(m)
    m = m.eval().to(DEV)
    m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    b = batch_to(make_batch(N=8, min_objs=2, max_objs=8, size=128, mask_size=32, num_objs=12, num_preds=4, num_attributes=35,
                            seed=11), DEV)
    outs = {}
    for factored in (False, True):
        m.factored_test_layout = factored
        with torch.no_grad():
            out = m(b.imgs, b.objs, b.triples, b.obj_to_img, boxes_gt=b.boxes, masks_gt=b.masks, attributes=b.attributes,
                    test_mode=True, use_gt_box=True)
        outs[factored] = (out[0].clone(), ops.ensure_dense(out[4]).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[False][0]).all()) and float(outs[False][0].abs().max()) > 0
    assert torch.equal(outs[True][1], outs[False][1])
    PARITY['128x128 N=8 factored vs dense'] = _dev_stats(outs[True][0], outs[False][0])
    close(outs[True][0], outs[False][0], 1e-4, 'factored vs dense images at 128 x 128')


def test_write_parity_record():
    """the observed deviations of the tests above -> sample_parity.json in the suite's output directory (a record, not a check)"""
    assert PARITY
    _dump('sample_parity.json', PARITY)


# ---- Sampler ------------------------------------------------------------------------------------------------------------------------
def _sampling_model():
    m = SH.small_model(Model).to(DEV)
    m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    return m


def _batch32(seed=321):
    return make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=12, num_preds=4, num_attributes=35, seed=seed)


@pytest.mark.parametrize('factored', [False, True])
def test_sampler_is_reproducible(factored):
    m = _sampling_model()
    bank = SH.make_banks()[0]
    s = sample.Sampler(m, features=bank, colors=torch.arange(36.).view(12, 3), factored=factored)
    outs = []
    for _ in range(2):
        random.seed(5)
        o = s.sample_batch(_batch32(), use_gt_boxes=True, use_gt_masks=True, want_layout_rgb=True, want_layout=True)
        outs.append([t.cpu().clone() for t in (o.images, o.boxes_pred, o.masks_pred, o.layout_rgb, o.layout)])
    a, b = outs
    assert a[0].dtype == torch.uint8 and a[0].shape == (3, 32, 32, 3) and a[3].shape == (3, 3, 32, 32)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a[0].numpy().tobytes() == b[0].numpy().tobytes()
    random.seed(6)                                           # other bank rows: another picture
    o = s.sample_batch(_batch32(), use_gt_boxes=True, use_gt_masks=True)
    assert not torch.equal(o.images.cpu(), a[0]) and o.layout_rgb is None and o.layout is None
    assert m.factored_test_layout is False and m.objs_host is None          # the model is handed back as it was
    summary = s.iou_summary()
    assert summary['total_boxes'] == 3 * (_batch32().objs.numel() - 3)
    with pytest.raises(ValueError, match='No features file'):
        sample.Sampler(m).sample_batch(_batch32())


def test_sampler_label_map_factored_equals_dense():
    m = _sampling_model()
    colors = torch.arange(36.).view(12, 3) + 1
    outs = []
    for factored in (False, True):
        s = sample.Sampler(m, colors=colors, factored=factored)
        o = s.sample_batch(_batch32(), use_gt_boxes=True, use_gt_masks=True, use_gt_textures=True, want_layout_rgb=True,
                           want_layout=True)
        outs.append(o)
    assert torch.equal(outs[0].layout, outs[1].layout)
    assert float((outs[0].layout_rgb - outs[1].layout_rgb).abs().max()) <= 1e-4
    want = SH.layout_rgb_ref(outs[0].layout.cpu(), colors, 12)
    assert float((outs[1].layout_rgb.cpu() - want).abs().max()) <= 1e-4


def test_sample_json():
    m = _sampling_model()
    s = sample.Sampler(m, factored=False)
    sgs = SH.scene_graphs()
    o = s.sample_json(sgs)
    assert o.images.shape == (2, 32, 32, 3) and o.images.dtype == torch.uint8 and o.objs.tolist() == [3, 5, 7, 0, 2, 9, 0]
    assert sgs[0]['objects'][-1] == '__image__'
    with torch.no_grad():
        out, _ = m.forward_json(SH.scene_graphs())
    assert torch.equal(o.images, ops.deprocess_images(out[0]))


@pytest.mark.parametrize('factored', [False, True])
def test_sampler_layout_kernel_launched(factored):
    """with ``factored`` and no layout asked for, the dense layout kernel never runs; without it, the planes kernel never does"""
    m = _sampling_model()
    s = sample.Sampler(m, factored=factored)
    b = _batch32()
    s.sample_batch(b, use_gt_boxes=True, use_gt_masks=True, use_gt_textures=True)          # warm-up outside the profile
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        s.sample_batch(b, use_gt_boxes=True, use_gt_masks=True, use_gt_textures=True)
        prof = ops.prof_read()
    finally:
        ops.prof_enable(False)
    planes, dense = prof['layout_test_planes']['launches'], prof['layout_fwd']['launches']
    assert (planes, dense) == ((1, 0) if factored else (0, 1))
    assert prof['deprocess']['launches'] == 1 and prof['layout_rgb']['launches'] == 0


def test_ema_weights_from_checkpoint_and_files(tmp_path):
    from trainer_helpers import _batch, _run, _trainer
    tr, ck, args = _trainer(tmp_path / 'train', ema_decay=0.5)
    _run(tr, _batch(), range(3))
    path = tr.save_checkpoint(ck, 3, args, 0)
    saved = torch.load(path, map_location='cpu', weights_only=False)
    assert 'model_ema_state' in saved and 'model_ema_best_state' not in saved
    noise = torch.linspace(-1, 1, 64).view(1, -1)
    flags = dict(use_gt_boxes=True, use_gt_masks=True, use_gt_textures=True)
    imgs = {}
    for which in ('model', 'ema'):
        a = sample.make_parser().parse_args(['--checkpoint', path, '--weights', which])
        m = sample.build_model(a, saved, DEV)
        assert not m.training
        m.noise_override = noise
        imgs[which] = sample.Sampler(m).sample_batch(_batch32(), **flags).images
    live = tr.ema_model()
    live.noise_override = noise
    want = sample.Sampler(live).sample_batch(_batch32(), **flags).images
    assert torch.equal(imgs['ema'], want) and not torch.equal(imgs['ema'], imgs['model'])
    with pytest.raises(ValueError, match='model_ema_best_state'):
        sample.build_model(sample.make_parser().parse_args(['--checkpoint', path, '--weights', 'ema_best']), saved, DEV)

    # run_model: one file per image, the bytes of the uint8 array
    out_dir = tmp_path / 'out'
    a = sample.make_parser().parse_args(['--checkpoint', path, '--weights', 'ema', '--output_dir', str(out_dir), '--use_gt_boxes', '1',
                                         '--use_gt_masks', '1', '--use_gt_textures', '1', '--save_layout', '1', '--save_gt_imgs', '1'])
    batches = [_batch32(321), _batch32(322)]
    res = sample.run_model(a, saved, str(out_dir), loader=batches)
    assert len(res['paths']) == 6 and sorted(os.listdir(out_dir / 'images')) == sorted(os.path.basename(p) for p in res['paths'])
    assert len(os.listdir(out_dir / 'layouts')) == 6 and len(os.listdir(out_dir / 'images_gt')) == 6
    assert res['iou']['total_boxes'] == sum(b.objs.numel() - 3 for b in batches)
    Image = pytest.importorskip('PIL.Image')
    m = sample.build_model(a, saved, DEV)
    want = sample.Sampler(m).sample_batch(batches[0], **flags).images.cpu().numpy()
    for i in range(3):
        assert res['paths'][i].endswith('%04d.png' % i)
        assert np.array_equal(np.asarray(Image.open(res['paths'][i])), want[i])
