#!/usr/bin/env python
"""Capture golden vectors from the REFERENCE implementation (build container only).

Imports /root/reference read-only under container-only shims (stub
torchvision / tensorboardX, map .cuda()/.to('cuda') to CPU, fake cuda.is_available() during
construction), fills every module with the closed-form pattern of
scene_generation_amd.synthetic.fill_deterministic, runs op / module / full-step cases at small sizes
and writes inputs + expected outputs to tests/golden/*.npz.  Only DATA is written; no reference
source travels.  Re-run:  python tools/make_golden.py
"""
import os
import random
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import PIL.Image  # noqa: F401  (data/utils.py touches PIL.Image after a bare `import PIL`)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = '/root/reference'
sys.path.insert(0, REF)
OUT = os.path.join(ROOT, 'tests', 'golden')

from scene_generation_amd.synthetic import fill_deterministic, make_batch, make_vocab, _hash_uniform  # noqa: E402

torch.set_num_threads(8)


def install_shims():
    nn.Module.cuda = lambda self, *a, **k: self
    _to = nn.Module.to
    nn.Module.to = lambda self, *a, **k: _to(
        self, *['cpu' if isinstance(x, str) and x.startswith('cuda') else x for x in a], **k)
    torch.cuda.FloatTensor = torch.FloatTensor
    tv = types.ModuleType('torchvision')
    for sub in ('models', 'transforms', 'utils'):
        m = types.ModuleType('torchvision.' + sub)
        setattr(tv, sub, m)
        sys.modules['torchvision.' + sub] = m
    for n in ('Normalize', 'Compose', 'ToTensor'):
        setattr(tv.transforms, n, type(n, (), {'__init__': lambda s, *a, **k: None}))
    sys.modules['torchvision'] = tv
    tbx = types.ModuleType('tensorboardX')
    tbx.SummaryWriter = type('SummaryWriter', (), {'__init__': lambda s, *a, **k: None,
                                                   'add_scalar': lambda s, *a, **k: None,
                                                   'add_image': lambda s, *a, **k: None})
    sys.modules['tensorboardX'] = tbx


class fake_cuda:
    def __enter__(self):
        self.real = torch.cuda.is_available
        torch.cuda.is_available = lambda: True

    def __exit__(self, *a):
        torch.cuda.is_available = self.real


def det(shape, salt, scale=1.0, shift=0.0):
    n = int(np.prod(shape))
    return (_hash_uniform(n, salt).view(*shape) * 2 * scale + shift)


def npz(name, **arrs):
    out = {}
    for k, v in arrs.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-28s %8.1f KB' % (name, os.path.getsize(path) / 1024))


def grads_of(out_scalar, tensors):
    gs = torch.autograd.grad(out_scalar, tensors, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(gs, tensors)]


def probe_weight(shape, salt):
    """deterministic cotangent so that sum(out*w) has a non-trivial gradient"""
    return det(shape, salt, 1.0)


# ------------------------------------------------------------------------------------------
def golden_gconv():
    from scene_generation.graph import GraphTripleConv, GraphTripleConvNet
    cases = {
        'small': dict(Din=8, A=0, H=16, Dout=8, O=9, T=16, pooling='avg'),
        'small_sum': dict(Din=8, A=0, H=16, Dout=8, O=9, T=16, pooling='sum'),
        'full': dict(Din=128, A=35, H=512, Dout=128, O=9, T=16, pooling='avg'),
        'dense': dict(Din=8, A=0, H=16, Dout=8, O=33, T=96, pooling='avg'),
        'one': dict(Din=8, A=0, H=16, Dout=8, O=3, T=1, pooling='avg'),
    }
    for name, c in cases.items():
        g = torch.Generator().manual_seed(11)
        O, T = c['O'], c['T']
        edges = torch.randint(0, O - 1, (T, 2), generator=g)      # node O-1 stays isolated
        if T >= 4:
            edges[1] = edges[0]                                     # duplicate triple
            edges[2, 1] = edges[2, 0]                               # self loop
        m = GraphTripleConv(c['Din'], attributes_dim=c['A'], output_dim=c['Dout'], hidden_dim=c['H'],
                            pooling=c['pooling'])
        fill_deterministic(m)
        obj = det((O, c['Din'] + c['A']), 1).requires_grad_()
        pred = det((T, c['Din']), 2).requires_grad_()
        cap = {}
        h1 = m.net1.register_forward_hook(lambda mod, i, o: cap.__setitem__('new_t', o.detach().clone()))
        h2 = m.net2.register_forward_hook(lambda mod, i, o: cap.__setitem__('pooled', i[0].detach().clone()))
        new_obj, new_pred = m(obj, pred, edges)
        h1.remove()
        h2.remove()
        wo, wp = probe_weight(new_obj.shape, 3), probe_weight(new_pred.shape, 4)
        loss = (new_obj * wo).sum() + (new_pred * wp).sum()
        params = list(m.parameters())
        gs = grads_of(loss, [obj, pred] + params)
        arrs = dict(edges=edges, obj=obj, pred=pred, new_obj=new_obj, new_pred=new_pred, wo=wo, wp=wp,
                    new_t=cap['new_t'], pooled=cap['pooled'], g_obj=gs[0], g_pred=gs[1],
                    cfg=np.array([c['Din'], c['A'], c['H'], c['Dout'], O, T, int(c['pooling'] == 'avg')]))
        for (n, _), gp in zip(m.named_parameters(), gs[2:]):
            if name == 'full' and gp.numel() > 70000:      # keep the fixture small: checksum the big ones
                arrs['gpstat_' + n] = np.array([float(gp.double().sum()), float(gp.double().abs().sum())])
            else:
                arrs['gp_' + n] = gp
        npz('gconv_' + name, **arrs)
    # stacked net
    net = GraphTripleConvNet(8, num_layers=3, hidden_dim=16)
    fill_deterministic(net)
    g = torch.Generator().manual_seed(5)
    edges = torch.randint(0, 9, (16, 2), generator=g)
    obj, pred = det((9, 8), 7), det((16, 8), 8)
    o2, p2 = net(obj, pred, edges)
    npz('gconvnet_small', edges=edges, obj=obj, pred=pred, new_obj=o2, new_pred=p2)


def demo_layout_inputs():
    """the known-input set of the reference's own demo (layout.py:188-254)"""
    vecs = torch.tensor([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32)
    boxes = torch.tensor([[0.25, 0.125, 0.5, 0.875], [0, 0, 1, 0.25], [0.6125, 0, 0.875, 1], [0, 0.8, 1, 1.0],
                          [0.25, 0.125, 0.5, 0.875], [0.6125, 0, 0.875, 1]], dtype=torch.float32)
    o2i = torch.tensor([0, 0, 0, 1, 1, 1])
    d = [[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]]
    r = [[0, 0, 1, 0, 0], [0, 1, 0, 1, 0], [1, 0, 0, 0, 1], [0, 1, 0, 1, 0], [0, 0, 1, 0, 0]]
    masks = torch.tensor([d, r, d, d, d, d], dtype=torch.float32)
    return vecs, boxes, masks, o2i


def golden_layout():
    from scene_generation.layout import masks_to_layout
    vecs, boxes, masks, o2i = demo_layout_inputs()
    for H in (16, 64):
        out = masks_to_layout(vecs, boxes, masks, o2i, H)
        npz('layout_demo_%d' % H, vecs=vecs, boxes=boxes, masks=masks, obj_to_img=o2i, out=out, H=H)
    g = torch.Generator().manual_seed(3)
    for name, M, H, W, dtype, pooling in [('i64_m32', 32, 24, 24, 'i64', 'sum'), ('f32_m16', 16, 20, 28, 'f32', 'sum'),
                                          ('f32_m5_avg', 5, 16, 16, 'f32', 'avg'), ('edge', 8, 16, 16, 'f32', 'sum')]:
        counts = [3, 1, 4]
        O = sum(counts)
        o2i = torch.cat([torch.full((c,), i, dtype=torch.long) for i, c in enumerate(counts)])
        D = 7
        vecs = det((O, D), 21).requires_grad_()
        x0 = torch.rand(O, generator=g) * 0.5
        y0 = torch.rand(O, generator=g) * 0.5
        boxes = torch.stack([x0, y0, x0 + 0.1 + 0.4 * torch.rand(O, generator=g),
                             y0 + 0.1 + 0.4 * torch.rand(O, generator=g)], 1)
        if name == 'edge':   # boxes touching / exceeding the unit square, full-image box
            boxes[0] = torch.tensor([0., 0., 1., 1.])
            boxes[1] = torch.tensor([-0.2, 0.3, 0.4, 1.3])
            boxes[2] = torch.tensor([0.7, 0.7, 1.0, 1.0])
        if dtype == 'i64':
            masks = (torch.rand(O, M, M, generator=g) < 0.6).long()
        else:
            masks = torch.rand(O, M, M, generator=g)
        out = masks_to_layout(vecs, boxes, masks, o2i, H, W, pooling=pooling)
        w = probe_weight(out.shape, 22)
        gv, = grads_of((out * w).sum(), [vecs])
        npz('layout_' + name, vecs=vecs, boxes=boxes, masks=masks, obj_to_img=o2i, out=out, w=w, g_vecs=gv,
            H=H, W=W, avg=int(pooling == 'avg'))


def golden_crop():
    from scene_generation.bilinear import crop_bbox_batch
    g = torch.Generator().manual_seed(9)
    feats = det((3, 4, 20, 24), 31).requires_grad_()
    for name, idx, HH in [('sorted_8', [0, 0, 1, 2, 2, 2], 8), ('perm_8', [1, 0, 1, 2, 0, 2], 8),
                          ('perm_32', [2, 0, 1, 1, 0, 2], 32)]:
        B = len(idx)
        x0 = torch.rand(B, generator=g) * 0.5
        y0 = torch.rand(B, generator=g) * 0.5
        boxes = torch.stack([x0, y0, x0 + 0.1 + 0.4 * torch.rand(B, generator=g),
                             y0 + 0.1 + 0.4 * torch.rand(B, generator=g)], 1)
        boxes[0] = torch.tensor([0., 0., 1., 1.])                      # full box (not identity at align_corners=False)
        boxes[1] = torch.tensor([0.25, 0.25, 0.75, 0.75])              # boxes of the reference's demo (bilinear.py:289-293)
        boxes[2] = torch.tensor([0., 0., 0.5, 0.5])
        idx_t = torch.tensor(idx)
        out = crop_bbox_batch(feats, boxes, idx_t, HH)
        w = probe_weight(out.shape, 32)
        gf, = grads_of((out * w).sum(), [feats])
        npz('crop_' + name, feats=feats, boxes=boxes, idx=idx_t, out=out, w=w, g_feats=gf, HH=HH)
    # the reference's non-'cudnn' batch branch (bilinear.py:42-56: per-image loop into a zero tensor; crop_bbox is called without
    # the backend, i.e. with grid_sample) on the permuted boxes above, rectangular crops
    out = crop_bbox_batch(feats, boxes, idx_t, 8, 12, backend='jj')
    same = crop_bbox_batch(feats, boxes, idx_t, 8, 12, backend='cudnn')
    assert torch.equal(out, same), "reference: backend='jj' of crop_bbox_batch is expected to equal 'cudnn'"
    w = probe_weight(out.shape, 33)
    gf, = grads_of((out * w).sum(), [feats])
    npz('crop_jj_batch', feats=feats, boxes=boxes, idx=idx_t, out=out, w=w, g_feats=gf, HH=8, WW=12)
    # crop_bbox(backend='jj') called directly: the bilinear_sample geometry (bilinear.py:127-128,188-243: pixel coordinate X * W
    # without the half-pixel shift, floor / floor + 1 taps clamped to the plane -- at X * W >= W - 1 both taps coincide and their
    # weights cancel).  One box per image, incl. the full box (whose last row / column hits that edge case)
    from scene_generation.bilinear import crop_bbox
    bj = torch.stack([torch.tensor([0., 0., 1., 1.]), torch.tensor([0.25, 0.25, 0.75, 0.75]), torch.tensor([0.1, 0.3, 0.62, 0.97])], 0)
    for name, HH, WW in (('sq', 8, 8), ('rect', 6, 11)):
        out = crop_bbox(feats, bj, HH, WW, backend='jj')
        w = probe_weight(out.shape, 34)
        gf, = grads_of((out * w).sum(), [feats])
        npz('crop_jj_direct_' + name, feats=feats, boxes=bj, out=out, w=w, g_feats=gf, HH=HH, WW=WW)


def run_module(name, mod, inputs, extra=None, train=True):
    """forward + backward of a reference module with deterministic params; stores everything"""
    fill_deterministic(mod)
    mod.train(train)
    ins = [t.clone().requires_grad_() if t.is_floating_point() else t for t in inputs]
    out = mod(*ins)
    flat = []

    def walk(o):
        if isinstance(o, torch.Tensor):
            flat.append(o)
        elif isinstance(o, (list, tuple)):
            for x in o:
                walk(x)
    walk(out)
    loss = 0
    ws = []
    for i, o in enumerate(flat):
        w = probe_weight(o.shape, 40 + i) if o.dim() > 0 else torch.tensor(1.0)
        ws.append(w)
        loss = loss + (o * w).sum()
    fins = [t for t in ins if t.is_floating_point()]
    params = list(mod.parameters())
    gs = grads_of(loss, fins + params)
    arrs = {}
    for i, t in enumerate(inputs):
        arrs['in%d' % i] = t
    for i, o in enumerate(flat):
        arrs['out%d' % i] = o
        arrs['w%d' % i] = ws[i]
    for i, gi in enumerate(gs[:len(fins)]):
        arrs['gin%d' % i] = gi
    for (n, _), gp in zip(mod.named_parameters(), gs[len(fins):]):
        arrs['gp_' + n] = gp
    for n, b in mod.named_buffers():
        arrs['buf_' + n] = b
    if extra:
        arrs.update(extra)
    npz(name, **arrs)


def golden_modules():
    from scene_generation.generators import mask_net, AppearanceEncoder, GlobalGenerator
    from scene_generation.layers import get_norm_layer, build_mlp
    from scene_generation.discriminators import (MultiscaleDiscriminator, MultiscaleMaskDiscriminator,
                                                 AcCropDiscriminator)
    vocab = make_vocab(12, 4, 0)
    run_module('mod_mlp', build_mlp([10, 16, 6]), [det((5, 10), 50)])
    run_module('mod_mask_net', mask_net(24, 8), [det((5, 24, 1, 1), 51)])
    run_module('mod_encoder', AppearanceEncoder(vocab, arch='C4-8-2,C4-16-2,C4-32-2', normalization='batch',
                                                activation='leakyrelu-0.2', padding='valid', vecs_size=24),
               [det((5, 3, 32, 32), 52)])
    # build_cnn with residual blocks (layers.py:84-118,172-177): BatchNorm inside the block -> the buffers pin the reference's
    # double evaluation of the branch; eval-mode dropout MLP (layers.py:229-230) is the identity
    from scene_generation.layers import build_cnn
    run_module('mod_cnn_residual', build_cnn('I6,R,C3-8-2,R,C3-4', normalization='batch', activation='leakyrelu-0.2',
                                             padding='same')[0], [det((3, 6, 12, 12), 57)])
    run_module('mod_mlp_dropout_eval', build_mlp([10, 16, 6], dropout=0.3), [det((5, 10), 58)], train=False)
    run_module('mod_globalgen', GlobalGenerator(12, 3, ngf=8, n_downsampling=2, n_blocks=2,
                                                norm_layer=get_norm_layer('instance')),
               [det((2, 12, 16, 16), 53)])
    run_module('mod_imgD', MultiscaleDiscriminator(7, ndf=8, n_layers=3, norm_layer=get_norm_layer('instance'),
                                                   use_sigmoid=False, num_D=2), [det((2, 7, 32, 32), 54)])
    cond = torch.zeros(5, 12)
    cond[torch.arange(5), torch.tensor([1, 3, 0, 11, 3])] = 1
    run_module('mod_maskD', MultiscaleMaskDiscriminator(1, ndf=8, n_layers=2, norm_layer=get_norm_layer('instance'),
                                                        use_sigmoid=False, num_D=1, num_objects=12),
               [det((5, 1, 16, 16), 55, 0.5, 0.5), cond])
    objs = torch.tensor([1, 3, 0, 11, 3])
    boxes = torch.tensor([[0.1, 0.1, 0.6, 0.7], [0.3, 0.2, 0.9, 0.9], [0., 0., 1., 1.], [0.5, 0.5, 0.95, 0.8],
                          [0.2, 0.4, 0.5, 0.9]])
    o2i = torch.tensor([0, 0, 0, 1, 1])
    run_module('mod_objD', AcCropDiscriminator(vocab, arch='C4-8-2,C4-16-2,C4-32-2', normalization='batch',
                                               activation='leakyrelu-0.2', object_size=32, padding='valid'),
               [det((2, 3, 40, 40), 56), objs, boxes, o2i])


def golden_losses():
    from scene_generation.losses import GANLoss, gan_g_loss, gan_d_loss
    import torch.nn.functional as F
    crit = GANLoss(use_lsgan=True, tensor=torch.FloatTensor)
    preds = [[det((2, 4, 5, 5), 60), det((2, 1, 6, 6), 61)], [det((2, 4, 3, 3), 62), det((2, 1, 4, 4), 63)]]
    reals = [[det((2, 4, 5, 5), 64), det((2, 1, 6, 6), 65)], [det((2, 4, 3, 3), 66), det((2, 1, 4, 4), 67)]]
    sr, sf = det((7, 1), 68, 3.0), det((7, 1), 69, 3.0)
    logits, tgt = det((6, 12), 70, 2.0), torch.tensor([0, 3, 11, 5, 5, 1])
    # trainer.py:331-340 restated by running the reference Trainer method unbound
    from scene_generation.trainer import Trainer
    holder = types.SimpleNamespace(criterionFeat=torch.nn.L1Loss())
    feat = Trainer.calculate_features_loss(holder, preds, reals)
    npz('losses', p00=preds[0][0], p01=preds[0][1], p10=preds[1][0], p11=preds[1][1],
        r00=reals[0][0], r01=reals[0][1], r10=reals[1][0], r11=reals[1][1],
        gan_true=crit(preds, True), gan_false=crit(preds, False), gan_single=crit(preds[0], True),
        feat=feat, sr=sr, sf=sf, g_loss=gan_g_loss(sf), d_loss=gan_d_loss(sr, sf),
        logits=logits, tgt=tgt, ce=F.cross_entropy(logits, tgt),
        mse=F.mse_loss(preds[0][0], reals[0][0]), l1=F.l1_loss(preds[0][0], reals[0][0]))


def tensor_stats(sd):
    keys = sorted(sd.keys())
    return keys, np.array([[float(sd[k].double().sum()), float(sd[k].double().abs().sum())] for k in keys])


def golden_step():
    """G7: one and two full G+D iterations (train.py:190-215) of the reference Trainer, reduced widths."""
    from scene_generation.args import parser
    from scene_generation.trainer import Trainer
    C, P, A = 12, 4, 35
    vocab = make_vocab(C, P, A)
    argv = ['--image_size', '32,32', '--batch_size', '3', '--vgg_features_weight', '0', '--output_dir', '/tmp/o',
            '--n_downsample_global', '2', '--gconv_hidden_dim', '64', '--gconv_num_layers', '3', '--mask_size', '8',
            '--ndf', '8', '--ndf_mask', '8', '--crop_size', '16', '--d_obj_arch', 'C4-8-2,C4-16-2', '--pool_size', '2']
    args = parser.parse_args(argv)
    with fake_cuda():
        tr = Trainer(args, vocab, {'model_kwargs': {}, 'd_obj_kwargs': {}, 'd_mask_kwargs': {}, 'd_img_kwargs': {}})
    for m in (tr.model, tr.netD, tr.obj_discriminator, tr.mask_discriminator):
        fill_deterministic(m)
    random.seed(1234)
    arrs = {'argv': np.array(argv)}
    for it in range(2):
        batch = make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=C, num_preds=P,
                           num_attributes=A, seed=100 + it)
        imgs, objs, boxes, masks, triples, o2i, _, attributes = batch
        use_gt = (it == 0)
        if not use_gt:
            attributes = torch.zeros_like(attributes)
        torch.manual_seed(777 + it)
        noise = torch.randn((1, args.mask_noise_dim))
        torch.manual_seed(777 + it)
        out = tr.model(imgs, objs, triples, o2i, boxes_gt=boxes, masks_gt=masks, attributes=attributes)
        imgs_pred, boxes_pred, masks_pred, layout, layout_pred, layout_wrong = out
        tr.train_generator(imgs, imgs_pred, masks, masks_pred, layout, objs, boxes, boxes_pred, o2i, use_gt)
        tr.train_mask_discriminator(masks, masks_pred.detach(), objs)
        tr.train_obj_discriminator(imgs, imgs_pred.detach(), objs, boxes, boxes.detach(), o2i)
        tr.train_image_discriminator(imgs, imgs_pred.detach(), layout.detach(), layout_wrong.detach())
        pre = 'it%d_' % it
        arrs[pre + 'noise'] = noise
        for n, t in zip(['imgs_pred', 'boxes_pred', 'masks_pred'], out[:3]):
            arrs[pre + n] = t
        for n, t in zip(['layout', 'layout_pred', 'layout_wrong'], out[3:]):
            arrs[pre + n + '_stats'] = np.array([float(t.double().sum()), float(t.double().abs().sum())])
        arrs[pre + 'layout_wrong_rep'] = layout_wrong[:, C:].detach()
        for lname, L in [('g', tr.generator_losses), ('dmask', tr.d_mask_losses), ('dobj', tr.d_obj_losses),
                         ('dimg', tr.d_img_losses)]:
            for k, v in L.items():
                arrs[pre + 'loss_' + lname + '_' + k] = v
        for mname, m in [('model', tr.model), ('netD', tr.netD), ('objD', tr.obj_discriminator),
                         ('maskD', tr.mask_discriminator)]:
            keys, st = tensor_stats(m.state_dict())
            arrs[pre + 'keys_' + mname] = np.array(keys)
            arrs[pre + 'stats_' + mname] = st
    npz('step_reduced', **arrs)
    # state_dict key inventory at FULL default sizes (drop-in contract)
    args = parser.parse_args(['--vgg_features_weight', '0', '--output_dir', '/tmp/o'])
    with fake_cuda():
        tr = Trainer(args, make_vocab(), {'model_kwargs': {}, 'd_obj_kwargs': {}, 'd_mask_kwargs': {},
                                          'd_img_kwargs': {}})
    inv = {}
    for mname, m in [('model', tr.model), ('netD', tr.netD), ('objD', tr.obj_discriminator),
                     ('maskD', tr.mask_discriminator)]:
        sd = m.state_dict()
        inv['keys_' + mname] = np.array(list(sd.keys()))
        inv['shapes_' + mname] = np.array([','.join(str(int(d)) for d in v.shape) for v in sd.values()])
    npz('state_dict_keys_full', **inv)


def _slices(t, n=64):
    """a few small, fixed slices of a tensor: the first and last n entries and n entries on a stride"""
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // n)
    return torch.cat([f[:n], f[-n:], f[::step][:n]])


def golden_step_full():
    """G7 at FULL default widths ("one full-size run storing only loss dicts + output checksums"): the reference
    Trainer (trainer.py:205-325 driven as train.py:190-215) for two iterations at
      * the BASELINE configs[1] shape: 128x128, <= 8 objects (+ __image__), default widths, N = 8 (= the per-kernel shapes
        of the bench line: Winograd 128-tiles, factored layout convs, 128-wide GEMM tiles), and
      * BASELINE configs[0]: 64x64, 4 objects, N = 4.
    Stored: the 16 named losses, (sum, |sum|) of the three outputs / three layouts and of EVERY post-step parameter and
    buffer, plus a few small slices of the outputs."""
    from scene_generation.args import parser
    from scene_generation.trainer import Trainer
    vocab = make_vocab()
    for tag, size, N, lo, hi in (('c2', 128, 8, 3, 8), ('c1', 64, 4, 4, 4)):
        argv = ['--image_size', '%d,%d' % (size, size), '--batch_size', str(N), '--vgg_features_weight', '0',
                '--output_dir', '/tmp/o']
        args = parser.parse_args(argv)
        with fake_cuda():
            tr = Trainer(args, vocab, {'model_kwargs': {}, 'd_obj_kwargs': {}, 'd_mask_kwargs': {}, 'd_img_kwargs': {}})
        for m in (tr.model, tr.netD, tr.obj_discriminator, tr.mask_discriminator):
            fill_deterministic(m)
        random.seed(4321)
        arrs = {'argv': np.array(argv), 'N': N, 'min_objs': lo, 'max_objs': hi, 'size': size}
        for it in range(2):
            batch = make_batch(N=N, min_objs=lo, max_objs=hi, size=size, seed=200 + it)
            imgs, objs, boxes, masks, triples, o2i, _, attributes = batch
            use_gt = (it == 0)
            if not use_gt:
                attributes = torch.zeros_like(attributes)
            torch.manual_seed(888 + it)
            noise = torch.randn((1, args.mask_noise_dim))
            torch.manual_seed(888 + it)
            out = tr.model(imgs, objs, triples, o2i, boxes_gt=boxes, masks_gt=masks, attributes=attributes)
            imgs_pred, boxes_pred, masks_pred, layout, layout_pred, layout_wrong = out
            tr.train_generator(imgs, imgs_pred, masks, masks_pred, layout, objs, boxes, boxes_pred, o2i, use_gt)
            tr.train_mask_discriminator(masks, masks_pred.detach(), objs)
            tr.train_obj_discriminator(imgs, imgs_pred.detach(), objs, boxes, boxes.detach(), o2i)
            tr.train_image_discriminator(imgs, imgs_pred.detach(), layout.detach(), layout_wrong.detach())
            pre = 'it%d_' % it
            arrs[pre + 'noise'] = noise
            for n, t in zip(['imgs_pred', 'boxes_pred', 'masks_pred', 'layout', 'layout_pred', 'layout_wrong'], out):
                arrs[pre + n + '_stats'] = np.array([float(t.double().sum()), float(t.double().abs().sum())])
                arrs[pre + n + '_slices'] = _slices(t)
            arrs[pre + 'boxes_pred'] = boxes_pred.detach()
            for lname, L in [('g', tr.generator_losses), ('dmask', tr.d_mask_losses), ('dobj', tr.d_obj_losses),
                             ('dimg', tr.d_img_losses)]:
                for k, v in L.items():
                    arrs[pre + 'loss_' + lname + '_' + k] = v
            for mname, m in [('model', tr.model), ('netD', tr.netD), ('objD', tr.obj_discriminator),
                             ('maskD', tr.mask_discriminator)]:
                keys, st = tensor_stats(m.state_dict())
                arrs[pre + 'keys_' + mname] = np.array(keys)
                arrs[pre + 'stats_' + mname] = st
            print(tag, 'iteration', it, 'done', flush=True)
        npz('step_full_' + tag, **arrs)
        del tr


def golden_eval():
    """f4 eval hooks: ``jaccard`` (metrics.py:27-35, the IoU that check_model accumulates, train.py:80-116) on boxes with
    empty / partial / full overlaps, and the feature bank of scripts/encode_features.py:103-146
    (``repr_net(image_encoder(crop_bbox_batch(...)))`` in eval mode) on a reduced model with closed-form weights."""
    from scene_generation.metrics import jaccard
    from scene_generation.bilinear import crop_bbox_batch
    from scene_generation.model import Model
    a = torch.tensor([[0.1, 0.1, 0.5, 0.6], [0.0, 0.0, 1.0, 1.0], [0.2, 0.3, 0.4, 0.9], [0.6, 0.6, 0.9, 0.9],
                      [0.05, 0.5, 0.45, 0.95], [0.3, 0.3, 0.7, 0.7]])
    b = torch.tensor([[0.1, 0.1, 0.5, 0.6], [0.25, 0.25, 0.75, 0.75], [0.5, 0.3, 0.8, 0.9], [0.55, 0.65, 0.95, 0.85],
                      [0.0, 0.45, 0.5, 1.0], [0.31, 0.28, 0.69, 0.74]])
    g = torch.Generator().manual_seed(5)
    ra = torch.rand(40, 2, generator=g) * 0.5
    ra = torch.cat([ra, ra + 0.1 + torch.rand(40, 2, generator=g) * 0.4], 1)
    rb = (ra + (torch.rand(40, 4, generator=g) - 0.5) * 0.3).clamp(0, 1)
    rb = torch.cat([torch.min(rb[:, :2], rb[:, 2:] - 0.02), rb[:, 2:]], 1)
    pa, pb = torch.cat([a, ra]), torch.cat([b, rb])
    tot, n5, n3 = jaccard(pa, pb)
    vocab = make_vocab(12, 4, 35)
    with fake_cuda():
        m = Model(vocab, image_size=(32, 32), gconv_hidden_dim=32, gconv_num_layers=2, mask_size=8, n_downsample_global=1,
                  appearance_normalization='batch', activation='leakyrelu-0.2', use_attributes=True, pool_size=2, rep_size=8)
    fill_deterministic(m)
    m.eval()
    batch = make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=12, num_preds=4, seed=33)
    with torch.no_grad():
        crops = crop_bbox_batch(batch.imgs, batch.boxes, batch.obj_to_img, 64)
        feat = m.repr_net(m.image_encoder(crops))
    npz('eval_hooks', boxes_a=pa, boxes_b=pb, iou_sum=tot, n_gt_05=n5, n_gt_03=n3, feat=feat, objs=batch.objs)


def golden_testmode():
    """masks_to_layout(test_mode=True) (layout.py:87-92,157-169) and Model.forward(test_mode=True,
    features=...) (model.py:111-117,158-163) of the reference, reduced widths."""
    from scene_generation.layout import masks_to_layout
    from scene_generation.model import Model
    vecs, boxes, masks, o2i = demo_layout_inputs()
    for H in (16, 64):
        out = masks_to_layout(vecs, boxes, masks, o2i, H, test_mode=True)
        npz('layout_test_demo_%d' % H, vecs=vecs, boxes=boxes, masks=masks, obj_to_img=o2i, out=out, H=H, W=H, avg=0)
    g = torch.Generator().manual_seed(5)
    for name, M, H, W, dtype, pooling, counts in [('i64_m32', 32, 24, 24, 'i64', 'sum', [3, 1, 4]),
                                                  ('f32_m16', 16, 20, 28, 'f32', 'sum', [5, 2]),
                                                  ('f32_m8_avg', 8, 16, 16, 'f32', 'avg', [2, 6, 1]),
                                                  ('many', 16, 32, 32, 'i64', 'sum', [17, 9])]:
        O = sum(counts)
        o2i = torch.cat([torch.full((c,), i, dtype=torch.long) for i, c in enumerate(counts)])
        D = 7
        vecs = det((O, D), 61) + 0.6          # mostly positive so the masses are well separated
        x0 = torch.rand(O, generator=g) * 0.5
        y0 = torch.rand(O, generator=g) * 0.5
        boxes = torch.stack([x0, y0, x0 + 0.15 + 0.45 * torch.rand(O, generator=g),
                             y0 + 0.15 + 0.45 * torch.rand(O, generator=g)], 1)
        boxes[0] = torch.tensor([0., 0., 1., 1.])          # an __image__-like full box behind everything else
        if dtype == 'i64':
            masks = (torch.rand(O, M, M, generator=g) < 0.7).long()
            masks[0] = 1
        else:
            masks = torch.rand(O, M, M, generator=g)
        out = masks_to_layout(vecs, boxes, masks, o2i, H, W, pooling=pooling, test_mode=True)
        npz('layout_test_' + name, vecs=vecs, boxes=boxes, masks=masks, obj_to_img=o2i, out=out, H=H, W=W,
            avg=int(pooling == 'avg'))
    # inference forward
    C, P, A = 12, 4, 35
    vocab = make_vocab(C, P, A)
    with fake_cuda():
        model = Model(vocab, image_size=(32, 32), gconv_hidden_dim=64, gconv_num_layers=3, mask_size=8,
                      mlp_normalization='none', appearance_normalization='batch', activation='leakyrelu-0.2',
                      n_downsample_global=2, use_attributes=True, pool_size=2)
    fill_deterministic(model)
    with torch.no_grad():       # the closed-form fill predicts degenerate boxes (x0 == x1 -> NaN layout): make them boxes
        model.box_net[2].weight.mul_(0.05)
        model.box_net[2].bias.copy_(torch.tensor([0.1, 0.15, 0.6, 0.7]))
    model.eval()
    batch = make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=C, num_preds=P, num_attributes=A,
                       seed=321)
    imgs, objs, boxes, masks, triples, o2i, _, attributes = batch
    O = objs.size(0)
    arrs = {}
    for tag, kw in [('gtbox_gtmask', dict(boxes_gt=boxes, masks_gt=masks, use_gt_box=True)),
                    ('predbox_predmask', dict(boxes_gt=boxes, masks_gt=None, use_gt_box=False)),
                    ('features', dict(boxes_gt=boxes, masks_gt=masks, use_gt_box=True,
                                      features=[det((32,), 70 + i).abs() if i % 2 == 0 else None for i in range(O)]))]:
        torch.manual_seed(4242)
        noise = torch.randn((1, 64))
        torch.manual_seed(4242)
        with torch.no_grad():
            out = model(imgs, objs, triples, o2i, attributes=attributes, test_mode=True, **kw)
        imgs_pred, boxes_pred, masks_pred, gt_layout, pred_layout, wrong_layout = out
        assert gt_layout is None and wrong_layout is None
        arrs[tag + '_noise'] = noise
        arrs[tag + '_imgs_pred'] = imgs_pred
        arrs[tag + '_boxes_pred'] = boxes_pred
        arrs[tag + '_masks_pred'] = masks_pred
        arrs[tag + '_pred_layout'] = pred_layout
    npz('model_test_mode', seed=321, **arrs)


def golden_vgg():
    """losses.py:179-224: the reference's own Vgg19 / VGGLoss classes on a torchvision SHIM whose vgg19().features follows
    torchvision's published configuration 'E' (torchvision and its ImageNet weights are absent here).  Pins the
    reference-side arithmetic: slice boundaries, the 1/32..1 weights, L1 against the detached target features."""
    import torchvision.models as tvm
    from oracle.sg_oracle import vgg19_features

    class _V(nn.Module):
        def __init__(self):
            super().__init__()
            self.features = vgg19_features()
    tvm.vgg19 = lambda pretrained=False, **kw: _V()
    import importlib
    import scene_generation.losses as RL
    importlib.reload(RL)                       # picks up the shimmed ``models``
    crit = RL.VGGLoss()
    fill_deterministic(crit.vgg)
    x = det((2, 3, 32, 32), 91).requires_grad_()
    y = det((2, 3, 32, 32), 92)
    loss = crit(x, y)
    gx, = grads_of(loss, [x])
    feats = crit.vgg(x)
    npz('vgg_loss', x=x, y=y, loss=loss, gx=gx, keys=np.array(list(crit.vgg.state_dict().keys())),
        shapes=np.array([','.join(str(int(d)) for d in v.shape) for v in crit.vgg.state_dict().values()]),
        feat_stats=np.array([[float(f.double().sum()), float(f.double().abs().sum())] for f in feats]),
        feat0=feats[0][:, :4], feat4=feats[4])


def golden_losses2():
    """the non-default loss variants behind the same flags: --gan_loss_type wgan|lsgan (losses.py:93-132) and
    GANLoss(use_lsgan=False) = nn.BCELoss on the sigmoid outputs (losses.py:147)."""
    from scene_generation.losses import GANLoss, wgan_g_loss, wgan_d_loss, lsgan_g_loss, lsgan_d_loss
    sr, sf = det((7, 1), 168, 3.0).requires_grad_(), det((7, 1), 169, 3.0).requires_grad_()
    arrs = dict(sr=sr, sf=sf)
    for name, fn, args in [('wgan_g', wgan_g_loss, (sf,)), ('wgan_d', wgan_d_loss, (sr, sf)),
                           ('lsgan_g', lsgan_g_loss, (sf,)), ('lsgan_d', lsgan_d_loss, (sr, sf))]:
        v = fn(*args)
        g = grads_of(v, [sr, sf])
        arrs[name] = v
        arrs[name + '_gsr'], arrs[name + '_gsf'] = g
    crit = GANLoss(use_lsgan=False, tensor=torch.FloatTensor)
    probs = [[det((2, 4, 5, 5), 160), (det((2, 1, 6, 6), 161) + 0.5).clamp(0.02, 0.98).requires_grad_()],
             [det((2, 4, 3, 3), 162), (det((2, 1, 4, 4), 163) + 0.5).clamp(0.02, 0.98).requires_grad_()]]
    for t in (True, False):
        v = crit(probs, t)
        g = grads_of(v, [probs[0][1], probs[1][1]])
        arrs['bce_%d' % t] = v
        arrs['bce_%d_g0' % t], arrs['bce_%d_g1' % t] = g
    arrs['p0'], arrs['p1'] = probs[0][1], probs[1][1]
    npz('losses_variants', **arrs)


def golden_legacy():
    """The reference under ``align_corners=True`` -- what its grid_sample calls (layout.py:51,86,88; bilinear.py:130) meant on
    the PyTorch 1.0 it was written for (requirements.txt:8).  Captured by making True the default of F.grid_sample while
    the reference's functions run; pins the ``legacy_align_corners`` switch of the oracle and of the HIP kernels."""
    import torch.nn.functional as F
    from scene_generation.layout import masks_to_layout
    from scene_generation.bilinear import crop_bbox_batch
    real = F.grid_sample

    def legacy(input, grid, mode='bilinear', padding_mode='zeros', align_corners=None):
        return real(input, grid, mode=mode, padding_mode=padding_mode, align_corners=True)
    F.grid_sample = legacy
    try:
        vecs, boxes, masks, o2i = demo_layout_inputs()
        out = masks_to_layout(vecs, boxes, masks, o2i, 16)
        out_t = masks_to_layout(vecs, boxes, masks, o2i, 16, test_mode=True)
        g = torch.Generator().manual_seed(13)
        counts = [3, 1, 4]
        O = sum(counts)
        o2 = torch.cat([torch.full((c,), i, dtype=torch.long) for i, c in enumerate(counts)])
        v2 = det((O, 7), 221).requires_grad_()
        x0, y0 = torch.rand(O, generator=g) * 0.5, torch.rand(O, generator=g) * 0.5
        b2 = torch.stack([x0, y0, x0 + 0.1 + 0.4 * torch.rand(O, generator=g), y0 + 0.1 + 0.4 * torch.rand(O, generator=g)], 1)
        b2[0] = torch.tensor([0., 0., 1., 1.])
        m2 = torch.rand(O, 16, 16, generator=g)
        out2 = masks_to_layout(v2, b2, m2, o2, 20, 28)
        w2 = probe_weight(out2.shape, 222)
        gv2, = grads_of((out2 * w2).sum(), [v2])
        feats = det((3, 4, 20, 24), 231).requires_grad_()
        idx = torch.tensor([1, 0, 1, 2, 0, 2])
        cb = b2[:6].clone()
        cb[1] = torch.tensor([0.25, 0.25, 0.75, 0.75])
        crop = crop_bbox_batch(feats, cb, idx, 8)
        wc = probe_weight(crop.shape, 232)
        gf, = grads_of((crop * wc).sum(), [feats])
    finally:
        F.grid_sample = real
    npz('legacy_align_corners', vecs=vecs, boxes=boxes, masks=masks, obj_to_img=o2i, out=out, out_test=out_t,
        v2=v2, b2=b2, m2=m2, o2=o2, out2=out2, w2=w2, gv2=gv2, feats=feats, idx=idx, cb=cb, crop=crop, wc=wc, gf=gf)


def golden_args():
    """flag names + defaults of the reference parser (args.py:10-109)"""
    import json
    from scene_generation.args import parser
    d = vars(parser.parse_args([]))
    npz('args_defaults', json=np.array(json.dumps({k: (list(v) if isinstance(v, tuple) else v) for k, v in d.items()})))



def golden_dropin():
    """what the reference's entry script asks of the package (train.py:1-15 import statements, as module / names pairs) and the
    schema of the fresh checkpoint dict its get_checkpoint builds (train.py:128-163: key -> kind of empty value)"""
    import ast
    import json
    tree = ast.parse(open(os.path.join(REF, 'train.py')).read())
    imports = [{'module': n.module if isinstance(n, ast.ImportFrom) else None, 'names': [a.name for a in n.names]}
               for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == 'get_checkpoint'][0]
    fresh = [n for n in ast.walk(fn) if isinstance(n, ast.Dict)][0]
    schema = {}
    for k, v in zip(fresh.keys, fresh.values):
        if isinstance(v, ast.Call):
            kind = 'defaultdict(list)'
        elif isinstance(v, ast.List):
            kind = 'list'
        elif isinstance(v, ast.Dict):
            kind = {ast.literal_eval(kk): None for kk in v.keys} if v.keys else 'dict'
        elif isinstance(v, ast.Attribute):
            kind = 'args'
        elif isinstance(v, ast.Name):
            kind = 'vocab'
        else:
            kind = ast.literal_eval(v)
        schema[ast.literal_eval(k)] = kind
    npz('dropin_train_py', json=np.array(json.dumps({'imports': imports, 'fresh_checkpoint': schema})))


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    install_shims()
    which = sys.argv[1:] or ['gconv', 'layout', 'crop', 'modules', 'losses', 'losses2', 'vgg', 'legacy', 'step', 'step_full', 'eval', 'testmode', 'args', 'dropin']
    for w in which:
        globals()['golden_' + w]()
