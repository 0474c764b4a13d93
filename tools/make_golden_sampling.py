#!/usr/bin/env python
"""Capture the sampling fixtures from the REFERENCE implementation (build container only), with the shims of tools/make_golden.py.

  sample_encode.npz        Model.encode_scene_graphs (model.py:174-250) on two scene graphs in one call
  sample_forward_json.npz  Model.forward_json (model.py:252-256) of the small model of ``model_test_mode`` (with its box_net override)
  sample_deprocess.npz     imagenet_deprocess_batch (data/utils.py:17-51) with and without rescale, one constant image
  sample_layout_rgb.npz    one_hot_to_rgb (scripts/sample_images.py:156-160) on a test-mode layout
  sample_iou.npz           the "remove the __image__ object" loop + jaccard of scripts/sample_images.py:241-255

torchvision is absent here.  ``torchvision.transforms.Normalize`` / ``Compose`` are therefore a SHIM with their published
arithmetic -- Normalize(mean, std)(x) = (x - mean[c]) / std[c] per channel on a copy, Compose(ts)(x) = the calls in sequence --
which pins the reference-side composition (std = 1 / 0.5 first, then mean = -0.5, then the optional rescale), not torchvision.
scripts/sample_images.py cannot be imported (COCO loaders, scipy's image writer): its two pieces are taken out of its syntax tree
when this tool runs and executed as they stand.  Only DATA is written; inputs come from tests/sampling_helpers.py.
Re-run:  python tools/make_golden_sampling.py"""
import ast
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import make_golden as MG  # noqa: E402
import sampling_helpers as SH  # noqa: E402


class _Normalize(object):
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        t = t.clone()
        mean = torch.as_tensor(self.mean, dtype=t.dtype).view(-1, 1, 1)
        std = torch.as_tensor(self.std, dtype=t.dtype).view(-1, 1, 1)
        return t.sub_(mean).div_(std)


class _Compose(object):
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


def _script_tree():
    with open(os.path.join(MG.REF, 'scripts', 'sample_images.py')) as f:
        return ast.parse(f.read())


def _script_function(name, env):
    for node in _script_tree().body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            exec(compile(ast.Module([node], []), 'sample_images.py', 'exec'), env)
            return env[name]
    raise KeyError(name)


def _script_iou_statements():
    """the statements of run_model's batch loop that build boxes_*_no_image and call jaccard"""
    run = [n for n in _script_tree().body if isinstance(n, ast.FunctionDef) and n.name == 'run_model'][0]
    loop = [n for n in ast.walk(run) if isinstance(n, ast.For) and ast.unparse(n.target) == 'batch'][0]
    picked = [n for n in loop.body if 'no_image' in ast.unparse(n)]
    assert len(picked) == 7, [ast.unparse(n) for n in picked]           # two lists, the loop, two stacks, jaccard, total_boxes
    return picked[:6]


def golden_sampling():
    MG.install_shims()
    import torchvision.transforms as T
    T.Normalize, T.Compose = _Normalize, _Compose
    from scene_generation.model import Model
    from scene_generation.data.utils import imagenet_deprocess_batch
    from scene_generation.layout import masks_to_layout
    from scene_generation.metrics import jaccard

    # ---- encode_scene_graphs ----
    with MG.fake_cuda():
        model = SH.small_model(Model)
    sgs = SH.scene_graphs()
    objs, triples, o2i, attributes, features = model.encode_scene_graphs(sgs)
    MG.npz('sample_encode', objs=objs, triples=triples, obj_to_img=o2i, attributes=attributes, features=torch.stack(features),
           mutated=np.array(json.dumps(sgs)), bank_seed=SH.BANK_SEED)

    # ---- forward_json ----
    sgs = SH.scene_graphs()
    torch.manual_seed(4242)
    noise = torch.randn((1, 64))
    torch.manual_seed(4242)
    with torch.no_grad():
        (imgs_pred, boxes_pred, masks_pred, gt_layout, pred_layout, wrong_layout), objs = model.forward_json(sgs)
    assert gt_layout is None and wrong_layout is None and bool(torch.isfinite(imgs_pred).all())
    MG.npz('sample_forward_json', noise=noise, imgs_pred=imgs_pred, boxes_pred=boxes_pred, masks_pred=masks_pred,
           pred_layout=pred_layout, objs=objs, bank_seed=SH.BANK_SEED)

    # ---- imagenet_deprocess_batch ----
    arrs = {}
    for tag, x in SH.deprocess_inputs().items():
        arrs[tag + '_rescale'] = imagenet_deprocess_batch(x, rescale=True)
        arrs[tag + '_plain'] = imagenet_deprocess_batch(x, rescale=False)
    assert bool(torch.isnan(arrs['a_rescale'][2]).all())                 # the constant image: 0 / 0
    MG.npz('sample_deprocess', **arrs)

    # ---- one_hot_to_rgb on a test-mode layout ----
    vecs, boxes, masks, o2i, objs, colors, num_objs, H = SH.layout_rgb_inputs()
    layout = masks_to_layout(vecs, boxes, masks, o2i, H, test_mode=True)
    one_hot_to_rgb = _script_function('one_hot_to_rgb', {'torch': torch})
    MG.npz('sample_layout_rgb', layout=layout, rgb=one_hot_to_rgb(layout.clone(), colors, num_objs))

    # ---- IoU without the __image__ objects ----
    boxes_pred, boxes_gt, o2i = SH.iou_inputs()
    env = {'torch': torch, 'jaccard': jaccard, 'obj_to_img': o2i, 'boxes_pred': boxes_pred, 'boxes': boxes_gt, 'len': len,
           'range': range}
    exec(compile(ast.Module(_script_iou_statements(), []), 'sample_images.py', 'exec'), env)
    MG.npz('sample_iou', iou_sum=env['iou'], bigger_05=env['bigger_05'], bigger_03=env['bigger_03'],
           total_boxes=env['boxes_pred_no_image'].size(0))


if __name__ == '__main__':
    golden_sampling()
