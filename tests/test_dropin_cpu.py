"""The drop-in switch (scene_generation_amd.install_as) against what the reference's entry script asks of the package, CPU only.

tests/golden/dropin_train_py.npz (tools/make_golden.py::golden_dropin) holds the import statements of the reference's train.py
(train.py:1-15, as module / names pairs) and the schema of the fresh checkpoint dict its get_checkpoint builds
(train.py:128-163).  A subprocess lays out a stand-in host checkout in a temporary directory -- ``scene_generation/data``,
``scene_generation/metrics.py`` and ``scripts/inception_score.py``, the parts of the reference this package does not replace --
aliases the package as ``scene_generation``, executes those import statements, then builds the checkpoint dict and the Trainer
the way train.py:119-188 does, saves with the reference's schema and restores.
"""
import json
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the stand-in host checkout: only names, no behaviour beyond what the script below calls
HOST_FILES = {
    'scene_generation/__init__.py': '',
    'scene_generation/data/__init__.py': '',
    'scene_generation/data/coco.py': 'class CocoSceneGraphDataset(object):\n    pass\n\n\ndef coco_collate_fn(batch):\n    return batch\n',
    'scene_generation/data/coco_panoptic.py': ('class CocoPanopticSceneGraphDataset(object):\n    pass\n\n\n'
                                               'def coco_panoptic_collate_fn(batch):\n    return batch\n'),
    'scene_generation/metrics.py': 'def jaccard(boxes_pred, boxes):\n    return 0.0, 0, 0\n',
    'scripts/__init__.py': '',
    'scripts/inception_score.py': 'class InceptionScore(object):\n    pass\n',
}

SCRIPT = r"""
import collections, importlib, json, os, sys
host, spec = %(host)r, json.loads(open(%(spec)r).read())
sys.path.insert(0, %(root)r)
sys.path.insert(0, host)
os.chdir(host)
import scene_generation_amd
scene_generation_amd.install_as('scene_generation')

# ---- train.py:1-15: every import statement of the reference's entry script ----
ns = {}
for imp in spec['imports']:
    if imp['module'] is None:
        for n in imp['names']:
            ns[n.split('.')[0]] = importlib.import_module(n)
    else:
        mod = importlib.import_module(imp['module'])
        for n in imp['names']:
            ns[n] = getattr(mod, n)
assert ns['Trainer'].__module__ == 'scene_generation_amd.trainer', ns['Trainer'].__module__
assert ns['get_args'].__module__ == 'scene_generation_amd.args'
assert ns['CocoSceneGraphDataset'].__module__ == 'scene_generation.data.coco'
for m in ('scene_generation.data.coco', 'scene_generation.data.coco_panoptic', 'scene_generation.metrics'):
    assert os.path.realpath(sys.modules[m].__file__).startswith(os.path.realpath(host)), m
import torch
# the evaluation script's only import from the package (scripts/inception_score.py:12,30)
from scene_generation.layers import Interpolate
up = Interpolate(size=(9, 9), mode='bilinear')
assert tuple(up(torch.zeros(1, 3, 4, 4)).shape) == (1, 3, 9, 9)


# ---- train.py:119-163 (get_checkpoint) + :166-170 (Trainer construction) ----
def get_checkpoint(args, vocab):
    if args.restore_from_checkpoint:
        checkpoint = torch.load(os.path.join(args.output_dir, '%%s_with_model.pt' %% args.checkpoint_name))
        return checkpoint['counters']['t'], checkpoint['counters']['epoch'], checkpoint
    kinds = {'args': lambda: args.__dict__, 'vocab': lambda: vocab, 'dict': dict, 'list': list,
             'defaultdict(list)': lambda: collections.defaultdict(list)}
    fresh = {k: (dict(v) if isinstance(v, dict) else kinds[v]() if isinstance(v, str) else v)
             for k, v in spec['fresh_checkpoint'].items()}
    return 0, 0, fresh


from scene_generation_amd.synthetic import make_vocab
args = ns['get_args'](['--output_dir', %(out)r, '--image_size', '32,32', '--n_downsample_global', '2', '--ndf', '8',
                       '--ndf_mask', '8', '--gconv_hidden_dim', '64'])
os.makedirs(args.output_dir, exist_ok=True)
vocab = make_vocab()
t, epoch, checkpoint = get_checkpoint(args, vocab)
assert (t, epoch) == (0, 0) and checkpoint['counters'] == {'t': None, 'epoch': None} and len(checkpoint) >= 30
trainer = ns['Trainer'](args, vocab, checkpoint)
for attr in ('model', 'netD', 'obj_discriminator', 'mask_discriminator', 'optimizer', 'optimizer_d_obj',
             'optimizer_d_mask', 'optimizer_d_img', 'num_obj', 'writer', 'criterionVGG', 'criterionGAN'):
    assert getattr(trainer, attr) is not None, attr
assert trainer.criterionVGG is not None          # the reference's default flags (vgg_features_weight 10) construct
assert set(checkpoint['model_kwargs']) >= {'vocab', 'image_size', 'rep_size'} and checkpoint['d_img_kwargs']['input_nc'] == 207
# save with the reference's schema, reload through restore_checkpoint (latest and *_best_state)
p0 = trainer.model.box_net[0].weight.detach().clone()
path = trainer.save_checkpoint(checkpoint, 7, args, 1, (0.1, 1.5, 0.2, None), (0.2, 1.7, 0.3, None))
ck = torch.load(path, map_location='cpu', weights_only=False)
for k in ('model_state', 'optim_state', 'd_obj_state', 'd_obj_optim_state', 'd_mask_state', 'd_mask_optim_state',
          'd_img_state', 'd_img_optim_state', 'model_best_state', 'optim_best_state', 'd_obj_best_state',
          'd_mask_best_state', 'd_img_best_state', 'd_img_optim_best_state', 'best_t', 'counters', 'val_inception',
          'train_inception', 'checkpoint_ts', 'model_kwargs', 'd_obj_kwargs', 'd_mask_kwargs', 'd_img_kwargs', 'vocab', 'args'):
    assert k in ck, k
assert ck['counters'] == {'t': 7, 'epoch': 1} and ck['best_t'] == [7]
with torch.no_grad():
    trainer.model.box_net[0].weight.add_(1.0)
trainer.restore_checkpoint(ck, best=True)
assert torch.equal(trainer.model.box_net[0].weight, p0)
_tl = torch.load                   # train.py:127 predates torch 2.6's weights_only=True default (the file holds dicts)
torch.load = lambda *a, **k: _tl(*a, **dict(k, weights_only=False))
args2 = ns['get_args'](['--output_dir', %(out)r, '--restore_from_checkpoint', '1', '--image_size', '32,32'])
t2, epoch2, ck2 = get_checkpoint(args2, vocab)          # train.py:121-125 reads the file just written
assert t2 == 7 and epoch2 == 1
tr2 = ns['Trainer'](args2, vocab, ck2)
tr2.restore_checkpoint(ck2)
assert torch.equal(tr2.model.box_net[0].weight, p0)
trainer.generator_losses = None
print('DROPIN_OK')
"""


def test_install_as_runs_reference_train_py_imports_and_trainer_construction(tmp_path, golden):
    spec = json.loads(str(golden('dropin_train_py')['json']))
    assert any(i['module'] == 'scene_generation.trainer' for i in spec['imports'])
    host = tmp_path / 'host'
    for rel, text in HOST_FILES.items():
        f = host / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text)
    (tmp_path / 'spec.json').write_text(json.dumps(spec))
    code = SCRIPT % dict(root=ROOT, host=str(host), spec=str(tmp_path / 'spec.json'), out=str(tmp_path / 'out'))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS='4'))
    assert r.returncode == 0 and 'DROPIN_OK' in r.stdout, textwrap.shorten(r.stdout + r.stderr, 4000)


def test_conv2d_rejects_the_reflection_pad_torch_refuses():
    """a reflection pad that reaches the plane's size on EITHER axis: torch refuses it, and so does the drop-in conv -- before any
    device call (the kernels mirror a coordinate once; the library's desc check is the second line)"""
    import pytest
    import torch
    import torch.nn.functional as F
    from scene_generation_amd import ops
    w = torch.zeros(4, 2, 7, 7)
    for shape, ups in (((1, 2, 8, 3), 1), ((1, 2, 3, 8), 1), ((1, 2, 3, 3), 1), ((1, 2, 4, 1), 2)):
        x = torch.zeros(shape)
        with pytest.raises(RuntimeError):
            ops.conv2d(x, w, None, stride=1, pad=3, reflect=True, upsample=ups)
        with pytest.raises(RuntimeError):
            F.pad(F.interpolate(x, scale_factor=ups, mode='nearest'), (3,) * 4, mode='reflect')
    with pytest.raises(RuntimeError):
        ops.conv2d(torch.zeros(1, 2, 5, 5), w, None, stride=1, pad=-1, reflect=True)


def test_install_as_without_host_checkout_only_overlays_hot_path(tmp_path):
    """On a box without the reference (the GPU box): the alias resolves the hot-path modules and leaves
    ``scene_generation.data`` absent instead of breaking them."""
    code = textwrap.dedent('''
        import sys
        sys.path = [p for p in sys.path if 'reference' not in p]
        sys.path.insert(0, %r)
        import scene_generation_amd
        scene_generation_amd.install_as('scene_generation', host_package_dir='')
        from scene_generation.model import Model
        from scene_generation.layout import masks_to_layout, boxes_to_layout
        from scene_generation.graph import GraphTripleConv, GraphTripleConvNet
        from scene_generation.losses import get_gan_losses, GANLoss, VGGLoss
        assert Model.__module__ == 'scene_generation_amd.model'
        for t in ('gan', 'wgan', 'lsgan'):
            get_gan_losses(t)
        print('OVERLAY_OK')
    ''' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0 and 'OVERLAY_OK' in r.stdout, r.stdout + r.stderr
