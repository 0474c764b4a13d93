"""A small deterministic Trainer, its batch and a seeded run of steps: what the GPU modules that train for a few steps share
(tests/test_gpu_ema.py and the metric modules' training-loop tests)."""
import random

import torch

from scene_generation_amd.args import parser
from scene_generation_amd.synthetic import batch_to, fill_deterministic, make_batch, make_vocab
from scene_generation_amd.trainer import Trainer

DEV = 'cuda:0'
ARGV = ['--image_size', '32,32', '--batch_size', '3', '--vgg_features_weight', '0', '--output_dir', '/tmp/o',
        '--n_downsample_global', '2', '--gconv_hidden_dim', '64', '--gconv_num_layers', '3', '--mask_size', '8',
        '--ndf', '8', '--ndf_mask', '8', '--crop_size', '16', '--d_obj_arch', 'C4-8-2,C4-16-2', '--pool_size', '2']


def _trainer(tmp_path=None, **kw):
    argv = ARGV if tmp_path is None else ARGV[:ARGV.index('--output_dir')] + ['--output_dir', str(tmp_path)] + \
        ARGV[ARGV.index('--output_dir') + 2:]
    args = parser.parse_args(argv)
    ck = {'model_kwargs': {}, 'd_obj_kwargs': {}, 'd_mask_kwargs': {}, 'd_img_kwargs': {}}
    tr = Trainer(args, make_vocab(12, 4, 35), checkpoint=ck, device=DEV, **kw)
    for m in (tr.model, tr.netD, tr.obj_discriminator, tr.mask_discriminator):
        if m is not None:
            fill_deterministic(m)
    tr.model.noise_override = torch.linspace(-1, 1, args.mask_noise_dim).view(1, -1)
    if tr.ema is not None:
        tr.ema.reset()                             # the weights were refilled after construction
    return tr, ck, args


def _batch():
    return batch_to(make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=12, num_preds=4, seed=100), DEV)


USE_GT = [True, False, True, False, True]


def _run(tr, batch, seeds, snapshots=None):
    losses = []
    for s in seeds:
        random.seed(s)
        tr.step(batch, use_gt=USE_GT[s % len(USE_GT)])
        if snapshots is not None:
            snapshots.append(tr.optimizer.fp.flat.double().cpu())
        losses.append(dict(tr.generator_losses.items()))
    torch.cuda.synchronize()
    return losses
