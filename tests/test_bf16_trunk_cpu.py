"""Host-side surface of the opt-in bf16 residual trunk (GlobalGenerator.set_trunk_precision, SG_TRUNK_PRECISION, the C ABI
of sg_conv3x3r_bf16_*): no GPU needed."""
import copy

import pytest

from scene_generation_amd import _hip, ops
from scene_generation_amd.args import parser
from scene_generation_amd.generators import GlobalGenerator
from scene_generation_amd.layers import InstanceNorm2d
from scene_generation_amd.synthetic import make_vocab
from scene_generation_amd.trainer import Trainer

ARGV = ['--image_size', '32,32', '--batch_size', '2', '--vgg_features_weight', '0', '--output_dir', '/tmp/o',
        '--n_downsample_global', '2', '--gconv_hidden_dim', '64', '--gconv_num_layers', '3', '--mask_size', '8',
        '--ndf', '8', '--ndf_mask', '8', '--crop_size', '16', '--d_obj_arch', 'C4-8-2,C4-16-2', '--pool_size', '2']


def _gen():
    return GlobalGenerator(5, 3, ngf=8, n_downsampling=2, n_blocks=9, norm_layer=InstanceNorm2d)


@pytest.mark.parametrize('value,want', [(None, 'fp32'), ('', 'fp32'), ('fp32', 'fp32'), ('bf16', 'bf16')])
def test_env_parsing(value, want):
    env = {} if value is None else {'SG_TRUNK_PRECISION': value}
    assert ops.trunk_precision_from_env(env) == want


@pytest.mark.parametrize('value', ['BF16', 'fp16', 'bfloat16', '1'])
def test_env_parsing_rejects(value):
    with pytest.raises(ValueError):
        ops.trunk_precision_from_env({'SG_TRUNK_PRECISION': value})


def test_property_and_deepcopy():
    g = _gen()
    assert g.trunk_precision == 'fp32'
    assert g.trunk_paths() == [None] * 9
    g.set_trunk_precision('bf16')
    assert g.trunk_precision == 'bf16'
    with pytest.raises(AttributeError):
        g.trunk_precision = 'fp32'                 # read-only
    with pytest.raises(ValueError):
        g.set_trunk_precision('fp16')
    h = copy.deepcopy(g)
    assert h.trunk_precision == 'bf16'
    blocks = [m for m in h.model if type(m).__name__ == 'ResnetBlock']
    assert len(blocks) == 9 and all(b.conv_block.trunk_bf16 for b in blocks)
    h.set_trunk_precision('fp32')
    assert h.trunk_precision == 'fp32' and g.trunk_precision == 'bf16'
    assert not any(b.conv_block.trunk_bf16 for b in blocks)


def test_trainer_setting_keeps_model_kwargs(monkeypatch):
    args = parser.parse_args(ARGV)
    vocab = make_vocab(12, 4, 35)
    monkeypatch.delenv('SG_TRUNK_PRECISION', raising=False)
    ck32 = {'model_kwargs': {}, 'd_obj_kwargs': {}, 'd_mask_kwargs': {}, 'd_img_kwargs': {}}
    ck16 = copy.deepcopy(ck32)
    t32 = Trainer(args, vocab, checkpoint=ck32, device='cpu')
    t16 = Trainer(args, vocab, checkpoint=ck16, device='cpu', trunk_precision='bf16')
    assert ck16['model_kwargs'] == ck32['model_kwargs'] and 'trunk_precision' not in ck16['model_kwargs']
    assert t32.model.layout_to_image.trunk_precision == 'fp32'
    assert t16.model.layout_to_image.trunk_precision == 'bf16'
    assert sorted(t32.model.state_dict()) == sorted(t16.model.state_dict())
    monkeypatch.setenv('SG_TRUNK_PRECISION', 'bf16')
    assert Trainer(args, vocab, device='cpu').model.layout_to_image.trunk_precision == 'bf16'
    monkeypatch.setenv('SG_TRUNK_PRECISION', 'half')
    with pytest.raises(ValueError):
        Trainer(args, vocab, device='cpu')
    assert 'trunk_precision' not in vars(args)


def test_header_declares_entry_points():
    protos = _hip.parse_header()
    for name in ('sg_conv3x3r_bf16_supported', 'sg_conv3x3r_bf16_ws_bytes', 'sg_conv3x3r_bf16_fwd', 'sg_conv3x3r_bf16_dgrad',
                 'sg_conv3x3r_bf16_wgrad'):
        assert name in protos, name
    assert protos['sg_conv3x3r_bf16_fwd'][2] == ['d', 'x', 'w', 'bias', 'y', 'ws', 'ws_bytes', 'stream']
    assert protos['sg_conv3x3r_bf16_wgrad'][2] == ['d', 'gy', 'x', 'gw', 'gb', 'ws', 'ws_bytes', 'stream']
