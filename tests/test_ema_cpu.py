"""Host-side surface of the generator's parameter EMA (optim.ParamEMA, FusedAdam.attach_ema, Trainer(ema_decay=...),
SG_G_EMA_DECAY, the C ABI of sg_adam_step_ema / sg_ema_update, the checkpoint keys): no GPU needed."""
import copy

import pytest
import torch

from scene_generation_amd import _hip, optim
from scene_generation_amd.args import parser
from scene_generation_amd.synthetic import make_vocab
from scene_generation_amd.trainer import Trainer

ARGV = ['--image_size', '32,32', '--batch_size', '2', '--vgg_features_weight', '0',
        '--n_downsample_global', '2', '--gconv_hidden_dim', '64', '--gconv_num_layers', '3', '--mask_size', '8',
        '--ndf', '8', '--ndf_mask', '8', '--crop_size', '16', '--d_obj_arch', 'C4-8-2,C4-16-2', '--pool_size', '2']
EMA_KEYS = {'model_ema_state', 'ema_state', 'model_ema_best_state'}


@pytest.mark.parametrize('value,want', [(None, None), ('', None), ('0.999', 0.999), ('0.5', 0.5)])
def test_env_parsing(value, want):
    env = {} if value is None else {'SG_G_EMA_DECAY': value}
    assert optim.ema_decay_from_env(env) == want


@pytest.mark.parametrize('value', ['0', '1', '-1', 'abc', '1.5', 'nan'])
def test_env_parsing_rejects(value):
    with pytest.raises(ValueError):
        optim.ema_decay_from_env({'SG_G_EMA_DECAY': value})


def test_header_declares_entry_points():
    protos = _hip.parse_header()
    assert protos['sg_adam_step_ema'][2] == ['p', 'g', 'm', 'v', 'e', 'n', 'lr', 'beta1', 'beta2', 'eps', 'bias_corr1',
                                              'bias_corr2_sqrt', 'grad_scale', 'ema_w', 'stream']
    assert protos['sg_ema_update'][2] == ['e', 'p', 'n', 'ema_w', 'stream']
    # the Adam part takes exactly sg_adam_step's arguments, in its order
    adam = protos['sg_adam_step'][2]
    assert [a for a in protos['sg_adam_step_ema'][2] if a not in ('e', 'ema_w')] == adam


def _fp(*shapes):
    return optim.FlatParams([torch.nn.Parameter(torch.full(s, float(k + 1))) for k, s in enumerate(shapes)])


def test_weight_schedule():
    ema = optim.ParamEMA(_fp((3,)), 0.99, start=3)
    assert [ema.weight(k) for k in range(6)] == [1.0, 1.0, 1.0] + [1.0 - 0.99] * 3
    assert ema.weight() == 1.0
    ema.updates = 3
    assert ema.weight() == 1.0 - 0.99
    assert optim.ParamEMA(_fp((3,)), 0.9).weight(0) == 1.0 - 0.9
    for bad in (0.0, 1.0, -0.5):
        with pytest.raises(ValueError):
            optim.ParamEMA(_fp((3,)), bad)
    with pytest.raises(ValueError):
        optim.ParamEMA(_fp((3,)), 0.9, start=-1)


def test_buffer_layout_and_state_dict():
    fp = _fp((3,), (2, 5), (70,))
    ema = optim.ParamEMA(fp, 0.9, start=2)
    assert ema.flat.shape == fp.flat.shape and ema.flat.data_ptr() != fp.flat.data_ptr()
    assert torch.equal(ema.flat, fp.flat)                    # a copy, alignment gaps (zero) included
    for i, p in enumerate(fp.params):
        assert torch.equal(ema.param_view(i), p)
    ema.updates = 7
    sd = ema.state_dict()
    assert sd == {'decay': 0.9, 'start': 2, 'updates': 7}
    other = optim.ParamEMA(fp, 0.5)
    other.load_state_dict(sd)
    assert (other.decay, other.start, other.updates) == (0.9, 2, 7)


@pytest.mark.parametrize('touched,steps,want', [
    ([True] * 4, [0] * 4, [(0, 3, True)]),
    ([False] * 3, [0] * 3, [(0, 2, False)]),
    ([True, False, True], [1, 1, 1], [(0, 0, True), (1, 1, False), (2, 2, True)]),
    ([False, False, True, True, False], [0, 0, 2, 2, 0], [(0, 1, False), (2, 3, True), (4, 4, False)]),
    # touched runs split where the step counts differ; untouched runs do not care about step counts
    ([True, True, True, False, False], [3, 3, 2, 3, 1], [(0, 1, True), (2, 2, True), (3, 4, False)]),
    ([True], [0], [(0, 0, True)]),
    ([], [], []),
])
def test_step_runs(touched, steps, want):
    runs = optim.step_runs(touched, steps)
    assert runs == want
    # a partition of all parameters, in order
    assert [q for i, j, _ in runs for q in range(i, j + 1)] == list(range(len(touched)))


def _trainer(tmp_path, **kw):
    args = parser.parse_args(ARGV + ['--output_dir', str(tmp_path)])
    ck = {'model_kwargs': {}, 'd_obj_kwargs': {}, 'd_mask_kwargs': {}, 'd_img_kwargs': {}}
    return Trainer(args, make_vocab(12, 4, 35), checkpoint=ck, device='cpu', **kw), ck, args


def _save(tr, ck, args, t=1):
    path = tr.save_checkpoint(ck, t, args, 0, val_results=(0.5, 1.0, 0.1))
    return torch.load(path, weights_only=False)


def test_trainer_configuration(tmp_path, monkeypatch):
    monkeypatch.delenv('SG_G_EMA_DECAY', raising=False)
    tr, ck, args = _trainer(tmp_path)
    assert tr.ema is None and tr.optimizer.ema is None
    with pytest.raises(RuntimeError):
        tr.ema_model()
    monkeypatch.setenv('SG_G_EMA_DECAY', '0.99')
    tr, ck, args = _trainer(tmp_path, ema_start=4)
    assert (tr.ema.decay, tr.ema.start, tr.ema.updates) == (0.99, 4, 0)
    assert tr.optimizer.ema is tr.ema
    for opt in (tr.optimizer_d_img, tr.optimizer_d_obj, tr.optimizer_d_mask):
        assert opt.ema is None                               # the discriminators get no EMA
    tr2, _, _ = _trainer(tmp_path, ema_decay=0.5)            # the argument wins over the variable
    assert tr2.ema.decay == 0.5
    monkeypatch.setenv('SG_G_EMA_DECAY', 'abc')
    with pytest.raises(ValueError):
        _trainer(tmp_path)
    assert 'ema_decay' not in vars(args) and 'g_ema_decay' not in vars(args)


def test_ema_model_aliases_buffer(tmp_path, monkeypatch):
    monkeypatch.delenv('SG_G_EMA_DECAY', raising=False)
    tr, _, _ = _trainer(tmp_path, ema_decay=0.9)
    m = tr.ema_model()
    assert m is tr.ema_model()                               # built once
    assert not m.training and not any(p.requires_grad for p in m.parameters())
    for i, p in enumerate(m.parameters()):
        assert p.data_ptr() == tr.ema.param_view(i).data_ptr() and p.shape == tr.optimizer.fp.params[i].shape
    assert sorted(m.state_dict()) == sorted(tr.model.state_dict())
    # buffers follow the live model on every call
    bufs = dict(tr.model.named_buffers())
    assert bufs, 'the test model has no BatchNorm buffers'
    with torch.no_grad():
        for b in bufs.values():
            b.add_(3) if b.is_floating_point() else b.add_(1)
    for name, b in tr.ema_model().named_buffers():
        assert torch.equal(b, bufs[name]), name


def test_checkpoint_keys_ema_off_unchanged(tmp_path, monkeypatch):
    monkeypatch.delenv('SG_G_EMA_DECAY', raising=False)
    tr, ck, args = _trainer(tmp_path)
    saved = _save(tr, ck, args)
    assert not EMA_KEYS & set(saved)
    assert {'model_state', 'optim_state', 'model_best_state', 'optim_best_state', 'd_img_state', 'model_kwargs'} <= set(saved)
    tr_on, ck_on, args_on = _trainer(tmp_path / 'on', ema_decay=0.9)
    saved_on = _save(tr_on, ck_on, args_on)
    assert set(saved_on) - set(saved) == EMA_KEYS           # exactly today's keys, plus the three EMA keys with EMA on


def test_checkpoint_round_trip(tmp_path, monkeypatch):
    monkeypatch.delenv('SG_G_EMA_DECAY', raising=False)
    tr, ck, args = _trainer(tmp_path, ema_decay=0.9, ema_start=2)
    with torch.no_grad():
        tr.ema.flat.mul_(0.5)                                # an average that differs from the weights
    tr.ema.updates = 5
    saved = _save(tr, ck, args)
    assert saved['ema_state'] == {'decay': 0.9, 'start': 2, 'updates': 5}
    assert sorted(saved['model_ema_state']) == sorted(saved['model_state'])
    for n, p in tr.model.named_parameters():
        assert torch.equal(saved['model_ema_state'][n], p.detach() * 0.5), n
        assert torch.equal(saved['model_state'][n], p.detach()), n
    assert sorted(saved['model_ema_best_state']) == sorted(saved['model_state'])

    fresh, _, _ = _trainer(tmp_path / 'b', ema_decay=0.5)
    fresh.restore_checkpoint(copy.deepcopy(saved))
    assert torch.equal(fresh.ema.flat, tr.ema.flat)
    assert (fresh.ema.decay, fresh.ema.start, fresh.ema.updates) == (0.9, 2, 5)
    assert torch.equal(fresh.optimizer.fp.flat, tr.optimizer.fp.flat)
    best, _, _ = _trainer(tmp_path / 'c', ema_decay=0.9)
    best.restore_checkpoint(copy.deepcopy(saved), best=True)
    assert torch.equal(best.ema.flat, tr.ema.flat)
    # a plain Model loads the averaged weights
    plain, _, _ = _trainer(tmp_path / 'd')
    plain.model.load_state_dict(saved['model_ema_state'])
    assert torch.equal(plain.optimizer.fp.flat, tr.ema.flat)


def test_checkpoint_without_ema_keys(tmp_path, monkeypatch):
    monkeypatch.delenv('SG_G_EMA_DECAY', raising=False)
    off, ck, args = _trainer(tmp_path)
    with torch.no_grad():
        off.optimizer.fp.flat.mul_(-2.0)
    saved = _save(off, ck, args)
    on, _, _ = _trainer(tmp_path / 'on', ema_decay=0.9)
    assert not torch.equal(on.ema.flat, off.optimizer.fp.flat)
    on.restore_checkpoint(saved)
    assert torch.equal(on.optimizer.fp.flat, off.optimizer.fp.flat)
    assert torch.equal(on.ema.flat, on.optimizer.fp.flat)   # the average starts as a copy of the restored weights
    assert on.ema.updates == 0
