"""The generator's parameter EMA on the GPU: sg_adam_step_ema / sg_ema_update against sg_adam_step and a float64 lerp, parameters
Adam skips, a Trainer with the EMA against one without (bitwise the same training), the EMA against a float64 replay of the
weights, the side-stream ordering, Trainer.ema_model() and the checkpoint round trip."""
import copy

import pytest
import torch

from scene_generation_amd import ops, optim, streams
from scene_generation_amd.model import Model
from trainer_helpers import _batch, _run, _trainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LR, B1, B2, EPS = 1e-3, 0.5, 0.999, 1e-8


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _operands(n, seed):
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    p = sign * (0.5 + 1.5 * torch.rand(n, generator=g))          # |p| in [0.5, 2]: the lerp stays away from cancellation
    e = p * (1 + 0.01 * torch.randn(n, generator=g))             # an average close to the weights
    grad = torch.randn(n, generator=g)
    m = 0.1 * torch.randn(n, generator=g)
    v = 0.01 * torch.rand(n, generator=g)
    return [t.to(DEV) for t in (p, grad, m, v, e)]


def _adam(p, grad, m, v, step, gs):
    p, m, v = p.clone(), m.clone(), v.clone()
    ops.adam_step(p, grad, m, v, LR, B1, B2, EPS, step, gs)
    return p, m, v


def _adam_ema(p, grad, m, v, e, step, gs, w):
    p, m, v, e = p.clone(), m.clone(), v.clone(), e.clone()
    ops.adam_step_ema(p, grad, m, v, e, LR, B1, B2, EPS, step, gs, w)
    return p, m, v, e


@pytest.mark.parametrize('n', [1, 255, 257, 3 * 1024 * 1024 + 17])
@pytest.mark.parametrize('gs', [1.0, 0.25])
def test_kernel(n, gs):
    p, grad, m, v, e = _operands(n, seed=n)
    for step, w in ((1, 1.0 - 0.999), (7, 0.3)):
        p1, m1, v1 = _adam(p, grad, m, v, step, gs)
        p2, m2, v2, e2 = _adam_ema(p, grad, m, v, e, step, gs, w)
        p3, m3, v3, e3 = _adam_ema(p, grad, m, v, e, step, gs, w)
        e4 = ops.ema_update(e.clone(), p1, w)
        torch.cuda.synchronize()
        # Adam is bitwise sg_adam_step's; the EMA is bitwise sg_adam_step followed by sg_ema_update; two runs agree
        for a, b in ((p2, p1), (m2, m1), (v2, v1), (e2, e4), (p3, p2), (m3, m2), (v3, v2), (e3, e2)):
            assert torch.equal(a, b)
        assert not torch.equal(e2, e) and not torch.equal(p1, p)
        # within 1 ulp of a float64 lerp of the same fp32 inputs (and the same fp32 weight)
        ref = e.double() + _f32(w) * (p1.double() - e.double())
        ulp = torch.nextafter(ref.float().abs(), torch.tensor(float('inf'), device=DEV)) - ref.float().abs()
        assert bool(((e2.double() - ref).abs() <= ulp.double()).all())
    # weight 1: an exact copy of the updated parameter
    p1, _, _ = _adam(p, grad, m, v, 3, gs)
    _, _, _, e1 = _adam_ema(p, grad, m, v, e, 3, gs, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(e1, p1)
    assert torch.equal(ops.ema_update(e.clone(), p1, 1.0), p1)


def test_skipped_parameter_still_averaged():
    torch.manual_seed(0)
    shapes = [(33,), (10, 7), (5,)]
    params = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in shapes]
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt, ref = optim.FusedAdam(params, lr=LR, betas=(B1, B2)), optim.FusedAdam(twins, lr=LR, betas=(B1, B2))
    ema = optim.ParamEMA(opt.fp, 0.9)
    opt.attach_ema(ema)
    with torch.no_grad():
        ema.flat.zero_()                           # an average away from every weight
    x = torch.randn(10, 7, device=DEV)
    for o, ps in ((opt, params), (ref, twins)):
        o.zero_grad()
        ((ps[0] ** 2).sum() + (ps[2] * 3).sum()).backward()      # parameter 1 receives no gradient
        o.step()
    torch.cuda.synchronize()
    w = torch.tensor(1.0 - 0.9, dtype=torch.float32)
    assert ema.updates == 1 and opt.steps == [1, 0, 1]
    # Adam is untouched by the EMA: the same parameters and moments as an optimiser without it
    for buf, rbuf in ((opt.fp.flat, ref.fp.flat), (opt.exp_avg, ref.exp_avg), (opt.exp_avg_sq, ref.exp_avg_sq)):
        assert torch.equal(buf, rbuf)
    o1, n1 = opt.fp.offsets[1], x.numel()
    assert not bool(opt.exp_avg[o1:o1 + n1].any()) and not bool(opt.exp_avg_sq[o1:o1 + n1].any())
    assert torch.equal(params[1].detach(), twins[1].detach())
    # every parameter moved once: 0 + w * (p - 0), one rounding; the skipped one toward its unchanged value
    for i, p in enumerate(params):
        assert torch.equal(ema.param_view(i), w.to(DEV) * p.detach()), i


def _flats(tr):
    return [o.fp.flat for o in (tr.optimizer, tr.optimizer_d_img, tr.optimizer_d_obj, tr.optimizer_d_mask)]


@pytest.fixture(scope='module')
def runs():
    """5 steps (use_gt alternating) without EMA, with EMA (decay 0.8) and float64 snapshots of the weights, with EMA and the
    generator's Adam kept on the launch stream, and with EMA started only after 5 updates"""
    batch = _batch()
    off, _, _ = _trainer(ema_decay=None)
    assert off.ema is None
    l_off = _run(off, batch, range(5))
    saved = set(streams.GROUPS)
    out = {'off': (off, l_off)}
    try:
        streams.GROUPS.add('adam')                 # the generator's Adam (and so the EMA) on its side stream
        on, _, _ = _trainer(ema_decay=0.8)
        start = on.ema.flat.double().cpu()
        snaps = []
        out['on'] = (on, _run(on, batch, range(5), snaps), start, snaps)
        late, _, _ = _trainer(ema_decay=0.8, ema_start=5)
        out['late'] = (late, _run(late, batch, range(5)))
        streams.GROUPS.discard('adam')
        main, _, _ = _trainer(ema_decay=0.8)
        out['main'] = (main, _run(main, batch, range(5)))
    finally:
        streams.GROUPS.clear()
        streams.GROUPS.update(saved)
    return out


def test_trainer_ema_keeps_training_bitwise(runs, monkeypatch):
    monkeypatch.delenv('SG_G_EMA_DECAY', raising=False)
    off, l_off = runs['off']
    for name in ('on', 'late', 'main'):
        tr, losses = runs[name][:2]
        assert losses == l_off, name
        for a, b in zip(_flats(tr), _flats(off)):
            assert torch.equal(a, b), name
        assert tr.ema.updates == 5


def test_trainer_ema_matches_fp64_replay(runs):
    on, _, start, snaps = runs['on']
    ref = start.clone()
    for k, snap in enumerate(snaps):
        ref = ref + _f32(on.ema.weight(k)) * (snap - ref)
    assert not torch.equal(on.ema.flat.cpu(), on.optimizer.fp.flat.cpu())
    err = float((on.ema.flat.double().cpu() - ref).abs().max())
    assert err <= 1e-6 * float(ref.abs().max()), err


def test_trainer_ema_start_copies_weights(runs):
    late = runs['late'][0]
    assert torch.equal(late.ema.flat, late.optimizer.fp.flat)


def test_trainer_ema_stream_ordering(runs):
    # the EMA written on the 'adam' side stream is the EMA written on the launch stream
    assert torch.equal(runs['on'][0].ema.flat, runs['main'][0].ema.flat)


def _sample(model, batch):
    imgs, objs, boxes, masks, triples, obj_to_img, triple_to_img, attributes = batch
    with torch.no_grad():
        out = model(imgs, objs, triples, obj_to_img, boxes_gt=boxes, masks_gt=masks, attributes=attributes, test_mode=True,
                    use_gt_box=True)
    torch.cuda.synchronize()
    return out[0].clone()


def test_ema_model(runs):
    batch = _batch()
    for name, same in (('late', True), ('on', False)):
        tr = runs[name][0]
        m = tr.ema_model()
        assert m is tr.ema_model() and not m.training
        for i, p in enumerate(m.parameters()):
            assert p.data_ptr() == tr.ema.param_view(i).data_ptr() and not p.requires_grad
        live = dict(tr.model.named_buffers())
        assert any('running_mean' in k for k in live)
        for k, b in m.named_buffers():
            assert torch.equal(b, live[k]), k
        m.noise_override = tr.model.noise_override
        tr.model.eval()
        try:
            want = _sample(tr.model, batch)
        finally:
            tr.model.train()
        got = _sample(m, batch)
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got, want) == same, name


def test_checkpoint_round_trip(tmp_path):
    batch = _batch()
    tr, ck, args = _trainer(tmp_path / 'a', ema_decay=0.8)
    _run(tr, batch, range(3))
    path = tr.save_checkpoint(ck, 3, args, 0, val_results=(0.5, 1.0, 0.1))
    saved = torch.load(path, map_location='cpu', weights_only=False)
    pool = copy.deepcopy(tr.model.fake_pool)       # the appearance pool is not part of a checkpoint (the reference's neither)
    _run(tr, batch, range(3, 5))

    fresh, _, _ = _trainer(tmp_path / 'b', ema_decay=0.8)
    fresh.restore_checkpoint(saved)
    fresh.model.fake_pool = pool
    assert fresh.ema.updates == 3
    for i, (n, _) in enumerate(fresh.model.named_parameters()):
        assert torch.equal(fresh.ema.param_view(i).cpu(), saved['model_ema_state'][n]), n
    _run(fresh, batch, range(3, 5))
    assert fresh.ema.updates == tr.ema.updates == 5
    assert torch.equal(fresh.ema.flat, tr.ema.flat)
    assert torch.equal(fresh.optimizer.fp.flat, tr.optimizer.fp.flat)
    # the averaged weights load into a plain Model
    plain = Model(**saved['model_kwargs']).to(DEV)
    plain.load_state_dict(saved['model_ema_state'])
    for n, p in plain.named_parameters():
        assert torch.equal(p.detach().cpu(), saved['model_ema_state'][n]), n
