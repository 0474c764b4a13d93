"""The gradient control of the fused Adam step on the GPU: sg_grad_norm against the float64 restatement (tests/gradctl_ref.py),
non-finite gradients, sg_adam_step_ctl / sg_adam_step_ema_ctl against sg_adam_step / sg_adam_step_ema / sg_ema_update bit for bit,
FusedAdam.set_grad_control against clip_grad_norm_ + torch.optim.Adam, and Trainers with the control against plain ones."""
import functools
import math
import random

import pytest
import torch
from torch import nn

import gradctl_ref as R
from scene_generation_amd import ops, optim
from scene_generation_amd.args import parser
from scene_generation_amd.synthetic import batch_to, fill_deterministic, make_batch, make_vocab
from scene_generation_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LR, B1, B2, EPS = 1e-3, 0.5, 0.999, 1e-8
BITS = ('sumsq', 'norm', 'coef', 'skip')


@functools.lru_cache(maxsize=None)
def _gradient(n, offset=0):
    """(host fp32 gradient of n elements, its float64 sum of squares); on the device it starts ``offset`` elements into its
    allocation"""
    g = torch.randn(n, generator=torch.Generator().manual_seed(n + offset))
    return g, R.record(g)['sumsq']


def _on_device(g, offset=0):
    buf = torch.empty(g.numel() + offset, device=DEV)
    buf[offset:].copy_(g)
    return buf[offset:]


def _read(ctl):
    return ops.grad_ctl_read(ctl)


def _same_bits(a, b):
    return all(R.np.float64(a[k]).tobytes() == R.np.float64(b[k]).tobytes() for k in BITS)


@pytest.mark.parametrize('gs', [1.0, 0.125])
@pytest.mark.parametrize('n,offset', [(1, 0), (255, 0), (256, 0), (257, 0), (65539, 0), (65539, 1), ((1 << 22) + 5, 0),
                                      # a dozen workgroups of the capped grid (1 024 workgroups x 256 lanes x 4 loads) go round twice
                                      (4 * (1024 * 1024 + 3075) + 3, 0)])
def test_grad_norm(n, offset, gs):
    host, sumsq = _gradient(n, offset)
    g = _on_device(host, offset)
    assert g.data_ptr() % 16 == 4 * offset
    ctl, ws = ops.grad_ctl_alloc(torch.device(DEV))
    rec = _read(ops.grad_norm(g, ctl, ws, gs, 0.0))
    ref = R.from_sumsq(sumsq, gs, 0.0)
    print('n=%d offset=%d gs=%g: sumsq rel err %.3g (bound %.3g), norm %r vs %r'
          % (n, offset, gs, abs(rec['sumsq'] - sumsq) / sumsq, n * 2.0 ** -53, rec['norm'], ref['norm']))
    assert abs(rec['sumsq'] - sumsq) <= n * 2.0 ** -53 * sumsq
    ulp = float(R.np.spacing(R.np.float32(ref['norm'])))
    assert abs(rec['norm'] - ref['norm']) <= ulp
    assert (rec['coef'], rec['skip'], rec['skipped'], rec['steps']) == (1.0, 0, 0, 1)
    # the clip coefficient is the formula on the device's own norm: clipping at half the norm, not at twice it, off
    calls = 1
    for max_norm in (0.5 * rec['norm'], 2.0 * rec['norm'], 0.0, float('inf'), -1.0):
        got = _read(ops.grad_norm(g, ctl, ws, gs, max_norm))
        calls += 1
        want = R.from_sumsq(got['sumsq'], gs, max_norm)
        assert got['coef'] == want['coef'] and got['norm'] == want['norm'] and got['skip'] == 0, (max_norm, got, want)
        assert (got['coef'] < 1.0) == (max_norm == 0.5 * rec['norm'])
        assert got['steps'] == calls and got['skipped'] == 0
    # the same bits on every call and on every stream
    again = _read(ops.grad_norm(g, ctl, ws, gs, 0.0))
    assert _same_bits(again, rec)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    ctl2, ws2 = ops.grad_ctl_alloc(torch.device(DEV))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = _read(ops.grad_norm(g, ctl2, ws2, gs, 0.0))
    side.synchronize()
    assert _same_bits(other, rec) and other['steps'] == 1


def _operands(n, seed):
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    p = sign * (0.5 + 1.5 * torch.rand(n, generator=g))
    e = p * (1 + 0.01 * torch.randn(n, generator=g))
    grad = torch.randn(n, generator=g)
    m = 0.1 * torch.randn(n, generator=g)
    v = 0.01 * torch.rand(n, generator=g)
    return [t.to(DEV) for t in (p, grad, m, v, e)]


N_BAD = 70001            # 17 500 float4s -- the last 256-lane group of them holds 92 -- then one tail element


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
@pytest.mark.parametrize('where', [0, N_BAD - 1, 4 * (17 * 1024 + 50) + 1])
def test_non_finite_gradient_skips_the_step(where, bad):
    p, grad, m, v, e = _operands(N_BAD, seed=7)
    ctl, ws = ops.grad_ctl_alloc(torch.device(DEV))
    rec = _read(ops.grad_norm(grad, ctl, ws, 1.0, 1.0))
    assert (rec['skip'], rec['skipped'], rec['steps']) == (0, 0, 1) and rec['coef'] < 1.0
    grad[where] = bad                      # data, like any other gradient value
    rec = _read(ops.grad_norm(grad, ctl, ws, 1.0, 1.0))
    assert (rec['skip'], rec['skipped'], rec['steps'], rec['coef']) == (1, 1, 2, 1.0) and not math.isfinite(rec['norm'])
    p1, m1, v1 = p.clone(), m.clone(), v.clone()
    ops.adam_step_ctl(p1, grad, m1, v1, ctl, LR, B1, B2, EPS, 3, 1.0)
    p2, m2, v2, e2 = p.clone(), m.clone(), v.clone(), e.clone()
    ops.adam_step_ema_ctl(p2, grad, m2, v2, e2, ctl, LR, B1, B2, EPS, 3, 1.0, 0.3)
    e3 = ops.ema_update(e.clone(), p, 0.3)
    torch.cuda.synchronize()
    for a, b in ((p1, p), (m1, m), (v1, v), (p2, p), (m2, m), (v2, v), (e2, e3)):
        assert torch.equal(a, b)
    assert not torch.equal(e2, e) and bool(torch.isfinite(e2).all())
    # a finite gradient afterwards: the flag clears, the count stays
    grad[where] = 0.5
    rec = _read(ops.grad_norm(grad, ctl, ws, 1.0, 1.0))
    assert (rec['skip'], rec['skipped'], rec['steps']) == (0, 1, 3) and math.isfinite(rec['norm'])
    ops.adam_step_ctl(p1, grad, m1, v1, ctl, LR, B1, B2, EPS, 3, 1.0)
    torch.cuda.synchronize()
    assert not torch.equal(p1, p) and bool(torch.isfinite(p1).all())


@pytest.mark.parametrize('n', [1, 257, 3 * 1024 * 1024 + 17])
@pytest.mark.parametrize('gs', [1.0, 0.25])
@pytest.mark.parametrize('clip', [False, True])
def test_kernel(n, gs, clip):
    p, grad, m, v, e = _operands(n, seed=n)
    ctl, ws = ops.grad_ctl_alloc(torch.device(DEV))
    norm = _read(ops.grad_norm(grad, ctl, ws, gs, 0.0))['norm']
    coef = _read(ops.grad_norm(grad, ctl, ws, gs, 0.37 * norm if clip else 0.0))['coef']
    assert (coef < 1.0) == clip and coef > 0.3
    scale = R.f32(R.f32(gs) * coef)        # the product of two fp32 numbers, rounded to fp32 once
    for step, w in ((1, 1.0 - 0.999), (7, 1.0)):
        p1, m1, v1 = p.clone(), m.clone(), v.clone()
        ops.adam_step(p1, grad, m1, v1, LR, B1, B2, EPS, step, scale)
        p2, m2, v2 = p.clone(), m.clone(), v.clone()
        ops.adam_step_ctl(p2, grad, m2, v2, ctl, LR, B1, B2, EPS, step, gs)
        p3, m3, v3, e3 = p.clone(), m.clone(), v.clone(), e.clone()
        ops.adam_step_ema(p3, grad, m3, v3, e3, LR, B1, B2, EPS, step, scale, w)
        p4, m4, v4, e4 = p.clone(), m.clone(), v.clone(), e.clone()
        ops.adam_step_ema_ctl(p4, grad, m4, v4, e4, ctl, LR, B1, B2, EPS, step, gs, w)
        torch.cuda.synchronize()
        for a, b in ((p2, p1), (m2, m1), (v2, v1), (p4, p3), (m4, m3), (v4, v3), (e4, e3), (p4, p1)):
            assert torch.equal(a, b)
        assert not torch.equal(p1, p) and not torch.equal(e4, e)
        if clip:                           # the coefficient did enter: the unclipped step differs
            p5, m5, v5 = p.clone(), m.clone(), v.clone()
            ops.adam_step(p5, grad, m5, v5, LR, B1, B2, EPS, step, gs)
            torch.cuda.synchronize()
            assert not torch.equal(m5, m2)


# ---- FusedAdam against torch -------------------------------------------------------------------------------------------------------

def _two_linear():
    model = nn.Sequential(nn.Linear(7, 5), nn.Linear(5, 3))
    fill_deterministic(model)
    return model


def _grads(model, it):
    g = torch.Generator().manual_seed(100 + it)
    # the scale changes from step to step: a threshold of 1 clips steps 1 and 4 and leaves the others alone
    return [(0.02, 3.0, 0.05)[it % 3] * torch.randn(p.shape, generator=g) for p in model.parameters()]


def _close(a, b, tol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), what


@pytest.mark.parametrize('pre_scale', [1.0, 0.25])
def test_fused_adam_matches_torch(pre_scale):
    """5 steps of clip_grad_norm_ + torch.optim.Adam on the CPU against FusedAdam.set_grad_control(max_norm=1); with
    ``pre_scale`` a pre-step hook sets grad_scale (what a data-parallel reducer with a deferred 1 / world does) and torch gets the
    scaled gradient"""
    ref, mine = _two_linear(), _two_linear().to(DEV)
    o_ref = torch.optim.Adam(ref.parameters(), lr=1e-2, betas=(0.5, 0.999))
    o_mine = optim.FusedAdam(mine.parameters(), lr=1e-2, betas=(0.5, 0.999))
    o_mine.set_grad_control(max_norm=1.0)
    twin = optim.FusedAdam(_two_linear().to(DEV).parameters(), lr=1e-2, betas=(0.5, 0.999))      # monitor only, never scaled
    twin.set_grad_control()
    if pre_scale != 1.0:
        o_mine.pre_step_hooks.append(lambda: setattr(o_mine, 'grad_scale', pre_scale))
    numel = sum(p.numel() for p in ref.parameters())
    clipped = []
    for it in range(5):
        grads = _grads(ref, it)
        o_ref.zero_grad()
        for o in (o_mine, twin):
            o.zero_grad()
            for q, g in zip(o.fp.params, grads):
                q.grad.add_(g.to(DEV))
            o.mark_all_touched()
        for p, g in zip(ref.parameters(), grads):
            p.grad = g * pre_scale
        total = float(nn.utils.clip_grad_norm_(ref.parameters(), 1.0))
        o_ref.step()
        o_mine.step()
        twin.step()
        st, st_twin = o_mine.grad_stats(), twin.grad_stats()
        assert sorted(st) == ['coef', 'norm', 'skip', 'skipped', 'steps']
        # torch sums the squares in fp32: at most one rounding of 2^-24 per element
        assert abs(st['norm'] - total) <= numel * 2.0 ** -24 * total
        assert st['norm'] == pre_scale * st_twin['norm']             # a power of two: exact
        assert st['coef'] == R.f32(min(1.0, 1.0 / (R.from_sumsq(R.record(torch.cat([g.reshape(-1) for g in grads]))['sumsq'],
                                                                pre_scale)['norm_d'] + 1e-6)))
        assert (st['skip'], st['skipped'], st['steps']) == (0, 0, it + 1) and st_twin['coef'] == 1.0
        assert o_mine.grad_scale == 1.0
        clipped.append(st['coef'] < 1.0)
        # p.grad is left as the backward wrote it
        assert torch.equal(o_mine.fp.packed(o_mine.fp.grad).cpu(), torch.cat([g.reshape(-1) for g in grads]))
    assert clipped == [False, True, False, False, True]
    for p, q in zip(ref.parameters(), mine.parameters()):
        _close(q, p, 1e-6, 'param after adam')
    sd, sd_ref = o_mine.state_dict(), o_ref.state_dict()
    for i in sd_ref['state']:
        _close(sd['state'][i]['exp_avg'], sd_ref['state'][i]['exp_avg'], 1e-6, 'exp_avg')
        _close(sd['state'][i]['exp_avg_sq'], sd_ref['state'][i]['exp_avg_sq'], 1e-6, 'exp_avg_sq')
        assert float(sd['state'][i]['step']) == float(sd_ref['state'][i]['step'])


def test_control_off_issues_the_plain_launches():
    def one_step(o):
        o.zero_grad()
        for q in o.fp.params:
            q.grad.add_(1.0)
        o.mark_all_touched()
        before = ops.CALLS[0]
        o.step()
        return ops.CALLS[0] - before
    plain = optim.FusedAdam(_two_linear().to(DEV).parameters(), lr=1e-2)
    other = optim.FusedAdam(_two_linear().to(DEV).parameters(), lr=1e-2)
    base = one_step(plain)
    other.set_grad_control(max_norm=1e30)
    assert one_step(other) == base + 1                 # the norm pass; the Adam launch is replaced, not added to
    other.set_grad_control(None, False)
    assert other.grad_stats() is None and one_step(other) == base
    one_step(plain)
    torch.cuda.synchronize()
    assert torch.equal(other.fp.flat, plain.fp.flat) and torch.equal(other.exp_avg_sq, plain.exp_avg_sq)


# ---- Trainer ----------------------------------------------------------------------------------------------------------------------

ARGV = ['--image_size', '32,32', '--batch_size', '3', '--vgg_features_weight', '0', '--output_dir', '/tmp/o',
        '--n_downsample_global', '2', '--gconv_hidden_dim', '64', '--gconv_num_layers', '3', '--mask_size', '8',
        '--ndf', '8', '--ndf_mask', '8', '--crop_size', '16', '--d_obj_arch', 'C4-8-2,C4-16-2', '--pool_size', '2']
USE_GT = [True, False, True]


def _trainer(**kw):
    args = parser.parse_args(ARGV)
    ck = {'model_kwargs': {}, 'd_obj_kwargs': {}, 'd_mask_kwargs': {}, 'd_img_kwargs': {}}
    tr = Trainer(args, make_vocab(12, 4, 35), checkpoint=ck, device=DEV, **kw)
    for m in (tr.model, tr.netD, tr.obj_discriminator, tr.mask_discriminator):
        fill_deterministic(m)
    tr.model.noise_override = torch.linspace(-1, 1, args.mask_noise_dim).view(1, -1)
    return tr


def _step(tr, batch, s):
    random.seed(s)
    tr.step(batch, use_gt=USE_GT[s])
    torch.cuda.synchronize()


def _flats(tr):
    return [o.fp.flat for _, o in tr.named_optimizers()]


def _g_state(tr):
    o = tr.optimizer
    return [t.clone() for t in (o.fp.flat, o.exp_avg, o.exp_avg_sq)]


@pytest.fixture(scope='module')
def runs(request):
    """three steps (default side streams) of a plain Trainer, of one clipping at 1e30, of a monitor-only one (with its state around
    step 1), of one whose generator gradient receives a NaN in step 2; one step of one clipping the generator at half the
    monitor-only twin's first norm"""
    import os
    saved = {k: os.environ.pop(k, None) for k in ('SG_GRAD_CLIP', 'SG_GRAD_NORMS', 'SG_G_EMA_DECAY')}
    request.addfinalizer(lambda: os.environ.update({k: v for k, v in saved.items() if v is not None}))
    batch = batch_to(make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=12, num_preds=4, seed=100), DEV)
    out = {}
    plain = _trainer()
    assert plain.grad_stats() == {}
    d_after = []
    for s in range(3):
        _step(plain, batch, s)
        d_after.append([f.clone() for f in _flats(plain)[1:]])
    out['plain'], out['plain_d_after'] = plain, d_after

    huge = _trainer(grad_clip=1e30)
    for s in range(3):
        _step(huge, batch, s)
    out['huge'] = huge

    mon = _trainer(grad_norms=True)
    p0 = mon.optimizer.fp.flat.clone()
    _step(mon, batch, 0)
    out['mon_first'] = (p0, mon.optimizer.fp.grad.clone(), list(mon.optimizer.steps), mon.grad_stats())
    for s in (1, 2):
        _step(mon, batch, s)
    out['mon'] = mon

    n0 = out['mon_first'][3]['g']['norm']
    half = _trainer(grad_clip={'g': n0 / 2})
    _step(half, batch, 0)
    out['half'] = half

    nan = _trainer(grad_norms=True)
    calls = []

    def plant():
        calls.append(1)
        if len(calls) == 2:
            nan.optimizer.fp.grad[nan.optimizer.fp.offsets[-1]] = float('nan')
    nan.optimizer.pre_step_hooks.append(plant)
    states, d_states, stats = [], [], []
    for s in range(3):
        _step(nan, batch, s)
        states.append(_g_state(nan))
        d_states.append([f.clone() for f in _flats(nan)[1:]])
        stats.append(nan.grad_stats())
    out['nan'] = (nan, states, d_states, stats)
    return out


@pytest.mark.parametrize('name', ['huge', 'mon'])
def test_trainer_control_keeps_training_bitwise(runs, name):
    tr, plain = runs[name], runs['plain']
    for a, b in zip(_flats(tr), _flats(plain)):
        assert torch.equal(a, b)
    for (_, o), (_, q) in zip(tr.named_optimizers(), plain.named_optimizers()):
        assert torch.equal(o.exp_avg, q.exp_avg) and torch.equal(o.exp_avg_sq, q.exp_avg_sq)
    stats = tr.grad_stats()
    assert sorted(stats) == ['d_img', 'd_mask', 'd_obj', 'g']
    for st in stats.values():
        assert (st['coef'], st['skip'], st['skipped'], st['steps']) == (1.0, 0, 0, 3) and 0.0 < st['norm'] < float('inf')


def test_trainer_clipping_is_the_scaled_step(runs):
    p0, grad, steps, first = runs['mon_first']
    half = runs['half']
    n0 = first['g']['norm']
    assert [n for n, o in half.named_optimizers() if o.grad_control] == ['g']
    rec = ops.grad_ctl_read(half.optimizer._gctl)
    want = R.from_sumsq(rec['sumsq'], 1.0, n0 / 2)
    assert rec['norm'] == n0 and rec['coef'] == want['coef'] and abs(rec['coef'] - 0.5) < 1e-3
    assert half.grad_stats()['g']['coef'] == rec['coef']
    assert torch.equal(half.optimizer.fp.grad, grad) and half.optimizer.steps == steps
    # the replay: the twin's gradient through the plain kernel with grad_scale = coef, over the parameters the step touched
    o = half.optimizer
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for i, j, active in optim.step_runs([s == 1 for s in steps], [0] * len(steps)):
        if active:
            lo, hi = o.fp.offsets[i], o.fp.offsets[j] + o.fp.params[j].numel()
            ops.adam_step(p[lo:hi], grad[lo:hi], m[lo:hi], v[lo:hi], o.lr, o.betas[0], o.betas[1], o.eps, 1, rec['coef'])
    torch.cuda.synchronize()
    assert any(s == 1 for s in steps)
    assert torch.equal(o.fp.flat, p) and torch.equal(o.exp_avg, m) and torch.equal(o.exp_avg_sq, v)
    assert not torch.equal(o.fp.flat, p0)
    # the discriminators took the plain step
    assert not torch.equal(o.fp.flat, runs['plain'].optimizer.fp.flat)


def test_trainer_skips_a_non_finite_generator_step(runs):
    nan, states, d_states, stats = runs['nan']
    for a, b in zip(states[1], states[0]):            # parameters and both moments after step 2 are those after step 1
        assert torch.equal(a, b)
    assert [st['g']['skipped'] for st in stats] == [0, 1, 1] and [st['g']['skip'] for st in stats] == [0, 1, 0]
    assert math.isnan(stats[1]['g']['norm']) and stats[1]['g']['coef'] == 1.0 and stats[2]['g']['steps'] == 3
    # step 3 trains again
    assert not torch.equal(states[2][0], states[1][0]) and all(bool(torch.isfinite(t).all()) for t in states[2])
    assert math.isfinite(stats[2]['g']['norm'])
    # the discriminators never noticed: after step 2 they are the plain Trainer's
    for a, b in zip(d_states[1], runs['plain_d_after'][1]):
        assert torch.equal(a, b)
    for name in ('d_obj', 'd_mask', 'd_img'):
        assert stats[2][name]['skipped'] == 0 and stats[2][name]['steps'] == 3


def test_write_losses(runs, capsys):
    mon, plain = runs['mon'], runs['plain']
    ck = {}
    mon.write_losses(ck, 10)
    out = capsys.readouterr().out
    stats = mon.grad_stats()
    assert ck['norm_g'] == [stats['g']['norm']] and ck['norm_g'][0] > 0
    assert ck['norm_d'] == [{n: stats[n]['norm'] for n in ('d_obj', 'd_mask', 'd_img')}]
    assert all(' %s [grad_norm]' % n in out for n in stats) and 'skipped' not in out
    ck_plain = {}
    plain.write_losses(ck_plain, 10)
    assert 'grad_norm' not in capsys.readouterr().out
    assert set(ck) - set(ck_plain) == {'norm_g', 'norm_d'}
    nan = runs['nan'][0]
    nan.write_losses(None, 10)
    assert ' g [skipped]: 1 of 3 steps' in capsys.readouterr().out
