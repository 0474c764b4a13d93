"""Float64 restatement of the gradient-control record (include/sg2im_hip.h: sgGradCtl) and of the step it steers, shared by
tests/test_gradctl_cpu.py (against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam) and tests/test_gpu_gradctl.py (against
sg_grad_norm / sg_adam_step_ctl).  Host arithmetic only."""
import math

import numpy as np
import torch


def f32(x):
    return float(np.float32(x))


def record(g, grad_scale=1.0, max_norm=0.0):
    """{'sumsq', 'norm_d', 'norm', 'coef', 'skip'} of the flat fp32 gradient ``g``: the squares summed in float64 (math.fsum: the
    exact sum rounded once), norm = |fp32(grad_scale)| * sqrt(sumsq) in float64 and rounded to fp32 once,
    coef = fp32(min(1, max_norm / (norm_double + 1e-6))) -- 1 for max_norm <= 0 or inf, and for a non-finite norm, which sets skip."""
    x = g.detach().double().cpu().reshape(-1).numpy()
    with np.errstate(over='ignore', invalid='ignore'):
        sq = x * x
        sumsq = math.fsum(sq.tolist()) if bool(np.isfinite(sq).all()) else float(sq.sum())
    out = from_sumsq(sumsq, grad_scale, max_norm)
    out['sumsq'] = sumsq
    return out


def from_sumsq(sumsq, grad_scale=1.0, max_norm=0.0):
    """the record's norm / coef / skip from a sum of squares, each operation rounded once in float64"""
    with np.errstate(over='ignore', invalid='ignore'):
        norm_d = float(np.float64(abs(f32(grad_scale))) * np.sqrt(np.float64(sumsq)))
        norm = float(np.float32(norm_d))
    skip = 0 if math.isfinite(norm) else 1
    coef = 1.0
    if not skip and max_norm > 0 and math.isfinite(max_norm):
        coef = f32(min(1.0, f32(max_norm) / (norm_d + 1e-6)))
    return {'norm_d': norm_d, 'norm': norm, 'coef': coef, 'skip': skip}


class RefAdam:
    """torch.optim.Adam (no weight decay / amsgrad) in float64 over a list of tensors, the gradient entering as
    g * fp32(grad_scale * coef); a set skip flag leaves everything alone except the step count (FusedAdam.set_grad_control)."""

    def __init__(self, params, lr, betas, eps=1e-8):
        self.p = [p.detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.lr, self.b1, self.b2, self.eps, self.t = lr, betas[0], betas[1], eps, 0
        self.records = []

    def step(self, grads, grad_scale=1.0, max_norm=0.0):
        flat = torch.cat([g.detach().float().reshape(-1) for g in grads])
        rec = record(flat, grad_scale, max_norm)
        self.records.append(rec)
        self.t += 1
        if rec['skip']:
            return rec
        scale = f32(f32(grad_scale) * rec['coef'])
        bc1, bc2 = 1 - self.b1 ** self.t, 1 - self.b2 ** self.t
        for p, m, v, g in zip(self.p, self.m, self.v, grads):
            gi = g.detach().double() * scale
            m.mul_(self.b1).add_(gi, alpha=1 - self.b1)
            v.mul_(self.b2).addcmul_(gi, gi, value=1 - self.b2)
            p.addcdiv_(m, v.sqrt() / math.sqrt(bc2) + self.eps, value=-self.lr / bc1)
        return rec
