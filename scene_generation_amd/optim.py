"""Flat-buffer Adam for MI355X.

All parameters of one optimiser live in ONE contiguous fp32 buffer (parameters become views into it), and so do
their gradients and both Adam moments.  Consequences:
  * optimizer.step()      = one HIP launch over 28 B/param of HBM traffic (sg_adam_step)
  * optimizer.zero_grad() = one fill launch -- or none (``lazy_zero``: the first contribution of a step overwrites its slice)
  * data-parallel reduce  = a handful of large RCCL all-reduces over slices of the flat gradient buffer
    (scene_generation_amd.parallel) instead of one small collective per tensor.
``state_dict()`` / ``load_state_dict()`` speak torch.optim.Adam's schema (trainer.py:138,186), so reference
checkpoints round-trip.

Optional: an exponential moving average of the parameters (``ParamEMA``, ``FusedAdam.attach_ema``) in a shadow buffer with the
flat buffer's layout, updated inside the same launch (sg_adam_step_ema: 36 instead of 28 B/param, no second pass).

Optional: global-norm clipping and a skip-on-non-finite guard (``FusedAdam.set_grad_control``, SG_GRAD_CLIP / SG_GRAD_NORMS): one
more read of the flat gradient (sg_grad_norm, 4 B/param) leaves norm, clip coefficient and skip flag in a device record the Adam
launch reads (sg_adam_step_ctl) -- no host synchronisation, no pass over parameters or moments.

``FusedSGD`` (at the end) is the same idea for torch.optim.SGD with momentum, the optimiser of the accuracy network.
"""
import os

import torch

from . import ops, streams

# what the Trainer passes as FusedAdam(lazy_zero=...): SG_LAZY_ZERO=0 restores the fill launch of every zero_grad() (A/B switch)
LAZY_ZERO = os.environ.get('SG_LAZY_ZERO', '1') == '1'


class FlatParams:
    """Re-homes ``params`` into one flat buffer (+ a flat gradient buffer).  Device-agnostic host logic."""
    ALIGN = 64          # elements

    def __init__(self, params):
        self.params = [p for p in params]
        assert self.params, 'no parameters'
        dev, dt = self.params[0].device, self.params[0].dtype
        assert all(p.device == dev and p.dtype == dt for p in self.params)
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            # 256-byte aligned slices: the conv kernels read weights with 16-byte vector loads only when aligned
            off += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.numel = off
        self.flat = torch.zeros(off, dtype=dt, device=dev)     # alignment gaps stay zero under Adam (zero gradient)
        self.grad = torch.zeros(off, dtype=dt, device=dev)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                self.flat[o:o + p.numel()].copy_(p.data.reshape(-1))
                p.data = self.flat[o:o + p.numel()].view(p.shape)
        self.attach_grads()

    def grad_view(self, i):
        p, o = self.params[i], self.offsets[i]
        return self.grad[o:o + p.numel()].view(p.shape)

    def packed(self, buf):
        """``buf`` (the flat parameter / gradient / moment buffer) without the alignment gaps, in parameter order"""
        return torch.cat([buf[o:o + p.numel()] for p, o in zip(self.params, self.offsets)])

    def attach_grads(self):
        """(re)point every p.grad at its slice of the flat buffer; autograd then accumulates IN PLACE."""
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None or g.data_ptr() != self.grad.data_ptr() + self.offsets[i] * self.grad.element_size():
                p.grad = self.grad_view(i)


def step_runs(touched, steps):
    """The launches of one FusedAdam.step(): ``(i, j, active)`` for every maximal run of parameters i..j, in order, covering all of
    them.  Active runs are touched parameters that share a step count (one Adam launch each); inactive runs are untouched
    parameters, which Adam skips (one EMA launch each when an EMA is attached)."""
    runs, i, n = [], 0, len(touched)
    while i < n:
        j = i
        if touched[i]:
            while j + 1 < n and touched[j + 1] and steps[j + 1] == steps[i]:
                j += 1
        else:
            while j + 1 < n and not touched[j + 1]:
                j += 1
        runs.append((i, j, bool(touched[i])))
        i = j + 1
    return runs


def ema_decay_from_env(environ=None):
    """SG_G_EMA_DECAY: the decay of the generator's parameter EMA when a Trainer is built without ``ema_decay``.  Unset or empty:
    None (no EMA); otherwise a float in (0, 1), anything else raises ValueError."""
    v = (os.environ if environ is None else environ).get('SG_G_EMA_DECAY', '')
    if v == '':
        return None
    return check_ema_decay(v, 'SG_G_EMA_DECAY=%r' % v)


def check_ema_decay(value, what='ema_decay'):
    try:
        d = float(value)
    except (TypeError, ValueError):
        raise ValueError('%s: expected a float in (0, 1)' % what)
    if not 0.0 < d < 1.0:              # (also rejects nan)
        raise ValueError('%s: expected a float in (0, 1), got %r' % (what, d))
    return d


GRAD_CLIP_NAMES = ('g', 'd_obj', 'd_mask', 'd_img')       # the Trainer's four optimisers, as SG_GRAD_CLIP and grad_clip= name them


def check_max_norm(value, what='max_norm'):
    try:
        m = float(value)
    except (TypeError, ValueError):
        raise ValueError('%s: expected a positive finite float' % what)
    if not 0.0 < m < float('inf'):      # (also rejects nan)
        raise ValueError('%s: expected a positive finite float, got %r' % (what, m))
    return m


def check_grad_clip(value, what='grad_clip'):
    """-> {name: max_norm} over (a subset of) GRAD_CLIP_NAMES.  ``value``: a number (all four optimisers), a dict over the names,
    or the spelling of SG_GRAD_CLIP: ``'10'`` or ``'g=10,d_img=5'``.  Unknown names, values that are not positive and finite,
    and anything else raise ValueError."""
    if isinstance(value, str):
        parts = [s.strip() for s in value.split(',')]
        if len(parts) == 1 and '=' not in parts[0]:
            value = parts[0]
        else:
            d = {}
            for s in parts:
                name, eq, v = s.partition('=')
                if not eq or name.strip() in d:
                    raise ValueError('%s: expected a float or name=float[,name=float...], got %r' % (what, value))
                d[name.strip()] = v.strip()
            value = d
    if isinstance(value, dict):
        out = {}
        for name, v in value.items():
            if name not in GRAD_CLIP_NAMES:
                raise ValueError('%s: unknown optimiser %r (expected one of %s)' % (what, name, ', '.join(GRAD_CLIP_NAMES)))
            out[name] = check_max_norm(v, '%s[%s]' % (what, name))
        if not out:
            raise ValueError('%s: empty' % what)
        return out
    m = check_max_norm(value, what)
    return {name: m for name in GRAD_CLIP_NAMES}


def grad_clip_from_env(environ=None):
    """SG_GRAD_CLIP: the clipping thresholds when a Trainer is built without ``grad_clip``.  Unset or empty: None (no clipping);
    ``10``: every optimiser; ``g=10,d_img=5``: the named ones; anything else raises ValueError (check_grad_clip)."""
    v = (os.environ if environ is None else environ).get('SG_GRAD_CLIP', '')
    if v.strip() == '':
        return None
    return check_grad_clip(v, 'SG_GRAD_CLIP=%r' % v)


def grad_norms_from_env(environ=None):
    """SG_GRAD_NORMS=1: gradient norms and the non-finite guard on every optimiser, without clipping.  Unset, empty or 0: off."""
    v = (os.environ if environ is None else environ).get('SG_GRAD_NORMS', '').strip()
    if v in ('', '0'):
        return False
    if v == '1':
        return True
    raise ValueError('SG_GRAD_NORMS=%r: expected 0 or 1' % v)


class ParamEMA:
    """Exponential moving average of the parameters of one ``FlatParams``: ``flat`` has the flat buffer's offsets and (zero)
    alignment gaps and starts as a copy of it.  Update ``k`` (0-based) moves every parameter by

        e = e + w_k * (p - e),   w_k = 1 if k < start (the average copies the weights) else 1 - decay

    (sg_adam_step_ema / sg_ema_update: one fmaf; w = 1 is an exact copy).  Attached to a FusedAdam (``attach_ema``), every step()
    is one update, fused into its Adam launches; ``update()`` is the standalone form for callers without Adam.
    ``state_dict()`` holds the schedule ({'decay', 'start', 'updates'}); the averaged values are ``flat`` itself."""

    def __init__(self, flat_params, decay, start=0):
        self.fp = flat_params
        self.decay = check_ema_decay(decay)
        self.start = int(start)
        if self.start < 0:
            raise ValueError('ParamEMA: start must be >= 0, got %d' % self.start)
        self.updates = 0
        self.flat = flat_params.flat.detach().clone()

    def weight(self, k=None):
        """the lerp weight of update ``k`` (default: the next one)"""
        k = self.updates if k is None else k
        return 1.0 if k < self.start else 1.0 - self.decay

    def update(self):
        """one update of the whole buffer toward the current parameters, on the current stream"""
        ops.ema_update(self.flat, self.fp.flat, self.weight())
        self.updates += 1

    def reset(self):
        """the average becomes a copy of the current parameters (the schedule is kept)"""
        with torch.no_grad():
            self.flat.copy_(self.fp.flat)

    def param_view(self, i):
        p, o = self.fp.params[i], self.fp.offsets[i]
        return self.flat[o:o + p.numel()].view(p.shape)

    def state_dict(self):
        return {'decay': self.decay, 'start': self.start, 'updates': self.updates}

    def load_state_dict(self, sd):
        self.decay = check_ema_decay(sd['decay'])
        self.start = int(sd['start'])
        self.updates = int(sd['updates'])


class FusedAdam:
    """torch.optim.Adam(params, lr, betas, eps, weight_decay=0, amsgrad=False) semantics on flat buffers.

    Like torch, a parameter that received NO gradient since the last zero_grad() is skipped entirely (no moment
    decay, no update, its step count does not advance) -- e.g. ``box_net`` in iterations with ``use_gt == False``
    (trainer.py:210-216).  "Received a gradient" is tracked with post-accumulate-grad hooks; step() launches the fused
    kernel once per maximal run of adjacent active parameters that share a step count (normally one launch)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, direct_grads=True, lazy_zero=False):
        self.fp = FlatParams(params)
        # lazy_zero (device buffers with gradient sinks only; the Trainer's four optimisers): zero_grad() does NOT fill the flat
        # gradient buffer (730 MB for the generator: 0.13 ms of HBM time per step).  Every backward kernel OVERWRITES the slice of
        # a parameter's first contribution (ops.GradOut mode 0) and Adam skips untouched parameters, so the fill only ever
        # mattered for parameters that receive nothing: their slices are zeroed when the first backward after zero_grad() ends
        # (or at step() / a reducer's wait()), whichever comes first.  Between zero_grad() and that point ``p.grad`` is None --
        # torch's ``set_to_none=True`` behaviour -- so a gradient autograd itself produces is assigned, never added to stale data.
        self.lazy_zero = bool(lazy_zero) and bool(direct_grads) and self.fp.flat.is_cuda
        self._stale, self._finalize_queued = False, False
        self._views = [self.fp.grad_view(i) for i in range(len(self.fp.params))] if self.lazy_zero else None
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.exp_avg = torch.zeros_like(self.fp.flat)
        self.exp_avg_sq = torch.zeros_like(self.fp.flat)
        n = len(self.fp.params)
        self.steps = [0] * n
        self._touched = [False] * n
        # spill buffers: gradient contributions 2, 3, ... a parameter receives between zero_grad() and step() (ops.GradOut),
        # same layout as the gradient buffer, all-zero outside a step
        self._contrib = [0] * n
        self._spill, self._spill_used, self._fold_queued = [], 0, False
        self._spill_k, self._spill_dirty = [0] * n, False     # per parameter: spilled contributions since the last fold
        # False: later contributions are added into the gradient slice at once (temporary + axpy).  A reducer that sends
        # buckets to the all-reduce DURING the backward needs that: a spilled contribution only reaches the slice when the
        # backward ends, after the bucket may have left (parallel.GradReducer(overlap=True), Trainer)
        self.use_spill = True
        # the gradient enters the update as grad * grad_scale; a data-parallel reducer whose all-reduce SUMs sets 1 / world for
        # the step that follows (GradReducer.wait(defer_scale=True)) instead of scaling the flat buffer in place: after such a
        # step() ``p.grad`` holds the sum over ranks, not the mean.  Reset to 1 by step().
        self.grad_scale = 1.0
        # side-stream groups (streams.py) whose kernels never write this optimiser's buffers: not waited for in zero_grad() /
        # step() (the Trainer's discriminator optimisers: ('front',) -- the generator's object front runs beside their steps)
        self.join_exclude = ()
        self.ema = None                   # ParamEMA updated by every step() (attach_ema)
        self.max_norm, self._gctl, self._gctl_ws = None, None, None      # gradient control (set_grad_control)
        self.pre_step_hooks = []          # e.g. GradReducer.wait
        self.zero_grad_hooks = []         # e.g. GradReducer.begin_step
        self.grad_listeners = []          # callables(i): parameter i just received (a contribution to) its gradient
        self.late_listeners = []          # callables(i): parameter i is ABOUT to receive a second contribution this step
        for i, p in enumerate(self.fp.params):
            p.register_post_accumulate_grad_hook(self._make_hook(i))
        if direct_grads and self.fp.flat.is_cuda:
            # backward kernels write parameter gradients straight into the flat buffer (ops.ParamSink) instead of
            # returning a tensor that autograd then adds into it with one ATen launch per parameter
            ops.register_param_sinks(self)

    def _make_hook(self, i):
        def hook(param):
            if self._stale:
                # lazy_zero: autograd ASSIGNED this gradient (p.grad was None): move it into the parameter's slice
                g, view = param.grad, self._views[i]
                if g is not None and g.data_ptr() != view.data_ptr():
                    if self._touched[i]:
                        view.add_(g)
                    else:
                        view.copy_(g)
                    param.grad = view
            self._on_grad(i)
        return hook

    def _on_grad(self, i):
        self._touched[i] = True
        self._contrib[i] += 1
        if self._stale and not self._finalize_queued:
            # p.grad is complete (untouched slices zero, every p.grad attached) as soon as the running ``.backward()`` returns
            try:
                from torch.autograd import Variable
                Variable._execution_engine.queue_callback(self.finalize_grads)
                self._finalize_queued = True
            except RuntimeError:                   # not inside a backward (a caller writing gradients by hand): step() finalizes
                pass
        for f in self.grad_listeners:
            f(i)

    def spill_view(self, i):
        """where the NEXT contribution to parameter ``i`` (which already has at least one) is written.  Only valid while a
        backward is running (ops.GradOut calls it from inside autograd Functions).  The index counts contributions since the
        last FOLD (every backward folds and clears the buffers when it ends), not since the last zero_grad(): gradient
        accumulation over micro-batches re-uses spill buffer 0 instead of growing one buffer per backward."""
        k = self._spill_k[i]
        self._spill_k[i] = k + 1
        self._spill_dirty = True
        while len(self._spill) <= k:
            self._new_spill_buffer()
        self._spill_used = max(self._spill_used, k + 1)
        if not self._fold_queued:
            # fold when the backward that is running right now ends: ``p.grad`` is complete as soon as ``.backward()`` returns
            # (gradient clipping, logging between backward and step see what torch would show them)
            from torch.autograd import Variable
            self._fold_queued = True
            Variable._execution_engine.queue_callback(self._fold_spill)
        p, o = self.fp.params[i], self.fp.offsets[i]
        return self._spill[k][o:o + p.numel()].view(p.shape)

    def finalize_grads(self):
        """lazy_zero: zero the slices of the parameters that received nothing since zero_grad() and re-attach every ``p.grad``.
        Idempotent; runs at the end of the first backward after zero_grad(), from step() and from GradReducer.wait()."""
        self._finalize_queued = False
        if not self._stale:
            return
        self._stale = False
        fp, t = self.fp, self._touched
        i, n = 0, len(fp.params)
        while i < n:
            if t[i]:
                i += 1
                continue
            j = i
            while j + 1 < n and not t[j + 1]:
                j += 1
            ops.fill_(fp.grad[fp.offsets[i]:fp.offsets[j] + fp.params[j].numel()], 0.0)
            i = j + 1
        for p, v in zip(fp.params, self._views):
            if p.grad is not v:
                p.grad = v

    def _new_spill_buffer(self):
        """A zeroed buffer that kernels of ANY stream may write slices of behind autograd's back.  With side streams on
        (streams.py) a zero fill still in flight on the allocating stream could wipe a slice another stream has already
        written, so the fill is completed before the buffer is handed out: one host synchronisation per buffer
        per optimiser, in the first step only (the buffers live as long as the optimiser)."""
        buf = torch.zeros_like(self.fp.grad)
        if (streams.ENABLED or streams.GROUPS) and buf.is_cuda:
            torch.cuda.current_stream(buf.device).synchronize()
        self._spill.append(buf)

    def _fold_spill(self):
        """grad = ((grad + spill[0]) + spill[1]) + ...: the order the per-parameter adds had; clears the spill buffers.
        Runs as an end-of-backward callback (and from step()): weight-gradient kernels of side streams write the gradient and
        spill slices behind autograd's back, so the reader joins them first (streams.py's rule for these buffers)."""
        self._fold_queued = False
        if self._spill_used:
            streams.join_all(self.fp.grad.device, self.join_exclude)
        for k in range(self._spill_used):
            ops.add_clear_(self.fp.grad, self._spill[k])
        self._spill_used = 0
        if self._spill_dirty:
            self._spill_k = [0] * len(self.fp.params)
            self._spill_dirty = False

    def attach_ema(self, ema):
        """Update ``ema`` (a ParamEMA of this optimiser's parameters) in every step(): each Adam launch becomes the fused Adam + EMA
        launch, and each run of parameters Adam skips gets one sg_ema_update, so every parameter moves once per step().  The Adam
        results are bitwise unchanged."""
        if ema is not None and (ema.fp is not self.fp or ema.flat.shape != self.fp.flat.shape):
            raise ValueError('attach_ema: the EMA must be built over this optimiser\'s FlatParams')
        self.ema = ema

    def set_grad_control(self, max_norm=None, monitor=True):
        """Global-norm clipping and a skip-on-non-finite guard for every step() that follows, decided on the device.

        With the control on, step() reads the flat gradient once more (sg_grad_norm, 4 B per parameter, after the spill fold, the
        lazy-zero finalisation and every pre_step hook, so it sees the reduced gradient and the deferred 1 / world in
        ``grad_scale``) and leaves norm = |grad_scale| * ||grad||_2, coef = min(1, max_norm / (norm + 1e-6)) -- the factor of
        torch.nn.utils.clip_grad_norm_ -- and a skip flag in a 32-byte device record; the Adam launches take the gradient as
        grad * (grad_scale * coef) and write nothing when the norm is not finite (an attached EMA still moves toward the unchanged
        weights).  No host synchronisation, no pass over parameters or moments, no temporary.  ``max_norm=None``: norms and the
        guard only (coef = 1: the bits of a step without the control, as long as no step is skipped).
        ``set_grad_control(None, False)`` switches it off: step() issues the plain launches again.

        Unlike torch's in-place clip ``p.grad`` is left as the backward wrote it (``scaled_grad()`` too).  Unlike a
        GradScaler-style skip the HOST step counts advance on a skipped step (the decision never reaches the host): the bias
        corrections of later steps are those of one step more, nothing else changes.

        The record and the partials buffer are allocated here, once, on the optimiser's device -- not from ``ops.workspace()``,
        which is per stream and hands out temporaries inside captures."""
        if max_norm is None and not monitor:
            self.max_norm, self._gctl, self._gctl_ws = None, None, None
            return
        self.max_norm = None if max_norm is None else check_max_norm(max_norm)
        if self._gctl is None:
            self._gctl, self._gctl_ws = ops.grad_ctl_alloc(self.fp.flat.device)

    @property
    def grad_control(self):
        return self._gctl is not None

    def grad_stats(self):
        """{'norm', 'coef', 'skip', 'skipped', 'steps'} of the last step() under set_grad_control (``skipped`` / ``steps``: counts
        since it was switched on); None with the control off.  One 32-byte device-to-host copy on the current stream: the only
        call of the gradient control that synchronises."""
        if self._gctl is None:
            return None
        rec = ops.grad_ctl_read(self._gctl)
        return {k: rec[k] for k in ('norm', 'coef', 'skip', 'skipped', 'steps')}

    @property
    def step_count(self):
        return max(self.steps) if self.steps else 0

    @property
    def param_groups(self):
        return [dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=0, amsgrad=False,
                     params=self.fp.params)]

    def zero_grad(self, set_to_none=False):
        streams.join_all(self.fp.grad.device, self.join_exclude)      # weight-gradient kernels of side streams write this buffer (streams.py)
        if self._spill_used:                        # contributions of a backward whose step never came: dropped with the rest
            for k in range(self._spill_used):
                ops.fill_(self._spill[k], 0.0)
            self._spill_used = 0
        if self.lazy_zero:
            self._stale, self._finalize_queued = True, False
            for p in self.fp.params:
                p.grad = None
        else:
            ops.fill_(self.fp.grad, 0.0)
            self.fp.attach_grads()
        self._touched = [False] * len(self.fp.params)
        self._contrib = [0] * len(self.fp.params)
        self._spill_k, self._spill_dirty = [0] * len(self.fp.params), False
        # a deferred 1 / world belongs to the gradients just cleared (a wait(defer_scale=True) whose step() never came, or a
        # step() that raised): it must not leak into the next step, which may run without a reduce
        self.grad_scale = 1.0
        for h in self.zero_grad_hooks:
            h()

    def mark_all_touched(self):
        """for callers that write gradients directly into the flat buffer (tests, custom reducers)"""
        self._touched = [True] * len(self.fp.params)
        self.finalize_grads()

    def scaled_grad(self, i=None):
        """The gradient the coming step() will apply -- ``grad * grad_scale`` -- of parameter ``i`` (None: the whole flat buffer),
        as a new tensor.  After a data-parallel reduce with a deferred scale (GradReducer.wait(defer_scale=True)) ``p.grad`` holds
        the SUM over ranks and ``grad_scale`` the 1 / world; a pre_step hook registered after the reducer's (gradient clipping,
        norm logging) reads the mean through this helper instead of the raw buffer."""
        self.finalize_grads()
        g = self.fp.grad if i is None else self.fp.grad_view(i)
        return g * self.grad_scale if self.grad_scale != 1.0 else g.clone()

    def step(self):
        try:
            streams.join_all(self.fp.grad.device, self.join_exclude)      # (see zero_grad)
            self._fold_spill()
            self.finalize_grads()
            for h in self.pre_step_hooks:
                h()
            self.fp.attach_grads()
            fp, ema = self.fp, self.ema
            w = ema.weight() if ema is not None else None
            ctl = self._gctl
            if ctl is not None:
                # the whole flat buffer: untouched slices and alignment gaps are zero here (finalize_grads; FlatParams)
                ops.grad_norm(fp.grad, ctl, self._gctl_ws, self.grad_scale, self.max_norm or 0.0)
            for i, j, active in step_runs(self._touched, self.steps):
                lo, hi = fp.offsets[i], fp.offsets[j] + fp.params[j].numel()
                if not active:
                    if ema is not None:        # skipped by Adam (no gradient), but the average still moves toward the weights
                        ops.ema_update(ema.flat[lo:hi], fp.flat[lo:hi], w)
                    continue
                st = self.steps[i]
                if ctl is not None:            # (the host counts advance also when the device skips the step: set_grad_control)
                    if ema is not None:
                        ops.adam_step_ema_ctl(fp.flat[lo:hi], fp.grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi],
                                              ema.flat[lo:hi], ctl, self.lr, self.betas[0], self.betas[1], self.eps, st + 1,
                                              self.grad_scale, w)
                    else:
                        ops.adam_step_ctl(fp.flat[lo:hi], fp.grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], ctl,
                                          self.lr, self.betas[0], self.betas[1], self.eps, st + 1, self.grad_scale)
                elif ema is not None:
                    ops.adam_step_ema(fp.flat[lo:hi], fp.grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], ema.flat[lo:hi],
                                      self.lr, self.betas[0], self.betas[1], self.eps, st + 1, self.grad_scale, w)
                else:
                    ops.adam_step(fp.flat[lo:hi], fp.grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], self.lr,
                                  self.betas[0], self.betas[1], self.eps, st + 1, self.grad_scale)
                for q in range(i, j + 1):
                    self.steps[q] = st + 1
            if ema is not None:
                ema.updates += 1
        finally:
            self.grad_scale = 1.0          # also when a hook or a launch raised: the scale never outlives its step

    # ---- torch.optim.Adam-compatible (de)serialisation ----
    def state_dict(self):
        state = {}
        for i, (p, o) in enumerate(zip(self.fp.params, self.fp.offsets)):
            if self.steps[i] == 0:
                continue
            n = p.numel()
            state[i] = {'step': torch.tensor(float(self.steps[i])),
                        'exp_avg': self.exp_avg[o:o + n].view(p.shape).clone(),
                        'exp_avg_sq': self.exp_avg_sq[o:o + n].view(p.shape).clone()}
        group = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=0, amsgrad=False, maximize=False,
                     foreach=None, capturable=False, differentiable=False, fused=None,
                     params=list(range(len(self.fp.params))))
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        g = sd['param_groups'][0]
        self.lr, self.betas, self.eps = float(g['lr']), tuple(float(b) for b in g['betas']), float(g['eps'])
        with torch.no_grad():
            for i, (p, o) in enumerate(zip(self.fp.params, self.fp.offsets)):
                st = sd['state'].get(i)
                n = p.numel()
                if st is None:
                    self.steps[i] = 0
                    self.exp_avg[o:o + n].zero_()
                    self.exp_avg_sq[o:o + n].zero_()
                    continue
                self.exp_avg[o:o + n].copy_(st['exp_avg'].reshape(-1))
                self.exp_avg_sq[o:o + n].copy_(st['exp_avg_sq'].reshape(-1))
                self.steps[i] = int(float(st['step']))


def _increment_version(p):
    """mark ``p`` as written (its version counter moves): a kernel wrote it behind torch's back.  torch.autograd.graph's
    increment_version where it exists; else an in-place no-op through torch, which bumps the counter like any write"""
    inc = getattr(getattr(torch.autograd, 'graph', None), 'increment_version', None)
    if inc is not None:
        inc(p)
    else:
        with torch.no_grad():
            p.add_(0)


class FusedSGD:
    """torch.optim.SGD(params, lr, momentum) semantics (no dampening, Nesterov or weight decay: scripts/train_accuracy_net.py:265)
    on flat buffers: the parameters that require gradients, their gradients and the momentum buffer each live in ONE contiguous
    fp32 buffer (FlatParams), so step() is one launch (sg_sgd_momentum_step, 20 B per parameter) and zero_grad() one fill.

    ``param_groups[0]['lr']`` (and ``['momentum']``) are read by every step(), so a StepLR-style schedule that writes them works.
    Unlike torch, a parameter that received no gradient since zero_grad() is stepped with a zero gradient (its momentum keeps
    moving it); every trainable parameter of the accuracy network receives one in every step.  ``state_dict()`` /
    ``load_state_dict()`` speak torch.optim.SGD's schema (``momentum_buffer``)."""

    def __init__(self, params, lr=1e-3, momentum=0.0, direct_grads=True):
        params = [p for p in params if p.requires_grad]
        self.fp = FlatParams(params)
        self.momentum_buffer = torch.zeros_like(self.fp.flat)
        self.param_groups = [dict(lr=float(lr), momentum=float(momentum), dampening=0, weight_decay=0, nesterov=False,
                                  maximize=False, foreach=None, differentiable=False, fused=None, params=self.fp.params)]
        self.steps = 0
        self.grad_scale = 1.0             # the gradient enters the update as grad * grad_scale; reset to 1 by step()
        n = len(self.fp.params)
        self._touched = [False] * n
        self.use_spill = False            # a second contribution to a parameter is added at once (ops.GradOut mode 1)
        for i, p in enumerate(self.fp.params):
            p.register_post_accumulate_grad_hook(self._make_hook(i))
        if direct_grads and self.fp.flat.is_cuda:
            ops.register_param_sinks(self)      # weight-gradient kernels write straight into the flat gradient buffer

    def _make_hook(self, i):
        def hook(param):
            self._on_grad(i)
        return hook

    def _on_grad(self, i):
        self._touched[i] = True

    @property
    def lr(self):
        return float(self.param_groups[0]['lr'])

    def zero_grad(self, set_to_none=False):
        if set_to_none:
            raise NotImplementedError('FusedSGD keeps every gradient in its flat buffer: zero_grad() fills it with zeros')
        if self.fp.grad.is_cuda:
            ops.fill_(self.fp.grad, 0.0)
        else:
            self.fp.grad.zero_()
        self.fp.attach_grads()
        self._touched = [False] * len(self.fp.params)
        self.grad_scale = 1.0

    def step(self):
        try:
            self.fp.attach_grads()
            g = self.param_groups[0]
            ops.sgd_momentum_step(self.fp.flat, self.fp.grad, self.momentum_buffer, g['lr'], g['momentum'], self.steps == 0,
                                  self.grad_scale)
            self.steps += 1
            for p in self.fp.params:      # the kernel wrote the parameters behind torch's back: let version-keyed caches
                _increment_version(p)     # (the accuracy network's folded BatchNorm weights) see the write
        finally:
            self.grad_scale = 1.0

    def state_dict(self):
        state = {}
        if self.steps > 0:
            for i, (p, o) in enumerate(zip(self.fp.params, self.fp.offsets)):
                state[i] = {'momentum_buffer': self.momentum_buffer[o:o + p.numel()].view(p.shape).clone()}
        group = {k: v for k, v in self.param_groups[0].items() if k != 'params'}
        group['params'] = list(range(len(self.fp.params)))
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        g = sd['param_groups'][0]
        self.param_groups[0]['lr'] = float(g['lr'])
        self.param_groups[0]['momentum'] = float(g['momentum'])
        have = [sd['state'].get(i) for i in range(len(self.fp.params))]
        have = [None if st is None else st.get('momentum_buffer') for st in have]
        with torch.no_grad():
            self.momentum_buffer.zero_()
            for (p, o), buf in zip(zip(self.fp.params, self.fp.offsets), have):
                if buf is not None:
                    self.momentum_buffer[o:o + p.numel()].copy_(buf.reshape(-1))
        self.steps = 1 if any(b is not None for b in have) else 0
