"""What the GPU test modules share: comparisons, the margins record, device operands, option handling and the fixtures.  One
copy of each; a family module imports what it needs by name (fixtures included: pytest collects them from the importing module's
namespace) and keeps its own case tables, entry-point wrappers, plan assertions and ``check()``.

Nothing here imports the oracle, the trainer or the argument parser, and the device library is loaded inside the fixtures only:
the comparisons are plain numpy / torch-CPU and tests/test_gpu_harness_cpu.py pins them without a device."""
import contextlib
import ctypes
import json
import os

import numpy as np
import pytest
import torch

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 12345.0         # pre-fill of results and of the words around a workspace
GUARD_WORDS = 256       # more than a tile's rows: a store one tile past the last row of a workspace still lands on a guard word
METRIC_GUARD = -777.0   # the guard / poison value of the metric modules' buffers (-777 in an integer buffer)
_CLOSE_LOG = []         # every relative-L2 ratio close() has seen, from all modules -> close_margins.json (test_gpu_parity.py)
_KEEP = []              # operands placed by the running test: a launch is asynchronous, its inputs must outlive the expression


# =============================================================================================
# comparison
# =============================================================================================
def close(a, b, tol=1e-5, name=''):
    """max|a-b| <= tol * max(1, max|b|)   AND   (an absolute bound scaled by the largest entry lets a
    small-magnitude channel be 100 % wrong) relative-L2 bounds per tensor and per channel:
        ||a - b||_2 <= 20 tol ||b||_2 + 0.25 tol max(1, max|b|) sqrt(n)
    i.e. the rms error of the tensor / of every channel (dim 1 of an (N,C,H,W) map, last dim of a matrix) must be 20 tol
    of that channel's own rms, plus an absolute rms floor four times tighter than the max-error bound (a channel that is the
    result of cancellation cannot be accurate relative to itself).  Calibration: the tightest margins of a full GPU run are
    written to close_margins.json in the suite's output directory (r4: worst 0.39 of the bound, a 4-element bias gradient;
    everything else < 0.15)."""
    a = a.detach().double().cpu()
    b = (torch.from_numpy(np.asarray(b)) if not isinstance(b, torch.Tensor) else b.detach()).double().cpu()
    assert a.shape == b.shape, (name, tuple(a.shape), tuple(b.shape))
    if a.numel() == 0:
        return
    assert torch.isfinite(a).all(), '%s: non-finite values' % name
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())
    assert err <= tol * scale, '%s: max err %.3e (scale %.3e, tol %.1e)' % (name, err, scale, tol)
    d = a - b
    groups = [('tensor', d.reshape(1, -1), b.reshape(1, -1))]
    if a.dim() == 4 and a.size(1) > 1:
        groups.append(('channel', d.transpose(0, 1).reshape(a.size(1), -1), b.transpose(0, 1).reshape(a.size(1), -1)))
    elif a.dim() == 2 and a.size(1) > 1 and a.size(0) > 1:
        groups.append(('column', d.t(), b.t()))
    for kind, dd, bb in groups:
        en, bn, n = dd.norm(dim=1), bb.norm(dim=1), dd.size(1)
        lim = 20 * tol * bn + 0.25 * tol * scale * (n ** 0.5)
        ratio = float((en / lim).max())
        _CLOSE_LOG.append((ratio, kind, name, tol))
        i = int((en / lim).argmax())
        assert ratio <= 1.0, '%s: %s %d relative-L2 error %.3e of |b| %.3e exceeds the bound %.3e (tol %.1e)' % (
            name, kind, i, float(en[i]), float(bn[i]), float(lim[i]), tol)


def _host(a, f64=False):
    """a numpy array or torch tensor (any device) as a numpy array on the host, widened to float64 on request"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64 if f64 else None)


def same(got, want, name=''):
    """value equality, element by element, of numpy arrays or torch tensors; a floating ``want`` is rounded to the dtype of a floating
    ``got`` first (the fp32 expectation of an fp32 result).  Returns True, so ``assert same(a, b), 'why'`` reads."""
    got, want = _host(got), _host(want)
    if got.dtype.kind == 'f':
        want = want.astype(got.dtype)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.equal(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(want))), (
        '%s: %d of %d elements differ from the expectation' % (name, int((got != want).sum()), got.size))
    return True


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b, name):
    assert np.array_equal(bits(a), bits(b)), '%s: %d of %d elements differ' % (name, int((bits(a) != bits(b)).sum()), a.size)


# =============================================================================================
# margins: the worst error / bound ratio per family, one record per module
# =============================================================================================
def _out_dir():
    """the directory next to tests/ that run output goes to: the one *_out/ entry of .gitignore.  No entry, or two different ones,
    is an error here rather than records that silently go nowhere or somewhere else"""
    with open(os.path.join(ROOT, '.gitignore')) as f:
        names = {line.strip().rstrip('/') for line in f if line.strip().endswith('_out/')}
    assert len(names) == 1, '.gitignore must name exactly one output directory (*_out/), it names %s' % sorted(names)
    return os.path.join(ROOT, names.pop())


def _dump(name, obj):
    d = _out_dir()
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name), 'w') as f:
            json.dump(obj, f, indent=1, sort_keys=True)
    except OSError:
        pass


class Margins:
    """family -> (worst ratio, the case that had it), plus ``extra`` entries a module writes as they are"""

    def __init__(self):
        self.worst, self.extra = {}, {}

    def note(self, family, ratio, name):
        ratio = float(ratio)
        if ratio != ratio:              # NaN compares false with everything: it would never replace a finite ratio
            ratio = float('inf')
        if family not in self.worst or ratio > self.worst[family][0]:
            self.worst[family] = (ratio, name)

    def within(self, family, got, ref, bound, name):
        """|got - ref| <= bound element by element (bound 0: equality)"""
        got, ref = _host(got, True), _host(ref, True)
        bound = np.broadcast_to(_host(bound, True), ref.shape)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        if got.size == 0:
            return
        if not np.isfinite(got).all():
            self.note(family, np.inf, name)
        assert np.isfinite(got).all(), '%s: non-finite values' % name
        err = np.abs(got - ref)
        ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
        worst = float(np.where(np.isnan(ratio), np.inf, ratio).max())        # (a NaN reference or bound: no ratio, so the worst)
        print('%s %s: worst error / bound %.3f' % (family, name, worst))
        self.note(family, worst, name)
        i = int(ratio.argmax())
        assert worst <= 1.0, '%s: error %.3e exceeds the rounding bound %.3e (element %d, %.2f of the bound)' % (
            name, err.reshape(-1)[i], bound.reshape(-1)[i], i, worst)

    def close_noted(self, family, a, b, tol, name):
        """close(), with the larger of the max-norm ratio and close()'s own relative-L2 ratios noted"""
        a, b = (torch.from_numpy(np.ascontiguousarray(_host(t, True))) for t in (a, b))
        n0 = len(_CLOSE_LOG)
        ratio = 0.0
        if a.numel() and a.shape == b.shape:
            ratio = float((a - b).abs().max()) / (tol * max(1.0, float(b.abs().max())))
        print('%s %s: max error / bound %.3f' % (family, name, ratio))
        try:
            close(a, b, tol, name)
        finally:
            self.note(family, max([ratio] + [r[0] for r in _CLOSE_LOG[n0:]]), name)

    def yardstick(self, family, name, got, ref64, ref32, factors, factor, floor):
        """|got - ref64| <= factor * max(|ref32 - ref64|, floor * max|ref64|), in max norm over the tensor: the error over the error
        of a float32 run of the same restatement; factor = factors[family], or ``factor`` for a family not in the table"""
        factor = factors.get(family, factor)
        got, ref64, ref32 = [torch.as_tensor(t).detach().double().cpu() for t in (got, ref64, ref32)]
        assert tuple(got.shape) == tuple(ref64.shape), (name, tuple(got.shape), tuple(ref64.shape))
        if not bool(torch.isfinite(got).all()):
            self.note(family, np.inf, name)
        assert bool(torch.isfinite(got).all()), '%s: non-finite values' % name
        scale = float(ref64.abs().max()) or 1.0
        e = float((got - ref64).abs().max()) / scale
        yard = max(float((ref32 - ref64).abs().max()) / scale, floor)
        ratio = e / yard
        self.note(family, ratio, name)
        print('%-10s %-44s err %.3e  fp32 yardstick %.3e  ratio %.3f' % (family, name, e, yard, ratio))
        assert ratio <= factor, '%s: error %.3e is %.1f x the fp32 yardstick %.3e (bound %g x)' % (name, e, ratio, yard, factor)

    def dump(self, filename, key='ratio_of_bound', bound=None, empty=True):
        """-> filename in the suite's output directory: {family: {key: worst, 'case': name[, 'bound': bound(family)]}}.  empty=False:
        a module none of whose recording tests ran writes no file"""
        out = {k: {key: v[0], 'case': v[1]} for k, v in self.worst.items()}
        if bound is not None:
            for k in out:
                out[k]['bound'] = bound(k)
        out.update(self.extra)
        if out or empty:
            _dump(filename, out)

    def dump_yardstick(self, filename, factors, factor):
        """dump() of a module that records with yardstick(): every family with its factor"""
        self.dump(filename, 'ratio_of_fp32_yardstick', lambda k: factors.get(k, factor), empty=False)


# =============================================================================================
# device operands of a C-ABI call
# =============================================================================================
def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dref(d):
    return ctypes.byref(d)


def call(L, name, *args):
    rc = getattr(L, name)(*args)
    assert rc == 0, '%s returned %d: %s' % (name, rc, L.sg_last_error_string().decode())


def place(a, off=0):
    """the fp32 array on the device, ``off`` floats into a buffer of its own (the view keeps the buffer alive)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    base = torch.empty(a.size + 8, dtype=torch.float32, device=DEV)
    assert base.data_ptr() % 16 == 0
    v = base[off:off + max(a.size, 1)]        # (never empty: an empty tensor has no address)
    v[:a.size].copy_(torch.from_numpy(a).reshape(-1))
    _KEEP.append(v)
    return v


def place_fenced(a, off=0):
    """place(), 4 + ``off`` floats into its buffer, with NaN in every float before and behind: a gather that is off by a few elements
    at either end of an input reads a NaN -- which no zero weight hides -- and stays inside the buffer"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    base = torch.full((a.size + 8 + off,), float('nan'), dtype=torch.float32, device=DEV)
    assert base.data_ptr() % 16 == 0
    v = base[4 + off:4 + off + max(a.size, 1)]
    v[:a.size].copy_(torch.from_numpy(a).reshape(-1))
    _KEEP.append(v)
    return v


def outbuf(n, off=0):
    """n floats to be written plus a guard value behind them"""
    base = torch.full((n + off + 1,), GUARD, dtype=torch.float32, device=DEV)
    return base[off:off + n + 1]


def take(o, shape):
    """the result as a numpy array; the guard must be untouched"""
    h = o.cpu().numpy()
    assert h[-1] == GUARD, 'the kernel wrote behind its output'
    return h[:-1].reshape(shape).copy()


def taken(o, shape, name):
    """take(), and no element may have kept the pre-fill"""
    y = take(o, shape)
    assert not (y == GUARD).any(), '%s: %d result elements were never written' % (name, int((y == GUARD).sum()))
    return y


class Workspace:
    """``nbytes`` of scratch that start ``off`` floats behind a 16-byte boundary: ``buf`` (hand it to the launch), NaN over the bytes
    offered -- a slab the launch reads without having written it is a NaN in the result, not a stale value -- and ``guards`` words of
    GUARD behind them (and in the ``off`` floats before).  nan=False, guards=0: plain uninitialised scratch"""

    def __init__(self, nbytes, off=0, guards=GUARD_WORDS, nan=True):
        self.n, self.words, self.off = nbytes, (nbytes + 3) // 4, off
        size = off + self.words + guards + 8
        self.base = torch.empty(size, dtype=torch.float32, device=DEV)
        if guards:
            self.base.fill_(GUARD)
        assert self.base.data_ptr() % 16 == 0
        self.buf = self.base[off:]
        if nan:
            self.buf[:self.words] = float('nan')
        _KEEP.append(self.base)

    def host(self):
        return self.base.cpu().numpy()

    def intact(self, name):
        h = self.host()
        assert (h[:self.off] == GUARD).all() and (h[self.off + self.words:] == GUARD).all(), (
            '%s: the launch wrote outside the workspace bytes it was given' % name)


def scratch(nbytes, off=0):
    """a Workspace without NaN or guards, for entry points whose launches write what they read of it -> its buffer"""
    return Workspace(nbytes, off, guards=0, nan=False).buf


# =============================================================================================
# run shaping
# =============================================================================================
@contextlib.contextmanager
def options(d):
    """the library options of the dict for the block (norm_cases.option each), restored on the way out"""
    from norm_cases import option
    with contextlib.ExitStack() as st:
        for k, v in d.items():
            st.enter_context(option(k, v))
        yield


def opt_tag(o, empty=''):
    return ' '.join('%s=%d' % kv for kv in sorted(o.items())) or empty


def twice(fn, name):
    """fn() -> a tuple; every numpy array in it is bit-identical in a second call"""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y), '%s: a second run differs' % name
    return a


# =============================================================================================
# metric-side placement
# =============================================================================================
def N(t):
    return t.detach().cpu().numpy()


def _place(x, extra=0, off=0):
    """a device copy of x [rows, D] with row stride D + extra that starts ``off`` elements into its allocation -> the strided view"""
    rows, D = x.shape
    buf = torch.full((off + rows * (D + extra) + 1,), float('nan'), dtype=torch.float32, device=DEV)
    view = buf[off:off + rows * (D + extra)].view(rows, D + extra)[:, :D]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 * off % 16 and (rows < 2 or view.stride(0) == D + extra)
    return view


def _guarded(shape, dtype=torch.float64, fill=METRIC_GUARD, words=1):
    """(whole buffer, the view of ``shape`` in its middle): ``words`` guard words of ``fill`` on each side"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * words,), fill, dtype=dtype, device=DEV)
    return buf, buf[words:words + n].view(*shape)


def _guards_ok(buf, fill=METRIC_GUARD, words=1):
    return bool((buf[:words] == fill).all()) and bool((buf[-words:] == fill).all())


# =============================================================================================
# fixtures: import them by name into the module that uses them
# =============================================================================================
@pytest.fixture(scope='module')
def L():
    """the C ABI (ctypes)"""
    assert torch.cuda.is_available(), 'gpu tests need a device'
    from scene_generation_amd import _hip
    return _hip.lib()      # fails loudly if the extension is missing


@pytest.fixture(scope='module')
def hip():
    """the operator layer"""
    assert torch.cuda.is_available(), 'gpu tests need a device'
    from scene_generation_amd import ops, _hip
    _hip.lib()      # fails loudly if the extension is missing
    return ops


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    del _KEEP[:]


def margins_fixture(write):
    """-> a module-scoped autouse fixture that calls write() after the module's last test"""
    @pytest.fixture(scope='module', autouse=True)
    def _margins():
        yield
        write()
    return _margins
