"""The measuring primitives of tools/benchkit.py without a device: every speed figure of the project comes out of them, so how
many calls they make, in which order, and what they return is pinned here on a fake device whose clock only advances when the
measured function is called."""
import ast
import glob
import json
import os
import statistics
from fractions import Fraction

import pytest

from tools import benchkit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeDevice:
    """stands in for torch.cuda and time.perf_counter: integer microseconds, so that every difference is exact"""

    def __init__(self, available=True):
        self.us, self.available, self.device, self.syncs = 0, available, None, 0

    def clock(self):
        return Fraction(self.us, 10 ** 6)

    def is_available(self):
        return self.available

    def set_device(self, k):
        self.device = k

    def synchronize(self):
        self.syncs += 1

    def Event(self, enable_timing=False):
        assert enable_timing
        return _Event(self)


class _Event:
    def __init__(self, dev):
        self.dev, self.at = dev, None

    def record(self):
        self.at = self.dev.us

    def elapsed_time(self, other):
        return (other.at - self.at) / 1e3


class Work:
    """a measured function: call k costs ms[k] (the last entry from then on); keeps the arguments of every call"""

    def __init__(self, dev, *ms):
        self.dev, self.ms, self.args = dev, ms, []

    def __call__(self, *args):
        self.dev.us += int(round(self.ms[min(len(self.args), len(self.ms) - 1)] * 1000))
        self.args.append(args)

    @property
    def calls(self):
        return len(self.args)


@pytest.fixture
def dev(monkeypatch):
    d = FakeDevice()
    monkeypatch.setattr(benchkit, 'cuda', d)
    monkeypatch.setattr(benchkit, 'clock', d.clock)
    return d


# ---- timed_block ---------------------------------------------------------------------------------------------------------------------
def test_timed_block_probes_with_one_call_then_sizes_the_block(dev):
    """10 ms a call, 0.5 s: one call is 10 ms, the count becomes max(2, int(1 * 0.5 * 1.2e3 / 10)) = 60, the second block is 600 ms"""
    fn = Work(dev, 10)
    assert benchkit.timed_block(fn, 0.5) == (10.0, 10.0, 60)
    assert fn.calls == 61 and fn.args == [()] * 61


def test_timed_block_keeps_a_first_call_that_is_long_enough(dev):
    fn = Work(dev, 600)
    assert benchkit.timed_block(fn, 0.5) == (600.0, 600.0, 1)
    assert fn.calls == 1


def test_timed_block_gates_on_the_host_clock_and_reads_both(dev, monkeypatch):
    """a host clock that runs twice as fast as the events: the block is sized by the host's 20 ms a call (count 30), and the two
    per-call times are each clock's own"""
    monkeypatch.setattr(benchkit, 'clock', lambda: 2 * dev.clock())
    fn = Work(dev, 10)
    assert benchkit.timed_block(fn, 0.5) == (20.0, 10.0, 30)


# ---- device_block --------------------------------------------------------------------------------------------------------------------
def test_device_block_resizes_once_and_counts_from_zero(dev):
    """10 ms a call, 0.5 s: the probe is dropped, the count becomes int(1 * 0.5 * 1.1e3 / 10) = 55, the counted block is 550 ms"""
    fn = Work(dev, 10)
    assert benchkit.device_block(fn, 0.5) == (10.0, 55)
    assert fn.args == [(0,)] + [(i,) for i in range(55)]


def test_device_block_accumulates_blocks_that_cannot_grow(dev):
    """200 ms a call, 0.5 s.  Pass 1: one call (index 0), 200 ms < 500, nothing counted yet, int(1 * 550 / 200) = 2 > 1: the count
    becomes 2 and the probe is dropped.  Pass 2: two calls (indices 0, 1), 400 ms < 500, nothing counted yet, int(2 * 550 / 400) = 2:
    no growth, so the block is counted (total 400 ms, 2 calls) -- dropping it to size the block again would give 2 once more, without
    end.  Pass 3: two calls (indices 2, 3), total 800 ms >= 500, 4 calls: (800 / 4, 4) after 5 calls of fn"""
    fn = Work(dev, 200)
    assert benchkit.device_block(fn, 0.5) == (200.0, 4)
    assert fn.args == [(0,), (0,), (1,), (2,), (3,)]


def test_device_block_counts_a_probe_that_is_long_enough(dev):
    fn = Work(dev, 600)
    assert benchkit.device_block(fn, 0.5) == (600.0, 1)
    assert fn.args == [(0,)]


# ---- measure -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('warmup', (2, 3))
def test_measure_honours_the_warm_up_and_summarises_uneven_blocks(dev, monkeypatch, warmup):
    """every call lasts at least the 0.1 s of a block, so a block is one call: blocks of 120, 100, 150, 110, 130 ms"""
    times = [120, 100, 150, 110, 130]
    fn = Work(dev, *([7] * warmup + times))
    calls_before_block, real = [], benchkit.timed_block
    monkeypatch.setattr(benchkit, 'timed_block', lambda f, s: (calls_before_block.append(f.calls), real(f, s))[1])
    r = benchkit.measure(fn, 0.1, 5, warmup=warmup)
    assert calls_before_block == [warmup + k for k in range(5)]
    assert r == {'ms': 120.0, 'spread': (150.0 - 100.0) / 120.0, 'blocks_ms': [float(t) for t in times]}
    assert r['ms'] == statistics.median(times)


def test_measure_reads_the_events_on_request(dev, monkeypatch):
    monkeypatch.setattr(benchkit, 'clock', lambda: 2 * dev.clock())
    assert benchkit.measure(Work(dev, 300), 0.5, 3)['blocks_ms'] == [600.0] * 3
    assert benchkit.measure(Work(dev, 300), 0.5, 3, device_events=True)['blocks_ms'] == [300.0] * 3


def test_measure_with_clocks_adds_the_keys_of_the_fid_family(dev, monkeypatch):
    monkeypatch.setattr(benchkit.glob, 'glob', lambda pattern: [])
    fn = Work(dev, 10)
    r = benchkit.measure(fn, 0.5, 2, clocks=True)
    assert set(r) == {'ms', 'spread', 'blocks_ms', 'device_events_ms', 'launches_per_block', 'clocks_before', 'clocks_after'}
    assert r['launches_per_block'] == 60 and r['device_events_ms'] == 10.0 and r['blocks_ms'] == [10.0, 10.0]
    assert r['clocks_before'] == r['clocks_after'] == {'sclk_mhz': None, 'mclk_mhz': None}
    assert fn.calls == 3 + 2 * 61 + 60                      # warm-up, two blocks with their probes, the pass between two events


def test_clocks_reads_the_active_level_and_nulls_without_the_files(monkeypatch, tmp_path):
    monkeypatch.setattr(benchkit.glob, 'glob', lambda pattern: [])
    assert benchkit.clocks() == {'sclk_mhz': None, 'mclk_mhz': None}
    for name, text in (('pp_dpm_sclk', '0: 132Mhz\n1: 2400Mhz *\n'), ('pp_dpm_mclk', '0: 900Mhz *\n1: 2000Mhz\n')):
        (tmp_path / name).write_text(text)
    monkeypatch.setattr(benchkit.glob, 'glob', lambda pattern: [str(tmp_path / os.path.basename(pattern)), '/nonexistent/' + pattern[-11:]])
    assert benchkit.clocks() == {'sclk_mhz': 2400, 'mclk_mhz': 900}


# ---- event_runs ----------------------------------------------------------------------------------------------------------------------
def test_event_runs_and_the_reductions_of_the_six_tools(dev):
    """2 warm-ups, then 3 runs of 4 calls at 3, 1 and 2 ms a call"""
    fn = Work(dev, *([9] * 2 + [3] * 4 + [1] * 4 + [2] * 4))
    ms = benchkit.event_runs(fn, 4, 3, 2)
    assert ms == [3.0, 1.0, 2.0] and fn.calls == 2 + 4 * 3 and fn.args == [()] * 14
    us = [t * 1e3 for t in ms]
    assert (statistics.median(us), min(us), max(us)) == (2000.0, 1000.0, 3000.0)        # bench_ema, _gradctl, _bf16_trunk: microseconds
    assert min(ms) == 1.0                                                                # bench_conv, _linear, _wino_gemm: best, ms


def test_event_runs_indexed_passes_the_call_index_of_the_run(dev):
    fn = Work(dev, 5)
    assert benchkit.event_runs(fn, 3, 2, 3, indexed=True) == [5.0, 5.0]
    assert fn.args == [(0,)] * 3 + [(0,), (1,), (2,)] * 2


# ---- host_ms, emit, require_device, profiled -----------------------------------------------------------------------------------------
def test_host_ms_returns_the_time_and_the_result(dev):
    fn = Work(dev, 25)
    assert benchkit.host_ms(lambda: (fn(), 'r')[1]) == (25.0, 'r') and dev.syncs == 0
    assert benchkit.host_ms(lambda: (fn(), 's')[1], sync=True) == (25.0, 's') and dev.syncs == 2


def test_emit_appends_one_sorted_line_and_prints_it(tmp_path, capsys):
    out = tmp_path / 'x.jsonl'
    out.write_text('before\n')
    benchkit.emit(str(out), {'b': 1, 'a': [2.5, None]})
    line = json.dumps({'a': [2.5, None], 'b': 1}, sort_keys=True)
    assert line.index('"a"') < line.index('"b"')
    assert out.read_text() == 'before\n' + line + '\n'
    assert capsys.readouterr().out == line + '\n'
    benchkit.emit(None, {'b': 1, 'a': 0})
    assert capsys.readouterr().out == '{"a": 0, "b": 1}\n'
    assert sorted(os.listdir(str(tmp_path))) == ['x.jsonl'] and out.read_text().count('\n') == 2


def test_require_device_fails_without_a_device(monkeypatch):
    none = FakeDevice(available=False)
    monkeypatch.setattr(benchkit, 'cuda', none)
    with pytest.raises(AssertionError, match='nothing is measured without a device'):
        benchkit.require_device()
    assert none.device is None
    one = FakeDevice()
    monkeypatch.setattr(benchkit, 'cuda', one)
    benchkit.require_device()
    assert one.device == 0


class FakeOps:
    def __init__(self):
        self.log, self.CALLS = [], [7]

    def prof_enable(self, on):
        self.log.append(('enable', on))

    def prof_reset(self):
        self.log.append('reset')

    def prof_read(self):
        self.log.append('read')
        return {'kind': {'ms': 1.0, 'launches': 2, 'flops': 0.0, 'bytes': 0.0}}


def test_profiled_counts_the_calls_and_disables_the_timers_when_fn_raises():
    ops = FakeOps()

    def three_calls():
        ops.log.append('fn')
        ops.CALLS[0] += 3
    assert benchkit.profiled(three_calls, ops=ops) == ({'kind': {'ms': 1.0, 'launches': 2, 'flops': 0.0, 'bytes': 0.0}}, 3)
    assert ops.log == [('enable', True), 'reset', 'fn', 'read', ('enable', False)]

    ops = FakeOps()

    def boom():
        raise ValueError('inside')
    with pytest.raises(ValueError, match='inside'):
        benchkit.profiled(boom, ops=ops)
    assert ops.log == [('enable', True), 'reset', ('enable', False)]


# ---- the tools' source ---------------------------------------------------------------------------------------------------------------
TOOLS = sorted(glob.glob(os.path.join(ROOT, 'tools', 'bench_*.py')))
OWNED = {'timed_block', 'measure', 'emit', 'timeit', 'clocks'}


def test_the_bench_tools_are_all_there():
    assert len(TOOLS) == 21


@pytest.mark.parametrize('path', TOOLS, ids=[os.path.basename(p) for p in TOOLS])
def test_a_bench_tool_keeps_no_copy_and_imports_no_other_tool(path):
    with open(path) as f:
        tree = ast.parse(f.read())
    imported, defined, uses_kit = [], [], False
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            imported += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            imported += [node.module or ''] + ['%s.%s' % (node.module, a.name) for a in node.names]
            uses_kit = uses_kit or node.module == 'tools.benchkit'
        elif isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
            defined.append(node.name)
    assert not [m for m in imported if any(part.startswith('bench_') for part in m.split('.'))], imported
    assert not OWNED & set(defined), sorted(OWNED & set(defined))
    assert uses_kit, 'every tool measures through tools/benchkit.py'
