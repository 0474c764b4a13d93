"""What the tools/bench_*.py scripts share: the measuring primitives, one copy of each.  A tool keeps its shapes, its byte and FLOP
counts and its records, and names its method by the primitive it calls:

* ``measure`` / ``timed_block``: a warm-up, then the median of blocks of at least ``seconds`` of back-to-back calls each; a block is
  sized on the host clock (the repeat count grows by 1.2) and read on the host clock around a device synchronise or between two
  device events.
* ``device_block``: back-to-back calls between two device events, accumulated until ``min_seconds`` of device time (1.1).
* ``event_runs``: ``reps`` runs of a fixed ``n`` calls between two device events.
* ``host_ms``: one call on the host clock.   * ``profiled``: one call under the library's per-kind event timers.

``cuda`` and ``clock`` are the seam: tests/test_benchkit_cpu.py drives everything here with a fake device in their place."""
import glob
import json
import statistics
import time

import torch

cuda = torch.cuda
clock = time.perf_counter


def require_device():
    assert cuda.is_available(), 'the benchmark needs cuda:0: nothing is measured without a device'
    cuda.set_device(0)


def emit(out, rec):
    """one JSON line on stdout and, unless ``out`` is None, appended to the file ``out``"""
    line = json.dumps(rec, sort_keys=True)
    print(line, flush=True)
    if out is not None:
        with open(out, 'a') as f:
            f.write(line + '\n')


def clocks():
    """{'sclk_mhz', 'mclk_mhz'} of the first card that reports an active level, else nulls"""
    out = {'sclk_mhz': None, 'mclk_mhz': None}
    for key, name in (('sclk_mhz', 'pp_dpm_sclk'), ('mclk_mhz', 'pp_dpm_mclk')):
        for path in sorted(glob.glob('/sys/class/drm/card*/device/' + name)):
            try:
                active = [l for l in open(path).read().splitlines() if l.strip().endswith('*')]
            except OSError:
                continue
            if active:
                out[key] = int(''.join(c for c in active[0].split(':')[1] if c.isdigit()))
                break
    return out


_clocks = clocks            # (measure's keyword of the same name hides the function inside it)


def _events():
    return cuda.Event(enable_timing=True), cuda.Event(enable_timing=True)


def timed_block(fn, min_seconds):
    """-> (host ms per call, device-event ms per call, calls) of one block of back-to-back calls that lasts >= min_seconds on the
    host clock around a final synchronise; the two events are always recorded"""
    reps = 1
    while True:
        cuda.synchronize()
        e0, e1 = _events()
        t0 = clock()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        cuda.synchronize()
        host_ms = (clock() - t0) * 1e3
        if host_ms >= min_seconds * 1e3:
            return host_ms / reps, e0.elapsed_time(e1) / reps, reps
        reps = max(reps + 1, int(reps * min_seconds * 1.2e3 / max(host_ms, 1e-3)))


def summary(blocks):
    med = statistics.median(blocks)
    return {'ms': med, 'spread': (max(blocks) - min(blocks)) / med, 'blocks_ms': blocks}


def measure(fn, seconds, blocks, warmup=3, device_events=False, clocks=False):
    """-> {'ms', 'spread', 'blocks_ms'} of ``blocks`` timed blocks after ``warmup`` calls, each block read between its device events
    or on the host clock.  clocks=True: also the driver's clocks before and after, the calls of the last block and the time of as
    many calls once more between two device events"""
    for _ in range(warmup):
        fn()
    cuda.synchronize()
    before = _clocks() if clocks else None
    runs = [timed_block(fn, seconds) for _ in range(blocks)]
    out = summary([r[1 if device_events else 0] for r in runs])
    if clocks:
        reps = runs[-1][2]
        out.update(device_events_ms=event_runs(fn, reps, 1, 0)[0], launches_per_block=reps, clocks_before=before, clocks_after=_clocks())
    return out


def device_block(fn, min_seconds):
    """-> (ms per call, calls): back-to-back ``fn(call index)`` between two device events until >= min_seconds of device time"""
    calls, reps, total = 0, 1, 0.0
    e0, e1 = _events()
    while total < min_seconds * 1e3:
        e0.record()
        for i in range(reps):
            fn(calls + i)
        e1.record()
        cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if calls == 0 and ms < min_seconds * 1e3:                # size one block to cover the whole time
            grown = int(reps * min_seconds * 1.1e3 / max(ms, 1e-3))
            if grown > reps:                                     # (a block that cannot grow is counted: a call of 0.4 of the time
                reps = grown                                     # gives 2 again and again, and would be repeated for ever)
                continue
        total += ms
        calls += reps
    return total / calls, calls


def event_runs(fn, n, reps, warmup, indexed=False):
    """-> [ms per call] of ``reps`` runs of ``n`` back-to-back calls between two device events, after ``warmup`` calls.
    indexed=True: ``fn(call index within the run)``, as device_block passes it (0 in the warm-up)"""
    call = fn if indexed else (lambda i: fn())
    for _ in range(warmup):
        call(0)
    cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = _events()
        e0.record()
        for i in range(n):
            call(i)
        e1.record()
        cuda.synchronize()
        out.append(e0.elapsed_time(e1) / n)
    return out


def host_ms(fn, sync=False):
    """-> (ms on the host clock, fn()); sync=True: between two device synchronises"""
    if sync:
        cuda.synchronize()
    t0 = clock()
    res = fn()
    if sync:
        cuda.synchronize()
    return (clock() - t0) * 1e3, res


def profiled(fn, ops=None):
    """-> (the library's prof_read() of one fn(): {kind: ms, launches, flops, bytes}, the C-ABI calls it made)"""
    if ops is None:
        from scene_generation_amd import ops
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        c0 = ops.CALLS[0]
        fn()
        calls = ops.CALLS[0] - c0
        prof = ops.prof_read()
    finally:
        ops.prof_enable(False)
    return prof, calls


def generator_flat_numel():
    """(parameters, elements of their FlatParams buffer) of the generator at BASELINE configs[1], counted on the meta device"""
    from scene_generation_amd.args import parser
    from scene_generation_amd.model import Model
    from scene_generation_amd.optim import FlatParams
    from scene_generation_amd.synthetic import make_vocab
    args = parser.parse_args(['--image_size', '128,128', '--output_dir', '/tmp/o'])
    kw = {'vocab': make_vocab(), 'image_size': args.image_size, 'embedding_dim': args.embedding_dim,
          'gconv_dim': args.gconv_dim, 'gconv_hidden_dim': args.gconv_hidden_dim, 'gconv_num_layers': args.gconv_num_layers,
          'mlp_normalization': args.mlp_normalization, 'appearance_normalization': args.appearance_normalization,
          'activation': args.activation, 'mask_size': args.mask_size, 'n_downsample_global': args.n_downsample_global,
          'box_dim': args.box_dim, 'use_attributes': args.use_attributes, 'box_noise_dim': args.box_noise_dim,
          'mask_noise_dim': args.mask_noise_dim, 'pool_size': args.pool_size, 'rep_size': args.rep_size}
    with torch.device('meta'):
        ps = list(Model(**kw).parameters())
    a = FlatParams.ALIGN
    return sum(p.numel() for p in ps), sum((p.numel() + a - 1) // a * a for p in ps)
