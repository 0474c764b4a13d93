"""What launches SHARE, on a real MI355X: the ticket counters of the in-launch finalisation (one ring per (device, stream), one
capture region per device), the tail-split scratch (per (device, stream), one more for captured launches) and the page-locked
staging slots of the input pipeline.  The per-kernel float64 tests all start from a fresh state -- one launch, one stream, counters
zero, scratch newly sized, nothing captured; the tests here look at the state one launch leaves to the next, through the host
query sg_runtime_state (include/sg2im_hip.h; ``ops.runtime_state``).

Nothing here rests on a timing except the 100 ms of queued work in front of the staging copy (section f), and that is measured
inside the test.
"""
import gc
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import norm_cases as NC
from gpu_harness import close
from gpu_harness import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARITY_SHAPE = ('up', 2, 512, 256, 8)                # the smallest case of test_parity_class_split_vs_plain_schedule
GENERAL_SHAPE = (24, 192, 16, 16, 192, 3, 1, 1)      # of test_tail_split_general_form_vs_plain_schedule: the smallest that splits
F43_SHAPE = (32, 1024, 8)                            # N, C, H: 36 * t % 256 == 128 needs t = 32 tiles, i.e. 32 planes of 8 x 8


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1).mul(scale).float()


def ring(st):
    return st['ring_laps'], st['ring_at']


def drew(s0, s1):
    """counters the launches between two readings of one stream's ring took (fewer than one lap of them)"""
    if s1['ring_laps'] == s0['ring_laps']:
        return s1['ring_at'] - s0['ring_at']
    assert s1['ring_laps'] == s0['ring_laps'] + 1, (s0, s1)
    return s1['ring_at']                             # a request that did not fit restarted at 0


_CACHE = {}


def shared(hip):
    """operands of the two launches most tests here repeat, and their one-stream results (computed once, never written again):
    BatchNorm statistics at C = 4096 (4096 counters under last_block = 2) and the small parity-split transposed conv"""
    if not _CACHE:
        kind, N, Cin, Cout, H = PARITY_SHAPE
        c = _CACHE
        c['px'], c['pw'], c['pb'] = [t.to(DEV) for t in (rnd((N, Cin, H, H), 341), rnd((Cin, Cout, 3, 3), 342, 0.05), rnd((Cout,), 343, 0.2))]
        c['bx'], c['bg'], c['bb'] = [t.to(DEV) for t in (rnd((2, 4096, 2, 2), 351, 2.0), rnd((4096,), 352), rnd((4096,), 353))]
        with torch.no_grad(), NC.option('last_block', 2):
            c['y_bn'], c['y_conv'] = run_bn(hip, c).clone(), run_conv(hip, c).clone()
        torch.cuda.synchronize()
    return _CACHE


def run_conv(hip, c):
    return hip.conv_transpose2d(c['px'], c['pw'], c['pb'], stride=2, pad=1, out_pad=1)


def run_bn(hip, c):
    return hip.batch_norm(c['bx'], c['bg'], c['bb'], None, None, None, True)


# =============================================================================================
# a. every ticket user leaves its counters at zero
# =============================================================================================
def _parity_launch(hip):
    c = shared(hip)
    return 'par_split', 1, 0, lambda: run_conv(hip, c)


def _general_launch(hip):
    N, C, H, W, Cout, KS, stride, pad = GENERAL_SHAPE
    x, w, b = [t.to(DEV) for t in (rnd((N, C, H, W), 331), rnd((Cout, C, KS, KS), 332, 0.05), rnd((Cout,), 333, 0.2))]
    return 'w43_tail_split', 2, 0, lambda: hip.conv2d(x, w, b, stride=stride, pad=pad)


def _f43_launch(hip):
    N, C, H = F43_SHAPE
    x, w, b = [t.to(DEV) for t in (rnd((N, C, H, H), 321), rnd((C, C, 3, 3), 322, 0.05), rnd((C,), 323, 0.2))]
    return 'w43_tail_split', 1, 0, lambda: hip.conv2d(x, w, b, pad=1, reflect=True)


@pytest.mark.parametrize('form', ['parity', 'general', 'f43_half_round'])
def test_gemm_split_forms_draw_counters_and_leave_them_zero(hip, form):
    """One forward launch per split form of the conv GEMMs: in split mode it draws counters from the ring of its stream (the count
    is read from the query, not written here), afterwards no counter of the device is non-zero, and the result equals the plain
    schedule's (mode 0, which draws nothing) at the bound of the existing split tests."""
    from scene_generation_amd import _hip
    option, on, off, run = {'parity': _parity_launch, 'general': _general_launch, 'f43_half_round': _f43_launch}[form](hip)
    saved = _hip.get_option(option)
    out = {}
    try:
        with torch.no_grad():
            for mode in (on, off):
                _hip.set_option(option, mode)
                s0 = hip.runtime_state()
                out[mode] = run().clone()
                s1 = hip.runtime_state(count_nonzero=True)
                n = drew(s0, s1)
                print('%s %s=%d: %d counters drawn, %d non-zero afterwards' % (form, option, mode, n, s1['counters_nonzero']))
                assert (n > 0) == (mode == on), '%s with %s = %d drew %d counters' % (form, option, mode, n)
                assert s1['counters_nonzero'] == 0, '%s with %s = %d left %d counters dirty' % (form, option, mode, s1['counters_nonzero'])
                assert 0 <= s1['ring_at'] <= s1['ring_size']
    finally:
        _hip.set_option(option, saved)
    close(out[on], out[off], 2e-6, form + ' split against plain')


def _loss_launch(hip):
    from scene_generation_amd.ops import _core as K
    from scene_generation_amd.ops.losses import multi_loss
    a = [rnd((n,), 361 + i).to(DEV) for i, n in enumerate((2049, 100001))]
    b = [rnd((n,), 371 + i).to(DEV) for i, n in enumerate((2049, 100001))]
    return lambda: [multi_loss(K.LOSS_L1, a, b, None, [0.75, -1.5], True)]


def _bn_fwd_launch(hip):
    x, g, b = rnd((8, 16, 31, 31), 381, 2.0).to(DEV), rnd((16,), 382).to(DEV), rnd((16,), 383).to(DEV)

    def run():
        rm, rv, nbt = torch.zeros(16, device=DEV), torch.ones(16, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        return [hip.batch_norm(x, g, b, rm, rv, nbt, True, act=1), rm, rv, nbt]
    return run


def _bn_bwd_launch(hip):
    from scene_generation_amd.layers import BatchNorm2d
    x, gy = rnd((8, 16, 31, 31), 381, 2.0).to(DEV), rnd((8, 16, 31, 31), 384).to(DEV)
    m = BatchNorm2d(16).to(DEV)
    with torch.no_grad():
        m.weight.copy_(rnd((16,), 382))
        m.bias.copy_(rnd((16,), 383))

    def prepare():
        m.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_()
        return xg, m(xg, act=1)

    def run(prepared):
        xg, y = prepared
        y.backward(gy)
        return [xg.grad, m.weight.grad, m.bias.grad]
    return prepare, run


def _channel_sum_launch(hip):
    import ctypes
    from scene_generation_amd import _hip
    L = _hip.lib()
    N, C, HW = 4, 16, 4096                                      # S = 4 slices (norm_cases.CHANNEL_SUM_CASES)
    g = rnd((N, C, HW), 391).to(DEV)
    wsb = L.sg_channel_sum_ws_bytes(C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    assert NC.channel_sum_plan(L, N, C, HW, wsb) > 1

    def run():
        out = torch.full((C,), float('nan'), device=DEV)
        _hip.check(L.sg_channel_sum(ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(out.data_ptr()), N, C, HW,
                                    ctypes.c_void_p(ws.data_ptr()), wsb, torch.cuda.current_stream().cuda_stream), 'sg_channel_sum')
        return [out]
    return run


@pytest.mark.parametrize('user', ['two_term_loss', 'batchnorm_fwd', 'batchnorm_bwd', 'channel_sum'])
def test_last_block_users_draw_counters_and_leave_them_zero(hip, user):
    """The in-launch finish of the two-stage reductions (option last_block = 7): the launch draws counters, leaves every counter of
    the device at zero, and its results are bit for bit those of the two-kernel form (last_block = 0, which draws nothing): the
    last arriver adds in the order the separate final kernel uses (common.h, sg_arrive_last)."""
    prepare = lambda: None
    if user == 'batchnorm_bwd':
        prepare, run_prepared = _bn_bwd_launch(hip)
        run = run_prepared
    else:
        launch = {'two_term_loss': _loss_launch, 'batchnorm_fwd': _bn_fwd_launch, 'channel_sum': _channel_sum_launch}[user](hip)
        run = lambda _: launch()
    out = {}
    for lb in (7, 0):
        with NC.option('last_block', lb):
            prepared = prepare()                    # (batchnorm_bwd: the forward, outside the readings)
            s0 = hip.runtime_state()
            res = run(prepared)
            s1 = hip.runtime_state(count_nonzero=True)
            out[lb] = [t.detach().clone() for t in res]
            n = drew(s0, s1)
            print('%s last_block=%d: %d counters drawn, %d non-zero afterwards' % (user, lb, n, s1['counters_nonzero']))
            assert (n > 0) == (lb == 7), '%s with last_block = %d drew %d counters' % (user, lb, n)
            assert s1['counters_nonzero'] == 0, '%s with last_block = %d left %d counters dirty' % (user, lb, s1['counters_nonzero'])
    assert len(out[7]) == len(out[0])
    for i, (u, v) in enumerate(zip(out[7], out[0])):
        assert torch.isfinite(u.float()).all() and torch.equal(u, v), '%s: result %d differs between last_block 7 and 0' % (user, i)


# =============================================================================================
# c. going round the ring
# =============================================================================================
def _rounds_until_two_laps(hip, c, handle=None, cap=100):
    """alternate the two launches of shared() on the current stream until its ring has wrapped twice more; -> (BatchNorm outputs,
    conv outputs).  Checked after every launch: the ring's index stays inside the ring, and a request that did not fit starts at 0."""
    bn_out, conv_out = [], []
    start = hip.runtime_state(stream=handle)
    st = start
    for _ in range(cap):
        for run, outs in ((run_bn, bn_out), (run_conv, conv_out)):
            outs.append(run(hip, c))
            now = hip.runtime_state(stream=handle)
            n = drew(st, now)
            assert n > 0 and 0 < now['ring_at'] <= now['ring_size'], (st, now)
            if outs is bn_out:
                assert n == 4096, 'BatchNorm statistics at C = 4096 ask for one counter per channel, drew %d' % n
            if now['ring_laps'] != st['ring_laps']:
                assert st['ring_at'] + n > st['ring_size'], 'the ring wrapped although the request fitted: %r -> %r' % (st, now)
            else:
                assert st['ring_at'] + n <= st['ring_size']
            st = now
        if st['ring_laps'] >= start['ring_laps'] + 2:
            return bn_out, conv_out
    raise AssertionError('the ring did not wrap twice in %d rounds: %r -> %r' % (cap, start, st))


def test_results_do_not_change_when_the_ring_goes_round(hip):
    """last_block = 2: BatchNorm statistics launches of 4096 counters alternate with the small parity-split transposed conv until
    the ring of the stream has wrapped twice (about 16 rounds a lap): every launch after the first wrap is handed counters that
    earlier launches used.  Every output is bit for bit the first one, the index never leaves the ring, no counter is left
    non-zero, and the conv is the float64 reference's at the bound of test_parity_class_split_vs_plain_schedule."""
    c = shared(hip)
    with torch.no_grad(), NC.option('last_block', 2):
        bn_out, conv_out = _rounds_until_two_laps(hip, c)
        end = hip.runtime_state(count_nonzero=True)
    assert end['ring_laps'] >= 2 and len(bn_out) == len(conv_out) >= 16
    print('%d rounds, ring at %d after %d laps' % (len(bn_out), end['ring_at'], end['ring_laps']))
    for i, (yb, yc) in enumerate(zip(bn_out, conv_out)):
        assert torch.equal(yb, c['y_bn']), 'BatchNorm output of round %d differs from the first' % i
        assert torch.equal(yc, c['y_conv']), 'conv output of round %d differs from the first' % i
    assert end['counters_nonzero'] == 0
    ref = F.conv_transpose2d(c['px'].double().cpu(), c['pw'].double().cpu(), c['pb'].double().cpu(), stride=2, padding=1, output_padding=1)
    close(c['y_conv'], ref, 5e-5, 'parity-split conv against float64')
    x64 = c['bx'].double().cpu()
    bn_ref = F.batch_norm(x64, None, None, c['bg'].double().cpu(), c['bb'].double().cpu(), True, 0.1, 1e-5)
    close(c['y_bn'], bn_ref, 2e-5, 'BatchNorm at C = 4096 against float64')


# =============================================================================================
# d. streams: one ring each
# =============================================================================================
def test_streams_have_their_own_rings(hip):
    """The pattern of the ring test from three side streams that fork from the current stream and are joined every round (the way
    Trainer.step uses its side streams), until each has wrapped its ring twice.  A launch on one stream leaves ring_at and
    ring_laps of every other stream as they were (one ring per (device, stream): with one ring shared by all streams, a wrap could
    hand the counters of a launch still queued on stream A to a launch on stream B, and only the per-step join of Trainer.step
    stood in the way); the results are bit for bit the one-stream results."""
    c = shared(hip)
    main = torch.cuda.current_stream()
    side = [torch.cuda.Stream() for _ in range(3)]
    handles = [s.cuda_stream for s in side] + [main.cuda_stream]
    assert len(set(handles)) == 4
    outs = []
    rings = lambda: [ring(hip.runtime_state(stream=h)) for h in handles]
    rounds = 0
    with torch.no_grad(), NC.option('last_block', 2):
        start = rings()
        while True:
            rounds += 1
            assert rounds <= 100, 'the rings did not wrap twice in 100 rounds: %r' % (rings(),)
            for i, s in enumerate(side):
                s.wait_stream(main)
                with torch.cuda.stream(s):
                    for run in (run_bn, run_conv):
                        before = rings()
                        outs.append((run, run(hip, c)))
                        after = rings()
                        assert after[i] != before[i], 'a launch on stream %d drew nothing from its own ring' % i
                        for j in range(4):
                            if j != i:
                                assert after[j] == before[j], ('a launch on stream %d moved the ring of stream %d: %r -> %r'
                                                               % (i, j, before[j], after[j]))
            for s in side:
                main.wait_stream(s)
            now = rings()
            if all(now[i][0] >= start[i][0] + 2 for i in range(3)):
                break
        end = hip.runtime_state(count_nonzero=True)
    assert rings()[3] == start[3], 'the current stream launched nothing, its ring moved'
    assert end['counters_nonzero'] == 0
    print('%d rounds on 3 streams' % rounds)
    for k, (run, y) in enumerate(outs):
        assert torch.equal(y, c['y_bn'] if run is run_bn else c['y_conv']), 'launch %d differs from the one-stream result' % k


# =============================================================================================
# e. captures
# =============================================================================================
def test_capture_takes_its_counters_once_and_without_tail_capture_the_plain_schedule(hip):
    """The parity-split conv captured on one stream after an eager warm-up: the capture draws its counters from the capture region
    (once -- replays draw nothing) and none from the ring, replays are bit for bit the eager split result and leave every counter at
    zero.  Captured again with tail_capture = 0 the launch gets no scratch: the region does not move and the replay is bit for bit the
    plain schedule (par_split = 0).  Exhaustion of the region by arithmetic: a region that is never reclaimed must hold every capture
    of a process; the captures of this suite that precede this test have used less than half of it, and the ones made here would fit
    a hundred times over."""
    c = shared(hip)
    with torch.no_grad():
        with NC.option('par_split', 0):
            y_plain = run_conv(hip, c).clone()
        y_split = run_conv(hip, c).clone()                     # eager warm-up: the captured scratch is large enough afterwards
        assert torch.equal(y_split, c['y_conv']) and not torch.equal(y_split, y_plain), 'the split schedule did not run'
        s0 = hip.runtime_state()
        assert s0['tail_captured_bytes'] > 0 and s0['tail_bytes'] > 0 and s0['captured_size'] > 0
        ga = torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga):
            ya = run_conv(hip, c)
        s1 = hip.runtime_state()
        per_capture = s1['captured_used'] - s0['captured_used']
        assert per_capture > 0, 'the captured launch drew no counters: it did not take the split schedule'
        assert ring(s1) == ring(s0), 'a captured launch drew from the ring of eager launches'
        for _ in range(3):
            ga.replay()
            assert torch.equal(ya, y_split)
        s2 = hip.runtime_state(count_nonzero=True)
        assert s2['captured_used'] == s1['captured_used'], 'replays drew counters'
        assert s2['counters_nonzero'] == 0
        with NC.option('tail_capture', 0):
            gp = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gp):
                yp = run_conv(hip, c)
        s3 = hip.runtime_state()
        assert s3['captured_used'] == s2['captured_used'], 'a capture without scratch drew counters'
        gp.replay()
        assert torch.equal(yp, y_plain), 'without scratch the capture must take the plain schedule'
        ga.replay()
        assert torch.equal(ya, y_split)
        s4 = hip.runtime_state(count_nonzero=True)
    assert s4['counters_nonzero'] == 0 and s4['captured_used'] == s3['captured_used']
    print('capture region: %d of %d used, %d per capture of this conv' % (s4['captured_used'], s4['captured_size'], per_capture))
    assert s4['captured_used'] <= s4['captured_size'] // 2
    assert (s4['captured_size'] - s4['captured_used']) // per_capture >= 100


def test_replay_after_the_captured_scratch_grew_in_a_fresh_process():
    """tests/shared_state_child.py in a process of its own (a fresh runtime: no pool, no scratch).  Before the first request every
    field of the query is 0.  A capture that is the first launch to ask for scratch gets none (nullptr: plain schedule, no counter,
    bit for bit the par_split = 0 result).  Then graph A (parity-split conv) is captured after its warm-up, the F(4x4,3x3) half-round
    conv runs eagerly and outgrows both scratch buffers (they are replaced, the old ones retired but held: graph A has the old
    address baked in), graph B captures that conv, and A, B, A, B replay bit for bit their eager results, leaving all counters zero;
    the capture region moved once per capture and not per replay."""
    env = dict(os.environ)
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'shared_state_child.py')], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, 'child failed (%d):\n%s\n%s' % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    o = json.loads(lines[0])
    print(json.dumps(o, indent=1))
    for when in ('fresh', 'after_plain'):
        want = dict.fromkeys(o[when], 0)
        assert o[when] == want, '%s: %r' % (when, o[when])                    # counters_nonzero too: asked for, nothing to count
    cold = o['after_cold_capture']
    assert cold['captured_used'] == 0 and cold['tail_captured_bytes'] == 0 and cold['ring_at'] == 0 and cold['tail_bytes'] == 0
    assert o['cold_capture_equals_plain'] is True
    assert o['par_split_differs_from_plain'] is True, 'the split schedule did not run'
    e, a, f, b, end = (o[k] for k in ('after_par_eager', 'after_capture_a', 'after_f43_eager', 'after_capture_b', 'after_replays'))
    assert e['ring_at'] > 0 and e['ring_size'] > 0 and e['tail_bytes'] > 0 and e['tail_captured_bytes'] >= e['tail_bytes']
    assert e['tail_retired'] == 0 and e['captured_used'] == 0 and e['captured_size'] > 0
    n_a = a['captured_used'] - e['captured_used']
    assert n_a > 0 and ring(a) == ring(e) and a['tail_retired'] == 0
    assert f['tail_captured_bytes'] > a['tail_captured_bytes'] and f['tail_bytes'] > a['tail_bytes']
    assert f['tail_retired'] == a['tail_retired'] + 2, 'the outgrown buffers of the stream and of the captures are both kept'
    assert f['captured_used'] == a['captured_used'] and drew(a, f) > 0
    n_b = b['captured_used'] - f['captured_used']
    assert n_b > 0 and ring(b) == ring(f) and b['tail_retired'] == f['tail_retired']
    assert o['replays_equal_eager'] == [True] * 4
    assert end['captured_used'] == b['captured_used'] == n_a + n_b, 'the region moves once per capture, never per replay'
    assert end['counters_nonzero'] == 0
    assert end['tail_captured_bytes'] == f['tail_captured_bytes'] and end['tail_retired'] == f['tail_retired']
    assert 100 * (n_a + n_b) <= end['captured_size']


# =============================================================================================
# f. the page-locked staging slots outlive their copies
# =============================================================================================
def _queue_blocker(min_ms=100.0):
    """at least ``min_ms`` of matmul launches on the current stream, by the measured duration of one of them; -> queued ms"""
    a = torch.empty(8192, 8192, device=DEV).fill_(1e-3)
    out = torch.empty_like(a)
    torch.mm(a, a, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.mm(a, a, out=out)
    e1.record()
    e1.synchronize()
    one = e0.elapsed_time(e1)
    n = int(math.ceil(3.0 * min_ms / one))                       # three times what the precondition needs
    assert one > 0 and n * one >= min_ms
    for _ in range(n):
        torch.mm(a, a, out=out)
    return n * one


@pytest.mark.parametrize('how', ['close', 'del'])
@pytest.mark.parametrize('threaded', [False, True])
def test_prefetcher_drains_its_copies_before_it_lets_go_of_the_slots(hip, threaded, how):
    """The copy kernel of a batch reads a page-locked slot that torch's host allocator does not track.  With the copy queued behind
    >= 100 ms of work, ``close()`` (or dropping the prefetcher) must wait for it before the slot's buffer goes back to the
    allocator: afterwards every slot event has completed, and a pinned tensor of the slot's size, allocated and overwritten at
    once, cannot reach the batch -- the device batch is the source batch byte for byte."""
    from scene_generation_amd.pipeline import DeviceBatchPrefetcher
    from scene_generation_amd.synthetic import make_batch
    host = [make_batch(N=4, min_objs=2, max_objs=5, size=64, seed=90 + i) for i in range(3)]
    pf = DeviceBatchPrefetcher(host, DEV, threaded=threaded)
    torch.cuda.synchronize()
    queued_ms = _queue_blocker()
    db = next(pf)
    events = [s['ev'] for s in pf._slots if s.get('ev') is not None]
    slot_bytes = max(s['buf'].numel() for s in pf._slots if s.get('buf') is not None)
    assert len(events) == 1 and queued_ms >= 100.0
    assert not events[0].query(), 'precondition: the copy must still be queued behind %.0f ms of work' % queued_ms
    worker = pf._thread                                # (holds the prefetcher through a weak reference only)
    if how == 'close':
        pf.close()
    else:
        del pf
        gc.collect()
        if worker is not None:                         # had the worker held the last reference for an instant, it ran __del__
            worker.join(5.0)
            assert not worker.is_alive()
    done = [e.query() for e in events]
    scribble = torch.empty(slot_bytes, dtype=torch.uint8, pin_memory=True).fill_(0xAB)
    torch.cuda.synchronize()
    assert all(done), 'the prefetcher let go of its slots while their copies were still queued'
    assert int(scribble[0]) == 0xAB
    for name, got, want in zip(db.batch._fields, db.batch, host[0]):
        assert got.dtype == want.dtype and got.shape == want.shape, name
        assert torch.equal(got.cpu().contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), \
            'field %s of the device batch is not the source batch' % name
