"""Data parallelism through the REAL HIP Trainer: two ranks, each trains on its shard of one batch.  backend 'gloo': both
ranks share cuda:0 (gloo moves the gradient slices; runs on a 1-GPU box); backend 'nccl' (= RCCL over xGMI): one GPU per
rank, two ranks when two devices are visible and one rank on a 1-GPU box (RCCL refuses two ranks on one device) -- the first
multi-GPU run of the suite exercises RCCL itself.  Checks (SURVEY 8e semantics: "the reference run independently on each
shard, gradients averaged"): (1) the all-reduced generator / discriminator gradients of the first step equal the mean of the
per-shard gradients of single-process trainers; (2) after two full G+D steps (use_gt on, then off: box_net is skipped by Adam
in the second one on EVERY rank) all four optimisers hold bit-identical parameters on every rank; (3) an all-reduce of the
backend over each trained buffer returns exactly world x the buffer."""
import os
import random
import socket
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

ARGV = ['--image_size', '32,32', '--batch_size', '4', '--vgg_features_weight', '0', '--output_dir', '/tmp/o',
        '--n_downsample_global', '2', '--gconv_hidden_dim', '64', '--gconv_num_layers', '3', '--mask_size', '8',
        '--ndf', '8', '--ndf_mask', '8', '--crop_size', '16', '--d_obj_arch', 'C4-8-2,C4-16-2', '--pool_size', '2']
OPTS = ('optimizer', 'optimizer_d_mask', 'optimizer_d_obj', 'optimizer_d_img')


def _make(distributed, device='cuda:0'):
    from scene_generation_amd.args import parser
    from scene_generation_amd.synthetic import make_vocab, fill_deterministic
    from scene_generation_amd.trainer import Trainer
    tr = Trainer(parser.parse_args(ARGV), make_vocab(12, 4, 35), device=device, distributed=distributed)
    for m in (tr.model, tr.netD, tr.obj_discriminator, tr.mask_discriminator):
        fill_deterministic(m)
    tr.model.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    grads = {}
    for n in OPTS:
        o = getattr(tr, n)
        # first step only.  Under data parallelism the buffer holds the all-reduced SUM here and the optimiser's grad_scale
        # the 1 / world the Adam kernel applies while reading it (this hook runs after the reducer's)
        o.pre_step_hooks.append(lambda o=o, n=n: grads.setdefault(n, (o.fp.grad.detach() * o.grad_scale).cpu().clone()))
    return tr, grads


def _batch():
    from scene_generation_amd.synthetic import make_batch
    return make_batch(N=4, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=12, num_preds=4, seed=7)


def _worker(rank, world, port, q, backend):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch.distributed as dist
    from scene_generation_amd.synthetic import shard_batch, batch_to
    dev = 'cuda:%d' % (rank if backend == 'nccl' else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    tr, grads = _make(True, dev)
    # buckets leave during the generator's backward: nothing may be parked in a spill buffer until the backward ends
    assert tr.optimizer.use_spill is False and tr.optimizer_d_img.use_spill is True
    if rank == 1:                                    # the broadcast at construction already happened: perturbing now would
        pass                                         # desynchronise on purpose; nothing to do
    shard = batch_to(shard_batch(_batch(), rank, world), dev)
    random.seed(100 + rank)                          # different local RNG streams: the coin must still agree
    coins = []
    for it in range(2):
        random.seed(5)                               # same VectorPool draws as the single-process references
        use_gt = (it == 0)
        coins.append(tr.draw_use_gt(random.Random(rank + it)))
        tr.step(shard, use_gt=use_gt)
    torch.cuda.synchronize()
    # one collective of the backend itself over every trained buffer (RCCL on the device for 'nccl', also with a single rank):
    # the ranks hold bit-identical parameters, so the SUM is exactly world x the buffer (exact in fp32 for world <= 2)
    summed = {}
    for n in OPTS:
        t = getattr(tr, n).fp.flat.detach().clone()
        dist.all_reduce(t)
        summed[n] = bool(torch.equal(t, getattr(tr, n).fp.flat.detach() * world))
    torch.cuda.synchronize()
    q.put((rank, {n: g.numpy() for n, g in grads.items()}, {n: getattr(tr, n).fp.flat.detach().cpu().numpy() for n in OPTS},
           coins, [r.world for r in tr.reducers], summed))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize('backend', ['gloo', 'nccl'])
def test_two_rank_hip_trainer_matches_sequential_shards(backend):
    import numpy as np
    import torch.multiprocessing as mp
    from scene_generation_amd.synthetic import shard_batch, batch_to
    # RCCL needs one GPU per rank (it refuses two ranks on one device): with a single GPU the 'nccl' case runs ONE rank -- the
    # RCCL communicator on the device, Trainer(distributed=True) under it and the all-reduce of every trained buffer -- and the
    # two-rank arithmetic is the 'gloo' case's, on the same GPU
    world = 2 if backend == 'gloo' else min(2, torch.cuda.device_count())
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, backend)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    # single-process references: one fresh trainer per shard, first step only
    want = {n: 0 for n in OPTS}
    for r in range(world):
        tr, grads = _make(False)
        random.seed(5)
        tr.step(batch_to(shard_batch(_batch(), r, world), 'cuda:0'), use_gt=True)
        torch.cuda.synchronize()
        for n in OPTS:
            want[n] = want[n] + grads[n].numpy() / world
        del tr
    for rank, grads, flats, coins, worlds, summed in res:
        assert worlds == [world] * 4
        assert all(summed.values()), 'rank %d: %s all-reduce of the trained buffers: %s' % (rank, backend, summed)
        for n in OPTS:
            g, w = grads[n], want[n]
            err = float(np.abs(g - w).max())
            assert err <= 2e-5 * max(1.0, float(np.abs(w).max())), 'rank %d %s: reduced gradient off by %g' % (rank, n, err)
    for other in res[1:]:
        assert res[0][3] == other[3], 'the use_gt coin must be identical on all ranks'
        for n in OPTS:
            assert np.array_equal(res[0][2][n], other[2][n]), '%s: ranks diverged after two steps' % n


# (round 6: the two-rank case ran batch 8 per rank for 2 timed steps and took 444 s of an 1100 s suite on one box of the pool: with
#  two ranks on one GPU every step sits ~20 s in gloo's waits for the 765 MB of gradient buckets (stack dumps, SG_BENCH_STACKS;
#  the isolated all-reduces take 0.23 s, eight ranks 1.3 s per step) -- an artefact of gloo on a shared device, nothing RCCL
#  shares.  The four-rank case carries the per-launch profiler pass; the two-rank case runs the protocol at its minimum:
#  batch 2, one timed / isolated / observed step, no profiler pass)
# At most four ranks share the one GPU: with the test process itself that is five processes holding the device open.  The
# eight-rank arithmetic of configs[2] (shards, bucket schedule, flag OR) is covered on the host by
# test_distributed_cpu.py::test_world8_generator_buckets_and_config3_shards.
@pytest.mark.parametrize('world,per_gpu,steps', [(2, 2, 1), (4, 2, 1)])
def test_bench_dp_leg_executes_two_ranks_on_one_gpu(world, per_gpu, steps):
    """bench.py's multi-GPU leg exactly as the driver launches it (``python -m torch.distributed.run --nproc-per-node N bench.py
    --gpus N``), with N = 2 and N = 4 ranks sharing this box's one GPU over gloo (SG_DIST_BACKEND=gloo SG_SHARE_GPU=1):
    first-contact check, Trainer(distributed=True) at FULL widths (ten >= 64 MB generator buckets), the Adam steps deferred
    behind the reduces, ``time_buckets``, ``exposed_ms`` and the JSON contract.  VERDICT r3 / r4: the first multi-GPU run must
    not be the first execution of this code -- the world-4 case runs the process group, rank arithmetic and bucket schedule of
    the multi-GPU line with everything but the transport (gloo through host memory instead of RCCL over xGMI)."""
    import json
    import subprocess
    env = dict(os.environ, SG_DIST_BACKEND='gloo', SG_SHARE_GPU='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr',
           '127.0.0.1', '--master-port', str(_free_port()), os.path.join(ROOT, 'bench.py'), '--gpus', str(world), '--steps',
           str(steps), '--warmup', '3', '--batch_per_gpu', str(per_gpu), '--full', '--no_secondary', '--no_legs', '--cpu_baseline',
           'off']
    if world == 2:
        cmd.append('--no_prof')
        env['SG_BENCH_QUICK'] = '1'
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, 'bench.py --gpus %d failed:\n%s\n%s' % (world, r.stdout[-3000:], r.stderr[-6000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{') and '"metric"' in ln]
    assert len(lines) == 1, 'exactly ONE JSON line from rank 0, got %d:\n%s' % (len(lines), r.stdout[-3000:])
    out = json.loads(lines[0])
    try:
        d = os.path.join(ROOT, 'gpurun_out')
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, 'bench_dp%d_gloo.json' % world), 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)
    except OSError:
        pass
    assert out['n_gpus'] == world and out['rccl_ranks'] == world and out['dist_backend'] == 'gloo'
    assert out['scaling'] == 'weak' and out['config']['global_batch'] == per_gpu * world and out['config']['parallelism'] == 'dp%d' % world
    assert out['steps'] == steps and out['warmup'] == 3 and out['value'] > 0 and out['ms_per_step'] > 0
    # ``value`` = whole-job images per second of the median timing block (max over ranks per block); the whole-region figure
    # (barrier + synchronize on both sides, max over ranks) rides along
    assert abs(out['value'] - per_gpu * world / (out['ms_per_step'] * 1e-3)) < 1e-6 * out['value']
    assert out['repeat']['blocks'] == min(5, steps) and sum(out['repeat']['steps_per_block']) == steps
    wr = out['whole_region']
    assert abs(wr['value'] - per_gpu * world * steps / wr['seconds']) < 1e-6 * wr['value'] and wr['ms_per_step'] > 0
    assert out['rccl']['backend'] == 'gloo' and 'torch_cuda_nccl_version' in out['rccl']
    ar = out['allreduce']
    assert ar['world'] == world
    # 764.7 MB of generator gradient in 64 MB buckets that close at parameter boundaries: 10 of them
    assert ar['G']['buckets'] >= 8 and ar['G']['bytes'] > 700e6 and ar['G']['overlap_mode'] is True
    for name in ('D_img', 'D_obj', 'D_mask'):
        assert ar[name]['buckets'] >= 1 and ar[name]['isolated_allreduce_ms'] > 0
    assert ar['overlap_fraction'] is not None and ar['overlap_fraction'] == ar['overlap_fraction']      # finite, not NaN
    assert ar['isolated_ms_per_step'] > 0 and ar['exposed_ms_per_step'] >= 0
    if world == 4:
        assert 'roofline' in out and out['roofline']['frac'] > 0
