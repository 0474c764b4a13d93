"""Parity of the hand-written HIP path (through the C ABI / ctypes) against the oracle on a real MI355X.

Integer / index work is compared bit-exactly (graph pool, crop permutation, one-hot, CSR); floating point within
the tolerance written at each assert (fp32; the MFMA f32 path is an exact k-ordered fma chain, differences come
from summation order only).  Sizes are chosen so the CPU oracle finishes in seconds; full-size (BASELINE config 2/5)
checks use size-independent properties.
"""
import os
import random

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import sg_oracle as O
from scene_generation_amd.synthetic import fill_deterministic, make_batch, make_vocab, batch_to
from scene_generation_amd.args import parser
from gpu_harness import _CLOSE_LOG, _dump, close
from gpu_harness import hip  # noqa: F401  (fixture)
from tools_det import det

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def _close_margins():
    """after the module: the 40 tightest relative-L2 margins of close() -> gpurun_out/close_margins.json (calibration record)"""
    yield
    worst = sorted(_CLOSE_LOG, key=lambda t: -t[0])[:40]
    _dump('close_margins.json', [{'ratio_of_bound': r, 'kind': k, 'name': n, 'tol': t} for r, k, n, t in worst])


# ------------------------------------------------------------------------------------------
# GEMM / conv kernels vs torch fp32 CPU
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', ['skinny', 'tiled'])
@pytest.mark.parametrize('rows,inf,outf,act', [(1, 7, 5, 0), (9, 163, 64, 1), (33, 454, 512, 1), (128, 512, 1152, 1),
                                               (70, 129, 33, 2), (16, 1024, 172, 0), (224, 454, 512, 1), (208, 512, 128, 1),
                                               (231, 1152, 454, 0), (1056, 512, 512, 1), (3, 2048, 4, 0), (40, 18, 90, 2)])
def test_linear(hip, rows, inf, outf, act, kernel):
    """nn.Linear forward / data gradient / weight gradient / bias gradient through BOTH dense kernels: the register-streaming
    one for small layers (skinny.hip: every operand form -- 16-, 8-, 4-byte K-contiguous loads, row-index-major loads -- K tails,
    K shorter than one round, ragged 32x32 tiles) and the LDS-tiled one (forced with the ``linear_skinny`` option at 0)."""
    from scene_generation_amd import _hip
    prev = _hip.get_option('linear_skinny')
    _hip.set_option('linear_skinny', (1 << 30) if kernel == 'skinny' else 0)
    try:
        _linear_case(hip, rows, inf, outf, act)
    finally:
        _hip.set_option('linear_skinny', prev)


def test_linear_kernels_are_deterministic_and_route_by_size(hip):
    """the skinny kernel adds its four k-partials in a fixed order: two runs are bit-identical; the default routing threshold
    sends the graph-conv shapes of BASELINE configs[1] to it and the 3072-row layers of configs[4] to the tiled kernel"""
    from scene_generation_amd import _hip
    assert _hip.get_option('linear_skinny') == 2048
    x, w, b = det((224, 454), 11).to(DEV), det((512, 454), 12, 0.1).to(DEV), det((512,), 13, 0.1).to(DEV)
    y1 = hip.linear(x, w, b, act=1)
    y2 = hip.linear(x, w, b, act=1)
    assert torch.equal(y1, y2)
    tiles = lambda M, N: ((M + 31) // 32) * ((N + 31) // 32)
    assert tiles(224, 1152) <= 2048 < tiles(3072, 1152)


def _linear_case(hip, rows, inf, outf, act):
    x, w, b = det((rows, inf), 1), det((outf, inf), 2, 0.1), det((outf,), 3, 0.1)
    gy = det((rows, outf), 4)
    xr, wr, br = [t.clone().requires_grad_() for t in (x, w, b)]
    yr = F.linear(xr, wr, br)
    yr = F.relu(yr) if act == 1 else (F.leaky_relu(yr, 0.2) if act == 2 else yr)
    yr.backward(gy)
    xg, wg, bg = [t.to(DEV).requires_grad_() for t in (x, w, b)]
    yg = hip.linear(xg, wg, bg, act=act, slope=0.2)
    yg.backward(gy.to(DEV))
    close(yg, yr, 2e-5, 'y')
    close(xg.grad, xr.grad, 2e-5, 'gx')
    close(wg.grad, wr.grad, 2e-5, 'gw')
    close(bg.grad, br.grad, 2e-5, 'gb')


CONV_CASES = [
    # (operator-level parity in fp32.  Which tile, loader, mask or split a shape runs on the forward gather -- and a float64 bound for
    #  each such plan, through the C ABI -- is the table of tests/forward_conv_cases.py, run by tests/test_gpu_forward_conv.py)
    # N, C1, C2, H, W, Cout, KS, stride, pad, reflect, ups, act
    (2, 5, 0, 12, 12, 8, 3, 1, 1, False, 1, 0),
    (2, 12, 0, 16, 16, 8, 7, 1, 3, True, 1, 1),        # ReflectionPad(3)+Conv7 (generators.py:68)
    (2, 8, 0, 16, 16, 16, 3, 2, 1, False, 1, 0),       # down-sampling conv
    (2, 16, 0, 8, 8, 16, 3, 1, 1, True, 1, 0),         # ResnetBlock conv
    (3, 7, 3, 17, 19, 8, 4, 2, 2, False, 1, 2),        # image-D first conv, concat folded, odd sizes
    (3, 8, 0, 9, 10, 16, 4, 1, 2, False, 1, 0),        # image-D k4 s1 p2
    (5, 3, 0, 32, 32, 8, 4, 2, 0, False, 1, 0),        # encoder C4-x-2 valid
    (5, 24, 0, 4, 4, 24, 3, 1, 1, False, 2, 0),        # mask_net: upsample folded
    (5, 24, 0, 8, 8, 1, 1, 1, 0, False, 1, 0),         # 1x1 head, Cout=1
    (5, 1, 0, 16, 16, 8, 3, 2, 1, False, 1, 2),        # mask-D first conv (K=9)
    (2, 64, 0, 16, 16, 3, 7, 1, 3, True, 1, 3),        # last G conv + tanh, Cout=3
    (3, 10, 0, 21, 20, 2, 7, 1, 3, True, 1, 3),        # direct small-M kernel: ragged tiles, Cout=2
    (2, 6, 0, 40, 136, 4, 7, 1, 3, True, 1, 0),        # direct small-M kernel: two column blocks, Cout=4
    (4, 130, 0, 8, 8, 140, 3, 1, 1, True, 1, 0),       # multi-tile M/N, ragged
    (2, 128, 0, 32, 32, 128, 3, 1, 1, False, 1, 0),    # big enough for the 128x128 tile
    (8, 128, 0, 8, 8, 128, 3, 1, 1, True, 1, 0),       # Winograd F(2x2,3x3) path (channels, tiles multiples of 128)
    (2, 256, 0, 16, 16, 128, 3, 1, 1, True, 1, 1),     # Winograd, Cin != Cout, fused ReLU
    (2, 128, 0, 16, 16, 256, 3, 1, 1, False, 1, 1),    # Winograd, ZERO padding (VGG19 convs), fused ReLU
    (8, 128, 0, 8, 12, 128, 3, 1, 1, False, 1, 0),     # zero padding, non-square plane; 8*4*6 = 192 tiles is no multiple of 128: the direct kernel (wino_tile() = 0)
    (3, 192, 0, 8, 8, 192, 3, 1, 1, False, 2, 0),      # folded x2 upsample, 192 channels (mask_net): no multiple of 128, the direct / sub-pixel kernels
    (4, 64, 0, 16, 16, 64, 3, 1, 1, False, 1, 1),      # 64 channels: stays on the direct kernel (VGG conv1_2)
    (2, 3, 0, 32, 32, 64, 3, 1, 1, False, 1, 1),       # VGG conv1_1
    (2, 16, 0, 15, 17, 8, 3, 2, 1, False, 1, 0),       # stride-2 dgrad: four parity classes of different sizes in one launch
    (8, 16, 0, 64, 64, 8, 3, 2, 1, False, 1, 0),       # stride-2 dgrad with >= 128 parity tiles in one tile row: classes dealt to the XCDs in chunks
    (2, 8, 0, 12, 12, 24, 4, 2, 1, False, 1, 0),       # k4 s2 p1: equal classes
    (3, 512, 0, 18, 18, 1, 4, 1, 2, False, 1, 0),      # PatchGAN score head (vector-ALU head kernels), full width
    (4, 40, 0, 9, 11, 1, 4, 1, 2, False, 1, 2),        # head kernels: ragged channel chunk, non-square, fused LeakyReLU
    (5, 64, 0, 8, 8, 1, 3, 1, 1, False, 1, 0),         # mask / object discriminator head (k3 p1)
    (6, 192, 0, 32, 32, 1, 1, 1, 0, False, 1, 0),      # mask_net 1x1 head at full size
    (7, 24, 0, 1, 1, 24, 3, 1, 1, False, 2, 0),        # mask_net first octave: 1x1 -> 2x2 (sub-pixel transposed conv)
    (3, 16, 0, 5, 7, 12, 3, 1, 1, False, 2, 0),        # sub-pixel transposed conv, odd non-square plane, Cin != Cout
    (9, 192, 0, 16, 16, 192, 3, 1, 1, False, 2, 0),    # mask_net last octave at full width (192 channels, 16 -> 32)
    (8, 128, 0, 17, 17, 128, 4, 1, 2, False, 1, 2),    # Winograd F(2x2,4x4): PatchGAN k4 s1 p2 (17 -> 18), fused LeakyReLU
    (8, 128, 0, 20, 14, 256, 4, 1, 1, False, 1, 0),    # F(2x2,4x4): pad 1, odd 19x13 output (clipped edge tiles), Cin != Cout
    (8, 256, 0, 19, 19, 128, 4, 1, 0, False, 1, 1),    # F(2x2,4x4): valid conv, data gradient with padding 3, k-chunked wgrad
    # (the chunking of the weight gradient -- chunk counts, the cap, XCD padding -- is asserted plan by plan against float64 in
    #  tests/wgrad_cases.py: row g_64x3_k4s2_32x32 is the next shape at the C ABI)
    (6, 3, 0, 64, 64, 64, 4, 2, 1, False, 1, 2),       # crop-D first conv: few-channel wgrad in 48 k-chunks (wide slab reduce)
    (40, 3, 0, 64, 64, 64, 4, 2, 1, False, 1, 2),      # the same at ~200 crops: the 256-chunk cap, XCD-padded chunk count
    (16, 128, 0, 8, 8, 128, 3, 1, 1, True, 1, 0),      # Winograd F(4x4,3x3): 16 * 2 * 2 = 64 tiles of 4x4 outputs (one 64-column GEMM tile)
    (8, 256, 0, 16, 16, 128, 3, 1, 1, True, 1, 1),     # F(4x4,3x3) at 16x16 planes (configs[3] trunk), Cin != Cout, fused ReLU
    (32, 128, 0, 8, 8, 256, 3, 1, 1, True, 1, 2),      # F(4x4,3x3): the benchmark's tile count (128), Cout > Cin, fused LeakyReLU
]


@pytest.mark.parametrize('case', CONV_CASES)
def test_conv2d(hip, case):
    _conv2d_case(hip, case, one_signed=False)


@pytest.mark.parametrize('case', [c for c in CONV_CASES if c[-1] in (1, 2)])
def test_conv2d_act_backward_independent_of_the_gpu_mask(hip, case):
    """the (Leaky)ReLU cases of test_conv2d hand the reference backward the GPU's derivative mask (after
    bounding the units the two masks disagree on), so their gradient check is not independent of the implementation under test.
    Here the operands are built so that NO pre-activation is near the kink -- positive inputs, every output channel's weights and
    bias of one sign (channels alternate) => |y_pre| is a sum of same-signed terms, >= 1e-3 of the scale everywhere (asserted)
    -- and the reference backward is plain autograd through its OWN activation: same kernels, same shapes, same tolerances, no
    borrowed mask.  Negative channels exercise the zero (ReLU) / slope (LeakyReLU) branch, positive ones the identity."""
    _conv2d_case(hip, case, one_signed=True)


def _conv2d_case(hip, case, one_signed):
    N, C1, C2, H, W, Cout, KS, stride, pad, reflect, ups, act = case
    x1, w = det((N, C1, H, W), 11), det((Cout, C1 + C2, KS, KS), 12, 0.2)
    x2 = det((N, C2, H, W), 13) if C2 else None
    b = det((Cout,), 14, 0.2)
    if one_signed:
        sgn = torch.where(torch.arange(Cout) % 2 == 0, torch.tensor(1.0), torch.tensor(-1.0))
        x1 = x1.abs() + 0.25
        x2 = (x2.abs() + 0.25) if C2 else None
        w = (w.abs() + 0.01) * sgn.view(-1, 1, 1, 1)
        b = (b.abs() + 0.05) * sgn
    r1, rw, rb = [t.clone().requires_grad_() for t in (x1, w, b)]
    r2 = x2.clone().requires_grad_() if C2 else None
    xin = torch.cat([r1, r2], 1) if C2 else r1
    if ups == 2:
        xin = F.interpolate(xin, scale_factor=2, mode='nearest')
    if reflect:
        yr = F.conv2d(F.pad(xin, (pad,) * 4, mode='reflect'), rw, rb, stride=stride)
    else:
        yr = F.conv2d(xin, rw, rb, stride=stride, padding=pad)
    ypre = yr
    yr = {0: lambda t: t, 1: F.relu, 2: lambda t: F.leaky_relu(t, 0.2), 3: torch.tanh}[act](ypre)
    gy = det(tuple(yr.shape), 15)
    g1, gw, gb = [t.to(DEV).requires_grad_() for t in (x1, w, b)]
    g2 = x2.to(DEV).requires_grad_() if C2 else None
    yg = hip.conv2d(g1, gw, gb, stride=stride, pad=pad, reflect=reflect, upsample=ups, act=act, slope=0.2, x2=g2)
    yg.backward(gy.to(DEV))
    if one_signed:
        margin = float(ypre.detach().abs().min()) / max(1.0, float(ypre.detach().abs().max()))
        assert margin >= 1e-3, 'construction failed: a pre-activation within %g of the kink' % margin
        yr.backward(gy)                              # the reference's own activation derivative: no mask from the GPU
    elif act in (1, 2):
        # (Leaky)ReLU: a unit whose pre-activation is within rounding error of 0 may sit on the other side of the kink in two
        # correct fp32 implementations, and ONE such unit moves a gradient entry by |w gy| ~ 0.1 (seen with Winograd F(4x4,3x3),
        # whose forward error is ~1e-5 of the scale: a few of 262 144 units flip).  The reference backward therefore uses the
        # derivative mask of the GPU result -- after checking that every unit the two masks disagree on IS within the forward
        # tolerance of 0.
        lo = 0.0 if act == 1 else 0.2
        dg = torch.where(yg.detach().cpu() > 0, torch.tensor(1.0), torch.tensor(lo))
        dr = torch.where(ypre.detach() > 0, torch.tensor(1.0), torch.tensor(lo))
        flipped = dg != dr
        assert float(ypre.detach()[flipped].abs().max() if flipped.any() else 0.0) <= 3e-5 * max(1.0, float(yr.detach().abs().max()))
        assert int(flipped.sum()) <= 1e-4 * flipped.numel() + 2
        ypre.backward(gy * dg)
    else:
        yr.backward(gy)
    close(yg, yr, 3e-5, 'y')
    close(g1.grad, r1.grad, 5e-5, 'gx1')
    if C2:
        close(g2.grad, r2.grad, 5e-5, 'gx2')
    close(gw.grad, rw.grad, 5e-5, 'gw')
    close(gb.grad, rb.grad, 5e-5, 'gb')


def test_winograd_f43_trunk_shape_vs_f23_and_fp64(hip):
    """The 1024-channel 8x8 ResnetBlock conv of the generator trunk (generators.py:80-82, layers.py:251-270) at N = 16: Winograd
    F(4x4,3x3) (the default since round 5) and F(2x2,3x3) (wino43 = 0) against an fp64 reference -- forward, data gradient,
    weight and bias gradient.  Both must hold the conv tolerances of the suite; the measured errors of the two forms go to
    gpurun_out/winograd_f43_errors.json (conv-level error of F(4x4,3x3) <= 2x the asserted bounds)."""
    from scene_generation_amd import _hip
    N, C, H = 16, 1024, 8
    x, w, b = det((N, C, H, H), 311), det((C, C, 3, 3), 312, 0.05), det((C,), 313, 0.2)
    gy = det((N, C, H, H), 314)
    xr, wr, br = [t.double().requires_grad_() for t in (x, w, b)]
    yr = F.conv2d(F.pad(xr, (1,) * 4, mode='reflect'), wr, br)
    yr.backward(gy.double())
    errs = {}
    saved = _hip.get_option('wino43')
    try:
        for form, flag in (('f43', 1), ('f23', 0)):
            _hip.set_option('wino43', flag)
            xg, wg, bg = [t.to(DEV).requires_grad_() for t in (x, w, b)]
            yg = hip.conv2d(xg, wg, bg, pad=1, reflect=True)
            yg.backward(gy.to(DEV))
            for name, got, want, tol in (('y', yg, yr, 3e-5), ('gx', xg.grad, xr.grad, 5e-5), ('gw', wg.grad, wr.grad, 5e-5),
                                         ('gb', bg.grad, br.grad, 5e-5)):
                e = float((got.detach().double().cpu() - want.detach()).abs().max() / want.detach().abs().max())
                errs['%s_%s' % (form, name)] = e
                close(got, want.detach().float(), tol, '%s %s' % (form, name))
    finally:
        _hip.set_option('wino43', saved)
    _dump('winograd_f43_errors.json', errs)
    # per-layer error budget of the trunk conv (all 18 trunk convs have this shape): ~2x what the form measures
    # with the channel sum accumulated in 256-chunks (TileCfg::KFOLD, round 6: y 3.4e-6, gx 2.4e-6, gw 2.9e-6 of the maxima -- one
    # fma chain over 1024 channels gave 9.9e-6 / 6.0e-6).  A regression of the accumulation order shows HERE, not as a whole-step drift.
    for name, bound in (('y', 7e-6), ('gx', 5e-6), ('gw', 6e-6)):
        assert errs['f43_' + name] <= bound, errs


def test_winograd_f43_tail_split_at_the_benchmark_shape(hip):
    """N = 32: the 36 x 32 = 1152 tiles of the F(4x4,3x3) forward / data-gradient GEMMs leave half a round of workgroups per CU on
    the 256 CUs of an MI355X, and the launch runs the tail-split schedule (igemm_kernel, TileCfg::TAILSPLIT: the tiles of the half
    round as two workgroups of half the channel range, the last arriver adds the other's accumulators).  Against an fp64
    reference at the per-layer budget of the trunk conv, and against the plain schedule (option w43_tail_split = 0): the two differ
    only in where the 256-chunks of the channel sum meet ((c0 + c1) + (c2 + c3) instead of ((c0 + c1) + c2) + c3 in 128 of the
    1152 tiles).  Ten repeats of the split launch are bit-identical (whichever half arrives last, x + y = y + x)."""
    from scene_generation_amd import _hip
    N, C, H = 32, 1024, 8
    x, w, b = det((N, C, H, H), 321), det((C, C, 3, 3), 322, 0.05), det((C,), 323, 0.2)
    gy = det((N, C, H, H), 324)
    xr, wr, br = [t.double().requires_grad_() for t in (x, w, b)]
    yr = F.conv2d(F.pad(xr, (1,) * 4, mode='reflect'), wr, br)
    yr.backward(gy.double())
    saved = _hip.get_option('w43_tail_split')
    res = {}
    try:
        for flag in (1, 0):
            _hip.set_option('w43_tail_split', flag)
            xg, wg, bg = [t.to(DEV).requires_grad_() for t in (x, w, b)]
            yg = hip.conv2d(xg, wg, bg, pad=1, reflect=True)
            yg.backward(gy.to(DEV))
            res[flag] = (yg.detach().clone(), xg.grad.clone(), wg.grad.clone())
            for name, got, want, bound in (('y', yg, yr, 7e-6), ('gx', xg.grad, xr.grad, 5e-6), ('gw', wg.grad, wr.grad, 6e-6)):
                e = float((got.detach().double().cpu() - want.detach()).abs().max() / want.detach().abs().max())
                assert e <= bound, (flag, name, e)
            if flag == 1:
                for _ in range(10):
                    x2 = x.to(DEV).requires_grad_()
                    y2 = hip.conv2d(x2, wg.detach(), bg.detach(), pad=1, reflect=True)
                    y2.backward(gy.to(DEV))
                    assert torch.equal(y2, res[1][0]) and torch.equal(x2.grad, res[1][1])
    finally:
        _hip.set_option('w43_tail_split', saved)
    for a, c, name in zip(res[1], res[0], ('y', 'gx', 'gw')):
        d = float((a - c).abs().max() / c.abs().max())
        assert d <= 2e-6, (name, d)
    assert not torch.equal(res[1][0], res[0][0]) or not torch.equal(res[1][1], res[0][1]), 'the split schedule did not run'


@pytest.mark.parametrize('shape', [(32, 64, 65, 65, 128, 4, 2, 2), (24, 192, 16, 16, 192, 3, 1, 1), (32, 124, 33, 33, 256, 4, 2, 2)])
def test_tail_split_general_form_vs_plain_schedule(hip, shape):
    """Option w43_tail_split = 2 (the default since the end of round 6): a plain conv GEMM launch whose last round of resident workgroups is ragged runs its last
    tiles as 2-4 workgroups of a fraction of the k range each; the last arriver re-reads all dumps and adds them in piece order.  At
    layer shapes of the step (PatchGAN scale-0 convs, an object-side 3x3 conv): forward and data gradient equal the plain schedule to
    fp32 summation order, and five repeats are bit-identical (the combine order does not depend on who arrives last).  That the
    forward launch took the split schedule is read from the ticket ring (sg_runtime_state): it drew counters in mode 2 and none in
    mode 0.  (The third shape had 128 input channels until the ring was looked at: K = 2048 reaches split_kmin, the launch runs
    split-K in both modes and the tail split never applied -- the test compared the plain schedule with itself; 124 channels keep
    the 580 tiles and stay below split_kmin.)"""
    from scene_generation_amd import _hip
    N, C, H, W, Cout, KS, stride, pad = shape
    x, w, b = det((N, C, H, W), 331), det((Cout, C, KS, KS), 332, 0.05), det((Cout,), 333, 0.2)
    saved = _hip.get_option('w43_tail_split')
    out = {}
    try:
        for mode in (2, 0):
            _hip.set_option('w43_tail_split', mode)
            reps = []
            for _ in range(5 if mode == 2 else 1):
                xg, wg, bg = [t.to(DEV).requires_grad_() for t in (x, w, b)]
                s0 = hip.runtime_state()
                yg = hip.conv2d(xg, wg, bg, stride=stride, pad=pad)
                s1 = hip.runtime_state()
                drew = (s1['ring_laps'], s1['ring_at']) != (s0['ring_laps'], s0['ring_at'])
                assert drew == (mode == 2), 'w43_tail_split = %d: the forward launch drew %s (ring %r -> %r)' % (
                    mode, 'counters' if drew else 'no counters', s0, s1)
                yg.backward(det(tuple(yg.shape), 334).to(DEV))
                reps.append((yg.detach().clone(), xg.grad.clone(), wg.grad.clone()))
            for r in reps[1:]:
                assert all(torch.equal(a, c) for a, c in zip(r, reps[0]))
            out[mode] = reps[0]
    finally:
        _hip.set_option('w43_tail_split', saved)
    for a, c, name in zip(out[2], out[0], ('y', 'gx', 'gw')):
        close(a, c, 2e-6, 'tail split ' + name)


@pytest.mark.parametrize('kind,N,Cin,Cout,H', [('up', 32, 512, 256, 8), ('up', 32, 256, 128, 16), ('down', 32, 256, 512, 16), ('up', 2, 512, 256, 8)])
def test_parity_class_split_vs_plain_schedule(hip, kind, N, Cin, Cout, H):
    """Option par_split (default on): 3x3 stride-2 transposed gathers -- the forward of the generator's up path (generators.py:84-87)
    and the data gradient of its stride-2 encoder convs (generators.py:73-76) -- run as four parity classes of 4 / 2 / 2 / 1 taps;
    with few tiles the 4-tap class's tiles run as two half-k workgroups that meet through the tail-split ticket (igemm_core.h,
    ParityClasses::split).  At the step's shapes (and at the two-image shapes of the multi-rank bench case): against torch fp32, against
    the unsplit schedule to fp32 summation order, and five repeats bit-identical (the sum of the two halves does not depend on who
    arrives last).  That the launch with the parity classes (the forward of 'up', the data gradient of 'down') took the split
    schedule is read from the ticket ring (sg_runtime_state): it drew counters with par_split = 1 and none with par_split = 0."""
    from scene_generation_amd import _hip
    saved = _hip.get_option('par_split')
    if kind == 'up':
        x, w, b = det((N, Cin, H, H), 341), det((Cin, Cout, 3, 3), 342, 0.05), det((Cout,), 343, 0.2)
        ref = lambda xr, wr, br: F.conv_transpose2d(xr, wr, br, stride=2, padding=1, output_padding=1)
        run = lambda xg, wg, bg: hip.conv_transpose2d(xg, wg, bg, stride=2, pad=1, out_pad=1)
    else:
        x, w, b = det((N, Cin, H, H), 344), det((Cout, Cin, 3, 3), 345, 0.05), det((Cout,), 346, 0.2)
        ref = lambda xr, wr, br: F.conv2d(xr, wr, br, stride=2, padding=1)
        run = lambda xg, wg, bg: hip.conv2d(xg, wg, bg, stride=2, pad=1)
    xr, wr, br = [t.clone().requires_grad_() for t in (x, w, b)]
    yr = ref(xr, wr, br)
    gy = det(tuple(yr.shape), 347)
    yr.backward(gy)
    out = {}
    try:
        for mode in (1, 0):
            _hip.set_option('par_split', mode)
            reps = []
            for _ in range(5 if mode == 1 else 1):
                xg, wg, bg = [t.to(DEV).requires_grad_() for t in (x, w, b)]
                gyg = gy.to(DEV)
                s0 = hip.runtime_state()
                yg = run(xg, wg, bg)
                s1 = hip.runtime_state()
                yg.backward(gyg)
                s2 = hip.runtime_state()
                a, c = (s0, s1) if kind == 'up' else (s1, s2)          # the launch that carries the parity classes
                drew = (c['ring_laps'], c['ring_at']) != (a['ring_laps'], a['ring_at'])
                assert drew == (mode == 1), 'par_split = %d: the parity-class launch drew %s (ring %r -> %r)' % (
                    mode, 'counters' if drew else 'no counters', a, c)
                reps.append((yg.detach().clone(), xg.grad.clone(), wg.grad.clone()))
            for r in reps[1:]:
                assert all(torch.equal(a, c) for a, c in zip(r, reps[0]))
            out[mode] = reps[0]
            for a, c, name in zip(reps[0], (yr, xr.grad, wr.grad), ('y', 'gx', 'gw')):
                close(a, c, 5e-5, 'par_split=%d %s' % (mode, name))
    finally:
        _hip.set_option('par_split', saved)
    for a, c, name in zip(out[1], out[0], ('y', 'gx', 'gw')):
        close(a, c, 2e-6, 'parity split ' + name)


@pytest.mark.parametrize('N,C,H,Cout,act,with_skip', [(16, 128, 8, 128, 1, True), (8, 128, 16, 256, 2, False), (32, 256, 8, 128, 0, True)])
def test_conv_instnorm_fused_vs_fp64_and_unfused(hip, N, C, H, Cout, act, with_skip):
    """ReflectionPad(1) + Conv3x3 + InstanceNorm (+ ReLU / LeakyReLU) (+ residual) of a ResnetBlock (layers.py:251-270) as the fused
    Winograd F(4x4,3x3) operator (output transform + norm in one launch, norm backward + gradient transform in one) against an
    fp64 reference and against the unfused pair of operators: output, input / weight / bias / skip gradients; 8x8 planes (one
    tile per thread) and 16x16 planes (four)."""
    from scene_generation_amd import _hip
    assert hip.conv_instnorm_fusable(torch.empty(N, C, H, H, device=DEV), torch.empty(Cout, C, 3, 3), 1, 1, 0)
    x, w, b = det((N, C, H, H), 411), det((Cout, C, 3, 3), 412, 0.1), det((Cout,), 413, 0.2)
    skip = det((N, Cout, H, H), 414) if with_skip else None
    gy = det((N, Cout, H, H), 415)
    xr, wr, br = [t.double().requires_grad_() for t in (x, w, b)]
    sr = skip.double().requires_grad_() if with_skip else None
    yr = F.instance_norm(F.conv2d(F.pad(xr, (1,) * 4, mode='reflect'), wr, br), eps=1e-5)
    zr = yr
    yr = {0: lambda t: t, 1: F.relu, 2: lambda t: F.leaky_relu(t, 0.2)}[act](yr)
    if with_skip:
        yr = yr + sr
    res = {}
    for fused in (1, 0):
        _hip.set_option('wino_in_fuse', fused)
        try:
            xg, wg, bg = [t.to(DEV).requires_grad_() for t in (x, w, b)]
            sg = skip.to(DEV).requires_grad_() if with_skip else None
            if fused:
                yg = hip.conv2d_instnorm(xg, wg, bg, skip=sg, eps=1e-5, act=act, slope=0.2)
            else:
                yg = hip.instance_norm(hip.conv2d(xg, wg, bg, pad=1, reflect=True), skip=sg, eps=1e-5, act=act, slope=0.2)
            if act and not res:
                # the reference backward takes the derivative mask of the first GPU result (units within rounding of the kink)
                lo = 0.0 if act == 1 else 0.2
                pre = (yg.detach().cpu().double() - (skip.double() if with_skip else 0.0))
                dg = torch.where(pre > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(lo, dtype=torch.float64))
                flipped = dg != torch.where(zr.detach() > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(lo, dtype=torch.float64))
                assert float(zr.detach()[flipped].abs().max() if flipped.any() else 0.0) <= 1e-4
                torch.autograd.backward([zr] + ([sr] if with_skip else []), [gy.double() * dg] + ([gy.double()] if with_skip else []))
            elif not res:
                yr.backward(gy.double())
            yg.backward(gy.to(DEV))
            res[fused] = (yg.detach(), xg.grad, wg.grad, bg.grad, sg.grad if with_skip else None)
        finally:
            _hip.set_option('wino_in_fuse', 1)
    for fused in (1, 0):
        yg, gx, gw, gb, gs = res[fused]
        tag = 'fused' if fused else 'unfused'
        close(yg, yr.detach().float(), 5e-5, tag + ' out')
        close(gx, xr.grad.float(), 1e-4, tag + ' gx')
        close(gw, wr.grad.float(), 1e-4, tag + ' gw')
        if with_skip:
            close(gs, sr.grad.float(), 1e-6, tag + ' gskip')
    # the conv bias is followed by a mean subtraction: its gradient is rounding noise around 0 in every implementation
    assert float(res[1][3].abs().max()) <= 1e-3 * float(gy.abs().sum(dim=(0, 2, 3)).max())
    close(res[1][0], res[0][0], 2e-5, 'fused vs unfused out')
    close(res[1][1], res[0][1], 5e-5, 'fused vs unfused gx')


@pytest.mark.parametrize('N,C,dense,H,Cout,KS,stride,pad,reflect,C2', [
    (5, 40, 6, 16, 64, 7, 1, 3, True, 0),      # generator stem: mask-free 64x64 tiles
    (3, 30, 4, 11, 24, 3, 1, 1, False, 0),     # ragged everything, zero padding
    (4, 24, 3, 9, 8, 4, 2, 2, False, 0),       # strided, 32-row tile, images of 25 pixels
    (2, 64, 8, 32, 128, 3, 1, 1, True, 0),
    (3, 40, 5, 17, 64, 4, 2, 2, False, 3),     # image-D first conv: layout | image, odd output grid (9x9)
    (2, 36, 4, 16, 16, 4, 2, 2, False, 3),
])
def test_conv2d_channel_sparse(hip, N, C, dense, H, Cout, KS, stride, pad, reflect, C2):
    """sg_conv2d_fwd_sparse / sg_conv2d_wgrad_sparse == the dense conv when every unlisted channel is zero."""
    from scene_generation_amd.utils import active_layout_channels
    num_objs = C - dense
    rng = np.random.RandomState(7)
    objs, o2i = [], []
    for n in range(N):
        k = rng.randint(1, 5)
        objs += list(rng.randint(0, num_objs, size=k)); o2i += [n] * k
    cl, cc = active_layout_channels(objs, o2i, N, num_objs, dense)
    x = det((N, C, H, H), 51)
    keep = torch.zeros(N, C)
    for n in range(N):
        keep[n, torch.from_numpy(cl[n, :cc[n]]).long()] = 1
    x = x * keep.view(N, C, 1, 1)
    x2 = det((N, C2, H, H), 55) if C2 else None
    w, b = det((Cout, C + C2, KS, KS), 52, 0.2), det((Cout,), 53, 0.2)
    xr, wr, br = [t.clone().requires_grad_() for t in (x, w, b)]
    x2r = x2.clone().requires_grad_() if C2 else None
    xin = torch.cat([xr, x2r], 1) if C2 else xr
    if reflect:
        yr = F.conv2d(F.pad(xin, (pad,) * 4, mode='reflect'), wr, br, stride=stride)
    else:
        yr = F.conv2d(xin, wr, br, stride=stride, padding=pad)
    yr = F.relu(yr)
    gy = det(tuple(yr.shape), 54)
    yr.backward(gy)
    xg, wg, bg = [t.to(DEV).requires_grad_() for t in (x, w, b)]
    x2g = x2.to(DEV).requires_grad_() if C2 else None
    if C2:
        cl, cc = active_layout_channels(objs, o2i, N, num_objs, dense, extra=C2)
        hip.set_hints(xg, sparse_cat={C2: (torch.from_numpy(cl).to(DEV), torch.from_numpy(cc).to(DEV))})
    else:
        hip.set_hints(xg, sparse=(torch.from_numpy(cl).to(DEV), torch.from_numpy(cc).to(DEV)))
    assert 2 * cl.shape[1] <= C
    yg = hip.conv2d(xg, wg, bg, stride=stride, pad=pad, reflect=reflect, act=1, x2=x2g)
    yg.backward(gy.to(DEV))
    close(yg, yr, 3e-5, 'y')
    close(xg.grad, xr.grad, 5e-5, 'gx')
    if C2:
        close(x2g.grad, x2r.grad, 5e-5, 'gx2')
    close(wg.grad, wr.grad, 5e-5, 'gw')
    close(bg.grad, br.grad, 5e-5, 'gb')


@pytest.mark.parametrize('KS,stride,pad,reflect,C2,H', [(7, 1, 3, True, 0, 32), (4, 2, 2, False, 3, 32), (3, 1, 1, False, 0, 16),
                                                       (4, 2, 2, False, 3, 17), (7, 1, 3, True, 0, 64)])
def test_factored_layout_conv_matches_dense(hip, KS, stride, pad, reflect, C2, H):
    """conv over a masks_to_layout() layout computed from its factored form (planes S_o + per-object filters) == the dense
    conv over the materialised layout: outputs, weight / bias / appearance-vector / second-source gradients."""
    from scene_generation_amd.layout import masks_to_layout
    num_objs, R, Cout = 14, 6, (64 if H == 64 else 16)
    b = make_batch(N=4, min_objs=2, max_objs=6, size=H, mask_size=8, num_objs=num_objs, seed=21)
    O_ = b.objs.numel()
    objs, o2i = b.objs.to(DEV), b.obj_to_img.to(DEV)
    rep0 = det((O_, R), 91).abs()
    w0, b0 = det((Cout, num_objs + R + C2, KS, KS), 92, 0.2), det((Cout,), 93, 0.2)
    x20 = det((4, C2, H, H), 94) if C2 else None
    outs = []
    for factored in (False, True):
        rep = rep0.to(DEV).requires_grad_()
        w, bias = w0.to(DEV).requires_grad_(), b0.to(DEV).requires_grad_()
        x2 = x20.to(DEV).requires_grad_() if C2 else None
        vecs = hip.concat_cols(hip.one_hot(objs, num_objs), rep)
        layout = masks_to_layout(vecs, b.boxes.to(DEV), b.masks.to(DEV), o2i, H, num_images=4, validate=False)
        if factored:
            counts, plane = [0] * 4, []
            for i in b.obj_to_img.tolist():
                plane.append(counts[i]); counts[i] += 1
            pidx = torch.tensor(plane, device=DEV)
            Z = hip.layout_planes(b.boxes.to(DEV), b.masks.to(DEV), hip.segment_offsets(o2i, 4), pidx, 4, max(counts), H, H)
            hip.set_hints(layout, factored=hip.FactoredLayout(Z, objs, vecs[:, num_objs:], num_objs, o2i, pidx, counts))
        y = hip.conv2d(layout, w, bias, stride=stride, pad=pad, reflect=reflect, act=2, slope=0.2, x2=x2)
        (y * det(tuple(y.shape), 95).to(DEV)).sum().backward()
        outs.append((y.detach(), w.grad, bias.grad, rep.grad, None if x2 is None else x2.grad))
    names = ['y', 'gw', 'gb', 'g_repr', 'g_x2']
    for nme, a, r in zip(names, outs[1], outs[0]):
        if r is not None:
            close(a, r.cpu(), 1e-4, nme)


@pytest.mark.parametrize('fold', [True, False])
@pytest.mark.parametrize('shape', [
    # N, C1, C2, H, W, Cout, KS, stride, pad, act, one_hot
    (6, 16, 12, 8, 8, 8, 3, 1, 1, 0, True),              # the round-1 case
    (7, 128, 172, 8, 8, 256, 3, 1, 1, 0, True),          # the mask discriminator's conditioned conv at its real widths
    (8, 128, 172, 8, 8, 256, 3, 1, 1, 2, True),          # ... with a multiple of 8 objects (the shape Winograd would take), LeakyReLU
    (5, 128, 172, 4, 4, 256, 3, 1, 1, 2, True),          # ... at the coarser scale (every pixel is a border pixel), fused LeakyReLU
    (4, 24, 10, 9, 7, 40, 3, 2, 1, 2, False),            # stride 2, odd plane, a dense condition row with its own gradient
    (3, 20, 6, 6, 5, 12, 4, 1, 2, 0, False),             # 4x4 kernel, padding 2 (output larger than the input)
    (3, 8, 5, 5, 5, 16, 1, 1, 0, 1, False),              # 1x1 kernel: the folded term is a per-sample bias
])
def test_conv2d_broadcast_second_source(hip, shape, fold):
    """mask-D: the class row broadcast over the grid == expand()+cat() of discriminators.py:107-110 -- as a second gather source
    of the full-width conv (fold off) and folded into a per-(sample, channel, tap) term of the C1-channel conv (ops.CondConv2dFn,
    the default): y, dx, dcond, dW (both channel blocks) and db against torch fp32 on the CPU."""
    N, C1, C2, H, W, Cout, KS, stride, pad, act, one_hot = shape
    x, w, b = det((N, C1, H, W), 21), det((Cout, C1 + C2, KS, KS), 22, 0.2), det((Cout,), 23)
    if one_hot:
        cond = torch.zeros(N, C2)
        cond[torch.arange(N), torch.tensor([0, 3, 11, 5, 5, 1, 9, 2][:N]) % C2] = 1
    else:
        cond = det((N, C2), 25)
    xr, wr, br, cr = (t.clone().requires_grad_() for t in (x, w, b, cond))
    yr = F.conv2d(torch.cat([xr, cr.view(N, C2, 1, 1).expand(-1, -1, H, W)], 1), wr, br, stride=stride, padding=pad)
    yr = {0: yr, 1: F.relu(yr), 2: F.leaky_relu(yr, 0.2)}[act]
    gy = det(tuple(yr.shape), 24)
    yr.backward(gy)
    saved = hip.COND_FOLD
    hip.COND_FOLD = fold
    try:
        xg, wg, bg, cg = (t.to(DEV).requires_grad_() for t in (x, w, b, cond))
        yg = hip.conv2d(xg, wg, bg, stride=stride, pad=pad, act=act, slope=0.2, x2=cg)
        assert (type(yg.grad_fn).__name__ == 'CondConv2dFnBackward') == fold
        yg.backward(gy.to(DEV))
    finally:
        hip.COND_FOLD = saved
    close(yg, yr, 3e-5)
    close(xg.grad, xr.grad, 5e-5, 'gx')
    close(wg.grad[:, :C1], wr.grad[:, :C1], 5e-5, 'gw1')
    close(wg.grad[:, C1:], wr.grad[:, C1:], 5e-5, 'gw2')
    close(bg.grad, br.grad, 5e-5, 'gb')
    close(cg.grad, cr.grad, 5e-5, 'gcond')


def test_upconv_subpixel_form_equals_folded_upsample_gather(hip):
    """Interpolate(x2)+Conv3x3 (generators.py:20-21): the sub-pixel transposed-conv form (ops.UpConv3Fn, the default) against
    the 3x3 gather over the folded upsample (SG_UPCONV=0) -- same results to fp32 round-off, forward and all gradients."""
    x, w, b = det((6, 40, 8, 8), 41), det((24, 40, 3, 3), 42, 0.2), det((24,), 43, 0.2)
    gy = det((6, 24, 16, 16), 44).to(DEV)
    res = []
    saved = hip.UPCONV
    try:
        for flag in (True, False):
            hip.UPCONV = flag
            xg, wg, bg = [t.to(DEV).requires_grad_() for t in (x, w, b)]
            y = hip.conv2d(xg, wg, bg, stride=1, pad=1, upsample=2)
            y.backward(gy)
            res.append((y, xg.grad, wg.grad, bg.grad))
    finally:
        hip.UPCONV = saved
    for a, c, name in zip(res[0], res[1], ('y', 'gx', 'gw', 'gb')):
        close(a, c, 2e-5, name)


# (8, 64, 32, 32): one tile row (Cout <= 64) and 4 x 128 pixel tiles of 64 -- the launch shape whose parity classes are dealt to the XCDs in
#  chunks (BatchInfo::par_chunk: the forward of generators.py:84-87 at 64x64 -> 128x128 ran all 4-tap tiles on two XCDs)
@pytest.mark.parametrize('N,Cin,Cout,H', [(2, 16, 8, 8), (3, 32, 16, 5), (2, 128, 64, 16), (8, 64, 32, 32)])
def test_conv_transpose2d(hip, N, Cin, Cout, H):
    x, w, b = det((N, Cin, H, H), 31), det((Cin, Cout, 3, 3), 32, 0.2), det((Cout,), 33, 0.2)
    xr, wr, br = [t.clone().requires_grad_() for t in (x, w, b)]
    yr = F.conv_transpose2d(xr, wr, br, stride=2, padding=1, output_padding=1)
    gy = det(tuple(yr.shape), 34)
    yr.backward(gy)
    xg, wg, bg = [t.to(DEV).requires_grad_() for t in (x, w, b)]
    yg = hip.conv_transpose2d(xg, wg, bg, stride=2, pad=1, out_pad=1)
    yg.backward(gy.to(DEV))
    close(yg, yr, 3e-5, 'y')
    close(xg.grad, xr.grad, 5e-5, 'gx')
    close(wg.grad, wr.grad, 5e-5, 'gw')
    close(bg.grad, br.grad, 5e-5, 'gb')


# ------------------------------------------------------------------------------------------
# normalisation / pooling
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,act,skip', [((3, 5, 8, 8), 1, False), ((2, 4, 40, 40), 0, True), ((2, 3, 7, 9), 2, False)])
def test_instance_norm(hip, shape, act, skip):
    x, gy = det(shape, 41, 2.0, 0.3), det(shape, 42)
    sk = det(shape, 43) if skip else None
    xr = x.clone().requires_grad_()
    sr = sk.clone().requires_grad_() if skip else None
    yr = F.instance_norm(xr, eps=1e-5)
    yr = F.relu(yr) if act == 1 else (F.leaky_relu(yr, 0.2) if act == 2 else yr)
    yr = yr + sr if skip else yr
    yr.backward(gy)
    xg = x.to(DEV).requires_grad_()
    sg = sk.to(DEV).requires_grad_() if skip else None
    yg = hip.instance_norm(xg, skip=sg, act=act, slope=0.2)
    yg.backward(gy.to(DEV))
    close(yg, yr, 2e-5, 'y')
    close(xg.grad, xr.grad, 1e-4, 'gx')
    if skip:
        close(sg.grad, sr.grad, 1e-6, 'gskip')


@pytest.mark.parametrize('shape,act,training', [((6, 5, 4, 4), 1, True), ((37, 8, 1, 1), 2, True), ((4, 3, 9, 9), 0, False)])
def test_batch_norm(hip, shape, act, training):
    C = shape[1]
    x, gy = det(shape, 51, 2.0, 0.3), det(shape, 52)
    ref = nn.BatchNorm2d(C)
    fill_deterministic(ref)
    ref.train(training)
    xr = x.clone().requires_grad_()
    yr = ref(xr)
    yr = F.relu(yr) if act == 1 else (F.leaky_relu(yr, 0.2) if act == 2 else yr)
    yr.backward(gy)
    from scene_generation_amd.layers import BatchNorm2d
    m = BatchNorm2d(C)
    fill_deterministic(m)
    m = m.to(DEV).train(training)
    xg = x.to(DEV).requires_grad_()
    yg = m(xg, act=act, slope=0.2)
    yg.backward(gy.to(DEV))
    close(yg, yr, 2e-5, 'y')
    close(xg.grad, xr.grad, 1e-4, 'gx')
    close(m.weight.grad, ref.weight.grad, 1e-4, 'ggamma')
    close(m.bias.grad, ref.bias.grad, 1e-4, 'gbeta')
    close(m.running_mean, ref.running_mean, 1e-5, 'running_mean')
    close(m.running_var, ref.running_var, 1e-5, 'running_var')
    assert int(m.num_batches_tracked) == int(ref.num_batches_tracked)


def test_pooling_and_pads(hip):
    x, = det((2, 3, 9, 12), 61),
    for name, fr, fg in [
        ('avgpool', lambda t: F.avg_pool2d(t, 3, 2, 1, count_include_pad=False), hip.avgpool3s2),
        ('gap', lambda t: t.flatten(2).mean(2), hip.global_avg_pool),
        ('up2', lambda t: F.interpolate(t, scale_factor=2, mode='nearest'), hip.upsample2),
        ('rpad', lambda t: F.pad(t, (3,) * 4, mode='reflect'), lambda t: hip.reflect_pad(t, 3)),
        ('sigmoid', torch.sigmoid, lambda t: hip.activation(t, hip.ACT_SIGMOID)),
        ('tanh', torch.tanh, lambda t: hip.activation(t, hip.ACT_TANH)),
    ]:
        xr = x.clone().requires_grad_()
        yr = fr(xr)
        gy = det(tuple(yr.shape), 62)
        yr.backward(gy)
        xg = x.to(DEV).requires_grad_()
        yg = fg(xg)
        yg.backward(gy.to(DEV))
        close(yg, yr, 1e-6, name)
        close(xg.grad, xr.grad, 1e-5, name + ' grad')


# ------------------------------------------------------------------------------------------
# graph convolution: bit-exact pool, float parity of the layer
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('O_,T_,H_', [(9, 16, 16), (33, 96, 64), (288, 512, 512), (1056, 3072, 512)])
def test_triple_pool_bit_exact(hip, O_, T_, H_):
    g = torch.Generator().manual_seed(O_)
    Dout = 8
    edges = torch.randint(0, O_ - 1, (T_, 2), generator=g)        # last node isolated
    edges[1] = edges[0]
    edges[2, 1] = edges[2, 0]
    new_t = torch.randn(T_, 2 * H_ + Dout, generator=g)
    for avg in (True, False):
        want = O.pool_triples(new_t[:, :H_], new_t[:, H_ + Dout:], edges[:, 0].contiguous(), edges[:, 1].contiguous(),
                              O_, 'avg' if avg else 'sum')
        e = edges.to(DEV)
        off, ent = hip.build_csr(e, O_)
        pooled, new_p = hip.TriplePoolFn.apply(new_t.to(DEV), e, off, ent, O_, H_, Dout, avg)
        assert torch.equal(pooled.cpu(), want), 'pool must be BIT-exact (graph.py:94-116)'
        assert torch.equal(new_p.cpu(), new_t[:, H_:H_ + Dout])
    # CSR structure itself (integer-exact)
    off_c = off.cpu().long()
    deg = torch.bincount(edges.reshape(-1), minlength=O_)
    assert torch.equal(off_c[1:] - off_c[:-1], deg)


@pytest.mark.parametrize('case', ['small', 'small_sum', 'full', 'dense', 'one'])
def test_gconv_layer(hip, golden, case):
    from scene_generation_amd.graph import GraphTripleConv
    g = golden('gconv_' + case)
    Din, A, H, Dout, On, Tn, avg = [int(v) for v in g['cfg']]
    m = GraphTripleConv(Din, attributes_dim=A, output_dim=Dout, hidden_dim=H, pooling='avg' if avg else 'sum')
    fill_deterministic(m)
    m = m.to(DEV)
    obj = torch.from_numpy(g['obj']).to(DEV).requires_grad_()
    pred = torch.from_numpy(g['pred']).to(DEV).requires_grad_()
    edges = torch.from_numpy(g['edges']).to(DEV)
    new_obj, new_pred = m(obj, pred, edges)
    close(new_obj, g['new_obj'], 2e-5, 'new_obj')
    close(new_pred, g['new_pred'], 2e-5, 'new_pred')
    loss = (new_obj * torch.from_numpy(g['wo']).to(DEV)).sum() + (new_pred * torch.from_numpy(g['wp']).to(DEV)).sum()
    loss.backward()
    close(obj.grad, g['g_obj'], 1e-4, 'g_obj')
    close(pred.grad, g['g_pred'], 1e-4, 'g_pred')
    for n, p in m.named_parameters():
        if 'gp_' + n in g.files:
            close(p.grad, g['gp_' + n], 1e-4, n)


def test_gconvnet_vs_reference_golden(hip, golden):
    """GraphTripleConvNet (graph.py:125-148) as a STACK -- three layers, the reference's own outputs -- through the HIP path
    (the net was on the GPU only inside the step goldens)."""
    from scene_generation_amd.graph import GraphTripleConvNet
    g = golden('gconvnet_small')
    net = fill_deterministic(GraphTripleConvNet(8, num_layers=3, hidden_dim=16)).to(DEV)
    o2, p2 = net(torch.from_numpy(g['obj']).to(DEV), torch.from_numpy(g['pred']).to(DEV), torch.from_numpy(g['edges']).to(DEV))
    close(o2, g['new_obj'], 1e-5, 'gconvnet new_obj')
    close(p2, g['new_pred'], 1e-5, 'gconvnet new_pred')


def test_multiscale_discriminators_on_side_streams_are_bit_identical(hip):
    """streams.py (SG_MULTISTREAM=1): the PatchGAN scales on one HIP stream each == all of them on the current stream: outputs
    and every gradient bit-identical (no atomics, one writer per buffer), incl. gradients delivered into a FusedAdam's flat
    buffer by kernels of the side streams (optimiser step after ``join_all``)."""
    from scene_generation_amd import streams
    from scene_generation_amd.discriminators import define_D, define_mask_D
    from scene_generation_amd.optim import FusedAdam
    lay, img = det((4, 9, 64, 64), 301), det((4, 3, 64, 64), 302)
    msk, cond = det((6, 1, 32, 32), 303), torch.zeros(6, 5)
    cond[torch.arange(6), torch.tensor([0, 3, 4, 1, 1, 2])] = 1
    res = []
    saved = streams.ENABLED
    try:
        for on in (False, True, False):
            streams.ENABLED = on
            netD = define_D(12, 16, 2, norm='instance', num_D=3).to(DEV)
            netM = define_mask_D(1, 16, 2, norm='instance', num_D=2, num_objects=5).to(DEV)
            fill_deterministic(netD); fill_deterministic(netM)
            opt = FusedAdam(list(netD.parameters()) + list(netM.parameters()), lr=1e-3)
            a, b = lay.to(DEV).requires_grad_(), img.to(DEV).requires_grad_()
            m = msk.to(DEV).requires_grad_()
            outs = netD(a, b) + netM(m, cond.to(DEV))
            feats = [t for scale in outs for t in scale]
            opt.zero_grad()
            sum((t * t).mean() for t in feats).backward()
            grads = opt.fp.grad.clone()
            opt.step()
            torch.cuda.synchronize()
            res.append([t.detach().clone() for t in feats] + [a.grad.clone(), b.grad.clone(), m.grad.clone(), grads,
                                                              opt.fp.flat.detach().clone()])
    finally:
        streams.ENABLED = saved
    assert len(streams._POOL) >= 3                       # the side streams were really used
    for i, (x, y, z) in enumerate(zip(*res)):
        assert torch.equal(x, y) and torch.equal(x, z), 'tensor %d differs between one stream and a stream per scale' % i


def test_embedding_onehot_concat(hip):
    table, idx = det((12, 16), 71), torch.tensor([3, 0, 11, 3, 3, 7])
    tr = table.clone().requires_grad_()
    yr = F.embedding(idx, tr)
    gy = det(tuple(yr.shape), 72)
    yr.backward(gy)
    tg = table.to(DEV).requires_grad_()
    yg = hip.embedding(tg, idx.to(DEV))
    yg.backward(gy.to(DEV))
    assert torch.equal(yg.cpu(), yr.detach())
    close(tg.grad, tr.grad, 1e-6)
    # several 64-index rounds of the ordered row search, rows hit 0..30 times, a row width that is not a multiple of 64
    table2 = det((20, 130), 76)
    idx2 = torch.randint(0, 19, (300,), generator=torch.Generator().manual_seed(5))        # row 19 never hit: stays zero
    tr2 = table2.clone().requires_grad_()
    gy2 = det((300, 130), 77)
    F.embedding(idx2, tr2).backward(gy2)
    tg2 = table2.to(DEV).requires_grad_()
    hip.embedding(tg2, idx2.to(DEV)).backward(gy2.to(DEV))
    close(tg2.grad, tr2.grad, 1e-6)
    assert float(tg2.grad[19].abs().max()) == 0.0
    oh = hip.one_hot(idx.to(DEV), 12).cpu()
    assert torch.equal(oh, F.one_hot(idx, 12).float())
    a, b = det((6, 5), 73), det((6, 3), 74)
    ag, bg = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    c = hip.concat_cols(ag, bg)
    assert torch.equal(c.cpu(), torch.cat([a, b], 1))
    gc = det((6, 8), 75)
    c.backward(gc.to(DEV))
    assert torch.equal(ag.grad.cpu(), gc[:, :5]) and torch.equal(bg.grad.cpu(), gc[:, 5:])


# ------------------------------------------------------------------------------------------
# layout + crops (oracle and reference goldens)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['demo_16', 'demo_64', 'i64_m32', 'f32_m16', 'f32_m5_avg', 'edge'])
def test_masks_to_layout_golden(hip, golden, case):
    from scene_generation_amd.layout import masks_to_layout
    g = golden('layout_' + case)
    vecs = torch.from_numpy(g['vecs']).to(DEV).requires_grad_()
    H = int(g['H'])
    W = int(g['W']) if 'W' in g.files else H
    pooling = 'avg' if ('avg' in g.files and int(g['avg'])) else 'sum'
    out = masks_to_layout(vecs, torch.from_numpy(g['boxes']).to(DEV), torch.from_numpy(g['masks']).to(DEV),
                          torch.from_numpy(g['obj_to_img']).to(DEV), H, W, pooling=pooling)
    close(out, g['out'], 1e-5, 'layout')
    if 'g_vecs' in g.files:
        (out * torch.from_numpy(g['w']).to(DEV)).sum().backward()
        close(vecs.grad, g['g_vecs'], 1e-4, 'g_vecs')


def test_masks_to_layout_validation(hip):
    from scene_generation_amd.layout import masks_to_layout
    with pytest.raises(ValueError):
        masks_to_layout(torch.ones(2, 3, device=DEV), torch.tensor([[0., 0, 1, 1]] * 2, device=DEV),
                        torch.ones(2, 4, 4, device=DEV), torch.tensor([0, 2], device=DEV), 8)
    with pytest.raises(RuntimeError):        # CPU tensors: no fallback
        masks_to_layout(torch.ones(2, 3), torch.tensor([[0., 0, 1, 1]] * 2), torch.ones(2, 4, 4), torch.tensor([0, 1]), 8,
                        num_images=2, validate=False)


@pytest.mark.parametrize('cfg', [dict(N=3, min_objs=2, max_objs=5, size=32, mask_size=8, seed=1),
                                 dict(N=2, min_objs=14, max_objs=20, size=36, mask_size=16, seed=2),     # > 12 per image: two passes
                                 dict(N=4, min_objs=3, max_objs=8, size=128, mask_size=32, seed=3)])
def test_masks_to_layout_vs_oracle(hip, cfg):
    from scene_generation_amd.layout import masks_to_layout
    b = make_batch(num_objs=20, **cfg)
    D = 20 + 6
    vecs = det((b.objs.numel(), D), 81)
    for masks in (b.masks, torch.rand(b.masks.shape, generator=torch.Generator().manual_seed(5))):
        vr = vecs.clone().requires_grad_()
        want = O.masks_to_layout(vr, b.boxes, masks, b.obj_to_img, cfg['size'])
        w = det(tuple(want.shape), 82)
        (want * w).sum().backward()
        vg = vecs.to(DEV).requires_grad_()
        got = masks_to_layout(vg, b.boxes.to(DEV), masks.to(DEV), b.obj_to_img.to(DEV), cfg['size'],
                              num_images=cfg['N'], validate=False, grad_from_channel=20, max_per_image=4)
        close(got, want, 1e-5, 'layout')
        (got * w.to(DEV)).sum().backward()
        close(vg.grad[:, 20:], vr.grad[:, 20:], 2e-4, 'g_vecs')
        assert float(vg.grad[:, :20].abs().max()) == 0.0


@pytest.mark.parametrize('case', ['demo_16', 'demo_64', 'i64_m32', 'f32_m16', 'f32_m8_avg', 'many'])
def test_masks_to_layout_test_mode_golden(hip, golden, case):
    """front-to-back compositing in ascending-mass order (layout.py:87-92,157-169), reference goldens."""
    from scene_generation_amd.layout import masks_to_layout
    g = golden('layout_test_' + case)
    with torch.no_grad():
        out = masks_to_layout(torch.from_numpy(g['vecs']).to(DEV), torch.from_numpy(g['boxes']).to(DEV),
                              torch.from_numpy(g['masks']).to(DEV), torch.from_numpy(g['obj_to_img']).to(DEV),
                              int(g['H']), int(g['W']), pooling='avg' if int(g['avg']) else 'sum', test_mode=True)
    close(out, g['out'], 1e-5, 'test-mode layout')


def test_masks_to_layout_test_mode_vs_oracle_config2_shape(hip):
    from scene_generation_amd.layout import masks_to_layout
    b = make_batch(N=6, min_objs=3, max_objs=8, size=128, mask_size=32, num_objs=30, seed=11)
    vecs = det((b.objs.numel(), 30 + 8), 83) + 0.55
    for masks in (b.masks, torch.rand(b.masks.shape, generator=torch.Generator().manual_seed(6))):
        want = O.masks_to_layout(vecs, b.boxes, masks, b.obj_to_img, 128, test_mode=True)
        with torch.no_grad():
            got = masks_to_layout(vecs.to(DEV), b.boxes.to(DEV), masks.to(DEV), b.obj_to_img.to(DEV), 128, test_mode=True)
        close(got, want, 1e-5, 'test-mode layout')
    with pytest.raises(NotImplementedError):          # inference only
        masks_to_layout(vecs.to(DEV).requires_grad_(), b.boxes.to(DEV), b.masks.to(DEV), b.obj_to_img.to(DEV), 128,
                        test_mode=True)


def test_model_inference_forward_golden(hip, golden):
    """Model.forward(test_mode=True[, features]) in eval mode == the reference (model.py:111-117,158-163)."""
    from sampling_helpers import inference_model, inference_cases
    from scene_generation_amd.model import Model
    from scene_generation_amd.synthetic import batch_to
    g = golden('model_test_mode')
    m, batch = inference_model(Model)
    m = m.to(DEV)
    imgs, objs, boxes, masks, triples, o2i, _, attributes = batch_to(batch, DEV)
    for tag, kw in inference_cases(batch, g):
        kw = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        m.noise_override = torch.from_numpy(g[tag + '_noise']).to(DEV)
        with torch.no_grad():
            out = m(imgs, objs, triples, o2i, attributes=attributes, test_mode=True, **kw)
        assert out[3] is None and out[5] is None
        close(out[1], g[tag + '_boxes_pred'], 2e-5, tag + ' boxes')
        close(out[2], g[tag + '_masks_pred'], 2e-5, tag + ' masks')
        close(out[4], g[tag + '_pred_layout'], 2e-5, tag + ' layout')
        close(out[0], g[tag + '_imgs_pred'], 1e-4, tag + ' imgs')


@pytest.mark.parametrize('case', ['sorted_8', 'perm_8', 'perm_32', 'jj_batch'])
def test_crop_golden(hip, golden, case):
    from scene_generation_amd.bilinear import crop_bbox_batch
    g = golden('crop_' + case)
    feats = torch.from_numpy(g['feats']).to(DEV).requires_grad_()
    WW = int(g['WW']) if 'WW' in g.files else None
    # 'jj_batch': crop_bbox_batch(backend='jj') of the reference (bilinear.py:42-56) = the grid_sample crop, rectangular here
    out = crop_bbox_batch(feats, torch.from_numpy(g['boxes']).to(DEV), torch.from_numpy(g['idx']).to(DEV), int(g['HH']), WW,
                          backend='jj' if case == 'jj_batch' else 'cudnn')
    close(out, g['out'], 1e-5, 'crop')
    (out * torch.from_numpy(g['w']).to(DEV)).sum().backward()
    close(feats.grad, g['g_feats'], 1e-4, 'g_feats')


@pytest.mark.parametrize('case', ['sq', 'rect'])
def test_crop_bbox_jj_direct_golden(hip, golden, case):
    """crop_bbox(feats, bbox, HH, WW, backend='jj') against the reference's own output (bilinear.py:101-130,188-243: pixel coordinate
    X * W, clamped floor / floor + 1 taps, the cancelling weights at the far edge) and its gradient w.r.t. feats"""
    from scene_generation_amd.bilinear import crop_bbox
    g = golden('crop_jj_direct_' + case)
    feats = torch.from_numpy(g['feats']).to(DEV).requires_grad_()
    out = crop_bbox(feats, torch.from_numpy(g['boxes']).to(DEV), int(g['HH']), int(g['WW']), backend='jj')
    close(out, g['out'], 1e-5, 'crop jj')             # (the tolerances of the grid_sample crops above; measured 1.6e-6: fma contraction)
    (out * torch.from_numpy(g['w']).to(DEV)).sum().backward()
    close(feats.grad, g['g_feats'], 1e-4, 'g_feats')


def test_vector_pool_matches_reference_semantics(hip):
    from scene_generation_amd.utils import VectorPool
    random.seed(7)
    ref, mine = O.VectorPool(3), VectorPool(3)
    st = random.getstate()
    g = torch.Generator().manual_seed(0)
    outs_ref, batches = [], []
    for it in range(6):
        objs = torch.randint(0, 5, (11,), generator=g)
        vec = torch.randn(11, 4, generator=g)
        batches.append((objs, vec))
        outs_ref.append(ref.query(objs, vec))
    random.setstate(st)
    for (objs, vec), want in zip(batches, outs_ref):
        got = mine.query(objs.to(DEV), vec.to(DEV))
        assert torch.equal(got.cpu(), want), 'VectorPool must replay utils.py:67-90 exactly'
    for c in range(5):
        a, b = ref.vectors.get(c, []), mine.vectors_of(c)
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------
# losses / optimiser
# ------------------------------------------------------------------------------------------
def test_losses(hip, golden):
    from scene_generation_amd.losses import GANLoss, gan_g_loss, gan_d_loss
    g = golden('losses')
    T = lambda k: torch.from_numpy(g[k]).to(DEV)
    preds = [[T('p00'), T('p01')], [T('p10'), T('p11')]]
    crit = GANLoss()
    close(crit(preds, True), g['gan_true'], 1e-6)
    close(crit(preds, False), g['gan_false'], 1e-6)
    close(crit(preds[0], True), g['gan_single'], 1e-6)
    close(gan_g_loss(T('sf')), g['g_loss'], 1e-6)
    close(gan_d_loss(T('sr'), T('sf')), g['d_loss'], 1e-6)
    close(hip.cross_entropy(T('logits'), T('tgt')), g['ce'], 1e-6)
    close(hip.mse(T('p00'), T('r00')), g['mse'], 1e-6)
    close(hip.l1(T('p00'), T('r00')), g['l1'], 1e-6)
    # gradients vs torch
    for name, fr, fg in [
        ('mse_const', lambda a: F.mse_loss(a, torch.full_like(a, 1.0)), lambda a: hip.mse_const(a, 1.0)),
        ('bce', lambda a: O.bce_loss(a.reshape(-1), torch.zeros(a.numel())), lambda a: hip.bce_logits_const(a.reshape(-1), 0.0)),
        ('l1', lambda a: F.l1_loss(a, det(tuple(a.shape), 92)), lambda a: hip.l1(a, det(tuple(a.shape), 92).to(DEV))),
        ('ce', lambda a: F.cross_entropy(a.view(10, 24), torch.arange(10) % 7),
         lambda a: hip.cross_entropy(a.view(10, 24), (torch.arange(10) % 7).to(DEV))),
    ]:
        a = det((2, 3, 5, 8), 91, 3.0)
        ar = a.clone().requires_grad_()
        lr = fr(ar) * 0.37
        lr.backward()
        ag = a.to(DEV).requires_grad_()
        lg = fg(ag) * 0.37
        lg.backward()
        close(lg, lr, 1e-6, name)
        close(ag.grad, ar.grad, 1e-6, name + ' grad')


def test_fused_adam_matches_torch(hip):
    from scene_generation_amd.optim import FusedAdam
    ref = nn.Sequential(nn.Linear(7, 5), nn.Linear(5, 3))
    fill_deterministic(ref)
    mine = nn.Sequential(nn.Linear(7, 5), nn.Linear(5, 3))
    fill_deterministic(mine)
    mine = mine.to(DEV)
    o_ref = torch.optim.Adam(ref.parameters(), lr=1e-2, betas=(0.5, 0.999))
    o_mine = FusedAdam(mine.parameters(), lr=1e-2, betas=(0.5, 0.999))
    for it in range(5):
        o_ref.zero_grad()
        o_mine.zero_grad()
        for (n, p), q in zip(ref.named_parameters(), mine.parameters()):
            gr = det(tuple(p.shape), 100 + it, 0.5)
            p.grad = gr.clone()
            q.grad.add_(gr.to(DEV))
        o_mine.mark_all_touched()
        o_ref.step()
        o_mine.step()
    for p, q in zip(ref.parameters(), mine.parameters()):
        close(q, p, 1e-6, 'param after adam')
    sd = o_mine.state_dict()
    sd_ref = o_ref.state_dict()
    for i in sd_ref['state']:
        close(sd['state'][i]['exp_avg'], sd_ref['state'][i]['exp_avg'], 1e-6)
        close(sd['state'][i]['exp_avg_sq'], sd_ref['state'][i]['exp_avg_sq'], 1e-6)
        assert float(sd['state'][i]['step']) == float(sd_ref['state'][i]['step'])


def test_fused_adam_skips_parameters_without_gradient(hip):
    """torch.optim.Adam leaves a parameter whose .grad is None untouched (no moment decay, step not advanced): e.g.
    box_net when use_gt is False (trainer.py:210-216).  The flat optimiser must do the same."""
    from scene_generation_amd.optim import FusedAdam
    ref = nn.Sequential(nn.Linear(4, 3), nn.Linear(3, 2), nn.Linear(2, 2))
    mine = nn.Sequential(nn.Linear(4, 3), nn.Linear(3, 2), nn.Linear(2, 2))
    fill_deterministic(ref)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(DEV)
    o_ref = torch.optim.Adam(ref.parameters(), lr=1e-2, betas=(0.5, 0.999))
    o_mine = FusedAdam(mine.parameters(), lr=1e-2, betas=(0.5, 0.999))
    x = det((5, 4), 131)
    for it in range(4):
        o_ref.zero_grad()
        o_mine.zero_grad()
        use_mid = it % 2 == 0                      # the middle layer only gets a gradient every other step
        for net, inp in ((ref, x), (mine, x.to(DEV))):
            h = net[0](inp)
            h = net[1](h) if use_mid else h[:, :2]
            net[2](h).pow(2).sum().backward()
        o_ref.step()
        o_mine.step()
    for p, q in zip(ref.parameters(), mine.parameters()):
        close(q, p, 1e-5, 'param')
    assert o_mine.steps == [4, 4, 2, 2, 4, 4]
    sd, sr = o_mine.state_dict(), o_ref.state_dict()
    for i in sr['state']:
        assert float(sd['state'][i]['step']) == float(sr['state'][i]['step'])
        close(sd['state'][i]['exp_avg'], sr['state'][i]['exp_avg'], 1e-5)


# ------------------------------------------------------------------------------------------
# modules vs reference goldens (same fixtures the oracle is pinned with)
# ------------------------------------------------------------------------------------------
def _run_module(g, mod, n_in, train=True):
    fill_deterministic(mod)
    mod = mod.to(DEV)
    mod.train(train)
    ins = []
    for i in range(n_in):
        t = torch.from_numpy(g['in%d' % i]).to(DEV)
        ins.append(t.clone().requires_grad_() if t.is_floating_point() else t)
    out = mod(*ins)
    flat = []

    def walk(o):
        if isinstance(o, torch.Tensor):
            flat.append(o)
        elif isinstance(o, (list, tuple)):
            for x in o:
                walk(x)
    walk(out)
    loss = 0
    for i, o in enumerate(flat):
        close(o, g['out%d' % i], 3e-5, 'out%d' % i)
        loss = loss + (o * torch.from_numpy(g['w%d' % i]).to(DEV)).sum()
    loss.backward()
    k = 0
    for t in ins:
        if t.is_floating_point():
            if t.grad is not None:
                close(t.grad, g['gin%d' % k], 3e-4, 'gin%d' % k)
            k += 1
    for n, p in mod.named_parameters():
        close(p.grad if p.grad is not None else torch.zeros_like(p), g['gp_' + n], 3e-4, n)
    for n, b in mod.named_buffers():
        close(b, g['buf_' + n], 1e-5, n)


def test_modules_vs_reference(hip, golden):
    from scene_generation_amd import layers as Lh, generators as Gh, discriminators as Dh
    vocab = make_vocab(12, 4, 0)
    IN = Lh.get_norm_layer('instance')
    _run_module(golden('mod_mlp'), Lh.build_mlp([10, 16, 6]), 1)
    _run_module(golden('mod_mask_net'), Gh.mask_net(24, 8), 1)
    # residual blocks of build_cnn (BatchNorm buffers pin the reference's double evaluation of the branch), eval-mode dropout
    _run_module(golden('mod_cnn_residual'), Lh.build_cnn('I6,R,C3-8-2,R,C3-4', normalization='batch',
                                                         activation='leakyrelu-0.2', padding='same')[0], 1)
    _run_module(golden('mod_mlp_dropout_eval'), Lh.build_mlp([10, 16, 6], dropout=0.3), 1, train=False)
    _run_module(golden('mod_encoder'), Gh.AppearanceEncoder(vocab, arch='C4-8-2,C4-16-2,C4-32-2', normalization='batch',
                                                            activation='leakyrelu-0.2', padding='valid', vecs_size=24), 1)
    _run_module(golden('mod_globalgen'), Gh.GlobalGenerator(12, 3, ngf=8, n_downsampling=2, n_blocks=2, norm_layer=IN), 1)
    _run_module(golden('mod_imgD'), Dh.MultiscaleDiscriminator(7, ndf=8, n_layers=3, norm_layer=IN, num_D=2), 1)
    _run_module(golden('mod_maskD'), Dh.MultiscaleMaskDiscriminator(1, ndf=8, n_layers=2, norm_layer=IN, num_D=1,
                                                                    num_objects=12), 2)
    _run_module(golden('mod_objD'), Dh.AcCropDiscriminator(vocab, arch='C4-8-2,C4-16-2,C4-32-2', normalization='batch',
                                                           activation='leakyrelu-0.2', object_size=32, padding='valid'), 4)


def test_dropout_and_residual_block_semantics(hip):
    """layers.Dropout: training = x * Bernoulli(1-p) mask / (1-p) with the mask torch's device generator draws (re-drawn here from
    the same seed), gradient through the same mask, eval = identity; ResnetBlock(use_dropout=True) builds and steps;
    ResidualBlock without padding is refused like the reference's empty shortcut (layers.py:111-113)."""
    from scene_generation_amd import layers as Lh
    x = det((6, 40), 401).to(DEV).requires_grad_()
    drop = Lh.Dropout(0.3).to(DEV)
    torch.manual_seed(77)
    y = drop(x)
    torch.manual_seed(77)
    mask = torch.empty_like(x).bernoulli_(0.7)
    assert torch.equal(y.detach(), (x.detach() * mask * (1.0 / 0.7))) or float((y.detach() - x.detach() * mask / 0.7).abs().max()) < 1e-6
    y.backward(torch.ones_like(y))
    close(x.grad, mask / 0.7, 1e-6, 'dropout gradient')
    drop.eval()
    assert drop(x) is x
    blk = Lh.ResnetBlock(16, 'reflect', Lh.get_norm_layer('instance'), use_dropout=True).to(DEV)
    assert [type(m).__name__ for m in blk.conv_block][4] == 'Dropout'
    out = blk(det((2, 16, 8, 8), 402).to(DEV))
    assert out.shape == (2, 16, 8, 8) and torch.isfinite(out).all()
    with pytest.raises(ValueError):
        Lh.ResidualBlock(8, padding='valid')


def test_imgD_folded_concat_equals_materialised(hip):
    from scene_generation_amd import layers as Lh, discriminators as Dh
    d = Dh.MultiscaleDiscriminator(7, ndf=8, n_layers=3, norm_layer=Lh.get_norm_layer('instance'), num_D=2)
    fill_deterministic(d)
    d = d.to(DEV)
    a, b = det((2, 4, 32, 32), 111).to(DEV), det((2, 3, 32, 32), 112).to(DEV)
    r1 = d(torch.cat([a, b], 1))
    r2 = d(a, b)
    for s1, s2 in zip(r1, r2):
        for f1, f2 in zip(s1, s2):
            close(f2, f1, 1e-6)


# ------------------------------------------------------------------------------------------
# full G+D step vs the reference golden (reduced widths) and vs the oracle (config 1, full widths)
# ------------------------------------------------------------------------------------------
def test_full_step_vs_reference_golden(hip, golden):
    """Two G+D iterations from the reference Trainer's golden run (reduced widths).

    Iteration 0 is tight.  Iteration 1 is loose BY NATURE: the first Adam step is sign descent
    (update = lr*g/(|g|+eps)), so weight elements whose true gradient is ~0 (bias in front of InstanceNorm, taps
    of all-zero one-hot channels, ...) move by +-lr with a sign decided by fp32 round-off, which differs between
    any two summation orders (the reference on CUDA vs CPU would differ the same way).  The tight second-iteration
    check is test_full_step_config1_vs_oracle, which re-synchronises the state between iterations."""
    from scene_generation_amd.trainer import Trainer
    g = golden('step_reduced')
    args = parser.parse_args(g['argv'].tolist())
    C, P, A = 12, 4, 35
    tr = Trainer(args, make_vocab(C, P, A))
    for m in (tr.model, tr.netD, tr.obj_discriminator, tr.mask_discriminator):
        fill_deterministic(m)
    random.seed(1234)
    for it in range(2):
        batch = batch_to(make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=C, num_preds=P,
                                    num_attributes=A, seed=100 + it), DEV)
        pre = 'it%d_' % it
        tr.model.noise_override = torch.from_numpy(g[pre + 'noise'])
        out = tr.step(batch, use_gt=(it == 0))
        tol = 5e-2 if it else 1e-4
        for n, t in zip(['imgs_pred', 'boxes_pred', 'masks_pred'], out[:3]):
            close(t, g[pre + n], tol, n)
        close(out[5][:, C:], g[pre + 'layout_wrong_rep'], tol, 'wrong layout')
        for lname, L in [('g', tr.generator_losses), ('dmask', tr.d_mask_losses), ('dobj', tr.d_obj_losses),
                         ('dimg', tr.d_img_losses)]:
            for k, v in L.items():
                ref = float(g[pre + 'loss_' + lname + '_' + k])
                assert abs(v - ref) <= (5e-2 if it else 2e-4) * max(1.0, abs(ref)), (it, lname, k, v, ref)
        for mname, m in [('model', tr.model), ('netD', tr.netD), ('objD', tr.obj_discriminator),
                         ('maskD', tr.mask_discriminator)]:
            sd = m.state_dict()
            for k, (s, a) in zip(g[pre + 'keys_' + mname].tolist(), g[pre + 'stats_' + mname]):
                got = sd[k].double().abs().sum().item()
                assert abs(got - a) <= 1e-2 * max(1.0, a), (it, mname, k, got, a)


@pytest.mark.parametrize('tag', ['c2', 'c1'])
def test_full_width_step_vs_reference_golden(hip, golden, tag):
    """The HIP Trainer against the reference Trainer's own two iterations at DEFAULT widths (tests/golden/step_full_*.npz,
    captured from trainer.py:205-325 / train.py:190-215 by tools/make_golden.py): BASELINE configs[1] shape (128x128, N = 8:
    Winograd 128-tiles, factored layout convs, sub-pixel mask_net, every kernel family of the bench line) and configs[0]
    (64x64, N = 4).  Tolerances ~2x the measured deviations (see tests/test_oracle_golden.py: iteration 1 follows a
    sign-descent Adam step).  The measured numbers are written to gpurun_out/parity_step_full_<tag>.json first."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from step_full_common import run_step_full
    from scene_generation_amd.trainer import Trainer
    from scene_generation_amd.synthetic import batch_to

    def make(args, vocab):
        return Trainer(args, vocab, device=DEV)
    devs = run_step_full(golden('step_full_' + tag), make, to_device=lambda b: batch_to(b, DEV))
    _dump('parity_step_full_%s.json' % tag, [{k: (float(v) if not isinstance(v, str) else v) for k, v in d.items()} for d in devs])
    tols = [dict(loss=2e-6, out_abs=1e-4, out_stat=2e-6, param_stat=5e-4),
            dict(loss=1.5e-3, out_abs=0.1, out_stat=1.5e-3, param_stat=6e-4) if tag == 'c2' else
            dict(loss=6e-3, out_abs=0.2, out_stat=1.5e-3, param_stat=8e-4)]
    for it, (dev, tol) in enumerate(zip(devs, tols)):
        for k, t in tol.items():
            assert dev[k] <= t, (tag, it, k, dev[k], t, dev)


class _HipGrads(object):
    """the flat gradient buffer of one FusedAdam as the test saw it right before the Adam step (ONE device clone instead of a
    device -> host copy per parameter), readable per parameter; ``len`` / indexing / iteration give CPU tensors like the list the
    oracle side stores, ``flat_pair(ref_list)`` gives both sides as float64 vectors ON THE DEVICE in the optimiser's flat layout"""

    def __init__(self, opt):
        self.flat = opt.fp.grad.detach().clone()
        self.offsets = list(opt.fp.offsets)
        self.shapes = [tuple(p.shape) for p in opt.fp.params]
        self.numels = [p.numel() for p in opt.fp.params]

    def __len__(self):
        return len(self.shapes)

    def view(self, i):
        o, n = self.offsets[i], self.numels[i]
        return self.flat[o:o + n].view(self.shapes[i])

    def __getitem__(self, i):
        return self.view(i).cpu()

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def flat_pair(self, ref_list):
        """(hip, ref) float64 on the device, flat layout of the optimiser (alignment gaps zero on both sides)"""
        host = torch.zeros(self.flat.numel(), dtype=torch.float32)
        for o, n, g in zip(self.offsets, self.numels, ref_list):
            if g is not None:
                host[o:o + n] = g.reshape(-1)
        fb = host.to(self.flat.device).double()
        fa = torch.zeros_like(fb)
        for o, n in zip(self.offsets, self.numels):          # (gaps of the live buffer are never written, but be explicit)
            fa[o:o + n] = self.flat[o:o + n].double()
        return fa, fb


def _grad_snapshots(ref, tr):
    """capture per-parameter gradients of all four optimisers right before their Adam steps.  Idempotent per trainer pair (a
    cached pair, _trainer_pair, is handed to several tests): the hooks are registered once, the dict is emptied on re-use."""
    prev = getattr(tr, '_test_grad_snaps', None)
    if prev is not None and prev[1] is ref:
        prev[0]['ref'].clear()
        prev[0]['hip'].clear()
        return prev[0], prev[2]
    snaps = {'ref': {}, 'hip': {}}
    names = ['optimizer', 'optimizer_d_mask', 'optimizer_d_obj', 'optimizer_d_img']
    handles = []
    for n in names:
        o_ref, o_hip = getattr(ref, n), getattr(tr, n)

        def pre_ref(opt, a, k, n=n):
            snaps['ref'][n] = [None if p.grad is None else p.grad.detach().clone() for p in opt.param_groups[0]['params']]
        handles.append(o_ref.register_step_pre_hook(pre_ref))

        def pre_hip(o=o_hip, n=n):
            snaps['hip'][n] = _HipGrads(o)
        o_hip.pre_step_hooks.append(pre_hip)
    tr._test_grad_snaps = (snaps, ref, handles)
    return snaps, handles


def _seg_norms(v, hg):
    """per-parameter L2 norms of a flat float64 device vector (one small reduction per parameter, results fetched once)"""
    return torch.stack([v[o:o + n].norm() for o, n in zip(hg.offsets, hg.numels)]).cpu()


_GRAD_LOG = {}


def _compare_grads(snaps, tag, rel_tol=3e-2, cos_tol=0.9995, small_floor=1e-3, collect=None):
    """HIP gradients of a whole step vs the fp32 oracle's.

    Single operators agree to ~1e-5 (tests above).  Through the 40-layer generator the forward activations differ
    by ~2e-5 (MFMA accumulates each K=2304..9216 dot product as ONE sequential fp32 fma chain, oneDNN on the CPU
    sums in blocks), so a few dozen of the ~1e6 ReLU / LeakyReLU units whose pre-activation is within 2e-5 of zero take
    the other branch and individual gradient entries move at the 1e-3..1e-2 level (measured with tests/debug_grads.py:
    d loss / d imgs_pred agrees to 1e-7, d loss / d layout after the generator backward to 4e-3 of its max).
    Checks that are robust to that: (1) flat gradient of every optimiser: cosine > 0.9995 (observed 0.9999 +- 1e-4
    depending on which units flip: any change of a summation order anywhere in the step moves it); (2) every tensor with a
    non-negligible norm: relative L2 error <= 3e-2; (3) no single entry off by more than half the tensor max."""
    for n, gr in snaps['ref'].items():
        gh = snaps['hip'][n]
        fa, fb = gh.flat_pair(gr)                     # float64, on the device
        cos = float(fa @ fb / (fa.norm() * fb.norm() + 1e-30))
        assert cos > cos_tol, '%s %s: flat gradient cosine %.6f' % (tag, n, cos)
        gmax, gnorm = float(fb.abs().max()), float(fb.norm())
        dn, bn = _seg_norms(fa - fb, gh), _seg_norms(fb, gh)
        dmax = torch.stack([(fa[o:o + k] - fb[o:o + k]).abs().max() for o, k in zip(gh.offsets, gh.numels)]).cpu()
        bmax = torch.stack([fb[o:o + k].abs().max() for o, k in zip(gh.offsets, gh.numels)]).cpu()
        for i in range(len(gh)):
            err = float(dmax[i])
            lim = 0.5 * float(bmax[i]) + 1e-4 * gmax + 1e-9      # single entries only; (2) bounds the bulk
            assert err <= lim, '%s %s param %d: grad err %.3e > %.3e (|g|max %.3e, global %.3e)' % (
                tag, n, i, err, lim, float(bmax[i]), gmax)
            if float(bn[i]) > small_floor * gnorm:
                rel = float(dn[i] / bn[i])
                key = '%s/%s' % (tag, n)
                _GRAD_LOG[key] = max(_GRAD_LOG.get(key, 0.0), rel)
                if collect is not None:
                    collect.setdefault((n, i), []).append(rel)
                assert rel <= rel_tol, '%s %s param %d: relative L2 gradient error %.3e' % (tag, n, i, rel)


def _compare_outputs(tr, ref, out, out_ref, tol):
    for n, a, b in zip(['imgs_pred', 'boxes_pred', 'masks_pred', 'layout', 'layout_pred', 'layout_wrong'], out, out_ref):
        close(a, b, tol, n)
    for La, Lb in [(tr.generator_losses, ref.generator_losses), (tr.d_mask_losses, ref.d_mask_losses),
                   (tr.d_obj_losses, ref.d_obj_losses), (tr.d_img_losses, ref.d_img_losses)]:
        a, b = dict(La.items()), dict(Lb.items())
        assert set(a) == set(b)
        for k in b:
            assert abs(a[k] - b[k]) <= 5 * tol * max(1.0, abs(b[k])), (k, a[k], b[k])


def _sync_state(ref, tr):
    for a, b in [(ref.model, tr.model), (ref.netD, tr.netD), (ref.obj_discriminator, tr.obj_discriminator),
                 (ref.mask_discriminator, tr.mask_discriminator)]:
        b.load_state_dict(a.state_dict())
    for n in ['optimizer', 'optimizer_d_mask', 'optimizer_d_obj', 'optimizer_d_img']:
        getattr(tr, n).load_state_dict(getattr(ref, n).state_dict())


@pytest.mark.parametrize('cfg', ['reduced', 'config1'])
def test_full_step_vs_oracle(hip, cfg):
    """Outputs, the 16 named losses and EVERY parameter gradient of two G+D iterations (train.py:190-215) against the
    oracle Trainer.  'config1' = BASELINE config 1: 4-object graphs, 64x64, batch 4, full widths (183 M-param G).
    State is re-synchronised between the iterations so that the second one (non-empty VectorPool, non-zero Adam
    moments, updated BatchNorm running stats, use_gt=False branch) is compared tightly too."""
    from scene_generation_amd.trainer import Trainer
    if cfg == 'config1':
        argv = ['--image_size', '64,64', '--batch_size', '4', '--vgg_features_weight', '0', '--output_dir', '/tmp/o']
        vocab, bk = make_vocab(), dict(N=4, min_objs=4, max_objs=4, size=64)
    else:
        argv = ['--image_size', '32,32', '--batch_size', '3', '--vgg_features_weight', '0', '--output_dir', '/tmp/o',
                '--n_downsample_global', '2', '--gconv_hidden_dim', '64', '--gconv_num_layers', '3', '--mask_size', '8',
                '--ndf', '8', '--ndf_mask', '8', '--crop_size', '16', '--d_obj_arch', 'C4-8-2,C4-16-2', '--pool_size', '2']
        vocab, bk = make_vocab(12, 4, 35), dict(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=12, num_preds=4)
    args = parser.parse_args(argv)
    from conftest import skip_random_init
    with skip_random_init():               # every parameter is overwritten by the fill / the state sync below
        ref = O.Trainer(args, vocab)
        tr = Trainer(args, vocab)
    for m in (ref.model, ref.netD, ref.obj_discriminator, ref.mask_discriminator):
        fill_deterministic(m)
    _sync_state(ref, tr)
    snaps, _ = _grad_snapshots(ref, tr)
    threads0 = torch.get_num_threads()
    if cfg == 'reduced':
        torch.set_num_threads(int(os.environ.get('SG_TEST_ORACLE_THREADS', '1')))      # (see the bounds below)
    try:
        _full_step_iterations(cfg, args, bk, ref, tr, snaps)
    finally:
        torch.set_num_threads(threads0)


_REDUCED_SEEDS = (0, 100, 300)


def _full_step_iterations(cfg, args, bk, ref, tr, snaps):
    # 'reduced' (every kernel family at small widths) is the configuration where a SYSTEMATIC error in one small parameter tensor can
    # be told from fp32 noise: most tensors agree with the oracle to 1e-6..3e-5.  Not all of them in every step, though: a scan
    # over six data seeds (round 6, tools/probe/r06_call39.sh) found a generator tensor at 4e-4 .. 1.5e-2 in seven of twelve
    # iterations (discriminators: always <= 1e-5) -- a unit of the generator within fp32 noise of a kink takes the other branch --
    # and WHICH iteration depends on every summation order of the step and on the CPU oracle's thread count (single-threaded here:
    # bit-reproducible).  So the tight bound -- 2e-4: the worst tensor's best sample measured 2.7e-5, a 1 % error is 50 bounds away --
    # is asked of every tensor in AT LEAST ONE of six independent samples (three data seeds x two iterations: a systematic error
    # shows in all of them, a flipped unit in its own), the full-width bound 3e-2 in all of them (the 3e-2
    # bound alone cannot see a 1 % error in a small tensor).
    seeds = _REDUCED_SEEDS if cfg == 'reduced' else (0,)
    if cfg == 'reduced' and os.environ.get('SG_TEST_REDUCED_SEED'):
        seeds = tuple(int(v) for v in os.environ['SG_TEST_REDUCED_SEED'].split(','))
    collect = {}
    for seed0 in seeds:
        for it in range(2):
            batch = make_batch(seed=seed0 + it, **bk)
            noise = det((1, args.mask_noise_dim), 121 + it)
            ref.model.noise_override = tr.model.noise_override = noise
            random.seed(5 + it)
            out_ref = ref.step(batch, use_gt=(it == 0))
            random.seed(5 + it)
            out = tr.step(batch_to(batch, DEV), use_gt=(it == 0))
            _compare_outputs(tr, ref, out, out_ref, 2e-4)
            if cfg == 'reduced':
                _compare_grads(snaps, '%s_s%d_it%d' % (cfg, seed0, it), cos_tol=0.9999, small_floor=1e-5, collect=collect)
            else:
                _compare_grads(snaps, '%s_it%d' % (cfg, it))
            _sync_state(ref, tr)
    if cfg == 'reduced':
        tight = float(os.environ.get('SG_TEST_REDUCED_TOL', '2e-4'))
        best = {k: min(v) for k, v in collect.items()}
        worst_best = max(best.values())
        _GRAD_LOG['reduced/best_of_samples'] = worst_best
        bad = {k: v for k, v in best.items() if v > tight}
        assert not bad, 'tensors off by more than %.0e in EVERY sample (optimiser, parameter index: smallest relative L2): %r' % (tight, bad)
    _dump('grad_rel_l2_%s.json' % cfg, {k: v for k, v in _GRAD_LOG.items() if k.startswith(cfg)})


# ------------------------------------------------------------------------------------------
# full-size (BASELINE config 2) size-independent properties
# ------------------------------------------------------------------------------------------
def test_layout_full_size_properties(hip):
    from scene_generation_amd.layout import masks_to_layout
    b = batch_to(make_batch(N=32, min_objs=3, max_objs=8, size=128, seed=0), DEV)
    Oc = b.objs.numel()
    g = torch.Generator().manual_seed(0)
    v1, v2 = torch.randn(Oc, 204, generator=g).to(DEV), torch.randn(Oc, 204, generator=g).to(DEV)
    kw = dict(num_images=32, validate=False)
    l1 = masks_to_layout(v1, b.boxes, b.masks, b.obj_to_img, 128, **kw)
    l2 = masks_to_layout(v2, b.boxes, b.masks, b.obj_to_img, 128, **kw)
    l12 = masks_to_layout(v1 + 2 * v2, b.boxes, b.masks, b.obj_to_img, 128, **kw)
    close(l12, l1 + 2 * l2, 1e-5, 'linearity in vecs')
    # per-image independence: image 7 computed alone equals its slice of the batch
    sel = b.obj_to_img == 7
    alone = masks_to_layout(v1[sel], b.boxes[sel], b.masks[sel], torch.zeros(int(sel.sum()), dtype=torch.long, device=DEV),
                            128, num_images=1, validate=False)
    assert torch.equal(alone[0], l1[7])
    # the __image__ node (box [0,0,1,1], all-ones mask) contributes its vector everywhere inside the image
    ones = torch.zeros(Oc, 204, device=DEV)
    last = torch.cat([b.obj_to_img[1:] != b.obj_to_img[:-1], torch.tensor([True], device=DEV)])
    ones[last] = 1.0
    lim = masks_to_layout(ones, b.boxes, b.masks, b.obj_to_img, 128, **kw)
    close(lim[:, :, 4:-4, 4:-4], torch.ones_like(lim[:, :, 4:-4, 4:-4]), 1e-6, 'image node')


@pytest.mark.parametrize('name,N', [('c4', 2), ('c5', 4)])
def test_step_runs_at_config4_and_config5_shapes(hip, name, N):
    """BASELINE configs[3] (256x256, <=16 objects) and configs[4] (32 objects / 96 triples per image) per-GPU shapes at
    full widths: two G+D steps finish with finite losses (Winograd at 16x16 planes, two column blocks in the RGB head,
    33 object planes in the factored layout convs, the dense-graph scatter)."""
    from scene_generation_amd.trainer import Trainer
    from scene_generation_amd.synthetic import make_config_batch
    b = make_config_batch(name, seed=3, N=N)
    S = b.imgs.size(-1)
    args = parser.parse_args(['--image_size', '%d,%d' % (S, S), '--batch_size', str(N), '--vgg_features_weight', '0',
                              '--output_dir', '/tmp/o'])
    torch.manual_seed(0)
    tr = Trainer(args, make_vocab())
    random.seed(0)
    for it in range(2):
        tr.step(batch_to(b, DEV), use_gt=(it == 0))
    for L in (tr.generator_losses, tr.d_img_losses, tr.d_obj_losses, tr.d_mask_losses):
        for k, v in L.items():
            assert v == v and abs(v) < 1e6, (name, k, v)


def test_fast_paths_agree_with_plain_paths(hip):
    """Winograd / factored layout convs / shared D forwards are exact re-formulations: one generator forward + the losses
    of a full step with every switch off equal the default path to fp32 rounding."""
    from scene_generation_amd import ops
    from scene_generation_amd.trainer import Trainer
    args = parser.parse_args(['--image_size', '64,64', '--batch_size', '4', '--vgg_features_weight', '0', '--output_dir', '/tmp/o'])
    b = batch_to(make_batch(N=4, min_objs=3, max_objs=6, size=64, seed=9), DEV)
    res = []
    saved = (ops.WINOGRAD, ops.FACTORED_LAYOUT)
    try:
        for fast in (True, False):
            ops.WINOGRAD = ops.FACTORED_LAYOUT = fast
            torch.manual_seed(0)
            tr = _filled_trainer(args, make_vocab())
            tr.share_d_forward = fast
            tr.model.noise_override = det((1, 64), 131).to(DEV)
            random.seed(3)
            out = tr.step(b, use_gt=True)
            losses = {}
            for L in (tr.generator_losses, tr.d_img_losses, tr.d_obj_losses, tr.d_mask_losses):
                losses.update(dict(L.items()))
            res.append((out[0].detach().cpu(), losses))
    finally:
        ops.WINOGRAD, ops.FACTORED_LAYOUT = saved
    close(res[0][0], res[1][0], 2e-4, 'imgs_pred fast vs plain')
    for k, v in res[1][1].items():
        assert abs(res[0][1][k] - v) <= 2e-3 * max(1.0, abs(v)), (k, res[0][1][k], v)


# ------------------------------------------------------------------------------------------
# round 2: pooling for VGG, loss variants, gradient sinks, deterministic crops, drop-in loop
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,k,avg', [((2, 3, 9, 12), 3, False), ((2, 3, 9, 12), 3, True), ((1, 4, 8, 8), 4, True),
                                         ((3, 2, 7, 10), 2, True), ((2, 5, 6, 6), 1, False), ((2, 2, 11, 13), 5, False)])
def test_pool2d_general_windows(hip, shape, k, avg):
    """build_cnn 'P<k>' (layers.py:181-189): nn.MaxPool2d(k, k) / nn.AvgPool2d(k, k), forward and backward vs torch CPU (exact:
    a max copies, the average divides one fp32 sum)."""
    x = det(shape, 931 + k, 2.0)
    w = det((shape[0], shape[1], shape[2] // k, shape[3] // k), 932 + k, 1.0)
    xr = x.clone().requires_grad_()
    yr = (F.avg_pool2d if avg else F.max_pool2d)(xr, k, k)
    (yr * w).sum().backward()
    xh = x.to(DEV).requires_grad_()
    yh = hip.pool2d(xh, k, avg=avg)
    (yh * w.to(DEV)).sum().backward()
    close(yh, yr, 1e-6, 'pool2d fwd')
    close(xh.grad, xr.grad, 1e-6, 'pool2d bwd')


@pytest.mark.parametrize('padding_type,dropout', [('zero', False), ('replicate', False), ('reflect', False), ('replicate', True)])
def test_resnet_block_padding_types(hip, padding_type, dropout):
    """ResnetBlock with every padding_type of the reference (layers.py:234-273): same state_dict keys as the reference module
    (the pad modules shift the indices), outputs and gradients vs the oracle's torch modules."""
    from scene_generation_amd.layers import ResnetBlock, get_norm_layer
    dim = 16
    m = ResnetBlock(dim, padding_type, get_norm_layer('instance'), use_dropout=dropout)
    fill_deterministic(m)
    pad = {'zero': [], 'replicate': [nn.ReplicationPad2d(1)], 'reflect': [nn.ReflectionPad2d(1)]}[padding_type]
    p = 1 if padding_type == 'zero' else 0
    ref_block = nn.Sequential(*pad, nn.Conv2d(dim, dim, 3, padding=p), nn.InstanceNorm2d(dim), nn.ReLU(),
                              *([nn.Dropout(0.5)] if dropout else []),
                              *[type(q)(1) for q in pad], nn.Conv2d(dim, dim, 3, padding=p), nn.InstanceNorm2d(dim))
    assert sorted(m.conv_block.state_dict()) == sorted(ref_block.state_dict())
    ref_block.load_state_dict(m.conv_block.state_dict())
    m = m.to(DEV).eval()                 # eval: the dropout of the pix2pixHD option is the identity (its mask has no pin)
    ref_block.eval()
    x = det((2, dim, 9, 7), 941, 2.0)
    w = det((2, dim, 9, 7), 942, 1.0)
    xr = x.clone().requires_grad_()
    yr = xr + ref_block(xr)
    (yr * w).sum().backward()
    xh = x.to(DEV).requires_grad_()
    yh = m(xh)
    (yh * w.to(DEV)).sum().backward()
    close(yh, yr, 3e-5, 'ResnetBlock(%s) out' % padding_type)
    close(xh.grad, xr.grad, 1e-4, 'ResnetBlock(%s) gx' % padding_type)
    for (n, a), (_, b) in zip(m.conv_block.named_parameters(), ref_block.named_parameters()):
        close(a.grad, b.grad, 1e-4, 'ResnetBlock(%s) g %s' % (padding_type, n))


def test_replicate_pad_adjoint(hip):
    """sg_replicate_pad_fwd / _bwd vs F.pad(mode='replicate') incl. pad 2 on a 3x4 map and pad >= size on a 1x1 map"""
    for shape, pad in (((2, 3, 5, 6), 1), ((1, 2, 3, 4), 2), ((2, 1, 1, 1), 3)):
        x = det(shape, 951 + pad, 1.0)
        w = det((shape[0], shape[1], shape[2] + 2 * pad, shape[3] + 2 * pad), 952 + pad, 1.0)
        xr = x.clone().requires_grad_()
        yr = F.pad(xr, (pad,) * 4, mode='replicate')
        (yr * w).sum().backward()
        xh = x.to(DEV).requires_grad_()
        yh = hip.replicate_pad(xh, pad)
        (yh * w.to(DEV)).sum().backward()
        assert torch.equal(yh.cpu(), yr)
        close(xh.grad, xr.grad, 1e-6, 'replicate pad bwd')


def test_build_cnn_pooling_layers(hip):
    """build_cnn with 'P3' max pooling and 'P2' average pooling (layers.py:181-189) against the oracle's build_cnn."""
    from scene_generation_amd.layers import build_cnn
    for arch, pooling in (('I4,C3-8,P3,C3-8', 'max'), ('I4,C3-8,P2,C3-8,P2', 'avg')):
        m, c = build_cnn(arch, normalization='batch', activation='leakyrelu-0.2', pooling=pooling)
        r, c2 = O.build_cnn(arch, normalization='batch', activation='leakyrelu-0.2', pooling=pooling)
        assert c == c2 == 8 and sorted(m.state_dict()) == sorted(r.state_dict())
        fill_deterministic(m)
        r.load_state_dict(m.state_dict())
        x = det((3, 4, 12, 12), 961, 2.0)
        close(m.to(DEV)(x.to(DEV)), r(x), 3e-5, 'build_cnn %s' % arch)


@pytest.mark.parametrize('shape', [(3, 5, 8, 12), (2, 4, 7, 9), (1, 2, 2, 2), (2, 64, 32, 32)])
def test_maxpool2(hip, shape):
    x = det(shape, 301)
    x[0, 0, :2, :2] = 0.25                                   # a tie: the first element of the window must win
    xr = x.clone().requires_grad_()
    yr = F.max_pool2d(xr, 2, 2)
    gy = det(tuple(yr.shape), 302)
    yr.backward(gy)
    xg = x.to(DEV).requires_grad_()
    yg = hip.maxpool2(xg)
    yg.backward(gy.to(DEV))
    assert torch.equal(yg.cpu(), yr)
    assert torch.equal(xg.grad.cpu(), xr.grad)


def test_loss_variants_vs_reference(hip, golden):
    """--gan_loss_type wgan | lsgan and GANLoss(use_lsgan=False) against the reference goldens (losses.py:93-132,147)."""
    from scene_generation_amd import losses as Lh
    g = golden('losses_variants')
    for name, two in [('wgan_g', False), ('wgan_d', True), ('lsgan_g', False), ('lsgan_d', True)]:
        gl, dl = Lh.get_gan_losses(name.split('_')[0])
        sr, sf = [torch.from_numpy(g[k]).to(DEV).requires_grad_() for k in ('sr', 'sf')]
        v = dl(sr, sf) if two else gl(sf)
        close(v, g[name], 2e-6, name)
        v.backward()
        close(sf.grad, g[name + '_gsf'], 2e-6)
        if two:
            close(sr.grad, g[name + '_gsr'], 2e-6)
    crit = Lh.GANLoss(use_lsgan=False)
    for t in (True, False):
        p0, p1 = [torch.from_numpy(g[k]).to(DEV).requires_grad_() for k in ('p0', 'p1')]
        v = crit([[None, p0], [None, p1]], t)
        close(v, g['bce_%d' % t], 2e-6)
        v.backward()
        close(p0.grad, g['bce_%d_g0' % t], 2e-6)
        close(p1.grad, g['bce_%d_g1' % t], 2e-6)


def test_vgg_loss_vs_reference_golden(hip, golden):
    """VGGLoss (losses.py:179-224) through the HIP conv / max-pool kernels against the reference's own classes (golden
    captured on the torchvision shim, tools/make_golden.py::golden_vgg): features, loss, d loss / d x."""
    from scene_generation_amd import losses as Lh
    g = golden('vgg_loss')
    crit = Lh.VGGLoss()
    assert list(crit.vgg.state_dict().keys()) == g['keys'].tolist()
    fill_deterministic(crit.vgg)
    crit = crit.to(DEV)
    x = torch.from_numpy(g['x']).to(DEV).requires_grad_()
    feats = crit.vgg(x)
    close(feats[0][:, :4], g['feat0'], 3e-5, 'relu1_1')
    close(feats[4], g['feat4'], 3e-5, 'relu5_1')
    loss = crit(x, torch.from_numpy(g['y']).to(DEV))
    close(loss, g['loss'], 2e-5, 'vgg loss')
    loss.backward()
    close(x.grad, g['gx'], 1e-4, 'd vgg / d x')
    assert all(p.grad is None for p in crit.parameters())          # frozen network: data gradients only


def test_vgg_full_width_vs_oracle(hip):
    """VGG19 at the widths / plane sizes of the training step (128x128 input: Winograd for the >= 128-channel convs, direct
    kernels for the 3/64-channel ones) vs the oracle restatement, He-normal weights."""
    from scene_generation_amd import losses as Lh
    mine = Lh.VGGLoss()
    ref = O.VGGLoss()
    ref.vgg.load_state_dict(mine.vgg.state_dict())
    mine = mine.to(DEV)
    x, y = det((8, 3, 128, 128), 311), det((8, 3, 128, 128), 312)
    xr = x.clone().requires_grad_()
    lr = ref(xr, y)
    lr.backward()
    xg = x.to(DEV).requires_grad_()
    lg = mine(xg, y.to(DEV))
    lg.backward()
    close(lg, lr, 1e-4, 'vgg loss')
    rel = float((xg.grad.cpu() - xr.grad).norm() / xr.grad.norm())
    assert rel < 2e-3, 'd vgg / d x relative L2 error %.3e' % rel     # 16 ReLU layers: a few units flip (see _compare_grads)


def test_weighted_sum_and_gradient_sinks(hip):
    """ops.weighted_sum (one launch) and the parameter-gradient sinks of FusedAdam: kernels write straight into the flat
    gradient buffer; a second backward before zero_grad() ACCUMULATES like torch; untouched parameters are skipped."""
    from scene_generation_amd.optim import FusedAdam
    from scene_generation_amd import layers as Lh
    ts = [det((1,), 320 + i).to(DEV).requires_grad_() for i in range(40)]
    ws = [0.1 * (i - 7) for i in range(40)]
    tot = hip.weighted_sum([t.reshape(()) for t in ts], ws)
    close(tot, sum(w * float(t) for w, t in zip(ws, ts)), 1e-6)
    tot.backward()
    for w, t in zip(ws, ts):
        close(t.grad, torch.tensor([w]), 1e-6)
    net = nn.Sequential(Lh.Conv2d(3, 8, 3, padding=1), Lh.BatchNorm2d(8), Lh.ReLU(), Lh.Conv2d(8, 4, 3, padding=1)).to(DEV)
    unused = Lh.Linear(5, 5).to(DEV)
    fill_deterministic(net)
    ref = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(), nn.Conv2d(8, 4, 3, padding=1))
    ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    opt = FusedAdam(list(net.parameters()) + list(unused.parameters()), lr=1e-3)
    x = det((2, 3, 8, 8), 330)
    opt.zero_grad()
    for rep in range(2):                                    # two backwards, one zero_grad: gradients add up
        net(x.to(DEV)).pow(2).sum().backward()
        ref(x).pow(2).sum().backward()
    for (n, p), q in zip(net.named_parameters(), ref.parameters()):
        assert p.grad.data_ptr() == opt.fp.grad_view([id(a) for a in opt.fp.params].index(id(p))).data_ptr()
        close(p.grad, q.grad, 1e-4, n)
    assert opt._touched == [True] * 6 + [False] * 2
    before = unused.weight.detach().clone()
    opt.step()
    assert torch.equal(unused.weight, before) and opt.steps == [1] * 6 + [0] * 2


def test_lazy_zero_grad_equals_eager_fill(hip):
    """FusedAdam(lazy_zero=True) -- what the Trainer builds: zero_grad() launches no fill; the first contribution of a step
    overwrites its slice, the slices nobody wrote are zeroed when the first backward ends.  Against the eager-fill optimiser over
    four steps with a parameter that is never used, one used every other step, a second backward without zero_grad() and a
    gradient autograd itself produces (a plain torch op on a parameter): same parameters, same moments, same step counts, bit for
    bit; ``p.grad`` is None between zero_grad() and the backward (torch's set_to_none) and the flat slice afterwards."""
    from scene_generation_amd.optim import FusedAdam
    from scene_generation_amd import layers as Lh

    def build():
        net = nn.Sequential(Lh.Conv2d(3, 8, 3, padding=1), Lh.BatchNorm2d(8), Lh.ReLU(), Lh.Conv2d(8, 4, 3, padding=1)).to(DEV)
        mid = Lh.Linear(4, 4).to(DEV)
        unused = Lh.Linear(5, 5).to(DEV)
        scale = nn.Parameter(torch.full((4,), 0.7, device=DEV))          # multiplied in with a plain torch op below
        fill_deterministic(net)
        fill_deterministic(mid)
        fill_deterministic(unused)
        return net, mid, unused, scale

    x = det((2, 3, 8, 8), 350).to(DEV)
    res = {}
    for lazy in (True, False):
        net, mid, unused, scale = build()
        params = list(net.parameters()) + list(mid.parameters()) + list(unused.parameters()) + [scale]
        opt = FusedAdam(params, lr=1e-2, betas=(0.5, 0.999), lazy_zero=lazy)
        assert opt.lazy_zero == lazy
        # stale data every step would have to overwrite: what the previous iteration left in the buffer, made loud
        for it in range(4):
            if lazy:
                for i in range(len(params)):           # (the alignment gaps between slices are never written: they stay zero)
                    opt.fp.grad_view(i).fill_(1e30)
            opt.zero_grad()
            if lazy:
                assert all(p.grad is None for p in params)
            for rep in range(2 if it == 3 else 1):
                h = net(x) * scale.view(1, 4, 1, 1)
                h = h.mean((2, 3))
                if it % 2 == 0:
                    h = mid(h)
                h.pow(2).sum().backward()
            for i, p in enumerate(params):
                assert p.grad is not None and p.grad.data_ptr() == opt.fp.grad_view(i).data_ptr()
            assert float(unused.weight.grad.abs().max()) == 0.0 and float(unused.bias.grad.abs().max()) == 0.0
            if it % 2 == 1:
                assert float(mid.weight.grad.abs().max()) == 0.0
            opt.step()
        res[lazy] = ([p.detach().clone() for p in params], opt.exp_avg.clone(), opt.exp_avg_sq.clone(), list(opt.steps))
    assert res[True][3] == res[False][3] == [4] * 6 + [2] * 2 + [0] * 2 + [4]
    for a, c in zip(res[True][0], res[False][0]):
        assert torch.equal(a, c)
    assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])


def test_crop_backward_is_deterministic_and_exact(hip):
    """the gather form of the crop gradient: bit-identical run to run, equals the transpose of the forward (autograd of
    F.grid_sample) incl. permuted / repeated / out-of-range boxes and up-sampling crops"""
    from scene_generation_amd.bilinear import crop_bbox_batch
    g = torch.Generator().manual_seed(5)
    feats = det((3, 3, 24, 20), 340)
    B = 14
    x0, y0 = torch.rand(B, generator=g) * 0.6, torch.rand(B, generator=g) * 0.6
    boxes = torch.stack([x0, y0, x0 + 0.05 + 0.5 * torch.rand(B, generator=g), y0 + 0.05 + 0.5 * torch.rand(B, generator=g)], 1)
    boxes[0] = torch.tensor([0., 0., 1., 1.])
    boxes[1] = torch.tensor([-0.2, 0.3, 0.4, 1.3])
    boxes[2] = torch.tensor([0.45, 0.45, 0.5, 0.5])            # tiny box, strongly up-sampled
    idx = torch.tensor([2, 0, 1, 1, 0, 2, 2, 0, 1, 0, 0, 2, 1, 1])
    for HH in (8, 32):
        fr = feats.clone().requires_grad_()
        out_r = O.crop_bbox_batch(fr, boxes, idx, HH)
        w = det(tuple(out_r.shape), 341)
        (out_r * w).sum().backward()
        grads = []
        for rep in range(2):
            fg = feats.to(DEV).requires_grad_()
            out = crop_bbox_batch(fg, boxes.to(DEV), idx.to(DEV), HH)
            (out * w.to(DEV)).sum().backward()
            grads.append(fg.grad.clone())
        close(out, out_r, 1e-5, 'crop')
        close(grads[0], fr.grad, 2e-5, 'crop gradient')
        assert torch.equal(grads[0], grads[1])


def test_boxes_to_layout_intended_semantics(hip):
    """boxes_to_layout (layout.py:28-61) raises TypeError in the reference: the intended semantics --
    every object paints its vector over its box (an all-ones 8x8 mask, layout.py:50) -- vs the oracle's statement of the
    same; parity with the reference itself is unpinned for this one function."""
    from scene_generation_amd.layout import boxes_to_layout, masks_to_layout
    b = make_batch(N=3, min_objs=2, max_objs=5, size=32, seed=77)
    vecs = det((b.objs.numel(), 9), 350)
    for pooling in ('sum', 'avg'):
        vr = vecs.clone().requires_grad_()
        ref = O.boxes_to_layout(vr, b.boxes, b.obj_to_img, 24, 32, pooling=pooling)
        w = det(tuple(ref.shape), 351)
        (ref * w).sum().backward()
        vg = vecs.to(DEV).requires_grad_()
        out = boxes_to_layout(vg, b.boxes.to(DEV), b.obj_to_img.to(DEV), 24, 32, pooling=pooling)
        (out * w.to(DEV)).sum().backward()
        close(out, ref, 1e-5, 'boxes_to_layout ' + pooling)
        close(vg.grad, vr.grad, 2e-5, 'boxes_to_layout gradient')
    # inside a box (away from its border) the layout is exactly the object's vector; outside every box it is zero
    one = boxes_to_layout(torch.ones(1, 2, device=DEV), torch.tensor([[0.25, 0.25, 0.75, 0.75]], device=DEV),
                          torch.zeros(1, dtype=torch.long, device=DEV), 32)
    assert float(one[0, :, 12:20, 12:20].min()) == 1.0 and float(one[0, :, :6].abs().max()) == 0.0


def _filled_trainer(args, vocab, *extra):
    """HIP Trainer whose four networks carry the deterministic fill; built without the random initialisation that the fill
    overwrites (conftest.skip_random_init: ~5 s per full-width Trainer)"""
    from conftest import skip_random_init
    from scene_generation_amd.trainer import Trainer
    with skip_random_init():
        tr = Trainer(args, vocab, *extra)
    for m in (tr.model, tr.netD, tr.obj_discriminator, tr.mask_discriminator):
        fill_deterministic(m)
    return tr


_PAIRS = {}          # (argv without --batch_size, with_vgg) -> dict(args, ref, tr, init): ONE full-width pair alive at a time


def _trainer_pair(argv, vocab, with_vgg):
    """(args, oracle Trainer, HIP Trainer) with the deterministic fill in the oracle.  Pairs are CACHED per configuration
    (``--batch_size`` is not part of a Trainer: nothing reads it) and handed out again restored to their initial state --
    modules, optimisers, VectorPools, per-test attributes -- so the three 128x128 / VGG-off full-size tests build two 183 M-
    parameter trainers once instead of three times; construction skips the random initialisation every parameter loses to
    fill_deterministic a moment later (the suite ran 887 s of the driver's 1200 s limit)."""
    from conftest import skip_random_init
    from scene_generation_amd.trainer import Trainer
    from scene_generation_amd.utils import VectorPool
    key_argv = tuple(a for i, a in enumerate(argv) if a != '--batch_size' and (i == 0 or argv[i - 1] != '--batch_size'))
    key = (key_argv, bool(with_vgg), tuple(sorted(vocab['object_to_idx'])) if isinstance(vocab, dict) else None)
    args = parser.parse_args(argv)
    hit = _PAIRS.get(key)
    if hit is None:
        _PAIRS.clear()
        import gc
        gc.collect()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        with skip_random_init():
            ref = O.Trainer(args, vocab)
            for m in (ref.model, ref.netD, ref.obj_discriminator, ref.mask_discriminator):
                fill_deterministic(m)
            tr = Trainer(args, vocab)
            for m in (tr.model, tr.netD, tr.obj_discriminator, tr.mask_discriminator):
                fill_deterministic(m)         # (cached patterns: a memcpy; a never-initialised parameter must not survive)
        if with_vgg:
            ref.criterionVGG.vgg.load_state_dict({k: v.cpu() for k, v in tr.criterionVGG.vgg.state_dict().items()})
        hit = _PAIRS[key] = dict(ref=ref, tr=tr, init_ref=_snapshot(ref), init_tr=_snapshot(tr))
    else:
        ref, tr = hit['ref'], hit['tr']
        _restore(ref, hit['init_ref'])
        _restore(tr, hit['init_tr'])
        ref.model.fake_pool = type(ref.model.fake_pool)(ref.model.fake_pool.pool_size)
        tr.model.fake_pool = VectorPool(tr.model.fake_pool.pool_size)
        tr.model.layout_objects_hint = 0
        tr.share_d_forward = True
        tr._shared = {}
        for t_ in (ref, tr):
            t_.args = args
    return args, hit['ref'], hit['tr']


def _snapshot(ref):
    import copy
    return ([copy.deepcopy(m.state_dict()) for m in (ref.model, ref.netD, ref.obj_discriminator, ref.mask_discriminator)],
            [copy.deepcopy(getattr(ref, n).state_dict()) for n in ('optimizer', 'optimizer_d_mask', 'optimizer_d_obj',
                                                                    'optimizer_d_img')], copy.deepcopy(ref.model.fake_pool))


def _restore(tr, snap):
    import copy
    for m, sd in zip((tr.model, tr.netD, tr.obj_discriminator, tr.mask_discriminator), snap[0]):
        m.load_state_dict(sd)
    for n, sd in zip(('optimizer', 'optimizer_d_mask', 'optimizer_d_obj', 'optimizer_d_img'), snap[1]):
        getattr(tr, n).load_state_dict(sd)


def _step_metrics(tr, ref, out, out_ref, snaps):
    """measured deviations of one HIP step from the oracle step (recorded to gpurun_out/ before anything is asserted)"""
    m = {}
    for n, a, b in zip(['imgs_pred', 'boxes_pred', 'masks_pred', 'layout', 'layout_pred', 'layout_wrong'], out, out_ref):
        m['out_' + n] = float((a.detach().cpu() - b.detach()).abs().max()) / max(1.0, float(b.detach().abs().max()))
    for tag, La, Lb in [('g', tr.generator_losses, ref.generator_losses), ('dmask', tr.d_mask_losses, ref.d_mask_losses),
                        ('dobj', tr.d_obj_losses, ref.d_obj_losses), ('dimg', tr.d_img_losses, ref.d_img_losses)]:
        a, b = dict(La.items()), dict(Lb.items())
        assert set(a) == set(b), (sorted(a), sorted(b))
        for k in b:
            m['loss_%s_%s' % (tag, k)] = abs(a[k] - b[k]) / max(1.0, abs(b[k]))
    for n, gr in snaps['ref'].items():
        gh = snaps['hip'][n]
        fa, fb = gh.flat_pair(gr)                     # float64, on the device
        fbn = float(fb.norm())
        m['cos_' + n] = float(fa @ fb / (fa.norm() * fb.norm() + 1e-30))
        m['rel_' + n] = float((fa - fb).norm() / (fbn + 1e-30))
        dn, bn = _seg_norms(fa - fb, gh), _seg_norms(fb, gh)
        big = bn > 1e-3 * fbn
        m['worst_tensor_rel_' + n] = float((dn[big] / bn[big]).max()) if bool(big.any()) else 0.0
    return m


def _assert_step_metrics(m, tag, out_tol, loss_tol, cos_min=0.9995, worst_tol=3e-2):
    bad = []
    for k, v in m.items():
        if k.startswith('out_') and not v <= out_tol:
            bad.append((k, v))
        elif k.startswith('loss_') and not v <= loss_tol:
            bad.append((k, v))
        elif k.startswith('cos_') and not v > cos_min:
            bad.append((k, v))
        elif k.startswith('worst_tensor_rel_') and not v <= worst_tol:
            bad.append((k, v))
    assert not bad, '%s: %s' % (tag, bad)


# Whole-step bounds of the full-size cases, ~2.5x the deviations measured on MI355X (profiles/r04_parity_headline_n32.json,
# r04_parity_config5_step.json: imgs_pred 4.2e-5, losses 1.9e-7, generator gradient cosine 0.999982..0.999997, worst tensor
# 8.7e-3 / 1.15e-2) -- VERDICT r4: the round-2 bounds (3e-4 / 2e-3 / 0.9995 / 3e-2) let a 5x accuracy regression pass
FULL_SIZE_BOUNDS = dict(out_tol=1e-4, loss_tol=1e-6, cos_min=0.9999, worst_tol=2.5e-2)


def test_full_step_at_benchmark_shape_vs_oracle(hip):
    """BASELINE configs[1] shape -- 128x128, <= 8 objects per image, reference default widths and DEFAULT FLAGS (VGG loss on)
    -- at N = 8 images (8*4*4 = 128 Winograd tiles in the 1024-channel trunk, i.e. every kernel family the bench line runs:
    Winograd fwd/dgrad/wgrad, factored 204-channel layout convs, 128x128 tiles + split-K, single-launch parity classes,
    shared D forwards, gradient sinks) against the oracle Trainer: outputs, all named losses, every parameter gradient of
    all four optimisers, two iterations (use_gt on / off).  The same two iterations with every fast path switched OFF
    (Winograd, factored layout, shared D forwards, lazy layouts) are checked against the same oracle run."""
    from scene_generation_amd import ops
    argv = ['--image_size', '128,128', '--batch_size', '8', '--output_dir', '/tmp/o']
    vocab = make_vocab()
    args, ref, tr_fast = _trainer_pair(argv, vocab, True)
    from scene_generation_amd.trainer import Trainer
    from conftest import skip_random_init
    with skip_random_init():               # (its state is restored from the oracle's snapshot before every step)
        tr_plain = Trainer(args, vocab)
    tr_plain.share_d_forward = False
    tr_plain.criterionVGG.vgg.load_state_dict(tr_fast.criterionVGG.vgg.state_dict())
    variants = [('fast', tr_fast, True), ('plain', tr_plain, False)]
    snaps = {}
    for name, tr, _ in variants:
        snaps[name], _h = _grad_snapshots(ref, tr)
    report = {}
    saved = (ops.WINOGRAD, ops.FACTORED_LAYOUT)
    try:
        for it in range(2):
            batch = make_batch(N=8, min_objs=3, max_objs=8, size=128, seed=40 + it)
            noise = det((1, args.mask_noise_dim), 141 + it)
            pre = _snapshot(ref)
            pool = pre[2]
            ref.model.noise_override = noise
            random.seed(15 + it)
            out_ref = ref.step(batch, use_gt=(it == 0))
            for name, tr, fast in variants:
                import copy
                _restore(tr, pre)
                tr.model.noise_override = noise
                ops.WINOGRAD = ops.FACTORED_LAYOUT = fast
                random.seed(15 + it)
                out = tr.step(batch_to(batch, DEV), use_gt=(it == 0))
                snaps[name]['ref'] = snaps['fast']['ref'] if name != 'fast' else snaps[name]['ref']
                report['%s_it%d' % (name, it)] = _step_metrics(tr, ref, out, out_ref, snaps[name])
    finally:
        ops.WINOGRAD, ops.FACTORED_LAYOUT = saved
    _dump('parity_benchmark_shape.json', report)
    for k, m in report.items():
        _assert_step_metrics(m, k, 3e-4, 2e-3)


def test_config4_shape_vs_oracle(hip):
    """BASELINE configs[3] per-GPU shape (256x256, <= 16 objects per image, default widths, default flags incl. VGG) at
    N = 2: outputs and every named loss of one G+D step against the oracle."""
    from scene_generation_amd.synthetic import make_config_batch
    argv = ['--image_size', '256,256', '--batch_size', '2', '--output_dir', '/tmp/o']
    args, ref, tr = _trainer_pair(argv, make_vocab(), True)
    _sync_state(ref, tr)
    b = make_config_batch('c4', seed=5, N=2)
    noise = det((1, args.mask_noise_dim), 151)
    ref.model.noise_override = tr.model.noise_override = noise
    random.seed(3)
    out_ref = ref.step(b, use_gt=True)
    random.seed(3)
    out = tr.step(batch_to(b, DEV), use_gt=True)
    m = _step_metrics(tr, ref, out, out_ref, {'ref': {}, 'hip': {}})
    _dump('parity_config4_shape.json', m)
    _assert_step_metrics(m, 'config4', 3e-4, 2e-3)


def test_full_step_n32_vs_oracle(hip):
    """THE headline workload at full size (VERDICT r3 "missing" 2): BASELINE configs[1] exactly as bench.py times it -- 128x128,
    3..8 objects per image, batch 32, reference default widths, VGG loss off -- one full G+D step against the
    oracle Trainer: the six outputs, all 16 named losses and the flat gradients of all four optimisers (cosine, relative L2,
    worst tensor).  The oracle needs ~15 s for the step on the GPU box's host cores."""
    argv = ['--image_size', '128,128', '--batch_size', '32', '--vgg_features_weight', '0', '--output_dir', '/tmp/o']
    args, ref, tr = _trainer_pair(argv, make_vocab(), False)
    _sync_state(ref, tr)
    tr.model.layout_objects_hint = 9                    # as bench.py sets it (static shapes for the factored layout convs)
    snaps, _ = _grad_snapshots(ref, tr)
    batch = make_batch(N=32, min_objs=3, max_objs=8, size=128, seed=1000)        # bench.py's first host batch of rank 0
    noise = det((1, args.mask_noise_dim), 171)
    ref.model.noise_override = tr.model.noise_override = noise
    random.seed(21)
    out_ref = ref.step(batch, use_gt=True)
    random.seed(21)
    out = tr.step(batch_to(batch, DEV), use_gt=True)
    m = _step_metrics(tr, ref, out, out_ref, snaps)
    _dump('parity_headline_n32.json', m)
    _assert_step_metrics(m, 'headline_n32', **FULL_SIZE_BOUNDS)


def test_config5_step_vs_oracle(hip):
    """BASELINE configs[4] (the GraphTripleConv scatter stress: 32 objects + __image__ and 96 triples per image, 128x128,
    default widths) at N = 4 (O = 132, T = 384): one full G+D step against the oracle -- outputs, every named loss and the flat
    gradients of all four optimisers.  The graph pool itself is bit-exact (test_triple_pool_bit_exact at O = 1056 / T = 3072,
    graph.py:94-116); this pins the whole step at that graph density: 33 object planes per image in the factored layout
    convs, 132 crops through the object discriminator, 132 masks through mask_net and the mask discriminator."""
    from scene_generation_amd.synthetic import make_config_batch
    argv = ['--image_size', '128,128', '--batch_size', '4', '--vgg_features_weight', '0', '--output_dir', '/tmp/o']
    args, ref, tr = _trainer_pair(argv, make_vocab(), False)
    _sync_state(ref, tr)
    snaps, _ = _grad_snapshots(ref, tr)
    b = make_config_batch('c5', seed=11, N=4)
    assert b.objs.numel() == 4 * 33 and b.triples.size(0) == 4 * 96
    noise = det((1, args.mask_noise_dim), 181)
    ref.model.noise_override = tr.model.noise_override = noise
    random.seed(23)
    out_ref = ref.step(b, use_gt=True)
    random.seed(23)
    out = tr.step(batch_to(b, DEV), use_gt=True)
    m = _step_metrics(tr, ref, out, out_ref, snaps)
    _dump('parity_config5_step.json', m)
    _assert_step_metrics(m, 'config5', **FULL_SIZE_BOUNDS)


@pytest.mark.slow
def test_config5_step_n32_vs_oracle(hip):
    """BASELINE configs[4] at ITS size: 32 objects + __image__ and 96 triples per image, N = 32 -- O = 1056,
    T = 3072, the shape of bench.py's c5 leg -- one full G+D step against the oracle at default widths.  The oracle needs
    a minute or two on the GPU box's host cores (1056 crops / masks through the object-side networks)."""
    from scene_generation_amd.synthetic import make_config_batch
    argv = ['--image_size', '128,128', '--batch_size', '32', '--vgg_features_weight', '0', '--output_dir', '/tmp/o']
    args, ref, tr = _trainer_pair(argv, make_vocab(), False)
    _sync_state(ref, tr)
    tr.model.layout_objects_hint = 33
    snaps, _ = _grad_snapshots(ref, tr)
    b = make_config_batch('c5', seed=2000)                 # the first host batch of bench.py's c5 leg
    assert b.objs.numel() == 1056 and b.triples.size(0) == 3072
    noise = det((1, args.mask_noise_dim), 191)
    ref.model.noise_override = tr.model.noise_override = noise
    random.seed(29)
    out_ref = ref.step(b, use_gt=True)
    random.seed(29)
    out = tr.step(batch_to(b, DEV), use_gt=True)
    m = _step_metrics(tr, ref, out, out_ref, snaps)
    _dump('parity_config5_step_n32.json', m)
    _assert_step_metrics(m, 'config5_n32', **FULL_SIZE_BOUNDS)


def test_check_indices_option_raises_index_error(hip):
    """``sg_set_option("check_indices", 1)``: a triple that names a node outside the batch, an object class outside the
    vocabulary and a crop that names an image outside the batch raise IndexError -- what the reference's indexing does at
    graph.py:79-80, model.py:131-132 and bilinear.py:36 -- instead of reading / corrupting memory; valid operands pass; with
    the option off (the default) nothing is checked and nothing synchronises."""
    from scene_generation_amd import _hip
    from scene_generation_amd.graph import GraphTripleConv
    assert _hip.get_option('check_indices') == 0
    m = GraphTripleConv(16, output_dim=16, hidden_dim=32).to(DEV)
    obj, pred = torch.randn(6, 16, device=DEV), torch.randn(4, 16, device=DEV)
    good = torch.tensor([[0, 1], [2, 3], [4, 5], [5, 0]], device=DEV)
    bad = good.clone()
    bad[2, 1] = 6                                          # one past the last node
    neg = good.clone()
    neg[0, 0] = -1
    table = torch.randn(5, 8, device=DEV)
    feats, boxes = torch.randn(2, 3, 8, 8, device=DEV), torch.tensor([[0., 0., 1., 1.]] * 3, device=DEV)
    _hip.set_option('check_indices', 1)
    try:
        m(obj, pred, good)
        for e in (bad, neg):
            with pytest.raises(IndexError, match='edges'):
                m(obj, pred, e)
            with pytest.raises(IndexError, match='edges'):
                hip.build_csr(e.clone(), 6)                # the C entry point itself (sg_build_csr returns SG_ERR_INDEX)
        hip.embedding(table, torch.tensor([0, 4, 2], device=DEV))
        with pytest.raises(IndexError, match=r'\[1\] = 5 is not in \[0, 5\)'):
            hip.embedding(table, torch.tensor([0, 5, 2], device=DEV))
        hip.CropBBoxFn.apply(feats, boxes, torch.tensor([0, 1, 1], device=DEV), 4, 4)
        with pytest.raises(IndexError, match='bbox_to_feats'):
            hip.CropBBoxFn.apply(feats, boxes, torch.tensor([0, 2, 1], device=DEV), 4, 4)
    finally:
        _hip.set_option('check_indices', 0)
    m(obj, pred, good)                                     # unchecked path still runs


def test_step_is_bit_reproducible(hip):
    """The same G+D step from the same state twice: outputs, losses, every gradient and every updated parameter are
    bit-identical (segmented sums, split-K slabs and the crop gradient all add in a fixed order; no atomics anywhere)."""
    from scene_generation_amd.trainer import Trainer
    args = parser.parse_args(['--image_size', '64,64', '--batch_size', '4', '--output_dir', '/tmp/o'])
    b = batch_to(make_batch(N=4, min_objs=3, max_objs=6, size=64, seed=9), DEV)
    res = []
    for rep in range(2):
        torch.manual_seed(0)
        tr = _filled_trainer(args, make_vocab())
        tr.model.noise_override = det((1, 64), 131).to(DEV)
        grads = {}
        for n in ('optimizer', 'optimizer_d_mask', 'optimizer_d_obj', 'optimizer_d_img'):
            o = getattr(tr, n)
            o.pre_step_hooks.append(lambda o=o, n=n: grads.__setitem__(n, o.fp.grad.clone()))
        random.seed(3)
        out = tr.step(b, use_gt=True)
        losses = {}
        for L in (tr.generator_losses, tr.d_img_losses, tr.d_obj_losses, tr.d_mask_losses):
            losses.update(dict(L.items()))
        params = torch.cat([getattr(tr, n).fp.flat for n in ('optimizer', 'optimizer_d_mask', 'optimizer_d_obj',
                                                            'optimizer_d_img')])
        res.append(([o.detach().clone() for o in out], losses, grads, params.clone()))
        del tr
    for a, b_ in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b_)
    assert res[0][1] == res[1][1]
    for n in res[0][2]:
        assert torch.equal(res[0][2][n], res[1][2][n]), n
    assert torch.equal(res[0][3], res[1][3])


def test_batched_real_and_wrong_discriminator_passes_equal_separate_passes(hip):
    """Trainer._real_and_wrong_pass: the image discriminator's real and wrong-texture passes run as one 2N batch over the stacked
    factored layouts.  Same step from the same state with the batch on and off: every named loss, the discriminator gradients and
    the updated parameters agree to fp32 summation order (InstanceNorm is per sample, so the batch halves ARE the two passes)."""
    from scene_generation_amd.trainer import Trainer
    args = parser.parse_args(['--image_size', '64,64', '--batch_size', '4', '--vgg_features_weight', '0', '--output_dir', '/tmp/o'])
    b = batch_to(make_batch(N=4, min_objs=3, max_objs=6, size=64, seed=19), DEV)
    res = []
    for batched in (True, False):
        torch.manual_seed(0)
        tr = _filled_trainer(args, make_vocab())
        tr.batch_real_wrong = batched
        tr.model.noise_override = det((1, 64), 133).to(DEV)
        grads = {}
        tr.optimizer_d_img.pre_step_hooks.append(lambda o=tr.optimizer_d_img: grads.__setitem__('d_img', o.fp.grad.clone()))
        calls0 = hip.CALLS[0]
        random.seed(3)
        tr.step(b, use_gt=True)
        calls = hip.CALLS[0] - calls0
        losses = {}
        for L in (tr.generator_losses, tr.d_img_losses, tr.d_obj_losses, tr.d_mask_losses):
            losses.update(dict(L.items()))
        res.append((losses, grads['d_img'], tr.optimizer_d_img.fp.flat.detach().clone(), tr.optimizer.fp.flat.detach().clone(), calls))
        del tr
    (la, ga, pa, gpa, ca), (lb, gb, pb, gpb, cb) = res
    assert set(la) == set(lb)
    for k in lb:
        assert abs(la[k] - lb[k]) <= 2e-6 * max(1.0, abs(lb[k])), (k, la[k], lb[k])
    close(ga, gb, 2e-5, 'image-discriminator flat gradient')
    cos = float((ga.double() @ gb.double()) / (ga.double().norm() * gb.double().norm()))
    assert cos > 0.999999, cos
    close(gpa, gpb, 1e-6, 'generator parameters (untouched by the batching)')
    assert ca < cb, 'the batched form issues fewer launches (%d vs %d)' % (ca, cb)


def test_reference_training_loop_through_the_alias(hip):
    """train.py:190-215 re-stated statement by statement against the ``scene_generation.*`` names that
    install_as() provides -- plain ``.detach()`` on the layouts, the one-hot channel slices, the four trainer calls -- gives
    exactly what Trainer.step gives."""
    import scene_generation_amd
    scene_generation_amd.install_as('scene_generation', host_package_dir='')
    from scene_generation.trainer import Trainer
    from scene_generation.args import get_args
    args = get_args(['--image_size', '64,64', '--batch_size', '4', '--output_dir', '/tmp/o'])
    vocab = make_vocab()
    batch = batch_to(make_batch(N=4, min_objs=3, max_objs=6, size=64, seed=19), DEV)
    res = []
    for loop in ('reference', 'step'):
        torch.manual_seed(0)
        checkpoint = {'model_kwargs': {}, 'd_obj_kwargs': {}, 'd_mask_kwargs': {}, 'd_img_kwargs': {}, 'losses': {},
                      'd_losses': {}, 'losses_ts': []}
        trainer = _filled_trainer(args, vocab, checkpoint)
        trainer.model.noise_override = det((1, 64), 171).to(DEV)
        random.seed(11)
        if loop == 'step':
            out = trainer.step(batch, use_gt=True)
            imgs_pred = out[0]
        else:
            imgs, objs, boxes, masks, triples, obj_to_img, triple_to_img, attributes = batch
            use_gt = True
            model_out = trainer.model(imgs, objs, triples, obj_to_img, boxes_gt=boxes, masks_gt=masks, attributes=attributes)
            imgs_pred, boxes_pred, masks_pred, layout, layout_pred, layout_wrong = model_out
            layout_one_hot = layout[:, :trainer.num_obj, :, :]
            layout_pred_one_hot = layout_pred[:, :trainer.num_obj, :, :]
            trainer.train_generator(imgs, imgs_pred, masks, masks_pred, layout, objs, boxes, boxes_pred, obj_to_img, use_gt)
            imgs_pred_detach = imgs_pred.detach()
            masks_pred_detach = masks_pred.detach()
            boxes_pred_detach = boxes.detach()
            layout_detach = layout.detach()
            layout_wrong_detach = layout_wrong.detach()
            trainer.train_mask_discriminator(masks, masks_pred_detach, objs)
            trainer.train_obj_discriminator(imgs, imgs_pred_detach, objs, boxes, boxes_pred_detach, obj_to_img)
            trainer.train_image_discriminator(imgs, imgs_pred_detach, layout_detach, layout_wrong_detach)
            trainer.write_losses(checkpoint, 1)
            trainer.write_images(1, imgs, imgs_pred, layout_one_hot, layout_pred_one_hot)
            assert checkpoint['losses_ts'] == [1] and 'total_loss' in checkpoint['losses']
        losses = {}
        for L in (trainer.generator_losses, trainer.d_img_losses, trainer.d_obj_losses, trainer.d_mask_losses):
            losses.update(dict(L.items()))
        flat = torch.cat([getattr(trainer, n).fp.flat for n in ('optimizer', 'optimizer_d_mask', 'optimizer_d_obj',
                                                                 'optimizer_d_img')]).clone()
        res.append((imgs_pred.detach().clone(), losses, flat))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1], (res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2])


def test_graphed_segments_are_bit_identical_to_eager(hip):
    """hipGraph replay of the generator tail and of VGG19 (graphs.py) vs the eager launches: five G+D steps with the
    reference's default flags give bit-identical losses and parameters (the first two steps are eager in both runs, the
    third captures, the rest replay; box_net-less use_gt=False steps alternate)."""
    from scene_generation_amd import graphs
    from scene_generation_amd.trainer import Trainer
    args = parser.parse_args(['--image_size', '64,64', '--batch_size', '4', '--output_dir', '/tmp/o'])
    batches = [batch_to(make_batch(N=4, min_objs=3, max_objs=6, size=64, seed=60 + i), DEV) for i in range(2)]
    res = []
    saved = graphs.ENABLED
    try:
        for enabled in (True, False):
            graphs.ENABLED = enabled
            torch.manual_seed(0)
            tr = _filled_trainer(args, make_vocab())
            tr.model.noise_override = det((1, 64), 181).to(DEV)
            random.seed(21)
            hist = []
            for it in range(5):
                out = tr.step(batches[it % 2], use_gt=(it % 2 == 0))
                losses = {}
                for L in (tr.generator_losses, tr.d_img_losses, tr.d_obj_losses, tr.d_mask_losses):
                    losses.update(dict(L.items()))
                hist.append((losses, out[0].detach().clone()))
            if enabled:
                tail = tr.model.layout_to_image._tail
                assert len(tail) == 3, 'the generator tail is cut into three graphed segments at residual-block boundaries'
                for seg in tail:
                    assert any(e not in (None, False) for e in seg.entries.values()), '%s was never captured' % seg.name
                assert any(e not in (None, False) for e in tr.criterionVGG.vgg._graphed.entries.values())
            flat = torch.cat([getattr(tr, n).fp.flat for n in ('optimizer', 'optimizer_d_mask', 'optimizer_d_obj',
                                                              'optimizer_d_img')]).clone()
            res.append((hist, flat, list(tr.optimizer.steps)))
            del tr
    finally:
        graphs.ENABLED = saved
    for (la, ia), (lb, ib) in zip(res[0][0], res[1][0]):
        assert la == lb, (la, lb)
        assert torch.equal(ia, ib)
    assert torch.equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]


@pytest.mark.parametrize('size,N,steps', [(64, 4, 5), (128, 32, 3)])
def test_object_front_on_a_side_stream_is_bit_identical(hip, size, N, steps):
    """streams group 'front' (default on): Model.forward issues embeddings, graph convolutions, box_net and mask_net on a side
    stream beside the image path (they share no tensor in the training branch, model.py:98-124) and autograd runs their
    backward there.  Five G+D steps with the reference's default flags, use_gt alternating (box_net untouched every other step),
    give bit-identical losses, images and parameters with the group on and off; the side stream was really used."""
    from scene_generation_amd import streams
    from scene_generation_amd.trainer import Trainer
    # (128, 32): the benchmark configuration itself -- full widths, batch 32, 128x128 -- where the launches are long enough to overlap
    args = parser.parse_args(['--image_size', '%d,%d' % (size, size), '--batch_size', str(N), '--output_dir', '/tmp/o'])
    batches = [batch_to(make_batch(N=N, min_objs=3, max_objs=6 if N == 4 else 8, size=size, seed=70 + i), DEV) for i in range(2)]
    res = []
    saved = set(streams.GROUPS)
    try:
        for on in (True, False):
            streams.GROUPS.clear()
            if on:
                streams.GROUPS.update(('front', 'adam', 'mstep', 'imgD', 'objD'))     # (+ the generator's Adam step on its own stream under the D
                #                                                        steps, the mask discriminator's work on the front's stream)
            torch.manual_seed(0)
            tr = _filled_trainer(args, make_vocab())
            tr.model.noise_override = det((1, 64), 182).to(DEV)
            random.seed(22)
            hist = []
            for it in range(steps):
                out = tr.step(batches[it % 2], use_gt=(it % 2 == 0))
                losses = {}
                for L in (tr.generator_losses, tr.d_img_losses, tr.d_obj_losses, tr.d_mask_losses):
                    losses.update(dict(L.items()))
                hist.append((losses, [t.detach().clone() for t in out[:3]]))
            torch.cuda.synchronize()
            flat = torch.cat([getattr(tr, n).fp.flat for n in ('optimizer', 'optimizer_d_mask', 'optimizer_d_obj',
                                                              'optimizer_d_img')]).clone()
            res.append((hist, flat, list(tr.optimizer.steps)))
            del tr
    finally:
        streams.GROUPS.clear()
        streams.GROUPS.update(saved)
    assert any(k[1] == 'front' for k in streams._POOL), 'the front never ran on its side stream'
    assert any(k[1] == 'adam' for k in streams._POOL), 'the generator Adam step never ran on its side stream'
    for (la, ta), (lb, tb) in zip(res[0][0], res[1][0]):
        assert la == lb, (la, lb)
        for x, y in zip(ta, tb):
            assert torch.equal(x, y)
    assert torch.equal(res[0][1], res[1][1])
    assert res[0][2] == res[1][2]


def test_legacy_align_corners_switch(hip, golden):
    """set_legacy_align_corners(True): the align_corners=True geometry of PyTorch 1.0 (what the reference's released
    checkpoints were trained with) against the reference goldens captured with that default; restored afterwards."""
    import scene_generation_amd
    from scene_generation_amd.layout import masks_to_layout
    from scene_generation_amd.bilinear import crop_bbox_batch
    g = golden('legacy_align_corners')
    d = lambda k: torch.from_numpy(g[k]).to(DEV)
    scene_generation_amd.set_legacy_align_corners(True)
    try:
        close(masks_to_layout(d('vecs'), d('boxes'), d('masks'), d('obj_to_img'), 16), g['out'], 1e-5, 'layout')
        with torch.no_grad():
            close(masks_to_layout(d('vecs'), d('boxes'), d('masks'), d('obj_to_img'), 16, test_mode=True), g['out_test'], 1e-5)
        v2 = d('v2').requires_grad_()
        out2 = masks_to_layout(v2, d('b2'), d('m2'), d('o2'), 20, 28)
        close(out2, g['out2'], 1e-5)
        (out2 * d('w2')).sum().backward()
        close(v2.grad, g['gv2'], 2e-5)
        f = d('feats').requires_grad_()
        crop = crop_bbox_batch(f, d('cb'), d('idx'), 8)
        close(crop, g['crop'], 1e-5)
        (crop * d('wc')).sum().backward()
        close(f.grad, g['gf'], 2e-5)
    finally:
        scene_generation_amd.set_legacy_align_corners(False)
    out = masks_to_layout(d('vecs'), d('boxes'), d('masks'), d('obj_to_img'), 16)
    assert float((out.cpu() - torch.from_numpy(g['out'])).abs().max()) > 1e-3      # the default geometry is back


@pytest.mark.parametrize('pooling', ['sum', 'avg'])
def test_masks_to_layout_gradients_wrt_masks_and_boxes(hip, pooling):
    """layout.py:85-86 is differentiable in vecs, masks AND boxes: all three gradients vs the oracle's autograd (float masks,
    boxes partly outside the image, a box that up-samples its mask strongly)."""
    from scene_generation_amd.layout import masks_to_layout
    g = torch.Generator().manual_seed(17)
    counts = [3, 1, 4]
    Oc = sum(counts)
    o2i = torch.cat([torch.full((c,), i, dtype=torch.long) for i, c in enumerate(counts)])
    vecs = det((Oc, 9), 401)
    x0, y0 = torch.rand(Oc, generator=g) * 0.5, torch.rand(Oc, generator=g) * 0.5
    boxes = torch.stack([x0, y0, x0 + 0.12 + 0.4 * torch.rand(Oc, generator=g), y0 + 0.12 + 0.4 * torch.rand(Oc, generator=g)], 1)
    boxes[1] = torch.tensor([-0.15, 0.3, 0.45, 1.2])
    boxes[2] = torch.tensor([0.05, 0.05, 0.95, 0.9])
    masks = torch.rand(Oc, 16, 16, generator=g)
    H, W = 24, 28
    vr, br, mr = [t.clone().requires_grad_() for t in (vecs, boxes, masks)]
    ref = O.masks_to_layout(vr, br, mr, o2i, H, W, pooling=pooling)
    wgt = det(tuple(ref.shape), 402)
    (ref * wgt).sum().backward()
    vg, bg, mg = [t.to(DEV).requires_grad_() for t in (vecs, boxes, masks)]
    out = masks_to_layout(vg, bg, mg, o2i.to(DEV), H, W, pooling=pooling)
    (out * wgt.to(DEV)).sum().backward()
    close(out, ref, 1e-5, 'layout')
    close(vg.grad, vr.grad, 2e-5, 'd/dvecs')
    close(mg.grad, mr.grad, 2e-5, 'd/dmasks')
    close(bg.grad, br.grad, 1e-4, 'd/dboxes')


# ------------------------------------------------------------------------------------------
# f3 / f4: the collate -> device adapter on the GPU, the validation loop and the feature bank
# ------------------------------------------------------------------------------------------
def test_device_batch_prefetcher_equals_direct_copies_and_steps_identically(hip):
    """f3 (coco.py:501-547 -> train.py:190-193): the adapter (batch packed into a re-used page-locked slot on a staging thread, one
    sg_stage_copy kernel on the consumer's stream, eight views of one allocation) delivers exactly ``batch_to`` of the collated
    batch plus host lists that match it -- also when the slots rotate (7 batches through depth + 2 = 4 slots, threaded and
    inline) --, and a training step fed through it (host lists handed to the model, as bench.py does) is bit-identical to a
    step fed the device batch directly.  Pageable memory is refused by the copy kernel's entry point."""
    from scene_generation_amd import ops
    from scene_generation_amd.pipeline import DeviceBatchPrefetcher
    from scene_generation_amd.trainer import Trainer
    host = [make_batch(N=4, min_objs=2, max_objs=5, size=64, seed=70 + i) for i in range(7)]
    staged = list(DeviceBatchPrefetcher(host, DEV))
    assert len(staged) == 7
    for hb, db in zip(host, DeviceBatchPrefetcher(host, DEV, threaded=False, depth=1)):
        for a, b in zip(batch_to(hb, DEV), db.batch):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    with pytest.raises(RuntimeError):
        ops.stage_copy(torch.empty(4096, dtype=torch.uint8, device=DEV), torch.zeros(4096, dtype=torch.uint8), 4096)
    for hb, db in zip(host, staged):
        for a, b in zip(batch_to(hb, DEV), db.batch):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert db.objs_host == hb.objs.tolist() and db.obj_to_img_host == hb.obj_to_img.tolist()
        assert db.num_images == hb.imgs.size(0) and db.seg_offsets_host[-1] == hb.objs.numel()
    args = parser.parse_args(['--image_size', '64,64', '--batch_size', '4', '--vgg_features_weight', '0', '--output_dir', '/tmp/o'])
    res = []
    for through in (True, False):
        torch.manual_seed(0)
        tr = _filled_trainer(args, make_vocab())
        tr.model.noise_override = det((1, 64), 182).to(DEV)
        random.seed(9)
        for i in range(2):
            if through:
                db = staged[i]
                tr.model.objs_host, tr.model.obj_to_img_host = db.objs_host, db.obj_to_img_host
                out = tr.step(db.batch, use_gt=(i == 0))
            else:
                tr.model.objs_host = tr.model.obj_to_img_host = None
                out = tr.step(batch_to(host[i], DEV), use_gt=(i == 0))
        losses = {}
        for L in (tr.generator_losses, tr.d_img_losses, tr.d_obj_losses, tr.d_mask_losses):
            losses.update(dict(L.items()))
        res.append((losses, out[0].detach().clone(), tr.optimizer.fp.flat.clone(), tr.optimizer_d_img.fp.flat.clone()))
        del tr
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1:], res[1][1:]):
        assert torch.equal(a, b)


def test_eval_hooks_feature_bank_and_check_model(hip, golden):
    """f4: encode_features (scripts/encode_features.py:103-146) through the HIP crop / encoder / MLP against the reference's
    rows; check_model (train.py:80-116) against the oracle's test-mode forward + the reference-pinned IoU."""
    from scene_generation_amd.evaluate import jaccard, check_model, encode_features
    from scene_generation_amd.model import Model
    g = golden('eval_hooks')
    tot, n5, n3 = jaccard(torch.from_numpy(g['boxes_a']).to(DEV), torch.from_numpy(g['boxes_b']).to(DEV))
    assert abs(float(tot) - float(g['iou_sum'])) <= 1e-5 and n5 == int(g['n_gt_05']) and n3 == int(g['n_gt_03'])
    kw = dict(image_size=(32, 32), gconv_hidden_dim=32, gconv_num_layers=2, mask_size=8, n_downsample_global=1,
              appearance_normalization='batch', activation='leakyrelu-0.2', use_attributes=True, pool_size=2, rep_size=8)
    vocab = make_vocab(12, 4, 35)
    m = Model(vocab, **kw).to(DEV)
    fill_deterministic(m)
    m.eval()
    b = make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=12, num_preds=4, seed=33)
    bank = encode_features(m, [b], object_size=64)
    assert sorted(bank) == list(range(12)) and sum(v.shape[0] for v in bank.values()) == b.objs.numel()
    assert all(v.dtype == np.float64 for v in bank.values()), 'the reference bank is float64 throughout (encode_features.py:121,133)'
    ref_rows = g['feat']
    seen = {k: 0 for k in bank}
    for row, label in zip(ref_rows, b.objs.tolist()):
        got = bank[label][seen[label]]
        seen[label] += 1
        assert np.abs(got - row).max() <= 3e-5 * max(1.0, np.abs(row).max()), (label, got, row)
    # check_model: same numbers as the oracle model run by hand (test-mode compositing, predicted vs ground-truth boxes)
    ref = O.Model(vocab, **kw)
    fill_deterministic(ref)
    ref.eval()
    noise = det((1, 64), 183)
    m.noise_override, ref.noise_override = noise.to(DEV), noise
    cfg = type('A', (), {'num_val_samples': 3})()
    for use_gt in (True, False):
        random.seed(4)
        got = check_model(cfg, [b], m, None, use_gt)
        random.seed(4)
        with torch.no_grad():
            if use_gt:
                out = ref(b.imgs, b.objs, b.triples, b.obj_to_img, boxes_gt=b.boxes, masks_gt=b.masks, attributes=b.attributes,
                          test_mode=True, use_gt_box=True)
            else:
                out = ref(b.imgs, b.objs, b.triples, b.obj_to_img, boxes_gt=b.boxes, masks_gt=None,
                          attributes=torch.zeros_like(b.attributes), test_mode=True, use_gt_box=False)
        want = float(jaccard(out[1], b.boxes)[0]) / b.boxes.size(0)
        assert got[1:] == (None, None, None) and abs(got[0] - want) <= 1e-4 * max(1.0, abs(want)), (use_gt, got, want)
