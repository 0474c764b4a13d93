"""The per-image weight gradient of the factored 7x7 stem over reflect-padded planes (option ``wgrad_padded``,
csrc/igemm_nk.hip) and the reflection fold with its interior fast path (``sg_pad_upsample_bwd``, csrc/norm.hip).

Both go through the C ABI.  The references are float64 on the CPU, built from ``F.pad(mode='reflect')`` and autograd; none of
them runs the code under test.

Weight gradient: the padded-plane route changes where the gathered element comes from, not which products meet in which order,
so it must equal the gather route (option off) bit for bit; against float64 every element is held to the derived bound of
tests/wgrad_cases.py, with the chunk count of the plan the library reports.  A workspace of the size the query returned before the padded planes were added must select the gather
route -- no fault, no error.

Fold: interior elements have one source; the others add up to nine values in a fixed order (row candidates outer, column
candidates inner).  The result must equal an fp32 fold evaluated in that order bit for bit, and lie within nine additions'
rounding of float64: 9 * 2^-24 * sum|g_k| over the source terms of the output."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_harness import L  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 12345.0
U = 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _call(L, name, *args):
    rc = getattr(L, name)(*args)
    assert rc == 0, '%s returned %d: %s' % (name, rc, L.sg_last_error_string().decode())


# ---- sg_conv2d_wgrad_perimage ---------------------------------------------------------------------------------------
#         N  L  Cout  H   W  KS pad
WGRAD = [(2, 3, 8, 9, 9, 7, 3),
         (3, 9, 64, 16, 12, 7, 3),
         (2, 5, 40, 10, 13, 7, 3),       # padded width 19 (no multiple of 4), M no multiple of the tile
         (1, 1, 64, 32, 32, 7, 3)]       # k-chunks inside the image (S > 1)
_wgrad_cache = {}


def _wgrad_case(case):
    """inputs of a case and its float64 reference (computed once, shared by the tests, never modified)"""
    if case in _wgrad_cache:
        return _wgrad_cache[case]
    N, Lc, M, H, W, KS, pad = case
    g = torch.Generator().manual_seed(1000 + 7 * N + Lc + M + H + W)
    J = Lc + 2                                             # channels of the stored planes: more than any image lists
    x = torch.randn(N, J, H, W, generator=g)
    gy = torch.randn(N, M, H, W, generator=g)
    cnt = [max(1, Lc - (b % 2)) for b in range(N)]         # every other image lists one channel less
    lst = np.zeros((N, Lc), dtype=np.int32)
    for b in range(N):
        ch = sorted(torch.randperm(J, generator=g)[:cnt[b]].tolist())
        lst[b, :cnt[b]] = ch
        lst[b, cnt[b]:] = ch[0]
    ref = torch.zeros(N, M, Lc, KS, KS, dtype=torch.float64)
    for b in range(N):
        xp = F.pad(x[b:b + 1, lst[b, :cnt[b]].tolist()].double(), (pad,) * 4, mode='reflect')
        w = torch.zeros(M, cnt[b], KS, KS, dtype=torch.float64, requires_grad=True)
        F.conv2d(xp, w).backward(gy[b:b + 1].double())
        ref[b, :, :cnt[b]] = w.grad
    out = _wgrad_cache[case] = (x, gy, torch.from_numpy(lst), torch.tensor(cnt, dtype=torch.int32), ref)
    return out


def _old_ws_bytes(L, N, M, C, Lc, KS):
    """what sg_conv2d_sparse_ws_bytes(d, L, 2) returned before the padded planes: slabs padded to 128 channels + the inverse lists"""
    a = N * M * ((Lc + 127) // 128 * 128) * KS * KS * 4 + N * C * 4
    return max(a, L.sg_channel_sum_ws_bytes(M))


def _run_wgrad(L, case, padded, ws_bytes=None):
    from scene_generation_amd import _hip
    from scene_generation_amd.ops._core import _conv_desc
    N, Lc, M, H, W, KS, pad = case
    x, gy, lst, cnt, _ = _wgrad_case(case)
    d = _conv_desc(N, x.size(1), 0, H, W, M, KS, 1, pad, 1, 1, H, W, 0, 0)
    full = L.sg_conv2d_sparse_ws_bytes(d._ref, Lc, 2)
    wsb = full if ws_bytes is None else ws_bytes
    xd, gyd, ld, cd = x.to(DEV), gy.to(DEV), lst.to(DEV), cnt.to(DEV)
    n = N * M * Lc * KS * KS
    out = torch.full((n + 1,), GUARD, dtype=torch.float32, device=DEV)
    ws = torch.full((full // 4 + 2,), GUARD, dtype=torch.float32, device=DEV)       # (a guard behind the bytes that were offered)
    saved = _hip.get_option('wgrad_padded')
    _hip.set_option('wgrad_padded', 1 if padded else 0)
    try:
        _call(L, 'sg_conv2d_wgrad_perimage', d._ref, _ptr(gyd), _ptr(xd), None, _ptr(ld), _ptr(cd), Lc, _ptr(out), _ptr(ws), wsb,
              _stream())
        torch.cuda.synchronize()
    finally:
        _hip.set_option('wgrad_padded', saved)
    h = out.cpu()
    assert float(h[-1]) == GUARD, 'the kernel wrote behind its output'
    wh = ws.cpu()
    assert bool((wh[(wsb + 3) // 4:] == GUARD).all()), 'the kernel wrote behind the workspace bytes it was given'
    return h[:-1].reshape(N, M, Lc, KS, KS).clone()


@pytest.mark.parametrize('case', WGRAD, ids=lambda c: 'N%d_L%d_M%d_%dx%d_k%dp%d' % c)
def test_stem_wgrad_padded_planes(L, case):
    ref = _wgrad_case(case)[4]
    on, off = _run_wgrad(L, case, True), _run_wgrad(L, case, False)
    err_on = float((on.double() - ref).abs().max())
    err_off = float((off.double() - ref).abs().max())
    print('wgrad_perimage %s: max|padded - f64| = %.4e, max|gather - f64| = %.4e, max|ref| = %.3e'
          % (case, err_on, err_off, float(ref.abs().max())))
    assert torch.equal(on, off), 'the padded-plane route differs from the gather route'
    assert on.view(torch.int32).equal(off.view(torch.int32)), 'the two routes differ in a sign of zero'
    # every element within its own rounding bound of float64 (tests/wgrad_cases.py): gamma(n + S) sum|gy||x|, n the terms of the
    # element, S the k-chunks of an image that the plan reports for this launch
    import wgrad_cases as WG
    N, Lc, M, H, W, KS, pad = case
    x, gy, lst, cnt = _wgrad_case(case)[:4]
    d = WG.make_desc(N, x.size(1), H, W, M, KS, 1, pad, True, 1, H, W)
    plan = WG.wgrad_plan(L, d, WG.WG_PERIMAGE, Lc, 0, L.sg_conv2d_sparse_ws_bytes(ctypes.byref(d), Lc, 2))
    assert plan['form'] == WG.WG_PADDED and plan['grid_z'] % N == 0, plan
    per = lambda g, v: WG.perimage_wgrad(WG.wgrad_images(g, v, KS, 1, pad, True, 1), lst.numpy(), cnt.numpy())
    g64, x64 = gy.double().numpy(), x.double().numpy()
    bound = WG.bound(per(np.ones_like(g64), np.ones_like(x64)), plan['grid_z'] // N, per(np.abs(g64), np.abs(x64)))
    err = (on.double() - ref).abs().numpy()
    print('wgrad_perimage %s: worst error / bound %.3f' % (case, float((err / np.maximum(bound, 1e-300)).max())))
    assert bool((err <= bound).all()), float((err / np.maximum(bound, 1e-300)).max())
    for b in range(case[0]):
        assert not bool(on[b, :, int(cnt[b]):].any()), 'columns beyond the image\'s channel list must be zero'


@pytest.mark.parametrize('case', WGRAD, ids=lambda c: 'N%d_L%d_M%d_%dx%d_k%dp%d' % c)
def test_stem_wgrad_workspace_query_grew_and_old_size_falls_back(L, case):
    from scene_generation_amd.ops._core import _conv_desc
    N, Lc, M, H, W, KS, pad = case
    x = _wgrad_case(case)[0]
    d = _conv_desc(N, x.size(1), 0, H, W, M, KS, 1, pad, 1, 1, H, W, 0, 0)
    old = _old_ws_bytes(L, N, M, x.size(1), Lc, KS)
    new = L.sg_conv2d_sparse_ws_bytes(d._ref, Lc, 2)
    assert new >= old + N * Lc * (H + 2 * pad) * (W + 2 * pad) * 4, (new, old)
    # the forward query and a zero-padded descriptor are what they were
    dz = _conv_desc(N, x.size(1), 0, H, W, M, KS, 1, pad, 0, 1, H, W, 0, 0)
    assert L.sg_conv2d_sparse_ws_bytes(dz._ref, Lc, 2) == old
    got = _run_wgrad(L, case, True, ws_bytes=old)          # asserts rc == 0 and that nothing behind ``old`` bytes was written
    assert torch.equal(got, _run_wgrad(L, case, False))


# ---- sg_pad_upsample_bwd --------------------------------------------------------------------------------------------
#        NC  H   W  pad ups
FOLD = [(3, 8, 8, 3, 1),         # corners with four sources
        (2, 5, 7, 3, 1),         # both reflection candidates live on one axis
        (4, 16, 18, 3, 1),       # 16-byte alignment of the rows varies
        (2, 6, 6, 1, 1),
        (2, 4, 5, 0, 2)]


def _sources(l, Ln, p):
    """padded-grid coordinates that reflect onto logical coordinate l, in the order the kernel adds them"""
    a = [l + p]
    if 1 <= l <= p:
        a.append(p - l)
    if Ln - 1 - p <= l <= Ln - 2:
        a.append(p + 2 * Ln - 2 - l)
    return a


def _fold_f32(g, H, W, pad, ups):
    NC = g.size(0)
    out = torch.zeros(NC, H, W, dtype=torch.float32)
    for h in range(H):
        for w in range(W):
            s = torch.zeros(NC, dtype=torch.float32)
            for dh in range(ups):
                for dw in range(ups):
                    for a in _sources(h * ups + dh, H * ups, pad):
                        for b in _sources(w * ups + dw, W * ups, pad):
                            s = s + g[:, a, b]
            out[:, h, w] = s
    return out


def _fold_f64(g, H, W, pad, ups):
    """adjoint of reflect_pad(pad) o nearest_upsample(ups) by autograd, in float64"""
    x = torch.zeros(g.size(0), 1, H, W, dtype=torch.float64, requires_grad=True)
    y = F.interpolate(x, scale_factor=ups, mode='nearest') if ups > 1 else x
    if pad:
        y = F.pad(y, (pad,) * 4, mode='reflect')
    y.backward(g.double().unsqueeze(1))
    return x.grad[:, 0]


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'offset1'])
@pytest.mark.parametrize('case', FOLD, ids=lambda c: 'NC%d_%dx%d_p%d_u%d' % c)
def test_reflection_fold(L, case, off):
    NC, H, W, pad, ups = case
    PH, PW = H * ups + 2 * pad, W * ups + 2 * pad
    gen = torch.Generator().manual_seed(77 + NC + 3 * H + 5 * W + pad + ups)
    g = torch.randn(NC, PH, PW, generator=gen)
    g[0, pad + min(H * ups - 1, pad + 1), :] = -0.0        # a row of negative zeros: 0 + (-0) = +0 in the kernel's sum
    gb = torch.empty(g.numel() + 8, dtype=torch.float32, device=DEV)
    gd = gb[off:off + g.numel()]
    gd.copy_(g.reshape(-1))
    n = NC * H * W
    ob = torch.full((n + off + 1,), GUARD, dtype=torch.float32, device=DEV)
    o = ob[off:]
    _call(L, 'sg_pad_upsample_bwd', _ptr(gd), _ptr(o), NC, H, W, pad, ups, _stream())
    torch.cuda.synchronize()
    h = o.cpu()
    assert float(h[-1]) == GUARD, 'the kernel wrote behind its output'
    assert bool((ob[:off].cpu() == GUARD).all())
    got = h[:-1].reshape(NC, H, W)
    exp32 = _fold_f32(g, H, W, pad, ups)
    assert got.view(torch.int32).equal(exp32.view(torch.int32)), \
        'differs from the fp32 fold in the same order: max %g' % float((got - exp32).abs().max())
    ref = _fold_f64(g, H, W, pad, ups)
    bound = 9 * U * _fold_f64(g.abs(), H, W, pad, ups)
    err = (got.double() - ref).abs()
    print('pad_upsample_bwd %s off %d: max err %.3e, max err / bound %.3f'
          % (case, off, float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
