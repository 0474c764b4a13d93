"""The diversity score's own operators (csrc/lpips.hip): the wide forward convolution (kernels up to 11 x 11, stride up to 4: AlexNet's
stem), the scaling layer of LPIPS and one tap of its distance -- and, for LPIPS as a training loss, the tap's gradient with respect to
the prediction's features, the scaling layer's backward and the autograd functions around them.  The convolution is forward only; no
wrapper synchronises.  (Part of scene_generation_amd.ops: see ops/__init__.py.)"""
import torch

from ._core import ACT_NONE, _L, _call, _dev, _f32, _p, _stream, workspace
from .fid import _pd
from .inception import _rect_fwd, _rect_plan

LPIPS_EPS = 1e-10


def conv2d_wide_plan(d, w_aligned16=True):
    """-> dict(tile, bm, bn, vec, splits, kchunk): the launch sg_conv2d_wide_fwd issues for desc ``d`` (``rect_desc``; a host-only
    query).  Raises for a desc the entry point rejects (more than 11 taps a side, stride above 4, pad >= kernel, wrong OH / OW)."""
    return _rect_plan('conv2d_wide', d, w_aligned16)


def conv2d_wide(x, w, bias=None, stride=1, pad=(0, 0), act=ACT_NONE, out=None, out_c0=0):
    """``conv2d_rect`` for kernels up to 11 x 11 and strides 1..4: act(conv2d(x, w [Cout, C, KH, KW], bias, stride, padding=pad))
    written to channels [out_c0, out_c0 + Cout) of ``out`` [N, Ctot, OH, OW] (a fresh [N, Cout, OH, OW] when None).  -> out"""
    return _rect_fwd('conv2d_wide', x, w, bias, stride, pad, act, out, out_c0, clamp=True)


def lpips_input(x, channels_last=False):
    """the scaling layer of LPIPS: ``(v - shift[c]) / scale[c]`` of pictures [N, 3, H, W] -- or, ``channels_last``, [N, H, W, 3] --
    float32 in [-1, 1] (v = x) or uint8 (v = x / 127.5 - 1) -> float32 [N, 3, H, W], every operation rounded on its own"""
    _dev(x, 'pictures')
    if x.dtype not in (torch.float32, torch.uint8):
        raise TypeError('lpips_input: pictures must be float32 or uint8, got %s' % x.dtype)
    if x.dim() != 4 or x.size(3 if channels_last else 1) != 3:
        raise ValueError('lpips_input: pictures %s, got %s' % ('[N, H, W, 3]' if channels_last else '[N, 3, H, W]', tuple(x.shape)))
    x = x if x.is_contiguous() else x.contiguous()
    N, H, W = (x.size(0), x.size(1), x.size(2)) if channels_last else (x.size(0), x.size(2), x.size(3))
    y = torch.empty(N, 3, H, W, dtype=torch.float32, device=x.device)
    _call('sg_lpips_input', _p(x), 1 if x.dtype == torch.uint8 else 0, 1 if channels_last else 0, N, H * W, _p(y), _stream())
    return y


def lpips_layer(f0, f1, w=None, out=None, accumulate=False, eps=LPIPS_EPS):
    """one tap of the LPIPS distance between feature maps ``f0`` and ``f1`` [P, C, ...] (float32; the two halves of one 2P forward):
    per pixel ``sum_c w[c] (f0_c / (|f0| + eps) - f1_c / (|f1| + eps))^2``, averaged over the pixels in float64.  ``w`` [C] float32
    (None: all ones).  -> ``out`` float64 [P] on the device, overwritten or, with ``accumulate``, added to (five calls build a pair's
    distance); a fresh tensor when None.  No host read."""
    _dev(f0, 'features')
    _dev(f1, 'features')
    if f0.dtype != torch.float32 or f1.dtype != torch.float32:
        raise TypeError('lpips_layer: features must be float32, got %s and %s' % (f0.dtype, f1.dtype))
    if f0.dim() < 2 or f0.shape != f1.shape or f0.device != f1.device:
        raise ValueError('lpips_layer: two feature maps [P, C, ...] of one shape and device, got %s and %s'
                         % (tuple(f0.shape), tuple(f1.shape)))
    f0 = f0 if f0.is_contiguous() else f0.contiguous()
    f1 = f1 if f1.is_contiguous() else f1.contiguous()
    P, C = f0.size(0), f0.size(1)
    HW = 1
    for n in f0.shape[2:]:
        HW *= int(n)
    if w is not None:
        w = _f32(w, 'lin weights').reshape(-1)
        if w.numel() != C:
            raise ValueError('lpips_layer: %d lin weights for %d channels' % (w.numel(), C))
    if out is None:
        if accumulate:
            raise ValueError('lpips_layer: accumulate needs the tensor to add to')
        out = torch.empty(P, dtype=torch.float64, device=f0.device)
    elif out.dtype != torch.float64 or not out.is_cuda or out.dim() != 1 or out.numel() != P or not out.is_contiguous():
        raise ValueError('lpips_layer: out must be a contiguous float64 device tensor [%d], got %s %s' % (P, out.dtype, tuple(out.shape)))
    nbytes = int(_L().sg_lpips_layer_ws_bytes(P, C, HW))
    ws = workspace(nbytes, f0.device) if nbytes else None
    _call('sg_lpips_layer', _p(f0), _p(f1), _p(w), P, C, HW, float(eps), _pd(out), 1 if accumulate else 0, _p(ws), nbytes, _stream())
    return out


def lpips_layer_bwd(f0, f1, w, gout, eps=LPIPS_EPS):
    """the gradient of ``lpips_layer(f0, f1, w)`` with respect to ``f0``: ``gout`` float64 [P] on the device (dL / d out, never read
    by the host) -> ``gf0`` float32 of f0's shape, every element written once.  ``f1`` is the target and gets no gradient.  A pixel
    of ``f0`` whose channels are all zero gets the finite ``g / (0 + eps)`` where autograd of the formula gives NaN (see
    sg_lpips_layer_bwd in the header: the ReLU in front of a tap drops that value)."""
    _dev(f0, 'features')
    _dev(f1, 'features')
    _dev(gout, 'distance gradient')
    if f0.dtype != torch.float32 or f1.dtype != torch.float32:
        raise TypeError('lpips_layer_bwd: features must be float32, got %s and %s' % (f0.dtype, f1.dtype))
    if f0.dim() < 2 or f0.shape != f1.shape or f0.device != f1.device:
        raise ValueError('lpips_layer_bwd: two feature maps [P, C, ...] of one shape and device, got %s and %s'
                         % (tuple(f0.shape), tuple(f1.shape)))
    f0 = f0 if f0.is_contiguous() else f0.contiguous()
    f1 = f1 if f1.is_contiguous() else f1.contiguous()
    P, C = f0.size(0), f0.size(1)
    HW = 1
    for n in f0.shape[2:]:
        HW *= int(n)
    if w is not None:
        w = _f32(w, 'lin weights').reshape(-1)
        if w.numel() != C:
            raise ValueError('lpips_layer_bwd: %d lin weights for %d channels' % (w.numel(), C))
    if gout.dtype != torch.float64 or gout.dim() != 1 or gout.numel() != P or gout.device != f0.device:
        raise ValueError('lpips_layer_bwd: gout must be a float64 tensor [%d] on the features\' device, got %s %s'
                         % (P, gout.dtype, tuple(gout.shape)))
    gout = gout if gout.is_contiguous() else gout.contiguous()
    gf0 = torch.empty_like(f0)
    _call('sg_lpips_layer_bwd', _p(f0), _p(f1), _p(w), _pd(gout), P, C, HW, float(eps), _p(gf0), _stream())
    return gf0


def lpips_input_bwd(gy):
    """the backward of ``lpips_input`` on float32 [N, 3, H, W] pictures: ``gy / scale[c]`` -> float32 [N, 3, H, W]"""
    gy = _f32(gy, 'lpips_input_bwd: the gradient')
    if gy.dim() != 4 or gy.size(1) != 3:
        raise ValueError('lpips_input_bwd: gradient [N, 3, H, W], got %s' % (tuple(gy.shape),))
    gx = torch.empty_like(gy)
    _call('sg_lpips_input_bwd', _p(gy), gy.size(0), gy.size(2) * gy.size(3), _p(gx), _stream())
    return gx


class LpipsInputFn(torch.autograd.Function):
    """``lpips_input`` of float32 [N, 3, H, W] pictures in [-1, 1] with its backward"""

    @staticmethod
    def forward(ctx, x):
        return lpips_input(x)

    @staticmethod
    def backward(ctx, gy):
        return lpips_input_bwd(gy)


class LpipsDistanceFn(torch.autograd.Function):
    """``apply(eps, *taps_x, *taps_y, *lins)``: the five taps of the prediction, the five of the target, the five lin weight vectors
    (None: ones) -> the float64 [P] distances, by the five ``lpips_layer`` launches of ``LPIPS.forward`` (the same bits).  The
    backward is one ``lpips_layer_bwd`` launch per tap on the incoming float64 [P] gradient; targets and weights get None."""

    @staticmethod
    def forward(ctx, eps, *tensors):
        n = len(tensors) // 3
        assert len(tensors) == 3 * n and n > 0
        fx, fy, lins = tensors[:n], tensors[n:2 * n], tensors[2 * n:]
        out = torch.empty(fx[0].size(0), dtype=torch.float64, device=fx[0].device)
        for k in range(n):
            lpips_layer(fx[k], fy[k], lins[k], out=out, accumulate=k > 0, eps=eps)
        ctx.eps, ctx.n = eps, n
        ctx.lins = lins                                  # frozen buffers, or None: not tensors autograd tracks
        ctx.save_for_backward(*fx, *fy)
        return out

    @staticmethod
    def backward(ctx, gout):
        n, saved = ctx.n, ctx.saved_tensors
        gout = gout.contiguous()
        grads = [lpips_layer_bwd(saved[k], saved[n + k], ctx.lins[k], gout, ctx.eps) if ctx.needs_input_grad[1 + k] else None
                 for k in range(n)]
        return (None,) + tuple(grads) + (None,) * (2 * n)
