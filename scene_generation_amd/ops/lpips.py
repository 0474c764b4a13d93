"""The diversity score's own operators (csrc/lpips.hip): the wide forward convolution (kernels up to 11 x 11, stride up to 4: AlexNet's
stem), the scaling layer of LPIPS and one tap of its distance.  Forward only (inference); no wrapper synchronises.  (Part of
scene_generation_amd.ops: see ops/__init__.py.)"""
import ctypes

import torch

from ._core import ACT_NONE, ACT_RELU, _L, _call, _dev, _f32, _p, _stream, workspace
from .fid import _pd
from .inception import conv_out_size, rect_desc, sgRectPlan

LPIPS_EPS = 1e-10


def conv2d_wide_plan(d, w_aligned16=True):
    """-> dict(tile, bm, bn, vec, splits, kchunk): the launch sg_conv2d_wide_fwd issues for desc ``d`` (``rect_desc``; a host-only
    query).  Raises for a desc the entry point rejects (more than 11 taps a side, stride above 4, pad >= kernel, wrong OH / OW)."""
    plan = sgRectPlan()
    rc = _L().sg_conv2d_wide_plan(d._ref, 1 if w_aligned16 else 0, ctypes.byref(plan))
    if rc != 0:
        from .. import _hip
        raise RuntimeError('sg_conv2d_wide_plan failed: %s' % _hip.last_error())
    return {n: int(getattr(plan, n)) for n, _ in sgRectPlan._fields_}


def conv2d_wide(x, w, bias=None, stride=1, pad=(0, 0), act=ACT_NONE, out=None, out_c0=0):
    """``conv2d_rect`` for kernels up to 11 x 11 and strides 1..4: act(conv2d(x, w [Cout, C, KH, KW], bias, stride, padding=pad))
    written to channels [out_c0, out_c0 + Cout) of ``out`` [N, Ctot, OH, OW] (a fresh [N, Cout, OH, OW] when None).  -> out"""
    x, w = _f32(x, 'conv input'), _f32(w, 'conv weight')
    if x.dim() != 4 or w.dim() != 4 or w.size(1) != x.size(1):
        raise ValueError('conv2d_wide: x [N, C, H, W] and w [Cout, C, KH, KW], got %s and %s' % (tuple(x.shape), tuple(w.shape)))
    if act not in (ACT_NONE, ACT_RELU):
        raise ValueError('conv2d_wide: act must be ACT_NONE or ACT_RELU')
    N, C, H, W = x.shape
    Cout, _, KH, KW = w.shape
    OH, OW = conv_out_size(H, KH, stride, pad[0]), conv_out_size(W, KW, stride, pad[1])
    if out is None:
        out = torch.empty(N, Cout, max(OH, 0), max(OW, 0), dtype=torch.float32, device=x.device)
    elif (out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.dim() != 4 or out.size(0) != N
          or tuple(out.shape[2:]) != (OH, OW) or out_c0 < 0 or out_c0 + Cout > out.size(1)):
        raise ValueError('conv2d_wide: out must be a contiguous float32 device tensor [%d, >= %d, %d, %d], got %s'
                         % (N, out_c0 + Cout, OH, OW, tuple(out.shape)))
    if bias is not None:
        bias = _f32(bias, 'conv bias')
        if bias.numel() != Cout:
            raise ValueError('conv2d_wide: bias of %d elements for %d output channels' % (bias.numel(), Cout))
    d = rect_desc(N, C, H, W, Cout, KH, KW, stride, pad[0], pad[1], out_c0, out.size(1))
    ws_bytes = getattr(d, '_wide_ws', None)
    if ws_bytes is None:
        ws_bytes = d._wide_ws = int(_L().sg_conv2d_wide_ws_bytes(d._ref))
    ws = workspace(ws_bytes, x.device) if ws_bytes else None
    _call('sg_conv2d_wide_fwd', d._ref, _p(x), _p(w), _p(bias), _p(out), act, _p(ws), ws_bytes, _stream())
    return out


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
