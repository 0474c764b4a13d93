"""The diversity score's own operators (csrc/lpips.hip): the wide forward convolution (kernels up to 11 x 11, stride up to 4: AlexNet's
stem), the scaling layer of LPIPS and one tap of its distance.  Forward only (inference); no wrapper synchronises.  (Part of
scene_generation_amd.ops: see ops/__init__.py.)"""
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
