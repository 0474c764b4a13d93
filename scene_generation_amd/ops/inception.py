"""The Inception score's own operators (csrc/inception.hip): the rectangular forward convolution that writes a channel slice, the
unpadded 3x3 stride-2 max-pool, the count_include_pad 3x3 average pool, the bilinear resize, softmax rows into a growing buffer and
the score itself.  Forward only (inference); no wrapper synchronises.  (Part of scene_generation_amd.ops: see ops/__init__.py.)"""
import ctypes

import torch

from .._hip import CONST, last_error, plan_dict, sgRectDesc, sgRectPlan      # noqa: F401  (the structs are re-exported)
from ._core import ACT_NONE, ACT_RELU, _L, _call, _f32, _p, _stream, workspace

RECT_TILE_64X64, RECT_TILE_32X128, RECT_TILE_64X128 = (CONST['SG_RECT_TILE_' + n] for n in ('64X64', '32X128', '64X128'))
RECT_TILES = {RECT_TILE_64X64: '64x64', RECT_TILE_32X128: '32x128', RECT_TILE_64X128: '64x128'}

_rect_cache = {}


def conv_out_size(size, k, stride, pad):
    return (size + 2 * pad - k) // stride + 1


def rect_desc(N, C, H, W, Cout, KH, KW, stride=1, padH=0, padW=0, out_c0=0, out_ctot=None):
    """sgRectDesc for these sizes (one instance per shape: the ctypes reference and the workspace sizes are kept on it)"""
    OH, OW = conv_out_size(H, KH, stride, padH), conv_out_size(W, KW, stride, padW)
    key = (N, C, H, W, Cout, KH, KW, stride, padH, padW, OH, OW, out_c0, Cout if out_ctot is None else out_ctot)
    d = _rect_cache.get(key)
    if d is None:
        d = sgRectDesc(*key)
        d._ref = ctypes.byref(d)
        d._ws = {}                      # stem of the entry point -> its workspace bytes
        _rect_cache[key] = d
    return d


def _rect_plan(name, d, w_aligned16):
    """the body of conv2d_rect_plan / conv2d_wide_plan (``name``: the stem of the entry point sg_<name>_plan)"""
    plan = sgRectPlan()
    if getattr(_L(), 'sg_%s_plan' % name)(d._ref, 1 if w_aligned16 else 0, ctypes.byref(plan)) != 0:
        raise RuntimeError('sg_%s_plan failed: %s' % (name, last_error()))
    return plan_dict(plan)


def _rect_fwd(name, x, w, bias, stride, pad, act, out, out_c0, clamp=False):
    """the body of conv2d_rect / conv2d_wide (``name``: the stem of the entry points sg_<name>_ws_bytes / _fwd).  ``clamp``: the
    fresh result of a kernel larger than the padded plane is allocated empty, for the entry point to refuse it."""
    x, w = _f32(x, 'conv input'), _f32(w, 'conv weight')
    if x.dim() != 4 or w.dim() != 4 or w.size(1) != x.size(1):
        raise ValueError('%s: x [N, C, H, W] and w [Cout, C, KH, KW], got %s and %s' % (name, tuple(x.shape), tuple(w.shape)))
    if act not in (ACT_NONE, ACT_RELU):
        raise ValueError('%s: act must be ACT_NONE or ACT_RELU' % name)
    N, C, H, W = x.shape
    Cout, _, KH, KW = w.shape
    OH, OW = conv_out_size(H, KH, stride, pad[0]), conv_out_size(W, KW, stride, pad[1])
    if out is None:
        out = torch.empty(N, Cout, max(OH, 0) if clamp else OH, max(OW, 0) if clamp else OW, dtype=torch.float32, device=x.device)
    elif (out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.dim() != 4 or out.size(0) != N
          or tuple(out.shape[2:]) != (OH, OW) or out_c0 < 0 or out_c0 + Cout > out.size(1)):
        raise ValueError('%s: out must be a contiguous float32 device tensor [%d, >= %d, %d, %d], got %s'
                         % (name, N, out_c0 + Cout, OH, OW, tuple(out.shape)))
    if bias is not None:
        bias = _f32(bias, 'conv bias')
        if bias.numel() != Cout:
            raise ValueError('%s: bias of %d elements for %d output channels' % (name, bias.numel(), Cout))
    d = rect_desc(N, C, H, W, Cout, KH, KW, stride, pad[0], pad[1], out_c0, out.size(1))
    ws_bytes = d._ws.get(name)
    if ws_bytes is None:
        ws_bytes = d._ws[name] = int(getattr(_L(), 'sg_%s_ws_bytes' % name)(d._ref))
    ws = workspace(ws_bytes, x.device) if ws_bytes else None
    _call('sg_%s_fwd' % name, d._ref, _p(x), _p(w), _p(bias), _p(out), act, _p(ws), ws_bytes, _stream())
    return out


def conv2d_rect_plan(d, w_aligned16=True):
    """-> dict(tile, bm, bn, vec, splits, kchunk): the launch sg_conv2d_rect_fwd issues for desc ``d`` (a host-only query)"""
    return _rect_plan('conv2d_rect', d, w_aligned16)


def conv2d_rect(x, w, bias=None, stride=1, pad=(0, 0), act=ACT_NONE, out=None, out_c0=0):
    """act(conv2d(x, w [Cout, C, KH, KW], bias, stride, padding=pad)) written to channels [out_c0, out_c0 + Cout) of ``out``
    [N, Ctot, OH, OW] (a fresh [N, Cout, OH, OW] when None); the other channels of ``out`` are left alone.  -> out"""
    return _rect_fwd('conv2d_rect', x, w, bias, stride, pad, act, out, out_c0)


def maxpool3s2v(x, out=None, out_c0=0):
    """max_pool2d(x, 3, stride=2) (no padding) into channels [out_c0, out_c0 + C) of ``out`` [N, Ctot, OH, OW] -> out"""
    x = _f32(x, 'max-pool input')
    N, C, H, W = x.shape
    if H < 3 or W < 3:
        raise ValueError('maxpool3s2v: the plane %dx%d is smaller than the window' % (H, W))
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    if out is None:
        out = torch.empty(N, C, OH, OW, dtype=torch.float32, device=x.device)
    elif (out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.dim() != 4 or out.size(0) != N
          or tuple(out.shape[2:]) != (OH, OW) or out_c0 < 0 or out_c0 + C > out.size(1)):
        raise ValueError('maxpool3s2v: out must be a contiguous float32 device tensor [%d, >= %d, %d, %d], got %s'
                         % (N, out_c0 + C, OH, OW, tuple(out.shape)))
    _call('sg_maxpool3s2v_fwd', _p(x), _p(out), N, C, H, W, OH, OW, out_c0, out.size(1), _stream())
    return out


def avgpool3s1(x):
    """avg_pool2d(x, 3, stride=1, padding=1) with count_include_pad=True (the divisor is 9 everywhere)"""
    x = _f32(x, 'avg-pool input')
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    _call('sg_avgpool3s1_fwd', _p(x), _p(y), N * C, H, W, _stream())
    return y


def resize_bilinear(x, size):
    """F.interpolate(x, size=size, mode='bilinear', align_corners=False)"""
    x = _f32(x, 'resize input')
    N, C, H, W = x.shape
    OH, OW = (size, size) if isinstance(size, int) else size
    y = torch.empty(N, C, OH, OW, dtype=torch.float32, device=x.device)
    _call('sg_resize_bilinear_fwd', _p(x), _p(y), N * C, H, W, OH, OW, _stream())
    return y


def softmax_rows(logits, out, row0):
    """softmax(logits [rows, classes], dim=1) -> rows [row0, row0 + rows) of ``out`` [capacity, classes] (the rest untouched)"""
    logits = _f32(logits, 'logits')
    if (logits.dim() != 2 or out.dim() != 2 or out.size(1) != logits.size(1) or out.dtype != torch.float32 or not out.is_cuda
            or not out.is_contiguous()):
        raise ValueError('softmax_rows: logits [rows, classes] and a contiguous float32 device out [capacity, classes], got %s and %s'
                         % (tuple(logits.shape), tuple(out.shape)))
    _call('sg_softmax_rows', _p(logits), logits.size(0), logits.size(1), _p(out), int(row0), out.size(0), _stream())
    return out


def inception_score(probs, n, splits):
    """-> float64 device tensor [2 + splits] = {mean, std, per-split scores} over the first ``n`` rows of probs [>= n, classes]
    (scripts/inception_score.py:48-62); no host read"""
    probs = _f32(probs, 'probabilities')
    if probs.dim() != 2 or n < 0 or n > probs.size(0) or splits < 1:
        raise ValueError('inception_score: probs [rows >= n, classes] and splits >= 1, got %s, n = %d, splits = %d'
                         % (tuple(probs.shape), n, splits))
    classes = probs.size(1)
    out = torch.empty(2 + splits, dtype=torch.float64, device=probs.device)
    nbytes = int(_L().sg_inception_score_ws_bytes(int(n), classes, int(splits)))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=probs.device)
    _call('sg_inception_score', _p(probs), int(n), classes, int(splits), _p(out), _p(ws), ws.numel() * 8, _stream())
    return out
