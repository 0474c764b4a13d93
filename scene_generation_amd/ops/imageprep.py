"""Pillow's uint8 ``Image.resize`` (bilinear / bicubic), bit for bit, over a ragged batch of packed RGB images, with the loader's
ToTensor + Normalize(0.5, 0.5) fused in (csrc/imageprep.hip).  The wrapper does not synchronise.  (Part of scene_generation_amd.ops:
see ops/__init__.py.)"""
import numpy as np
import torch

from .._hip import CONST
from ._core import _L, _call, _p, _stream, workspace

PIL_FILTERS = {'bilinear': CONST['SG_PIL_BILINEAR'], 'bicubic': CONST['SG_PIL_BICUBIC']}
# the launches of one call
PIL_COEF, PIL_HORIZONTAL, PIL_VERTICAL, PIL_ALL = (CONST['SG_PIL_' + n] for n in ('COEF', 'HORIZONTAL', 'VERTICAL', 'ALL'))
PIL_MAX_IN, PIL_MAX_OUT, PIL_MAX_IMAGES, _TABLE_COLS = (CONST['SG_PIL_' + n] for n in ('MAX_IN', 'MAX_OUT', 'MAX_IMAGES', 'TABLE_COLS'))

_lut_cache = {}


def _lut(device):
    """float32 [256] on ``device``: ``inception.read_image``'s own expression on every byte value, evaluated where the loader evaluates
    it (the host), so that the device result is bitwise the loader's"""
    t = _lut_cache.get(device)
    if t is None:
        t = _lut_cache[device] = ((torch.arange(256, dtype=torch.float32) / 255.0 - 0.5) / 0.5).to(device)
    return t


def _pil_table(table, nbytes, who):
    """the host descriptor table [N, 3] (byte offset, H, W) -> contiguous int64 NumPy array, every image checked against the limits
    and the ``nbytes`` of the buffer"""
    if isinstance(table, torch.Tensor):
        if table.is_cuda:
            raise ValueError('%s: the descriptor table is a host array (it is range-checked before the upload)' % who)
        table = table.numpy()
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != 3 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError('%s: an integer table [N, 3] of (byte offset, H, W), got %s %s' % (who, t.dtype, t.shape))
    t = np.ascontiguousarray(t, dtype=np.int64)
    if t.shape[0] > PIL_MAX_IMAGES:
        raise ValueError('%s: %d images, more than %d' % (who, t.shape[0], PIL_MAX_IMAGES))
    if t.shape[0]:
        off, H, W = t[:, 0], t[:, 1], t[:, 2]
        if int(H.min()) < 1 or int(W.min()) < 1 or int(H.max()) > PIL_MAX_IN or int(W.max()) > PIL_MAX_IN:
            raise ValueError('%s: image sizes span %d..%d x %d..%d, outside 1..%d' % (who, H.min(), H.max(), W.min(), W.max(), PIL_MAX_IN))
        end = off + H * W * 3
        if int(off.min()) < 0 or int(end.max()) > nbytes:
            bad = int(np.argmax((off < 0) | (end > nbytes)))
            raise ValueError('%s: image %d (%d x %d x 3 bytes at offset %d) leaves the buffer of %d bytes'
                             % (who, bad, H[bad], W[bad], off[bad], nbytes))
    return t


def _pil_out(out, shape, dtype, device, who):
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise ValueError('%s must be a contiguous %s tensor %s on %s, got %s %s on %s'
                         % (who, dtype, tuple(shape), device, out.dtype, tuple(out.shape), out.device))
    return out


def pil_resize(packed, table, size, filter='bilinear', out=None, out_u8=None, phases=PIL_ALL):
    """``PIL.Image.resize((OW, OH), BILINEAR | BICUBIC)`` of every image of a packed batch, on the device, bit for bit.

    ``packed``: uint8 device tensor [bytes], the images stored as tight [H, W, 3] rows at the byte offsets of ``table``, a HOST integer
    array [N, 3] of (byte offset, H, W) -- offsets need no alignment; the table is range-checked here (ValueError, nothing is
    launched) and then uploaded.  ``size`` = (OH, OW); ``filter`` 'bilinear' | 'bicubic'.

    -> ``out`` float32 [N, 3, OH, OW] = ToTensor + Normalize(0.5, 0.5) of the resized bytes (``inception.read_image``'s expression,
    bitwise), and, when ``out_u8`` (uint8 [N, OH, OW, 3]) is given, the bytes themselves: ``(out, out_u8)``.  ``out=False`` with
    ``out_u8`` writes the bytes alone and returns them.  ``phases``: a subset of the call's launches (tools/bench_imageprep.py times
    them one by one); anything but ``PIL_ALL`` leaves the outputs to whatever the workspace holds."""
    who = 'pil_resize'
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError('%s: packed must be a contiguous uint8 tensor [bytes], got %s %s' % (
            who, getattr(packed, 'dtype', type(packed)), tuple(getattr(packed, 'shape', ()))))
    if filter not in PIL_FILTERS:
        raise ValueError('%s: filter %r is not one of %s' % (who, filter, ', '.join(sorted(PIL_FILTERS))))
    try:
        OH, OW = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError('%s: size must be (OH, OW), got %r' % (who, size))
    if not (1 <= OH <= PIL_MAX_OUT and 1 <= OW <= PIL_MAX_OUT):
        raise ValueError('%s: target %d x %d is outside 1..%d' % (who, OH, OW, PIL_MAX_OUT))
    desc = _pil_table(table, packed.numel(), who + ' table')
    if not packed.is_cuda:
        raise ValueError('%s: packed is on %s -- the resize runs on the device (there is no CPU fallback)' % (who, packed.device))
    N, dev = desc.shape[0], packed.device
    if out is False and out_u8 is None:
        raise ValueError('%s: out=False needs out_u8' % who)
    if out is None:
        out = torch.empty((N, 3, OH, OW), dtype=torch.float32, device=dev)
    elif out is not False:
        _pil_out(out, (N, 3, OH, OW), torch.float32, dev, who + ' out')
    if out_u8 is not None:
        _pil_out(out_u8, (N, OH, OW, 3), torch.uint8, dev, who + ' out_u8')
    ret = out_u8 if out is False else (out if out_u8 is None else (out, out_u8))
    if N == 0:
        return ret
    if packed.data_ptr() % 4:                       # a view that starts mid-dword: the kernel loads aligned dwords
        packed = packed.clone()
    host = np.empty((N + 1, _TABLE_COLS), np.int64)
    totals = np.empty(4, np.int64)
    rc = _L().sg_pil_resize_plan(desc.ctypes.data, N, packed.numel(), OH, OW, PIL_FILTERS[filter], host.ctypes.data, totals.ctypes.data)
    if rc != 0:
        from .. import _hip
        raise ValueError('%s: %s' % (who, _hip.last_error()))
    coef_ints, inter_bytes, hblocks, nbytes = (int(v) for v in totals)
    with torch.cuda.device(dev):
        dtab = torch.from_numpy(host).to(dev)
        ws = workspace(nbytes, dev)
        _call('sg_pil_resize', _p(packed), packed.numel(), _p(dtab), N, OH, OW, PIL_FILTERS[filter], coef_ints, inter_bytes, hblocks,
              _p(_lut(dev)) if out is not False else None, _p(out_u8), _p(out) if out is not False else None, _p(ws), ws.numel(), int(phases), _stream())
    return ret
