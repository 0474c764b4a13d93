"""Quasi-random inputs of the generator (csrc/qmc.hip): thin wrappers of sg_sobol_points / sg_qmc_unpack / sg_bank_draw.  Every
argument is validated here -- dtype, shape, contiguity, device -- with a ValueError that names it; no wrapper synchronises; outputs are
fresh device tensors.  (Part of scene_generation_amd.ops: see ops/__init__.py.)"""
import torch

from .._hip import CONST
from ._core import _call, _p, _stream

QMC_MAXBIT, QMC_MAX_DIMS = CONST['SG_QMC_MAXBIT'], CONST['SG_QMC_MAX_DIMS']
QMC_POINTS = 1 << QMC_MAXBIT                                   # points of the sequence, and the range of a coordinate's integer


def _qmc_arg(t, name, dtype, shape, device=None):
    """``t``: a contiguous device tensor of ``dtype`` whose shape matches ``shape`` (None: any extent) on ``device`` (None: any GPU)"""
    if not torch.is_tensor(t):
        raise ValueError('%s must be a tensor, got %s' % (name, type(t).__name__))
    if not t.is_cuda:
        raise ValueError('%s is on %s: the quasi-random kernels have no CPU fallback' % (name, t.device))
    if device is not None and t.device != device:
        raise ValueError('%s is on %s, the other operands on %s' % (name, t.device, device))
    if t.dtype != dtype:
        raise ValueError('%s must be %s, got %s' % (name, str(dtype).replace('torch.', ''), str(t.dtype).replace('torch.', '')))
    if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
        raise ValueError('%s must be [%s], got %s' % (name, ', '.join('*' if s is None else str(s) for s in shape), tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % name)
    return t


def sg_sobol_points(dirs, shift, first, n, ld=None):
    """-> int32 [n, D] (a view of a fresh [n, ld] tensor when ``ld`` > D; the padding columns are not written): the 30-bit integer
    states of points ``first`` .. ``first + n - 1`` of the digitally shifted Sobol sequence with direction numbers ``dirs`` [D, 30]
    and shift ``shift`` [D], both int32 on the device"""
    dirs = _qmc_arg(dirs, 'dirs', torch.int32, (None, QMC_MAXBIT))
    D = dirs.size(0)
    if not 1 <= D <= QMC_MAX_DIMS:
        raise ValueError('dirs holds %d dimensions: expected 1..%d' % (D, QMC_MAX_DIMS))
    shift = _qmc_arg(shift, 'shift', torch.int32, (D,), dirs.device)
    first, n = int(first), int(n)
    ld = D if ld is None else int(ld)
    if ld < D:
        raise ValueError('ld = %d is below the %d dimensions of dirs' % (ld, D))
    if first < 0 or n < 0 or first + n > QMC_POINTS:
        raise ValueError('points %d .. %d + %d: first and n must not be negative and first + n at most 2^%d' % (first, first, n, QMC_MAXBIT))
    buf = torch.empty(n, ld, dtype=torch.int32, device=dirs.device)
    _call('sg_sobol_points', _p(dirs), _p(shift), _p(buf), first, n, D, ld, _stream())
    return buf if ld == D else buf[:, :D]


def sg_qmc_unpack(points, obj_to_img, seg_off, noise_dim, max_objects):
    """points int32 [N, >= noise_dim + 3 * max_objects] (rows contiguous; a column slice of a wider tensor is fine), obj_to_img int64
    [O] sorted ascending, seg_off int32 [N + 1] (ops.segment_offsets) -> (noise fp32 [N, noise_dim], pick int32 [O], u fp32 [O, 2]);
    an object in a slot >= max_objects gets pick = -1 and u = 0"""
    noise_dim, max_objects = int(noise_dim), int(max_objects)
    D = noise_dim + 3 * max_objects
    if noise_dim < 0 or max_objects < 0 or not 1 <= D <= QMC_MAX_DIMS:
        raise ValueError('noise_dim = %d and max_objects = %d: neither may be negative and noise_dim + 3 * max_objects must be in 1..%d'
                         % (noise_dim, max_objects, QMC_MAX_DIMS))
    _qmc_arg(points if not torch.is_tensor(points) or points.is_contiguous() else points[:0], 'points', torch.int32, (None, None))
    if points.size(1) < D:                                     # (rows with a stride are fine: only the rest is checked above)
        raise ValueError('points has %d columns: noise_dim + 3 * max_objects = %d are needed' % (points.size(1), D))
    if points.size(0) > 1 and points.stride(0) < points.size(1) or points.size(1) > 1 and points.stride(1) != 1:
        raise ValueError('points must have contiguous rows (strides %s)' % (tuple(points.stride()),))
    N = points.size(0)
    ld = points.stride(0) if N > 1 else max(points.size(1), 1)
    obj_to_img = _qmc_arg(obj_to_img, 'obj_to_img', torch.int64, (None,), points.device)
    seg_off = _qmc_arg(seg_off, 'seg_off', torch.int32, (N + 1,), points.device)
    O = obj_to_img.numel()
    noise = torch.empty(N, noise_dim, dtype=torch.float32, device=points.device)
    pick = torch.empty(O, dtype=torch.int32, device=points.device)
    u = torch.empty(O, 2, dtype=torch.float32, device=points.device)
    _call('sg_qmc_unpack', _p(points), ld, _p(obj_to_img), _p(seg_off), _p(noise), _p(pick), _p(u), N, O, noise_dim, max_objects, _stream())
    return noise, pick, u


def sg_bank_draw(bank, class_off, objs, pick):
    """bank fp32 [R, rep] (the rows of all classes back to back), class_off int64 [C + 1], objs int64 [O], pick int32 [O] (30-bit
    integers) -> (rows fp32 [O, rep], row_idx int32 [O]): row (pick * rows_c) >> 30 of the object's class; -1 and a row of zeros for a
    class outside the table or without rows, and for a negative pick"""
    bank = _qmc_arg(bank, 'bank', torch.float32, (None, None))
    if bank.size(1) < 1:
        raise ValueError('bank must have at least one column, got %s' % (tuple(bank.shape),))
    class_off = _qmc_arg(class_off, 'class_off', torch.int64, (None,), bank.device)
    if class_off.numel() < 2:
        raise ValueError('class_off must hold C + 1 >= 2 offsets, got %d' % class_off.numel())
    objs = _qmc_arg(objs, 'objs', torch.int64, (None,), bank.device)
    O = objs.numel()
    pick = _qmc_arg(pick, 'pick', torch.int32, (O,), bank.device)
    rows = torch.empty(O, bank.size(1), dtype=torch.float32, device=bank.device)
    row_idx = torch.empty(O, dtype=torch.int32, device=bank.device)
    _call('sg_bank_draw', _p(bank), _p(class_off), _p(objs), _p(pick), _p(row_idx), _p(rows), O, class_off.numel() - 1, bank.size(1),
          bank.size(0), _stream())
    return rows, row_idx
