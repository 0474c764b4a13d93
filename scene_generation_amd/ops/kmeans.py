"""Segmented k-means (csrc/kmeans.hip): thin wrappers of sg_kmeans_assign / _update / _relocate / _pp_step over one fp32 array
x [P, D] whose rows are grouped by class (offsets [C + 1] int32).  Every per-problem tensor carries a leading restart dimension R.
(Part of scene_generation_amd.ops: see ops/__init__.py.)"""
import numpy as np
import torch

from .._hip import CONST
from ._core import _L, _call, _dev, _f32, _p, _stream, workspace

KMEANS_TILE, KMEANS_MAX_K, KMEANS_MAX_D = CONST['SG_KMEANS_TILE'], CONST['SG_KMEANS_MAX_K'], CONST['SG_KMEANS_MAX_D']


def _i32(t, name):
    _dev(t, name)
    if t.dtype != torch.int32:
        raise TypeError('%s must be int32, got %s' % (name, t.dtype))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % name)
    return t


def _fout(t, name):
    """an fp32 tensor the kernel writes: must be contiguous (a copy would swallow the result)"""
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % name)
    return _f32(t, name)


class KMeansPlan(object):
    """How the launches walk the classes: ``tiles`` [T, 2] int32 = (class, first row relative to the class's start) in pieces of at
    most KMEANS_TILE rows and ``tile_off`` [C + 1], both on the device; ``sizes`` (numpy int64 [C]) stays on the host.  Built once
    per (x, offsets) from ONE device-to-host read of the offsets."""

    def __init__(self, offsets):
        self.offsets = _i32(offsets, 'offsets')
        off = self.offsets.cpu().numpy().astype(np.int64)
        assert off.ndim == 1 and off.size >= 2 and off[0] == 0 and (np.diff(off) >= 0).all(), 'offsets must be a CSR row pointer'
        self.C, self.P = off.size - 1, int(off[-1])
        self.sizes = np.diff(off)
        per = (self.sizes + KMEANS_TILE - 1) // KMEANS_TILE
        tile_off = np.concatenate([[0], np.cumsum(per)])
        self.T = int(tile_off[-1])
        cls = np.repeat(np.arange(self.C), per)
        first = (np.arange(self.T) - tile_off[cls]) * KMEANS_TILE
        tiles = np.stack([cls, first], 1).astype(np.int32).reshape(-1, 2)
        dev = offsets.device
        self.tiles = torch.from_numpy(np.ascontiguousarray(tiles) if self.T else np.zeros((1, 2), np.int32)).to(dev)
        self.tile_off = torch.from_numpy(tile_off.astype(np.int32)).to(dev)


def kmeans_plan(offsets):
    return KMeansPlan(offsets)


def _dims(x, centers, plan):
    x = _f32(x, 'x')
    centers = _fout(centers, 'centers')
    assert x.dim() == 2 and x.size(0) == plan.P, 'x must be [P, D] with P = offsets[-1]'
    if centers.dim() == 3:
        centers = centers.unsqueeze(0)
    R, C, K, D = centers.shape
    assert C == plan.C and D == x.size(1), 'centers must be [R, C, K, D]'
    return x, centers, R, K, D


def kmeans_assign(x, plan, centers, labels, mind2, changed, acount, state=None, final_pass=False):
    """labels [R, P] int32 / mind2 [R, P] <- nearest of the class's centres (a tie: the lowest index); ADDS the number of labels that
    changed to ``changed`` [R, C] and the rows per centre to ``acount`` [R, C, K] (int32; kmeans_update clears them)."""
    x, centers, R, K, D = _dims(x, centers, plan)
    _call('sg_kmeans_assign', _p(x), _p(plan.offsets), _p(plan.tiles), _p(centers), _p(state), _p(_i32(labels, 'labels')),
          _p(_fout(mind2, 'mind2')), _p(_i32(changed, 'changed')), _p(_i32(acount, 'acount')), plan.P, plan.C, K, D, R, plan.T,
          1 if final_pass else 0, _stream())


def kmeans_update(x, plan, labels, mind2, centers, counts, inertia, shift, tolvar=None, state=None, n_iter=None, changed=None,
                  acount=None, final_pass=False):
    """centers [R, C, K, D] <- the means of the rows per label (in place), counts [R, C, K] int32, inertia / shift [R, C]; the
    bookkeeping of one Lloyd iteration on ``state`` / ``n_iter`` [R, C] int32 when given (include/sg2im_hip.h)."""
    x, centers, R, K, D = _dims(x, centers, plan)
    wsb = _L().sg_kmeans_update_ws_bytes(plan.T, K, D, R)
    _call('sg_kmeans_update', _p(x), _p(plan.offsets), _p(plan.tiles), _p(plan.tile_off), _p(_i32(labels, 'labels')),
          _p(_fout(mind2, 'mind2')), _p(centers), _p(_i32(counts, 'counts')), _p(_fout(inertia, 'inertia')), _p(_fout(shift, 'shift')),
          _p(tolvar), _p(state), _p(n_iter), _p(changed), _p(acount), _p(workspace(wsb, x.device)), wsb, plan.P, plan.C, K, D, R,
          plan.T, 1 if final_pass else 0, _stream())


def kmeans_relocate(plan, labels, mind2, acount, state=None):
    """per empty centre of a class (ascending): the row farthest from its centre (among rows that are not alone) takes its label"""
    labels, acount = _i32(labels, 'labels'), _i32(acount, 'acount')
    R, K = acount.size(0), acount.size(-1)
    assert acount.dim() == 3 and acount.size(1) == plan.C
    _call('sg_kmeans_relocate', _p(plan.offsets), _p(state), _p(labels), _p(_fout(mind2, 'mind2')), _p(acount), plan.P, plan.C, K, R,
          _stream())


def kmeans_pp_step(x, plan, u, centers, mind2, picks, round):
    """one round of k-means++ seeding for every class: centers[..., round, :] and picks [R, C, K] int32 (class-relative rows)"""
    x, centers, R, K, D = _dims(x, centers, plan)
    u = _f32(u, 'u')
    assert u.numel() == R * plan.C * K and picks.numel() == R * plan.C * K
    wsb = _L().sg_kmeans_pp_step_ws_bytes(plan.T, R)
    _call('sg_kmeans_pp_step', _p(x), _p(plan.offsets), _p(plan.tiles), _p(plan.tile_off), _p(u), _p(centers),
          _p(_fout(mind2, 'mind2')), _p(_i32(picks, 'picks')), _p(workspace(wsb, x.device)), wsb, plan.P, plan.C, K, D, R, plan.T,
          int(round), _stream())
