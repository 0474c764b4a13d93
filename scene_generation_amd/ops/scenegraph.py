"""Scene graphs from layouts (csrc/scenegraph.hip): thin wrappers of sg_object_centers / sg_object_attributes / sg_pair_predicates /
sg_draw_pairs / sg_triple_agreement / sg_attribute_agreement.  No wrapper synchronises; outputs are fresh device tensors unless the
caller hands in an accumulator.  (Part of scene_generation_amd.ops: see ops/__init__.py.)"""
import torch

from .._hip import CONST
from ._core import _call, _dev, _f32, _i64, _p, _stream

SCENEGRAPH_MAX_M, SCENEGRAPH_MAX_P = CONST['SG_SCENEGRAPH_MAX_M'], CONST['SG_SCENEGRAPH_MAX_P']


def _sg_i32(t, name):
    _dev(t, name)
    if t.dtype != torch.int32:
        raise TypeError('%s must be int32, got %s' % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _sg_boxes(boxes):
    boxes = _f32(boxes, 'boxes')
    if boxes.dim() != 2 or boxes.size(1) != 4:
        raise ValueError('boxes must be [O, 4], got %s' % (tuple(boxes.shape),))
    return boxes


def _sg_centers(centers, O):
    centers = _f32(centers, 'centers')
    if tuple(centers.shape) != (O, 2):
        raise ValueError('centers must be [%d, 2], got %s' % (O, tuple(centers.shape)))
    return centers


def _sg_counts(counts, shape, device):
    """an int64 accumulator the kernel ADDS to: a fresh zeroed one, or the caller's (contiguous: a copy would swallow the sums)"""
    if counts is None:
        return torch.zeros(shape, dtype=torch.int64, device=device)
    _dev(counts, 'counts')
    if counts.dtype != torch.int64 or tuple(counts.shape) != tuple(shape) or not counts.is_contiguous():
        raise ValueError('counts must be a contiguous int64 tensor of shape %s' % (tuple(shape),))
    return counts


def sg_object_centers(boxes, masks):
    """-> (centers [O, 2] fp32, count [O] int32) of masks [O, M, M] (int64: set when == 1; fp32: set when > 0.5)"""
    boxes = _sg_boxes(boxes)
    _dev(masks, 'masks')
    if masks.dtype not in (torch.int64, torch.float32):
        raise TypeError('masks must be int64 or float32, got %s' % masks.dtype)
    O = boxes.size(0)
    if masks.dim() != 3 or masks.size(0) != O or masks.size(1) != masks.size(2):
        raise ValueError('masks must be [%d, M, M], got %s' % (O, tuple(masks.shape)))
    masks = masks if masks.is_contiguous() else masks.contiguous()
    centers = torch.empty(O, 2, dtype=torch.float32, device=boxes.device)
    count = torch.empty(O, dtype=torch.int32, device=boxes.device)
    _call('sg_object_centers', _p(boxes), _p(masks), 1 if masks.dtype == torch.int64 else 0, _p(centers), _p(count), O,
          masks.size(1), _stream())
    return centers, count


def sg_object_attributes(boxes, centers, size_len=10, grid=5, onehot=True):
    """-> (size_idx [O] int32, loc_idx [O] int32, one-hot block [O, size_len + grid * grid] fp32 or None)"""
    boxes = _sg_boxes(boxes)
    O = boxes.size(0)
    centers = _sg_centers(centers, O)
    size_idx = torch.empty(O, dtype=torch.int32, device=boxes.device)
    loc_idx = torch.empty(O, dtype=torch.int32, device=boxes.device)
    block = torch.empty(O, size_len + grid * grid, dtype=torch.float32, device=boxes.device) if onehot else None
    _call('sg_object_attributes', _p(boxes), _p(centers), _p(size_idx), _p(loc_idx), _p(block), O, int(size_len), int(grid), _stream())
    return size_idx, loc_idx, block


def sg_pair_predicates(boxes, centers, s, o):
    """-> p [T] int64 for the pairs (s[t], o[t]) of global object ids"""
    boxes = _sg_boxes(boxes)
    O = boxes.size(0)
    centers = _sg_centers(centers, O)
    s, o = _i64(s, 's'), _i64(o, 'o')
    if s.dim() != 1 or s.shape != o.shape:
        raise ValueError('s and o must be [T]')
    p = torch.empty_like(s)
    _call('sg_pair_predicates', _p(boxes), _p(centers), _p(s), _p(o), 1, _p(p), 1, s.numel(), O, _stream())
    return p


def sg_draw_pairs(seg_off, tri_off, u, boxes, centers, T):
    """-> (triples [T, 3], triple_to_img [T]) int64 in collate order; u [O, r, 2] fp32, T = tri_off[N] (known to the caller)"""
    boxes = _sg_boxes(boxes)
    O = boxes.size(0)
    centers = _sg_centers(centers, O)
    seg_off, tri_off = _sg_i32(seg_off, 'seg_off'), _sg_i32(tri_off, 'tri_off')
    u = _f32(u, 'u')
    if u.dim() != 3 or u.size(0) != O or u.size(2) != 2 or u.size(1) < 1:
        raise ValueError('u must be [%d, r, 2], got %s' % (O, tuple(u.shape)))
    if seg_off.dim() != 1 or seg_off.shape != tri_off.shape or seg_off.numel() < 1:
        raise ValueError('seg_off and tri_off must be [N + 1]')
    N = seg_off.numel() - 1
    # zero-filled: an image whose triple count does not fit its object count is left unwritten by the kernel
    triples = torch.zeros(T, 3, dtype=torch.int64, device=boxes.device)
    triple_to_img = torch.zeros(T, dtype=torch.int64, device=boxes.device)
    _call('sg_draw_pairs', _p(seg_off), _p(tri_off), _p(u), _p(boxes), _p(centers), _p(triples), _p(triple_to_img), N, O, int(T),
          u.size(1), _stream())
    return triples, triple_to_img


def sg_triple_agreement(triples, boxes, centers, num_preds, counts=None):
    """counts [num_preds, 2] int64 += (triples seen, triples whose derived predicate agrees) per predicate >= 1"""
    boxes = _sg_boxes(boxes)
    O = boxes.size(0)
    centers = _sg_centers(centers, O)
    triples = _i64(triples, 'triples')
    if triples.dim() != 2 or triples.size(1) != 3:
        raise ValueError('triples must be [T, 3]')
    counts = _sg_counts(counts, (int(num_preds), 2), boxes.device)
    _call('sg_triple_agreement', _p(triples), _p(boxes), _p(centers), _p(counts), triples.size(0), O, int(num_preds), _stream())
    return counts


def sg_attribute_agreement(attributes, size_idx, loc_idx, size_len=10, grid=5, counts=None):
    """counts [2, 2] int64 += ((size blocks with one bit, of which agreeing), (location blocks with one bit, of which agreeing))"""
    attributes = _f32(attributes, 'attributes')
    O = attributes.size(0)
    if attributes.dim() != 2 or attributes.size(1) != size_len + grid * grid:
        raise ValueError('attributes must be [O, %d], got %s' % (size_len + grid * grid, tuple(attributes.shape)))
    size_idx, loc_idx = _sg_i32(size_idx, 'size_idx'), _sg_i32(loc_idx, 'loc_idx')
    if size_idx.numel() != O or loc_idx.numel() != O:
        raise ValueError('size_idx and loc_idx must be [%d]' % O)
    counts = _sg_counts(counts, (2, 2), attributes.device)
    _call('sg_attribute_agreement', _p(attributes), _p(size_idx), _p(loc_idx), _p(counts), O, int(size_len), int(grid), _stream())
    return counts
