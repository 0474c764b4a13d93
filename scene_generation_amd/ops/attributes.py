"""Size and location attributes from class statistics (csrc/attributes.hip): thin wrappers of sg_attribute_histogram /
sg_sample_attributes.  No wrapper synchronises; outputs are fresh device tensors unless the caller hands in an accumulator.  (Part of
scene_generation_amd.ops: see ops/__init__.py.)"""
import torch

from .._hip import CONST
from ._core import _call, _dev, _f32, _i64, _p, _stream
from .scenegraph import _sg_counts

ATTR_MAX_OBJS, ATTR_MAX_CELLS = CONST['SG_ATTR_MAX_OBJS'], 64           # cells: one lane of a wavefront per cell
ATTR_SIZE_RULES = {'reference': CONST['SG_ATTR_RULE_REFERENCE'], 'geometric': CONST['SG_ATTR_RULE_GEOMETRIC']}


def _attr_block(t, O, A, name):
    t = _f32(t, name)
    if t.dim() != 2 or t.size(0) != O or t.size(1) != A:
        raise ValueError('%s must be [%d, %d] (size_len + grid * grid columns), got %s' % (name, O, A, tuple(t.shape)))
    return t


def _attr_vec(t, name):
    t = _i64(t, name)
    if t.dim() != 1:
        raise ValueError('%s must be a vector, got %s' % (name, tuple(t.shape)))
    return t


def sg_attribute_histogram(objs, attributes, num_classes, size_len=10, grid=5, image_class=0, counts=None):
    """counts [num_classes, size_len + grid * grid] int64 += the first set bit of every row's size block and location block, per
    class; rows of ``image_class`` and of classes outside the table are skipped"""
    objs = _attr_vec(objs, 'objs')
    A = int(size_len) + int(grid) * int(grid)
    attributes = _attr_block(attributes, objs.numel(), A, 'attributes')
    counts = _sg_counts(counts, (int(num_classes), A), objs.device)
    _call('sg_attribute_histogram', _p(objs), _p(attributes), _p(counts), objs.numel(), int(num_classes), int(size_len), int(grid),
          int(image_class), _stream())
    return counts


def sg_sample_attributes(objs, obj_to_img, triples, triple_to_img, counts, u, num_images, given=None, size_len=10, grid=5,
                         image_class=0, size_rule='reference'):
    """-> (size_idx [O] int32, loc_idx [O] int32, one-hot block [O, size_len + grid * grid] fp32) drawn from ``counts``
    [C, size_len + grid * grid] int64 with the uniforms u [O, 2]; bits of ``given`` are kept.  ``obj_to_img`` / ``triple_to_img``
    sorted ascending."""
    S, g = int(size_len), int(grid)
    if not 1 <= S <= ATTR_MAX_CELLS or g < 1 or g * g > ATTR_MAX_CELLS:
        raise ValueError('a draw holds one cell per lane of a wavefront: size_len = %d and grid * grid = %d must be in 1..%d'
                         % (S, g * g, ATTR_MAX_CELLS))
    if size_rule not in ATTR_SIZE_RULES:
        raise ValueError('size_rule %r: expected one of %s' % (size_rule, ', '.join(sorted(ATTR_SIZE_RULES))))
    objs, obj_to_img = _attr_vec(objs, 'objs'), _attr_vec(obj_to_img, 'obj_to_img')
    O, A = objs.numel(), S + g * g
    if obj_to_img.numel() != O:
        raise ValueError('obj_to_img has %d entries for %d objects' % (obj_to_img.numel(), O))
    triples, triple_to_img = _i64(triples, 'triples'), _attr_vec(triple_to_img, 'triple_to_img')
    if triples.dim() != 2 or triples.size(1) != 3 or triple_to_img.numel() != triples.size(0):
        raise ValueError('triples must be [T, 3] and triple_to_img [T], got %s and %s'
                         % (tuple(triples.shape), tuple(triple_to_img.shape)))
    _dev(counts, 'counts')
    if counts.dtype != torch.int64 or counts.dim() != 2 or counts.size(1) != A or counts.size(0) < 1 or not counts.is_contiguous():
        raise ValueError('counts must be a contiguous int64 tensor [C, %d] (size_len + grid * grid columns), got %s %s'
                         % (A, counts.dtype, tuple(counts.shape)))
    u = _f32(u, 'u')
    if tuple(u.shape) != (O, 2):
        raise ValueError('u must be [%d, 2], got %s' % (O, tuple(u.shape)))
    if given is not None:
        given = _attr_block(given, O, A, 'given')
    size_idx = torch.empty(O, dtype=torch.int32, device=objs.device)
    loc_idx = torch.empty(O, dtype=torch.int32, device=objs.device)
    block = torch.empty(O, A, dtype=torch.float32, device=objs.device)
    _call('sg_sample_attributes', _p(objs), _p(obj_to_img), _p(triples), _p(triple_to_img), _p(counts), _p(u), _p(given),
          _p(size_idx), _p(loc_idx), _p(block), int(num_images), O, triples.size(0), counts.size(0), S, g, int(image_class),
          ATTR_SIZE_RULES[size_rule], _stream())
    return size_idx, loc_idx, block
