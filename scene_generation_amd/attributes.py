"""Size and location attributes sampled from class statistics, on the device.

The reference's sampler has two ends.  ``scripts/create_attributes_file.py`` counts, per object class, how often each size bucket
and each location cell occurs in a dataset (``attributes_10_25.pickle``); ``--sample_attributes 1`` of ``scripts/sample_images.py``
then draws every object's size and location bits from those counts instead of deriving them from the ground truth, the locations
constrained by the graph's relations (data/coco_panoptic.py:336-340,389-391,432-449,468-521): the subject of "left of" lands in a
column left of its partner, the subject of "inside" takes its partner's cell, and so on.  That is what lets a person write only
``sheep left of tree`` and still get a plausible layout.  Here both ends are launches over a collated batch (csrc/attributes.hip,
exact rules in include/sg2im_hip.h and DESIGN.md section 4n):

* ``AttributeStats``: the table counts [num_classes, size_len + grid * grid] int64 on the device; ``update`` adds a batch without
  a host read; ``save`` / ``load`` as ``.npz`` (the dense table) or ``.pickle`` (the reference's dictionary of per-name lists, in
  both directions).
* ``sample_attributes``: one launch, one wavefront per image, that fills the size and location blocks the caller did not give.
  The draws come from a table of uniforms made on the host from ``seed`` and uploaded before the launch (``draw_uniforms``), row o
  for object o, so an image's result does not depend on its place in the batch.

    python -m scene_generation_amd.attributes build --output F.pickle [--num_samples n]     statistics of the synthetic loader
    python -m scene_generation_amd.attributes show F.pickle                                 the per-class tables

Every object id is global (collated) and every image ends with its ``__image__`` object (class 0)."""
import argparse
import pickle

import numpy as np
import torch

from . import ops
from .scenegraph import GRID, SIZE_LEN
from .utils import to_device_async

SIZE_RULES = ('reference', 'geometric')
MAX_OBJS, MAX_CELLS = ops.ATTR_MAX_OBJS, ops.ATTR_MAX_CELLS


def check_sizes(size_len, grid):
    """a draw holds one cell per lane of a wavefront"""
    if not 1 <= int(size_len) <= MAX_CELLS or int(grid) < 1 or int(grid) ** 2 > MAX_CELLS:
        raise ValueError('size_len = %d and grid * grid = %d must be in 1..%d (one lane of a wavefront per cell)'
                         % (size_len, int(grid) ** 2, MAX_CELLS))


def _class_names(vocab):
    """{name: class index} through the two tables Model.encode_scene_graphs uses (dataset id in between)"""
    if vocab is None or 'object_name_to_idx' not in vocab or 'object_to_idx' not in vocab:
        raise ValueError('the pickle format names classes: it needs a vocab with object_name_to_idx and object_to_idx')
    to_idx = vocab['object_to_idx']
    out = {}
    for name, data_id in vocab['object_name_to_idx'].items():
        c = to_idx.get(str(data_id), to_idx.get(data_id))
        if c is not None:
            out[name] = int(c)
    return out


class AttributeStats(object):
    """counts [num_classes, size_len + grid * grid] int64: per class, how often each size bucket (first ``size_len`` columns) and each
    location cell was seen.  ``device='cpu'`` holds a table for saving / loading only; ``update`` needs the GPU."""

    def __init__(self, num_classes, size_len=SIZE_LEN, grid=GRID, device='cuda', image_class=0, counts=None):
        check_sizes(size_len, grid)
        self.num_classes, self.size_len, self.grid, self.image_class = int(num_classes), int(size_len), int(grid), int(image_class)
        self.device = torch.device(device)
        shape = (self.num_classes, self.size_len + self.grid ** 2)
        if counts is None:
            self.counts = torch.zeros(shape, dtype=torch.int64, device=self.device)
        else:
            counts = torch.as_tensor(np.ascontiguousarray(counts, dtype=np.int64)) if not torch.is_tensor(counts) else counts
            if tuple(counts.shape) != shape or counts.dtype != torch.int64:
                raise ValueError('counts must be int64 %s (num_classes, size_len + grid * grid), got %s %s'
                                 % (shape, counts.dtype, tuple(counts.shape)))
            self.counts = counts.contiguous() if self.device.type == 'cpu' else to_device_async(counts.contiguous(), self.device)

    @property
    def width(self):
        return self.size_len + self.grid ** 2

    def update(self, objs, attributes):
        """adds one collated batch (objs [O] int64, attributes [O, size_len + grid * grid] fp32); no host synchronisation"""
        if attributes.dim() != 2 or attributes.size(1) != self.width:
            raise ValueError('attributes must be [O, %d] (size_len + grid * grid), got %s' % (self.width, tuple(attributes.shape)))
        ops.sg_attribute_histogram(objs, attributes, self.num_classes, self.size_len, self.grid, self.image_class, counts=self.counts)
        return self

    # -- files ---------------------------------------------------------------------------------------------------------------------
    def to_dict(self, vocab):
        """the reference's {'location': {name: [...]}, 'size': {name: [...]}} (create_attributes_file.py:118-137); the __image__
        class, which it never counts, is left out"""
        rows = self.counts.cpu().numpy()
        out = {'location': {}, 'size': {}}
        for name, c in _class_names(vocab).items():
            if c == self.image_class or not 0 <= c < self.num_classes:
                continue
            out['size'][name] = [int(v) for v in rows[c, :self.size_len]]
            out['location'][name] = [int(v) for v in rows[c, self.size_len:]]
        return out

    @classmethod
    def from_dict(cls, d, vocab, num_classes=None, device='cuda', image_class=0):
        """a dictionary in the reference's shape; names the vocab does not know are ignored, classes it does not list stay zero"""
        names = _class_names(vocab)
        if num_classes is None:
            num_classes = len(vocab['object_to_idx'])
        sizes, locs = d.get('size', {}), d.get('location', {})
        some = next(iter(sizes.values()), None), next(iter(locs.values()), None)
        if some[0] is None or some[1] is None:
            raise ValueError('the attributes file lists no class')
        size_len, cells = len(some[0]), len(some[1])
        grid = int(round(cells ** 0.5))
        if grid * grid != cells:
            raise ValueError('%d location cells are not a square grid' % cells)
        counts = np.zeros((num_classes, size_len + cells), dtype=np.int64)
        for block, lo, width in ((sizes, 0, size_len), (locs, size_len, cells)):
            for name, row in block.items():
                c = names.get(name)
                if c is None or not 0 <= c < num_classes:
                    continue
                if len(row) != width:
                    raise ValueError('class %r has %d entries, the others %d' % (name, len(row), width))
                counts[c, lo:lo + width] = np.asarray(row, dtype=np.int64)
        return cls(num_classes, size_len, grid, device, image_class, counts=counts)

    def save(self, path, vocab=None):
        """``.npz``: the dense table with its shape parameters; anything else: the reference's pickle (needs ``vocab``)"""
        if str(path).endswith('.npz'):
            np.savez(path, counts=self.counts.cpu().numpy(), size_len=self.size_len, grid=self.grid, image_class=self.image_class)
        else:
            with open(path, 'wb') as f:
                pickle.dump(self.to_dict(vocab), f)
        return path

    @classmethod
    def load(cls, path, vocab=None, device='cuda', num_classes=None):
        if str(path).endswith('.npz'):
            with np.load(path) as z:
                counts = z['counts']
                return cls(counts.shape[0], int(z['size_len']), int(z['grid']), device, int(z['image_class']), counts=counts)
        with open(path, 'rb') as f:
            return cls.from_dict(pickle.load(f), vocab, num_classes, device)


def draw_uniforms(seed, O):
    """the table of the draws: numpy.random.RandomState(seed).random_sample((O, 2)) as fp32, kept below 1; column 0 is an object's
    size draw, column 1 its location draw"""
    u = np.random.RandomState(seed).random_sample((O, 2)).astype(np.float32)
    return np.minimum(u, np.float32(1.0 - 2.0 ** -24))


def check_image_sizes(obj_to_img_host):
    """raises when the host list shows an image with more objects than the kernel keeps state for"""
    run, prev = 0, None
    for n in obj_to_img_host:
        run = run + 1 if n == prev else 1
        prev = n
        if run > MAX_OBJS:
            raise ValueError('image %d has more than %d objects: sample_attributes keeps the state of at most that many per image'
                             % (n, MAX_OBJS))


def sample_attributes(objs, triples, obj_to_img, stats, given=None, seed=0, u=None, triple_to_img=None, num_images=None,
                      obj_to_img_host=None, size_rule='reference'):
    """-> (attributes [O, size_len + grid * grid] fp32 one-hot blocks, size_idx [O] int32, loc_idx [O] int32) drawn from ``stats``
    (an ``AttributeStats``) under the relations of ``triples``; bits of ``given`` are kept.

    ``u`` [O, 2]: uniforms in [0, 1) (numpy or tensor; default ``draw_uniforms(seed, O)``), uploaded before the launch.
    ``triple_to_img`` defaults to ``obj_to_img[triples[:, 0]]``, a device gather.  ``num_images`` / ``obj_to_img_host`` (the host
    list of obj_to_img): without either the call reads ``obj_to_img`` back once -- its only synchronisation.  With the host list an
    image over the object limit raises."""
    S, g = stats.size_len, stats.grid
    check_sizes(S, g)
    if size_rule not in SIZE_RULES:
        raise ValueError('size_rule %r: expected one of %s' % (size_rule, ', '.join(SIZE_RULES)))
    O, A = objs.numel(), S + g * g
    if given is not None and (given.dim() != 2 or tuple(given.shape) != (O, A)):
        raise ValueError('given must be [%d, %d] (size_len + grid * grid columns), got %s' % (O, A, tuple(given.shape)))
    if tuple(stats.counts.shape)[1:] != (A,):
        raise ValueError('the statistics have %d columns, size_len + grid * grid is %d' % (stats.counts.size(1), A))
    if obj_to_img_host is None and num_images is None:
        obj_to_img_host = obj_to_img.tolist()                   # the documented read
    if obj_to_img_host is not None:
        if len(obj_to_img_host) != O:
            raise ValueError('obj_to_img has %d entries for %d objects' % (len(obj_to_img_host), O))
        check_image_sizes(obj_to_img_host)
        if num_images is None:
            num_images = obj_to_img_host[-1] + 1 if O else 0
    if u is None:
        u = draw_uniforms(seed, O)
    if not torch.is_tensor(u):
        u = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32))
    if tuple(u.shape) != (O, 2):
        raise ValueError('u must be [%d, 2], got %s' % (O, tuple(u.shape)))
    ops._dev(objs, 'objs')
    u = u if u.is_cuda else to_device_async(u, objs.device)
    if triple_to_img is None:
        triple_to_img = obj_to_img[triples[:, 0].clamp(0, max(O - 1, 0))] if O else triples.new_zeros(triples.size(0))
    size_idx, loc_idx, block = ops.sg_sample_attributes(objs, obj_to_img, triples, triple_to_img, stats.counts, u, int(num_images),
                                                        given=given, size_len=S, grid=g, image_class=stats.image_class,
                                                        size_rule=size_rule)
    return block, size_idx, loc_idx


# ---- command line -------------------------------------------------------------------------------------------------------------------
def build_stats(batches, num_classes, size_len=SIZE_LEN, grid=GRID, device='cuda'):
    """the statistics of any iterable of collated batches (imgs, objs, boxes, masks, triples, obj_to_img, triple_to_img,
    attributes); nothing is read back"""
    stats = AttributeStats(num_classes, size_len, grid, device)
    for batch in batches:
        stats.update(batch[1].to(stats.device), batch[7].to(stats.device))
    return stats


def format_tables(stats, vocab=None):
    """one line per class that was seen: name, size counts, location counts row by row"""
    rows = stats.counts.cpu().numpy()
    names = {}
    if vocab is not None:
        names = {c: n for n, c in _class_names(vocab).items()}
    lines = []
    for c in range(stats.num_classes):
        if not rows[c].any():
            continue
        cells = rows[c, stats.size_len:].reshape(stats.grid, stats.grid)
        lines.append('%s  size %s  location %s' % (names.get(c, 'class %d' % c), ' '.join(str(v) for v in rows[c, :stats.size_len]),
                                                   ' / '.join(' '.join(str(v) for v in r) for r in cells)))
    return lines


def make_parser():
    p = argparse.ArgumentParser(prog='python -m scene_generation_amd.attributes', description=__doc__.split('\n')[0])
    sub = p.add_subparsers(dest='command', required=True)
    b = sub.add_parser('build', help='statistics of the synthetic loader with attributes derived from its own boxes and masks')
    b.add_argument('--output', required=True, help='.pickle (the reference\'s format) or .npz (the dense table)')
    b.add_argument('--num_samples', default=256, type=int)
    b.add_argument('--batch_size', default=32, type=int)
    b.add_argument('--num_objs', default=None, type=int, help='object classes including __image__ (default: the synthetic vocabulary)')
    b.add_argument('--image_size', default=64, type=int)
    b.add_argument('--mask_size', default=16, type=int)
    b.add_argument('--seed', default=0, type=int)
    s = sub.add_parser('show', help='print the per-class tables of a file')
    s.add_argument('file')
    s.add_argument('--num_objs', default=None, type=int)
    return p


def main(argv=None):
    from .scenegraph import regraph
    from .synthetic import VOCAB_C, make_batch, make_sampling_vocab
    args = make_parser().parse_args(argv)
    num_objs = args.num_objs or VOCAB_C
    vocab = make_sampling_vocab(num_objs)
    if args.command == 'show':
        stats = AttributeStats.load(args.file, vocab, device='cpu')
        for line in format_tables(stats, vocab):
            print(line)
        return stats

    def batches():
        done, k = 0, 0
        while done < args.num_samples:
            n = min(args.batch_size, args.num_samples - done)
            batch = make_batch(N=n, size=args.image_size, mask_size=args.mask_size, num_objs=num_objs, seed=args.seed + k)
            yield regraph(batch, seed=args.seed + k)
            done, k = done + n, k + 1
    stats = build_stats(batches(), num_objs)
    stats.save(args.output, vocab)
    print('Saved attributes file to {}'.format(args.output))
    return stats


if __name__ == '__main__':
    main()
