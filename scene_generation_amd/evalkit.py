"""What the evaluation metrics (accuracy, inception, fid, featsets, lpips, imageprep) share, in one place.  A leaf: it imports none
of them, and each of them imports it.

* ``state_dict_of``: a ``state_dict`` from a file or a mapping, a DataParallel ``module.`` prefix stripped.
* ``folded`` / ``FoldCache``: the cached conv + BatchNorm fold (sg_bn_fold) and the ``nn.Module`` base that owns and drops the cache.
* ``grow_rows``: the device buffer that doubles when full, as a function over a plain tensor attribute.
* ``find_images`` / ``read_image`` / ``stored_size_chunks``: a directory's image files, one of them as a tensor, and the files of k
  directories side by side in chunks of one stored size.
"""
import os

import torch
import torch.nn as nn

from . import ops

__all__ = ['state_dict_of', 'folded', 'FoldCache', 'grow_rows', 'find_images', 'read_image', 'stored_size_chunks']


# ---- weights --------------------------------------------------------------------------------------------------------------------------
def state_dict_of(src):
    """a state_dict (a fresh dict) from a path (``torch.load`` onto the host) or a mapping; the ``module.`` prefix of a
    torch.nn.DataParallel save ('module.conv1.weight') is stripped when every key carries it"""
    if isinstance(src, str):
        src = torch.load(src, map_location='cpu')
    sd = dict(src)
    if sd and all(k.startswith('module.') for k in sd):
        return {k[len('module.'):]: v for k, v in sd.items()}
    return sd


# ---- the BatchNorm fold cache ---------------------------------------------------------------------------------------------------------
def _fold_key(conv, bn):
    ts = (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    return tuple((t.data_ptr(), t._version) for t in ts) + (float(bn.eps),)


def folded(conv, bn, cache):
    """the folded (weight, bias) of conv + bn from ``cache``, rebuilt when a tensor of the pair was replaced or written in place"""
    key = _fold_key(conv, bn)
    hit = cache.get(id(bn))
    if hit is None or hit[0] != key:
        w, b = ops.bn_fold(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        hit = cache[id(bn)] = (key, w, b)
    return hit[1], hit[2]


class FoldCache(nn.Module):
    """base of a network that runs conv + BatchNorm pairs folded: owns ``_fold_cache`` (what ``folded`` fills) and drops it wherever
    the tensors behind it change wholesale -- ``load_state_dict()``, ``.to()`` / ``.cuda()`` / ``.float()`` and ``drop_fold()``"""

    def __init__(self):
        super().__init__()
        self._fold_cache = {}

    def drop_fold(self):
        self._fold_cache.clear()

    def load_state_dict(self, *args, **kwargs):
        self.drop_fold()
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):          # the tensors move, the folded copies would not
        self.drop_fold()
        return super()._apply(fn, *args, **kwargs)


# ---- a device buffer that doubles when full -------------------------------------------------------------------------------------------
def grow_rows(buf, count, rows, first_cap, tail, dtype, device):
    """``buf`` ([capacity, *tail], or None for capacity 0) when ``count + rows`` rows fit; else a fresh buffer that holds its first
    ``count`` rows, of capacity max(capacity, ``first_cap``) doubled until they do.  One copy when it grows, no synchronisation."""
    need = count + rows
    cap = 0 if buf is None else buf.size(0)
    if need <= cap:
        return buf
    new_cap = max(cap, first_cap)
    while new_cap < need:
        new_cap *= 2
    grown = torch.empty((new_cap,) + tuple(tail), dtype=dtype, device=device)
    if count:
        grown[:count].copy_(buf[:count])
    return grown


# ---- image files ----------------------------------------------------------------------------------------------------------------------
_EXT = ('.png', '.jpg', '.jpeg', '.bmp', '.ppm', '.webp')


def find_images(root):
    """every image file under ``root``, recursively, in sorted order"""
    out = []
    for d, _, files in sorted(os.walk(root)):
        out += [os.path.join(d, f) for f in sorted(files) if f.lower().endswith(_EXT)]
    return out


def read_image(path):
    """[3, H, W] float32 in [-1, 1]: ToTensor + Normalize(0.5, 0.5) of the reference's ``__main__``"""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert('RGB'), dtype=np.float32)
    return (torch.from_numpy(a).permute(2, 0, 1) / 255.0 - 0.5) / 0.5


def stored_size_chunks(columns, batch_size):
    """``columns``: k equally long lists of paths, read side by side.  Yields k-tuples of stacked ``read_image`` tensors [n, 3, H, W],
    n <= ``batch_size``: a chunk ends where the stored size changes, where it is full, and where the paths end.  The k files at one
    index must be of one size."""
    groups, shape = [[] for _ in columns], None
    for paths in zip(*columns):
        first = read_image(paths[0])
        if groups[0] and (tuple(first.shape) != shape or len(groups[0]) == batch_size):      # one chunk per image size
            yield tuple(torch.stack(g) for g in groups)
            groups = [[] for _ in columns]
        groups[0].append(first)
        for g, path in zip(groups[1:], paths[1:]):
            img = read_image(path)
            if img.shape != first.shape:
                raise SystemExit('%s and %s differ in size' % (paths[0], path))
            g.append(img)
        shape = tuple(first.shape)
    if groups[0]:
        yield tuple(torch.stack(g) for g in groups)
