"""Real images at the model's resolution, the way the training loader makes them: Pillow's ``Image.resize`` on the uint8 picture
(antialiased: the filter widens with the reduction; rounded to uint8 after each of its two passes), then ToTensor and
Normalize(0.5, 0.5) -- on the device, bit for bit (``ops.pil_resize``, csrc/imageprep.hip), over batches of differently sized images.

* ``pack_images(arrays)``: uint8 [H, W, 3] arrays of any sizes -> one page-locked byte buffer, back to back, and the (offset, H, W)
  table ``ops.pil_resize`` takes.
* ``resize_batch(arrays, image_size, filter)``: the one-call form -> float32 [n, 3, H, W] on the device.
* ``ImageDirFeeder(root, batch_size, image_size, ...)``: a directory -> full, uniformly sized device batches in ``find_images`` order
  (the last one may be short).  Files are decoded on the host by a small thread pool; everything after the decode runs on the device.
  ``--image_size H,W`` of the evaluation command lines (inception, fid, featsets, lpips) reads every directory through it, so a real
  set and a generated set pass through the same chain, and the Inception forward runs at the full batch size whatever the sizes of
  the files are.
* ``_feed_dir(feed, root, batch_size, ...)``: what those command lines read a directory with -- through the feeder under
  ``--image_size``, else the files at their stored sizes (``evalkit.stored_size_chunks``).  ``fid._feed_dir`` is this function.
"""
import argparse
import ctypes

import numpy as np
import torch

from . import ops
from .evalkit import find_images, stored_size_chunks

__all__ = ['pack_images', 'resize_batch', 'ImageDirFeeder', 'add_arguments', 'size_arg', 'FILTERS']

FILTERS = tuple(sorted(ops.PIL_FILTERS))
_ALIGN = 16                         # sg_stage_copy moves whole 16-byte vectors


def _check(arrays):
    out = []
    for i, a in enumerate(arrays):
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError('pack_images: image %d must be a uint8 array [H >= 1, W >= 1, 3], got %s %s' % (i, a.dtype, a.shape))
        out.append(a if a.flags['C_CONTIGUOUS'] else np.ascontiguousarray(a))
    return out


def pack_images(arrays, out=None):
    """uint8 [H, W, 3] arrays -> (``packed``, ``table``): the images back to back (no padding: an image of an odd byte count leaves
    the next one at an odd offset) in a uint8 tensor -- page-locked when CUDA is available, plain otherwise -- and the int64 NumPy
    table [n, 3] of (byte offset, H, W).  ``out``: a uint8 host tensor to fill (a staging slot) instead of a fresh one; ``packed`` is
    then its leading slice.  The fill is plain single-threaded ``memmove``: ``Tensor.copy_`` fans out over the OpenMP pool, and a burst
    of more runnable threads than the container's CPU quota freezes the whole process, the launching thread included (README, "The
    host path, root-caused")."""
    arrays = _check(arrays)
    table = np.zeros((len(arrays), 3), np.int64)
    total = 0
    for i, a in enumerate(arrays):
        table[i] = (total, a.shape[0], a.shape[1])
        total += a.nbytes
    if out is None:
        out = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    elif out.dtype != torch.uint8 or out.is_cuda or out.dim() != 1 or not out.is_contiguous() or out.numel() < total:
        raise ValueError('pack_images: out must be a contiguous uint8 host tensor of at least %d bytes' % total)
    base = out.data_ptr()
    for a, (off, _, _) in zip(arrays, table):
        ctypes.memmove(base + int(off), a.ctypes.data, a.nbytes)
    return out[:total], table


def _size(image_size):
    try:
        H, W = (int(v) for v in image_size)
    except (TypeError, ValueError):
        raise ValueError('image_size must be (H, W), got %r' % (image_size,))
    if not (1 <= H <= ops.PIL_MAX_OUT and 1 <= W <= ops.PIL_MAX_OUT):
        raise ValueError('image_size %d x %d is outside 1..%d' % (H, W, ops.PIL_MAX_OUT))
    return H, W


def resize_batch(arrays, image_size, filter='bilinear', device='cuda'):
    """uint8 [H_i, W_i, 3] arrays -> float32 [n, 3, H, W] on ``device``: each image through ``Image.resize((W, H), filter)`` and
    ToTensor + Normalize(0.5, 0.5), bitwise what Pillow and ``evalkit.read_image``'s expression give"""
    size = _size(image_size)
    packed, table = pack_images(arrays)
    return ops.pil_resize(packed.to(torch.device(device), non_blocking=True), table, size, filter)


def decode(path):
    """the file as a uint8 [H, W, 3] array (``convert('RGB')``: what ``evalkit.read_image`` reads)"""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'), dtype=np.uint8)


class ImageDirFeeder(object):
    """Iterates float32 [n, 3, H, W] device batches over the images under ``root`` in ``evalkit.find_images`` order: n =
    ``batch_size`` but for the last one.  ``image_size`` = (H, W); ``filter`` 'bilinear' | 'bicubic'.

    The files are decoded with Pillow by ``workers`` threads (default: the thread count ``utils.respect_cpu_quota`` leaves in effect,
    at most 8 -- never the host's CPU count, of which a container may own a fraction) at most two batches ahead; the results are
    taken in path order, so a batch's contents do not depend on which thread finished first.  A batch is packed into one of two
    page-locked staging slots, copied to the device by one kernel (``ops.stage_copy``) and resized there; a slot is packed again only
    after the event recorded behind its copy has completed.  An image already at the target size passes through unchanged."""

    SLOTS = 2

    def __init__(self, root, batch_size, image_size, filter='bilinear', device='cuda', workers=None):
        if int(batch_size) < 1:
            raise ValueError('ImageDirFeeder: batch_size %r' % (batch_size,))
        if filter not in ops.PIL_FILTERS:
            raise ValueError('ImageDirFeeder: filter %r is not one of %s' % (filter, ', '.join(FILTERS)))
        self.root, self.batch_size, self.size, self.filter = root, int(batch_size), _size(image_size), filter
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('ImageDirFeeder: the resize runs on the device (there is no CPU fallback), got %s' % self.device)
        if workers is None:
            from .utils import respect_cpu_quota
            workers = min(8, respect_cpu_quota(verbose=False))
        self.workers = max(1, int(workers))
        self.paths = find_images(root)

    def __len__(self):
        return len(self.paths)

    def _upload(self, slot, arrays):
        if slot.get('ev') is not None:
            slot['ev'].synchronize()                # the copy kernel that last read this slot
            slot['ev'] = None
        total = sum(a.nbytes for a in arrays)
        cap = (total + _ALIGN - 1) // _ALIGN * _ALIGN
        if slot.get('buf') is None or slot['buf'].numel() < cap:
            slot['buf'] = torch.empty(cap * 5 // 4 + 4096, dtype=torch.uint8, pin_memory=True)
        _, table = pack_images(arrays, out=slot['buf'])
        with torch.cuda.device(self.device):
            dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
            ops.stage_copy(dev, slot['buf'], cap)
            slot['ev'] = torch.cuda.Event()
            slot['ev'].record()
        return dev[:total], table

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor
        chunks = [self.paths[a:a + self.batch_size] for a in range(0, len(self.paths), self.batch_size)]
        slots = [dict() for _ in range(self.SLOTS)]
        with ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix='sg-decode') as pool:
            pending = []
            try:
                for k in range(len(chunks) + self.SLOTS):
                    if k < len(chunks):
                        pending.append([pool.submit(decode, p) for p in chunks[k]])
                    if k >= self.SLOTS:
                        arrays = [f.result() for f in pending.pop(0)]      # path order, whichever thread decoded what
                        packed, table = self._upload(slots[k % self.SLOTS], arrays)
                        yield ops.pil_resize(packed, table, self.size, self.filter)
            finally:
                for futs in pending:
                    for f in futs:
                        f.cancel()
                for slot in slots:                  # the staging slots are released here: their last copies must have read them
                    if slot.get('ev') is not None:
                        slot['ev'].synchronize()


def _feed_dir(feed, root, batch_size, *, image_size=None, resize_filter='bilinear', device='cuda'):
    """``feed(imgs)`` over the images under ``root`` -> their number.  Without ``image_size``: the files at their stored sizes, one
    chunk per run of equal sizes (``evalkit.stored_size_chunks``).  With it: every file brought to ``image_size`` by the loader's resize
    on ``device`` (``ImageDirFeeder``), in full chunks of ``batch_size``."""
    paths = find_images(root)
    if not paths:
        raise SystemExit('no images under %s' % root)
    if image_size is not None:
        batches = ImageDirFeeder(root, batch_size, image_size, resize_filter, device)
    else:
        batches = (imgs for imgs, in stored_size_chunks([paths], batch_size))
    for imgs in batches:
        feed(imgs)
    return len(paths)


# ---- command lines ----------------------------------------------------------------------------------------------------------------------
def size_arg(s):
    """'H,W' -> (H, W)"""
    try:
        H, W = (int(v) for v in s.split(','))
        return _size((H, W))
    except ValueError as e:
        raise argparse.ArgumentTypeError('--image_size takes H,W (%s)' % e)


def add_arguments(p):
    """the two flags every evaluation command line shares"""
    p.add_argument('--image_size', default=None, type=size_arg, metavar='H,W',
                   help='bring every image read from a directory to H x W first, as the training loader does: Pillow\'s antialiased uint8 '
                   'resize, bit for bit, on the device (real statistics for a model trained at H x W are made with this flag); default: '
                   'the files at their stored sizes')
    p.add_argument('--resize_filter', default='bilinear', choices=FILTERS, help='the Pillow filter of --image_size')
    return p
