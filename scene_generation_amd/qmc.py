"""Quasi-random inputs for the generator: one scrambled Sobol point per image, generated and consumed on the device.

Chong & Forsyth extrapolate FID and the Inception score to an infinite number of images (fidinf.py, isinf.py) and note
that the extrapolated scores repeat from run to run when the generator's random inputs come from a scrambled low-discrepancy
sequence instead of a pseudo-random stream.  One image's randomness in this model is: the mask-noise row, one appearance-bank pick
per object, two attribute uniforms per object.  Here all three are coordinates of ONE point of a Sobol sequence of
``noise_dim + 3 * max_objects`` dimensions (csrc/qmc.hip, exact definitions in include/sg2im_hip.h):

* ``SobolStream``: the direction numbers and the digital shift of a ``torch.quasirandom.SobolEngine`` built on the host (the tables
  ship with torch: 21201 dimensions), uploaded once; ``draw(n)`` is one launch that writes the 30-bit integers of the next n points,
  each computed from its own number (no recurrence), so a stream can be cut anywhere.
* ``DeviceBank``: the appearance bank {class: rows} packed once into one device matrix; ``draw`` scales a 30-bit pick to a row of
  each object's class and copies it, one launch.
* ``QuasiRandomInputs``: the stream plus the column layout; ``draw`` gives the (noise, pick, u) tables of the next N images.

Everything is opt-in (``Sampler(quasi_random=...)``, ``--quasi_random 1``).  What is NOT claimed: that FID-infinity / IS-infinity
vary less across seeds with these inputs on a trained checkpoint -- nobody has measured that here."""
import numpy as np
import torch

from . import ops
from .utils import to_device_async

MAXBIT, MAX_DIMS, POINTS = ops.QMC_MAXBIT, ops.QMC_MAX_DIMS, ops.QMC_POINTS


def _count(n, name):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError('%s must be a non-negative integer, got %r' % (name, n))
    return int(n)


class SobolStream(object):
    """``draw(n)`` -> int32 [n, dimension] on ``device``: the integers x of the next n points (x * 2^-30 is the coordinate in
    [0, 1)).  ``scramble=False`` is for tests: its point 0 is all zeros.  ``device='cpu'`` holds the tables only; ``draw`` needs the
    GPU."""

    def __init__(self, dimension, scramble=True, seed=0, device='cuda'):
        if isinstance(dimension, bool) or not isinstance(dimension, (int, np.integer)) or not 1 <= dimension <= MAX_DIMS:
            raise ValueError('dimension must be an integer in 1..%d, got %r' % (MAX_DIMS, dimension))
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer))):
            raise ValueError('seed must be an integer or None, got %r' % (seed,))
        from torch.quasirandom import SobolEngine
        if SobolEngine.MAXBIT != MAXBIT:
            raise RuntimeError('torch.quasirandom.SobolEngine works on %d bits, the kernels on %d' % (SobolEngine.MAXBIT, MAXBIT))
        engine = SobolEngine(int(dimension), scramble=bool(scramble), seed=None if seed is None else int(seed))
        self.dimension, self.scramble, self.seed = int(dimension), bool(scramble), seed
        self.device = torch.device(device)
        self.dirs = to_device_async(engine.sobolstate.to(torch.int32).contiguous(), self.device)      # [D, 30], below 2^30
        self.shift = to_device_async(engine.shift.to(torch.int32).contiguous(), self.device)          # [D] (zeros when not scrambled)
        self.position = 0                       # the number of the next point

    def draw(self, n):
        n = _count(n, 'n')
        if self.position + n > POINTS:
            raise ValueError('drawing %d points from position %d leaves the sequence: it has 2^%d points' % (n, self.position, MAXBIT))
        out = ops.sg_sobol_points(self.dirs, self.shift, self.position, n)
        self.position += n
        return out

    def fast_forward(self, n):
        n = _count(n, 'n')
        if self.position + n > POINTS:
            raise ValueError('skipping %d points from position %d leaves the sequence: it has 2^%d points' % (n, self.position, MAXBIT))
        self.position += n
        return self

    def reset(self):
        self.position = 0
        return self


class DeviceBank(object):
    """``bank`` fp32 [R, rep]: the rows of class 0, then class 1, ...; ``class_off`` int64 [num_classes + 1]; ``rows_per_class``: the
    host list of the counts.  A class the dictionary does not hold has no rows."""

    def __init__(self, bank, class_off, rows_per_class):
        self.bank, self.class_off, self.rows_per_class = bank, class_off, list(rows_per_class)
        self.num_classes, self.rep = len(self.rows_per_class), bank.size(1)

    @classmethod
    def from_dict(cls, features, num_classes, device='cuda'):
        """``features``: {class id: array [rows, rep]}, what sample.load_features / load_bank return"""
        if not isinstance(features, dict) or not features:
            raise ValueError('features must be a non-empty dictionary {class id: array [rows, rep]}, got %s' % type(features).__name__)
        if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or num_classes < 1:
            raise ValueError('num_classes must be a positive integer, got %r' % (num_classes,))
        rep, blocks, counts = None, [], [0] * int(num_classes)
        for c in sorted(features):
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < num_classes:
                raise ValueError('features holds the class %r: expected integers in 0..%d' % (c, num_classes - 1))
            a = np.asarray(features[c], dtype=np.float32)
            if a.ndim != 2 or a.shape[1] < 1 or (rep is not None and a.shape[1] != rep):
                raise ValueError('features[%d] must be [rows, %s], got %s' % (c, 'rep' if rep is None else rep, a.shape))
            rep = a.shape[1]
            counts[int(c)] = a.shape[0]
            blocks.append(a)
        bank = torch.from_numpy(np.ascontiguousarray(np.concatenate(blocks, 0)))
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
        device = torch.device(device)
        return cls(to_device_async(bank, device), to_device_async(off, device), counts)

    def draw(self, objs, pick, objs_host=None):
        """-> (rows fp32 [O, rep], row_idx int32 [O]).  With the host list of the classes, an object whose class has no rows raises
        (the reference: a KeyError of its features dictionary, or its 'No features file'); without it that object gets row_idx = -1
        and a row of zeros."""
        if objs_host is not None:
            if len(objs_host) != objs.numel():
                raise ValueError('objs_host has %d entries for %d objects' % (len(objs_host), objs.numel()))
            for c in objs_host:
                if not 0 <= c < self.num_classes or self.rows_per_class[c] == 0:
                    raise ValueError('No features for class %d: the appearance bank holds no rows of it' % c)
        return ops.sg_bank_draw(self.bank, self.class_off, objs, pick)


class QuasiRandomInputs(object):
    """The randomness of the next N images from the next N points of one stream of ``noise_dim + 3 * max_objects`` dimensions:
    columns [0, noise_dim) are the image's mask-noise row; the object in slot j of its image (the j-th of the image in batch order)
    owns the columns noise_dim + 3 j (bank pick), + 1 (size uniform), + 2 (location uniform)."""

    def __init__(self, noise_dim, max_objects=32, seed=0, device='cuda'):
        for name, v, lo in (('noise_dim', noise_dim, 0), ('max_objects', max_objects, 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
                raise ValueError('%s must be an integer >= %d, got %r' % (name, lo, v))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
            raise ValueError('seed must be an integer, got %r' % (seed,))
        self.noise_dim, self.max_objects, self.seed = int(noise_dim), int(max_objects), int(seed)
        if self.dimension > MAX_DIMS:
            raise ValueError('noise_dim + 3 * max_objects = %d dimensions: the Sobol tables hold %d' % (self.dimension, MAX_DIMS))
        self.stream = SobolStream(self.dimension, scramble=True, seed=self.seed, device=device)

    @property
    def dimension(self):
        return self.noise_dim + 3 * self.max_objects

    @property
    def position(self):
        return self.stream.position

    def columns(self, slot):
        """(pick, size uniform, location uniform) columns of the object in ``slot`` of its image"""
        if not 0 <= slot < self.max_objects:
            raise ValueError('slot %r: expected 0..%d' % (slot, self.max_objects - 1))
        c = self.noise_dim + 3 * int(slot)
        return c, c + 1, c + 2

    def check_image_sizes(self, obj_to_img_host):
        """raises when the host list shows an image with more objects than a point has slots for"""
        run, prev = 0, None
        for n in obj_to_img_host:
            run = run + 1 if n == prev else 1
            prev = n
            if run > self.max_objects:
                raise ValueError('image %d has more than %d objects: a point of the quasi-random stream holds the draws of at most '
                                 'max_objects = %d per image' % (n, self.max_objects, self.max_objects))

    def draw(self, obj_to_img, seg_off, N, obj_to_img_host=None):
        """-> (noise fp32 [N, noise_dim], pick int32 [O], u fp32 [O, 2]) from the next N points; the stream moves on by N.  No host
        synchronisation.  With the host list of obj_to_img an image over ``max_objects`` raises before anything is drawn; without it
        the objects past the limit get pick = -1 and u = 0."""
        N = _count(N, 'N')
        if obj_to_img_host is not None:
            if len(obj_to_img_host) != obj_to_img.numel():
                raise ValueError('obj_to_img_host has %d entries for %d objects' % (len(obj_to_img_host), obj_to_img.numel()))
            self.check_image_sizes(obj_to_img_host)
        if self.stream.position + N > POINTS:
            raise ValueError('drawing %d points from position %d leaves the sequence: it has 2^%d points' % (N, self.stream.position, MAXBIT))
        points = self.stream.draw(N)
        return ops.sg_qmc_unpack(points, obj_to_img, seg_off, self.noise_dim, self.max_objects)
