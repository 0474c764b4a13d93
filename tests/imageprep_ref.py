"""Integer NumPy restatement of Pillow's uint8 ``Image.resize`` (bilinear / bicubic, no ``box``, no ``reducing_gap``): the arithmetic
csrc/imageprep.hip reproduces on the device.  Shared by tests/test_imageprep_cpu.py (restatement == Pillow) and
tests/test_gpu_imageprep.py (the unclipped accumulators; Pillow itself is the reference of the device result there).

Per axis, float64 throughout: scale = in / out, fs = max(scale, 1), support = S fs (S = 1 bilinear, 2 bicubic); for output index xx:
center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in), tap x has
weight f((x + xmin - center + 0.5) (1 / fs)); ww = the sum in tap order from 0.0; w / ww when ww != 0; the fixed-point coefficient is
(int)(+-0.5 + w 2^22) by the sign of w, (int) truncating toward zero.  An output byte is clip((2^21 + sum pixel k) >> 22, 0, 255) in
int32.  The horizontal pass runs first and is rounded to uint8; a pass whose input and output length are equal is skipped."""
import numpy as np

PRECISION_BITS = 22
SUPPORT = {'bilinear': 1.0, 'bicubic': 2.0}


def _bilinear(t):
    t = abs(t)
    return 1.0 - t if t < 1.0 else 0.0


def _bicubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


FILTER = {'bilinear': _bilinear, 'bicubic': _bicubic}


def coefficients(n_in, n_out, filt):
    """-> (xmin [n_out] int, count [n_out] int, k [n_out, ksize] int32: the fixed-point coefficients, zero past count)"""
    f, S = FILTER[filt], SUPPORT[filt]
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = S * fs
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmins, counts, k = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        xmins[xx], counts[xx] = xmin, xmax - xmin
    return xmins, counts, k


def _pass(a, n_out, filt):
    """resample axis 0 of uint8 ``a`` [n_in, ...] -> (uint8 [n_out, ...], the unclipped (2^21 + sum) >> 22 as int64)"""
    xmins, counts, k = coefficients(a.shape[0], n_out, filt)
    acc = np.empty((n_out,) + a.shape[1:], np.int64)
    src = a.astype(np.int64)
    for xx in range(n_out):
        taps = src[xmins[xx]:xmins[xx] + counts[xx]]
        kk = k[xx, :counts[xx]].astype(np.int64).reshape((-1,) + (1,) * (a.ndim - 1))
        s = (1 << (PRECISION_BITS - 1)) + (taps * kk).sum(0)
        assert np.abs(s).max() < 2 ** 31                    # the device accumulates in int32
        acc[xx] = s >> PRECISION_BITS
    return np.clip(acc, 0, 255).astype(np.uint8), acc


def resize(a, size, filt='bilinear', unclipped=False):
    """uint8 [H, W, 3] -> uint8 [OH, OW, 3], ``size`` = (OH, OW).  ``unclipped``: also the two passes' values before the clamp (None for
    a skipped pass)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    OH, OW = size
    raw = [None, None]
    if a.shape[1] != OW:
        t, raw[0] = _pass(a.transpose(1, 0, 2), OW, filt)
        a = t.transpose(1, 0, 2)
    if a.shape[0] != OH:
        a, raw[1] = _pass(a, OH, filt)
    a = np.ascontiguousarray(a)
    return (a, raw) if unclipped else a


def pil_resize(a, size, filt='bilinear'):
    """the reference itself: ``Image.resize`` of the uint8 array"""
    from PIL import Image
    res = {'bilinear': Image.BILINEAR, 'bicubic': Image.BICUBIC}[filt]
    return np.asarray(Image.fromarray(np.ascontiguousarray(a, dtype=np.uint8)).resize((size[1], size[0]), res))


def normalise(u8):
    """uint8 [..., H, W, 3] -> float32 [..., 3, H, W]: the expression of ``inception.read_image``"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(u8).astype(np.float32))
    t = t.permute(*range(t.dim() - 3), t.dim() - 1, t.dim() - 3, t.dim() - 2)
    return ((t / 255.0 - 0.5) / 0.5).contiguous()


def checkerboard(H, W, cell=1):
    """0 / 255 checkerboard [H, W, 3] of ``cell`` x ``cell`` squares: the bicubic filter overshoots on both sides of every edge"""
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat(((((y // cell) + (x // cell)) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def random_image(rs, H, W):
    return rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
