"""Plain restatements of what LPIPS as a training loss computes (scene_generation_amd/lpips.py LPIPSLoss, ops.lpips_layer_bwd,
ops.lpips_input_bwd), shared by tests/test_lpips_loss_cpu.py and tests/test_gpu_lpips_loss.py: the gradient
of one tap by torch autograd of ``lpips_ref.layer_ref``, the closed form the kernel implements in NumPy (for the zero-norm rule,
where autograd has no answer), the whole loss through ``lpips_ref.vgg16_taps``, and the case tables.  CPU only, float64 and float32;
nothing here touches the library."""
import numpy as np
import torch
import torch.nn.functional as F

import lpips_ref as LR

EPS = LR.EPS
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# (P, C, HW) of the kernel cases, each with the reason it is there.  The backward launches by the forward's plan (csrc/lpips.hip
# layer_plan): 64-pixel tiles of 4 channel groups while C <= 128 and the launch has 256 workgroups, else 16-pixel tiles of 16 groups;
# 16 or 32 channels of a thread in registers, the rest read again.
LAYER_BWD = [
    ((1, 1, 1), 'one element; C below the 16 channel groups'),
    ((2, 3, 5), 'C below the channel-group count, a partial tile'),
    ((2, 65, 35), 'odd C, two full 16-pixel tiles and a tail tile of 3'),
    ((2, 192, 9), '12 channels a thread: the 16-register form, partly empty'),
    ((2, 256, 16), 'exactly 16 channels a thread, exactly one tile'),
    ((1, 512, 20), '32 channels a thread: the 32-register form, full'),
    ((1, 520, 9), 'channels past the 32 registers of a thread: the re-read loops of all three phases'),
    ((4, 64, 4096), '64-pixel tiles, 16 registers (256 workgroups: the threshold of the wide form)'),
    ((4, 128, 4095), '64-pixel tiles, 32 registers, a ragged last tile of 63'),
    ((3, 128, 4096), 'one pair fewer than the threshold: 192 workgroups of the wide form are too few, so 16-pixel tiles, 8 of 16 registers'),
]
INPUT_BWD = [(1, 3, 1, 1), (2, 3, 5, 7), (3, 3, 33, 31)]


def layer_inputs(shape):
    """-> f0, f1 [P, C, HW] float32 as behind a ReLU (about half the entries 0) but with no all-zero pixel, w [C] float32 with a
    fifth of its entries 0, gout [P] float64 of mixed sign and unequal magnitudes"""
    P, C, HW = shape
    g = torch.Generator().manual_seed(P * 1000003 + C * 101 + HW + 17)
    out = []
    for shift in (0.0, 0.2):
        f = F.relu(torch.randn(P, C, HW, generator=g) + shift)
        lift = 0.5 + torch.rand(P, HW, generator=g)
        dead = f.pow(2).sum(1) == 0
        f[:, 0, :] = torch.where(dead, lift, f[:, 0, :])
        assert bool((f.pow(2).sum(1) > 0).all())
        out.append(f)
    w = torch.rand(C, generator=g)
    w[::5] = 0
    gout = torch.tensor([(-1.0) ** p * (0.5 + 0.37 * p) for p in range(P)], dtype=torch.float64)
    return out[0], out[1], w, gout


def layer_grad_autograd(f0, f1, w, gout, dtype, eps=EPS):
    """d (sum_p gout[p] * layer_ref(f0, f1, w)[p]) / d f0 by torch autograd in ``dtype`` -> tensor of f0's shape in ``dtype``"""
    a = f0.detach().to(dtype).clone().requires_grad_(True)
    out = LR.layer_ref(a, f1.detach().to(dtype), None if w is None else w.to(dtype), eps)
    (out * gout.to(dtype)).sum().backward()
    return a.grad


def layer_grad_closed(f0, f1, w, gout, dtype, eps=EPS):
    """the closed form the kernel implements, in NumPy in ``dtype`` (np.float64 or np.float32), every operation rounded to it:
        g_c = 2 w_c t_c (gout[p] / HW),  dot = sum_c g_c f0_c,  gf0_k = g_k / s0 - (f0_k / s0) * ((dot / s0) / n0)
    with the second term 0 where n0 == 0.  f0, f1 [P, C, HW]; -> array [P, C, HW]"""
    f0, f1 = np.asarray(f0, dtype), np.asarray(f1, dtype)
    P, C, HW = f0.shape
    wv = np.ones(C, dtype) if w is None else np.asarray(w, dtype)
    gs = (np.asarray(gout, np.float64) / HW).astype(dtype).reshape(P, 1, 1)
    eps = dtype(eps)
    n0 = np.sqrt((f0 * f0).sum(1, keepdims=True, dtype=dtype))
    n1 = np.sqrt((f1 * f1).sum(1, keepdims=True, dtype=dtype))
    s0, s1 = n0 + eps, n1 + eps
    t = f0 / s0 - f1 / s1
    g = (dtype(2) * wv.reshape(1, C, 1)) * t * gs
    dot = (g * f0).sum(1, keepdims=True, dtype=dtype)
    with np.errstate(divide='ignore', invalid='ignore'):
        k = np.where(n0 > 0, (dot / s0) / n0, dtype(0))
    return (g / s0 - (f0 / s0) * k).astype(dtype)


def input_bwd_np(gy):
    """the scaling layer's backward as NumPy float32: gy / scale[c], one division"""
    gy = np.asarray(gy)
    assert gy.dtype == np.float32
    return (gy / np.array(LR.SCALE, np.float32).reshape(1, 3, 1, 1)).astype(np.float32)


def pictures(P, size, seed):
    """smooth random pictures in [-1, 1], float32 [P, 3, size, size]"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(P, 3, 5, 5, generator=g) * 2 - 1
    return (0.8 * F.interpolate(low, size=(size, size), mode='bilinear', align_corners=False)
            + 0.2 * (torch.rand(P, 3, size, size, generator=g) * 2 - 1)).clamp(-1, 1)


def imagenet_normalize(unit):
    """[-1, 1] pictures -> the ImageNet-normalised pictures a Trainer holds ((v - mean) / std of v in [0, 1]), in unit's dtype"""
    mean = torch.tensor(IMAGENET_MEAN, dtype=unit.dtype).view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, dtype=unit.dtype).view(1, 3, 1, 1)
    return ((unit * 0.5 + 0.5) - mean) / std


def loss_ref(sd, lins, x, y, dtype, input='imagenet'):
    """the whole loss in ``dtype``: mean over the batch of the VGG-16 LPIPS distance of x to the detached y -> (value, d value / d x).
    ``input``: 'imagenet' (x, y feed the backbone as they are) or 'unit' ([-1, 1] pictures through the scaling layer)"""
    a = x.detach().to(dtype).clone().requires_grad_(True)
    b = y.detach().to(dtype)
    xa, xb = (LR.input_ref(a), LR.input_ref(b)) if input == 'unit' else (a, b)
    ta = LR.vgg16_taps(sd, xa)
    with torch.no_grad():
        tb = LR.vgg16_taps(sd, xb)
    total = torch.zeros(a.size(0), dtype=dtype)
    for k in range(5):
        total = total + LR.layer_ref(ta[k], tb[k], None if lins is None else lins[k])
    value = total.mean()
    value.backward()
    return value.detach(), a.grad
