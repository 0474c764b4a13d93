"""Plain-torch restatements of what scene_generation_amd/lpips.py computes, shared by tests/test_lpips_cpu.py, tests/test_gpu_lpips.py
and tools/bench_lpips.py: the two backbones (F.conv2d, F.max_pool2d), the scaling layer (torch and NumPy float32), one tap of the
distance and the whole distance.  They run on the CPU in float64 and float32; nothing here touches the library."""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10
# (torchvision features index, cin, cout, kernel, stride, pad, MaxPool2d(3, 2) in front)
ALEX = ((0, 3, 64, 11, 4, 2, False), (3, 64, 192, 5, 1, 2, True), (6, 192, 384, 3, 1, 1, True), (8, 384, 256, 3, 1, 1, False),
        (10, 256, 256, 3, 1, 1, False))
VGG16_CFG = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512)
VGG16_TAPS = (3, 8, 15, 22, 29)                                  # the ReLUs relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
CHANNELS = {'alex': (64, 192, 384, 256, 256), 'vgg': (64, 128, 256, 512, 512)}


def vgg16_convs():
    """[(torchvision features index, cin, cout)] of the 13 convs"""
    out, cin, idx = [], 3, 0
    for v in VGG16_CFG:
        if v == 'M':
            idx += 1
        else:
            out.append((idx, cin, v))
            cin, idx = v, idx + 2
    return out


def random_backbone(net, seed):
    """a torchvision-keyed float32 state_dict (features.<i>.weight|bias) with He-scaled weights, plus classifier entries a loader
    has to ignore"""
    g = torch.Generator().manual_seed(seed)
    convs = [(i, cin, cout, k) for i, cin, cout, k, _, _, _ in ALEX] if net == 'alex' else [(i, cin, cout, 3) for i, cin, cout in vgg16_convs()]
    sd = {}
    for i, cin, cout, k in convs:
        sd['features.%d.weight' % i] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        sd['features.%d.bias' % i] = torch.randn(cout, generator=g) * 0.05
    sd['classifier.1.weight'] = torch.zeros(2, 2)
    sd['classifier.1.bias'] = torch.zeros(2)
    return sd


def random_lins(net, seed):
    """five non-negative weight vectors [1, C, 1, 1], a fifth of each exactly zero (the learned ones are sparse)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for C in CHANNELS[net]:
        w = torch.rand(1, C, 1, 1, generator=g)
        w[:, ::5] = 0
        out.append(w)
    return out


def lin_state_dict(lins, form='lin'):
    """'lin': lin<k>.model.1.weight (the package's weight files); 'lins': lins.<k>.model.1.weight (a module's state_dict)"""
    fmt = 'lin%d.model.1.weight' if form == 'lin' else 'lins.%d.model.1.weight'
    return {fmt % k: w.clone() for k, w in enumerate(lins)}


def whole_module_state_dict(net, backbone, lins):
    """the state_dict of the package's LPIPS module: scaling layer buffers, the backbone under net.slice<j>.<i>.* with torchvision's
    index kept, the lins under lins.<k> and lin<k> both"""
    cuts = (2, 5, 8, 10, 12) if net == 'alex' else (4, 9, 16, 23, 30)
    sd = {'scaling_layer.shift': torch.tensor(SHIFT).view(1, 3, 1, 1), 'scaling_layer.scale': torch.tensor(SCALE).view(1, 3, 1, 1)}
    for k, v in backbone.items():
        if k.startswith('features.'):
            i = int(k.split('.')[1])
            j = 1 + sum(i >= c for c in cuts)
            sd['net.slice%d.%d.%s' % (j, i, k.split('.')[2])] = v.clone()
    sd.update(lin_state_dict(lins, 'lins'))
    sd.update(lin_state_dict(lins, 'lin'))
    return sd


def input_ref(x):
    """the scaling layer in torch: x [N, 3, H, W] float in [-1, 1] (any float dtype) -> same dtype"""
    shift = torch.tensor(SHIFT, dtype=x.dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=x.dtype).view(1, 3, 1, 1)
    return (x - shift) / scale


def input_ref_np(x):
    """the scaling layer as NumPy float32, every operation rounded on its own: x [N, 3, H, W] float32 in [-1, 1], or uint8
    (v = u / 127.5 - 1) -> float32 [N, 3, H, W]"""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        v = x.astype(np.float32) / np.float32(127.5) - np.float32(1)
    else:
        assert x.dtype == np.float32
        v = x
    shift = np.array(SHIFT, np.float32).reshape(1, 3, 1, 1)
    scale = np.array(SCALE, np.float32).reshape(1, 3, 1, 1)
    return ((v - shift) / scale).astype(np.float32)


def uint8_to_unit(u, dtype):
    """uint8 pictures [N, 3, H, W] -> [-1, 1] in ``dtype``"""
    return u.to(dtype) / 127.5 - 1


def alex_taps(sd, x):
    """the five taps of AlexNet on the scaled input ``x`` (dtype of x; ``sd`` is cast to it)"""
    taps = []
    for i, _, _, _, s, p, pool in ALEX:
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sd['features.%d.weight' % i].to(x.dtype), sd['features.%d.bias' % i].to(x.dtype), s, p))
        taps.append(x)
    return taps


def vgg16_taps(sd, x):
    taps, idx = [], 0
    for v in VGG16_CFG:
        if v == 'M':
            x = F.max_pool2d(x, 2)
            idx += 1
        else:
            x = F.relu(F.conv2d(x, sd['features.%d.weight' % idx].to(x.dtype), sd['features.%d.bias' % idx].to(x.dtype), 1, 1))
            idx += 2
            if idx - 1 in VGG16_TAPS:
                taps.append(x)
    return taps


def layer_ref(f0, f1, w=None, eps=EPS):
    """one tap: f0, f1 [P, C, ...] -> [P] in their dtype: normalise over the channels, difference, square, weight, sum over the
    channels, mean over the pixels (the direct form)"""
    P, C = f0.shape[:2]
    f0, f1 = f0.reshape(P, C, -1), f1.reshape(P, C, -1)
    n0 = f0.pow(2).sum(1, keepdim=True).sqrt()
    n1 = f1.pow(2).sum(1, keepdim=True).sqrt()
    d = (f0 / (n0 + eps) - f1 / (n1 + eps)).pow(2)
    if w is not None:
        d = d * w.to(f0.dtype).reshape(1, C, 1)
    return d.sum(1).mean(1)


def lpips_ref(net, sd, lins, x0, x1, dtype):
    """the whole distance of pairs of pictures [P, 3, H, W] in [-1, 1] -> [P] in ``dtype``; lins: five tensors or None (w = 1)"""
    P = x0.size(0)
    x = input_ref(torch.cat([x0, x1]).to(dtype))
    taps = (alex_taps if net == 'alex' else vgg16_taps)(sd, x)
    total = torch.zeros(P, dtype=dtype)
    for k, t in enumerate(taps):
        total = total + layer_ref(t[:P], t[P:], None if lins is None else lins[k])
    return total
