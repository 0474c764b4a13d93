"""Yardsticks of the accuracy-network tests: a plain torch.nn restatement of the ResNet layout (run on the CPU, in float64 for the
reference and in float32 for the error yardstick), and NumPy restatements of the padded max-pool with its backward tie rule, the
SGD-momentum step with separately rounded operations, relu(a + b), the BatchNorm fold and the classify record.  Nothing here
imports the code under test."""
import numpy as np
import torch
import torch.nn as nn

CONFIGS = {'resnet18': ('basic', (2, 2, 2, 2)), 'resnet34': ('basic', (3, 4, 6, 3)), 'resnet50': ('bottleneck', (3, 4, 6, 3)),
           'resnet101': ('bottleneck', (3, 4, 23, 3)), 'resnet152': ('bottleneck', (3, 8, 36, 3))}


def _c(cin, cout, k, stride=1):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False)


class RefBasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1, self.bn1 = _c(inplanes, planes, 3, stride), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = _c(planes, planes, 3), nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        out = torch.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return torch.relu(out + (x if self.downsample is None else self.downsample(x)))


class RefBottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1, self.bn1 = _c(inplanes, planes, 1), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = _c(planes, planes, 3, stride), nn.BatchNorm2d(planes)
        self.conv3, self.bn3 = _c(planes, planes * 4, 1), nn.BatchNorm2d(planes * 4)
        self.downsample = downsample

    def forward(self, x):
        out = torch.relu(self.bn1(self.conv1(x)))
        out = torch.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return torch.relu(out + (x if self.downsample is None else self.downsample(x)))


def ref_downsample(inplanes, outplanes, stride):
    return nn.Sequential(_c(inplanes, outplanes, 1, stride), nn.BatchNorm2d(outplanes))


class RefResNet(nn.Module):
    def __init__(self, name, num_classes=1000):
        super().__init__()
        kind, sizes = CONFIGS[name]
        block = RefBasicBlock if kind == 'basic' else RefBottleneck
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        inplanes = 64
        for li, (planes, n) in enumerate(zip((64, 128, 256, 512), sizes)):
            stride = 1 if li == 0 else 2
            ds = ref_downsample(inplanes, planes * block.expansion, stride) if (stride != 1 or inplanes != planes * block.expansion) else None
            mods = [block(inplanes, planes, stride, ds)]
            inplanes = planes * block.expansion
            mods += [block(inplanes, planes) for _ in range(1, n)]
            setattr(self, 'layer%d' % (li + 1), nn.Sequential(*mods))
        self.fc = nn.Linear(inplanes, num_classes)

    def forward(self, x):
        x = self.maxpool(torch.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(x.mean((2, 3)))


# ---- nn.MaxPool2d(3, stride=2, padding=1) -----------------------------------------------------------------------------------------
def _pool_winners(x):
    """x [NC, H, W] -> (max [NC, OH, OW], flat index of the winner [NC, OH, OW]): torch's scan over the part of the window inside
    the plane, from -inf, taking a value that is greater than the running maximum or a NaN (first maximum, last NaN)"""
    NC, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    best = np.full((NC, OH, OW), -np.inf, x.dtype)
    at = np.zeros((NC, OH, OW), np.int64)
    for oh in range(OH):
        for ow in range(OW):
            m = np.full(NC, -np.inf, x.dtype)
            a = None
            for h in range(max(2 * oh - 1, 0), min(2 * oh + 2, H)):
                for w in range(max(2 * ow - 1, 0), min(2 * ow + 2, W)):
                    v = x[:, h, w]
                    if a is None:
                        a = np.full(NC, h * W + w, np.int64)
                    take = (v > m) | np.isnan(v)
                    m = np.where(take, v, m)
                    a = np.where(take, h * W + w, a)
            best[:, oh, ow], at[:, oh, ow] = m, a
    return best, at


def maxpool3s2_ref(x):
    return _pool_winners(x)[0]


def maxpool3s2_bwd_ref(x, gy):
    """gx [NC, H, W]: every window's gradient goes to its winner; a pixel's sum runs over its windows in (oh, ow) order, in fp32"""
    NC, H, W = x.shape
    _, at = _pool_winners(x)
    gx = np.zeros((NC, H * W), np.float32)
    rows = np.arange(NC)
    for oh in range(at.shape[1]):
        for ow in range(at.shape[2]):
            gx[rows, at[:, oh, ow]] = (gx[rows, at[:, oh, ow]] + gy[:, oh, ow]).astype(np.float32)
    return gx.reshape(NC, H, W)


def add_relu_ref(a, b):
    s = (a + b).astype(np.float32)
    return np.where((s > 0) | np.isnan(s), s, np.float32(0)).astype(np.float32)


def bn_fold_ref(w, gamma, beta, mean, var, eps):
    """float64: (w * s[co], beta - mean * s), s = gamma / sqrt(var + eps), from the fp32 operands (eps as the fp32 the kernel gets)"""
    w, gamma, beta, mean, var = [np.asarray(t, np.float64) for t in (w, gamma, beta, mean, var)]
    s = gamma / np.sqrt(var + np.float64(np.float32(eps)))
    return w * s.reshape((-1,) + (1,) * (w.ndim - 1)), beta - mean * s


def sgd_ref(p, g, buf, lr, momentum, first, grad_scale=1.0):
    """one torch.optim.SGD(lr, momentum) step in fp32 with every product and sum rounded on its own -> (p, buf)"""
    f = np.float32
    gs = (g * f(grad_scale)).astype(f)
    if first:
        nb = gs.copy()
    else:
        nb = ((f(momentum) * buf).astype(f) + gs).astype(f)
    return (p - (f(lr) * nb).astype(f)).astype(f), nb


def classify_ref(logits, target, ignore_label):
    """-> (preds [rows]: the first index of the maximum, a NaN counting as the maximum; (correct, counted, rows))"""
    rows = logits.shape[0]
    preds = np.zeros(rows, np.int64)
    for r in range(rows):
        row = logits[r]
        nan = np.flatnonzero(np.isnan(row))
        preds[r] = nan[0] if nan.size else int(np.flatnonzero(row == row.max())[0])
    counted = target != ignore_label
    return preds, (int((counted & (preds == target)).sum()), int(counted.sum()), rows)
