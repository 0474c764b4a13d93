"""Plain restatements for the Inception-score tests: torchvision's Inception-v3 layout in torch.nn / torch.nn.functional (run on the
CPU in float64 and float32), and NumPy forms of the pools, the resize, the softmax and the score.  The tree only."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class RefConv(nn.Module):
    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class RefA(nn.Module):
    def __init__(self, cin, pf):
        super().__init__()
        self.branch1x1 = RefConv(cin, 64, kernel_size=1)
        self.branch5x5_1 = RefConv(cin, 48, kernel_size=1)
        self.branch5x5_2 = RefConv(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = RefConv(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = RefConv(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = RefConv(96, 96, kernel_size=3, padding=1)
        self.branch_pool = RefConv(cin, pf, kernel_size=1)

    def forward(self, x):
        return torch.cat([self.branch1x1(x), self.branch5x5_2(self.branch5x5_1(x)),
                          self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          self.branch_pool(F.avg_pool2d(x, 3, stride=1, padding=1))], 1)


class RefB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = RefConv(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = RefConv(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = RefConv(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = RefConv(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        return torch.cat([self.branch3x3(x), self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          F.max_pool2d(x, 3, stride=2)], 1)


class RefC(nn.Module):
    def __init__(self, cin, c7):
        super().__init__()
        self.branch1x1 = RefConv(cin, 192, kernel_size=1)
        self.branch7x7_1 = RefConv(cin, c7, kernel_size=1)
        self.branch7x7_2 = RefConv(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = RefConv(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = RefConv(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = RefConv(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = RefConv(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = RefConv(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = RefConv(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = RefConv(cin, 192, kernel_size=1)

    def forward(self, x):
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_5(self.branch7x7dbl_4(self.branch7x7dbl_3(self.branch7x7dbl_2(self.branch7x7dbl_1(x)))))
        return torch.cat([self.branch1x1(x), b7, bd, self.branch_pool(F.avg_pool2d(x, 3, stride=1, padding=1))], 1)


class RefD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = RefConv(cin, 192, kernel_size=1)
        self.branch3x3_2 = RefConv(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = RefConv(cin, 192, kernel_size=1)
        self.branch7x7x3_2 = RefConv(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = RefConv(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = RefConv(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([self.branch3x3_2(self.branch3x3_1(x)), b7, F.max_pool2d(x, 3, stride=2)], 1)


class RefE(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch1x1 = RefConv(cin, 320, kernel_size=1)
        self.branch3x3_1 = RefConv(cin, 384, kernel_size=1)
        self.branch3x3_2a = RefConv(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = RefConv(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = RefConv(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = RefConv(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = RefConv(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = RefConv(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = RefConv(cin, 192, kernel_size=1)

    def forward(self, x):
        t = self.branch3x3_1(x)
        b3 = torch.cat([self.branch3x3_2a(t), self.branch3x3_2b(t)], 1)
        t = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        bd = torch.cat([self.branch3x3dbl_3a(t), self.branch3x3dbl_3b(t)], 1)
        return torch.cat([self.branch1x1(x), b3, bd, self.branch_pool(F.avg_pool2d(x, 3, stride=1, padding=1))], 1)


class RefAux(nn.Module):
    def __init__(self, cin, num_classes):
        super().__init__()
        self.conv0 = RefConv(cin, 128, kernel_size=1)
        self.conv1 = RefConv(128, 768, kernel_size=5)
        self.fc = nn.Linear(768, num_classes)


class RefInception3(nn.Module):
    """Inception-v3 as the issue's table spells it out; eval-mode forward without the auxiliary head and without transform_input"""

    def __init__(self, num_classes=1000, aux_logits=True):
        super().__init__()
        self.Conv2d_1a_3x3 = RefConv(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = RefConv(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = RefConv(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = RefConv(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = RefConv(80, 192, kernel_size=3)
        self.Mixed_5b = RefA(192, 32)
        self.Mixed_5c = RefA(256, 64)
        self.Mixed_5d = RefA(288, 64)
        self.Mixed_6a = RefB(288)
        self.Mixed_6b = RefC(768, 128)
        self.Mixed_6c = RefC(768, 160)
        self.Mixed_6d = RefC(768, 160)
        self.Mixed_6e = RefC(768, 192)
        if aux_logits:
            self.AuxLogits = RefAux(768, num_classes)
        self.Mixed_7a = RefD(768)
        self.Mixed_7b = RefE(1280)
        self.Mixed_7c = RefE(2048)
        self.fc = nn.Linear(2048, num_classes)

    def features(self, x):
        x = self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(self.Conv2d_1a_3x3(x)))
        x = F.max_pool2d(x, 3, stride=2)
        x = self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(x))
        x = F.max_pool2d(x, 3, stride=2)
        for name in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e', 'Mixed_7a',
                     'Mixed_7b', 'Mixed_7c'):
            x = getattr(self, name)(x)
        return x.mean((2, 3))

    def forward(self, x):
        return self.fc(self.features(x))


def randomise(net, seed):
    """seeded He-scaled conv weights and randomised BatchNorm statistics and affine terms (so that a fold has something to fold)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
            elif isinstance(m, nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (1.0 / m.in_features) ** 0.5)
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    return net


# ---- NumPy restatements ---------------------------------------------------------------------------------------------------------------
def maxpool3s2v_ref(x):
    """max_pool2d(3, stride=2) without padding on [..., H, W]; a NaN in a window wins"""
    H, W = x.shape[-2:]
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    wins = np.stack([x[..., kh:kh + 2 * OH - 1:2, kw:kw + 2 * OW - 1:2] for kh in range(3) for kw in range(3)])
    return np.max(wins, axis=0)               # np.max propagates NaN


def avgpool3s1_ref(x, count_include_pad=True):
    """avg_pool2d(3, stride=1, padding=1) on [..., H, W] in the array's precision, taps added in (kh, kw) order"""
    H, W = x.shape[-2:]
    pad = np.zeros(x.shape[:-2] + (H + 2, W + 2), x.dtype)
    pad[..., 1:-1, 1:-1] = x
    ones = np.zeros((H + 2, W + 2), x.dtype)
    ones[1:-1, 1:-1] = 1
    s, cnt = np.zeros_like(x), np.zeros((H, W), x.dtype)
    for kh in range(3):
        for kw in range(3):
            s = s + pad[..., kh:kh + H, kw:kw + W]
            cnt = cnt + ones[kh:kh + H, kw:kw + W]
    return s / (np.array(9, x.dtype) if count_include_pad else cnt)


def _axis(out, inp):
    src = np.maximum((np.arange(out, dtype=np.float64) + 0.5) * (inp / out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), inp - 1)
    i1 = np.minimum(i0 + 1, inp - 1)
    return i0, i1, src - i0


def resize_bilinear_ref(x, OH, OW):
    """F.interpolate(mode='bilinear', align_corners=False) on [..., H, W] in float64"""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    h0, h1, lh = _axis(OH, H)
    w0, w1, lw = _axis(OW, W)
    top = x[..., h0, :][..., :, w0] * (1 - lw) + x[..., h0, :][..., :, w1] * lw
    bot = x[..., h1, :][..., :, w0] * (1 - lw) + x[..., h1, :][..., :, w1] * lw
    return top * (1 - lh)[:, None] + bot * lh[:, None]


def softmax_ref(logits):
    z = np.asarray(logits, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _entropy(pk, qk):
    """scipy.stats.entropy(pk, qk): both normalised to sum 1, sum pk log(pk / qk) with 0 log 0 = 0"""
    pk = np.asarray(pk, np.float64)
    qk = np.asarray(qk, np.float64)
    pk, qk = pk / pk.sum(), qk / qk.sum()
    nz = pk > 0
    with np.errstate(divide='ignore'):
        return float(np.sum(pk[nz] * np.log(pk[nz] / qk[nz])))


def inception_score_ref(preds, splits, entropy=_entropy):
    """scripts/inception_score.py:48-62 -> (mean, std, [split scores]); ``entropy``: the KL function (scipy's in the cross-check)"""
    preds = np.asarray(preds, np.float64)
    n = preds.shape[0]
    per = n // splits
    scores = []
    with np.errstate(invalid='ignore', divide='ignore'), __import__('warnings').catch_warnings():
        __import__('warnings').simplefilter('ignore')
        for k in range(splits):
            part = preds[k * per:(k + 1) * per]
            py = np.mean(part, axis=0)
            kl = [entropy(part[i], py) for i in range(part.shape[0])]
            scores.append(np.exp(np.mean(kl)))
        return float(np.mean(scores)), float(np.std(scores)), [float(s) for s in scores]
