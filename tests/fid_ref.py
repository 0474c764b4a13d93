"""Plain restatements for the FID tests: NumPy forms of the two branch pools, the raw moments, the covariance and the exact
nuclear-norm form of the Frechet distance, and the FID form of Inception-v3 (pytorch-fid's FIDInceptionA / C / E_1 / E_2) in
torch.nn.functional on top of tests/inception_ref.py.  The tree only."""
import numpy as np
import torch
import torch.nn.functional as F

import inception_ref as R


# ---- pools ----------------------------------------------------------------------------------------------------------------------------
def avgpool3s1x_ref(x):
    """avg_pool2d(3, stride=1, padding=1, count_include_pad=False) on [..., H, W] in the array's precision, taps in (kh, kw) order"""
    return R.avgpool3s1_ref(x, count_include_pad=False)


def maxpool3s1_ref(x):
    """max_pool2d(3, stride=1, padding=1) on [..., H, W]: the padding is -inf, a NaN in a window wins"""
    H, W = x.shape[-2:]
    pad = np.full(x.shape[:-2] + (H + 2, W + 2), -np.inf, x.dtype)
    pad[..., 1:-1, 1:-1] = x
    return np.max(np.stack([pad[..., kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)]), axis=0)      # np.max propagates NaN


# ---- moments --------------------------------------------------------------------------------------------------------------------------
def relu_gauss(rs, n, d):
    """ReLU-ed Gaussian float32 features with a per-column offset and scale: non-negative, many exact zeros, correlated columns"""
    base = rs.randn(n, d) * (0.5 + rs.rand(d)) + 0.3 * rs.randn(d) + 0.5 * rs.randn(n, 1)
    return np.maximum(base, 0.0).astype(np.float32)


def int_moments(x):
    """(sum, outer) of integer-valued rows, exactly, in int64"""
    xi = np.asarray(x).astype(np.int64)
    assert np.array_equal(xi, np.asarray(x))
    return xi.sum(0), xi.T @ xi


def float_moments(x):
    """(sum, outer, sum of |x|, sum of |x_i||x_j|) in float64 (the products of float32 values are exact in float64)"""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    return x.sum(0), x.T @ x, a.sum(0), a.T @ a


# ---- the distance ---------------------------------------------------------------------------------------------------------------------
def fid_nuclear(f1, f2):
    """the Frechet distance of two feature sets [n, D], float64, with the trace term in its exact rank-revealing form:
    tr (S1 S2)^1/2 = |A_c B_c^T|_* / sqrt((n1 - 1)(n2 - 1)) with A_c, B_c the centred rows (the nonzero eigenvalues of S1 S2 are
    the squared singular values of A_c B_c^T over (n1 - 1)(n2 - 1)).  -> (fid, tr S1 + tr S2)"""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    n1, n2 = f1.shape[0], f2.shape[0]
    mu1, mu2 = f1.mean(0), f2.mean(0)
    a, b = f1 - mu1, f2 - mu2
    tr = float((a * a).sum() / (n1 - 1) + (b * b).sum() / (n2 - 1))
    nuc = float(np.linalg.svd(a @ b.T, compute_uv=False).sum()) / np.sqrt((n1 - 1.0) * (n2 - 1.0))
    d = mu1 - mu2
    return float(d @ d) + tr - 2.0 * nuc, tr


def stats(f):
    f = np.asarray(f, np.float64)
    return f.mean(0), np.cov(f, rowvar=False)


# ---- the FID form of the network ------------------------------------------------------------------------------------------------------
def _avgx(x):
    return F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)


def _max1(x):
    return F.max_pool2d(x, 3, stride=1, padding=1)


class FidA(R.RefA):
    def forward(self, x):
        return torch.cat([self.branch1x1(x), self.branch5x5_2(self.branch5x5_1(x)),
                          self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))), self.branch_pool(_avgx(x))], 1)


class FidC(R.RefC):
    def forward(self, x):
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_5(self.branch7x7dbl_4(self.branch7x7dbl_3(self.branch7x7dbl_2(self.branch7x7dbl_1(x)))))
        return torch.cat([self.branch1x1(x), b7, bd, self.branch_pool(_avgx(x))], 1)


class FidE(R.RefE):
    pool = staticmethod(_avgx)

    def forward(self, x):
        t = self.branch3x3_1(x)
        b3 = torch.cat([self.branch3x3_2a(t), self.branch3x3_2b(t)], 1)
        t = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        bd = torch.cat([self.branch3x3dbl_3a(t), self.branch3x3dbl_3b(t)], 1)
        return torch.cat([self.branch1x1(x), b3, bd, self.branch_pool(self.pool(x))], 1)


class FidE2(FidE):
    pool = staticmethod(_max1)


class RefFidInception3(R.RefInception3):
    """pytorch-fid's network: torchvision's layout with 1008 classes, no auxiliary head, and four kinds of branch pool changed"""

    def __init__(self, num_classes=1008):
        super().__init__(num_classes=num_classes, aux_logits=False)
        self.Mixed_5b, self.Mixed_5c, self.Mixed_5d = FidA(192, 32), FidA(256, 64), FidA(288, 64)
        self.Mixed_6b, self.Mixed_6c, self.Mixed_6d, self.Mixed_6e = FidC(768, 128), FidC(768, 160), FidC(768, 160), FidC(768, 192)
        self.Mixed_7b, self.Mixed_7c = FidE(1280), FidE2(2048)
