"""The object-accuracy classifier's own operators (csrc/classifier.hip): the padded 3x3 stride-2 max-pool and relu(a + b) as autograd
Functions, the BatchNorm fold, the SGD-momentum step and the argmax + accuracy record.  No wrapper synchronises.
(Part of scene_generation_amd.ops: see ops/__init__.py.)"""
import torch
from torch.autograd import Function

from ._core import ACT_RELU, _call, _dev, _f32, _i64, _p, _stream


class MaxPool3s2Fn(Function):
    """nn.MaxPool2d(3, stride=2, padding=1) (the stem of a torchvision ResNet); the backward recomputes the winners from x"""

    @staticmethod
    def forward(ctx, x):
        x = _f32(x, 'max-pool input')
        N, C, H, W = x.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty(N, C, OH, OW, dtype=torch.float32, device=x.device)
        _call('sg_maxpool3s2_fwd', _p(x), _p(y), N * C, H, W, OH, OW, _stream())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, = ctx.saved_tensors
        gy = _f32(gy)
        N, C, H, W = x.shape
        gx = torch.empty_like(x)
        _call('sg_maxpool3s2_bwd', _p(x), _p(gy), _p(gx), N * C, H, W, gy.size(2), gy.size(3), _stream())
        return gx


def maxpool3s2(x):
    return MaxPool3s2Fn.apply(x)


class AddReluFn(Function):
    """relu(a + b): the tail of a residual block.  One sg_act_bwd on y gives the gradient of both operands."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _f32(a, 'add_relu lhs'), _f32(b, 'add_relu rhs')
        assert a.shape == b.shape, 'add_relu: shapes %s and %s differ' % (tuple(a.shape), tuple(b.shape))
        y = torch.empty_like(a)
        _call('sg_add_relu_fwd', _p(a), _p(b), _p(y), a.numel(), _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, = ctx.saved_tensors
        gy = _f32(gy)
        g = torch.empty_like(gy)
        _call('sg_act_bwd', _p(y), _p(gy), _p(g), gy.numel(), ACT_RELU, 0.0, _stream())
        return g, g


def add_relu(a, b):
    return AddReluFn.apply(a, b)


def bn_fold(weight, gamma, beta, mean, var, eps):
    """-> (w', b') of the convolution that equals conv(weight) followed by the eval-mode BatchNorm (gamma, beta, mean, var, eps):
    s = gamma / sqrt(var + eps), w' = weight * s[co], b' = beta - mean * s"""
    weight = _f32(weight.detach(), 'conv weight')
    Cout = weight.size(0)
    vecs = [_f32(t.detach(), 'batch-norm vector') for t in (gamma, beta, mean, var)]
    if any(v.numel() != Cout for v in vecs):
        raise ValueError('bn_fold: the BatchNorm has %s channels, the convolution %d' % ([v.numel() for v in vecs], Cout))
    w_out = torch.empty_like(weight)
    b_out = torch.empty(Cout, dtype=torch.float32, device=weight.device)
    _call('sg_bn_fold', _p(weight), _p(vecs[0]), _p(vecs[1]), _p(vecs[2]), _p(vecs[3]), float(eps), _p(w_out), _p(b_out), Cout,
          weight.numel() // max(Cout, 1), _stream())
    return w_out, b_out


def sgd_momentum_step(p, g, buf, lr, momentum, first, grad_scale=1.0):
    """torch.optim.SGD(lr, momentum) over flat contiguous buffers, in place: buf = g (first) or momentum * buf + g; p -= lr * buf"""
    for t, name in ((p, 'p'), (g, 'g'), (buf, 'buf')):
        _dev(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
            raise ValueError('sgd_momentum_step: %s must be a contiguous float32 buffer of %d elements' % (name, p.numel()))
    _call('sg_sgd_momentum_step', _p(p), _p(g), _p(buf), p.numel(), float(lr), float(momentum), 1 if first else 0, float(grad_scale),
          _stream())


def new_classify_record(device):
    """a zeroed record {correct, counted, rows} (int64 [3]) for classify_stats to add to"""
    return torch.zeros(3, dtype=torch.int64, device=device)


def classify_stats(logits, target, ignore_label=-1, acc=None, want_preds=False):
    """acc [3] int64 += {rows whose argmax equals their target, rows whose target != ignore_label, rows} of logits [rows, classes]
    against target [rows] int64 (a row whose target is ``ignore_label`` is neither counted nor correct; -1 counts every row).
    -> (acc, preds [rows] int64 or None); preds = torch.max(logits, 1)[1]."""
    logits, target = _f32(logits, 'logits'), _i64(target, 'target')
    if logits.dim() != 2 or target.dim() != 1 or target.numel() != logits.size(0) or logits.size(1) < 1:
        raise ValueError('classify_stats: logits [rows, classes >= 1] and target [rows], got %s and %s'
                         % (tuple(logits.shape), tuple(target.shape)))
    if acc is None:
        acc = new_classify_record(logits.device)
    else:
        _dev(acc, 'acc')
        if acc.dtype != torch.int64 or tuple(acc.shape) != (3,) or not acc.is_contiguous():
            raise ValueError('acc must be a contiguous int64 tensor of shape (3,)')
    preds = torch.empty(logits.size(0), dtype=torch.int64, device=logits.device) if want_preds else None
    _call('sg_classify_stats', _p(logits), _p(target), logits.size(0), logits.size(1), int(ignore_label), _p(preds), _p(acc), _stream())
    return acc, preds
