"""The Inception score: the reference's last evaluation figure (scripts/inception_score.py, train.py:177-225) on this stack.

    python -m scene_generation_amd.inception --dir DIR --weights PATH [--splits 5] [--batch_size 32]     -> mean and std
                                             [--image_size H,W [--resize_filter bilinear|bicubic]] [--save_probs OUT.npy]

* ``InceptionV3``: torchvision's Inception-v3 (``inception_v3(transform_input=False)``) with its ``state_dict`` keys and shapes, so
  the published ``inception_v3_google-*.pth`` loads with ``strict=True``.  Inference only: every conv + BatchNorm + ReLU is ONE
  sg_conv2d_rect_fwd launch (the BatchNorm folded into weights and bias by sg_bn_fold, cached), and every branch of a block writes
  straight into its channel slice of the block's output -- no concatenation, no BatchNorm pass.  The auxiliary head exists so the
  file loads and never runs.
* ``InceptionScore``: the reference's object -- ``clean()``, ``__call__(imgs)``, ``compute_score(splits) -> (mean, std)`` -- that
  ``evaluate.check_model`` and ``Trainer`` drive.  Softmax rows accumulate in a device buffer that grows by doubling; ``__call__``
  never synchronises, ``compute_score`` does the one host read.  ``rows()`` is the view of the rows ``isinf.ISInfinity`` works on.
* ``inception_network`` / ``pooled_features``: what the score, ``fid`` and ``featsets`` share -- the network a ``weights`` argument
  stands for, and the chunk / resize / ``features`` loop.  File, image and buffer helpers live in ``evalkit``, directory feeding in
  ``imageprep``.
* Nothing is ever downloaded: ``weights`` is a local ``state_dict`` file; without it the network keeps a seeded random
  initialisation and says loudly that the score is then meaningless.
"""
import argparse
import sys

import torch
import torch.nn as nn

from . import layers, ops
from .evalkit import find_images, read_image      # noqa: F401 (importable from here as well: the command line's helpers)
from .evalkit import FoldCache, folded, grow_rows, state_dict_of
from .imageprep import _feed_dir, add_arguments

__all__ = ['InceptionV3', 'InceptionScore', 'load_inception', 'conv_units', 'main', 'DEFAULT_WEIGHTS']

# the state_dict file ``InceptionScore(weights=None)`` loads: for callers whose constructor call cannot be changed (the reference's
# train.py:177); None: random weights and a warning
DEFAULT_WEIGHTS = None
FID_CLASSES = 1008          # the class count of the TF-ported FID weights: what ``load_inception`` recognises them by


class BasicConv2d(nn.Module):
    """conv (no bias) + BatchNorm(eps=0.001) + ReLU; holds the parameters under torchvision's names, runs as one folded launch"""

    def __init__(self, cin, cout, kernel_size, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)
        self.name = ''

    def forward(self, x):
        raise NotImplementedError('a BasicConv2d runs through InceptionV3.forward (one folded launch per unit)')


# ---- two executors of the same network walk: the kernels, and a shape trace (the list of conv units with their geometry) ----------
class _Kernels(object):
    def __init__(self, fold):
        self.fold = fold

    @staticmethod
    def shape(x):
        return tuple(x.shape)

    @staticmethod
    def alloc(x, C, H, W):
        return torch.empty(x.size(0), C, H, W, dtype=torch.float32, device=x.device)

    def conv(self, unit, x, out=None, c0=0):
        w, b = folded(unit.conv, unit.bn, self.fold)
        return ops.conv2d_rect(x, w, b, stride=unit.conv.stride[0], pad=unit.conv.padding, act=ops.ACT_RELU, out=out, out_c0=c0)

    @staticmethod
    def maxpool(x, out=None, c0=0):
        return ops.maxpool3s2v(x, out, c0)

    @staticmethod
    def avgpool(x):
        return ops.avgpool3s1(x)

    @staticmethod
    def avgpool3s1x(x):
        return ops.avgpool3s1x(x)

    @staticmethod
    def maxpool3s1(x):
        return ops.maxpool3s1(x)


class _Trace(object):
    """tensors are (N, C, H, W) tuples; ``units`` collects one record per conv unit in launch order"""

    def __init__(self):
        self.units = []

    @staticmethod
    def shape(x):
        return x

    @staticmethod
    def alloc(x, C, H, W):
        return (x[0], C, H, W)

    def conv(self, unit, x, out=None, c0=0):
        N, C, H, W = x
        c = unit.conv
        (kh, kw), (ph, pw), s = c.kernel_size, c.padding, c.stride[0]
        assert C == c.in_channels, (unit.name, C, c.in_channels)
        oh, ow = ops.conv_out_size(H, kh, s, ph), ops.conv_out_size(W, kw, s, pw)
        ctot = c.out_channels if out is None else out[1]
        assert out is None or (out[2], out[3]) == (oh, ow), (unit.name, out, oh, ow)
        self.units.append(dict(name=unit.name, N=N, C=C, H=H, W=W, Cout=c.out_channels, KH=kh, KW=kw, stride=s, padH=ph, padW=pw,
                               OH=oh, OW=ow, out_c0=c0, out_ctot=ctot))
        return (N, c.out_channels, oh, ow) if out is None else out

    @staticmethod
    def maxpool(x, out=None, c0=0):
        N, C, H, W = x
        return (N, C, (H - 3) // 2 + 1, (W - 3) // 2 + 1) if out is None else out

    @staticmethod
    def avgpool(x):
        return x

    avgpool3s1x = maxpool3s1 = avgpool          # the FID form's branch pools keep the plane too


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, 1)
        self.branch5x5_1 = BasicConv2d(cin, 48, 1)
        self.branch5x5_2 = BasicConv2d(48, 64, 5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, 1)
        self.cout = 64 + 64 + 96 + pool_features
        self.pool = 'avgpool'               # the executor's branch pool; InceptionV3(fid_variant=True) changes it

    def run(self, E, x):
        _, _, H, W = E.shape(x)
        out = E.alloc(x, self.cout, H, W)
        E.conv(self.branch1x1, x, out, 0)
        E.conv(self.branch5x5_2, E.conv(self.branch5x5_1, x), out, 64)
        E.conv(self.branch3x3dbl_3, E.conv(self.branch3x3dbl_2, E.conv(self.branch3x3dbl_1, x)), out, 128)
        E.conv(self.branch_pool, getattr(E, self.pool)(x), out, 224)
        return out


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, 3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, stride=2)
        self.cout = 384 + 96 + cin

    def run(self, E, x):
        _, _, H, W = E.shape(x)
        out = E.alloc(x, self.cout, (H - 3) // 2 + 1, (W - 3) // 2 + 1)
        E.conv(self.branch3x3, x, out, 0)
        E.conv(self.branch3x3dbl_3, E.conv(self.branch3x3dbl_2, E.conv(self.branch3x3dbl_1, x)), out, 384)
        E.maxpool(x, out, 480)
        return out


class InceptionC(nn.Module):
    def __init__(self, cin, channels_7x7):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(cin, 192, 1)
        self.branch7x7_1 = BasicConv2d(cin, c7, 1)
        self.branch7x7_2 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, (7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, 1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, (1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, 1)
        self.cout = 768
        self.pool = 'avgpool'               # the executor's branch pool; InceptionV3(fid_variant=True) changes it

    def run(self, E, x):
        _, _, H, W = E.shape(x)
        out = E.alloc(x, self.cout, H, W)
        E.conv(self.branch1x1, x, out, 0)
        E.conv(self.branch7x7_3, E.conv(self.branch7x7_2, E.conv(self.branch7x7_1, x)), out, 192)
        t = E.conv(self.branch7x7dbl_3, E.conv(self.branch7x7dbl_2, E.conv(self.branch7x7dbl_1, x)))
        E.conv(self.branch7x7dbl_5, E.conv(self.branch7x7dbl_4, t), out, 384)
        E.conv(self.branch_pool, getattr(E, self.pool)(x), out, 576)
        return out


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, 1)
        self.branch3x3_2 = BasicConv2d(192, 320, 3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, 1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, (1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, (7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, 3, stride=2)
        self.cout = 320 + 192 + cin

    def run(self, E, x):
        _, _, H, W = E.shape(x)
        out = E.alloc(x, self.cout, (H - 3) // 2 + 1, (W - 3) // 2 + 1)
        E.conv(self.branch3x3_2, E.conv(self.branch3x3_1, x), out, 0)
        t = E.conv(self.branch7x7x3_3, E.conv(self.branch7x7x3_2, E.conv(self.branch7x7x3_1, x)))
        E.conv(self.branch7x7x3_4, t, out, 320)
        E.maxpool(x, out, 512)
        return out


class InceptionE(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 320, 1)
        self.branch3x3_1 = BasicConv2d(cin, 384, 1)
        self.branch3x3_2a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, 1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, 3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, 1)
        self.cout = 2048
        self.pool = 'avgpool'               # the executor's branch pool; InceptionV3(fid_variant=True) changes it

    def run(self, E, x):
        _, _, H, W = E.shape(x)
        out = E.alloc(x, self.cout, H, W)
        E.conv(self.branch1x1, x, out, 0)
        t = E.conv(self.branch3x3_1, x)
        E.conv(self.branch3x3_2a, t, out, 320)
        E.conv(self.branch3x3_2b, t, out, 704)
        t = E.conv(self.branch3x3dbl_2, E.conv(self.branch3x3dbl_1, x))
        E.conv(self.branch3x3dbl_3a, t, out, 1088)
        E.conv(self.branch3x3dbl_3b, t, out, 1472)
        E.conv(self.branch_pool, getattr(E, self.pool)(x), out, 1856)
        return out


class InceptionAux(nn.Module):
    """the auxiliary classifier of the training recipe: parameters only (the published file holds them); never run"""

    def __init__(self, cin, num_classes):
        super().__init__()
        self.conv0 = BasicConv2d(cin, 128, 1)
        self.conv1 = BasicConv2d(128, 768, 5)
        self.fc = nn.Linear(768, num_classes)

    def forward(self, x):
        raise NotImplementedError('the auxiliary head of Inception-v3 is a training device; this network is inference only')


_BLOCKS = ('Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6a', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e', 'Mixed_7a', 'Mixed_7b',
           'Mixed_7c')


class InceptionV3(FoldCache):
    """torchvision.models.Inception3(num_classes, aux_logits, transform_input=False), inference only.

    ``forward(x)`` -> logits [N, num_classes]; ``features(x)`` -> the pooled [N, 2048] vector (where an FID would start).  Both run
    under ``no_grad`` on the running statistics; ``train(True)`` raises.  Inputs of any size from 75 x 75 up (299 is the
    network's own).  The folded weights are cached; the cache is dropped by ``load_state_dict()``, ``.to()`` / ``.cuda()`` and
    ``drop_fold()``, and an entry is rebuilt when one of its tensors was replaced or written through torch (version counters).

    Random initialisation: He-normal convolutions (fan-in), BatchNorm at identity -- torchvision's truncated normal of fixed
    std 0.1 is a starting point for TRAINING under batch statistics and overflows in eval mode.

    ``fid_variant=True`` is the form every published FID is computed with (the TF-ported pt_inception-2015-12-05 weights: 1008
    classes, no auxiliary head): the branch pools of InceptionA, InceptionC and Mixed_7b average over the taps INSIDE the plane
    (count_include_pad=False) and the branch pool of Mixed_7c is a max-pool.  Nothing else changes; the default is torchvision's."""

    def __init__(self, num_classes=1000, aux_logits=True, fid_variant=False):
        super().__init__()
        self.fid_variant = bool(fid_variant)
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, 3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, 3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, 3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, 1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, 3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        if aux_logits:
            self.AuxLogits = InceptionAux(768, num_classes)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)
        self.avgpool = layers.GlobalAvgPool()
        self.fc = layers.Linear(2048, num_classes)
        if self.fid_variant:                # pytorch-fid's FIDInceptionA / C / E_1 and E_2: four kinds of branch pool, nothing else
            for name in _BLOCKS:
                if hasattr(getattr(self, name), 'pool'):
                    getattr(self, name).pool = 'maxpool3s1' if name == 'Mixed_7c' else 'avgpool3s1x'
        for name, m in self.named_modules():
            if isinstance(m, BasicConv2d):
                m.name = name
                nn.init.kaiming_normal_(m.conv.weight, mode='fan_in', nonlinearity='relu')
        super().train(False)

    # ---- inference only -----------------------------------------------------------------------------------------------------------
    def train(self, mode=True):
        if mode:
            raise NotImplementedError('InceptionV3 is inference only (folded BatchNorm, no backward, no auxiliary head): train(True) '
                                      'is not available')
        return super().train(False)

    def _walk(self, E, x):
        """the network up to the 8 x 8 x 2048 grid, on executor ``E``"""
        x = E.conv(self.Conv2d_1a_3x3, x)
        x = E.conv(self.Conv2d_2a_3x3, x)
        x = E.conv(self.Conv2d_2b_3x3, x)
        x = E.maxpool(x)
        x = E.conv(self.Conv2d_3b_1x1, x)
        x = E.conv(self.Conv2d_4a_3x3, x)
        x = E.maxpool(x)
        for name in _BLOCKS:
            x = getattr(self, name).run(E, x)
        return x

    def features(self, x):
        if x.dim() != 4 or x.size(1) != 3 or min(x.shape[2:]) < 75:
            raise ValueError('InceptionV3: input [N, 3, H >= 75, W >= 75], got %s' % (tuple(x.shape),))
        with torch.no_grad():
            return self.avgpool(self._walk(_Kernels(self._fold_cache), x)).flatten(1)

    def forward(self, x):
        with torch.no_grad():
            return self.fc(self.features(x))


def conv_units(size=299, n=1, net=None):
    """the conv units ``InceptionV3.forward`` launches on an n x 3 x size x size input, in launch order: one dict per unit with its
    name and the fields of its sgRectDesc (94 units; the two of the auxiliary head never run)"""
    net = net if net is not None else _skeleton()
    tr = _Trace()
    net._walk(tr, (n, 3, size, size))
    return tr.units


_SKELETON = []


def _skeleton():
    """a network built once on the meta device (shapes only, no storage) for ``conv_units``"""
    if not _SKELETON:
        with torch.device('meta'):
            _SKELETON.append(InceptionV3())
    return _SKELETON[0]


def unit_plan(u, w_aligned16=True):
    """the launch plan (ops.conv2d_rect_plan) of one ``conv_units`` record"""
    d = ops.rect_desc(u['N'], u['C'], u['H'], u['W'], u['Cout'], u['KH'], u['KW'], u['stride'], u['padH'], u['padW'], u['out_c0'],
                      u['out_ctot'])
    return ops.conv2d_rect_plan(d, w_aligned16)


def load_inception(path, device='cuda'):
    """an ``InceptionV3`` with the ``state_dict`` file ``path`` loaded strictly (torchvision's ``inception_v3_google-*.pth``, or a
    save of this class; a DataParallel ``module.`` prefix is stripped), on ``device``.  A file whose ``fc.weight`` has 1008 rows is
    the TF-ported FID network (pt_inception-2015-12-05: 1008 classes, no auxiliary head): it is loaded, strictly, into the FID form
    (``fid_variant=True, aux_logits=False``)."""
    sd = state_dict_of(path)
    classes = int(sd['fc.weight'].shape[0])
    if classes == FID_CLASSES:
        net = InceptionV3(num_classes=classes, aux_logits=False, fid_variant=True)
    else:
        net = InceptionV3(num_classes=classes, aux_logits=any(k.startswith('AuxLogits.') for k in sd))
    net.load_state_dict(sd, strict=True)
    return net.to(device)


def inception_network(weights, device, who, fid_form, numbers='numbers are MEANINGLESS'):
    """the network of a metric object, on ``device`` in eval mode.  ``weights``: the path of a ``state_dict`` file
    (``load_inception``), an instance (moved to ``device``), or None for the module attribute ``DEFAULT_WEIGHTS`` (read here, at call
    time) and, when that is None too, a random network under a fixed seed -- the FID form when ``fid_form`` -- and a loud warning
    that names ``who`` and says what its ``numbers`` are then worth."""
    weights = weights if weights is not None else DEFAULT_WEIGHTS
    if weights is not None:
        net = load_inception(weights, device) if isinstance(weights, str) else weights.to(device)
    else:
        print('WARNING: %s is built WITHOUT pretrained weights (weights=None): a seeded random initialisation. Its %s; pass the path '
              'of %s.' % (who, numbers, 'pt_inception-2015-12-05-*.pth' if fid_form else 'inception_v3_google-*.pth'), file=sys.stderr)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(0)
            net = InceptionV3(num_classes=FID_CLASSES, aux_logits=False, fid_variant=True) if fid_form else InceptionV3()
            net = net.to(device)
    return net.eval()


def _chunks(imgs, batch_size, device):
    imgs = imgs.detach().to(device, torch.float32)
    for a in range(0, imgs.size(0), batch_size):
        yield imgs[a:a + batch_size]


def _chunk_features(net, x, resize):
    if resize and tuple(x.shape[2:]) != (299, 299):
        x = ops.resize_bilinear(x, (299, 299))
    return net.features(x)


def pooled_features(net, imgs, batch_size, resize, device):
    """the pooled features [n <= batch_size, dim] of ``imgs`` [N, 3, H, W], chunk by chunk (resized to 299 x 299 on the device first
    when ``resize``); no synchronisation"""
    for x in _chunks(imgs, batch_size, device):
        yield _chunk_features(net, x, resize)


class InceptionScore(nn.Module):
    """scripts/inception_score.py:15-62.  ``imgs`` are [N, 3, H, W] in [-1, 1]; ``resize=True`` resizes them to 299 x 299 on the
    device (sg_resize_bilinear_fwd).  Each call adds softmax rows to a device buffer (doubled when full); nothing is read back
    until ``compute_score``, which reads two numbers.

    ``weights``: the path of a ``state_dict`` file (``load_inception``), an ``InceptionV3`` instance, or None.  None takes the
    module attribute ``DEFAULT_WEIGHTS`` -- process-wide state: every scorer built afterwards without ``weights`` loads that file
    (it exists for callers whose constructor call cannot be changed) -- and, when that is None too, builds a
    random network under a fixed seed and warns.

    ``fid``: a ``fid.FrechetInceptionDistance``; every chunk's pooled features then also go to its fake side (``add_features``), so
    the score and the distance share one forward of THIS scorer's network.  The logits, and the score, are bit-identical."""

    def __init__(self, cuda=True, batch_size=32, resize=False, weights=None, device=None, fid=None):
        super().__init__()
        assert batch_size > 0
        self.fid = fid                      # a fid.FrechetInceptionDistance whose fake side shares this scorer's forward, or None
        if device is None:
            if not cuda:
                raise RuntimeError('InceptionScore: the HIP path has no CPU fallback (cuda=False)')
            device = 'cuda'
        self.resize, self.batch_size, self.device = resize, batch_size, torch.device(device)
        self.inception_model = inception_network(weights, self.device, 'InceptionScore', False,
                                                 'scores are MEANINGLESS as Inception scores')
        self.classes = self.inception_model.fc.out_features
        self.probs, self.count = None, 0
        self.clean()

    def clean(self):
        self.count = 0

    def get_pred(self, x):
        """logits of one chunk (resized first when ``resize``): ``InceptionV3.forward`` is fc(features(x)) under ``no_grad``, so the
        features ``fid`` takes on the way cost no second forward and leave the logits as they are"""
        f = _chunk_features(self.inception_model, x, self.resize)
        if self.fid is not None:
            self.fid.add_features(f)
        with torch.no_grad():
            return self.inception_model.fc(f)

    def forward(self, imgs):
        for x in _chunks(imgs, self.batch_size, self.device):
            logits = self.get_pred(x)
            self.probs = grow_rows(self.probs, self.count, logits.size(0), 4 * self.batch_size, (self.classes,), torch.float32,
                                   self.device)
            ops.softmax_rows(logits, self.probs, self.count)
            self.count += logits.size(0)

    def rows(self):
        """the softmax rows added since ``clean()``, float32 [count, classes] on the device (a view of the buffer); no host read"""
        if self.probs is None:
            return torch.empty(0, self.classes, dtype=torch.float32, device=self.device)
        return self.probs[:self.count]

    def scores(self, splits=1):
        """float64 device tensor {mean, std, per-split scores}; no host read"""
        probs = self.probs if self.probs is not None else torch.empty(1, self.classes, dtype=torch.float32, device=self.device)
        return ops.inception_score(probs, self.count, splits)

    def compute_score(self, splits=1):
        mean, std = self.scores(splits)[:2].tolist()              # the one host read
        return mean, std


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog='python -m scene_generation_amd.inception',
                                description='Inception score of the images under --dir (resized to 299 x 299 on the device)')
    p.add_argument('--dir', required=True, type=str)
    p.add_argument('--weights', default=None, type=str, help='state_dict file of torchvision\'s inception_v3 (never downloaded)')
    p.add_argument('--splits', default=5, type=int)
    p.add_argument('--batch_size', default=32, type=int)
    p.add_argument('--device', default='cuda', type=str)
    p.add_argument('--save_probs', default=None, type=str, help='write the softmax rows [N, classes] as an .npy (what python -m '
                   'scene_generation_amd.isinf --probs reads)')
    return add_arguments(p)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not find_images(args.dir):               # said before a network is built
        raise SystemExit('no images under %s' % args.dir)
    scorer = InceptionScore(batch_size=args.batch_size, resize=True, weights=args.weights, device=args.device)
    print('Calculating Inception Score...')
    _feed_dir(scorer, args.dir, args.batch_size, image_size=args.image_size, resize_filter=args.resize_filter, device=scorer.device)
    mean, std = scorer.compute_score(splits=args.splits)
    print('Inception {} {}'.format(mean, std))
    if args.save_probs is not None:
        import numpy as np
        with open(args.save_probs, 'wb') as f:      # (an open file: numpy.save appends no suffix to it)
            np.save(f, scorer.rows().cpu().numpy())
    return mean, std


if __name__ == '__main__':
    main()
