"""The diversity score: the mean LPIPS distance (richzhang/PerceptualSimilarity) between two pictures generated from the same scene
graph with different appearance draws -- the "Diversity" column of the reference's results table.

    python -m scene_generation_amd.lpips --net alex --backbone W --lin L --dir0 A --dir1 B   -> Diversity MEAN STD
                                         [--image_size H,W [--resize_filter bilinear|bicubic]]

* ``AlexFeatures`` / ``Vgg16Features``: the two backbones, frozen (``forward`` is inference only), parameters under torchvision's names
  (``features.<i>.weight|bias``), five taps each.  AlexNet's 11 x 11 stride-4 stem is ``ops.conv2d_wide``, its other convs
  ``ops.conv2d_rect``, its pools ``ops.maxpool3s2v``; VGG-16 runs the conv + ReLU and 2 x 2 pool launches ``losses.Vgg19`` runs.
* ``LPIPS``: the scaling layer (``ops.lpips_input``), ONE forward of the 2P pictures of P pairs, five ``ops.lpips_layer`` launches
  that add the taps into a float64 [P] device tensor.  No host synchronisation.
* ``LPIPSLoss``: the same distance on VGG-16 as a training objective (``Trainer(lpips_loss=...)`` / SG_LPIPS_LOSS): the backbone run
  with the caller's grad mode (``Vgg16Features.taps``), the target half under ``no_grad``, ``ops.lpips_layer_bwd`` per tap backward.
* ``Diversity``: the scorer ``Sampler(diversity=...)`` drives -- distances gathered in a device buffer, read once by ``compute()``.
* Published numbers come from the package's pretrained backbone and its learned "lin" weights.  Nothing is ever downloaded: both are
  local files.  Without lin weights the unweighted baseline runs, with a loud warning.
"""
import argparse
import os
import re
import sys

import torch
import torch.nn as nn

from . import ops
from .evalkit import find_images, grow_rows, state_dict_of, stored_size_chunks
from .imageprep import ImageDirFeeder, add_arguments

__all__ = ['AlexFeatures', 'Vgg16Features', 'LPIPS', 'LPIPSLoss', 'lpips_loss_from_env', 'check_lpips_loss', 'Diversity', 'load_lin_weights', 'backbone_state_dict', 'pair_files', 'main']

# (torchvision ``features`` index, cin, cout, kernel, stride, pad, 3 x 3 stride-2 max-pool in front)
_ALEX_CONVS = ((0, 3, 64, 11, 4, 2, False), (3, 64, 192, 5, 1, 2, True), (6, 192, 384, 3, 1, 1, True), (8, 384, 256, 3, 1, 1, False),
               (10, 256, 256, 3, 1, 1, False))
_VGG16_CFG = (64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512)
_VGG16_SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))          # end behind relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
CHANNELS = {'alex': (64, 192, 384, 256, 256), 'vgg': (64, 128, 256, 512, 512)}


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
def backbone_state_dict(src):
    """the ``features.<i>.weight|bias`` entries of a backbone file: a torchvision ``alexnet`` / ``vgg16`` state_dict (its
    ``classifier.*`` entries are dropped) or a whole LPIPS module's, where the backbone sits under ``net.slice<j>.<i>.*`` with
    torchvision's index ``i`` kept.  -> dict, or None when ``src`` holds no backbone entry"""
    out = {}
    for k, v in state_dict_of(src).items():
        m = re.match(r'(?:features|net\.slice\d+)\.(\d+)\.(weight|bias)$', k)
        if m:
            out['features.%s.%s' % (m.group(1), m.group(2))] = v
    return out or None


def load_lin_weights(src, channels):
    """the five learned "lin" weight vectors of an LPIPS file as float32 tensors [C_k]: ``lin<k>.model.1.weight`` (the package's
    weights/v0.1/<net>.pth) or ``lins.<k>.model.1.weight`` (a whole module's state_dict), each [1, C_k, 1, 1].  A negative weight
    is refused: the distance is a weighted sum of squares and the package clamps its weights at zero during training."""
    sd = state_dict_of(src)
    out = []
    for k, C in enumerate(channels):
        w = sd.get('lin%d.model.1.weight' % k, sd.get('lins.%d.model.1.weight' % k))
        if w is None:
            raise KeyError('LPIPS lin weights: no lin%d.model.1.weight / lins.%d.model.1.weight' % (k, k))
        w = torch.as_tensor(w, dtype=torch.float32).reshape(-1)
        if w.numel() != C:
            raise ValueError('LPIPS lin weights: tap %d has %d weights, the backbone %d channels' % (k, w.numel(), C))
        if bool((w < 0).any()) or not bool(torch.isfinite(w).all()):
            raise ValueError('LPIPS lin weights: tap %d holds a negative or non-finite weight' % k)
        out.append(w.contiguous())
    return out


class _Backbone(nn.Module):
    def load_backbone(self, src):
        """``src``: a path or a state_dict in one of ``backbone_state_dict``'s forms; loaded strictly"""
        sd = backbone_state_dict(src)
        if sd is None:
            raise KeyError('%s: no features.<i>.weight (or net.slice<j>.<i>.weight) entry' % type(self).__name__)
        self.load_state_dict(sd, strict=True)
        return self

    def _he_init(self, seed):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for m in self.features:
                if isinstance(m, nn.Conv2d):
                    fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
                    m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
        for p in self.parameters():
            p.requires_grad = False


class AlexFeatures(_Backbone):
    """torchvision ``alexnet().features`` up to the ReLU behind conv 10 -> the five taps behind the ReLUs of convs 0, 3, 6, 8, 10.
    Only the convs are modules (under torchvision's indices); ReLU is the conv launch's epilogue."""
    channels = CHANNELS['alex']

    def __init__(self, seed=11):
        super().__init__()
        self.features = nn.Sequential()
        for idx, cin, cout, k, s, p, _ in _ALEX_CONVS:
            self.features.add_module(str(idx), nn.Conv2d(cin, cout, k, stride=s, padding=p))
        self._he_init(seed)

    def forward(self, x):
        taps = []
        with torch.no_grad():
            for idx, _, _, k, s, p, pool in _ALEX_CONVS:
                c = getattr(self.features, str(idx))
                if pool:
                    x = ops.maxpool3s2v(x)
                conv = ops.conv2d_wide if idx == 0 else ops.conv2d_rect
                x = conv(x, c.weight, c.bias, stride=s, pad=(p, p), act=ops.ACT_RELU)
                taps.append(x)
        return taps


class Vgg16Features(_Backbone):
    """torchvision ``vgg16().features[0:30]`` -> relu1_2, relu2_2, relu3_3, relu4_3, relu5_3: conv3x3(pad 1) + ReLU in one launch and
    MaxPool2d(2), the layers and container of ``losses.Vgg19``, under torchvision's indices."""
    channels = CHANNELS['vgg']

    def __init__(self, seed=16):
        super().__init__()
        from .layers import Conv2d, FusedSequential, MaxPool2d, ReLU
        self.features = FusedSequential()
        cin, idx = 3, 0
        for v in _VGG16_CFG:
            if v == 'M':
                self.features.add_module(str(idx), MaxPool2d(2, 2))
                idx += 1
            else:
                self.features.add_module(str(idx), Conv2d(cin, v, kernel_size=3, padding=1))
                self.features.add_module(str(idx + 1), ReLU(True))
                cin, idx = v, idx + 2
        assert idx == 30
        self._he_init(seed)

    def forward(self, x):
        with torch.no_grad():
            return self.taps(x)

    def taps(self, x):
        """the five taps under the CALLER's grad mode: the parameters are frozen, so a backward through them is data gradients only
        (what ``LPIPSLoss`` differentiates; ``forward`` is this under ``no_grad``)"""
        taps = []
        for lo, hi in _VGG16_SLICES:
            x = self.features(x, start=lo, end=hi)
            taps.append(x)
        return taps


# ---- the distance -----------------------------------------------------------------------------------------------------------------------
def _load_weights(module, who, net, backbone_weights, lin_weights):
    """what ``LPIPS`` and ``LPIPSLoss`` share: ``module.net`` loaded from ``backbone_weights`` (or from ``lin_weights`` when that is a
    whole LPIPS module's state_dict), the five lin vectors registered as buffers ``lin<k>`` (None: the unweighted form), and the loud
    warnings for whatever is missing"""
    lin_sd = state_dict_of(lin_weights) if lin_weights is not None else None
    if backbone_weights is None and lin_sd is not None and backbone_state_dict(lin_sd) is not None:
        backbone_weights = lin_sd
    if backbone_weights is not None:
        module.net.load_backbone(backbone_weights)
    else:
        print('WARNING: %s(%s) is built WITHOUT pretrained backbone weights: a seeded random initialisation. Its distances '
              'are MEANINGLESS as LPIPS; pass the path of a torchvision %s state_dict.'
              % (who, net, 'alexnet' if net == 'alex' else 'vgg16'), file=sys.stderr)
    if lin_sd is not None:
        lins = load_lin_weights(lin_sd, module.net.channels)
    else:
        print('WARNING: %s(%s) runs WITHOUT lin weights (lin_weights=None): the unweighted baseline, every channel weight 1. '
              'ITS NUMBERS DO NOT COMPARE WITH PUBLISHED LPIPS / DIVERSITY VALUES.' % (who, net), file=sys.stderr)
        lins = [None] * 5
    for k, w in enumerate(lins):
        module.register_buffer('lin%d' % k, w)


class LPIPS(nn.Module):
    """``forward(x0, x1)`` -> float64 [P] on the device: the LPIPS distance of each pair of pictures [P, 3, H, W], float32 in [-1, 1]
    or uint8 (``channels_last=True``: [P, H, W, 3]).

    ``net``: 'alex' or 'vgg'.  ``backbone_weights``: a torchvision ``alexnet`` / ``vgg16`` state_dict (path or mapping; never
    downloaded), or None -- then the backbone of ``lin_weights`` when that is a whole LPIPS module's state_dict, else a seeded random
    network and a loud warning.  ``lin_weights``: the package's lin file or a whole module's state_dict (``load_lin_weights``), or
    None for the unweighted form (w = 1), which does NOT compare with published numbers."""

    def __init__(self, net='alex', backbone_weights=None, lin_weights=None, device='cuda'):
        super().__init__()
        if net not in CHANNELS:
            raise ValueError("LPIPS: net must be 'alex' or 'vgg', got %r (the SqueezeNet variant is not built)" % (net,))
        self.net_name = net
        self.net = AlexFeatures() if net == 'alex' else Vgg16Features()
        _load_weights(self, 'LPIPS', net, backbone_weights, lin_weights)
        self.to(device)
        self.eval()

    def lin(self, k):
        return getattr(self, 'lin%d' % k)

    def forward(self, x0, x1, channels_last=False):
        if x0.shape != x1.shape or x0.dtype != x1.dtype:
            raise ValueError('LPIPS: two picture batches of one shape and type, got %s %s and %s %s'
                             % (x0.dtype, tuple(x0.shape), x1.dtype, tuple(x1.shape)))
        P = x0.size(0)
        device = self.lin_device()
        x = ops.lpips_input(torch.cat([x0.detach().to(device), x1.detach().to(device)]), channels_last=channels_last)
        out = torch.empty(P, dtype=torch.float64, device=device)
        for k, t in enumerate(self.net(x)):
            ops.lpips_layer(t[:P], t[P:], self.lin(k), out=out, accumulate=k > 0)
        return out

    def lin_device(self):
        return next(self.net.parameters()).device


class LPIPSLoss(nn.Module):
    """LPIPS-VGG as a training objective: ``forward(x, y)`` -> a float32 scalar, the mean over the batch of LPIPS(x, y), with a
    gradient for ``x`` only.  ``y`` (the target) is detached and its taps are taken under ``no_grad`` in a second pass of the frozen
    backbone, as ``losses.VGGLoss`` does: no data gradient is spent on the target half.  The distance is ``ops.LpipsDistanceFn``: the
    five ``ops.lpips_layer`` launches of ``LPIPS`` forward, one ``ops.lpips_layer_bwd`` launch per tap backward.  Runs eagerly.

    ``input``: 'imagenet' -- pictures normalised with the ImageNet mean (0.485, 0.456, 0.406) and std (0.229, 0.224, 0.225), what a
    ``Trainer`` holds; they feed the backbone directly, because the scaling layer of LPIPS on [-1, 1] pictures IS that normalisation
    (shift = 2 mean - 1, scale = 2 std, to within 3e-8).  The two routes differ by the float32 rounding of the input: a picture that
    went through [-1, 1] and ``ops.lpips_input`` is not bit for bit the one normalised from [0, 1].  'unit' -- pictures in [-1, 1],
    through ``ops.lpips_input`` and its backward.

    Weights and warnings as for ``LPIPS``.  VGG-16 only: the AlexNet form would need a data gradient of the 11 x 11 stride-4 stem.
    A pixel of a tap whose channels are all zero gets a finite gradient from the distance, which the ReLU in front of the tap then
    drops (sg_lpips_layer_bwd in the header)."""

    def __init__(self, backbone_weights=None, lin_weights=None, input='imagenet', net='vgg', device='cuda'):
        super().__init__()
        if net != 'vgg':
            raise ValueError("LPIPSLoss: net must be 'vgg', got %r (no other backbone has a data gradient here)" % (net,))
        if input not in ('imagenet', 'unit'):
            raise ValueError("LPIPSLoss: input must be 'imagenet' or 'unit', got %r" % (input,))
        self.net_name, self.input = net, input
        self.net = Vgg16Features()
        _load_weights(self, 'LPIPSLoss', net, backbone_weights, lin_weights)
        self.to(device)
        self.eval()

    def lin(self, k):
        return getattr(self, 'lin%d' % k)

    def forward(self, x, y):
        if x.shape != y.shape or x.dim() != 4 or x.size(1) != 3 or x.dtype != torch.float32 or y.dtype != torch.float32:
            raise ValueError('LPIPSLoss: two float32 picture batches [N, 3, H, W] of one shape, got %s %s and %s %s'
                             % (x.dtype, tuple(x.shape), y.dtype, tuple(y.shape)))
        y = y.detach()
        if self.input == 'unit':
            x, y = ops.LpipsInputFn.apply(x), ops.lpips_input(y)
        fx = self.net.taps(x)
        with torch.no_grad():            # the target and a frozen network: nothing to record
            fy = self.net.taps(y)
        d = ops.LpipsDistanceFn.apply(ops.LPIPS_EPS, *fx, *fy, *[self.lin(k) for k in range(5)])
        return d.mean().float()


_LOSS_KEYS = ('weight', 'backbone', 'lin')


def check_lpips_loss(value, what='lpips_loss'):
    """-> {'weight': float > 0, 'backbone': path or None, 'lin': path or None}: the ``Trainer``'s LPIPS term.  ``value``: a number
    (the weight), a dict over those keys, or the spelling of SG_LPIPS_LOSS: ``'1.0'`` or ``'weight=1.0,backbone=PATH,lin=PATH'``
    (``weight`` is required, the paths are optional).  Anything else raises ValueError naming ``what``."""
    if isinstance(value, str):
        parts = [s.strip() for s in value.split(',')]
        if len(parts) == 1 and '=' not in parts[0]:
            value = parts[0]
        else:
            d = {}
            for s in parts:
                name, eq, v = s.partition('=')
                if not eq or name.strip() in d or not v.strip():
                    raise ValueError('%s: expected a float or weight=float[,backbone=PATH][,lin=PATH], got %r' % (what, value))
                d[name.strip()] = v.strip()
            value = d
    if not isinstance(value, dict):
        value = {'weight': value}
    for name in value:
        if name not in _LOSS_KEYS:
            raise ValueError('%s: unknown key %r (expected %s)' % (what, name, ', '.join(_LOSS_KEYS)))
    if 'weight' not in value:
        raise ValueError('%s: no weight' % what)
    try:
        w = float(value['weight'])
    except (TypeError, ValueError):
        raise ValueError('%s: expected a positive finite weight, got %r' % (what, value['weight']))
    if isinstance(value['weight'], bool) or not 0.0 < w < float('inf'):      # (also rejects nan)
        raise ValueError('%s: expected a positive finite weight, got %r' % (what, value['weight']))
    out = {'weight': w}
    for name in ('backbone', 'lin'):
        v = value.get(name)
        if v is not None and not isinstance(v, (str, dict)):
            raise ValueError('%s: %s must be a path (or a state_dict), got %r' % (what, name, type(v).__name__))
        out[name] = v
    return out


def lpips_loss_from_env(environ=None):
    """SG_LPIPS_LOSS: the LPIPS term of a Trainer built without ``lpips_loss``.  Unset or empty: None (no term); ``1.0``: the weight;
    ``weight=1.0,backbone=PATH,lin=PATH``: the weight and the weight files; anything else raises ValueError (check_lpips_loss)."""
    v = (os.environ if environ is None else environ).get('SG_LPIPS_LOSS', '')
    if v.strip() == '':
        return None
    return check_lpips_loss(v, 'SG_LPIPS_LOSS=%r' % v)


class Diversity(object):
    """mean and population std of the LPIPS distance over pairs of pictures.  ``__call__(imgs0, imgs1)``: two batches of one shape,
    float32 [N, 3, H, W] in [-1, 1], uint8 [N, 3, H, W], or uint8 [N, H, W, 3] (what ``SampleOut.images`` holds); the distances go
    into a float64 device buffer (doubled when full); nothing is read back until ``compute()``."""

    def __init__(self, lpips, batch_size=32):
        assert batch_size > 0
        self.lpips, self.batch_size = lpips, int(batch_size)
        self.dist, self.count = None, 0

    def clean(self):
        self.count = 0

    def __call__(self, imgs0, imgs1):
        channels_last = imgs0.dim() == 4 and imgs0.dtype == torch.uint8 and imgs0.size(3) == 3 and imgs0.size(1) != 3
        for a in range(0, imgs0.size(0), self.batch_size):
            d = self.lpips(imgs0[a:a + self.batch_size], imgs1[a:a + self.batch_size], channels_last=channels_last)
            self.dist = grow_rows(self.dist, self.count, d.numel(), 4 * self.batch_size, (), torch.float64, d.device)
            self.dist[self.count:self.count + d.numel()].copy_(d)
            self.count += d.numel()

    def compute(self):
        """{'mean', 'std', 'pairs'}: float64 mean and POPULATION std of the distances; the one device-to-host read"""
        if self.count == 0:
            return {'mean': float('nan'), 'std': float('nan'), 'pairs': 0}
        d = self.dist[:self.count]
        mean = d.mean()
        std = ((d - mean) ** 2).mean().sqrt()
        mean, std = torch.stack([mean, std]).tolist()
        return {'mean': mean, 'std': std, 'pairs': self.count}


# ---- command line -----------------------------------------------------------------------------------------------------------------------
def pair_files(dir0, dir1):
    """[(path in dir0, path in dir1)]: the image files of both directories (``evalkit.find_images``: recursive, sorted), the i-th
    of one with the i-th of the other"""
    a, b = find_images(dir0), find_images(dir1)
    if not a:
        raise SystemExit('no images under %s' % dir0)
    if len(a) != len(b):
        raise SystemExit('%d images under %s against %d under %s: the directories do not pair up' % (len(a), dir0, len(b), dir1))
    return list(zip(a, b))


def build_parser():
    p = argparse.ArgumentParser(prog='python -m scene_generation_amd.lpips',
                                description='Diversity: mean LPIPS distance between the pictures of two directories, paired by sorted name')
    p.add_argument('--net', default='alex', choices=sorted(CHANNELS))
    p.add_argument('--backbone', default=None, type=str, help='torchvision alexnet / vgg16 state_dict file (never downloaded)')
    p.add_argument('--lin', default=None, type=str, help='the LPIPS lin weights (weights/v0.1/<net>.pth of the package, or a whole '
                   'module\'s state_dict); without them the unweighted baseline runs and the number compares with nothing published')
    p.add_argument('--dir0', required=True, type=str)
    p.add_argument('--dir1', required=True, type=str)
    p.add_argument('--batch_size', default=32, type=int)
    p.add_argument('--device', default='cuda', type=str)
    return add_arguments(p)


def main(argv=None):
    args = build_parser().parse_args(argv)
    pairs = pair_files(args.dir0, args.dir1)
    scorer = Diversity(LPIPS(args.net, backbone_weights=args.backbone, lin_weights=args.lin, device=args.device), args.batch_size)
    if args.image_size is not None:             # both directories through the loader's resize on the device: full chunks of one size
        chunks = zip(*[ImageDirFeeder(d, args.batch_size, args.image_size, args.resize_filter, args.device) for d in (args.dir0, args.dir1)])
    else:                                       # the files at their stored sizes: a pair must agree, a chunk holds one size
        chunks = stored_size_chunks([list(column) for column in zip(*pairs)], args.batch_size)
    for a, b in chunks:
        scorer(a, b)
    r = scorer.compute()
    print('Diversity {} {}'.format(r['mean'], r['std']))
    return r['mean'], r['std']


if __name__ == '__main__':
    main()
