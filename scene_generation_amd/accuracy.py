"""The object-accuracy classifier: the reference's last evaluation step (scripts/train_accuracy_net.py and the ``Accuracy`` line
of scripts/sample_images.py:180-182,224-239,294-295) on this stack.

    python -m scene_generation_amd.accuracy train [--model_name resnet101] [--epochs 20] ...   -> <name>_<n>_classes.pth
    python -m scene_generation_amd.accuracy score --model PATH --checkpoint CKPT.pt [...]      -> Accuracy X

* ``ResNet`` (``resnet18 / 34 / 50 / 101 / 152``): torchvision's v1.5 layout -- 7x7 stride-2 stem, 3x3 stride-2 max-pool, the
  stride of a ``Bottleneck`` on its 3x3 ``conv2``, a strided 1x1 ``downsample`` (conv + BatchNorm) where the shape changes -- built
  from this project's modules, with torchvision's ``state_dict`` keys and shapes, so the reference's ``.pth`` files load.
* ``all_pretrained_models`` / ``load_model`` / ``train_model``: the reference's script functions, quirks included (see each).
* Eval fast path (``ResNet.fold_batchnorm``): under ``eval()`` with gradients off every conv + BatchNorm (+ ReLU) runs as ONE
  convolution with folded weights and bias (sg_bn_fold) and the convolution's own activation: no BatchNorm pass over the activations.
* ``AccuracyMeter``: crops -> network -> sg_classify_stats in chunks, accumulated on the device, read once by ``summary()``.
"""
import argparse
import sys

import torch
import torch.nn as nn

from . import layers, ops
from .bilinear import crop_bbox_batch
from .evalkit import FoldCache, folded, state_dict_of

__all__ = ['BasicBlock', 'Bottleneck', 'ResNet', 'resnet18', 'resnet34', 'resnet50', 'resnet101', 'resnet152',
           'all_pretrained_models', 'load_model', 'train_model', 'StepLR', 'AccuracyMeter']


def _conv_bn(conv, bn, x, relu, fold):
    """act(bn(conv(x))).  ``fold``: None (two launches: convolution, BatchNorm with the fused activation) or the owning network's
    fold cache (one launch: the convolution with the BatchNorm folded into its weights and bias)."""
    act = ops.ACT_RELU if relu else ops.ACT_NONE
    if fold is None:
        return bn(conv(x), act=act)
    w, b = folded(conv, bn, fold)
    return ops.conv2d(x, w, b, stride=conv.stride[0], pad=conv.padding[0], act=act)


def _conv(cin, cout, k, stride=1):
    return layers.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=k // 2, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv(inplanes, planes, 3, stride)
        self.bn1 = layers.BatchNorm2d(planes)
        self.conv2 = _conv(planes, planes, 3)
        self.bn2 = layers.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x, fold=None):
        out = _conv_bn(self.conv1, self.bn1, x, True, fold)
        out = _conv_bn(self.conv2, self.bn2, out, False, fold)
        idt = x if self.downsample is None else _conv_bn(self.downsample[0], self.downsample[1], x, False, fold)
        return ops.add_relu(out, idt)


class Bottleneck(nn.Module):
    """torchvision v1.5: the stride sits on the 3x3 ``conv2``, not on the first 1x1"""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv(inplanes, planes, 1)
        self.bn1 = layers.BatchNorm2d(planes)
        self.conv2 = _conv(planes, planes, 3, stride)
        self.bn2 = layers.BatchNorm2d(planes)
        self.conv3 = _conv(planes, planes * 4, 1)
        self.bn3 = layers.BatchNorm2d(planes * 4)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x, fold=None):
        out = _conv_bn(self.conv1, self.bn1, x, True, fold)
        out = _conv_bn(self.conv2, self.bn2, out, True, fold)
        out = _conv_bn(self.conv3, self.bn3, out, False, fold)
        idt = x if self.downsample is None else _conv_bn(self.downsample[0], self.downsample[1], x, False, fold)
        return ops.add_relu(out, idt)


class ResNet(FoldCache):
    """torchvision.models.ResNet(block, layers, num_classes) with its ``state_dict`` keys: conv1, bn1, layer1..4, fc.

    Eval fast path (``fold_batchnorm``, a class attribute; ON by default: measured on MI355X, ResNet-101 at 224 in 64-crop chunks,
    12.73 against 14.85 ms with spreads of 0.1 %; ``ResNet.fold_batchnorm = False`` keeps the plain form
    everywhere): with ``self.training`` off and gradients disabled every conv + BatchNorm pair runs as one convolution with folded
    weights.
    The folded weights are cached; the cache is dropped by ``train()``, ``load_state_dict()`` and ``drop_fold()``, and an entry is
    rebuilt when one of its tensors was replaced or written in place (version counters: torch's own writes, and
    ``FusedSGD.step()``, which bumps the counters of the parameters its kernel wrote).  Running statistics only move in training
    mode, which is left through ``train(False)``.  Any other raw-pointer write needs ``drop_fold()``.

    The longest prefix of (stem, layer1, ..., layer4) without a parameter that requires a gradient runs without a tape when the
    input needs none: under ``all_pretrained_models`` that is the stem and layer1, whose BatchNorms still run -- and move their
    running statistics -- in training mode, as in the reference."""
    fold_batchnorm = True

    def __init__(self, block, layer_sizes, num_classes=1000):
        super().__init__()
        self.inplanes = 64
        self.conv1 = layers.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = layers.BatchNorm2d(64)
        self.maxpool = layers.MaxPool3s2()
        self.layer1 = self._make_layer(block, 64, layer_sizes[0])
        self.layer2 = self._make_layer(block, 128, layer_sizes[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layer_sizes[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layer_sizes[3], stride=2)
        self.avgpool = layers.GlobalAvgPool()
        self.fc = layers.Linear(512 * block.expansion, num_classes)
        for m in self.modules():        # torchvision's init
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(_conv(self.inplanes, planes * block.expansion, 1, stride),
                                       layers.BatchNorm2d(planes * block.expansion))
        mods = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            mods.append(block(self.inplanes, planes))
        return nn.Sequential(*mods)

    def train(self, mode=True):         # on top of evalkit.FoldCache: running statistics move in training mode
        self.drop_fold()
        return super().train(mode)

    def _stages(self):
        return [[self.conv1, self.bn1], [self.layer1], [self.layer2], [self.layer3], [self.layer4]]

    def frozen_stages(self):
        """how many leading stages (stem, layer1, ..., layer4) hold no parameter that requires a gradient"""
        k = 0
        for mods in self._stages():
            if any(p.requires_grad for m in mods for p in m.parameters()):
                break
            k += 1
        return k

    def _stage(self, i, x, fold):
        if i == 0:
            return self.maxpool(_conv_bn(self.conv1, self.bn1, x, True, fold))
        for blk in getattr(self, 'layer%d' % i):
            x = blk(x, fold)
        return x

    def forward(self, x):
        fold = self._fold_cache if (self.fold_batchnorm and not self.training and not torch.is_grad_enabled()) else None
        k = self.frozen_stages() if (torch.is_grad_enabled() and not x.requires_grad) else 0
        if k:
            with torch.no_grad():
                for i in range(k):
                    x = self._stage(i, x, fold)
        for i in range(k, 5):
            x = self._stage(i, x, fold)
        return self.fc(self.avgpool(x))


_CONFIGS = {'resnet18': (BasicBlock, (2, 2, 2, 2)), 'resnet34': (BasicBlock, (3, 4, 6, 3)), 'resnet50': (Bottleneck, (3, 4, 6, 3)),
            'resnet101': (Bottleneck, (3, 4, 23, 3)), 'resnet152': (Bottleneck, (3, 8, 36, 3))}


def _build(name, num_classes=1000):
    if name not in _CONFIGS:
        raise ValueError('unknown network %r: expected one of %s' % (name, ', '.join(sorted(_CONFIGS))))
    block, sizes = _CONFIGS[name]
    return ResNet(block, sizes, num_classes)


def resnet18(num_classes=1000):
    return _build('resnet18', num_classes)


def resnet34(num_classes=1000):
    return _build('resnet34', num_classes)


def resnet50(num_classes=1000):
    return _build('resnet50', num_classes)


def resnet101(num_classes=1000):
    return _build('resnet101', num_classes)


def resnet152(num_classes=1000):
    return _build('resnet152', num_classes)


def conv_descs(name, size=224):
    """the distinct convolutions of network ``name`` on a size x size input, in order of first use:
    [(Cin, Cout, KS, stride, H)] with H the (square) input plane of the convolution; the padding is KS // 2"""
    block, sizes = _CONFIGS[name]
    out = [(3, 64, 7, 2, size)]
    h = (size + 6 - 7) // 2 + 1
    h = (h - 1) // 2 + 1
    inplanes = 64

    def add(*d):
        if d not in out:
            out.append(d)

    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), sizes)):
        for b in range(n):
            stride = 2 if (li > 0 and b == 0) else 1
            oh = (h - 1) // stride + 1
            wide = planes * block.expansion
            if block is BasicBlock:
                add(inplanes, planes, 3, stride, h)
                add(planes, planes, 3, 1, oh)
            else:
                add(inplanes, planes, 1, 1, h)
                add(planes, planes, 3, stride, h)
                add(planes, wide, 1, 1, oh)
            if stride != 1 or inplanes != wide:
                add(inplanes, wide, 1, stride, h)
            inplanes, h = wide, oh
    return out


def all_pretrained_models(n_class, name='resnet101', weights=None):
    """train_accuracy_net.py:62-101.  Every parameter is frozen, a fresh ``fc`` with ``n_class`` outputs is trainable, and every
    child after ``layer1`` is made trainable again: conv1, bn1 and layer1 stay frozen (their BatchNorms still run in training
    mode under ``model.train(True)``, as in the reference).

    ``weights``: the path of a torchvision ImageNet ``state_dict`` (or the dict itself) -- what ``pretrained='imagenet'`` downloads
    in the reference; everything but ``fc`` is loaded.  Without it the network keeps its random init and says so loudly: the
    arithmetic, shapes and cost are the reference's, the features are not."""
    print('[Building %s]' % name)
    model = _build(name, 1000)
    if weights is not None:
        sd = {k: v for k, v in state_dict_of(weights).items() if not k.startswith('fc.')}
        missing, unexpected = model.load_state_dict(sd, strict=False)
        missing = [k for k in missing if not k.startswith('fc.')]
        if missing or unexpected:
            raise KeyError('ImageNet weights do not fit %s: missing %s, unexpected %s' % (name, missing, list(unexpected)))
    else:
        print('WARNING: %s is built WITHOUT ImageNet weights (none given: weights=None): random initialisation. The reference '
              'fine-tunes torchvision\'s pretrained network; accuracies of this one are not comparable.' % name, file=sys.stderr)
    for p in model.parameters():
        p.requires_grad = False
    model.fc = layers.Linear(model.fc.in_features, n_class)
    print('[Resnet: Freezing layers only till layer1 including]')
    seen = []
    for child_name, child in model.named_children():
        if 'layer1' in seen:
            for p in child.parameters():
                p.requires_grad = True
        seen.append(child_name)
    return model


def load_model(path, name='resnet101', n_class=172, device='cuda'):
    """train_accuracy_net.py:237-242: the classifier saved by ``train`` (or by the reference), on ``device``, in eval mode.  Also
    accepts the ``module.`` prefix of a DataParallel save.  ``n_class=None`` takes the class count from the file's ``fc.weight``."""
    sd = state_dict_of(path)
    if n_class is None:
        n_class = int(sd['fc.weight'].shape[0])
    model = _build(name, n_class)
    model.load_state_dict(sd)
    model = model.to(device)
    model.eval()
    return model


class StepLR(object):
    """torch.optim.lr_scheduler.StepLR(optimizer, step_size, gamma) with the counting of the reference's torch: the first
    ``step()`` enters epoch 0, so with ``step()`` at the top of every epoch (train_model) epochs 0 .. step_size - 1 run at the base
    rate.  Writes ``optimizer.param_groups[*]['lr']``."""

    def __init__(self, optimizer, step_size, gamma=0.1):
        self.optimizer, self.step_size, self.gamma = optimizer, int(step_size), float(gamma)
        self.base_lrs = [float(g['lr']) for g in optimizer.param_groups]
        self.last_epoch = -1

    def get_lr(self):
        return [b * self.gamma ** (max(self.last_epoch, 0) // self.step_size) for b in self.base_lrs]

    def step(self):
        self.last_epoch += 1
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            g['lr'] = lr


def _classify_record(outputs, labels, acc):
    return ops.classify_stats(outputs, labels, ignore_label=-1, acc=acc)[0]


def train_model(model, test_dataloader, val_dataloader, criterion, optimizer, scheduler, use_gpu, num_epochs=10, input_shape=224,
                *, keep_best=False, crop=None, classify=None):
    """train_accuracy_net.py:156-234, reproduced with its quirks:
      * ``scheduler.step()`` comes BEFORE an epoch's training;
      * ``epoch_loss`` is the sum of the batch-MEAN losses divided by the number of OBJECTS; ``epoch_acc`` is correct / objects;
      * the reference's "best" weights are ``model.state_dict()`` -- an alias of the live tensors -- so what it loads back at the
        end is the LAST epoch's model, whichever epoch scored best.  ``keep_best=True`` (keyword-only, not in the reference) copies
        the tensors instead, so the returned model is the best epoch's.
    The loss sum and the correct count stay on the device (sg_classify_stats); a phase ends with ONE read of both.
    ``crop(imgs, boxes, obj_to_img, size)`` and ``classify(outputs, labels, acc) -> acc`` (acc: int64 [3] = correct, counted, rows,
    or None) replace the cropper and the device record (tests, other croppers).  -> model."""
    crop = crop_bbox_batch if crop is None else crop
    classify = _classify_record if classify is None else classify
    best_model_wts = model.state_dict()
    best_acc = 0.0
    device = 'cuda' if use_gpu else 'cpu'
    for epoch in range(num_epochs):
        print('Epoch {}/{}'.format(epoch, num_epochs - 1))
        print('-' * 10)
        for phase in ['train', 'val']:
            if phase == 'train':
                scheduler.step()
                model.train(True)
                dataloader = test_dataloader
            else:
                model.train(False)
                dataloader = val_dataloader
            running_loss, acc, objects_len = None, None, 0
            for data in dataloader:
                imgs, objs, boxes, masks, triples, obj_to_img, triple_to_img, attributes = data
                imgs, boxes, obj_to_img, labels = imgs.to(device), boxes.to(device), obj_to_img.to(device), objs.to(device)
                objects_len += obj_to_img.shape[0]
                with torch.no_grad():
                    crops = crop(imgs, boxes, obj_to_img, input_shape)
                optimizer.zero_grad()
                with torch.set_grad_enabled(phase == 'train'):
                    outputs = model(crops)
                    if type(outputs) == tuple:
                        outputs, _ = outputs
                    loss = criterion(outputs, labels)
                if phase == 'train':
                    loss.backward()
                    optimizer.step()
                with torch.no_grad():
                    acc = classify(outputs.detach(), labels, acc)
                    running_loss = loss.detach().clone() if running_loss is None else running_loss + loss.detach()
            if objects_len:
                total, corrects = torch.cat([running_loss.double().view(1), acc[:1].double()]).tolist()     # the phase's one read
            else:
                total, corrects = 0.0, 0.0
            epoch_loss = total / objects_len if objects_len else float('nan')
            epoch_acc = corrects / objects_len if objects_len else float('nan')
            print('{} Loss: {:.4f} Acc: {:.4f}'.format(phase, epoch_loss, epoch_acc))
            if phase == 'val' and epoch_acc > best_acc:
                best_acc = epoch_acc
                best_model_wts = model.state_dict()
                if keep_best:
                    best_model_wts = {k: v.detach().clone() for k, v in best_model_wts.items()}
        print()
    print('Best val Acc: {:4f}'.format(best_acc))
    model.load_state_dict(best_model_wts)
    return model


class AccuracyMeter(object):
    """sample_images.py:224-239 without its two ``.item()`` per object: ``update`` crops the images at the boxes
    (crop_bbox_batch, ``input_shape`` x ``input_shape``), runs the network on ``crop_chunk`` crops at a time and adds to a device
    record through sg_classify_stats with ``ignore_label=0`` (the __image__ class is neither counted nor correct); ``summary()`` is
    the single host read.

    Chunks exist because the activations are large (conv1's output alone is 3.2 MB per crop at 224).  The chunk size also decides
    the kernel route of the 3x3 stride-1 convs: Winograd takes those with >= 128 channels (in multiples of 128) on an even plane
    whose tile count N * OH/2 * OW/2 is a multiple of 128.  At 224 a chunk of 64 crops qualifies only the 128-channel convs on
    28 x 28 (64 * 14 * 14 = 98 * 128); the 256-channel convs on 14 x 14 give 64 * 7 * 7 = 3136, no multiple of 128, and need 128
    crops (6272 = 49 * 128); the 512-channel convs on the odd 7 x 7 plane never qualify.  A ragged last chunk runs the direct
    kernels throughout, so its logits differ from a full chunk's in the last bits.  The default is 128 crops: measured on MI355X
    (ResNet-101, folded), 0.166 ms per crop against 0.199 ms at 64 crops; conv1's output is then 411 MB."""

    def __init__(self, model, input_shape=224, crop_chunk=128):
        self.model, self.input_shape, self.crop_chunk = model, int(input_shape), int(crop_chunk)
        if self.crop_chunk < 1:
            raise ValueError('crop_chunk must be >= 1')
        self.acc = None

    def logits(self, imgs, boxes, obj_to_img):
        """the network's outputs for every box, chunk by chunk (no host synchronisation)"""
        outs = []
        with torch.no_grad():
            for a in range(0, boxes.size(0), self.crop_chunk):
                b = min(a + self.crop_chunk, boxes.size(0))
                crops = crop_bbox_batch(imgs, boxes[a:b], obj_to_img[a:b], self.input_shape)
                out = self.model(crops)
                outs.append(out[0] if type(out) == tuple else out)
        return outs

    def update(self, imgs, boxes, obj_to_img, objs):
        if self.acc is None:
            self.acc = ops.new_classify_record(boxes.device)
        a = 0
        for out in self.logits(imgs, boxes, obj_to_img):
            ops.classify_stats(out, objs[a:a + out.size(0)], ignore_label=0, acc=self.acc)
            a += out.size(0)

    def summary(self):
        """the ONE device-to-host read: {'accuracy', 'correct', 'counted'}"""
        correct, counted, _ = self.acc.tolist() if self.acc is not None else (0, 0, 0)
        return {'accuracy': correct / counted if counted else float('nan'), 'correct': int(correct), 'counted': int(counted)}


# ---- command line -------------------------------------------------------------------------------------------------------------
def _synthetic_batches(n_batches, batch_size, image_size, n_class, seed):
    from .synthetic import make_batch
    return [make_batch(N=batch_size, size=image_size, num_objs=n_class, seed=seed + k) for k in range(n_batches)]


def _host_loaders(args):
    """the host checkout's COCO loaders (train_accuracy_net.py:104-153) when ``scene_generation.data`` imports, else None"""
    try:
        from scene_generation.data.coco import CocoSceneGraphDataset, coco_collate_fn     # noqa: F401
    except ImportError:
        return None
    from torch.utils.data import DataLoader
    kw = dict(stuff_only=True, image_size=(args.image_size, args.image_size), mask_size=args.mask_size, min_object_size=0.02,
              min_objects_per_image=3, include_other=False, include_relationships=True, no__img__=True)
    coco = args.coco_dir
    train = CocoSceneGraphDataset(image_dir=coco + '/images/train2017', instances_json=coco + '/annotations/instances_train2017.json',
                                  stuff_json=coco + '/annotations/stuff_train2017.json', max_samples=args.num_train_samples, **kw)
    val = CocoSceneGraphDataset(image_dir=coco + '/images/val2017', instances_json=coco + '/annotations/instances_val2017.json',
                                stuff_json=coco + '/annotations/stuff_val2017.json', max_samples=args.num_val_samples, **kw)
    lk = dict(batch_size=args.batch_size, num_workers=args.loader_num_workers, collate_fn=coco_collate_fn)
    return DataLoader(train, shuffle=True, **lk), DataLoader(val, shuffle=True, **lk)


def make_parser():
    p = argparse.ArgumentParser(prog='python -m scene_generation_amd.accuracy', description=__doc__.split('\n')[0])
    sub = p.add_subparsers(dest='command', required=True)
    t = sub.add_parser('train', help='fine-tune a ResNet on object crops (scripts/train_accuracy_net.py)')
    t.add_argument('-mo', '--model_name', default='resnet101', choices=sorted(_CONFIGS))
    t.add_argument('--weights', default=None, help='torchvision ImageNet state_dict (.pth) to start from')
    t.add_argument('-ep', '--epochs', default=20, type=int)
    t.add_argument('-b', '--batch_size', default=4, type=int)
    t.add_argument('-is', '--input_shape', default=224, type=int)
    t.add_argument('-sl', '--save_loc', default='.')
    t.add_argument('--n_class', default=172, type=int)
    t.add_argument('--image_size', default=256, type=int)
    t.add_argument('--mask_size', default=32, type=int)
    t.add_argument('--num_train_samples', default=None, type=int)
    t.add_argument('--num_val_samples', default=1024, type=int)
    t.add_argument('--loader_num_workers', default=4, type=int)
    t.add_argument('--coco_dir', default='datasets/coco')
    t.add_argument('--synthetic_batches', default=8, type=int, help='batches per epoch of the synthetic generator (no COCO loader)')
    t.add_argument('--keep_best', default=0, type=int, help='1: return the best epoch\'s weights (the reference returns the last)')
    t.add_argument('--seed', default=0, type=int)
    s = sub.add_parser('score', help='the Accuracy line of scripts/sample_images.py for a generator checkpoint')
    s.add_argument('--model', required=True, help='the classifier (<name>_<n>_classes.pth)')
    s.add_argument('--model_name', default='resnet101', choices=sorted(_CONFIGS))
    s.add_argument('--checkpoint', required=True)
    s.add_argument('--input_shape', default=224, type=int)
    s.add_argument('--crop_chunk', default=128, type=int)
    s.add_argument('--batch_size', default=24, type=int)
    s.add_argument('--num_samples', default=24, type=int)
    s.add_argument('--features', default=None)
    s.add_argument('--weights', default='model')
    for flag in ('use_gt_boxes', 'use_gt_masks', 'use_gt_attr', 'use_gt_textures'):
        s.add_argument('--' + flag, default=0, type=int)
    return p


def main(argv=None):
    import os
    args = make_parser().parse_args(argv)
    if args.command == 'train':
        from .optim import FusedSGD
        torch.manual_seed(args.seed)
        loaders = _host_loaders(args)
        if loaders is None:
            print('scene_generation.data is not importable: training on the synthetic generator')
            loaders = (_synthetic_batches(args.synthetic_batches, args.batch_size, args.image_size, args.n_class, args.seed),
                       _synthetic_batches(max(args.synthetic_batches // 4, 1), args.batch_size, args.image_size, args.n_class,
                                          args.seed + 10 ** 6))
        model = all_pretrained_models(args.n_class, name=args.model_name, weights=args.weights).to('cuda')
        optimizer = FusedSGD([p for p in model.parameters() if p.requires_grad], lr=0.001, momentum=0.9)
        scheduler = StepLR(optimizer, step_size=7, gamma=0.1)
        model = train_model(model, loaders[0], loaders[1], ops.cross_entropy, optimizer, scheduler, True, num_epochs=args.epochs,
                            input_shape=args.input_shape, keep_best=bool(args.keep_best))
        path = os.path.join(args.save_loc, '{}_{}_classes.pth'.format(args.model_name, args.n_class))
        torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, path)
        print('Saved', path)
        return path
    from . import sample
    checkpoint = torch.load(args.checkpoint, map_location='cpu', weights_only=False)
    model = sample.build_model(args, checkpoint, 'cuda')
    meter = AccuracyMeter(load_model(args.model, args.model_name, n_class=None), args.input_shape, args.crop_chunk)
    features = None if args.use_gt_textures else sample.load_features(args)
    sampler = sample.Sampler(model, features=features, accuracy=meter)
    for batch in sample.synthetic_loader(model, args.batch_size, args.num_samples, checkpoint['model_kwargs'].get('mask_size', 32)):
        sampler.sample_batch(batch, bool(args.use_gt_boxes), bool(args.use_gt_masks), bool(args.use_gt_textures), bool(args.use_gt_attr))
    summary = meter.summary()
    print('Accuracy {}'.format(summary['accuracy']))
    return summary


if __name__ == '__main__':
    main()
