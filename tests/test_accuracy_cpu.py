"""The accuracy network's host logic, without a GPU: torchvision's parameter counts and state_dict keys, the freeze rule of
all_pretrained_models, the DataParallel prefix, train_model's schedule and bookkeeping quirks (with a stub network), and the
yardsticks of tests/accuracy_ref.py themselves against torch on the CPU."""
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import accuracy_ref as R
from conftest import skip_random_init
from scene_generation_amd import accuracy as A

COUNTS = {'resnet18': (11689512, 122), 'resnet34': (21797672, 218), 'resnet50': (25557032, 320), 'resnet101': (44549160, 626),
          'resnet152': (60192808, 932)}


@pytest.mark.parametrize('name', sorted(COUNTS))
def test_parameter_and_entry_counts(name):
    with skip_random_init():
        m = getattr(A, name)()
        ref = R.RefResNet(name)
    params, entries = COUNTS[name]
    assert sum(p.numel() for p in m.parameters()) == params
    sd, rsd = m.state_dict(), ref.state_dict()
    assert len(sd) == entries
    assert list(sd) == list(rsd)                                  # same keys, same order as the plain torch.nn restatement
    assert all(sd[k].shape == rsd[k].shape and sd[k].dtype == rsd[k].dtype for k in sd)


def _bn(prefix):
    return [prefix + '.' + s for s in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')]


def test_resnet18_keys():
    want = ['conv1.weight'] + _bn('bn1')
    for layer in (1, 2, 3, 4):
        for b in (0, 1):
            p = 'layer%d.%d' % (layer, b)
            want += [p + '.conv1.weight'] + _bn(p + '.bn1') + [p + '.conv2.weight'] + _bn(p + '.bn2')
            if layer > 1 and b == 0:
                want += [p + '.downsample.0.weight'] + _bn(p + '.downsample.1')
    want += ['fc.weight', 'fc.bias']
    with skip_random_init():
        sd = A.resnet18(172).state_dict()
    assert list(sd) == want
    assert 'layer2.0.downsample.0.weight' in sd and 'layer2.0.downsample.1.running_var' in sd
    assert not any(k.startswith('layer1.0.downsample') for k in sd)
    assert sd['conv1.weight'].shape == (64, 3, 7, 7) and sd['fc.weight'].shape == (172, 512)
    assert sd['layer2.0.downsample.0.weight'].shape == (128, 64, 1, 1) and sd['layer4.1.conv2.weight'].shape == (512, 512, 3, 3)
    with skip_random_init():
        sd50 = A.resnet50(172).state_dict()
    assert sd50['layer1.0.downsample.0.weight'].shape == (256, 64, 1, 1)          # Bottleneck: layer1 changes the width
    assert sd50['layer2.0.conv2.weight'].shape == (128, 128, 3, 3) and sd50['fc.weight'].shape == (172, 2048)


def test_bottleneck_stride_on_conv2():
    with skip_random_init():
        m = A.resnet50(10)
    b = m.layer2[0]
    assert b.conv1.stride == (1, 1) and b.conv2.stride == (2, 2) and b.conv3.stride == (1, 1) and b.downsample[0].stride == (2, 2)
    assert m.conv1.stride == (2, 2) and m.conv1.padding == (3, 3) and m.conv1.bias is None


def test_all_pretrained_models_freeze_rule(capsys):
    with skip_random_init():
        m = A.all_pretrained_models(17, name='resnet18')
    out = capsys.readouterr()
    assert 'WITHOUT ImageNet weights' in out.err                   # the loud warning
    assert '[Building resnet18]' in out.out and 'Freezing layers only till layer1' in out.out
    assert m.fc.out_features == 17 and m.fc.in_features == 512
    for k, p in m.named_parameters():
        frozen = k.startswith(('conv1.', 'bn1.', 'layer1.'))
        assert p.requires_grad == (not frozen), k
    assert m.frozen_stages() == 2
    m.train(True)
    assert m.bn1.training and m.layer1[0].bn1.training            # frozen, but still in training mode


def test_all_pretrained_models_loads_weights_except_fc():
    with skip_random_init():
        src = R.RefResNet('resnet18', 1000)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in src.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    with skip_random_init():
        m = A.all_pretrained_models(9, name='resnet18', weights=src.state_dict())
    sd = m.state_dict()
    for k, v in src.state_dict().items():
        if not k.startswith('fc.'):
            assert torch.equal(sd[k], v), k
    assert sd['fc.weight'].shape == (9, 512)
    with pytest.raises(KeyError):
        A.all_pretrained_models(9, name='resnet34', weights=src.state_dict())


def test_load_model_module_prefix(tmp_path):
    with skip_random_init():
        src = A.resnet18(11)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in src.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    plain, prefixed = str(tmp_path / 'a.pth'), str(tmp_path / 'b.pth')
    torch.save(src.state_dict(), plain)
    torch.save({'module.' + k: v for k, v in src.state_dict().items()}, prefixed)
    with skip_random_init():
        for path, n_class in ((plain, 11), (prefixed, 11), (prefixed, None)):
            m = A.load_model(path, name='resnet18', n_class=n_class, device='cpu')
            assert not m.training
            assert all(torch.equal(v, m.state_dict()[k]) for k, v in src.state_dict().items())


def test_step_lr_counts_like_the_reference():
    class Opt:
        param_groups = [{'lr': 0.5}]
    s = A.StepLR(Opt, step_size=2, gamma=0.1)
    seen = []
    for _ in range(5):
        s.step()
        seen.append(Opt.param_groups[0]['lr'])
    assert seen == pytest.approx([0.5, 0.5, 0.05, 0.05, 0.005])


# ---- train_model with a stub network ---------------------------------------------------------------------------------------------
class _Stub(nn.Module):
    def __init__(self, log, opt_ref):
        super().__init__()
        self.fc = nn.Linear(12, 4)
        self.log, self.opt_ref = log, opt_ref

    def forward(self, x):
        self.log.append(('train' if self.training else 'val', self.opt_ref[0].param_groups[0]['lr'], torch.is_grad_enabled()))
        return self.fc(x.flatten(1))


def _loader(seed, sizes):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n_img, n_obj in sizes:
        imgs = torch.randn(n_img, 3, 2, 2, generator=g)
        o2i = torch.randint(0, n_img, (n_obj,), generator=g)
        objs = torch.randint(0, 4, (n_obj,), generator=g)
        boxes = torch.rand(n_obj, 4, generator=g)
        out.append((imgs, objs, boxes, None, None, o2i, None, None))
    return out


def _run_train(keep_best, val_correct, capsys):
    log, opt_ref, snaps, calls = [], [None], [], [0]
    torch.manual_seed(0)
    model = _Stub(log, opt_ref)
    opt = opt_ref[0] = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9)
    train, val = _loader(1, [(2, 5), (3, 7)]), _loader(2, [(2, 3), (1, 1)])
    crit = nn.CrossEntropyLoss()

    def crop(imgs, boxes, o2i, size):
        assert size == 6 and not torch.is_grad_enabled()
        return imgs[o2i]

    def classify(outputs, labels, acc):
        assert not outputs.requires_grad
        acc = torch.zeros(3, dtype=torch.int64) if acc is None else acc
        if model.training:
            acc[0] += int((outputs.argmax(1) == labels).sum())
        else:                                   # scripted validation result: one batch carries the epoch's count
            calls[0] += 1
            if calls[0] % 2 == 0:
                acc[0] += val_correct[calls[0] // 2 - 1]
                snaps.append({k: v.clone() for k, v in model.state_dict().items()})
        return acc

    out = A.train_model(model, train, val, crit, opt, A.StepLR(opt, 2, 0.1), False, num_epochs=3, input_shape=6,
                        keep_best=keep_best, crop=crop, classify=classify)
    return out, log, snaps, capsys.readouterr().out, (train, val)


def test_train_model_schedule_and_bookkeeping(capsys):
    model, log, snaps, text, (train, val) = _run_train(False, [4, 1, 1], capsys)
    # scheduler.step() before an epoch's training: epochs 0 and 1 at the base rate, epoch 2 a tenth of it
    lrs = [lr for phase, lr, _ in log if phase == 'train']
    assert lrs == pytest.approx([0.1, 0.1, 0.1, 0.1, 0.01, 0.01])
    assert [g for phase, _, g in log if phase == 'train'] == [True] * 6 and [g for phase, _, g in log if phase == 'val'] == [False] * 6
    assert [p for p, _, _ in log] == ['train', 'train', 'val', 'val'] * 3
    # epoch_acc = correct / objects; the scripted validation counts over 4 objects
    accs = [float(v) for v in re.findall(r'val Loss: [\d.]+ Acc: ([\d.]+)', text)]
    assert accs == pytest.approx([1.0, 0.25, 0.25])
    assert 'Best val Acc: 1.0' in text
    # epoch_loss = sum of batch-MEAN losses / objects: recompute the last validation phase from the returned model
    with torch.no_grad():
        total = sum(float(nn.functional.cross_entropy(model.fc(b[0][b[5]].flatten(1)), b[1])) for b in val)
    losses = [float(v) for v in re.findall(r'val Loss: ([\d.]+)', text)]
    assert losses[-1] == pytest.approx(total / 4, abs=1e-4)
    # the reference's "best" weights alias the live tensors: the returned model is the LAST epoch's
    assert all(torch.equal(v, snaps[-1][k]) for k, v in model.state_dict().items())
    assert not all(torch.equal(v, snaps[0][k]) for k, v in model.state_dict().items())


def test_train_model_keep_best_copies(capsys):
    model, _, snaps, _, _ = _run_train(True, [4, 1, 1], capsys)
    assert all(torch.equal(v, snaps[0][k]) for k, v in model.state_dict().items())


# ---- the yardsticks against torch ----------------------------------------------------------------------------------------------
def ulps_of_operands(a, b, scale):
    """max |a - b| in units of the fp32 spacing at ``scale``, elementwise"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float((d / np.spacing(np.maximum(np.abs(scale), np.float32(1e-30)).astype(np.float32)).astype(np.float64)).max())


@pytest.mark.parametrize('n', [1, 63, 1027])
def test_sgd_ref_against_torch(n):
    """The separately rounded restatement against torch.optim.SGD, one step at a time from torch's own state.  DEVIATION from
    "within 2 ulp" read as spacings of the RESULT: the ulp is the spacing at the largest of the step's operands and result, |p|,
    |lr * buf| and |p - lr * buf|.  p - lr * buf cancels and torch's CPU kernel fuses the product into the subtraction, so the two differ by up to
    hundreds of spacings of a small result and by at most one spacing of the operands (both are printed)."""
    rs = np.random.RandomState(n)
    p0 = rs.randn(n).astype(np.float32)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([tp], lr=0.05, momentum=0.9)
    worst = at_result = 0.0
    for step in range(3):
        g = rs.randn(n).astype(np.float32)
        if step == 2:
            opt.param_groups[0]['lr'] = 0.005
        lr = opt.param_groups[0]['lr']
        p_before = tp.detach().numpy().copy()
        b_before = opt.state[tp]['momentum_buffer'].numpy().copy() if step else np.zeros(n, np.float32)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, buf = R.sgd_ref(p_before, g, b_before, lr, 0.9, step == 0)
        assert np.array_equal(buf, opt.state[tp]['momentum_buffer'].numpy())       # momentum * buf + 1 * g: no product to fuse
        scale = np.maximum(np.maximum(np.abs(p_before), np.abs(np.float32(lr) * buf)), np.abs(p))
        worst = max(worst, ulps_of_operands(p, tp.detach().numpy(), scale))
        at_result = max(at_result, ulps_of_operands(p, tp.detach().numpy(), p))
    print('n=%d: worst distance to torch.optim.SGD %.2f ulp of the operands (%.0f ulp of the result)' % (n, worst, at_result))
    assert worst <= 2


def _pool_cases():
    rs = np.random.RandomState(7)
    cases = []
    for (H, W) in [(1, 1), (2, 3), (7, 7), (8, 5), (13, 14)]:
        for NC in (1, 130):
            x = rs.randn(NC, H, W).astype(np.float32)
            cases.append(('random', x))
            cases.append(('negative', -np.abs(x) - 1))
            cases.append(('ties', np.round(x).astype(np.float32)))
            if H * W > 1:
                y = x.copy()
                y[0, H // 2, W // 2] = np.nan
                y[-1, 0, 0] = np.nan
                cases.append(('nan', y))
    return cases


def test_maxpool_ref_reproduces_torch():
    for tag, x in _pool_cases():
        t = torch.from_numpy(x.copy()).unsqueeze(0).requires_grad_(True)
        y = nn.functional.max_pool2d(t, 3, stride=2, padding=1)
        gy = torch.from_numpy(np.random.RandomState(1).randn(*y.shape).astype(np.float32))
        y.backward(gy)
        want, got = y.detach().numpy()[0], R.maxpool3s2_ref(x)
        assert got.shape == want.shape, tag
        assert np.array_equal(got, want, equal_nan=True), tag
        if tag == 'negative':
            assert (got < 0).all()                   # padding is -inf, not 0
        assert np.array_equal(R.maxpool3s2_bwd_ref(x, gy.numpy()[0]), t.grad.numpy()[0]), (tag, x.shape)


def test_ref_resnet_matches_itself_in_both_precisions():
    """the float32 run of the restatement (the error yardstick of the GPU tests) is close to its float64 run: the cases are well
    conditioned"""
    torch.manual_seed(0)
    m = R.RefResNet('resnet18', 7).eval()
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        a = m(x)
        b = m.double()(x.double())
    assert float((a.double() - b).abs().max() / b.abs().max()) < 1e-5


def test_classify_ref():
    logits = np.array([[1, 3, 3, 0], [np.nan, 5, np.nan, 9], [2, 2, 2, 2], [0, 1, 2, 3]], np.float32)
    target = np.array([1, 0, 0, 0], np.int64)
    preds, rec = R.classify_ref(logits, target, 0)
    assert preds.tolist() == [1, 0, 0, 3] and rec == (1, 1, 4)
    assert preds.tolist() == torch.max(torch.from_numpy(logits), 1)[1].tolist()
    assert R.classify_ref(logits, target, -1)[1] == (3, 4, 4)
