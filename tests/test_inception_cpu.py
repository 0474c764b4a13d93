"""The Inception score without a GPU: the network's layout against the plain restatement (keys, shapes, counts, strict loads), the
inference-only contract, the launch-plan query over every conv unit, the NumPy score restatement against scipy, the command line."""
import numpy as np
import pytest
import torch

import inception_ref as R
from scene_generation_amd import inception as I
from scene_generation_amd import ops


@pytest.fixture(scope='module')
def net():
    return I.InceptionV3()


def test_state_dict_matches_the_restatement(net):
    ref = R.RefInception3()
    sd, rsd = net.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in rsd.items()}
    assert len(sd) == 580
    assert sum(p.numel() for p in net.parameters()) == 27161264
    for k in ('Mixed_6c.branch7x7dbl_3.conv.weight', 'AuxLogits.conv1.bn.num_batches_tracked', 'Mixed_7c.branch3x3dbl_3b.bn.running_var',
              'AuxLogits.fc.bias', 'fc.weight'):
        assert k in sd
    assert tuple(sd['Mixed_6c.branch7x7dbl_3.conv.weight'].shape) == (160, 160, 1, 7)
    assert all(m.eps == 0.001 for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    # without the auxiliary head: its 6 conv-unit entries x 2 and the fc pair are gone
    assert len(I.InceptionV3(aux_logits=False).state_dict()) == 580 - 14


def test_strict_load_round_trip(net, tmp_path):
    ref = R.randomise(R.RefInception3(num_classes=7), 5)
    fresh = I.InceptionV3(num_classes=7)
    fresh.load_state_dict(ref.state_dict(), strict=True)
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, ref.state_dict()[k]), k
    path = str(tmp_path / 'inception.pth')
    torch.save({'module.' + k: v for k, v in ref.state_dict().items()}, path)
    loaded = I.load_inception(path, device='cpu')
    assert loaded.fc.out_features == 7 and not loaded.training
    for k, v in loaded.state_dict().items():
        assert torch.equal(v, ref.state_dict()[k]), k
    bad = dict(ref.state_dict())
    del bad['Mixed_5b.branch1x1.bn.running_mean']
    with pytest.raises(RuntimeError):
        fresh.load_state_dict(bad, strict=True)


def test_inference_only(net):
    assert not net.training and all(not m.training for m in net.modules())
    with pytest.raises(NotImplementedError, match='inference only'):
        net.train(True)
    with pytest.raises(NotImplementedError, match='inference only'):
        net.train()
    assert net.eval() is net and net.train(False) is net
    with pytest.raises(NotImplementedError):
        net.AuxLogits(torch.zeros(1, 768, 17, 17))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.zeros(1, 3, 75, 75))                               # a CPU tensor is an error, not a slow path
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 74, 74))


def test_fold_cache_is_dropped(net):
    net._fold_cache[1] = 'stale'
    net.load_state_dict(net.state_dict())
    assert not net._fold_cache
    net._fold_cache[1] = 'stale'
    net.float()
    assert not net._fold_cache


GRIDS = {'Mixed_5b': 35, 'Mixed_5c': 35, 'Mixed_5d': 35, 'Mixed_6a': 35, 'Mixed_6b': 17, 'Mixed_6c': 17, 'Mixed_6d': 17, 'Mixed_6e': 17,
         'Mixed_7a': 17, 'Mixed_7b': 8, 'Mixed_7c': 8}


def test_conv_units_and_plans_at_299(net):
    units = I.conv_units(299, 32)
    assert len(units) == 94
    names = [u['name'] for u in units]
    want = [n for n, m in net.named_modules() if isinstance(m, I.BasicConv2d) and not n.startswith('AuxLogits.')]
    assert sorted(names) == sorted(want) and len(set(names)) == 94
    assert I.conv_units(299, 32, net=net) == units                   # the shape-only skeleton walks like a real network
    for u in units:
        blk = u['name'].split('.')[0]
        if blk in GRIDS:
            assert u['H'] == u['W'] == GRIDS[blk], u
    assert [(u['H'], u['OH']) for u in units[:5]] == [(299, 149), (149, 147), (147, 147), (73, 73), (73, 71)]
    # every slice lies inside its block's output and the slices of a block tile it together with the pooled branch
    for blk, ctot in (('Mixed_5b', 256), ('Mixed_5c', 288), ('Mixed_5d', 288), ('Mixed_6a', 768), ('Mixed_6e', 768), ('Mixed_7a', 1280),
                      ('Mixed_7b', 2048), ('Mixed_7c', 2048)):
        sl = sorted((u['out_c0'], u['out_c0'] + u['Cout']) for u in units if u['name'].startswith(blk + '.') and u['out_ctot'] == ctot)
        assert sl and all(a[1] == b[0] for a, b in zip(sl, sl[1:])) and sl[0][0] == 0, (blk, sl)
        assert sl[-1][1] == ctot - ({'Mixed_6a': 288, 'Mixed_7a': 768}.get(blk, 0)), (blk, sl)
    plans = [I.unit_plan(u) for u in units]
    for u, p in zip(units, plans):
        K = u['C'] * u['KH'] * u['KW']
        assert p['tile'] in ops.RECT_TILES and (p['bm'], p['bn']) == {1: (64, 64), 2: (32, 128), 3: (64, 128)}[p['tile']]
        assert p['vec'] == (1 if K % 4 == 0 else 0)
        assert p['splits'] >= 1 and p['kchunk'] % 16 == 0 or p['splits'] == 1
        assert (p['splits'] - 1) * p['kchunk'] < K <= p['splits'] * p['kchunk']
        assert I.unit_plan(u, w_aligned16=False)['vec'] == 0
    assert {p['tile'] for p in plans} == set(ops.RECT_TILES)
    assert plans[0]['vec'] == 0 and plans[0]['tile'] == ops.RECT_TILE_32X128          # K = 27
    last = {u['name']: p for u, p in zip(units, plans) if u['name'].startswith(('Mixed_7b.', 'Mixed_7c.'))}
    assert all(p['splits'] > 1 for n, p in last.items() if n.endswith(('branch1x1', 'branch_pool', 'branch3x3_1', 'branch3x3dbl_1')))
    # one image: the 8 x 8 blocks are 64 pixels, every 1x1 of them splits
    one = {u['name']: I.unit_plan(u) for u in I.conv_units(299, 1) if u['name'].startswith('Mixed_7c.')}
    assert one['Mixed_7c.branch_pool']['splits'] == 8 and one['Mixed_7c.branch_pool']['kchunk'] == 256


def test_plan_rejects_bad_descs():
    with pytest.raises(RuntimeError):
        ops.conv2d_rect_plan(ops.rect_desc(1, 3, 9, 9, 4, 7, 7))       # 49 taps
    with pytest.raises(RuntimeError):
        ops.conv2d_rect_plan(ops.rect_desc(1, 3, 9, 9, 4, 3, 3, stride=3))


def _probs(n, classes, seed, zeros=False):
    rs = np.random.RandomState(seed)
    p = R.softmax_ref(3.0 * rs.randn(n, classes)).astype(np.float32)
    if zeros:
        p[::2, ::3] = 0.0
        p[1, :] = 0.0
        p[1, 2] = 1.0
    return p


@pytest.mark.parametrize('zeros', [False, True])
def test_score_restatement_against_scipy(zeros):
    entropy = pytest.importorskip('scipy.stats').entropy
    for n, classes in ((13, 5), (40, 1000)):
        p = _probs(n, classes, n + classes, zeros)
        for splits in (1, 5):
            a = R.inception_score_ref(p, splits)
            b = R.inception_score_ref(p, splits, entropy=entropy)
            assert np.allclose(a[0], b[0], rtol=1e-12, atol=0) and np.allclose(a[1], b[1], rtol=1e-9, atol=1e-13)
            assert np.allclose(a[2], b[2], rtol=1e-12, atol=0)
            # the reference's own lines (its ``preds`` is a float64 array the float32 rows are appended to)
            per, q = n // splits, p.astype(np.float64)
            scores = [np.exp(np.mean([entropy(r, np.mean(q[k * per:(k + 1) * per], axis=0)) for r in q[k * per:(k + 1) * per]]))
                      for k in range(splits)]
            assert np.allclose(a[0], np.mean(scores), rtol=1e-12) and np.allclose(a[1], np.std(scores), rtol=1e-9, atol=1e-13)


def test_score_restatement_tail_rows_and_empty_parts():
    p = _probs(13, 5, 1)
    m5, s5, parts = R.inception_score_ref(p, 5)
    assert len(parts) == 5 and (m5, s5) == R.inception_score_ref(p[:10], 5)[:2]      # 13 // 5 = 2: rows 10..12 are dropped
    assert (m5, s5) != R.inception_score_ref(p[1:11], 5)[:2]
    m, s, parts = R.inception_score_ref(p[:3], 5)                     # n < splits: every part is empty
    assert np.isnan(m) and np.isnan(s) and all(np.isnan(v) for v in parts)
    one_hot = np.eye(5, dtype=np.float32)
    assert abs(R.inception_score_ref(one_hot, 1)[0] - 5.0) < 1e-12   # distinct one-hot rows: the score is the class count
    assert abs(R.inception_score_ref(np.full((4, 5), 0.2, np.float32), 1)[0] - 1.0) < 1e-12


def test_pool_and_resize_restatements_against_torch():
    import torch.nn.functional as F
    rs = np.random.RandomState(0)
    x = rs.randn(2, 3, 9, 8)
    t = torch.from_numpy(x)
    assert np.array_equal(R.maxpool3s2v_ref(x), F.max_pool2d(t, 3, stride=2).numpy())
    assert np.allclose(R.avgpool3s1_ref(x), F.avg_pool2d(t, 3, stride=1, padding=1).numpy(), rtol=0, atol=1e-15)
    assert np.allclose(R.avgpool3s1_ref(x, False), F.avg_pool2d(t, 3, stride=1, padding=1, count_include_pad=False).numpy(), rtol=0,
                       atol=1e-15)
    for size in ((11, 13), (4, 5), (9, 8)):
        want = F.interpolate(t, size=size, mode='bilinear', align_corners=False).numpy()
        assert np.allclose(R.resize_bilinear_ref(x, *size), want, rtol=0, atol=1e-14)


def test_cli_parser_and_image_reader(tmp_path):
    a = I.build_parser().parse_args(['--dir', 'x', '--weights', 'w.pth'])
    assert (a.dir, a.weights, a.splits, a.batch_size) == ('x', 'w.pth', 5, 32)
    a = I.build_parser().parse_args(['--dir', 'x', '--splits', '2', '--batch_size', '8'])
    assert (a.weights, a.splits, a.batch_size) == (None, 2, 8)
    with pytest.raises(SystemExit):
        I.build_parser().parse_args([])
    Image = pytest.importorskip('PIL.Image')
    (tmp_path / 'a' / 'b').mkdir(parents=True)
    px = np.zeros((4, 6, 3), np.uint8)
    px[..., 0], px[..., 2] = 255, 51
    Image.fromarray(px).save(str(tmp_path / 'a' / 'b' / 'z.png'))
    Image.fromarray(px).save(str(tmp_path / 'a' / 'y.png'))
    (tmp_path / 'a' / 'notes.txt').write_text('no image')
    found = I.find_images(str(tmp_path))
    assert [p[len(str(tmp_path)):] for p in found] == ['/a/y.png', '/a/b/z.png']
    img = I.read_image(found[0])
    assert tuple(img.shape) == (3, 4, 6) and img.dtype == torch.float32
    assert float(img[0].min()) == 1.0 and float(img[1].max()) == -1.0 and abs(float(img[2, 0, 0]) - (-0.6)) < 1e-6
    with pytest.raises(SystemExit):
        I.main(['--dir', str(tmp_path / 'a' / 'none')])
