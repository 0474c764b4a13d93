"""The Frechet Inception Distance without a GPU: ``frechet_distance`` against closed forms, the exact nuclear-norm form and scipy's
matrix square root; the statistics file; the argument errors of the two C entry points; the checkpoint bookkeeping; the FID form of
the network's layout.

Bound of every distance check: 1e-12 (tr S1 + tr S2).  The symmetric eigen-solver's backward error is of order D 2^-52 (1.4e-14 at
D = 64, 5.7e-14 at D = 256) relative to the spectrum; the bound leaves about 70 x over it at D = 64."""
import ctypes

import numpy as np
import pytest
import torch

import fid_ref as FR
import inception_ref as R
from scene_generation_amd import _hip, fid
from scene_generation_amd import inception as I

RTOL = 1e-12


def _orth(rs, d):
    q, r = np.linalg.qr(rs.randn(d, d))
    return q * np.sign(np.diag(r))


@pytest.mark.parametrize('zeros', [0, 20])
def test_frechet_distance_closed_form(zeros):
    """commuting covariances S1 = Q diag(a) Q^T, S2 = Q diag(b) Q^T: tr (S1 S2)^1/2 = sum sqrt(a_i b_i)"""
    rs = np.random.RandomState(7 + zeros)
    d = 64
    q = _orth(rs, d)
    a, b = 0.1 + rs.rand(d) * 3, 0.1 + rs.rand(d) * 3
    a[rs.permutation(d)[:zeros]] = 0.0
    s1, s2 = (q * a) @ q.T, (q * b) @ q.T
    mu1, mu2 = rs.randn(d), rs.randn(d)
    want = float((mu1 - mu2) @ (mu1 - mu2)) + a.sum() + b.sum() - 2.0 * np.sqrt(a * b).sum()
    got = fid.frechet_distance(mu1, s1, mu2, s2)
    scale = a.sum() + b.sum()
    print('closed form, %d zero eigenvalues: got %.17g want %.17g  err / scale %.2e' % (zeros, got, want, abs(got - want) / scale))
    assert isinstance(got, float) and abs(got - want) <= RTOL * scale
    # the roles swapped: the truncated side is now S2
    assert abs(fid.frechet_distance(mu2, s2, mu1, s1) - want) <= RTOL * scale


@pytest.mark.parametrize('shape', [(64, 40, 50), (256, 100, 300), (256, 300, 100)], ids=lambda s: '%d_%d_%d' % s)
def test_frechet_distance_rank_deficient_against_nuclear_norm(shape):
    d, n1, n2 = shape
    rs = np.random.RandomState(d + n1)
    f1, f2 = FR.relu_gauss(rs, n1, d), FR.relu_gauss(rs, n2, d) * np.float32(1.1)
    want, scale = FR.fid_nuclear(f1, f2)
    (mu1, s1), (mu2, s2) = FR.stats(f1), FR.stats(f2)
    assert np.linalg.matrix_rank(s1) < d or np.linalg.matrix_rank(s2) < d
    got = fid.frechet_distance(mu1, s1, mu2, s2)
    print('nuclear %s: got %.17g want %.17g  err / scale %.2e' % (shape, got, want, abs(got - want) / scale))
    assert abs(got - want) <= RTOL * scale
    assert want > 1e-3 * scale                                   # a distance that is not all cancellation


def test_frechet_distance_full_rank_against_sqrtm():
    sqrtm = pytest.importorskip('scipy.linalg').sqrtm
    rs = np.random.RandomState(3)
    d, n = 64, 512
    f1, f2 = FR.relu_gauss(rs, n, d), FR.relu_gauss(rs, n, d) * np.float32(1.1)
    (mu1, s1), (mu2, s2) = FR.stats(f1), FR.stats(f2)
    assert np.linalg.matrix_rank(s1) == d and np.linalg.matrix_rank(s2) == d
    root = sqrtm(s1 @ s2)
    want = float((mu1 - mu2) @ (mu1 - mu2) + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(root).real)
    scale = np.trace(s1) + np.trace(s2)
    nuclear = FR.fid_nuclear(f1, f2)[0]
    print('sqrtm: reference %.17g  nuclear %.17g  (apart %.2e of scale)' % (want, nuclear, abs(want - nuclear) / scale))
    assert abs(want - nuclear) <= RTOL * scale                   # the reference itself is good here (full rank)
    got = fid.frechet_distance(mu1, s1, mu2, s2)
    assert abs(got - want) <= RTOL * scale


def test_frechet_distance_structure_and_errors():
    rs = np.random.RandomState(11)
    f1, f2 = FR.relu_gauss(rs, 30, 48), FR.relu_gauss(rs, 70, 48)
    (mu1, s1), (mu2, s2) = FR.stats(f1), FR.stats(f2)
    scale = np.trace(s1) + np.trace(s2)
    assert abs(fid.frechet_distance(mu1, s1, mu1, s1)) <= RTOL * 2 * np.trace(s1)
    assert abs(fid.frechet_distance(mu2, s2, mu2, s2)) <= RTOL * 2 * np.trace(s2)
    a, b = fid.frechet_distance(mu1, s1, mu2, s2), fid.frechet_distance(mu2, s2, mu1, s1)
    assert abs(a - b) <= RTOL * scale and a > 0
    assert fid.frechet_distance(mu1, s1, mu2, s2, root1=fid.psd_sqrt(s1)) == a        # the cached root is the same computation
    with pytest.raises(ValueError):
        fid.frechet_distance(mu1, s1, mu2[:-1], s2)
    with pytest.raises(ValueError):
        fid.frechet_distance(mu1, s1[:-1], mu2, s2)


def test_statistics_file_round_trip(tmp_path):
    rs = np.random.RandomState(2)
    mu, sigma = FR.stats(FR.relu_gauss(rs, 20, 12))
    path = str(tmp_path / 'stats.npz')
    np.savez(path, mu=mu, sigma=sigma)                           # what pytorch-fid writes: mu and sigma only
    m2, s2 = fid.load_statistics(path)
    assert m2.dtype == np.float64 and np.array_equal(m2, mu) and np.array_equal(s2, sigma)
    np.savez(path, mu=mu.astype(np.float32), sigma=sigma.astype(np.float32), n=np.int64(20))
    m3, s3 = fid.load_statistics(path)
    assert m3.dtype == np.float64 and s3.dtype == np.float64 and tuple(s3.shape) == (12, 12)
    np.savez(path, mu=mu, sigma=sigma[:5])
    with pytest.raises(ValueError):
        fid.load_statistics(path)


def test_moment_entry_points_reject_bad_arguments():
    """negative codes with the function's name, before anything touches a device"""
    L = _hip.lib()
    buf = np.zeros(64, np.float64)
    pd = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    odd = ctypes.cast(buf.ctypes.data + 4, ctypes.POINTER(ctypes.c_double))
    x = np.zeros(64, np.float32).ctypes.data
    upd, fin = L.sg_fid_moments_update, L.sg_fid_moments_finalize
    for args in ((None, 4, 4, 4, pd, pd, None), (x, 4, 4, 4, None, pd, None), (x, 4, 4, 4, pd, None, None),      # null pointers
                 (x, 4, 4, 3, pd, pd, None), (x, 4, 0, 4, pd, pd, None), (x, -1, 4, 4, pd, pd, None),            # ldx < D, D < 1, rows < 0
                 (x, 4, 4, 4, odd, pd, None), (x, 4, 4, 4, pd, odd, None)):                                       # misaligned doubles
        assert upd(*args) < 0 and 'sg_fid_moments_update' in _hip.last_error(), args
    assert upd(None, 0, 4, 4, pd, pd, None) == 0                 # no rows: nothing to launch, x is not looked at
    for args in ((pd, pd, 1, 4, pd, pd, None), (pd, pd, 0, 4, pd, pd, None), (pd, pd, -5, 4, pd, pd, None),      # n < 2
                 (None, pd, 9, 4, pd, pd, None), (pd, None, 9, 4, pd, pd, None), (pd, pd, 9, 4, None, pd, None),
                 (pd, pd, 9, 4, pd, None, None), (pd, pd, 9, 0, pd, pd, None), (pd, pd, 9, 4, pd, odd, None)):
        assert fin(*args) < 0 and 'sg_fid_moments_finalize' in _hip.last_error(), args
    assert 'n >= 2' in (fin(pd, pd, 1, 4, pd, pd, None), _hip.last_error())[1]


def test_save_checkpoint_val_fid_keys(tmp_path):
    from scene_generation_amd.args import parser
    from scene_generation_amd.synthetic import make_vocab
    from scene_generation_amd.trainer import Trainer
    argv = ['--image_size', '32,32', '--batch_size', '3', '--vgg_features_weight', '0', '--n_downsample_global', '2',
            '--gconv_hidden_dim', '64', '--gconv_num_layers', '3', '--mask_size', '8', '--ndf', '8', '--ndf_mask', '8', '--crop_size', '16',
            '--d_obj_arch', 'C4-8-2,C4-16-2', '--pool_size', '2']
    saved = {}
    for name, val in (('three', (0.5, 1.5, 0.1)), ('none', (0.5, 1.5, 0.1, None)), ('fid', (0.5, 1.5, 0.1, 42.25))):
        args = parser.parse_args(argv + ['--output_dir', str(tmp_path / name)])
        tr = Trainer(args, make_vocab(12, 4, 35), device='cpu')
        scalars = []
        tr.writer = type('W', (), {'add_scalar': lambda self, tag, v, i: scalars.append(tag)})()
        ck = {}
        path = tr.save_checkpoint(ck, 10, args, 0, val_results=val)
        if name == 'fid':
            tr.save_checkpoint(ck, 20, args, 0, val_results=(0.5, 1.6, 0.1, 40.0))
        saved[name] = (torch.load(path, weights_only=False), scalars)
    assert sorted(saved['none'][0]) == sorted(saved['three'][0]) and saved['none'][1] == saved['three'][1]
    assert 'val_fid' not in saved['three'][0] and 'checkpoint/val_fid' not in saved['three'][1]
    assert sorted(saved['fid'][0]) == sorted(list(saved['three'][0]) + ['val_fid'])
    assert saved['fid'][0]['val_fid'] == [42.25, 40.0] and saved['fid'][1].count('checkpoint/val_fid') == 2
    assert saved['fid'][0]['val_inception'] == [1.5, 1.6] and saved['fid'][0]['best_t'] == [10]      # "best" stays keyed on the Inception mean


def test_fid_form_of_the_network_layout(tmp_path):
    """the flag changes four kinds of branch pool and nothing else; a 1008-class file loads, strictly, into the FID form"""
    with torch.device('meta'):
        plain, fidnet = I.InceptionV3(), I.InceptionV3(num_classes=1008, aux_logits=False, fid_variant=True)
    pools = {n: getattr(fidnet, n).pool for n in I._BLOCKS if hasattr(getattr(fidnet, n), 'pool')}
    assert pools == dict({n: 'avgpool3s1x' for n in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d', 'Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e',
                                                      'Mixed_7b')}, Mixed_7c='maxpool3s1')
    assert all(getattr(plain, n).pool == 'avgpool' for n in pools) and not plain.fid_variant and fidnet.fid_variant
    assert I.conv_units(299, 2, net=fidnet) == I.conv_units(299, 2, net=plain) == I.conv_units(299, 2)      # the trace walks both
    ref = R.randomise(FR.RefFidInception3(), 5)
    sd = ref.state_dict()
    assert list(sd) == list(I.InceptionV3(num_classes=1008, aux_logits=False, fid_variant=True).state_dict())
    path = str(tmp_path / 'pt_inception.pth')
    torch.save(sd, path)
    net = I.load_inception(path, device='cpu')
    assert net.fid_variant and net.fc.out_features == 1008 and not hasattr(net, 'AuxLogits')
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    torch.save(dict(sd, **{'AuxLogits.fc.bias': torch.zeros(1008)}), path)              # the FID file has no auxiliary head: strict
    with pytest.raises(RuntimeError):
        I.load_inception(path, device='cpu')
    torch.save(R.RefInception3(num_classes=1000).state_dict(), path)                    # torchvision's file: as before
    net = I.load_inception(path, device='cpu')
    assert not net.fid_variant and hasattr(net, 'AuxLogits') and net.Mixed_7c.pool == 'avgpool'


def test_cli_parser():
    a = fid.build_parser().parse_args(['--weights', 'w.pth', '--real', 'stats.npz', '--fake', 'dir'])
    assert (a.weights, a.real, a.fake, a.save_stats, a.batch_size) == ('w.pth', 'stats.npz', 'dir', None, 32)
    with pytest.raises(SystemExit):
        fid.build_parser().parse_args(['--real', 'x'])
    from scene_generation_amd import sample
    assert sample.make_parser().parse_args(['--checkpoint', 'c']).fid_stats is None
    assert sample.make_parser().parse_args(['--checkpoint', 'c', '--fid_stats', 's.npz']).fid_stats == 's.npz'
