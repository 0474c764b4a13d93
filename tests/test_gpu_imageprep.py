"""The Pillow-exact resize on the GPU (csrc/imageprep.hip, ops/imageprep.py, scene_generation_amd/imageprep.py).

Every comparison is bit equality: the resized bytes against ``PIL.Image.resize`` itself, the normalised floats against
``inception.read_image``'s expression on those bytes, every output between guard bytes / guard floats.  The references are computed
once per (target, filter) and shared.  The tree only: no reference checkout."""
import os

import numpy as np
import pytest
import torch

import imageprep_ref as R
from scene_generation_amd import _hip
from scene_generation_amd import featsets as FS
from scene_generation_amd import fid as FID
from scene_generation_amd import imageprep as IP
from scene_generation_amd import inception as I
from scene_generation_amd import lpips as LP
from scene_generation_amd import ops

pytestmark = pytest.mark.gpu
pytest.importorskip('PIL.Image')
DEV = 'cuda:0'
GUARD8, GUARDF = 0xA5, -777.0
NG8 = 5             # guard bytes on each side of y8: the output then starts at an odd address


def N(t):
    return t.detach().cpu().numpy()


def run(arrays, size, filt, want='both', packed_table=None):
    """ops.pil_resize of the packed ``arrays`` into guarded outputs -> (y8 uint8 [n, OH, OW, 3] or None, y float32 [n, 3, OH, OW] or None)"""
    packed, table = packed_table if packed_table is not None else IP.pack_images(arrays)
    n, (OH, OW) = table.shape[0], size
    dev = packed.to(DEV)
    b8 = torch.full((n * OH * OW * 3 + 2 * NG8,), GUARD8, dtype=torch.uint8, device=DEV)
    bf = torch.full((n * 3 * OH * OW + 2,), GUARDF, dtype=torch.float32, device=DEV)
    y8 = b8[NG8:b8.numel() - NG8].view(n, OH, OW, 3) if want in ('both', 'u8') else None
    y = bf[1:-1].view(n, 3, OH, OW) if want in ('both', 'f32') else None
    got = ops.pil_resize(dev, table, size, filt, out=y if y is not None else False, out_u8=y8)
    if want == 'both':
        assert got[0] is y and got[1] is y8
    else:
        assert got is (y if want == 'f32' else y8)
    assert (b8[:NG8] == GUARD8).all() and (b8[-NG8:] == GUARD8).all() and bf[0].item() == GUARDF and bf[-1].item() == GUARDF
    if y8 is None:
        assert (b8 == GUARD8).all()
    if y is None:
        assert (bf == GUARDF).all()
    return (N(y8) if y8 is not None else None), (N(y) if y is not None else None)


# =====================================================================================================================================
# 1. one ragged batch
# =====================================================================================================================================
def lds_chunk():
    """SG_PIL_LDS_CHUNK (include/sg2im_hip.h): the bytes of a source row the horizontal kernel stages in LDS at once"""
    return _hip.CONST['SG_PIL_LDS_CHUNK']


def ragged_batch(size):
    rs = np.random.RandomState(11)
    long_w = lds_chunk() // 3 + 135                  # a row of 3 long_w bytes > SG_PIL_LDS_CHUNK: a tile's taps span more than one chunk
    assert 3 * long_w > lds_chunk()
    # an image of an odd byte count first, so that the even-sized ones after it all start at odd offsets
    shapes = [(1, 1),
              (128, 300),                            # to 128 x 128 the vertical pass is skipped
              (40, size[1]),                         # the horizontal pass is skipped: the vertical one reads the packed source itself
              size,                                  # already at the target size: both are skipped
              (3, long_w),                           # longer than the LDS chunk
              (480, 640),                            # the workload's own shape
              (1, 9), (7, 5),                        # with 1 x 1: clamped xmin / xmax at both borders, fewer taps than ksize
              (33, 17),                              # enlargement: fs = 1
              (257, 1031)]                           # to 8 x 8 about 129-fold: hundreds of taps
    arrays = [R.random_image(rs, h, w) for h, w in shapes]
    arrays.insert(CHECKER, R.checkerboard(24, 24, 3))      # 0 / 255 edges: the bicubic filter leaves 0..255 on both sides
    return arrays


CHECKER = 2         # position of the checkerboard in the ragged batch
TARGETS = [(3, 4), (64, 64), (128, 128), (8, 8)]
_REF = {}


def reference(size, filt):
    key = (size, filt)
    if key not in _REF:
        arrays = ragged_batch(size)
        want8 = np.stack([R.pil_resize(a, size, filt) for a in arrays])
        want8.setflags(write=False)
        _REF[key] = (arrays, want8, N(R.normalise(want8)))
    return _REF[key]


@pytest.mark.parametrize('filt', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('size', TARGETS, ids=lambda s: '%dx%d' % s)
def test_ragged_batch_equals_pillow(size, filt):
    arrays, want8, want = reference(size, filt)
    packed, table = IP.pack_images(arrays)
    assert sum(int(o) % 2 for o in table[:, 0]) > len(arrays) // 2 and len({int(o) % 4 for o in table[:, 0]}) >= 3     # most offsets are odd
    if filt == 'bicubic' and size == (64, 64):       # the clamp is really exercised: the unclipped values leave 0..255 on both sides
        raw = R.resize(arrays[CHECKER], size, filt, unclipped=True)[1]
        assert all(r.min() < 0 and r.max() > 255 for r in raw)
    y8, y = run(arrays, size, filt, packed_table=(packed, table))
    for i, a in enumerate(arrays):
        bad = np.argwhere(y8[i] != want8[i])
        assert bad.size == 0, ('image %d %s -> %s %s: %d bytes differ, first at %s: got %d, Pillow %d'
                               % (i, a.shape, size, filt, len(bad), bad[0], y8[i][tuple(bad[0])], want8[i][tuple(bad[0])]))
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))


def test_read_image_expression_on_every_byte_value():
    a = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)
    y8, y = run([a], (16, 16), 'bilinear')           # both passes skipped: the bytes themselves, every value once per channel
    assert np.array_equal(y8[0], a)
    want = (torch.from_numpy(a.astype(np.float32)).permute(2, 0, 1) / 255.0 - 0.5) / 0.5
    assert np.array_equal(y[0].view(np.uint32), N(want).view(np.uint32))


# =====================================================================================================================================
# 2. batch sizes: an image's result does not depend on its position or its neighbours
# =====================================================================================================================================
@pytest.mark.parametrize('filt', ['bilinear', 'bicubic'])
def test_batch_sizes_and_positions(filt):
    rs = np.random.RandomState(5)
    size = (24, 40)
    kinds = [R.random_image(rs, h, w) for h, w in ((7, 5), (33, 17), (61, 97), (24, 40), (24, 9), (50, 40))]
    alone = [run([a], size, filt) for a in kinds]                               # N = 1
    for a, (y8, y) in zip(kinds, alone):
        assert np.array_equal(y8[0], R.pil_resize(a, size, filt))
    order = [int(i) for i in rs.randint(0, len(kinds), size=33)]
    order[:len(kinds)] = range(len(kinds))
    y8, y = run([kinds[i] for i in order], size, filt)                          # N = 33, sizes repeating
    for pos, i in enumerate(order):
        assert np.array_equal(y8[pos], alone[i][0][0]) and np.array_equal(y[pos].view(np.uint32), alone[i][1][0].view(np.uint32)), (pos, i)


# =====================================================================================================================================
# 3. output selection, repeats
# =====================================================================================================================================
def test_output_selection_and_repeats():
    arrays = ragged_batch((64, 64))[:8]
    both = run(arrays, (64, 64), 'bicubic', 'both')
    only8 = run(arrays, (64, 64), 'bicubic', 'u8')
    onlyf = run(arrays, (64, 64), 'bicubic', 'f32')
    again = run(arrays, (64, 64), 'bicubic', 'both')
    assert only8[1] is None and onlyf[0] is None
    assert np.array_equal(only8[0], both[0]) and np.array_equal(onlyf[1].view(np.uint32), both[1].view(np.uint32))
    assert np.array_equal(again[0], both[0]) and np.array_equal(again[1].view(np.uint32), both[1].view(np.uint32))
    packed, table = IP.pack_images(arrays)
    fresh = ops.pil_resize(packed.to(DEV), table, (64, 64), 'bicubic')          # the outputs allocated by the wrapper
    assert fresh.dtype == torch.float32 and np.array_equal(N(fresh).view(np.uint32), both[1].view(np.uint32))
    assert np.array_equal(N(IP.resize_batch(arrays, (64, 64), 'bicubic', DEV)).view(np.uint32), both[1].view(np.uint32))
    empty = ops.pil_resize(torch.zeros(4, dtype=torch.uint8, device=DEV), np.zeros((0, 3), np.int64), (8, 8))
    assert tuple(empty.shape) == (0, 3, 8, 8)


def test_wrapper_refuses_before_any_launch():
    buf = torch.zeros(100, dtype=torch.uint8, device=DEV)
    calls = ops.CALLS[0]
    for table, size, filt in ((np.array([[53, 4, 4]]), (8, 8), 'bilinear'), (np.array([[0, 0, 4]]), (8, 8), 'bilinear'),
                              (np.array([[0, 4, 4]]), (8, 8), 'box'), (np.array([[0, 4, 4]]), (8, ops.PIL_MAX_OUT + 1), 'bilinear')):
        with pytest.raises(ValueError):
            ops.pil_resize(buf, table, size, filt)
    with pytest.raises(ValueError):
        ops.pil_resize(buf, np.array([[0, 4, 4]]), (8, 8), out=torch.empty(1, 3, 8, 9, device=DEV))
    with pytest.raises(ValueError):
        ops.pil_resize(buf, torch.tensor([[0, 4, 4]], device=DEV), (8, 8))      # a device table cannot be checked: refused
    assert ops.CALLS[0] == calls


# =====================================================================================================================================
# 4. the feeder
# =====================================================================================================================================
FEED_SHAPES = [(40, 52), (33, 17), (32, 32), (40, 52), (61, 97), (33, 17), (33, 17), (32, 32), (61, 97), (40, 52), (40, 52)]


def _write_dir(root, shapes, seed):
    from PIL import Image
    rs = np.random.RandomState(seed)
    root.mkdir()
    arrays = [R.random_image(rs, h, w) for h, w in shapes]
    for i, a in enumerate(arrays):
        Image.fromarray(a).save(str(root / ('%02d.png' % i)))
    return arrays


@pytest.mark.parametrize('filt', ['bilinear', 'bicubic'])
def test_feeder_batches_in_path_order(tmp_path, filt):
    arrays = _write_dir(tmp_path / 'd', FEED_SHAPES, 2)
    feeder = IP.ImageDirFeeder(str(tmp_path / 'd'), 4, (32, 32), filt, DEV, workers=3)
    assert len(feeder) == 11 and feeder.paths == I.find_images(str(tmp_path / 'd'))
    batches = [N(b) for b in feeder]
    assert [b.shape for b in batches] == [(4, 3, 32, 32), (4, 3, 32, 32), (3, 3, 32, 32)]
    want = N(R.normalise(np.stack([R.pil_resize(a, (32, 32), filt) for a in arrays])))
    assert np.array_equal(np.concatenate(batches).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.concatenate([N(b) for b in feeder]), np.concatenate(batches))      # a second pass over the same feeder


def test_feed_dir_with_and_without_image_size(tmp_path):
    _write_dir(tmp_path / 'd', FEED_SHAPES, 2)
    seen = []
    assert FID._feed_dir(lambda x: seen.append((x.is_cuda, tuple(x.shape))), str(tmp_path / 'd'), 4, image_size=(32, 32), device=DEV) == 11
    assert seen == [(True, (4, 3, 32, 32)), (True, (4, 3, 32, 32)), (True, (3, 3, 32, 32))]
    seen = []
    FID._feed_dir(lambda x: seen.append(tuple(x.shape[2:])), str(tmp_path / 'd'), 4)            # as before: one chunk per run of equal sizes
    assert seen == [(40, 52), (33, 17), (32, 32), (40, 52), (61, 97), (33, 17), (32, 32), (61, 97), (40, 52)]


# =====================================================================================================================================
# 5. the command lines
# =====================================================================================================================================
def _resized_copy(src, dst, size, filt):
    from PIL import Image
    dst.mkdir()
    for p in I.find_images(str(src)):
        Image.fromarray(R.pil_resize(IP.decode(p), size, filt)).save(str(dst / os.path.basename(p)))


@pytest.fixture()
def dirs(tmp_path):
    mixed = [(40, 52), (33, 17), (32, 32), (61, 97), (40, 52)]
    _write_dir(tmp_path / 'real', mixed, 5)
    _write_dir(tmp_path / 'fake', mixed[::-1], 6)
    for name in ('real', 'fake'):
        _resized_copy(tmp_path / name, tmp_path / (name + '32'), (32, 32), 'bilinear')
    return tmp_path


def test_fid_and_featsets_command_lines(dirs, capsys):
    flag = ['--image_size', '32,32', '--batch_size', '8']
    a = FID.main(['--real', str(dirs / 'real'), '--fake', str(dirs / 'fake')] + flag)
    out_a = capsys.readouterr().out.strip().splitlines()[-1]
    b = FID.main(['--real', str(dirs / 'real32'), '--fake', str(dirs / 'fake32'), '--batch_size', '8'])
    out_b = capsys.readouterr().out.strip().splitlines()[-1]
    assert a == b and out_a == out_b and out_a.startswith('FID ') and np.isfinite(a)
    kid = ['--kid_subsets', '3', '--seed', '1']
    c = FS.main(['--real', str(dirs / 'real'), '--fake', str(dirs / 'fake')] + flag + kid)
    out_c = capsys.readouterr().out.strip().splitlines()[-3:]
    d = FS.main(['--real', str(dirs / 'real32'), '--fake', str(dirs / 'fake32'), '--batch_size', '8'] + kid)
    out_d = capsys.readouterr().out.strip().splitlines()[-3:]
    assert c == d and out_c == out_d == FS.format_lines(c) and c['real'] == c['fake'] == 5


def test_lpips_and_inception_command_lines(dirs, capsys):
    a = LP.main(['--dir0', str(dirs / 'real'), '--dir1', str(dirs / 'fake'), '--image_size', '32,32', '--batch_size', '8'])
    out_a = capsys.readouterr().out.strip().splitlines()[-1]
    b = LP.main(['--dir0', str(dirs / 'real32'), '--dir1', str(dirs / 'fake32'), '--batch_size', '8'])
    out_b = capsys.readouterr().out.strip().splitlines()[-1]
    assert a == b and out_a == out_b and out_a.startswith('Diversity ') and a[0] > 0
    c = I.main(['--dir', str(dirs / 'real'), '--image_size', '32,32', '--batch_size', '8', '--splits', '1'])
    out_c = capsys.readouterr().out.strip().splitlines()[-1]
    d = I.main(['--dir', str(dirs / 'real32'), '--batch_size', '8', '--splits', '1'])
    out_d = capsys.readouterr().out.strip().splitlines()[-1]
    assert c == d and out_c == out_d and out_c.startswith('Inception ')
