"""The Pillow-exact resize, without a GPU (tests/imageprep_ref.py, scene_generation_amd/imageprep.py, ops/imageprep.py): the integer
restatement of the arithmetic the kernels implement against ``PIL.Image.resize`` itself, the host packing, the command-line flags, the
untouched default path of ``fid._feed_dir`` and the wrapper's checks."""
import numpy as np
import pytest
import torch

import imageprep_ref as R
from scene_generation_amd import featsets as FS
from scene_generation_amd import fid as FID
from scene_generation_amd import imageprep as IP
from scene_generation_amd import inception as I
from scene_generation_amd import lpips as LP
from scene_generation_amd import ops

pytest.importorskip('PIL.Image')

# (source H x W) -> (OH, OW): the shapes of tests/test_gpu_imageprep.py and the two of the loader's own data
CASES = [((1, 1), (3, 4)), ((1, 9), (3, 4)), ((7, 5), (3, 4)), ((33, 17), (64, 64)), ((128, 300), (128, 128)), ((64, 64), (64, 64)),
         ((257, 1031), (8, 8)), ((3, 1500), (64, 64)), ((480, 640), (128, 128)), ((1, 1), (64, 64)), ((7, 5), (128, 128)),
         ((257, 1031), (3, 4)), ((9, 6), (1, 1)), ((427, 640), (128, 128)), ((500, 375), (299, 299))]


@pytest.mark.parametrize('filt', ['bilinear', 'bicubic'])
def test_restatement_equals_pillow(filt):
    rs = np.random.RandomState(3)
    for (H, W), size in CASES:
        a = R.random_image(rs, H, W)
        assert np.array_equal(R.resize(a, size, filt), R.pil_resize(a, size, filt)), (H, W, size, filt)


def test_restatement_equals_pillow_on_the_checkerboard_and_the_clamp_is_exercised():
    a = R.checkerboard(24, 24, 3)
    out, raw = R.resize(a, (64, 64), 'bicubic', unclipped=True)
    assert np.array_equal(out, R.pil_resize(a, (64, 64), 'bicubic'))
    assert all(r.min() < 0 and r.max() > 255 for r in raw)


def test_coefficients_follow_the_rules():
    xmin, count, k = R.coefficients(640, 128, 'bilinear')
    assert k.shape == (128, 11) and xmin[0] == 0 and (xmin + count).max() == 640
    assert (np.abs(k.sum(1) - (1 << 22)) <= k.shape[1]).all()                   # each row is a partition of one, to the rounding
    xmin, count, k = R.coefficients(17, 64, 'bicubic')
    assert k.shape == (64, 5) and count.min() >= 2 and count.max() <= 5 and (k < 0).any()
    xmin, count, k = R.coefficients(1031, 8, 'bicubic')
    assert k.shape[1] == 2 * 258 + 1 and count.max() > 500


def test_pack_images_offsets_and_tight_packing():
    rs = np.random.RandomState(0)
    shapes = [(1, 1), (7, 5), (2, 3), (33, 17), (1, 9)]
    arrays = [R.random_image(rs, h, w) for h, w in shapes]
    arrays[3] = np.asfortranarray(arrays[3])                                    # a non-contiguous input is packed in C order
    packed, table = IP.pack_images(arrays)
    assert packed.dtype == torch.uint8 and not packed.is_cuda and packed.dim() == 1
    assert packed.is_pinned() == torch.cuda.is_available()
    sizes = [h * w * 3 for h, w in shapes]
    assert any(s % 2 for s in sizes) and table.dtype == np.int64
    assert table[:, 0].tolist() == [0] + list(np.cumsum(sizes)[:-1]) and packed.numel() == sum(sizes)
    assert [tuple(r) for r in table[:, 1:].tolist()] == shapes
    assert any(int(o) % 2 for o in table[:, 0]) and any(int(o) % 4 for o in table[:, 0])
    for a, (off, h, w) in zip(arrays, table.tolist()):
        assert np.array_equal(packed[off:off + h * w * 3].numpy().reshape(h, w, 3), a)
    slot = torch.zeros(sum(sizes) + 100, dtype=torch.uint8)
    again, table2 = IP.pack_images(arrays, out=slot)
    assert again.data_ptr() == slot.data_ptr() and torch.equal(again, packed) and np.array_equal(table, table2)
    empty, t0 = IP.pack_images([])
    assert empty.numel() == 0 and t0.shape == (0, 3)
    with pytest.raises(ValueError):
        IP.pack_images([np.zeros((4, 4), np.uint8)])
    with pytest.raises(ValueError):
        IP.pack_images([np.zeros((4, 4, 3), np.float32)])
    with pytest.raises(ValueError):
        IP.pack_images(arrays, out=torch.zeros(10, dtype=torch.uint8))


@pytest.mark.parametrize('mod,required', [(I, ['--dir', 'd']), (FID, ['--real', 'r', '--fake', 'f']), (FS, ['--real', 'r', '--fake', 'f']),
                                          (LP, ['--dir0', 'a', '--dir1', 'b'])], ids=['inception', 'fid', 'featsets', 'lpips'])
def test_parsers_accept_the_flags_and_default_to_none(mod, required):
    p = mod.build_parser()
    args = p.parse_args(required)
    assert args.image_size is None and args.resize_filter == 'bilinear'
    args = p.parse_args(required + ['--image_size', '64,128', '--resize_filter', 'bicubic'])
    assert args.image_size == (64, 128) and args.resize_filter == 'bicubic'
    for bad in (['--image_size', '64'], ['--image_size', '0,4'], ['--image_size', '64,%d' % (ops.PIL_MAX_OUT + 1)], ['--resize_filter', 'box']):
        with pytest.raises(SystemExit):
            p.parse_args(required + bad)


def test_feed_dir_with_three_positional_arguments_chunks_as_before(tmp_path):
    from PIL import Image
    rs = np.random.RandomState(1)
    shapes = [(8, 8), (8, 8), (8, 8), (6, 9), (8, 8), (8, 8), (6, 9), (6, 9)]      # runs of 3 (split 2 + 1 by the batch), 1, 2, 2
    for i, (h, w) in enumerate(shapes):
        Image.fromarray(R.random_image(rs, h, w)).save(str(tmp_path / ('%02d.png' % i)))
    seen = []
    assert FID._feed_dir(lambda imgs: seen.append(tuple(imgs.shape)), str(tmp_path), 2) == 8
    assert seen == [(2, 3, 8, 8), (1, 3, 8, 8), (1, 3, 6, 9), (2, 3, 8, 8), (2, 3, 6, 9)]
    with pytest.raises(TypeError):
        FID._feed_dir(seen.append, str(tmp_path), 2, (4, 4))                    # the new parameters are keyword-only


def test_wrapper_checks_raise_before_touching_the_library(monkeypatch):
    from scene_generation_amd.ops import imageprep as OI

    def untouchable():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(OI, '_L', untouchable)
    monkeypatch.setattr(OI, '_call', lambda *a: untouchable())
    buf = torch.zeros(100, dtype=torch.uint8)
    good = np.array([[0, 4, 4], [48, 1, 2]], np.int64)
    with pytest.raises(ValueError, match='leaves the buffer'):
        ops.pil_resize(buf, np.array([[0, 4, 4], [53, 4, 4]]), (8, 8))          # offset + H W 3 = 101 > 100
    with pytest.raises(ValueError, match='leaves the buffer'):
        ops.pil_resize(buf, np.array([[-1, 4, 4]]), (8, 8))
    with pytest.raises(ValueError, match='outside 1\\.\\.'):
        ops.pil_resize(buf, np.array([[0, 0, 4]]), (8, 8))                      # H = 0
    with pytest.raises(ValueError, match='outside 1\\.\\.'):
        ops.pil_resize(buf, np.array([[0, 1, ops.PIL_MAX_IN + 1]]), (8, 8))
    with pytest.raises(ValueError, match='uint8'):
        ops.pil_resize(buf.float(), good, (8, 8))
    with pytest.raises(ValueError, match='filter'):
        ops.pil_resize(buf, good, (8, 8), 'lanczos')
    with pytest.raises(ValueError, match='target'):
        ops.pil_resize(buf, good, (ops.PIL_MAX_OUT + 1, 8))
    with pytest.raises(ValueError, match='target'):
        ops.pil_resize(buf, good, (8, 0))
    with pytest.raises(ValueError, match='table'):
        ops.pil_resize(buf, good[:, :2], (8, 8))
    with pytest.raises(ValueError, match='table'):
        ops.pil_resize(buf, good.astype(np.float64), (8, 8))
    with pytest.raises(ValueError, match='no CPU fallback'):
        ops.pil_resize(buf, good, (8, 8))                                       # everything in range, but on the host: still nothing is called


def test_limits_match_the_header():
    import re
    from scene_generation_amd import _hip
    src = open(_hip.HEADER).read()
    get = lambda name: int(re.search(r'#define\s+%s\s+(\d+)' % name, src).group(1))
    assert (get('SG_PIL_MAX_IN'), get('SG_PIL_MAX_OUT'), get('SG_PIL_MAX_IMAGES')) == (ops.PIL_MAX_IN, ops.PIL_MAX_OUT, ops.PIL_MAX_IMAGES)
    assert get('SG_PIL_TABLE_COLS') == ops.imageprep._TABLE_COLS
    assert ops.PIL_MAX_IN >= 8192 and ops.PIL_MAX_OUT >= 1024
    for name in ('sg_pil_resize_plan', 'sg_pil_resize'):
        assert name in _hip.PROTOS
