"""The shared base of the evaluation metrics (``evalkit``, and the two Inception helpers every metric object goes through): the
buffer growth rule, the chunker over stored image sizes, state_dict loading, the choice of network from ``weights``, and the import
order the modules keep."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from scene_generation_amd import evalkit as E
from scene_generation_amd import inception as I


# ---- grow_rows --------------------------------------------------------------------------------------------------------------------------
def test_grow_rows_capacities_and_held_rows():
    buf, count, caps = None, 0, []
    want = torch.arange(20 * 3, dtype=torch.float32).view(20, 3)
    for step in range(4):                                       # rows arrive 5, 5, 5, 5 into an empty buffer
        grown = E.grow_rows(buf, count, 5, 8, (3,), torch.float32, 'cpu')
        assert (grown is buf) == (step == 2)                    # 15 rows fit the 16 of step 1: the same object comes back
        buf = grown
        buf[count:count + 5] = want[count:count + 5]
        count += 5
        caps.append(buf.size(0))
        assert torch.equal(buf[:count], want[:count])           # held rows survive every growth
    assert caps == [8, 16, 16, 32]
    assert buf.dtype == torch.float32 and tuple(buf.shape[1:]) == (3,)


def test_grow_rows_from_a_held_capacity_and_without_a_tail():
    buf = torch.arange(4, dtype=torch.float64)
    grown = E.grow_rows(buf, 4, 5, 1, (), torch.float64, 'cpu')             # 9 rows from capacity 4, first_cap 1: 4 -> 8 -> 16
    assert tuple(grown.shape) == (16,) and grown.dtype == torch.float64 and torch.equal(grown[:4], buf)
    assert E.grow_rows(buf, 2, 2, 1, (), torch.float64, 'cpu') is buf
    assert E.grow_rows(None, 0, 0, 8, (), torch.float64, 'cpu') is None     # nothing asked of nothing


# ---- stored_size_chunks -------------------------------------------------------------------------------------------------------------------
_SIZES = {'A': (4, 6), 'B': (5, 3)}


def _write_dir(root, pattern, seed):
    Image = pytest.importorskip('PIL.Image')
    root.mkdir()
    rs = np.random.RandomState(seed)
    for i, c in enumerate(pattern):
        Image.fromarray(rs.randint(0, 256, _SIZES[c] + (3,)).astype(np.uint8)).save(str(root / ('%02d.png' % i)))
    return E.find_images(str(root))


def test_stored_size_chunks_one_directory(tmp_path):
    paths = _write_dir(tmp_path / 'd', 'AAABBAAA', 0)
    assert [p[-6:] for p in paths] == ['%02d.png' % i for i in range(8)]
    chunks = list(E.stored_size_chunks([paths], 2))
    assert all(isinstance(c, tuple) and len(c) == 1 for c in chunks)
    assert [c[0].size(0) for c in chunks] == [2, 1, 2, 2, 1]
    flat = [img for c in chunks for img in c[0]]                # the files in find_images order, each what read_image gives
    assert len(flat) == 8 and all(torch.equal(img, E.read_image(p)) for img, p in zip(flat, paths))
    assert list(E.stored_size_chunks([[]], 2)) == []


def test_stored_size_chunks_two_directories(tmp_path):
    a, b = _write_dir(tmp_path / 'a', 'AAABBAAA', 1), _write_dir(tmp_path / 'b', 'AAABBAAA', 2)
    chunks = list(E.stored_size_chunks([a, b], 2))
    assert [c[0].size(0) for c in chunks] == [2, 1, 2, 2, 1]
    assert all(len(c) == 2 and c[0].shape == c[1].shape for c in chunks)
    assert all(torch.equal(img, E.read_image(p)) for k, col in enumerate((a, b)) for img, p in zip([i for c in chunks for i in c[k]], col))
    odd = _write_dir(tmp_path / 'c', 'AAABAAAA', 3)             # index 4 differs from its partner in size
    with pytest.raises(SystemExit) as exc:
        list(E.stored_size_chunks([a, odd], 2))
    assert str(exc.value) == '%s and %s differ in size' % (a[4], odd[4])


# ---- state_dict_of ------------------------------------------------------------------------------------------------------------------------
def test_state_dict_of(tmp_path):
    sd = {'conv.weight': torch.ones(2), 'fc.bias': torch.zeros(3)}
    got = E.state_dict_of(sd)
    assert type(got) is dict and got is not sd and list(got) == list(sd) and all(got[k] is sd[k] for k in sd)
    wrapped = {'module.' + k: v for k, v in sd.items()}
    got = E.state_dict_of(wrapped)
    assert list(got) == list(sd) and all(got[k] is sd[k] for k in sd) and list(wrapped) == ['module.conv.weight', 'module.fc.bias']
    mixed = dict(wrapped, **{'fc.bias': sd['fc.bias']})         # not every key carries the prefix: nothing is stripped
    assert list(E.state_dict_of(mixed)) == list(mixed)
    assert E.state_dict_of({}) == {}
    path = str(tmp_path / 'w.pth')
    torch.save(wrapped, path)
    got = E.state_dict_of(path)
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


# ---- inception_network --------------------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(4, 2)


def test_inception_network_default_weights_are_read_at_call_time(monkeypatch, capsys):
    seen = []

    def load(path, device='cuda'):
        seen.append((path, str(device)))
        return _Net().train()

    monkeypatch.setattr(I, 'load_inception', load)
    monkeypatch.setattr(I, 'DEFAULT_WEIGHTS', 'default.pth')    # assigned after import, as INTEGRATION.md tells users to
    net = I.inception_network(None, 'cpu', 'X', True)
    assert seen == [('default.pth', 'cpu')] and isinstance(net, _Net) and not net.training
    I.inception_network('given.pth', 'cpu', 'X', False)         # given weights win over the default: a path ...
    assert seen[1:] == [('given.pth', 'cpu')]
    mine = _Net().train()
    assert I.inception_network(mine, 'cpu', 'X', False) is mine and not mine.training and len(seen) == 2      # ... and an instance
    assert capsys.readouterr().err == ''


@pytest.mark.parametrize('fid_form', [False, True])
def test_inception_network_without_weights_warns_and_builds_the_asked_form(fid_form, monkeypatch, capsys):
    monkeypatch.setattr(I, 'DEFAULT_WEIGHTS', None)
    state = torch.random.get_rng_state()
    with torch.device('meta'):
        net = I.inception_network(None, 'meta', 'SomeMetric', fid_form, 'figures are MEANINGLESS as anything')
    err = capsys.readouterr().err
    assert err.startswith('WARNING: SomeMetric is built WITHOUT pretrained weights (weights=None): a seeded random initialisation. ')
    assert 'Its figures are MEANINGLESS as anything; pass the path of ' in err
    assert ('pt_inception-2015-12-05-*.pth' in err) == fid_form and ('inception_v3_google-*.pth' in err) == (not fid_form)
    assert isinstance(net, I.InceptionV3) and not net.training and net.fid_variant == fid_form
    assert net.fc.out_features == (I.FID_CLASSES if fid_form else 1000) and hasattr(net, 'AuxLogits') == (not fid_form)
    assert torch.equal(torch.random.get_rng_state(), state)     # the fixed seed is set inside a fork of the generator


# ---- import order -------------------------------------------------------------------------------------------------------------------------
_IMPORT_ORDER = r'''
import importlib, sys
metrics = ('accuracy', 'inception', 'fid', 'featsets', 'lpips', 'imageprep')
for module in ('evalkit', 'imageprep', 'lpips'):        # one fresh interpreter serves all three: each one's imports hold the last one's
    importlib.import_module('scene_generation_amd.' + module)
    print(module, *[m for m in metrics if 'scene_generation_amd.' + m in sys.modules])
'''


def test_import_order():
    """evalkit is a leaf; imageprep needs evalkit alone; lpips needs those two and neither the classifier nor the Inception network"""
    out = subprocess.run([sys.executable, '-c', _IMPORT_ORDER], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split('\n')[:3] == ['evalkit', 'imageprep imageprep', 'lpips lpips imageprep']
