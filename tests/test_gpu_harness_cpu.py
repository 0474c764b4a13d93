"""The comparison primitives of tests/gpu_harness.py without a device: every GPU family module is judged by them, so what they let
pass and what they record is pinned here on plain numpy / torch-CPU data."""
import json
import os

import numpy as np
import pytest
import torch

import gpu_harness as H
from gpu_harness import Margins

ONE = np.float64(1.0)
UP = np.nextafter(ONE, 2.0)              # one ulp above 1


# ---- within ----------------------------------------------------------------------------------------------------------------------------
def test_within_passes_at_the_bound_and_fails_one_ulp_above():
    m = Margins()
    ref, bound = np.zeros(4), np.full(4, 0.25)
    m.within('f', np.array([0.0, 0.25, -0.25, 0.125]), ref, bound, 'at the bound')
    assert m.worst['f'] == (1.0, 'at the bound')
    with pytest.raises(AssertionError, match='exceeds the rounding bound'):
        m.within('f', np.array([0.0, 0.25 * UP, 0.0, 0.0]), ref, bound, 'one ulp above')
    assert m.worst['f'] == (float(UP), 'one ulp above')              # recorded before the assertion fired


def test_within_bound_zero_means_equality():
    m = Margins()
    x = np.array([1.5, -2.0, 0.0])
    m.within('eq', x, x.copy(), 0.0, 'equal')
    assert m.worst['eq'] == (0.0, 'equal')
    with pytest.raises(AssertionError):
        m.within('eq', x, np.nextafter(x, np.inf), 0.0, 'a last bit')
    assert m.worst['eq'] == (float('inf'), 'a last bit')
    m.within('mixed', np.array([1.0, 2.0]), np.array([1.0, 2.5]), np.array([0.0, 1.0]), 'per element')
    assert m.worst['mixed'] == (0.5, 'per element')


@pytest.mark.parametrize('bad', (np.nan, np.inf, -np.inf))
def test_within_fails_on_non_finite_results_and_notes_inf_first(bad):
    m = Margins()
    m.within('f', np.zeros(3), np.zeros(3), 1.0, 'fine')
    with pytest.raises(AssertionError, match='non-finite'):
        m.within('f', np.array([0.0, bad, 0.0]), np.zeros(3), 1.0, 'bad')
    assert m.worst['f'] == (float('inf'), 'bad')
    m.within('f', np.zeros(3), np.zeros(3), 1.0, 'fine again')       # and nothing finite replaces it
    assert m.worst['f'] == (float('inf'), 'bad')


def test_within_fails_on_a_nan_reference_or_bound():
    for ref, bound in ((np.array([np.nan]), 1.0), (np.zeros(1), np.array([np.nan]))):
        m = Margins()
        with pytest.raises(AssertionError):
            m.within('f', np.ones(1), ref, bound, 'nan')
        assert m.worst['f'] == (float('inf'), 'nan')


def test_within_shape_mismatch_and_empty():
    m = Margins()
    with pytest.raises(AssertionError):
        m.within('f', np.zeros((2, 3)), np.zeros((3, 2)), 1.0, 'shapes')
    with pytest.raises(AssertionError):
        m.within('f', np.zeros(6), np.zeros((2, 3)), 1.0, 'flat')
    assert m.within('f', np.zeros((0, 4)), np.zeros((0, 4)), 1.0, 'empty') is None
    assert m.worst == {}


def test_within_numpy_and_torch_inputs_note_the_same_ratio():
    rng = np.random.RandomState(5)
    got, ref = rng.randn(7, 5).astype(np.float32), rng.randn(7, 5)
    bound = np.abs(rng.randn(5)) * 8 + 8                           # broadcast over the rows
    a, b = Margins(), Margins()
    a.within('f', got, ref, bound, 'numpy')
    b.within('f', torch.from_numpy(got).requires_grad_(), torch.from_numpy(ref), torch.from_numpy(bound), 'torch')
    assert a.worst['f'][0] == b.worst['f'][0] and 0 < a.worst['f'][0] < 1
    assert a.worst['f'][0] == float((np.abs(got.astype(np.float64) - ref) / bound).max())


# ---- Margins ---------------------------------------------------------------------------------------------------------------------------
def test_margins_keep_the_worst_ratio_and_its_case_per_family():
    m = Margins()
    for fam, r, name in (('a', 0.25, 'a1'), ('a', 0.5, 'a2'), ('a', 0.125, 'a3'), ('a', 0.5, 'a4'), ('b', 0.0, 'b1'), ('c', np.nan, 'c1'),
                         ('c', 3.0, 'c2')):
        m.note(fam, r, name)
    assert m.worst == {'a': (0.5, 'a2'), 'b': (0.0, 'b1'), 'c': (float('inf'), 'c1')}
    m.note('a', np.float32(0.75), 'a5')
    assert m.worst['a'] == (0.75, 'a5') and type(m.worst['a'][0]) is float


def test_two_instances_do_not_see_each_other():
    """the conv modules' checks once landed in the dense module's table: within() notes into the instance it is called on, only"""
    dense, conv = Margins(), Margins()
    conv.within('conv family', np.ones(2), np.ones(2), 1.0, 'case')
    assert dense.worst == {} and list(conv.worst) == ['conv family']
    dense.close_noted('dense family', np.ones(2), np.ones(2), 1e-6, 'case')
    assert list(dense.worst) == ['dense family'] and list(conv.worst) == ['conv family']


def _dumped(monkeypatch, write):
    out = {}
    monkeypatch.setattr(H, '_dump', lambda name, obj: out.update({name: json.loads(json.dumps(obj, indent=1, sort_keys=True))}))
    write()
    return out


def test_the_three_layouts_round_trip_through_json(monkeypatch):
    m = Margins()
    m.note('fam', 0.5, 'case 1')
    m.note('other', float('inf'), 'case 2')
    got = _dumped(monkeypatch, lambda: m.dump('a.json'))
    assert got == {'a.json': {'fam': {'ratio_of_bound': 0.5, 'case': 'case 1'}, 'other': {'ratio_of_bound': float('inf'), 'case': 'case 2'}}}
    got = _dumped(monkeypatch, lambda: m.dump('b.json', 'share_of_bound', empty=False))
    assert got == {'b.json': {'fam': {'share_of_bound': 0.5, 'case': 'case 1'}, 'other': {'share_of_bound': float('inf'), 'case': 'case 2'}}}
    m.extra['e2e'] = {'ratio_of_yardstick': 2.0, 'bound': 64.0}
    got = _dumped(monkeypatch, lambda: m.dump_yardstick('c.json', {'fam': 8.0}, 16.0))
    assert got == {'c.json': {'fam': {'ratio_of_fp32_yardstick': 0.5, 'bound': 8.0, 'case': 'case 1'},
                              'other': {'ratio_of_fp32_yardstick': float('inf'), 'bound': 16.0, 'case': 'case 2'},
                              'e2e': {'ratio_of_yardstick': 2.0, 'bound': 64.0}}}
    assert _dumped(monkeypatch, lambda: Margins().dump('d.json')) == {'d.json': {}}          # a family module always leaves its file
    assert _dumped(monkeypatch, lambda: Margins().dump('d.json', empty=False)) == {}       # a metric module only what it recorded


def test_dump_writes_the_file_json_reads_back(tmp_path, monkeypatch):
    monkeypatch.setattr(H, 'ROOT', str(tmp_path))
    (tmp_path / '.gitignore').write_text('*.pyc\nrecords_out/\nbuild/\nrecords_out/\n')
    m = Margins()
    m.note('fam', 0.1, 'case')
    m.dump('x_margins.json')
    with open(tmp_path / 'records_out' / 'x_margins.json') as f:
        text = f.read()
    assert json.loads(text) == {'fam': {'ratio_of_bound': 0.1, 'case': 'case'}}
    assert text == json.dumps({'fam': {'case': 'case', 'ratio_of_bound': 0.1}}, indent=1, sort_keys=True)
    (tmp_path / 'records_out' / 'x_margins.json').unlink()
    (tmp_path / 'records_out').rmdir()
    (tmp_path / 'records_out').write_text('a file in the way')      # the directory cannot be made: swallowed, as ever
    m.dump('x_margins.json')
    for text in ('*.pyc\n', 'records_out/\nother_out/\n'):          # no output directory named, or two: loud, not lost
        (tmp_path / '.gitignore').write_text(text)
        with pytest.raises(AssertionError, match='exactly one output directory'):
            m.dump('x_margins.json')


def test_the_repository_names_one_output_directory():
    assert os.path.dirname(H._out_dir()) == H.ROOT == os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- close -----------------------------------------------------------------------------------------------------------------------------
def test_close_max_norm_failure():
    b = torch.ones(1, 2, 4, 4)
    a = b.clone()
    a[0, 0, 0, 0] += 1e-3
    n0 = len(H._CLOSE_LOG)
    with pytest.raises(AssertionError, match='max err'):
        H.close(a, b, 1e-5, 'max norm')
    assert len(H._CLOSE_LOG) == n0                                   # it fails before the relative-L2 lines
    with pytest.raises(AssertionError, match='non-finite'):
        H.close(a * float('nan'), b, 1e-5, 'nan')
    with pytest.raises(AssertionError):
        H.close(a[:, :1], b, 1e-5, 'shape')


def test_close_a_small_channel_that_is_all_wrong_passes_the_max_norm_and_fails_per_channel():
    tol = 1e-5
    b = torch.ones(1, 2, 8, 8, dtype=torch.float64)
    b[:, 1] = 1e-6                                                  # a channel far below the largest entry
    a = b.clone()
    a[:, 1] = 4e-6                                                  # 300 % wrong, yet 3e-6 <= tol * max(1, max|b|)
    assert float((a - b).abs().max()) <= tol * 1.0
    n0 = len(H._CLOSE_LOG)
    with pytest.raises(AssertionError, match='channel 1 relative-L2'):
        H.close(a, b, tol, 'small channel')
    kinds = [(k, r > 1.0) for r, k, name, t in H._CLOSE_LOG[n0:]]
    assert kinds == [('tensor', False), ('channel', True)]           # the tensor as a whole passes; the log grew by both lines


def test_close_log_is_one_list_and_grows():
    n0 = len(H._CLOSE_LOG)
    x = torch.arange(12.0).view(3, 4)
    H.close(x, x.numpy(), 1e-6, 'matrix')                            # tensor + columns
    H.close(x.view(-1), x.view(-1), 1e-6, 'vector')                  # tensor
    H.close(x[:0], x[:0], 1e-6, 'empty')                             # nothing
    assert [(k, n) for r, k, n, t in H._CLOSE_LOG[n0:]] == [('tensor', 'matrix'), ('column', 'matrix'), ('tensor', 'vector')]
    m = Margins()
    m.close_noted('f', x.double(), x.double() + 2.0 ** -20, 2.0 ** -10, 'noted')          # max-norm ratio 2^-10 / max|b|, over close()'s own
    assert len(H._CLOSE_LOG) == n0 + 5
    assert m.worst['f'] == (max([2.0 ** -10 / (11 + 2.0 ** -20)] + [r[0] for r in H._CLOSE_LOG[n0 + 3:]]), 'noted')


# ---- the fp32 yardstick ----------------------------------------------------------------------------------------------------------------
def test_yardstick_floor_applies_when_the_float32_run_is_exact():
    floor = 2.0 ** -24
    ref64 = torch.tensor([1.0, -4.0, 2.0], dtype=torch.float64)
    m = Margins()
    got = ref64.clone()
    got[1] += 4 * 16 * floor                                          # relative error 16 floors: at the factor
    m.yardstick('fam', 'at the factor', got, ref64, ref64.clone(), {}, 16.0, floor)
    assert m.worst['fam'] == (16.0, 'at the factor')
    got[1] = -4.0 + 4 * 16 * floor * (1 + 2.0 ** -20)
    with pytest.raises(AssertionError, match='fp32 yardstick'):
        m.yardstick('fam', 'above', got, ref64, ref64.clone(), {}, 16.0, floor)
    assert m.worst['fam'][1] == 'above' and m.worst['fam'][0] > 16.0


def test_yardstick_factor_comes_from_the_table():
    floor = 2.0 ** -24
    ref64 = torch.tensor([2.0, 0.5], dtype=torch.float64)
    ref32 = ref64 + torch.tensor([2.0 ** -10, 0.0], dtype=torch.float64)         # yardstick 2^-11 of the scale
    got = ref64 + torch.tensor([0.0, 10 * 2.0 ** -10], dtype=torch.float64)       # 10 yardsticks
    m = Margins()
    m.yardstick('loose', 'ten', got.float().numpy(), ref64, ref32, {'tight': 8.0}, 16.0, floor)
    assert m.worst['loose'] == (10.0, 'ten')
    with pytest.raises(AssertionError, match=r'bound 8 x'):
        m.yardstick('tight', 'ten', got, ref64, ref32, {'tight': 8.0}, 16.0, floor)
    with pytest.raises(AssertionError, match='non-finite'):
        m.yardstick('nan', 'nan', got * float('nan'), ref64, ref32, {}, 16.0, floor)
    assert m.worst['nan'] == (float('inf'), 'nan')
    with pytest.raises(AssertionError):
        m.yardstick('shape', 'shape', got[:1], ref64, ref32, {}, 16.0, floor)


# ---- bits, tags, options ---------------------------------------------------------------------------------------------------------------
def test_same_bits_tells_the_zeros_apart_and_same_does_not():
    pz, nz = np.array([0.0, 1.0], dtype=np.float32), np.array([-0.0, 1.0], dtype=np.float32)
    assert H.same(pz, nz, 'values')
    H.same_bits(pz, pz.copy(), 'bits')
    with pytest.raises(AssertionError, match='1 of 2 elements differ'):
        H.same_bits(pz, nz, 'bits')
    assert H.bits(np.array([1.0])).dtype == np.int32 and H.bits(np.array([1.0]))[0] == 0x3f800000
    nan = np.array([np.nan], dtype=np.float32)
    H.same_bits(nan, nan.copy(), 'the same NaN')
    with pytest.raises(AssertionError):
        H.same(nan, nan.copy(), 'NaN is no value')


def test_same_rounds_a_float_expectation_and_compares_integers_by_value():
    third = np.array([1.0 / 3.0])
    assert H.same(third.astype(np.float32), third, 'fp32 expectation') and H.same(torch.from_numpy(third.astype(np.float32)), third)
    assert H.same(torch.tensor([1, 2], dtype=torch.int32), np.array([1, 2], dtype=np.int64))
    with pytest.raises(AssertionError):
        H.same(torch.tensor([1, 2], dtype=torch.int32), np.array([1, 3]))
    with pytest.raises(AssertionError):
        H.same(np.zeros(3, dtype=np.float32), np.zeros((3, 1)), 'shape')


def test_opt_tag_is_sorted_and_names_the_empty_set_on_request():
    assert H.opt_tag({'tile': 2, 'fixedtap': 0, 'par_split': 1}) == 'fixedtap=0 par_split=1 tile=2'
    assert H.opt_tag({}) == '' and H.opt_tag({}, 'defaults') == 'defaults' and H.opt_tag({'a': 1}, 'defaults') == 'a=1'


def test_options_restore_on_exit_and_on_exception(monkeypatch):
    from scene_generation_amd import _hip
    state, calls = {'a': 1, 'b': 2, 'c': 3}, []
    monkeypatch.setattr(_hip, 'get_option', lambda k: state[k])
    monkeypatch.setattr(_hip, 'set_option', lambda k, v: (calls.append((k, v)), state.__setitem__(k, v)))
    with H.options({'a': 10, 'b': None, 'c': 30}):
        assert state == {'a': 10, 'b': 2, 'c': 30}                  # None leaves an option alone
        with H.options({'a': 11}):
            assert state['a'] == 11
        assert state['a'] == 10
    assert state == {'a': 1, 'b': 2, 'c': 3}
    assert calls == [('a', 10), ('c', 30), ('a', 11), ('a', 10), ('c', 3), ('a', 1)]         # restored in reverse order
    with pytest.raises(RuntimeError):
        with H.options({'a': 5, 'c': 6}):
            raise RuntimeError('inside')
    assert state == {'a': 1, 'b': 2, 'c': 3}
    with pytest.raises(KeyError):
        with H.options({'a': 7, 'nope': 1}):                         # the second option does not exist: the first is put back
            pass
    assert state == {'a': 1, 'b': 2, 'c': 3}


def test_twice_compares_the_arrays_of_two_calls():
    seq = iter([(np.ones(2), 'x'), (np.ones(2), 'y'), (np.ones(2), 1), (np.zeros(2), 1)])
    assert H.twice(lambda: next(seq), 'same')[1] == 'x'
    with pytest.raises(AssertionError, match='a second run differs'):
        H.twice(lambda: next(seq), 'differs')


def test_the_harness_imports_no_oracle_no_trainer_no_parser():
    """read from its source, since this process has long imported everything"""
    import ast
    with open(H.__file__) as f:
        tree = ast.parse(f.read())
    names = lambda n: [a.name for a in n.names] if isinstance(n, ast.Import) else [n.module] + ['%s.%s' % (n.module, a.name) for a in n.names]
    every = {m for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom)) for m in names(n)}
    assert not [m for m in every if m.split('.')[0] == 'oracle' or m.startswith('test_') or m.endswith(('.trainer', '.args'))], every
