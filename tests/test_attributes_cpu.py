"""Host-side surface of the attribute sampler (scene_generation_amd/attributes.py, the Sampler's new arguments, the C ABI's
argument checks) and the numpy restatement the GPU tests compare against (tests/attributes_ref.py): that the shared case set reaches
every branch, that the directional masks at g = 4 are the hand-written tables, that a draw lands in its allowed set, that an image's
result does not depend on its place in the batch, and the file formats.  No GPU."""
import pickle

import numpy as np
import pytest
import torch

import attributes_cases as cases
import attributes_ref as ref
from scene_generation_amd import _hip, attributes, sample
from scene_generation_amd.synthetic import make_sampling_vocab


def _run(case, rule='reference', given=True, **over):
    c = dict(case, **over)
    return ref.sample(c['objs'], c['obj_to_img'], c['triples'], c['triple_to_img'], c['counts'], c['u'],
                      c['given'] if given else None, c['N'], c['S'], c['g'], 0, rule)


def test_case_set_reaches_every_branch():
    """a condition of the GPU comparison: it only shows what the cases exercise"""
    total = dict.fromkeys(ref.COUNTERS, 0)
    for case in cases.all_cases():
        assert case['objs'].size <= 150 and case['N'] == 10
        for rule in ('reference', 'geometric'):
            for given in (True, False):
                k = _run(case, rule, given)[3]
                for name, v in k.items():
                    total[name] += v
    assert sorted(total) == sorted(ref.COUNTERS)
    missing = [name for name, v in total.items() if v == 0]
    assert not missing, (missing, total)
    # ... and per shape the ones a shape can reach at all (g = 1 has one cell: every mask is the whole grid)
    for case in cases.all_cases():
        k = _run(case)[3]
        for name in ('copy_inside', 'copy_surrounding', 'given_size_kept', 'given_loc_kept', 'step5_fill', 'images_0', 'images_1',
                     'images_2plus', 'skip_pred', 'skip_self', 'skip_image_obj', 'skip_outside', 'never_seen_class', 'mask_left',
                     'mask_right', 'mask_above', 'mask_below', 'size_adjusted_reference', 'size_kept_reference'):
            assert k[name] > 0, (case['S'], case['g'], name)


L0, L2, L3 = [0, 4, 8, 12], [0, 1, 4, 5, 8, 9, 12, 13], [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]
R0, R1, R2 = [1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 14, 15], [2, 3, 6, 7, 10, 11, 14, 15], [3, 7, 11, 15]
A0, A2, A3 = [0, 1, 2, 3], [0, 1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
B0, B1, B2 = [4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [8, 9, 10, 11, 12, 13, 14, 15], [12, 13, 14, 15]
# allowed cells of the subject per (predicate, partner's cell 0..15) on the 4 x 4 grid, cell = col + 4 * row
TABLE_G4 = {
    1: [L0, L0, L2, L3, L0, L0, L2, L3, L0, L0, L2, L3, L0, L0, L2, L3],
    2: [R0, R1, R2, R2, R0, R1, R2, R2, R0, R1, R2, R2, R0, R1, R2, R2],
    3: [A0, A0, A0, A0, A0, A0, A0, A0, A2, A2, A2, A2, A3, A3, A3, A3],
    4: [B0, B0, B0, B0, B1, B1, B1, B1, B2, B2, B2, B2, B2, B2, B2, B2],
}


@pytest.mark.parametrize('q', [1, 2, 3, 4])
def test_allowed_masks_at_g4(q):
    for cell in range(16):
        assert np.nonzero(ref.allowed(q, cell, 4))[0].tolist() == TABLE_G4[q][cell], (q, cell)


def test_draw_rule():
    """the smallest c whose inclusive prefix sum exceeds u * sum; zero mass falls back to the allowed cells"""
    allow = np.array([1, 1, 0, 1], dtype=bool)
    hist = np.array([2, 0, 100, 6], dtype=np.int64)                 # weights 2 0 0 6, prefix 2 2 2 8
    assert ref.draw(hist, allow, 0.0) == 0
    assert ref.draw(hist, allow, np.float32(0.2499)) == 0
    assert ref.draw(hist, allow, 0.25) == 3                         # 2 > 2 is false
    assert ref.draw(hist, allow, cases.U_MAX) == 3
    k = dict.fromkeys(ref.COUNTERS, 0)
    zero = np.array([0, 0, 7, 0], dtype=np.int64)                   # seen, but never in an allowed cell: weights 1 1 0 1
    assert [ref.draw(zero, allow, u, k) for u in (0.0, 0.34, 0.67, cases.U_MAX)] == [0, 1, 3, 3]
    assert k['zero_mass_fallback'] == 4 and k['never_seen_class'] == 0
    assert ref.draw(None, allow, 0.5, k) == 1 and k['never_seen_class'] == 1
    big = np.array([1 << 62, 1 << 62, 0, 1], dtype=np.int64)        # 2^63 + 1 does not fit an int64: exact in Python ints
    assert ref.draw(big, allow, 0.4) == 0 and ref.draw(big, allow, 0.6) == 1


@pytest.mark.parametrize('S,g', cases.SHAPES)
def test_draws_land_in_their_allowed_set(S, g):
    case = cases.make_case(S, g)
    size, loc, attrs, _, draws = _run(case)
    assert draws
    for o, allow, cell in draws:
        assert allow[cell] and loc[o] >= 0
    real = case['objs'] != 0
    assert (size[real] >= 0).all() and (size[real] < S).all() and (loc >= 0).all() and (loc < g * g).all()
    assert (attrs[:, :S].sum(1) == 1).all() and (attrs[:, S:].sum(1) == 1).all()
    gs = np.array([ref.first_bit(r[:S]) for r in case['given']])
    gl = np.array([ref.first_bit(r[S:]) for r in case['given']])
    assert (size[gs >= 0] == gs[gs >= 0]).all() and (loc[gl >= 0] == gl[gl >= 0]).all()        # given bits win


@pytest.mark.parametrize('rule', ['reference', 'geometric'])
def test_permuting_the_images_permutes_the_rows(rule):
    case = cases.make_case(10, 5)
    size, loc, attrs = _run(case, rule)[:3]
    perm = [7, 2, 9, 0, 4, 1, 8, 3, 6, 5]
    pcase, order = cases.permute_case(case, perm)
    psize, ploc, pattrs = _run(pcase, rule)[:3]
    assert (psize == size[order]).all() and (ploc == loc[order]).all() and (pattrs == attrs[order]).all()


def test_size_rules_differ_only_in_copied_sizes():
    case = cases.make_case(10, 5)
    a, b = _run(case, 'reference'), _run(case, 'geometric')
    assert (a[1] == b[1]).all() and (a[0] != b[0]).any()


def test_object_limit_in_the_restatement():
    """objects past the limit stay at -1 and their triples are skipped"""
    case = cases.make_case(10, 5)
    size, loc, attrs = ref.sample(case['objs'], case['obj_to_img'], case['triples'], case['triple_to_img'], case['counts'], case['u'],
                                  case['given'], case['N'], 10, 5, max_objs=40)[:3]
    late = np.concatenate([np.nonzero(case['obj_to_img'] == n)[0][40:] for n in range(case['N'])])
    assert late.size == 31 and (size[late] == -1).all() and (loc[late] == -1).all() and not attrs[late].any()


def test_histogram_restatement():
    S, g = 3, 2
    objs = np.array([1, 1, 0, 2, 9, -1, 1])
    attrs = np.zeros((7, 7), dtype=np.float32)
    attrs[0, [1, 2, 3]] = 1          # first size bit 1, location 0
    attrs[1, 6] = 1                  # no size bit, location 3
    attrs[2, [0, 4]] = 1             # the __image__ class: skipped
    attrs[3, 2] = 0.75
    attrs[3, 5] = 0.5                # not above the threshold
    attrs[4, 0] = attrs[5, 0] = 1    # classes outside the table
    counts = ref.histogram(objs, attrs, 3, S, g)
    want = np.zeros((3, 7), dtype=np.int64)
    want[1, [1, 3, 6]] = 1
    want[2, 2] = 1
    assert (counts == want).all()
    assert (ref.histogram(objs, attrs, 3, S, g, counts=counts) == 2 * want).all()


# ---- files ---------------------------------------------------------------------------------------------------------------------------
def test_npz_and_pickle_round_trips(tmp_path):
    vocab = make_sampling_vocab(6)
    rs = np.random.RandomState(3)
    counts = rs.randint(0, 1000, size=(6, 35)).astype(np.int64)
    counts[0] = 0
    stats = attributes.AttributeStats(6, device='cpu', counts=counts)
    back = attributes.AttributeStats.load(stats.save(str(tmp_path / 'a.npz')), device='cpu')
    assert (back.size_len, back.grid, back.num_classes) == (10, 5, 6) and torch.equal(back.counts, stats.counts)
    path = stats.save(str(tmp_path / 'attributes_10_25.pickle'), vocab)
    with open(path, 'rb') as f:
        d = pickle.load(f)
    assert sorted(d) == ['location', 'size'] and sorted(d['size']) == ['obj%d' % k for k in range(1, 6)]        # no __image__
    assert d['size']['obj3'] == counts[3, :10].tolist() and d['location']['obj5'] == counts[5, 10:].tolist()
    assert all(type(v) is int for v in d['size']['obj1'])
    back = attributes.AttributeStats.load(path, vocab, device='cpu')
    assert torch.equal(back.counts, stats.counts) and back.counts.dtype == torch.int64
    with pytest.raises(ValueError, match='vocab'):
        stats.save(str(tmp_path / 'b.pickle'))
    with pytest.raises(ValueError, match='vocab'):
        attributes.AttributeStats.load(path, device='cpu')


def test_reference_shaped_dict_with_unknown_and_missing_names(tmp_path):
    vocab = make_sampling_vocab(5)
    d = {'location': {'obj1': list(range(16)), 'zebra': [9] * 16, 'obj4': [1] * 16},
         'size': {'obj1': [5, 0, 7], 'zebra': [1, 1, 1], 'obj4': [0, 0, 2]}}
    path = str(tmp_path / 'ref.pickle')
    with open(path, 'wb') as f:
        pickle.dump(d, f)
    stats = attributes.AttributeStats.load(path, vocab, device='cpu')
    assert (stats.size_len, stats.grid, stats.num_classes) == (3, 4, 5)
    want = np.zeros((5, 19), dtype=np.int64)
    want[1] = [5, 0, 7] + list(range(16))
    want[4] = [0, 0, 2] + [1] * 16
    assert (stats.counts.numpy() == want).all()                    # zebra ignored, obj2 / obj3 zero
    with open(path, 'wb') as f:
        pickle.dump({'location': {'obj1': [1] * 15}, 'size': {'obj1': [1]}}, f)
    with pytest.raises(ValueError, match='square'):
        attributes.AttributeStats.load(path, vocab, device='cpu')


def test_draw_uniforms():
    u = attributes.draw_uniforms(5, 40)
    assert u.dtype == np.float32 and u.shape == (40, 2) and (u >= 0).all() and (u < 1).all()
    assert (u == np.minimum(np.random.RandomState(5).random_sample((40, 2)).astype(np.float32), cases.U_MAX)).all()
    assert (attributes.draw_uniforms(5, 40)[:7] == attributes.draw_uniforms(5, 7)).all()      # row o belongs to object o


# ---- argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    with pytest.raises(ValueError, match='1..64'):
        attributes.AttributeStats(4, size_len=65, device='cpu')
    with pytest.raises(ValueError, match='1..64'):
        attributes.AttributeStats(4, grid=9, device='cpu')
    with pytest.raises(ValueError, match='counts must be'):
        attributes.AttributeStats(4, device='cpu', counts=np.zeros((4, 34), dtype=np.int64))
    stats = attributes.AttributeStats(4, device='cpu')
    objs, o2i = torch.tensor([1, 2, 0]), torch.tensor([0, 0, 0])
    triples = torch.tensor([[0, 1, 1]])
    with pytest.raises(ValueError, match=r'given must be \[3, 35\]'):
        attributes.sample_attributes(objs, triples, o2i, stats, given=torch.zeros(3, 26), num_images=1)
    with pytest.raises(ValueError, match=r'attributes must be \[O, 35\]'):
        stats.update(objs, torch.zeros(3, 36))
    with pytest.raises(ValueError, match='size_rule'):
        attributes.sample_attributes(objs, triples, o2i, stats, num_images=1, size_rule='bigger')
    with pytest.raises(ValueError, match=r'u must be \[3, 2\]'):
        attributes.sample_attributes(objs, triples, o2i, stats, num_images=1, u=np.zeros((3, 1), dtype=np.float32))
    many = attributes.MAX_OBJS + 1
    with pytest.raises(ValueError, match='more than %d objects' % attributes.MAX_OBJS):
        attributes.sample_attributes(torch.ones(many + 2, dtype=torch.int64), triples, torch.zeros(many + 2, dtype=torch.int64), stats,
                                     obj_to_img_host=[0] + [1] * many + [2])
    attributes.check_image_sizes([0] * attributes.MAX_OBJS + [1] * attributes.MAX_OBJS)
    with pytest.raises(RuntimeError, match='no CPU fallback'):      # everything checked: the launch itself needs the device
        attributes.sample_attributes(objs, triples, o2i, stats, num_images=1)


def test_sample_attributes_flag_needs_a_file(tmp_path):
    args = sample.make_parser().parse_args(['--checkpoint', 'none.pt', '--sample_attributes', '1'])
    assert args.attribute_size_rule == 'reference' and args.attributes_file is None
    with pytest.raises(ValueError, match='--sample_attributes 1 needs --attributes_file'):
        sample.run_model(args, {}, str(tmp_path))
    with pytest.raises(ValueError, match='attribute_stats'):
        sample.Sampler(None, sample_attributes=True)
    with pytest.raises(ValueError, match='attribute_size_rule'):
        sample.Sampler(None, sample_attributes=True, attribute_stats=attributes.AttributeStats(4, device='cpu'),
                       attribute_size_rule='bigger')
    with pytest.raises(SystemExit):
        sample.make_parser().parse_args(['--checkpoint', 'none.pt', '--attribute_size_rule', 'bigger'])


def test_c_abi_prototypes_and_argument_checks():
    protos = _hip.parse_header()
    assert protos['sg_attribute_histogram'][2] == ['objs', 'attrs', 'counts', 'O', 'C', 'S', 'g', 'image_class', 'stream']
    assert protos['sg_sample_attributes'][2] == ['objs', 'obj_to_img', 'triples', 'triple_to_img', 'counts', 'u', 'given', 'size_idx',
                                                 'loc_idx', 'attrs', 'N', 'O', 'T', 'C', 'S', 'g', 'image_class', 'size_rule', 'stream']
    lib = _hip.lib()
    kinds = [lib.sg_prof_kind_name(i).decode() for i in range(lib.sg_prof_num_kinds())]
    assert kinds[-2:] == ['attributes_hist', 'attributes_sample'] and kinds.index('grad_norm') == len(kinds) - 3
    buf = (_hip.ctypes.c_char * 4096)()
    p = _hip.ctypes.cast(buf, _hip.ctypes.c_void_p)
    call = lambda **kw: lib.sg_sample_attributes(p, p, p, p, p, p, None, p, p, p, kw.get('N', 1), kw.get('O', 4), 1, kw.get('C', 3),
                                                 kw.get('S', 10), kw.get('g', 5), 0, kw.get('rule', 0), None)
    for bad, word in ((dict(S=65), b'one cell per lane'), (dict(g=9), b'one cell per lane'), (dict(S=0), b'one cell per lane'),
                      (dict(rule=2), b'size_rule'), (dict(C=0), b'bad sizes'), (dict(O=1 << 26, S=64, g=8), b'2^31')):
        assert call(**bad) < 0 and word in lib.sg_last_error_string(), bad
    assert lib.sg_sample_attributes(None, p, p, p, p, p, None, p, p, p, 1, 4, 1, 3, 10, 5, 0, 0, None) < 0
    assert b'null operand' in lib.sg_last_error_string()
    assert lib.sg_sample_attributes(None, None, None, None, None, None, None, None, None, None, 0, 0, 0, 3, 10, 5, 0, 0, None) == 0      # O = 0
    assert lib.sg_attribute_histogram(None, None, None, 0, 3, 10, 5, 0, None) == 0
    assert lib.sg_attribute_histogram(p, p, None, 4, 3, 10, 5, 0, None) < 0 and b'null operand' in lib.sg_last_error_string()
    assert lib.sg_attribute_histogram(p, p, p, 4, 0, 10, 5, 0, None) < 0 and b'bad sizes' in lib.sg_last_error_string()
