"""The attribute sampler on the GPU (csrc/attributes.hip through scene_generation_amd.attributes): sg_attribute_histogram against
numpy, sg_sample_attributes against the restatement of tests/attributes_ref.py -- integer equality on every case of
tests/attributes_cases.py (which test_attributes_cpu.py shows to reach every branch), both size rules, with and without given
bits -- run-to-run and batch-order invariance, the Sampler's opt-in sampling and the command line.  The tree only."""
import os

import numpy as np
import pytest
import torch

import attributes_cases as cases
import attributes_ref as ref
import sampling_helpers as SH
from scene_generation_amd import attributes, ops, sample, scenegraph
from scene_generation_amd.model import Model
from scene_generation_amd.synthetic import fill_deterministic, make_batch, make_sampling_vocab

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KINDS = ('attributes_hist', 'attributes_sample')
_REF = {}


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _expected(S, g, rule, given):
    """the restatement's answer, computed once per case"""
    key = (S, g, rule, given)
    if key not in _REF:
        c = cases.make_case(S, g)
        _REF[key] = ref.sample(c['objs'], c['obj_to_img'], c['triples'], c['triple_to_img'], c['counts'], c['u'],
                               c['given'] if given else None, c['N'], S, g, 0, rule)[:3]
    return _REF[key]


def _device(case, given=True):
    stats = attributes.AttributeStats(case['C'], case['S'], case['g'], DEV, counts=case['counts'])
    return dict(objs=T(case['objs']), triples=T(case['triples']), obj_to_img=T(case['obj_to_img']), stats=stats,
                given=T(case['given']) if given else None, u=case['u'], triple_to_img=T(case['triple_to_img']),
                num_images=case['N'])


def _get(out):
    block, size_idx, loc_idx = out
    assert block.dtype == torch.float32 and size_idx.dtype == torch.int32 and loc_idx.dtype == torch.int32
    return size_idx.cpu().numpy(), loc_idx.cpu().numpy(), block.cpu().numpy()


# ---- statistics ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,g', cases.SHAPES + ((70, 9),))
def test_histogram_equals_numpy(S, g):
    rs = np.random.RandomState(S + g)
    O, C, A = 700, 9, S + g * g                               # three workgroups, the last one ragged
    objs = rs.randint(0, C, size=O)
    odd = rs.rand(O) < 0.1
    objs[odd] = rs.choice([-1, -7, C, C + 5, 1 << 40], size=int(odd.sum()))          # classes outside the table
    attrs = np.zeros((O, A), dtype=np.float32)
    attrs[np.arange(O), rs.randint(0, S, size=O)] = 1
    attrs[np.arange(O), S + rs.randint(0, g * g, size=O)] = 1
    attrs[rs.rand(O) < 0.2, :S] = 0                           # rows without a size bit ...
    attrs[rs.rand(O) < 0.2, S:] = 0                           # ... without a location bit
    extra = rs.rand(O, A) < 0.03                              # second bits (the first counts), values at and below the threshold
    attrs[extra] = rs.choice(np.array([1.0, 0.5, 0.75, 0.25], dtype=np.float32), size=int(extra.sum()))
    assert (objs == 0).any() and (attrs[:, :S].max(1) <= 0.5).any()
    want = ref.histogram(objs, attrs, C, S, g)
    assert want.sum() > 0 and want[0].sum() == 0
    got = ops.sg_attribute_histogram(T(objs), T(attrs), C, S, g)
    assert got.dtype == torch.int64 and (got.cpu().numpy() == want).all()
    again = ops.sg_attribute_histogram(T(objs[:300]), T(attrs[:300]), C, S, g, counts=got)       # the call ADDS
    assert again is got and (got.cpu().numpy() == ref.histogram(objs[:300], attrs[:300], C, S, g, counts=want.copy())).all()
    before = got.clone()
    ops.sg_attribute_histogram(T(objs[:0]), T(attrs[:0]), C, S, g, counts=got)                   # O = 0
    assert torch.equal(got, before)
    other = ops.sg_attribute_histogram(T(objs), T(attrs), C, S, g, image_class=3)
    assert (other.cpu().numpy() == ref.histogram(objs, attrs, C, S, g, image_class=3)).all()


def test_attribute_stats_update_accumulates():
    b1, b2 = [make_batch(N=4, size=16, mask_size=4, num_objs=12, seed=s) for s in (1, 2)]
    stats = attributes.build_stats([b1, b2], 12, device=DEV)
    want = ref.histogram(b1.objs.numpy(), b1.attributes.numpy(), 12, 10, 5)
    want = ref.histogram(b2.objs.numpy(), b2.attributes.numpy(), 12, 10, 5, counts=want)
    assert (stats.counts.cpu().numpy() == want).all() and want.sum() == 2 * ((b1.objs != 0).sum() + (b2.objs != 0).sum())


# ---- the draw --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('given', [True, False])
@pytest.mark.parametrize('rule', ['reference', 'geometric'])
@pytest.mark.parametrize('S,g', cases.SHAPES)
def test_sample_attributes_equals_restatement(S, g, rule, given):
    case = cases.make_case(S, g)
    size, loc, block = _get(attributes.sample_attributes(size_rule=rule, **_device(case, given)))
    wsize, wloc, wblock = _expected(S, g, rule, given)
    bad = np.nonzero((size != wsize) | (loc != wloc))[0]
    assert bad.size == 0, (bad[:8], size[bad[:8]], wsize[bad[:8]], loc[bad[:8]], wloc[bad[:8]])
    assert (block == wblock).all()


def test_sample_attributes_overwrites_every_output_element():
    """the raw entry point on sentinel-filled outputs, with objects that belong to no image of the call at both ends"""
    case = cases.make_case(10, 5)
    O = case['objs'].size
    o2i = case['obj_to_img'].copy() - 1                        # image 0 becomes -1; with N = 8 the old image 9 (now 8) is past the end
    t2i = case['triple_to_img'].copy() - 1
    N = 8
    size_idx = torch.full((O,), 77, dtype=torch.int32, device=DEV)
    loc_idx = torch.full((O,), 77, dtype=torch.int32, device=DEV)
    block = torch.full((O, 35), float('nan'), device=DEV)
    d = dict(objs=T(case['objs']), o2i=T(o2i), tri=T(case['triples']), t2i=T(t2i), counts=T(case['counts']), u=T(case['u']),
             given=T(case['given']))
    ops._call('sg_sample_attributes', d['objs'].data_ptr(), d['o2i'].data_ptr(), d['tri'].data_ptr(), d['t2i'].data_ptr(),
              d['counts'].data_ptr(), d['u'].data_ptr(), d['given'].data_ptr(), size_idx.data_ptr(), loc_idx.data_ptr(),
              block.data_ptr(), N, O, case['triples'].shape[0], case['C'], 10, 5, 0, 0, ops._stream())
    wsize, wloc, wblock = ref.sample(case['objs'], o2i, case['triples'], t2i, case['counts'], case['u'], case['given'], N, 10, 5)[:3]
    outside = (o2i < 0) | (o2i >= N)
    assert outside.sum() == 4 + 3 and (wsize[outside] == -1).all() and not wblock[outside].any()
    assert (size_idx.cpu().numpy() == wsize).all() and (loc_idx.cpu().numpy() == wloc).all()
    assert (block.cpu().numpy() == wblock).all()               # no NaN left
    # N = 0: nothing is assigned, everything is written
    block.fill_(float('nan'))
    size_idx.fill_(77)
    ops._call('sg_sample_attributes', d['objs'].data_ptr(), d['o2i'].data_ptr(), d['tri'].data_ptr(), d['t2i'].data_ptr(),
              d['counts'].data_ptr(), d['u'].data_ptr(), None, size_idx.data_ptr(), loc_idx.data_ptr(), block.data_ptr(), 0, O,
              case['triples'].shape[0], case['C'], 10, 5, 0, 0, ops._stream())
    assert (size_idx == -1).all() and (loc_idx == -1).all() and (block == 0).all()


def test_two_runs_are_bit_identical_and_batch_order_does_not_matter():
    case = cases.make_case(10, 5)
    a = _get(attributes.sample_attributes(**_device(case)))
    b = _get(attributes.sample_attributes(**_device(case)))
    assert all((x == y).all() for x, y in zip(a, b))
    pcase, order = cases.permute_case(case, [7, 2, 9, 0, 4, 1, 8, 3, 6, 5])
    p = _get(attributes.sample_attributes(**_device(pcase)))
    assert all((x == y[order]).all() for x, y in zip(p, a))


def test_defaults_read_obj_to_img_once(monkeypatch):
    """without num_images / the host list: one read of obj_to_img; triple_to_img from a device gather; u from the seed"""
    case = cases.make_case(10, 4)
    d = _device(case)
    reads = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, 'tolist', lambda self: (reads.append(self.is_cuda), real(self))[1])
    tri = d['triples'].clone()
    ok = (tri[:, 0] >= 0) & (tri[:, 0] < case['objs'].size)    # the gather needs subjects inside the batch
    got = _get(attributes.sample_attributes(d['objs'], tri[ok], d['obj_to_img'], d['stats'], given=d['given'], seed=11))
    assert reads == [True]
    keep = ok.cpu().numpy()
    tri_h = case['triples'][keep]
    want = ref.sample(case['objs'], case['obj_to_img'], tri_h, case['obj_to_img'][tri_h[:, 0]], case['counts'],
                      attributes.draw_uniforms(11, case['objs'].size), case['given'], case['N'], 10, 4)[:3]
    assert all((x == y).all() for x, y in zip(got, want))
    del reads[:]
    attributes.sample_attributes(d['objs'], tri[ok], d['obj_to_img'], d['stats'], obj_to_img_host=case['obj_to_img'].tolist())
    assert reads == []


# ---- the sampler -----------------------------------------------------------------------------------------------------------------
def _model():
    m = SH.small_model(Model, make_sampling_vocab(SH.C, 7, SH.A)).to(DEV)
    m.noise_override = torch.linspace(-1, 1, 64).view(1, -1)
    return m


def _batch():
    b = make_batch(N=3, min_objs=2, max_objs=4, size=32, mask_size=8, num_objs=SH.C, num_preds=7, num_attributes=35, seed=321)
    return scenegraph.regraph(b, seed=1)


def _stats():
    rs = np.random.RandomState(8)
    counts = rs.randint(0, 30, size=(SH.C, 35)).astype(np.int64)
    counts[0] = 0
    return attributes.AttributeStats(SH.C, device=DEV, counts=counts)


def test_sampler_fills_what_the_batch_leaves_open():
    m, b, stats = _model(), _batch(), _stats()
    plain = sample.Sampler(m).sample_batch(b, use_gt_textures=True)
    off = sample.Sampler(m, attribute_stats=stats, sample_attributes=False).sample_batch(b, use_gt_textures=True)
    assert torch.equal(plain.images, off.images) and torch.equal(plain.boxes_pred, off.boxes_pred)
    dev = [t.to(DEV) for t in b]
    seen = []
    real = m.forward

    def spy(*a, **k):
        seen.append(k['attributes'].clone())
        return real(*a, **k)
    m.forward = spy
    try:
        s = sample.Sampler(m, attribute_stats=stats, sample_attributes=True, attribute_seed=5, graph_metrics=True)
        on = s.sample_batch(b, use_gt_textures=True)                               # nothing given: everything drawn, seed 5
        on2 = s.sample_batch(b, use_gt_textures=True)                              # seed 6
        given = b.attributes.clone()
        given[::2] = 0                                                             # every other row left open
        b2 = b._replace(attributes=given)
        s.sample_batch(b2, use_gt_textures=True, use_gt_attr=True)                 # seed 7: the given rows stay
    finally:
        del m.forward
    zero = torch.zeros_like(dev[7])
    want5 = attributes.sample_attributes(dev[1], dev[4], dev[5], stats, given=zero, seed=5, triple_to_img=dev[6])[0]
    want6 = attributes.sample_attributes(dev[1], dev[4], dev[5], stats, given=zero, seed=6, triple_to_img=dev[6])[0]
    want7 = attributes.sample_attributes(dev[1], dev[4], dev[5], stats, given=given.to(DEV), seed=7, triple_to_img=dev[6])[0]
    assert torch.equal(seen[0], want5) and torch.equal(seen[1], want6) and torch.equal(seen[2], want7)
    assert not torch.equal(want5, want6)                                           # successive batches differ
    assert (seen[0][:, :10].sum(1) == 1).all() and (seen[0][:, 10:].sum(1) == 1).all()
    assert torch.equal(seen[2][1::2], dev[7][1::2])                                # given rows untouched
    assert not torch.equal(on.images, plain.images) and not torch.equal(on.images, on2.images)
    g = s.graph_summary()                                                          # the metrics scored the sampled attributes
    assert 0.0 <= g['size_acc'] <= 1.0 and 0.0 <= g['loc_acc'] <= 1.0
    assert int(s.graph_counts[7, 0]) == 3 * dev[1].numel() and int(s.graph_counts[8, 0]) == 3 * dev[1].numel()
    with pytest.raises(ValueError, match='given must be'):
        sample.Sampler(m, attribute_stats=attributes.AttributeStats(SH.C, 10, 4, DEV), sample_attributes=True).sample_batch(
            b, use_gt_textures=True)


def test_sampler_json_graph_without_attributes():
    m, stats = _model(), _stats()
    sgs = SH.scene_graphs()
    for sg in sgs:
        sg['attributes'] = {'size': [], 'location': []}
    sgs[0]['attributes'] = {'size': [1], 'location': [3]}                          # obj3 of the first graph: given
    seen = []
    real = m.forward

    def spy(*a, **k):
        seen.append(k['attributes'].clone())
        return real(*a, **k)
    m.forward = spy
    try:
        out = sample.Sampler(m, attribute_stats=stats, sample_attributes=True).sample_json(sgs)
    finally:
        del m.forward
    assert out.images.shape[0] == 2
    a = seen[0].cpu().numpy()
    assert a.shape == (7, 35) and (a[:, :10].sum(1) == 1).all() and (a[:, 10:].sum(1) == 1).all()
    assert a[0, 1] == 1 and a[0, 10 + 3] == 1 and a[3, 9] == 1 and a[3, 10 + 12] == 1 and a[6, 9] == 1 and a[6, 10 + 12] == 1
    # obj3 (cell 3: column 3, row 0) is left of obj5, so obj5 draws from the columns right of it -- column 4 -- and sits above obj7
    assert (np.argmax(a[1, 10:]) % 5) == 4 and np.argmax(a[2, 10:]) // 5 >= min(np.argmax(a[1, 10:]) // 5 + 1, 4)


def test_sampler_launches_and_host_reads(monkeypatch):
    """off: none of the new kernels runs; on: one more launch -- and still ONE host read"""
    m, b, stats = _model(), _batch(), _stats()
    reads = []
    for name in ('tolist', 'item', 'cpu', 'numpy'):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    profs = {}
    for on in (False, True):
        s = sample.Sampler(m, attribute_stats=stats, sample_attributes=on)
        s.sample_batch(b, use_gt_textures=True)                          # warm-up outside the profile
        ops.prof_enable(True)
        try:
            ops.prof_reset()
            del reads[:]
            s.sample_batch(b, use_gt_textures=True)
            n_reads = list(reads)
            profs[on] = ops.prof_read()
        finally:
            ops.prof_enable(False)
        assert n_reads == ['tolist'], n_reads
    assert [profs[False][k]['launches'] for k in KINDS] == [0, 0]
    assert [profs[True][k]['launches'] for k in KINDS] == [0, 1]
    for k in profs[False]:
        if k not in KINDS:
            assert profs[True][k]['launches'] == profs[False][k]['launches'], k


KW = dict(image_size=(32, 32), gconv_hidden_dim=32, gconv_num_layers=2, mask_size=8, n_downsample_global=1,
          appearance_normalization='batch', activation='leakyrelu-0.2', use_attributes=True, pool_size=2, rep_size=8)


def test_command_line(tmp_path, capsys):
    vocab = make_sampling_vocab(12, 7, 35)
    m = Model(vocab, **KW).to(DEV)
    fill_deterministic(m)
    ckpt = str(tmp_path / 'ckpt.pt')
    torch.save({'model_kwargs': dict(vocab=vocab, **KW), 'model_state': m.state_dict()}, ckpt)
    path = str(tmp_path / 'attributes_10_25.pickle')
    stats = attributes.main(['build', '--output', path, '--num_samples', '12', '--batch_size', '5', '--num_objs', '12',
                             '--image_size', '16', '--mask_size', '8'])
    assert 'Saved attributes file' in capsys.readouterr().out
    counts = stats.counts.cpu()
    assert counts.sum() > 0 and counts[0].sum() == 0 and torch.equal(counts[:, :10].sum(1), counts[:, 10:].sum(1))
    assert torch.equal(attributes.AttributeStats.load(path, vocab, device='cpu').counts, counts)
    shown = attributes.main(['show', path, '--num_objs', '12'])
    out = capsys.readouterr().out
    assert torch.equal(shown.counts, counts) and 'obj1  size ' in out and 'location ' in out
    res = sample.main(['--checkpoint', ckpt, '--output_dir', str(tmp_path / 'a'), '--num_samples', '6', '--batch_size', '3',
                       '--use_gt_textures', '1', '--sample_attributes', '1', '--attributes_file', path, '--graph_metrics', '1',
                       '--attribute_size_rule', 'geometric'])
    assert len(res['paths']) == 6 and all(os.path.isfile(p) for p in res['paths'])
    g = res['graph']
    assert 0.0 <= g['size_acc'] <= 1.0 and 0.0 <= g['loc_acc'] <= 1.0
    out = capsys.readouterr().out
    assert 'size_acc %s' % g['size_acc'] in out and 'loc_acc %s' % g['loc_acc'] in out
    npz = stats.save(str(tmp_path / 'a.npz'))
    res2 = sample.main(['--checkpoint', ckpt, '--output_dir', str(tmp_path / 'b'), '--num_samples', '6', '--batch_size', '3',
                        '--use_gt_textures', '1', '--sample_attributes', '1', '--attributes_file', npz, '--graph_metrics', '1',
                        '--attribute_size_rule', 'geometric'])
    assert res2['graph'] == g                                   # the same table from either file, the same seeds: the same run
