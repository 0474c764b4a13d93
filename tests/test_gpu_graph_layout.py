"""Every branch of the scene-graph (csrc/graph.hip), gathered-loader (csrc/skinny.hip), layout and crop (csrc/layout.hip) kernels
against a float64 reference of the same operation.  The cases, their inputs and the references are tests/graph_layout_cases.py;
tests/test_graph_layout_cases_cpu.py shows that the cases reach the branches and that the references are sound.

Sums in a fixed order are held to two things: bit-equality with a sequential fp32 sum in the documented order (the kernels'
"same adds, same order" contract) and the rounding bound gamma(n - 1) sum|x_i| against float64.  Layout and crop outputs also
carry the rounding of the sample coordinate and use close() of tests/gpu_harness.py with the project's tolerances
(graph_layout_cases.LAYOUT_TOL / CROP_TOL).  The worst error / bound ratio of every family is written to
graph_layout_margins.json next to the suite's other calibration records."""
import functools

import numpy as np
import pytest
import torch

import graph_layout_cases as GL
import norm_cases as NC
from gpu_harness import Margins, margins_fixture, same
from gpu_harness import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGINS = Margins()
within, close_noted = MARGINS.within, MARGINS.close_noted
_margins = margins_fixture(lambda: MARGINS.dump('graph_layout_margins.json'))      # the worst error / bound ratio per family


def dev(a, grad=False):
    t = (GL.t32(a) if isinstance(a, np.ndarray) else a).to(DEV)
    return t.requires_grad_() if grad else t


# =============================================================================================
# CSR
# =============================================================================================
@pytest.mark.parametrize('O_,T,kind', GL.CSR_CASES)
def test_build_csr(hip, O_, T, kind):
    e = GL.csr_edges(O_, T, kind)
    off, ent = hip.build_csr(dev(e), O_)
    want_off, want_ent = GL.csr_ref(e, O_)
    assert off.dtype == torch.int32 and ent.dtype == torch.int32
    assert same(off, want_off), 'csr_off'
    assert same(ent[:2 * T], want_ent), 'csr_ent: (pass, t) ascending inside every node'


# =============================================================================================
# segment sums: TriplePoolFn, GatherConcatFn backward, pool_bwd
# =============================================================================================
@functools.lru_cache(maxsize=None)
def _pool_case(H, wide):
    degrees = GL.WIDE_DEGREES if wide else GL.POOL_DEGREES
    e, new_t = GL.pool_inputs(degrees, H, GL.POOL_DOUT)
    return len(degrees), e, new_t


@pytest.mark.parametrize('H,wide', [(H, False) for H in GL.POOL_WIDTHS] + [(H, True) for H in GL.WIDE_WIDTHS])
def test_triple_pool(hip, H, wide):
    O_, e, new_t = _pool_case(H, wide)
    Dout = GL.POOL_DOUT
    T = e.shape[0]
    ed = dev(e)
    off, ent = hip.build_csr(ed, O_)
    assert same(off, GL.csr_ref(e, O_)[0])
    rng = np.random.RandomState(H)
    gp, gnp = GL._f32(rng, (O_, H)), GL._f32(rng, (T, Dout))
    for avg in (False, True):
        name = 'H=%d %s' % (H, 'avg' if avg else 'sum')
        seq, s64, bound = GL.pool_ref(new_t[:, :H], new_t[:, H + Dout:], e, O_, avg)
        x = dev(new_t, grad=True)
        pooled, new_p = hip.TriplePoolFn.apply(x, ed, off, ent, O_, H, Dout, avg)
        assert same(new_p, new_t[:, H:H + Dout]), 'new_p is the column slice'
        within('pool', pooled, s64, bound, name)
        assert same(pooled, seq), '%s: the pool adds in (pass, t) order, one fp32 add per entry' % name
        again, _ = hip.TriplePoolFn.apply(dev(new_t), ed, off, ent, O_, H, Dout, avg)
        assert torch.equal(again, pooled), 'bit-identical from run to run'
        # pool_bwd, g_new_p given (through autograd) and absent (the entry point itself)
        ((pooled * dev(gp)).sum() + (new_p * dev(gnp)).sum()).backward()
        ref, bnd = GL.pool_bwd_ref(gp, gnp, e, O_, H, Dout, avg)
        within('pool_bwd', x.grad, ref, bnd, name)
        g = torch.empty(T, 2 * H + Dout, device=DEV)
        gpd = dev(gp)
        hip._call('sg_pool_bwd', gpd.data_ptr(), None, ed.data_ptr(), off.data_ptr(), g.data_ptr(), T, H, Dout, 1 if avg else 0,
                  hip._stream())
        ref, bnd = GL.pool_bwd_ref(gp, None, e, O_, H, Dout, avg)
        within('pool_bwd', g, ref, bnd, name + ' (no g_new_p)')
        assert float(g[:, H:H + Dout].abs().max()) == 0.0


def test_graph_without_triples(hip):
    """T = 0: empty per-triple tensors have no storage; the entry points take their null pointers and still write the rest"""
    O_, H, Dout = 9, 70, 3
    ed = torch.zeros(0, 2, dtype=torch.int64, device=DEV)
    off, ent = hip.build_csr(ed, O_)
    assert same(off, np.zeros(O_ + 1, dtype=np.int32))
    for avg in (False, True):
        x = torch.zeros(0, 2 * H + Dout, device=DEV, requires_grad=True)
        pooled, new_p = hip.TriplePoolFn.apply(x, ed, off, ent, O_, H, Dout, avg)
        assert tuple(pooled.shape) == (O_, H) and float(pooled.detach().abs().max()) == 0.0
        assert tuple(new_p.shape) == (0, Dout)
        (pooled.sum() + new_p.sum()).backward()
        assert tuple(x.grad.shape) == (0, 2 * H + Dout)
    # the gather side of the layer on the same empty graph: empty rows out, all-zero node gradients back
    Do, Dp, out_f = 6, 10, 40
    rng = np.random.RandomState(0)
    for fused in (False, True):
        obj, pred = dev(GL._f32(rng, (O_, Do)), grad=True), torch.zeros(0, Dp, device=DEV, requires_grad=True)
        if fused:
            w, b = dev(GL._f32(rng, (out_f, 2 * Do + Dp)), grad=True), dev(GL._f32(rng, (out_f,)), grad=True)
            out = hip.gather_linear(obj, pred, ed, off, ent, w, b, 1, 0.0)
            assert tuple(out.shape) == (0, out_f)
        else:
            out = hip.GatherConcatFn.apply(obj, pred, ed, off, ent)
            assert tuple(out.shape) == (0, 2 * Do + Dp)
        out.sum().backward()
        assert tuple(obj.grad.shape) == (O_, Do) and float(obj.grad.abs().max()) == 0.0
        assert tuple(pred.grad.shape) == (0, Dp)
        if fused:
            assert float(w.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0


@pytest.mark.parametrize('Do,Dp', GL.GATHER_CONCAT_DIMS)
def test_gather_concat_backward(hip, Do, Dp):
    """the col_off1 = Do + Dp, src_ld = 2 Do + Dp form of the segment sum"""
    O_, T = GL.GATHER_CONCAT_OT
    e = GL.csr_edges(O_, T, 'random', seed=Do)
    rng = np.random.RandomState(Do + Dp)
    obj, pred, g = GL._f32(rng, (O_, Do)), GL._f32(rng, (T, Dp)), GL._f32(rng, (T, 2 * Do + Dp))
    ed = dev(e)
    off, ent = hip.build_csr(ed, O_)
    od, pd = dev(obj, grad=True), dev(pred, grad=True)
    out = hip.GatherConcatFn.apply(od, pd, ed, off, ent)
    assert same(out, np.concatenate([obj[e[:, 0]], pred, obj[e[:, 1]]], 1))
    out.backward(dev(g))
    seq, s64, bound = GL.pool_ref(g[:, :Do], g[:, Do + Dp:], e, O_, False)
    within('gather_concat_bwd', od.grad, s64, bound, 'Do=%d Dp=%d' % (Do, Dp))
    assert same(od.grad, seq) and same(pd.grad, g[:, Do:Do + Dp])


# =============================================================================================
# embedding, one_hot, concat_cols
# =============================================================================================
@pytest.mark.parametrize('n,rows,dim', GL.EMBEDDING_CASES)
def test_embedding(hip, n, rows, dim):
    table, idx, g = GL.embedding_inputs(n, rows, dim)
    seq, s64, bound = GL.embedding_bwd_ref(idx, g, rows)
    grads = []
    for rep in range(2):
        td = dev(table, grad=True)
        out = hip.embedding(td, dev(idx))
        assert same(out, table[idx]), 'the forward is a copy'
        out.backward(dev(g))
        grads.append(td.grad)
    name = 'n=%d rows=%d dim=%d' % (n, rows, dim)
    assert tuple(grads[0].shape) == (rows, dim)
    within('embedding_bwd', grads[0], s64, bound, name)
    assert same(grads[0], seq), '%s: rows of g are added in ascending i, one fp32 add each' % name
    assert torch.equal(grads[0], grads[1]), 'bit-identical from run to run'
    hit = np.bincount(idx, minlength=rows) > 0
    assert float(grads[0][dev(~hit)].abs().max() if (~hit).any() else 0.0) == 0.0, 'never-hit rows are exactly zero'


@pytest.mark.parametrize('n,classes', [(70, 37), (33, 179), (1, 1)])
def test_one_hot_at_odd_widths(hip, n, classes):
    idx = np.random.RandomState(n).randint(0, classes, size=(n,)).astype(np.int64)
    assert same(hip.one_hot(dev(idx), classes), np.eye(classes, dtype=np.float32)[idx])


@pytest.mark.parametrize('rows,widths', [(33, (5, 67, 130)), (1, (1, 63)), (70, (179, 3))])
def test_concat_cols_at_odd_widths(hip, rows, widths):
    rng = np.random.RandomState(rows)
    parts = [GL._f32(rng, (rows, w)) for w in widths]
    g = GL._f32(rng, (rows, sum(widths)))
    ds = [dev(p, grad=True) for p in parts]
    out = hip.concat_cols(*ds)
    assert same(out, np.concatenate(parts, 1))
    out.backward(dev(g))
    o = 0
    for d, w in zip(ds, widths):
        assert same(d.grad, g[:, o:o + w])
        o += w


# =============================================================================================
# gather-linear
# =============================================================================================
GL_MODES = [('default', 'linear_skinny', None), ('materialised', 'gconv_fused_gather', 0), ('tiled', 'linear_skinny', 0)]


def _misaligned(a, grad):
    """a [1:] view of a flat device buffer: 4 bytes off 16-byte alignment"""
    buf = torch.empty(a.size + 4, dtype=torch.float32, device=DEV)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(GL.t32(a))
    assert v.data_ptr() % 16 == 4
    return v.detach().requires_grad_() if grad else v


def _gather_linear_run(hip, inp, act, misaligned=False):
    ed = dev(inp['edges'])
    off, ent = hip.build_csr(ed, inp['O'])
    obj, w = dev(inp['obj'], grad=True), dev(inp['w'], grad=True)
    pred = _misaligned(inp['pred'], True) if misaligned else dev(inp['pred'], grad=True)
    b = None if inp['b'] is None else dev(inp['b'], grad=True)
    y = hip.gather_linear(obj, pred, ed, off, ent, w, b, act, GL.LEAKY_SLOPE)
    y.backward(dev(inp['gy']))
    got = dict(y=y.detach(), g_obj=obj.grad, g_pred=pred.grad, gw=w.grad)
    if b is not None:
        got['gb'] = b.grad
    return got


@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('case', GL.GATHER_LINEAR_CASES, ids=lambda c: 'T%d_Do%d_Dp%d_out%d_act%d' % c)
def test_gather_linear(hip, case, with_bias):
    T, Do, Dp, out_f, act = case
    inp = GL.gather_linear_inputs(*case, with_bias=with_bias)
    ref = GL.gather_linear_ref(inp, act)
    res = {}
    runs = [(m, False) for m in GL_MODES]
    if case == GL.GATHER_LINEAR_MISALIGNED:
        runs.append((GL_MODES[0], True))
    for (mode, opt, val), mis in runs:
        with NC.option(opt, val):
            got = _gather_linear_run(hip, inp, act, mis)
        tag = '%s %s%s%s' % (case, mode, ' bias' if with_bias else '', ' misaligned pred' if mis else '')
        for k, (want, bound) in ref.items():
            within('gather_linear_y' if k == 'y' else 'gather_linear_grads', got[k], want, bound, '%s %s' % (tag, k))
        res[(mode, mis)] = got
    # the fused loader and the materialised rows feed the same register-streaming MFMA chain with the same values
    assert torch.equal(res[('default', False)]['y'], res[('materialised', False)]['y']), 'a gathered loader read another element'
    if case == GL.GATHER_LINEAR_MISALIGNED:
        assert torch.equal(res[('default', True)]['y'], res[('default', False)]['y']), '4-byte and 16-byte gathered loaders differ'


# =============================================================================================
# layout
# =============================================================================================
@functools.lru_cache(maxsize=None)
def _layout_case(case):
    H, W, M, D, mdtype, pooling = case
    inp = GL.layout_inputs(H, W, M, D, mdtype)
    return inp, GL.layout_ref(inp, H, W, pooling)


def _layout_fwd(inp, H, W, pooling, **kw):
    from scene_generation_amd.layout import masks_to_layout
    N = len(GL.LAYOUT_COUNTS)
    with torch.no_grad():
        return masks_to_layout(dev(inp['vecs']), dev(inp['boxes']), dev(inp['masks']), dev(inp['obj_to_img']), H, W, pooling=pooling,
                               num_images=N, validate=False, **kw)


@pytest.mark.parametrize('case', GL.LAYOUT_CASES, ids=lambda c: '%dx%d_M%d_D%d_%s_%s' % c)
def test_layout_forward(hip, case):
    H, W, M, D, mdtype, pooling = case
    inp, ref = _layout_case(case)
    empty = [n for n, c in enumerate(GL.LAYOUT_COUNTS) if c == 0]
    name = '%dx%d M=%d D=%d %s %s' % case
    runs = []
    if GL.layout_reg_plan(W, D, 1) is not None:
        runs += [('layout_reg=1 dsplit=%d' % s, 1, s, 0) for s in GL.LAYOUT_DSPLITS]
    runs += [('layout_reg=0 max_per_image=%d' % m, 0, None, m) for m in GL.LAYOUT_MAX_PER_IMAGE]
    outs = {}
    for tag, reg, dsplit, mpi in runs:
        with NC.option('layout_reg', reg), NC.option('layout_dsplit', dsplit):
            out = _layout_fwd(inp, H, W, pooling, max_per_image=mpi)
            again = _layout_fwd(inp, H, W, pooling, max_per_image=mpi)
        close_noted('layout', out, ref['out'], GL.LAYOUT_TOL['out'], '%s %s' % (name, tag))
        assert float(out[empty].abs().max()) == 0.0, '%s: images without objects are exactly zero' % tag
        assert torch.equal(out, again), '%s: bit-identical from run to run' % tag
        outs.setdefault(reg, []).append((tag, out))
    for reg, lst in outs.items():           # chunking over channels / objects changes neither the adds nor their order
        for tag, out in lst[1:]:
            assert torch.equal(out, lst[0][1]), '%s differs from %s' % (tag, lst[0][0])


@pytest.mark.parametrize('grad_from', GL.LAYOUT_GRAD_FROM)
@pytest.mark.parametrize('case', GL.LAYOUT_CASES, ids=lambda c: '%dx%d_M%d_D%d_%s_%s' % c)
def test_layout_backward(hip, case, grad_from):
    from scene_generation_amd.layout import masks_to_layout
    H, W, M, D, mdtype, pooling = case
    inp, ref = _layout_case(case)
    name = '%dx%d M=%d D=%d %s %s grad_from=%d' % (case + (grad_from,))
    vecs = dev(inp['vecs'], grad=True)
    masks = dev(inp['masks'], grad=(mdtype == 'f32'))
    out = masks_to_layout(vecs, dev(inp['boxes']), masks, dev(inp['obj_to_img']), H, W, pooling=pooling,
                          num_images=len(GL.LAYOUT_COUNTS), validate=False, grad_from_channel=grad_from)
    close_noted('layout', out, ref['out'], GL.LAYOUT_TOL['out'], name)
    (out * dev(inp['w'])).sum().backward()
    close_noted('layout_g_vecs', vecs.grad[:, grad_from:], ref['g_vecs'][:, grad_from:], GL.LAYOUT_TOL['g_vecs'], name + ' g_vecs')
    if grad_from:
        assert float(vecs.grad[:, :grad_from].abs().max()) == 0.0
    if mdtype == 'f32':
        close_noted('layout_g_masks', masks.grad, ref['g_masks'], GL.LAYOUT_TOL['g_masks'], name + ' g_masks')


# =============================================================================================
# crops
# =============================================================================================
@pytest.mark.parametrize('case', GL.CROP_CASES, ids=lambda c: 'C%d_B%d_%dx%d' % c)
def test_crop(hip, case):
    from scene_generation_amd.bilinear import crop_bbox_batch
    C, B, HH, WW = case
    inp = GL.crop_inputs(C, B, HH, WW)
    ref = GL.crop_ref(inp, HH, WW)
    name = 'C=%d B=%d %dx%d' % case
    grads = []
    for rep in range(2):
        feats = dev(inp['feats'], grad=True)
        junk = torch.full_like(feats, 7.0)       # freed at once: the gradient buffer allocated next reuses a block that is not zero
        del junk
        out = crop_bbox_batch(feats, dev(inp['boxes']), dev(inp['idx']), HH, WW)
        assert tuple(out.shape) == (B, C, HH, WW)
        (out * dev(inp['w'])).sum().backward()
        grads.append(feats.grad)
    close_noted('crop', out, ref['out'], GL.CROP_TOL['out'], name)
    close_noted('crop_g_feats', grads[0], ref['g_feats'], GL.CROP_TOL['g_feats'], name + ' g_feats')
    assert float(grads[0][GL.CROP_FEATS[0] - 1].abs().max()) == 0.0, 'the image no box points at'
    assert torch.equal(grads[0], grads[1]), 'bit-identical from run to run'
    if B == 0:
        assert float(grads[0].abs().max()) == 0.0, 'no boxes: an all-zero gradient'


# =============================================================================================
# factored weights
# =============================================================================================
@pytest.mark.parametrize('O_,C2', GL.FACTORED_CASES)
def test_factored_weights(hip, O_, C2):
    d = GL.FACTORED_DIMS
    inp = GL.factored_inputs(O_, C2)
    ref = GL.factored_ref(inp, C2)
    weight, rp = dev(inp['weight'], grad=True), dev(inp['repr'], grad=True)
    wimg = hip.FactoredWeightsFn.apply(weight, rp, dev(inp['objs']), dev(inp['seg']), dev(inp['img_idx']), d['N'], inp['L'], d['C'], C2)
    (wimg * dev(inp['g'])).sum().backward()
    name = 'O=%d C2=%d' % (O_, C2)
    within('factored_weights', wimg, ref['wimg'][0], ref['wimg'][1], name + ' wimg')
    within('factored_weights', weight.grad, ref['gw'][0], ref['gw'][1], name + ' gw')
    within('factored_weights', rp.grad, ref['grepr'][0], ref['grepr'][1], name + ' grepr')
