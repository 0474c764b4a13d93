"""The case tables of tests/graph_layout_cases.py reach the kernel branches they are there for, and its references are sound
(no GPU): the staging constants the tables were built around are the ones in the .hip sources, every case has the property that
sends it down its branch, the CSR / sequential references agree with brute-force loops and with the oracle's pool, every layout
and crop case is well enough conditioned that the fp32 CPU oracle stays within half of the GPU tolerance of the float64
reference, and every gather-linear case keeps its pre-activations away from the activation's kink."""
import os
import re

import numpy as np
import pytest
import torch

import graph_layout_cases as GL
from oracle import sg_oracle as O
from gpu_harness import close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'scene_generation_amd', 'csrc')


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.findall(pattern, text)
    assert len(set(m)) == 1, '%s: %r found %s' % (what, pattern, m)
    return int(m[0])


# =============================================================================================
# constants
# =============================================================================================
def test_constants_match_the_sources():
    g, l = _src('graph.hip'), _src('layout.hip')
    assert _one(r'constexpr int CSR_LDS_NODES = (\d+);', g, 'CSR_LDS_NODES') == GL.CSR_LDS_NODES
    assert 'if (O <= CSR_LDS_NODES)' in g, 'the CSR dispatch'
    assert _one(r'for \(int base = 0; base < 2 \* T; base \+= (\d+)\)', g, 'CSR round') == GL.CSR_ROUND
    assert _one(r'constexpr int PASS_SHIFT = (\d+);', g, 'PASS_SHIFT') == GL.PASS_SHIFT
    assert _one(r'constexpr int SEG_CAP = (\d+);', g, 'SEG_CAP') == GL.SEG_CAP
    emb = g[g.index('embedding_bwd_kernel('):]
    assert _one(r'constexpr int CAP = (\d+);', emb[:emb.index('copy_cols_kernel')], 'embedding CAP') == GL.EMB_CAP
    assert _one(r'int ysplit = \((\d+) \+ num_rows - 1\) / num_rows;', g, 'embedding blocks') == GL.EMB_BLOCKS
    assert _one(r'const int maxy = dim / (\d+) > 0', g, 'embedding columns') == GL.EMB_COLS_MIN
    assert 'if (width <= 4 * threads)' in g, 'the segment-sum dispatch'
    m = re.search(r'inline int row_threads\(int width\) \{ int t = \(\(width \+ 63\) / 64\) \* 64; '
                  r'return t > 256 \? 256 : \(t < 64 \? 64 : t\); \}', g)
    assert m, 'row_threads() changed: restate it in graph_layout_cases.row_threads'
    assert _one(r'layout_fwd_reg_kernel<(?:true|false), (\d+)>', l, 'register layout CAP') == GL.LAYOUT_REG_CAP
    assert _one(r'int cap = max_per_image > 0 \? max_per_image : (\d+);', l, 'default LDS hint') == GL.LAYOUT_REG_CAP
    assert _one(r'\(size_t\)D \* (\d+) \* sizeof\(float\) <= 64 \* 1024', l, 'register layout LDS') == GL.LAYOUT_REG_CAP
    bwd = l[l.index('layout_bwd_vecs_kernel('):]
    assert _one(r'constexpr int OC = (\d+);', bwd[:bwd.index('zero_cols_kernel')], 'OC') == GL.LAYOUT_BWD_OC
    assert _one(r'O <= (\d+) && \(size_t\)N \* M \* L', l, 'factored weights dispatch') == GL.FACTORED_LDS_OBJECTS
    assert _one(r'for \(int b0 = 0; b0 < B; b0 \+= (\d+)\)', l, 'crop round') == GL.CROP_ROUND
    assert _one(r'crop_bwd_gather_kernel<(\d+)>, dim3\(sg_cdiv\(H \* W, 256\), N\), dim3\(256\), 0, s, gout, boxes, box_to_feat,\s+'
                r'g_feats, C, H, W, B, HH, WW, g_align_corners\);\s+SG_LAUNCH', l, 'crop CT') == GL.CROP_CT
    assert 'if (C <= 1)' in l, 'the crop backward dispatch'
    assert 'const int use_vec = (W % 4 == 0) ? 4 : 1;' in l and 'if (regform && use_vec == 4 &&' in l, 'the layout dispatch'


# =============================================================================================
# branch properties
# =============================================================================================
def test_csr_cases_reach_both_builders_and_the_round_edges():
    Os = [c[0] for c in GL.CSR_CASES]
    assert GL.CSR_LDS_NODES in Os and GL.CSR_LDS_NODES + 1 in Os
    assert any(O_ > GL.CSR_LDS_NODES + 64 * 4 for O_ in Os), 'several rounds of the single-wave scan'
    assert any(T == 0 for _, T, _ in GL.CSR_CASES)
    assert any(2 * T == GL.CSR_ROUND for _, T, _ in GL.CSR_CASES)
    assert any(2 * T == GL.CSR_ROUND + 2 and T % 64 not in (0, 63) for _, T, _ in GL.CSR_CASES), 'pass boundary inside a wave'
    for O_, T, kind in GL.CSR_CASES:
        e = GL.csr_edges(O_, T, kind)
        assert e.shape == (T, 2) and (T == 0 or (e.min() >= 0 and e.max() < O_))
        if T >= 3:
            assert (e[1] == e[0]).all() and e[2, 0] == e[2, 1]
        if kind == 'star':
            ds, do = int((e[:, 0] == 0).sum()), int((e[:, 1] == 0).sum())
            assert ds + do >= GL.STAR_MIN_DEGREE > GL.SEG_CAP and ds > 4 * GL.CSR_ROUND // 2 and do > 4 * GL.CSR_ROUND // 2
    assert GL.csr_edges(1, 1, 'random').tolist() == [[0, 0]]


def test_pool_cases_cross_the_staging_chunk_and_the_column_blocks():
    e = GL.edges_with_degrees(GL.POOL_DEGREES)
    deg = np.bincount(e.reshape(-1), minlength=len(GL.POOL_DEGREES))
    assert deg.tolist() == GL.POOL_DEGREES
    assert set(deg.tolist()) == {0, 1, 7, 8, 9, 1023, 1024, 1025, 2050}
    assert {GL.SEG_CAP - 1, GL.SEG_CAP, GL.SEG_CAP + 1} <= set(deg.tolist()) and deg.max() > 2 * GL.SEG_CAP
    for i, d in enumerate(deg):                      # spread over both passes
        if d > 8:
            assert 0 < (e[:, 0] == i).sum() < d
    for H in GL.POOL_WIDTHS:
        assert not GL.segment_sum_is_wide(H)
    assert max(GL.POOL_WIDTHS) == 4 * GL.row_threads(max(GL.POOL_WIDTHS)), 'the widest staged form'
    assert any(H % GL.row_threads(H) != 0 and H > GL.row_threads(H) for H in GL.POOL_WIDTHS), 'a ragged column block'
    assert any(H < 64 for H in GL.POOL_WIDTHS)
    for H in GL.WIDE_WIDTHS:
        assert GL.segment_sum_is_wide(H)
    assert min(GL.WIDE_WIDTHS) == 4 * 256 + 1
    wd = np.bincount(GL.edges_with_degrees(GL.WIDE_DEGREES).reshape(-1), minlength=len(GL.WIDE_DEGREES))
    assert wd.tolist() == GL.WIDE_DEGREES and wd.max() >= 1030
    for Do, Dp in GL.GATHER_CONCAT_DIMS:
        assert not GL.segment_sum_is_wide(Do)


def test_embedding_cases_cross_the_chunk_and_split_the_columns_raggedly():
    ns = set(c[0] for c in GL.EMBEDDING_CASES)
    assert {0, 1, 63, 64, 65, GL.EMB_CAP, GL.EMB_CAP + 1} <= ns and max(ns) > 2 * GL.EMB_CAP
    assert set(c[1] for c in GL.EMBEDDING_CASES) == {1, 20, 180}
    assert set(c[2] for c in GL.EMBEDDING_CASES) == {1, 63, 130, 777, 3136}
    assert GL.embedding_ysplit(20, 777) == (3, 259)
    assert GL.embedding_ysplit(180, 3136) == (6, 523) and 6 * 523 > 3136, 'a shorter last column chunk'
    ragged = [(n, r, d) for n, r, d in GL.EMBEDDING_CASES
              if GL.embedding_ysplit(r, d)[0] > 1 and GL.embedding_ysplit(r, d)[1] % GL.row_threads(d) != 0]
    assert any(n > GL.EMB_CAP for n, _, _ in ragged), 'the chunk that re-reads the table gradient, with split columns'
    for n, rows, dim in GL.EMBEDDING_CASES:
        _, idx, g = GL.embedding_inputs(n, rows, dim)
        assert idx.shape == (n,) and g.shape == (n, dim)
        if rows > 1 and n:
            assert idx.max() < rows - 1, 'a never-hit row'
        if n > GL.EMB_CAP:
            assert idx[0] == idx[n - 1] == 0 and (n - 1) // GL.EMB_CAP > 0, 'row 0 is hit in the first and in the last chunk'


def test_gather_linear_cases_reach_both_loaders_and_keep_the_preactivation_margin():
    vec4 = [c for c in GL.GATHER_LINEAR_CASES if c[1] % 4 == 0 and c[2] % 4 == 0]
    vec1 = [c for c in GL.GATHER_LINEAR_CASES if not (c[1] % 4 == 0 and c[2] % 4 == 0)]
    assert any(T > 32 for T, *_ in vec4) and any(T > 32 for T, *_ in vec1), 'more than one 32-row tile per loader'
    assert GL.GATHER_LINEAR_MISALIGNED in vec4
    assert {c[4] for c in GL.GATHER_LINEAR_CASES} == {0, 1, 2}
    for case in GL.GATHER_LINEAR_CASES:
        T, Do, Dp, out_f, act = case
        for with_bias in (True, False):
            inp = GL.gather_linear_inputs(*case, with_bias=with_bias)
            assert (inp['b'] is not None) == with_bias
            assert inp['edges'][0, 0] == inp['edges'][0, 1]
            z = GL.gather_linear_preact(inp['obj'], inp['pred'], inp['edges'], inp['w'], inp['b'])
            if act != 0:
                assert np.abs(z).min() >= GL.PREACT_MARGIN, case
            ref = GL.gather_linear_ref(inp, act)
            # the fp32 rounding of the pre-activation is far below the margin: the masks of fp32 and float64 agree
            assert float(ref['y'][1].max()) < 0.5 * GL.PREACT_MARGIN
            assert set(ref) == {'y', 'g_obj', 'g_pred', 'gw'} | ({'gb'} if with_bias else set())
            # an fp32 evaluation on the CPU meets the bounds the GPU results are held to
            o, p, w = (GL.t32(inp[k]).requires_grad_() for k in ('obj', 'pred', 'w'))
            b = None if inp['b'] is None else GL.t32(inp['b']).requires_grad_()
            e = GL.t32(inp['edges'])
            y = torch.cat([o[e[:, 0]], p, o[e[:, 1]]], 1) @ w.t()
            y = GL._act64(y if b is None else y + b, act, float(np.float32(GL.LEAKY_SLOPE)))
            y.backward(GL.t32(inp['gy']))
            got = dict(y=y.detach(), g_obj=o.grad, g_pred=p.grad, gw=w.grad)
            if b is not None:
                got['gb'] = b.grad
            for k, (want, bound) in ref.items():
                assert bool(((got[k].double() - want).abs() <= bound).all()), (case, k)


def test_layout_cases_reach_both_kernels_every_chunk_count_and_empty_images():
    counts = GL.LAYOUT_COUNTS
    O_ = sum(counts)
    cap, oc = GL.LAYOUT_REG_CAP, GL.LAYOUT_BWD_OC
    assert 0 in counts[1:-1] and counts[-1] == 0 and counts[0] > 0, 'an empty image inside and at the end (o_beg == O)'
    assert cap in counts and 1 in counts and any(cap < c <= 2 * cap for c in counts) and any(c > 2 * cap for c in counts)
    assert any(c > oc and c % oc for c in counts)
    assert {(c[0], c[1]) for c in GL.LAYOUT_CASES} == {(16, 16), (22, 30), (9, 7), (33, 32), (17, 61)}
    assert {c[2] for c in GL.LAYOUT_CASES} == {5, 16} and {c[3] for c in GL.LAYOUT_CASES} == {7, 38, 200}
    assert {c[4] for c in GL.LAYOUT_CASES} == {'f32', 'i64'} and {c[5] for c in GL.LAYOUT_CASES} == {'sum', 'avg'}
    from itertools import combinations
    fields = [lambda c: (c[0], c[1]), lambda c: c[2], lambda c: c[3], lambda c: c[4], lambda c: c[5]]
    for fa, fb in combinations(fields, 2):               # every pair of values of any two fields occurs together
        va, vb = {fa(c) for c in GL.LAYOUT_CASES}, {fb(c) for c in GL.LAYOUT_CASES}
        assert {(fa(c), fb(c)) for c in GL.LAYOUT_CASES} == {(a, b) for a in va for b in vb}
    reg = [c for c in GL.LAYOUT_CASES if GL.layout_reg_plan(c[1], c[3], 1) is not None]
    lds_only = [c for c in GL.LAYOUT_CASES if c[1] % 4 != 0]
    assert reg and lds_only and len(reg) + len(lds_only) == len(GL.LAYOUT_CASES)
    for grp in (reg, lds_only):                           # both kernels (and both forms of the LDS kernel) see both mask types
        assert {c[4] for c in grp} == {'f32', 'i64'} and {c[5] for c in grp} == {'sum', 'avg'}
    assert any(c[0] * c[1] > GL.LAYOUT_REG_TILE for c in reg), 'two pixel tiles of the vector kernels'
    assert any(c[0] * c[1] > 256 and (c[0] * c[1]) % 256 for c in lds_only), 'several ragged tiles of the scalar kernel'
    plans = {(c[3], s): GL.layout_reg_plan(c[1], c[3], s) for c in reg for s in GL.LAYOUT_DSPLITS}
    assert any(z > 1 for _, z in plans.values()), 'grid.z > 1'
    assert any(s > D // 16 > 0 and z == D // 16 for (D, s), (_, z) in plans.items()), 'the D / 16 clamp'
    assert any(s > 1 and z == 1 for (D, s), (_, z) in plans.items() if D < 16), 'the clamp to one chunk'
    assert any(z > 1 and dc * z != D for (D, s), (dc, z) in plans.items()), 'a ragged last channel chunk'
    caps = {GL.layout_lds_cap(c[1], c[3], O_, m) for c in GL.LAYOUT_CASES for m in GL.LAYOUT_MAX_PER_IMAGE}
    assert cap in caps and 4 in caps and any(k >= max(counts) for k in caps)
    assert any(GL.layout_lds_cap(c[1], c[3], O_, 1000) < O_ for c in GL.LAYOUT_CASES), 'the hint clamped to what fits in LDS'
    assert 0 in GL.LAYOUT_GRAD_FROM and any(0 < g < min(c[3] for c in GL.LAYOUT_CASES) for g in GL.LAYOUT_GRAD_FROM)


def test_crop_cases_reach_both_forms_the_channel_tail_and_a_second_round():
    assert {c[0] for c in GL.CROP_CASES} == {1, 3, 4, 5, 9} and {c[1] for c in GL.CROP_CASES} == {0, 1, 256, 257, 300}
    assert {(c[2], c[3]) for c in GL.CROP_CASES} == {(1, 1), (1, 5), (7, 9), (32, 32)}
    assert any(C > 1 and C % GL.CROP_CT for C, *_ in GL.CROP_CASES) and any(C > GL.CROP_CT for C, *_ in GL.CROP_CASES)
    assert {GL.CROP_ROUND, GL.CROP_ROUND + 1} <= {c[1] for c in GL.CROP_CASES}
    N = GL.CROP_FEATS[0]
    for C, B, HH, WW in GL.CROP_CASES:
        inp = GL.crop_inputs(C, B, HH, WW)
        assert N - 1 not in inp['idx'], 'an image no box points at'
        if B > 2:
            assert (np.diff(inp['idx']) < 0).any(), 'unsorted'
        if B >= 6:
            assert set(inp['kinds']) == set(GL.CROP_BOX_KINDS)
        if B > GL.CROP_ROUND:
            assert all((inp['idx'][GL.CROP_ROUND:] == n).any() for n in (0, 1)) or B == GL.CROP_ROUND + 1
        b = inp['boxes']
        for k, (x0, y0, x1, y1) in zip(inp['kinds'], b):
            if k == 'flipped':
                assert x1 < x0
            elif k == 'zero_width':
                assert x1 == x0
            elif k == 'outside':
                assert min(x0, x1) > 1 and max(y0, y1) < 0
            elif k == 'partly_outside':
                assert x0 < 0 < x1 and y0 < 1 < y1
            elif k == 'full':
                assert (x0, y0, x1, y1) == (0, 0, 1, 1)
        assert np.isfinite(b).all()
    assert GL.crop_inputs(3, 1, 1, 1)['kinds'] == ['flipped']


def test_factored_cases_sit_on_both_sides_of_the_dispatch():
    Os = {c[0] for c in GL.FACTORED_CASES}
    assert Os == {GL.FACTORED_LDS_OBJECTS, GL.FACTORED_LDS_OBJECTS + 1} and {c[1] for c in GL.FACTORED_CASES} == {0, 2}
    inp = GL.factored_inputs(4097, 2)
    assert inp['seg'].tolist() == [0, 2000, 2001, 4097] and inp['L'] == 2098 and inp['img_idx'].shape == (4097,)


# =============================================================================================
# references
# =============================================================================================
@pytest.mark.parametrize('O_,T,kind', [c for c in GL.CSR_CASES if c[0] * c[1] <= 40 * 1300] + [(7, 40, 'random')])
def test_csr_reference_equals_the_brute_force_loop(O_, T, kind):
    e = GL.csr_edges(O_, T, kind)
    off, ent = GL.csr_ref(e, O_)
    off_b, ent_b = GL.csr_brute(e.tolist(), O_)
    assert off.dtype == np.int32 and ent.dtype == np.int32 and ent.shape == (2 * T,)
    assert np.array_equal(off, off_b) and np.array_equal(ent, ent_b)
    p, t = GL.csr_decode(ent)
    assert np.array_equal(np.sort(p * T + t), np.arange(2 * T))


@pytest.mark.parametrize('avg', [False, True])
def test_sequential_reference_equals_the_oracle_pool_and_a_plain_loop(avg):
    H = 70
    for degrees in (GL.POOL_DEGREES, GL.WIDE_DEGREES):
        e, new_t = GL.pool_inputs(degrees, H, GL.POOL_DOUT)
        O_ = len(degrees)
        rs, ro = new_t[:, :H], new_t[:, H + GL.POOL_DOUT:]
        seq, s64, bound = GL.pool_ref(rs, ro, e, O_, avg)
        want = O.pool_triples(GL.t32(rs), GL.t32(ro), GL.t32(e[:, 0]), GL.t32(e[:, 1]), O_, 'avg' if avg else 'sum')
        assert seq.dtype == np.float32 and np.array_equal(seq, want.numpy()), 'np.add.at is the sequential scatter_add order'
        idx, rows = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([rs, ro], 0)
        assert np.array_equal(GL.scatter_rows(idx, rows, O_, np.float32), GL.scatter_rows_loop(idx, rows, O_, np.float32))
        assert (np.abs(seq.astype(np.float64) - s64) <= bound).all(), 'the sequential fp32 sum meets its own bound'
        assert (bound[np.asarray(degrees) <= 1] == 0).all() or avg
        # and the bound is not vacuous: the long sums really round
        assert np.abs(seq.astype(np.float64) - s64).max() > 0


def test_embedding_reference_equals_index_add():
    n, rows, dim = 1025, 20, 777
    _, idx, g = GL.embedding_inputs(n, rows, dim)
    seq, s64, bound = GL.embedding_bwd_ref(idx, g, rows)
    want = torch.zeros(rows, dim).index_add_(0, GL.t32(idx), GL.t32(g))
    assert np.array_equal(seq, want.numpy())
    assert (np.abs(seq.astype(np.float64) - s64) <= bound).all() and (seq[rows - 1] == 0).all()


@pytest.mark.parametrize('case', GL.LAYOUT_CASES, ids=lambda c: '%dx%d_M%d_D%d_%s_%s' % c)
def test_layout_cases_are_well_conditioned(case):
    """the fp32 CPU oracle stays within half of the GPU tolerance of the float64 reference"""
    H, W, M, D, mdtype, pooling = case
    inp = GL.layout_inputs(H, W, M, D, mdtype)
    r64 = GL.layout_ref(inp, H, W, pooling)
    r32 = GL.layout_ref(inp, H, W, pooling, torch.float32)
    empty = [n for n, c in enumerate(GL.LAYOUT_COUNTS) if c == 0]
    assert float(r64['out'][empty].abs().max()) == 0.0
    for k, tol in GL.LAYOUT_TOL.items():
        if r64[k] is None:
            assert k == 'g_masks' and mdtype == 'i64'
            continue
        close(r32[k], r64[k], tol / 2, '%s (fp32 oracle vs float64)' % k)


@pytest.mark.parametrize('case', GL.CROP_CASES, ids=lambda c: 'C%d_B%d_%dx%d' % c)
def test_crop_cases_are_well_conditioned(case):
    C, B, HH, WW = case
    inp = GL.crop_inputs(C, B, HH, WW)
    r64, r32 = GL.crop_ref(inp, HH, WW), GL.crop_ref(inp, HH, WW, torch.float32)
    assert torch.isfinite(r64['out']).all() and tuple(r64['out'].shape) == (B, C, HH, WW)
    assert float(r64['g_feats'][GL.CROP_FEATS[0] - 1].abs().max()) == 0.0, 'the image no box points at'
    for k, tol in GL.CROP_TOL.items():
        close(r32[k], r64[k], tol / 2, '%s (fp32 oracle vs float64)' % k)
    for b, kind in enumerate(inp['kinds']):
        if kind == 'outside':
            assert float(r64['out'][b].abs().max()) == 0.0


def test_factored_reference_equals_the_dense_statement():
    """the float64 restatement against the definition it abbreviates: conv weights applied to [one_hot(class) | repr]"""
    inp = GL.factored_inputs(4097, 2)
    ref = GL.factored_ref(inp, 2)
    d = GL.FACTORED_DIMS
    W = GL.t32(inp['weight']).double()[:, :, 0, 0]                                  # [M, Ct]
    vec = torch.cat([torch.nn.functional.one_hot(GL.t32(inp['objs']), d['C']).double(), GL.t32(inp['repr']).double()], 1)
    weff = vec @ W[:, :d['C'] + d['R']].t()                                         # [O, M]
    wimg = ref['wimg'][0][..., 0, 0]
    beg = 0
    for n, c in enumerate(inp['counts']):
        assert torch.allclose(wimg[n, :, :c], weff[beg:beg + c].t(), rtol=0, atol=1e-14)
        assert torch.equal(wimg[n, :, c:c + 2], W[:, d['C'] + d['R']:]) and float(wimg[n, :, c + 2:].abs().max() if c + 2 < inp['L'] else 0) == 0
        beg += c
    for k in ('wimg', 'gw', 'grepr'):
        assert ref[k][0].shape == ref[k][1].shape and float(ref[k][1].min()) >= 0
