"""Case tables, input builders and float64 references of the scene-graph, layout and crop kernel tests, shared by
tests/test_graph_layout_cases_cpu.py (every table entry reaches the branch it is there for; the references are sound) and
tests/test_gpu_graph_layout.py (every case on the device).  Nothing here needs a GPU.

The tables are built around the staging sizes of the kernels, restated below; test_graph_layout_cases_cpu.py reads the same
numbers out of the .hip sources, so a changed constant fails there instead of silently un-covering a branch.

Error bounds: u = 2^-24 (fp32 unit roundoff), gamma(n) = n u / (1 - n u).  A sum of n fp32 terms in any fixed order differs from
the exact sum by at most gamma(n - 1) sum|x_i|; every further rounding of the result (a division, a product) adds one to n.
"""
import numpy as np
import torch

U = 2.0 ** -24

# ---- constants of the kernels (scene_generation_amd/csrc/graph.hip, layout.hip) -----------------------------------------------
CSR_LDS_NODES = 8192         # graph.hip: largest O of the one-workgroup csr_build_kernel
CSR_ROUND = 256              # entries placed per round of csr_build_kernel
SEG_CAP = 1024               # graph.hip: entries staged per chunk of segment_sum_kernel
EMB_CAP = 1024               # graph.hip: indices searched per chunk of embedding_bwd_kernel
EMB_COLS_MIN = 256           # graph.hip: sg_embedding_bwd gives a column chunk at least this many columns
EMB_BLOCKS = 1024            # graph.hip: workgroups sg_embedding_bwd aims at
LAYOUT_REG_CAP = 12          # layout.hip: objects per pass of layout_fwd_reg_kernel<., 12>; also the default LDS hint
LAYOUT_BWD_OC = 8            # layout.hip: objects per pass of layout_bwd_vecs_kernel
LAYOUT_REG_TILE = 1024       # pixels per workgroup of the register kernel (256 threads x 4)
CROP_ROUND = 256             # layout.hip: boxes compacted per round of crop_bwd_gather_kernel
CROP_CT = 4                  # layout.hip: channels per pass of crop_bwd_gather_kernel<4>
FACTORED_LDS_OBJECTS = 4096  # layout.hip: largest O of factored_weights_bwd_w_lds_kernel
PASS_SHIFT = 30              # graph.hip: csr_ent = t | pass << 30


def gamma(n):
    n = np.maximum(np.asarray(n, dtype=np.float64), 0.0)
    return n * U / (1.0 - n * U)


def row_threads(width):
    """graph.hip: row_threads()"""
    t = ((width + 63) // 64) * 64
    return 256 if t > 256 else (64 if t < 64 else t)


def segment_sum_is_wide(width):
    """graph.hip: sg_segment_sum launches segment_sum_wide_kernel"""
    return width > 4 * row_threads(width)


def embedding_ysplit(rows, dim):
    """graph.hip: sg_embedding_bwd -> (grid.y, columns per chunk)"""
    ysplit = (EMB_BLOCKS + rows - 1) // rows
    maxy = max(dim // EMB_COLS_MIN, 1)
    ysplit = min(ysplit, maxy)
    return ysplit, (dim + ysplit - 1) // ysplit


def _rng(seed):
    return np.random.RandomState(seed)


def _f32(rng, shape, lo=-1.0, hi=1.0):
    return (rng.rand(*shape) * (hi - lo) + lo).astype(np.float32)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# =============================================================================================
# CSR
# =============================================================================================
# (O, T, kind)
CSR_CASES = [
    (1, 1, 'random'),            # self loop
    (9, 0, 'random'),            # T = 0
    (64, 128, 'random'),         # exactly one 256-entry round
    (300, 129, 'random'),        # one round plus two entries; the pass boundary (entry 129) falls inside a wave
    (8192, 700, 'random'),       # largest O on the LDS path
    (8193, 700, 'random'),       # the three-kernel path
    (9000, 1500, 'random'),      # the three-kernel path, several waves of the scan and its 64-wide carry
    (40, 1300, 'star'),          # node 0 holds >= 1100 entries spread over both passes
]
STAR_MIN_DEGREE = 1100


def csr_edges(O, T, kind, seed=0):
    """(T, 2) int64.  'random': uniform node ids with a duplicate triple and a self loop; 'star': node 0 is the subject of 600
    triples and the object of 550 others, in shuffled positions"""
    rng = _rng(1000 + 7 * O + T + seed)
    e = rng.randint(0, O, size=(T, 2)).astype(np.int64)
    if kind == 'star':
        assert T >= 1150 and O > 1
        e = rng.randint(1, O, size=(T, 2)).astype(np.int64)
        pos = rng.permutation(T)
        e[pos[:600], 0] = 0
        e[pos[600:1150], 1] = 0
    if T >= 2:
        e[1] = e[0]                  # duplicate triple
    if T >= 3:
        e[2, 1] = e[2, 0]            # s == o
    return e


def csr_ref(edges, O):
    """-> (off [O + 1] int32, ent [2 T] int32): the entries (pass, t), pass in (0, 1) and t ascending, stably sorted by destination
    node; ent = t | pass << 30"""
    edges = np.asarray(edges)
    T = edges.shape[0]
    dest = np.concatenate([edges[:, 0], edges[:, 1]]) if T else np.zeros((0,), dtype=np.int64)
    order = np.argsort(dest, kind='stable')
    ent = np.where(order >= T, (order - T) | (1 << PASS_SHIFT), order).astype(np.int32)
    deg = np.bincount(dest, minlength=O)
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    return off, ent


def csr_brute(edges, O):
    """the same, by the definition: node by node, the s pass then the o pass"""
    off, ent = [0], []
    for i in range(O):
        for p in (0, 1):
            for t in range(len(edges)):
                if edges[t][p] == i:
                    ent.append(t | (p << PASS_SHIFT))
        off.append(len(ent))
    return np.asarray(off, dtype=np.int32), np.asarray(ent, dtype=np.int32)


def csr_decode(ent):
    ent = np.asarray(ent)
    return ent >> PASS_SHIFT, ent & ((1 << PASS_SHIFT) - 1)


# =============================================================================================
# segment sums / pool / embedding gradient: the order reference (fp32, sequential) and float64
# =============================================================================================
def scatter_rows(idx, rows, O, dtype):
    """out[idx[e]] += rows[e] for e ascending, one add per element in ``dtype``"""
    out = np.zeros((O, rows.shape[1]), dtype=dtype)
    np.add.at(out, np.asarray(idx), rows.astype(dtype))
    return out


def scatter_rows_loop(idx, rows, O, dtype):
    out = np.zeros((O, rows.shape[1]), dtype=dtype)
    rows = rows.astype(dtype)
    for e, i in enumerate(idx):
        out[i] += rows[e]
    return out


def pool_ref(rows_s, rows_o, edges, O, avg):
    """TriplePool / segment sums over the (pass, t) entries: rows_s[t] goes to edges[t, 0], then rows_o[t] to edges[t, 1].
    -> (sequential fp32 result, float64 result, per-element bound of |fp32 kernel - float64|)"""
    idx = np.concatenate([edges[:, 0], edges[:, 1]])
    rows = np.concatenate([rows_s, rows_o], 0)
    deg = np.bincount(idx, minlength=O).astype(np.float64)
    seq = scatter_rows(idx, rows, O, np.float32)
    s64 = scatter_rows(idx, rows, O, np.float64)
    mag = scatter_rows(idx, np.abs(rows), O, np.float64)
    bound = gamma(deg - 1)[:, None] * mag
    if avg:
        den = np.maximum(deg, 1.0)
        seq = seq / den.astype(np.float32)[:, None]
        s64 = s64 / den[:, None]
        bound = bound / den[:, None]
        bound = bound + U * (np.abs(s64) + bound)        # one more rounding, of the computed quotient
    return seq, s64, bound


def pool_bwd_ref(gp, gnp, edges, O, H, Dout, avg):
    """-> (float64 [T, 2 H + Dout], bound): [gp[s] / deg_s | gnp or 0 | gp[o] / deg_o]; a copy or one division: 2 u |value|"""
    T = edges.shape[0]
    deg = np.maximum(np.bincount(edges.reshape(-1), minlength=O), 1).astype(np.float64)
    gp = gp.astype(np.float64)
    ds = deg[edges[:, 0]][:, None] if avg else 1.0
    do = deg[edges[:, 1]][:, None] if avg else 1.0
    mid = np.zeros((T, Dout)) if gnp is None else gnp.astype(np.float64)
    ref = np.concatenate([gp[edges[:, 0]] / ds, mid, gp[edges[:, 1]] / do], 1)
    return ref, 2 * U * np.abs(ref)


# degrees (number of (pass, t) entries) per node: every value of {0, 1, 7, 8, 9, 1023, 1024, 1025, 2050} -- around the 8-entry
# unroll and the SEG_CAP chunk, two full chunks plus two entries -- and a second node of degree 1 (an even number of entries)
POOL_DEGREES = [0, 1, 7, 8, 9, 1023, 1024, 1025, 2050, 1]
POOL_WIDTHS = [1, 5, 70, 257, 1024]                  # H: one thread live, a ragged block, two / four ragged column blocks, the cap
POOL_DOUT = 3
WIDE_DEGREES = [1040, 3, 0, 9, 2]                    # one node beyond SEG_CAP
WIDE_WIDTHS = [1025, 1100]                           # > 4 * row_threads: segment_sum_wide_kernel
GATHER_CONCAT_DIMS = [(3, 5), (8, 8), (163, 128)]    # (Do, Dp) of the GatherConcatFn backward form
GATHER_CONCAT_OT = (30, 80)


def edges_with_degrees(degrees, seed=0):
    """(T, 2) int64 whose nodes have exactly these entry counts: the multiset of node ids is shuffled and split into the subject
    and the object column, so every node's entries are spread over both passes"""
    ids = np.repeat(np.arange(len(degrees), dtype=np.int64), degrees)
    assert ids.size % 2 == 0
    ids = ids[_rng(77 + seed).permutation(ids.size)]
    T = ids.size // 2
    return np.stack([ids[:T], ids[T:]], 1)


def pool_inputs(degrees, H, Dout, seed=0):
    edges = edges_with_degrees(degrees, seed)
    new_t = _f32(_rng(500 + H + seed), (edges.shape[0], 2 * H + Dout))
    return edges, new_t


# =============================================================================================
# embedding
# =============================================================================================
# (n, rows, dim).  n around the 64-index ballot round and the EMB_CAP chunk; (20, 777): three column chunks of 259 (neither a
# multiple of the wave nor of the block); (180, 3136): the factored-conv shape, six chunks of 523 of which the last has 521
EMBEDDING_CASES = [
    (0, 20, 130),
    (1, 1, 1),
    (63, 20, 63),
    (64, 1, 130),
    (65, 180, 63),
    (1024, 180, 1),
    (1024, 20, 777),
    (1025, 20, 777),
    (2500, 1, 63),
    (2500, 180, 3136),
]


def embedding_inputs(n, rows, dim, seed=0):
    """-> (table, idx, g).  The last row is never hit when there is more than one row; beyond one chunk row 0 is hit by the
    first and by the last index, i.e. in the first and in the last chunk"""
    rng = _rng(900 + n + 3 * rows + dim + seed)
    idx = rng.randint(0, max(rows - 1, 1), size=(n,)).astype(np.int64)
    if n > EMB_CAP:
        idx[0] = idx[n - 1] = 0
    return _f32(rng, (rows, dim)), idx, _f32(rng, (n, dim))


def embedding_bwd_ref(idx, g, rows):
    """-> (sequential fp32, float64, bound)"""
    hits = np.bincount(idx, minlength=rows).astype(np.float64)
    seq = scatter_rows(idx, g, rows, np.float32)
    s64 = scatter_rows(idx, g, rows, np.float64)
    mag = scatter_rows(idx, np.abs(g), rows, np.float64)
    return seq, s64, gamma(hits - 1)[:, None] * mag


# =============================================================================================
# gather-linear
# =============================================================================================
# (T, Do, Dp, out_f, act)
GATHER_LINEAR_CASES = [
    (1, 8, 8, 16, 0),
    (33, 163, 128, 64, 1),        # the first layer's 163-dim object rows: 4-byte loads
    (100, 128, 128, 512, 1),      # the 128-dim layers: 16-byte loads, several row tiles
    (70, 12, 4, 33, 2),
    (45, 6, 10, 40, 0),
    (64, 4, 4, 32, 1),
]
GATHER_LINEAR_MISALIGNED = (100, 128, 128, 512, 1)   # run once more with pred 4 bytes off 16-byte alignment
GATHER_LINEAR_O = 20
LEAKY_SLOPE = 0.2
PREACT_MARGIN = 1e-3


def _act64(z, act, slope):
    if act == 1:
        return torch.relu(z)
    if act == 2:
        return torch.where(z > 0, z, z * slope)
    return z


def gather_linear_inputs(T, Do, Dp, out_f, act, with_bias, seed=0):
    """-> dict(obj, pred, edges, w, b, gy) of numpy arrays.  With an activation every pre-activation value (in float64, of the
    fp32 inputs) is at least PREACT_MARGIN away from 0: rows that come too close get a fresh predicate vector."""
    rng = _rng(4000 + T + 5 * Do + 11 * Dp + out_f + (17 if with_bias else 0) + seed)
    O = GATHER_LINEAR_O if T > 1 else 3
    K = 2 * Do + Dp
    obj, pred = _f32(rng, (O, Do)), _f32(rng, (T, Dp))
    edges = rng.randint(0, O, size=(T, 2)).astype(np.int64)
    edges[0, 1] = edges[0, 0]                              # s == o
    w = (_f32(rng, (out_f, K)) * (3.0 / np.sqrt(K))).astype(np.float32)
    b = _f32(rng, (out_f,)) if with_bias else None
    if act != 0:
        for _ in range(200):
            z = gather_linear_preact(obj, pred, edges, w, b)
            bad = np.nonzero((np.abs(z) < 2 * PREACT_MARGIN).any(1))[0]
            if bad.size == 0:
                break
            pred[bad] = _f32(rng, (bad.size, Dp))
        else:
            raise AssertionError('no pre-activation margin for %s' % ((T, Do, Dp, out_f, act),))
    return dict(obj=obj, pred=pred, edges=edges, w=w, b=b, gy=_f32(rng, (T, out_f)), O=O)


def gather_linear_preact(obj, pred, edges, w, b):
    a = np.concatenate([obj[edges[:, 0]], pred, obj[edges[:, 1]]], 1).astype(np.float64)
    z = a @ w.astype(np.float64).T
    return z if b is None else z + b.astype(np.float64)


def gather_linear_ref(inp, act, slope=LEAKY_SLOPE):
    """float64 torch of act([obj[s] | pred | obj[o]] W^T + b), its autograd gradients and the per-element rounding bounds of an
    fp32 evaluation.  -> dict name -> (reference, bound) for y, g_obj, g_pred, gw, gb (gb only with a bias)"""
    slope = float(np.float32(slope))
    obj = t32(inp['obj']).double().requires_grad_()
    pred = t32(inp['pred']).double().requires_grad_()
    w = t32(inp['w']).double().requires_grad_()
    b = None if inp['b'] is None else t32(inp['b']).double().requires_grad_()
    e = t32(inp['edges'])
    gy = t32(inp['gy']).double()
    T, K = e.size(0), w.size(1)
    Do, Dp, out_f, O = obj.size(1), pred.size(1), w.size(0), obj.size(0)
    a = torch.cat([obj[e[:, 0]], pred, obj[e[:, 1]]], 1)
    z = a @ w.t()
    if b is not None:
        z = z + b
    y = _act64(z, act, slope)
    leaves = [obj, pred, w] + ([b] if b is not None else [])
    grads = torch.autograd.grad(y, leaves, gy)
    out = {}
    with torch.no_grad():
        x = 1 if act == 2 else 0                   # the product with the leaky slope is one more rounding
        mag = a.abs() @ w.abs().t()
        if b is not None:
            mag = mag + b.abs()
        dact = torch.ones_like(z) if act == 0 else (z > 0).double() + (z <= 0).double() * (slope if act == 2 else 0.0)
        out['y'] = (y.detach(), gamma(K + 2) * mag * dact)
        g2 = (gy * dact).abs()
        gmag = g2 @ w.abs()                         # [T, K]: sum_n |g2 w|
        deg = torch.bincount(e.reshape(-1), minlength=O).double()
        omag = torch.zeros(O, Do, dtype=torch.float64)
        omag.index_add_(0, e[:, 0], gmag[:, :Do])
        omag.index_add_(0, e[:, 1], gmag[:, Do + Dp:])
        gam_o = torch.from_numpy(gamma(out_f + x + np.maximum(deg.numpy() - 1, 0)))
        out['g_obj'] = (grads[0], gam_o[:, None] * omag)
        out['g_pred'] = (grads[1], gamma(out_f + x) * gmag[:, Do:Do + Dp])
        out['gw'] = (grads[2], gamma(T + x) * (g2.t() @ a.abs()))
        if b is not None:
            out['gb'] = (grads[3], gamma(T - 1 + x) * g2.sum(0))
    return out


# =============================================================================================
# layout
# =============================================================================================
LAYOUT_COUNTS = [13, 0, 25, 12, 1, 0]        # objects per image: two / three register passes, exactly one, one object, empty
#                                              images in the middle and at the end (o_beg == O)
# (H, W, M, D, masks dtype, pooling): every (H, W) with every D; every pair of values of any two fields occurs in some case
LAYOUT_CASES = [
    (16, 16, 16, 7, 'f32', 'sum'),
    (16, 16, 16, 38, 'i64', 'sum'),
    (16, 16, 5, 200, 'f32', 'avg'),
    (22, 30, 16, 7, 'f32', 'avg'),           # W % 4 != 0: the scalar LDS-staged kernel only, three 256-pixel tiles
    (22, 30, 5, 38, 'f32', 'avg'),
    (22, 30, 16, 200, 'i64', 'sum'),
    (9, 7, 5, 7, 'i64', 'avg'),              # W % 4 != 0, less than one tile
    (9, 7, 5, 38, 'f32', 'avg'),
    (9, 7, 16, 200, 'f32', 'sum'),
    (33, 32, 16, 7, 'f32', 'sum'),           # 1056 pixels: two tiles of the vector kernels
    (33, 32, 5, 38, 'f32', 'sum'),
    (33, 32, 5, 200, 'i64', 'avg'),
    (17, 61, 5, 7, 'f32', 'avg'),            # W % 4 != 0, five tiles, the last of 13 pixels
    (17, 61, 16, 38, 'i64', 'avg'),
    (17, 61, 5, 200, 'f32', 'sum'),
]
LAYOUT_DSPLITS = [1, 2, 3, 8]                # option layout_dsplit under layout_reg = 1 (3: a ragged last channel chunk at D = 200)
LAYOUT_MAX_PER_IMAGE = [0, 4, 1000]          # the LDS hint under layout_reg = 0: default 12, seven chunks, all objects at once
LAYOUT_GRAD_FROM = [0, 3]
LAYOUT_TOL = dict(out=1e-5, g_vecs=2e-5, g_masks=2e-5)


def layout_reg_plan(W, D, dsplit):
    """layout.hip: sg_masks_to_layout_fwd under layout_reg = 1 -> None (the LDS-staged kernel) or (channel chunk, grid.z)"""
    if W % 4 != 0 or D * LAYOUT_REG_CAP * 4 > 64 * 1024:
        return None
    dsplit = min(max(dsplit, 1), 8)
    if dsplit > D // 16:
        dsplit = max(D // 16, 1)
    dchunk = (D + dsplit - 1) // dsplit
    return dchunk, (D + dchunk - 1) // dchunk


def layout_lds_cap(W, D, O, max_per_image):
    """layout.hip: objects per chunk of layout_fwd_kernel"""
    vec = 4 if W % 4 == 0 else 1
    cap = max_per_image if max_per_image > 0 else LAYOUT_REG_CAP
    cap = min(cap, O)
    return min(cap, (160 * 1024 - 1024) // ((256 * vec + D) * 4))


def layout_inputs(H, W, M, D, mdtype, seed=0):
    """-> dict(vecs, boxes, masks, obj_to_img, w) for LAYOUT_COUNTS; boxes inside the image, at least a tenth of it wide"""
    rng = _rng(7000 + 31 * H + W + 3 * M + D + seed)
    o2i = np.repeat(np.arange(len(LAYOUT_COUNTS), dtype=np.int64), LAYOUT_COUNTS)
    O = o2i.size
    x0, y0 = rng.rand(O) * 0.6, rng.rand(O) * 0.6
    boxes = np.stack([x0, y0, x0 + 0.1 + 0.3 * rng.rand(O), y0 + 0.1 + 0.3 * rng.rand(O)], 1).astype(np.float32)
    if mdtype == 'i64':
        masks = (rng.rand(O, M, M) > 0.4).astype(np.int64)
    else:
        masks = rng.rand(O, M, M).astype(np.float32)
    return dict(vecs=_f32(rng, (O, D)), boxes=boxes, masks=masks, obj_to_img=o2i,
                w=_f32(rng, (len(LAYOUT_COUNTS), D, H, W)))


def layout_ref(inp, H, W, pooling, dtype=torch.float64):
    """oracle.sg_oracle.masks_to_layout in ``dtype`` over the non-empty images (the oracle refuses empty ones), exact zeros
    inserted for the empty ones.  -> dict(out, g_vecs, g_masks (float masks only)) of loss = sum(out * w)"""
    from oracle import sg_oracle as O
    o2i = inp['obj_to_img']
    N = inp['w'].shape[0]
    present = np.unique(o2i)
    compact = np.searchsorted(present, o2i)
    vecs = t32(inp['vecs']).to(dtype).requires_grad_()
    fm = inp['masks'].dtype != np.int64
    masks = t32(inp['masks']).to(dtype).requires_grad_() if fm else t32(inp['masks'])
    dense = O.masks_to_layout(vecs, t32(inp['boxes']).to(dtype), masks, t32(compact), H, W, pooling=pooling)
    out = torch.zeros((N,) + tuple(dense.shape[1:]), dtype=dtype)
    out[t32(present)] = dense
    (out * t32(inp['w']).to(dtype)).sum().backward()
    return dict(out=out.detach(), g_vecs=vecs.grad, g_masks=masks.grad if fm else None)


# =============================================================================================
# crops
# =============================================================================================
CROP_FEATS = (3, 19, 23)                     # (N, H, W) of feats; image 2 is never cropped
# (C, B, HH, WW): C = 1 the one-channel form, 3 / 5 / 9 a channel tail of the four-channel form; B around the 256-box round
CROP_CASES = [
    (1, 300, 7, 9),
    (3, 257, 1, 5),              # one crop row: the n_crop == 1 early-out of the row range
    (4, 256, 1, 1),
    (5, 300, 7, 9),
    (9, 1, 32, 32),
    (4, 257, 32, 32),
    (5, 0, 7, 9),                # no boxes at all
    (3, 1, 1, 1),
]
CROP_TOL = dict(out=1e-5, g_feats=1e-4)
CROP_BOX_KINDS = ['ordinary', 'full', 'flipped', 'zero_width', 'partly_outside', 'outside']


def crop_inputs(C, B, HH, WW, seed=0):
    """-> dict(feats, boxes, idx, w, kinds).  Box b is of kind CROP_BOX_KINDS[(b + 2) % 6] (a single box is a flipped one); idx is
    unsorted over images 0 and 1"""
    rng = _rng(8000 + 13 * C + B + HH + WW + seed)
    N, H, W = CROP_FEATS
    kinds = [CROP_BOX_KINDS[(b + 2) % 6] for b in range(B)]
    boxes = np.zeros((B, 4), dtype=np.float32)
    for b, k in enumerate(kinds):
        x0, y0 = rng.rand() * 0.5, rng.rand() * 0.5
        x1, y1 = x0 + 0.1 + 0.4 * rng.rand(), y0 + 0.1 + 0.4 * rng.rand()
        if k == 'full':
            x0, y0, x1, y1 = 0.0, 0.0, 1.0, 1.0
        elif k == 'flipped':
            x0, x1 = x1, x0
        elif k == 'zero_width':
            x1 = x0
        elif k == 'partly_outside':
            x0, y1 = -0.1 - 0.4 * rng.rand(), 1.0 + 0.1 + 0.3 * rng.rand()
        elif k == 'outside':
            x0, x1, y0, y1 = x0 + 1.2, x1 + 1.3, y0 - 1.5, y1 - 1.6
        boxes[b] = (x0, y0, x1, y1)
    idx = rng.randint(0, 2, size=(B,)).astype(np.int64)
    if B > 2:
        idx[0], idx[1] = 1, 0
    return dict(feats=_f32(rng, (N, C, H, W)), boxes=boxes, idx=idx, w=_f32(rng, (B, C, HH, WW)), kinds=kinds)


def crop_ref(inp, HH, WW, dtype=torch.float64):
    """oracle.sg_oracle.crop_bbox_batch in ``dtype`` -> dict(out, g_feats) of loss = sum(out * w)"""
    from oracle import sg_oracle as O
    feats = t32(inp['feats']).to(dtype).requires_grad_()
    B = inp['boxes'].shape[0]
    if B == 0:
        return dict(out=torch.zeros((0, feats.size(1), HH, WW), dtype=dtype), g_feats=torch.zeros_like(feats))
    out = O.crop_bbox_batch(feats, t32(inp['boxes']).to(dtype), t32(inp['idx']), HH, WW)
    (out * t32(inp['w']).to(dtype)).sum().backward()
    return dict(out=out.detach(), g_feats=feats.grad)


# =============================================================================================
# factored weights
# =============================================================================================
# (O, C2) at N = 3, M = 2, KS = 1, C = 5, R = 3
FACTORED_DIMS = dict(N=3, M=2, KS=1, C=5, R=3)
FACTORED_CASES = [(4097, 0), (4097, 2), (4096, 0), (4096, 2)]


def factored_inputs(O, C2, seed=0):
    d = FACTORED_DIMS
    rng = _rng(9000 + O + C2 + seed)
    counts = [2000, 1, O - 2001]
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    L = max(counts) + C2
    Ct = d['C'] + d['R'] + C2
    return dict(weight=_f32(rng, (d['M'], Ct, d['KS'], d['KS'])), repr=_f32(rng, (O, d['R'])),
                objs=rng.randint(0, d['C'], size=(O,)).astype(np.int64), seg=seg,
                img_idx=np.repeat(np.arange(3, dtype=np.int64), counts), counts=counts, L=L,
                g=_f32(rng, (d['N'], d['M'], L, d['KS'], d['KS'])))


def factored_ref(inp, C2):
    """float64 restatement of the comment above factored_weights_fwd_kernel: wimg[n][m][j] = W_eff of the j-th object of image n,
    W_eff[o] = W[:, class_o] + sum_d repr[o, d] W[:, C + d]; then the C2 second-source channels; else 0.  Gradients by autograd.
    -> dict name -> (reference, bound) for wimg, gw, grepr"""
    d = FACTORED_DIMS
    N, M, C, R, KS = d['N'], d['M'], d['C'], d['R'], d['KS']
    W = t32(inp['weight']).double().requires_grad_()
    rp = t32(inp['repr']).double().requires_grad_()
    objs, counts, L = t32(inp['objs']), inp['counts'], inp['L']
    g = t32(inp['g']).double()
    O = rp.size(0)

    def build(W, rp):
        weff = W[:, objs] + torch.einsum('od,mdyx->moyx', rp, W[:, C:C + R])            # [M, O, KS, KS]
        wimg = torch.zeros(N, M, L, KS, KS, dtype=W.dtype)
        beg = 0
        for n, c in enumerate(counts):
            wimg[n, :, :c] = weff[:, beg:beg + c]
            if C2:
                wimg[n, :, c:c + C2] = W[:, C + R:]
            beg += c
        return wimg
    wimg = build(W, rp)
    gw, gr = torch.autograd.grad(wimg, [W, rp], g)
    with torch.no_grad():
        Wa, ra, ga = W.abs(), rp.abs(), g.abs()
        wmag = build(Wa, ra)
        # gradient magnitudes: the same sums over absolute values
        slot = torch.cat([ga[n, :, :c] for n, c in enumerate(counts)], 1)                # [M, O, KS, KS]: |g| at every object's slot
        gw_mag = torch.zeros_like(W)
        gw_mag.index_add_(1, objs, slot)
        gw_mag[:, C:C + R] = torch.einsum('od,moyx->mdyx', ra, slot)
        n_cls = torch.bincount(objs, minlength=C).double().numpy()
        gam = np.concatenate([gamma(n_cls - 1), np.full(R, gamma(O)), np.full(C2, gamma(N - 1))])
        if C2:
            gw_mag[:, C + R:] = sum(ga[n, :, c:c + C2] for n, c in enumerate(counts))
        gr_mag = torch.einsum('moyx,mdyx->od', slot, Wa[:, C:C + R])
    return dict(wimg=(wimg.detach(), gamma(R + 1) * wmag),
                gw=(gw, torch.from_numpy(gam).view(1, -1, 1, 1) * gw_mag),
                grepr=(gr, gamma(M * KS * KS) * gr_mag))
