"""Shared case builder of tests/test_attributes_cpu.py and tests/test_gpu_attributes.py: a few small collated batches (numpy) that
between them reach every branch of the attribute draw (tests/attributes_ref.py counts them), and the image permutation of a
batch.  Per case about ten images and at most ~150 objects: images with 0, 1, 2, 3, 8, 33 and 70 real objects (below, past half of
and past one wavefront), all six predicates, __in_image__ triples before and after the spatial ones, self pairs, ids outside the
image, out-of-range predicates, rows with given bits, a class that was never seen, a class whose histogram is zero on a whole
column and row, a class outside the table, and uniforms of exactly 0 and 1 - 2^-24."""
import numpy as np

SHAPES = ((10, 5), (10, 4), (64, 8), (3, 1))          # (size_len, grid)
REAL_COUNTS = (3, 0, 70, 1, 8, 2, 33, 5, 4, 2)         # real objects per image
NUM_CLASSES = 8                                        # 0 __image__, 1 never seen, 2 zero on column 0 and row 0, 3..7 random
U_MAX = np.float32(1.0 - 2.0 ** -24)
_CACHE = {}


def make_counts(S, g, rs):
    counts = rs.randint(0, 50, size=(NUM_CLASSES, S + g * g)).astype(np.int64)
    counts[rs.rand(*counts.shape) < 0.3] = 0
    counts[0] = 0
    counts[1] = 0
    cells = counts[2, S:].reshape(g, g)
    cells[0, :] = 0
    cells[:, 0] = 0
    counts[3, S:] = 1 + rs.randint(0, 9, size=g * g)   # a class seen everywhere
    counts[4, 0] = 3 << 40                             # weights past 2^32: the prefix sums are 64-bit
    return counts


def make_case(S, g, seed=0):
    """-> dict(objs, obj_to_img, triples, triple_to_img, counts, u, given, N, S, g, C) of numpy arrays"""
    key = (S, g, seed)
    if key in _CACHE:
        return _CACHE[key]
    rs = np.random.RandomState(1000 * seed + 10 * S + g)
    A = S + g * g
    objs, o2i, triples, t2i = [], [], [], []
    base = 0
    total = sum(REAL_COUNTS) + len(REAL_COUNTS)
    for n, k in enumerate(REAL_COUNTS):
        cls = rs.choice(np.arange(1, NUM_CLASSES), size=k, p=[0.2, 0.3, 0.1, 0.1, 0.1, 0.1, 0.1])
        if k >= 8:
            cls[3] = NUM_CLASSES + 2                   # a class outside the table
        objs.extend(cls.tolist() + [0])
        o2i.extend([n] * (k + 1))
        in_image = [[base + i, 0, base + k] for i in range(k)]
        tri = []
        if n % 2 == 0:                                 # __in_image__ triples first, like a person's JSON would not have them
            tri += in_image
        if k >= 2:
            for _ in range(k + k // 2 + 2):
                s = int(rs.randint(0, k))
                o = int(rs.randint(0, k - 1))
                o += o >= s
                p = int(rs.choice([1, 2, 3, 4, 5, 6], p=[0.15, 0.15, 0.15, 0.15, 0.2, 0.2]))
                tri.append([base + s, p, base + o])
        if k >= 1:
            tri.append([base, int(rs.randint(1, 7)), base])                    # a self pair
            tri.append([base, 7, base + k - 1])                                # predicates outside 1..6
            tri.append([base + k - 1, -1, base])
            tri.append([base, int(rs.randint(1, 7)), base + k])                # the __image__ object as an end
            tri.append([base + k, int(rs.randint(1, 7)), base + k - 1])
            tri.append([base, 1, (base + k + 1) % total])                      # ids outside the image
            tri.append([-5, 2, base])
            tri.append([base, 3, total + 10])
        if n % 2 == 1:
            tri += in_image
        triples.extend(tri)
        t2i.extend([n] * len(tri))
        base += k + 1
    O = len(objs)
    objs = np.asarray(objs, dtype=np.int64)
    u = np.minimum(rs.random_sample((O, 2)).astype(np.float32), U_MAX)
    u[rs.randint(0, O, size=6), rs.randint(0, 2, size=6)] = 0.0
    u[rs.randint(0, O, size=6), rs.randint(0, 2, size=6)] = U_MAX
    given = np.zeros((O, A), dtype=np.float32)
    for o in range(O):
        if rs.rand() < 0.2:
            given[o, rs.randint(0, S)] = 1.0
        if rs.rand() < 0.2:
            given[o, S + rs.randint(0, g * g)] = 1.0
        if rs.rand() < 0.03:                           # a second bit and a value below the threshold: the first set bit counts
            given[o, S - 1] = 1.0
            given[o, 0] = max(given[o, 0], 0.5)
    case = dict(objs=objs, obj_to_img=np.asarray(o2i, dtype=np.int64), triples=np.asarray(triples, dtype=np.int64).reshape(-1, 3),
                triple_to_img=np.asarray(t2i, dtype=np.int64), counts=make_counts(S, g, rs), u=u, given=given,
                N=len(REAL_COUNTS), S=S, g=g, C=NUM_CLASSES)
    _CACHE[key] = case
    return case


def all_cases():
    return [make_case(S, g) for S, g in SHAPES]


def permute_case(case, perm):
    """the same images in the order ``perm`` (new image j is old image perm[j]) -> (case, old object index of every new object)"""
    o2i, t2i = case['obj_to_img'], case['triple_to_img']
    O = case['objs'].size
    order = np.concatenate([np.nonzero(o2i == n)[0] for n in perm])
    new_id = np.full(O, -1, dtype=np.int64)
    new_id[order] = np.arange(O)
    torder = np.concatenate([np.nonzero(t2i == n)[0] for n in perm])
    tri = case['triples'][torder].copy()
    for col in (0, 2):                                 # ids outside [0, O) stay what they are: outside
        ok = (tri[:, col] >= 0) & (tri[:, col] < O)
        tri[ok, col] = new_id[tri[ok, col]]
    inv = np.empty(len(perm), dtype=np.int64)
    inv[np.asarray(perm)] = np.arange(len(perm))
    out = dict(case, objs=case['objs'][order], obj_to_img=inv[o2i[order]], triples=tri, triple_to_img=inv[t2i[torder]],
               u=case['u'][order], given=case['given'][order])
    return out, order
