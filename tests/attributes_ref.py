"""Plain-numpy restatement of the attribute statistics and the attribute draw (include/sg2im_hip.h: sg_attribute_histogram,
sg_sample_attributes), shared by tests/test_attributes_cpu.py and tests/test_gpu_attributes.py.  Host
arithmetic only, written from the rules, one Python loop per rule.  ``sample`` also returns branch counters (which rule fired how
often) and the list of location draws with the allowed set each one used, so the tests can show that a case set reaches every
branch."""
import numpy as np

OPPOSITE = {1: 2, 2: 1, 3: 4, 4: 3, 5: 6, 6: 5}
U_MAX = np.float32(1.0 - 2.0 ** -24)
COUNTERS = ('mask_left', 'mask_right', 'mask_above', 'mask_below', 'copy_inside', 'copy_surrounding',
            'size_adjusted_reference', 'size_kept_reference', 'size_adjusted_geometric', 'size_kept_geometric',
            'zero_mass_fallback', 'never_seen_class', 'given_size_kept', 'given_loc_kept', 'step5_fill',
            'images_0', 'images_1', 'images_2plus', 'skip_pred', 'skip_self', 'skip_image_obj', 'skip_outside')


def first_bit(block):
    """index of the first element > 0.5f, or -1"""
    hit = np.nonzero(np.asarray(block, dtype=np.float32) > np.float32(0.5))[0]
    return int(hit[0]) if hit.size else -1


def histogram(objs, attrs, C, S, g, image_class=0, counts=None):
    counts = np.zeros((C, S + g * g), dtype=np.int64) if counts is None else counts
    for c, row in zip(np.asarray(objs).tolist(), np.asarray(attrs, dtype=np.float32)):
        if c < 0 or c >= C or c == image_class:
            continue
        si, li = first_bit(row[:S]), first_bit(row[S:])
        if si >= 0:
            counts[c, si] += 1
        if li >= 0:
            counts[c, S + li] += 1
    return counts


def allowed(q, cell, g):
    """the cells a subject of predicate q (1 left of, 2 right of, 3 above, 4 below) may take when its partner sits in ``cell``"""
    col_b, row_b = cell % g, cell // g
    out = np.zeros(g * g, dtype=bool)
    for c in range(g * g):
        col, row = c % g, c // g
        if q == 1:
            out[c] = col <= max(col_b - 1, 0)
        elif q == 2:
            out[c] = col >= min(col_b + 1, g - 1)
        elif q == 3:
            out[c] = row <= max(row_b - 1, 0)
        elif q == 4:
            out[c] = row >= min(row_b + 1, g - 1)
        else:
            raise ValueError(q)
    return out


def draw(hist, allow, u, counters=None):
    """hist: int64 weights of the class, or None for a class outside the table"""
    n = allow.size
    hist = np.zeros(n, dtype=np.int64) if hist is None else np.asarray(hist, dtype=np.int64)
    w = [int(hist[c]) * int(allow[c]) for c in range(n)]
    total = sum(w)
    if total == 0:
        if counters is not None:
            counters['zero_mass_fallback'] += 1
            if not hist.any():
                counters['never_seen_class'] += 1
        w = [int(allow[c]) for c in range(n)]
        total = sum(w)
    u = np.float32(u)
    u = np.float32(0) if not u >= 0 else min(u, U_MAX)
    t = float(u) * float(total)                 # both conversions exact or round-to-nearest, as in C
    run = 0
    for c in range(n):
        run += w[c]
        if float(run) > t:
            return c
    return n - 1


def sample(objs, obj_to_img, triples, triple_to_img, counts, u, given, N, S, g, image_class=0, size_rule='reference', max_objs=1024):
    """-> (size_idx [O] int32, loc_idx [O] int32, attrs [O, S + g*g] fp32, counters, draws); draws: (object, allowed mask, cell) of
    every location draw"""
    objs, obj_to_img = np.asarray(objs, dtype=np.int64), np.asarray(obj_to_img, dtype=np.int64)
    triples = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    triple_to_img = np.asarray(triple_to_img, dtype=np.int64)
    counts, u = np.asarray(counts, dtype=np.int64), np.asarray(u, dtype=np.float32)
    O, G, C = objs.size, g * g, counts.shape[0]
    A = S + G
    size, loc = np.full(O, -1, dtype=np.int32), np.full(O, -1, dtype=np.int32)
    size_given = np.zeros(O, dtype=bool)
    k = dict.fromkeys(COUNTERS, 0)
    draws = []
    everything = np.ones(G, dtype=bool)

    def hist_of(o, block):
        c = int(objs[o])
        if c < 0 or c >= C:
            return None
        return counts[c, :S] if block == 'size' else counts[c, S:]

    def draw_loc(o, allow):
        cell = draw(hist_of(o, 'loc'), allow, u[o, 1], k)
        draws.append((o, allow.copy(), cell))
        return cell

    def step(a, q, b):
        if loc[a] >= 0:
            return
        if loc[b] < 0:
            loc[a] = draw_loc(a, everything)
            return
        if q in (5, 6):
            loc[a] = loc[b]
            k['copy_inside' if q == 5 else 'copy_surrounding'] += 1
            if size_given[a]:
                return
            za, zb, new = int(size[a]), int(size[b]), None
            if size_rule == 'reference':
                if q == 6 and zb <= za:
                    new = max(0, zb - 1)
                if q == 5 and zb >= za:
                    new = min(S - 1, zb + 1)
            elif size_rule == 'geometric':
                if q == 6 and za <= zb:
                    new = min(S - 1, zb + 1)
                if q == 5 and za >= zb:
                    new = max(0, zb - 1)
            else:
                raise ValueError(size_rule)
            k['size_%s_%s' % ('kept' if new is None else 'adjusted', size_rule)] += 1
            if new is not None:
                size[a] = new
            return
        k[('mask_left', 'mask_right', 'mask_above', 'mask_below')[q - 1]] += 1
        loc[a] = draw_loc(a, allowed(q, int(loc[b]), g))

    cc = int(np.rint(0.5 * (g - 1)))            # ties to even
    for n in range(N):
        members = np.nonzero(obj_to_img == n)[0]
        if members.size == 0:
            continue
        ob = int(members[0])
        members = members[:max_objs]
        inside = set(members.tolist())
        real = [o for o in members.tolist() if objs[o] != image_class]
        k['images_0' if len(real) == 0 else ('images_1' if len(real) == 1 else 'images_2plus')] += 1
        for o in members.tolist():
            gs = first_bit(given[o, :S]) if given is not None else -1
            gl = first_bit(given[o, S:]) if given is not None else -1
            is_real = objs[o] != image_class
            if gs >= 0:
                size[o], size_given[o] = gs, True
                k['given_size_kept'] += 1
            elif is_real:
                size[o] = draw(hist_of(o, 'size'), np.ones(S, dtype=bool), u[o, 0], k)
            else:
                size[o] = S - 1
            if gl >= 0:
                loc[o] = gl
                k['given_loc_kept'] += 1
            elif not is_real:
                loc[o] = cc + g * cc
        for t in np.nonzero(triple_to_img == n)[0].tolist():
            s, p, o = [int(v) for v in triples[t]]
            if p < 1 or p > 6:
                k['skip_pred'] += 1
            elif s == o:
                k['skip_self'] += 1
            elif s not in inside or o not in inside:
                k['skip_outside'] += 1
            elif objs[s] == image_class or objs[o] == image_class:
                k['skip_image_obj'] += 1
            else:
                step(s, p, o)
                step(o, OPPOSITE[p], s)
        for o in real:
            if loc[o] < 0:
                loc[o] = draw_loc(o, everything)
                k['step5_fill'] += 1
    attrs = np.zeros((O, A), dtype=np.float32)
    for o in range(O):
        if size[o] >= 0:
            attrs[o, size[o]] = 1
        if loc[o] >= 0:
            attrs[o, S + loc[o]] = 1
    return size, loc, attrs, k, draws
