"""Float64 NumPy restatement of IS-infinity (scene_generation_amd/isinf.py, csrc/isinf.hip), the synthetic softmax rows its tests use
and the rounding bounds they hold the device to.  No import from the package: the subset sizes, tables and the line are restated too.

The definition (include/sg2im_hip.h).  With p the stored float32 row, s_i its float64 sum and ph_ij = double(p_ij) / s_i:
    h_i = sum_j ph_ij log ph_ij                      a term whose ph is not > 0 is 0: a row of sum 0 contributes nothing
and for a subset of n_q rows t_i:
    q_j = sum_i double(p[t_i][j]),  qh_j = q_j / sum_j q_j,  mh_j = (sum_i ph[t_i][j]) / n_q
    log score = (sum_i h[t_i]) / n_q - sum_j mh_j log qh_j                                  a term whose mh_j is not > 0 is 0

The bounds, to first order in u = 2^-53 (the second-order terms are below 1e-12 of them at these sizes).  Every sum below has terms of
one sign, so ANY order of adding k of them errs by at most (k - 1) u of the sum's magnitude; a division or product adds u, a log or
exp 2 u of its value (a generous figure for both libraries).
    s_i:   (C - 1) u s_i
    ph_ij: relative a = C u (the sum, the division); log ph moves by a, so ph log ph moves by a (|ph log ph| + ph), and sum_j ph = 1:
    h_i:   u ((2 C + 2) |h_i| + C)                    (a (|h_i| + 1), the log and the product 3 u |h_i|, the sum (C - 1) u |h_i|)
    H = sum_i h[t_i]: the h errors and (n_q - 1) u |H|;  H / n_q: one more u
    qh_j:  relative b = (2 n_q + C) u (q_j, then Q over the classes, the division); log qh_j moves by b
    mh_j:  relative c = (C + n_q) u (each ph, the sum over the rows, the division)
    T = sum_j mh_j log qh_j: (c + 3 u) |T| + b sum_j mh_j + (C - 1) u |T| <= u ((2 C + n_q + 2) |T| + 2 n_q + C)       (sum_j mh_j <= 1)
    log score = H / n_q - T, the subtraction one more u of each:
        |error| <= u ((2 C + n_q + 4) (|H| / n_q + |T|) + 2 C + 2 n_q)  =  ``log_score_bound`` / 2
Device and restatement each stay within that of the exact value, so they differ by at most twice it: ``log_score_bound``.  The same
expression bounds the one-split score of sg_inception_score (its KL terms are ph log ph - ph log qh_j: the same magnitudes), which is
what the cross-check of the two kernels uses."""
import numpy as np

U = 2.0 ** -53


# ---- the rows ---------------------------------------------------------------------------------------------------------------------------
def rows(seed, n, C, alpha=0.02):
    """softmax-like rows: a sparse gamma background and one strong class per row; float32 [n, C], each row of sum ~1"""
    rs = np.random.RandomState(seed)
    g = rs.gamma(alpha, size=(n, C))
    k = rs.randint(C, size=n)
    g[np.arange(n), k] += rs.gamma(8.0, size=n)
    return (g / g.sum(1, keepdims=True)).astype(np.float32)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def row_terms(p):
    """(s [n], h [n]) float64, row by row"""
    p = np.asarray(p)
    s, h = np.zeros(p.shape[0]), np.zeros(p.shape[0])
    for i in range(p.shape[0]):
        r = p[i].astype(np.float64)
        s[i] = r.sum()
        with np.errstate(divide='ignore', invalid='ignore'):
            ph = r / s[i]
        ph = ph[ph > 0]
        h[i] = (ph * np.log(ph)).sum()
    return s, h


def subset_parts(p, s, h, t):
    """(H, T, n_q) of the subset whose row numbers are ``t``: log score = H / n_q - T"""
    t = np.asarray(t, np.int64)
    n = float(t.size)
    r = p[t].astype(np.float64)
    q = r.sum(0)
    with np.errstate(divide='ignore', invalid='ignore'):
        ph = r / s[t][:, None]
    mh = np.where(ph > 0, ph, 0.0).sum(0) / n
    qh = q / q.sum()
    keep = mh > 0
    T = (mh[keep] * np.log(qh[keep])).sum()
    return float(h[t].sum()), float(T), int(t.size)


def subset_scores(p, idx, sizes, terms=None):
    """[S, 2] = {log score, score} of the subsets of a table (idx [S, smax], sizes [S]), and the parts (H, T, n_q) of each"""
    s, h = terms if terms is not None else row_terms(p)
    out, parts = np.zeros((len(sizes), 2)), []
    for k, nq in enumerate(np.asarray(sizes).tolist()):
        H, T, n = subset_parts(p, s, h, idx[k, :nq])
        out[k] = (H / n - T, np.exp(H / n - T))
        parts.append((H, T, n))
    return out, parts


def direct_score(p):
    """exp(mean_i KL(ph_i || qh)) the way scripts/inception_score.py computes one split (scipy.stats.entropy normalises both)"""
    p = np.asarray(p, np.float64)
    py = p.mean(0)
    qh = py / py.sum()
    kl = []
    for i in range(p.shape[0]):
        ph = p[i] / p[i].sum()
        keep = ph > 0
        kl.append((ph[keep] * np.log(ph[keep] / qh[keep])).sum())
    return float(np.exp(np.mean(kl)))


# ---- the bounds -------------------------------------------------------------------------------------------------------------------------
def row_bounds(s, h, C):
    """(bound on |s - s_ref|, bound on |h - h_ref|): twice the one-sided figures of the module docstring"""
    return 2.0 * C * U * np.abs(s), 2.0 * U * ((2 * C + 2) * np.abs(h) + C * (np.abs(s) > 0))


def log_score_bound(H, T, nq, C):
    return 2.0 * U * ((2 * C + nq + 4) * (abs(H) / nq + abs(T)) + 2 * C + 2 * nq)


def score_bound(score, H, T, nq, C):
    """the score is exp of the log score: its relative error is the log score's absolute one, and 2 u of each side's exp"""
    return abs(score) * (log_score_bound(H, T, nq, C) + 4.0 * U)


# ---- the host's share, restated ---------------------------------------------------------------------------------------------------------
def sizes_of(n, num_points=15, min_size=None):
    min_size = n // 2 if min_size is None else min_size
    return np.unique(np.linspace(min_size, n, num_points).astype(int))


def tables(seed, sizes, n):
    rs = np.random.RandomState(seed)
    idx = np.zeros((len(sizes), int(max(sizes))), np.int32)
    for q, s in enumerate(np.asarray(sizes).tolist()):
        idx[q, :s] = np.arange(n) if s == n else rs.permutation(n)[:s]
    return idx


def line(sizes, values):
    """(intercept, slope) of the least-squares line in 1 / n, by numpy.polyfit"""
    slope, intercept = np.polyfit(1.0 / np.asarray(sizes, np.float64), np.asarray(values, np.float64), 1)
    return float(intercept), float(slope)


def pipeline(p, num_points=15, min_size=None, seed=0, repeats=1):
    """is_infinity restated: the first draw under ``seed``, repeat r >= 1 of the sizes below n under [seed, r]; the per-size means"""
    n = p.shape[0]
    sizes = sizes_of(n, num_points, min_size)
    terms = row_terms(p)
    acc = np.zeros((len(sizes), 2))
    cnt = np.zeros(len(sizes))
    for r in range(repeats):
        sub = sizes if r == 0 else sizes[sizes < n]
        where = np.arange(len(sizes)) if r == 0 else np.flatnonzero(sizes < n)
        if not len(sub):
            continue
        out, _ = subset_scores(p, tables(seed if r == 0 else [seed, r], sub, n), sub, terms)
        acc[where] += out
        cnt[where] += 1
    logs, scores = acc[:, 0] / cnt, acc[:, 1] / cnt
    return {'sizes': sizes, 'scores': scores, 'logs': logs, 'is': float(scores[-1]), 'is_inf': line(sizes, scores)[0],
            'slope': line(sizes, scores)[1], 'is_inf_log': float(np.exp(line(sizes, logs)[0]))}


def large_sample_score(total, C, chunk=4096, seed0=1000):
    """the score of ``total`` rows of the generator (chunk k under seed0 + k), accumulated chunk by chunk: sum h, q and m"""
    H, q, m, n = 0.0, np.zeros(C), np.zeros(C), 0
    k = 0
    while n < total:
        p = rows(seed0 + k, min(chunk, total - n), C).astype(np.float64)
        s = p.sum(1, keepdims=True)
        ph = p / s
        with np.errstate(divide='ignore', invalid='ignore'):
            H += np.where(ph > 0, ph * np.log(ph), 0.0).sum()
        q += p.sum(0)
        m += ph.sum(0)
        n += p.shape[0]
        k += 1
    mh, qh = m / n, q / q.sum()
    keep = mh > 0
    return float(np.exp(H / n - (mh[keep] * np.log(qh[keep])).sum()))
