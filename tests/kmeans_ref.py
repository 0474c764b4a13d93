"""numpy float64 restatement of what csrc/kmeans.hip computes for ONE class: assign, empty-cluster relocation, update, one round of
k-means++ and the Lloyd loop with the device's bookkeeping.  Shared by tests/test_kmeans_cpu.py (which pins it to scikit-learn's
Lloyd) and tests/test_gpu_kmeans.py; ``blobs`` / ``segmented`` are the generators both use."""
import numpy as np

EPS = 2.0 ** -23


def dist2(x, c):
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1)


def assign(x, c):
    """-> (labels, mind2): nearest centre, a tie goes to the lowest index (np.argmin)"""
    d = dist2(x, c)
    lab = d.argmin(1)
    return lab, d[np.arange(len(x)), lab]


def relocate(labels, mind2, k):
    """per empty centre (ascending): the row with the largest mind2 (a tie: the lowest row) whose centre has more than one row"""
    labels = labels.copy()
    cnt = np.bincount(labels, minlength=k)
    for e in range(k):
        if cnt[e]:
            continue
        cand = np.where(cnt[labels] > 1)[0]
        if not len(cand):
            break
        i = cand[np.argmax(mind2[cand])]                 # argmax: the first (lowest row) of a tie
        cnt[labels[i]] -= 1
        labels[i], cnt[e] = e, 1
    return labels


def update(x, labels, c_old):
    """-> (centres, counts): mean per label; a centre without rows keeps its value"""
    k = len(c_old)
    cnt = np.bincount(labels, minlength=k)
    c = c_old.copy()
    for j in np.where(cnt > 0)[0]:
        c[j] = x[labels == j].mean(0)
    return c, cnt


def pp_round(x, mind2, u, prev=None, first=False):
    """one round of k-means++ (one trial): -> (pick, mind2).  Round 0 (``prev`` None): row floor(u * n)."""
    if prev is None:
        return min(int(u * len(x)), len(x) - 1), mind2
    d = ((x - x[prev]) ** 2).sum(1)
    mind2 = d if first else np.minimum(mind2, d)
    cum = np.cumsum(mind2)
    return int(np.searchsorted(cum, u * cum[-1], side='right')), mind2


def lloyd(x, init, max_iter=300, tol=0.0, trace=None):
    """-> dict(centers, labels, counts, inertia, n_iter).  A class is finished when an assign changed no label; it is converged when
    the squared centre shift is at most tol * mean per-dimension variance, or when it has one centre: then one more assign gives the
    labels and the inertia of the final centres.  ``events``: centres found empty by an assign.  ``trace``: a list that receives the centres every assign saw."""
    n, k = len(x), len(init)
    c = np.array(init, dtype=np.float64)
    labels = -np.ones(n, dtype=np.int64)
    tolv = tol * x.var(0).mean() if n else 0.0
    finished, n_iter, mind2, events = False, 0, np.zeros(n), 0
    for it in range(max_iter if n else 0):
        if trace is not None:
            trace.append(c.copy())
        new, mind2 = assign(x, c)
        changed = int((new != labels).sum())
        events += int((np.bincount(new, minlength=k) == 0).sum())
        labels = relocate(new, mind2, k)
        c_new, _ = update(x, labels, c)
        shift = ((c_new - c) ** 2).sum()
        c, n_iter = c_new, it + 1
        if changed == 0:
            finished = True
            break
        if k == 1 or shift <= tolv:
            break
    if n and not finished:
        if trace is not None:
            trace.append(c.copy())
        labels, mind2 = assign(x, c)
    return dict(centers=c, labels=labels, counts=np.bincount(labels, minlength=k) if n else np.zeros(k, np.int64),
                inertia=mind2.sum(), n_iter=n_iter, events=events)


# ---- generators --------------------------------------------------------------------------------------------------------------------
def blobs(rs, n, K, D):
    """n rows around K Gaussian blobs: N(0, 4^2) means, unit noise"""
    means = rs.randn(K, D) * 4.0
    return means[rs.randint(0, K, n)] + rs.randn(n, D)


def class_sizes(rs, K, extra=6, hi=400):
    return [0, 1, K - 3, K] + [int(v) for v in rs.randint(K + 1, hi, extra)]


def segmented(rs, sizes, K, D, kind='blobs'):
    """-> (x [P, D] float64, offsets [C + 1])"""
    parts = []
    for n in sizes:
        if kind == 'blobs':
            parts.append(blobs(rs, n, K, D))
        elif kind == 'relu':
            parts.append(np.maximum(rs.randn(n, D) + 0.5, 0.0) * 3.0)
        else:
            parts.append(rs.randn(n, D))
    x = np.concatenate(parts, 0) if parts else np.zeros((0, D))
    return x, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def tie_band(x, c):
    """4 (D + 3) eps (|x|^2 + max_j |c_j|^2) per row: the rounding bound of either form of the fp32 distance, times 4"""
    return 4.0 * (x.shape[1] + 3) * EPS * ((x ** 2).sum(1) + (c ** 2).sum(1).max())
