"""Plain float64 NumPy restatements for the FID-infinity tests, written from the formulas:

* the D x D symmetric form of the Frechet distance, per subset (mean and numpy.cov of the gathered rows);
* the Gram form of the same number: P = Z Z^T, G = Z Sigma_r Z^T over ALL rows once, then sums and the doubly centred block per subset;
* the subset sizes, the subset tables and the least-squares line in 1 / n;
* the synthetic Gaussian populations whose true distance is known in closed form;
* the summation bounds the GPU tests hold the kernels to.
What is independent of the code under test is the D x D form (its own square root, its own product, no n x n matrix anywhere): every
Frechet distance the tests assert is in the end compared with it.  The Gram half restates what the kernels compute (P, G, the sums,
the centred blocks) in NumPy; its last step, ``fid_from_gram`` with the eigenvalue cut ``_cut``, is necessarily the expression of
``fidinf.fid_from_terms`` and ``fid._truncate`` -- there is one way to write it -- and is checked by the D x D form, not by itself.
The tree only."""
import numpy as np
import torch

U = 2.0 ** -53


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of a sum of k rounded terms"""
    return k * U / (1.0 - k * U)


# ---- data ------------------------------------------------------------------------------------------------------------------------------
def population(seed, D, shift=0.05, lo=0.7, hi=1.3):
    """(mean [D], covariance [D, D], factor A with covariance = A A^T) of a Gaussian: a mean near 0.4, standard deviations from ``hi``
    down to ``lo`` along the columns of a random orthogonal matrix"""
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.randn(D, D))
    A = Q * np.linspace(hi, lo, D)[None, :]
    return 0.4 + shift * rs.randn(D), A @ A.T, A


def moved(pop, seed, shift=0.5, scale=1.1):
    """the population a generator that is slightly off would have: the mean moved by ``shift`` in all (a vector of that length, about),
    every standard deviation times ``scale``"""
    mean, cov, A = pop
    rs = np.random.RandomState(seed)
    return mean + shift * rs.randn(mean.size) / np.sqrt(mean.size), cov * scale * scale, A * scale


def draw(seed, pop, n):
    """n float32-rounded rows of the population (as float32)"""
    mean, _, A = pop
    rs = np.random.RandomState(seed)
    return (mean + rs.randn(n, mean.size) @ A.T).astype(np.float32)


def pooled_like(seed, n, D):
    """non-negative float32 rows with a mean near 0.4 and correlated columns, like pooled features"""
    rs = np.random.RandomState(seed)
    base = 0.4 + 0.3 * rs.randn(n, D) * (0.5 + rs.rand(D)) + 0.2 * rs.randn(n, 1)
    return np.abs(base).astype(np.float32)


def stats(rows):
    rows = np.asarray(rows, np.float64)
    return rows.mean(0), np.atleast_2d(np.cov(rows, rowvar=False))


# ---- the D x D symmetric form --------------------------------------------------------------------------------------------------------
def _cut(lam):
    top = lam.max() if lam.size else 0.0
    return np.where(lam > lam.size * 2.0 ** -52 * top, lam, 0.0)


def frechet_sym(mu1, s1, mu2, s2):
    """|mu1 - mu2|^2 + tr s1 + tr s2 - 2 tr (s1 s2)^1/2 with the trace term as the sum of the square roots of the eigenvalues of
    R s2 R, R = s1^1/2 from eigh: right for rank-deficient covariances"""
    lam, V = np.linalg.eigh(s1)
    R = (V * np.sqrt(_cut(lam))) @ V.T
    M = R @ s2 @ R
    root = np.sqrt(_cut(np.linalg.eigvalsh(0.5 * (M + M.T)))).sum()
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * root)


def subset_fids_dxd(rows, mu, sigma, idx, sizes):
    """the FID of each subset to (mu, sigma) by the D x D route: statistics of the gathered rows, then ``frechet_sym``"""
    rows = np.asarray(rows, np.float64)
    out = []
    for q, s in enumerate(sizes):
        m, c = stats(rows[idx[q, :s]])
        out.append(frechet_sym(mu, sigma, m, c))
    return np.array(out)


# ---- the Gram form -------------------------------------------------------------------------------------------------------------------
def grams(rows, mu, sigma):
    """(Z, P, G): Z = double(rows) - mu, P = Z Z^T, G = (Z sigma) Z^T"""
    Z = np.asarray(rows, np.float64) - np.asarray(mu, np.float64)[None, :]
    return Z, Z @ Z.T, (Z @ sigma) @ Z.T


def gram_bounds(Z, sigma):
    """entrywise |P - P_ref| <= 2 gamma_{D+2} |Z||Z|^T and |G - G_ref| <= 2 gamma_{2D+4} |Z||sigma||Z|^T: each side (the kernel, this
    file) is a sum of D (P) or a sum of D sums of D (G) rounded terms in its own order"""
    D = Z.shape[1]
    a = np.abs(Z)
    return 2.0 * gamma(D + 2) * (a @ a.T), 2.0 * gamma(2 * D + 4) * ((a @ np.abs(sigma)) @ a.T)


def subset_terms(P, G, idx, sizes):
    """per subset: (sum_i P_ii, sum_ij P_ij) and M = (G_SS - (r_i + r_j) / n + t / n^2) / (n - 1), r the row sums of G_SS, t their sum"""
    sums, Ms = [], []
    for q, s in enumerate(sizes):
        t = idx[q, :s]
        Pq, Gq = P[np.ix_(t, t)], G[np.ix_(t, t)]
        r = Gq.sum(1)
        n = float(s)
        sums.append((np.trace(Pq), Pq.sum()))
        Ms.append((Gq - (r[:, None] + r[None, :]) / n + r.sum() / (n * n)) / (n - 1.0))
    return np.array(sums), Ms


def subset_terms_bounds(P, G, bP, bG, idx, sizes):
    """what the terms may differ by when P and G themselves are within (bP, bG) of this file's and every sum of n terms is rounded in
    some order: sums within the gathered bP plus gamma_{n+1} of the absolute sum (n^2 terms for the second: gamma_{n^2+1}); an entry
    of M is G_ij and three more terms of the size of the absolute row sums over n -- their input errors add up, each row sum adds
    gamma_{n+1} sum|G|, the total gamma_{n^2+1} sum|G|, and the four operations (two subtractions, an addition, a division) and two
    quotients another 6 u of the largest intermediate"""
    sb, Mb = [], []
    for q, s in enumerate(sizes):
        t = idx[q, :s]
        n = float(s)
        aP, eP = np.abs(P[np.ix_(t, t)]), bP[np.ix_(t, t)]
        aG, eG = np.abs(G[np.ix_(t, t)]), bG[np.ix_(t, t)]
        sb.append((np.trace(eP) + 2.0 * gamma(s + 1) * np.trace(aP), eP.sum() + 2.0 * gamma(s * s + 1) * aP.sum()))
        r_abs, r_err = aG.sum(1), eG.sum(1) + 2.0 * gamma(s + 1) * aG.sum(1)
        t_abs, t_err = aG.sum(), eG.sum() + 2.0 * gamma(s * s + 1) * aG.sum()
        size = aG + (r_abs[:, None] + r_abs[None, :]) / n + t_abs / (n * n)
        err = eG + (r_err[:, None] + r_err[None, :]) / n + t_err / (n * n) + 12.0 * U * size
        Mb.append(err / (n - 1.0))
    return np.array(sb), Mb


def fid_from_gram(sums_q, M_q, n_q, trace_r):
    n = float(n_q)
    lam = _cut(np.linalg.eigvalsh(M_q))
    return float(sums_q[1] / (n * n) + trace_r + (sums_q[0] - sums_q[1] / n) / (n - 1.0) - 2.0 * np.sqrt(lam).sum())


def subset_fids_gram(rows, mu, sigma, idx, sizes):
    _, P, G = grams(rows, mu, sigma)
    sums, Ms = subset_terms(P, G, idx, sizes)
    tr = float(np.trace(sigma))
    return np.array([fid_from_gram(sums[q], Ms[q], s, tr) for q, s in enumerate(sizes)])


# ---- sizes, tables, the line ---------------------------------------------------------------------------------------------------------
def sizes_of(n, points=15, lo=None):
    lo = n // 2 if lo is None else lo
    out = []
    for v in np.linspace(lo, n, points).astype(int).tolist():
        if v not in out:
            out.append(v)
    return np.array(out, np.int32)


def tables(seed, sizes, n):
    rs = np.random.RandomState(seed)
    idx = np.zeros((len(sizes), int(max(sizes))), np.int32)
    for q, s in enumerate(sizes):
        s = int(s)
        idx[q, :s] = np.arange(n) if s == n else rs.permutation(n)[:s]
    return idx


def line(sizes, fids):
    """(intercept, slope) of the least-squares fit fid ~ intercept + slope / n"""
    A = np.stack([np.ones(len(sizes)), 1.0 / np.asarray(sizes, np.float64)], 1)
    (c, m), *_ = np.linalg.lstsq(A, np.asarray(fids, np.float64), rcond=None)
    return float(c), float(m)


def pipeline_gram(rows, mu, sigma, points=15, lo=None, seed=0):
    """the whole estimate by the Gram form: {'sizes', 'fids', 'fid_inf', 'slope', 'fid'}"""
    n = rows.shape[0]
    sizes = sizes_of(n, points, lo)
    idx = tables(seed, sizes, n)
    fids = subset_fids_gram(rows, mu, sigma, idx, sizes)
    c, m = line(sizes, fids)
    return {'sizes': sizes, 'idx': idx, 'fids': fids, 'fid_inf': c, 'slope': m, 'fid': float(fids[-1])}


def case(D, N, n_real, seed=0):
    """one evaluation: ``n_real`` real rows of a population, ``N`` fake rows of the moved one -> {'fake' float32 [N, D], 'mu', 'sigma'
    (the SAMPLE real statistics), 'truth': the closed-form distance of the fake POPULATION to those statistics}"""
    preal = population(10 + seed, D)
    pfake = moved(preal, 50 + seed)
    mu, sigma = stats(draw(30 + seed, preal, n_real))
    return {'fake': draw(40 + seed, pfake, N), 'mu': mu, 'sigma': sigma, 'truth': frechet_sym(mu, sigma, pfake[0], pfake[1])}


# The two float64 formulations of this file (D x D symmetric form, Gram form) disagree by at most 1.95e-14 relative on the
# 30 subsets of tests/test_fidinf_cpu.py (profiles/fidinf_test_margins.md); the forms under test are held to 8 x that.
REL = 8 * 1.95e-14


class _Net(torch.nn.Module):
    """stands in for an InceptionV3 where only ``fc.in_features`` is read"""

    def __init__(self, dim=8):
        super().__init__()
        self.fc = torch.nn.Linear(dim, 2)
