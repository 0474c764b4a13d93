"""Plain NumPy restatements for the feature-set tests (KID, precision / recall, density / coverage): float64 throughout, int64 where
the data is integer-valued, with the summation bounds the GPU tests hold the kernels to.  The tree only.

Bounds (u = 2^-53; products of float32 values are exact in float64, so only sums, the affine map and the powers round):
* With T = |gamma| sum|a_k b_k| + |coef0| >= |gamma a.b + coef0|: a dot product over D terms is off by at most D u sum|a_k b_k|, so
  t = gamma a.b + coef0 by (D + 2) u T and t^3 by 3 (D + 2) u T^3 plus two roundings of the multiplications -- (3 D + 9) u T^3 with
  room for the second order; summing P such terms adds at most P u sum T^3.  Kernel and oracle both round, hence the factor 2:
  2 u [(3 D + 9) + P] sum T^3.
* d2 = |a|^2 + |b|^2 - 2 a.b: three sums of D terms and two additions, 2 (D + 2) u (|a|^2 + |b|^2 + 2 sum|a_k b_k|) with both sides
  rounding."""
import numpy as np

U = 2.0 ** -53


def relu_gauss(seed, n, d):
    """ReLU-ed Gaussian float32 rows from RandomState(seed)"""
    return np.maximum(np.random.RandomState(seed).randn(n, d), 0.0).astype(np.float32)


# ---- the kernel sums --------------------------------------------------------------------------------------------------------------------
def _poly(g, gamma, coef0, degree):
    t = gamma * g + coef0
    v = t
    for _ in range(degree - 1):
        v = v * t
    return v


def poly_sums_int(x, y, ix, iy, gamma, coef0, degree):
    """integer-valued rows, integer gamma and coef0: (sums [S, 3] int64, the largest sum of |k| of any of them) -- exact"""
    xi, yi = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    assert np.array_equal(xi, np.asarray(x)) and np.array_equal(yi, np.asarray(y)) and int(gamma) == gamma and int(coef0) == coef0
    S, s = ix.shape
    out, mass = np.zeros((S, 3), np.int64), 0
    off = ~np.eye(s, dtype=bool)
    for q in range(S):
        a, b = xi[ix[q]], yi[iy[q]]
        kxx, kyy, kxy = (_poly(g, int(gamma), int(coef0), degree) for g in (a @ a.T, b @ b.T, a @ b.T))
        out[q] = kxx[off].sum(), kyy[off].sum(), kxy.sum()
        mass = max(mass, int(np.abs(kxx).sum()), int(np.abs(kyy).sum()), int(np.abs(kxy).sum()))
    return out, mass


def poly_sums_float(x, y, ix, iy, gamma, coef0, degree=3):
    """float rows: (sums [S, 3] float64, bound [S, 3]) with bound = 2 u [(3 D + 9) + P] sum T^degree"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    S, s = ix.shape
    D = x.shape[1]
    out, bound = np.zeros((S, 3)), np.zeros((S, 3))
    off = ~np.eye(s, dtype=bool)
    for q in range(S):
        a, b = x[ix[q]], y[iy[q]]
        for c, (p, r, mask) in enumerate(((a, a, off), (b, b, off), (a, b, np.ones((s, s), bool)))):
            k = _poly(p @ r.T, gamma, coef0, degree)
            T = abs(gamma) * (np.abs(p) @ np.abs(r).T) + abs(coef0)
            out[q, c] = k[mask].sum()
            bound[q, c] = 2.0 * U * ((3 * D + 9) + mask.sum()) * (T ** degree)[mask].sum()
    return out, bound


def kid_from_sums(sums, s):
    sums = np.asarray(sums, np.float64).reshape(-1, 3)
    per = np.array([row[0] / (s * (s - 1.0)) + row[1] / (s * (s - 1.0)) - 2.0 * row[2] / (s * s) for row in sums])
    return float(np.mean(per)), float(np.sqrt(np.mean((per - np.mean(per)) ** 2)))


def kid_bound(bound, s):
    """per subset: the propagated (Bxx + Byy) / (s (s - 1)) + 2 Bxy / s^2"""
    bound = np.asarray(bound, np.float64).reshape(-1, 3)
    return (bound[:, 0] + bound[:, 1]) / (s * (s - 1.0)) + 2.0 * bound[:, 2] / (s * s)


def draw_subsets(seed, subsets, size, n_real, n_fake):
    rs = np.random.RandomState(seed)
    ix, iy = [], []
    for _ in range(subsets):
        ix.append(rs.permutation(n_real)[:size])
        iy.append(rs.permutation(n_fake)[:size])
    return np.array(ix, np.int32), np.array(iy, np.int32)


# ---- distances --------------------------------------------------------------------------------------------------------------------------
def dist2_int(a, b):
    ai, bi = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    assert np.array_equal(ai, np.asarray(a)) and np.array_equal(bi, np.asarray(b))
    return np.maximum((ai * ai).sum(1)[:, None] + (bi * bi).sum(1)[None, :] - 2 * (ai @ bi.T), 0)


def dist2_float(a, b):
    """(d2 [n, m] float64, bound [n, m])"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = (a * a).sum(1), (b * b).sum(1)
    d = np.maximum(na[:, None] + nb[None, :] - 2.0 * (a @ b.T), 0.0)
    bound = 2.0 * (a.shape[1] + 2) * U * (na[:, None] + nb[None, :] + 2.0 * (np.abs(a) @ np.abs(b).T))
    return d, bound


def knn_radius(d2_self, k):
    """the k-th smallest of each row of a square distance matrix with the diagonal (the row itself, by index) left out"""
    d = np.array(d2_self, dtype=np.float64 if np.issubdtype(np.asarray(d2_self).dtype, np.floating) else np.int64)
    n = d.shape[0]
    rows = np.array([np.sort(np.delete(d[i], i))[k - 1] for i in range(n)])
    return rows


def manifold_counts(d2_ab, r2):
    """d2_ab [n references, m queries], r2 [n] -> (count [m], mind2 [n])"""
    return (d2_ab <= np.asarray(r2)[:, None]).sum(0), d2_ab.min(1)


def prdc(count_fake, count_real, covered, k):
    count_fake, count_real = np.asarray(count_fake), np.asarray(count_real)
    return {'precision': float(np.mean(count_fake > 0)), 'recall': float(np.mean(count_real > 0)),
            'density': float(count_fake.sum() / (float(k) * len(count_fake))), 'coverage': float(np.mean(np.asarray(covered) != 0))}


def metrics(real, fake, k=3, subsets=100, size=1000, seed=0):
    """the whole of ``FeatureSetMetrics.compute()`` on float feature rows -> (dict, dict of what the comparison needs: the KID bound,
    the numbers of membership pairs inside the rounding band per query / reference)"""
    real, fake = np.asarray(real, np.float32), np.asarray(fake, np.float32)
    n, m, D = real.shape[0], fake.shape[0], real.shape[1]
    size = min(size, n, m)
    ix, iy = draw_subsets(seed, subsets, size, n, m)
    sums, bound = poly_sums_float(real, fake, ix, iy, 1.0 / D, 1.0, 3)
    mean, std = kid_from_sums(sums, size)
    drr, brr = dist2_float(real, real)
    dff, bff = dist2_float(fake, fake)
    drf, brf = dist2_float(real, fake)
    r2r, r2f = knn_radius(drr, k), knn_radius(dff, k)
    count_fake, mind2 = manifold_counts(drf, r2r)
    count_real, _ = manifold_counts(drf.T, r2f)
    out = {'kid_mean': mean, 'kid_std': std, 'kid_subset_size': size, 'real': n, 'fake': m}
    out.update(prdc(count_fake, count_real, mind2 <= r2r, k))
    band_p = np.abs(drf - r2r[:, None]) <= 2.0 * (brf + brr.max(1)[:, None])
    band_r = np.abs(drf.T - r2f[:, None]) <= 2.0 * (brf.T + bff.max(1)[:, None])
    return out, {'kid_bound': float(kid_bound(bound, size).max()), 'band_precision': int(band_p.sum()), 'band_recall': int(band_r.sum())}
