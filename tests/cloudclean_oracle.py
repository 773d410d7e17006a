"""The arithmetic of csrc/svs_cloudknn.hip restated in float64 numpy (include/svolsdf_hip.h section f4c): brute-force k
nearest neighbours in the (d2, index) order, the two-pass statistics of the outlier scores, and the PCA normals with
np.linalg.eigh.  Also the small synthetic clouds the tests of svs_hip.cloudclean share."""
import numpy as np


# ---- neighbours ----------------------------------------------------------------------------------------------------------
def knn(ref, query, k, max_radius=np.inf, exclude_same_index=False, first_row=0):
    """-> (dist (nq,k) float64 ascending, idx (nq,k) int32, mean (nq,) float64).  d2 = ex*ex + ey*ey + ez*ez with e = ref -
    query, every product and sum rounded on its own (numpy does not contract); order (d2, index); dist = sqrt(d2); a slot
    whose neighbour is not strictly closer than max_radius, or that does not exist, holds inf / -1.  exclude_same_index:
    reference first_row + j is skipped for query j.  mean: the finite slots summed in ascending slot order over their
    number, inf without any."""
    ref, query = np.asarray(ref, np.float64).reshape(-1, 3), np.asarray(query, np.float64).reshape(-1, 3)
    nr, nq = len(ref), len(query)
    dist = np.full((nq, k), np.inf)
    idx = np.full((nq, k), -1, np.int32)
    index = np.arange(nr)
    for j in range(nq):
        ex, ey, ez = ref[:, 0] - query[j, 0], ref[:, 1] - query[j, 1], ref[:, 2] - query[j, 2]
        d2 = ex * ex + ey * ey + ez * ez
        order = np.lexsort((index, d2))
        if exclude_same_index:
            order = order[order != first_row + j]
        order = order[:k]
        d = np.sqrt(d2[order])
        ok = d < max_radius
        m = int(ok.sum())
        assert ok[:m].all()                                  # sqrt is monotone: the finite slots are a prefix
        dist[j, :m], idx[j, :m] = d[:m], order[:m]
    return dist, idx, row_means(dist)


def row_means(dist):
    """the finite slots of every row summed left to right (np.cumsum is sequential) over their number; inf for none"""
    finite = np.isfinite(dist)
    count = finite.sum(1)
    total = np.cumsum(np.where(finite, dist, 0.0), 1)[:, -1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(count > 0, total / count, np.inf)


# ---- outliers ------------------------------------------------------------------------------------------------------------
def outlier_stats(mean):
    """(count, mean, sample std) of the finite entries: two passes, the deviations about the mean, denominator count - 1"""
    v = np.asarray(mean, np.float64)
    v = v[np.isfinite(v)]
    c = len(v)
    m = float(v.sum() / c) if c else 0.0
    s = float(np.sqrt(((v - m) ** 2).sum() / (c - 1))) if c >= 2 else 0.0
    return c, m, s


def outlier_mask(mean, threshold):
    mean = np.asarray(mean, np.float64)
    return np.isfinite(mean) & (mean <= threshold)


def clean_scores(pts, k, max_radius, std_ratio):
    """the whole outlier rule -> (keep, scores, dict(count, mean, std, threshold))"""
    _, _, scores = knn(pts, pts, k, max_radius, exclude_same_index=True)
    c, m, s = outlier_stats(scores)
    thr = m + std_ratio * s
    return outlier_mask(scores, thr), scores, dict(count=c, mean=m, std=s, threshold=thr)


# ---- normals -------------------------------------------------------------------------------------------------------------
def normals(pts, idx, include_self=True, view_index=None, centres=None):
    """-> (normals (n,3) float64 unit, curvature (n,), eigenvalues (n,3) ascending, facing (n,) = n . (c - p) / |c - p| BEFORE
    the flip, nan without centres).  The covariance of the neighbours 0 <= idx[i] < n (and the point) about their centroid,
    np.linalg.eigh; the normal is negated when n . (c - p) < 0, c = centres[view_index[i]] (clamped to [0, n_views)) or the
    nearest centre (lowest index on a tie).  Fewer than three points: zeros.
    A covariance that is diagonal as summed is not rotated by the kernel's Jacobi: the normal is then the POSITIVE axis of
    its smallest diagonal entry, the lowest axis among equal ones (include/svolsdf_hip.h, f4c) -- eigh's choice inside an
    eigenspace of equal eigenvalues is LAPACK's, not the contract's."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    out, curv, lam, facing = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 3)), np.full(n, np.nan)
    for i in range(n):
        sel = [j for j in idx[i] if 0 <= j < n]
        S = pts[([i] if include_self else []) + sel]
        if len(S) < 3:
            continue
        d = S - S.mean(0)
        cov = d.T @ d / len(S)
        if not (cov - np.diag(np.diag(cov))).any():
            w, nrm = np.sort(np.diag(cov)), np.eye(3)[int(np.argmin(np.diag(cov)))]
        else:
            w, v = np.linalg.eigh(cov)
            nrm = v[:, 0] / np.linalg.norm(v[:, 0])
        lam[i] = w
        curv[i] = max(w[0], 0.0) / w.sum() if w.sum() > 0 else 0.0
        if centres is not None:
            C = np.asarray(centres, np.float64).reshape(-1, 3)
            if view_index is not None:
                c = C[min(max(int(view_index[i]), 0), len(C) - 1)]
            else:
                e = C - pts[i]
                c = C[int(np.argmin(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]))]
            to_c = c - pts[i]
            facing[i] = float(nrm @ to_c) / max(float(np.linalg.norm(to_c)), 1e-300)
            if nrm @ to_c < 0:
                nrm = -nrm
        out[i] = nrm
    return out, curv, lam, facing


def angle(a, b, signed=False):
    """the angle between the rows of a and b (radians), up to sign unless `signed`; atan2 of cross and dot: accurate near 0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    cr = np.linalg.norm(np.cross(a, b), axis=1)
    dt = (a * b).sum(1)
    return np.arctan2(cr, dt if signed else np.abs(dt))


# ---- the clouds of the tests ------------------------------------------------------------------------------------------------
def random_cloud(n, seed, scale=1.0):
    return np.random.default_rng(seed).uniform(-scale, scale, (n, 3))


def lattice_cloud(side=6, copies=60, seed=0):
    """the integer lattice [0, side)^3 with `copies` of its points repeated, shuffled: equal distances everywhere, so the
    index rule decides"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([g, g[rng.integers(0, len(g), copies)]])
    return pts[rng.permutation(len(pts))]


def noisy_sphere(n=2000, seed=0, radius=1.0, noise=0.002):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (radius + noise * rng.normal(size=(n, 1)))


def noisy_plane(n=2000, seed=0, noise=0.002):
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-1, 1, (n, 2)), noise * rng.normal(size=(n, 1))], 1)
    # tilted, so that no axis is special
    a, b = 0.6, -0.4
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    return p @ (Rx @ Ry).T


def surface_with_floaters(n=1500, n_far=12, seed=0):
    """a noisy sphere of radius 1 and n_far planted points on the shell of radius 3, far from the surface and from each
    other's neighbourhoods -> (pts, planted (n + n_far,) bool), shuffled"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n_far, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.concatenate([noisy_sphere(n, seed + 1), 3.0 * d])
    planted = np.arange(n + n_far) >= n
    order = rng.permutation(n + n_far)
    return pts[order], planted[order]
