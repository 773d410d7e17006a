"""TEST INFRASTRUCTURE ONLY -- the criterion and the case table of the cloud normals (`normals_kernel` of
csrc/svs_cloudknn.hip with the Jacobi of csrc/svs_jacobi3.h).  Numpy only; tests/test_normals_cases_cpu.py proves the
table on the oracle, tests/test_gpu_normals_edges.py holds the GPU to it.  NOTES/normals_edges.md has the reasoning.

THE CRITERION (`figures`, `failures`) holds for EVERY point with m >= 3 points in its set, not only where the
spectrum is clear.  With C the covariance summed here with math.fsum (two passes, a sum the kernel did not compute),
lam = eigvalsh(C) ascending and n the float32 normal widened:
  residual    |C n - lam0 n|_2 <= 2e-7 lam2     a float32 unit vector is within sqrt(3) 2^-24 ~ 1.04e-7 of the float64 one
                                                and |C - lam0 I|_2 <= lam2; the rest covers a float64 solver and the norm
  length      | |n| - 1 | <= 1e-6
  curvature   |curv - lam0 / trace| <= 1e-7     curv <= 1/3: its float32 rounding is <= 2^-24 / 3 ~ 2e-8
              and curv >= +0                    the documented range: a negative rounding of lam0 counts as 0
  angle       to the oracle's normal <= 1e-6 rad where (lam1 - lam0) / lam2 >= 1e-3 (only there is the vector conditioned)
  m < 3       normal and curvature exactly zero
The residual is backward-stable where the angle is not: nearly equal eigenvalues let the eigenvector turn freely inside
their eigenspace, but every vector of that eigenspace satisfies the eigen-equation to the size of the gap.

`kernel_normals` restates the kernel in numpy float64 IN ITS OPERATION ORDER (sums slot by slot, mean = sum * (1 / m),
Rutishauser's rotation term by term, the selects of the pick); the GPU test holds the kernel to it bit for bit.  It exists
to run MUTANTS without a GPU, so that the CPU test can show that the table is sharp: each mutant breaks the criterion on
some case.
  sweeps2         kJacobiSweeps = 2
  pick_lt         the pick's l1 <= l2 as l1 < l2
  no_clamp        lmin used without the clamp at 0
  first_centroid  the centroid taken from the first point of the set instead of the mean
  dot_le          the facing rule flips at dot <= 0
  nearest_le      the nearest centre taken with d2 <= best (the last of equal ones wins)
"""
import functools
import math

import numpy as np

import cloudclean_oracle as co

MUTANTS = ("sweeps2", "pick_lt", "no_clamp", "first_centroid", "dot_le", "nearest_le")
RESIDUAL, LENGTH, CURVATURE, ANGLE, CLEAR = 2e-7, 1e-6, 1e-7, 1e-6, 1e-3
K, RADIUS = 16, 0.5                                          # the scan-scale clouds: tests/test_gpu_cloudclean.py's
CENTRES = np.array([[4.0, 0.3, 0.2], [-0.5, 3.5, 1.0], [0.2, -0.4, -3.8]])
SCALES = {"unit": (1.0, (0.0, 0.0, 0.0)), "dtu": (100.0, (-250.0, 410.0, 630.0)),
          "small": (2.0 ** -10, (0.37, -0.12, 0.05)), "far": (1.0, (1e6, -1e6, 1e6))}
# (r1, r0): the covariance of a neighbourhood has the eigenvalues (1, r1, r0) -- spreads sqrt(1), sqrt(r1), sqrt(r0)
RUNGS = {"plane": (1.0, 1e-2), "sharp_plane": (1.0, 1e-6), "needle": (1e-4, 1e-8), "needle_tie": (1e-3, 1e-3 * (1 + 1e-9)),
         "ball": (1 - 1e-9, 1 - 2e-9)}
COUNTS = (1, 255, 256, 257, 513)


# ---- the reference covariance and the criterion ------------------------------------------------------------------------------
def neighbour_sets(pts, idx, include_self):
    """per point the rows of its set, in the order cloudclean_oracle.normals reads them: the point, then the valid slots"""
    n = len(pts)
    return [([i] if include_self else []) + [int(j) for j in idx[i] if 0 <= j < n] for i in range(n)]


def reference_covariance(pts, idx, include_self):
    """-> (C (n,3,3) float64, m (n,)): per entry two passes of math.fsum (exactly rounded sums); zeros where m < 3"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    sets = neighbour_sets(pts, idx, include_self)
    C, m = np.zeros((len(pts), 3, 3)), np.array([len(s) for s in sets])
    for i, s in enumerate(sets):
        if len(s) < 3:
            continue
        S = pts[s]
        d = S - np.array([math.fsum(S[:, a]) / len(s) for a in range(3)])
        for a in range(3):
            for b in range(a, 3):
                C[i, a, b] = C[i, b, a] = math.fsum(d[:, a] * d[:, b]) / len(s)
    return C, m


def figures(c, nrm, curv):
    """Every number the criterion needs of the outputs (nrm (n,3), curv (n,)) on case c; nothing is asserted here."""
    nrm, curv = np.asarray(nrm), np.asarray(curv)
    C, m, lam = c["C"], c["m"], c["lam"]
    live = m >= 3
    n64 = nrm.astype(np.float64)
    res = np.linalg.norm(np.einsum("nab,nb->na", C, n64) - lam[:, :1] * n64, axis=1)
    bound = RESIDUAL * lam[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, res / bound, np.where(res == 0, 0.0, np.inf))
        want_curv = np.where(lam.sum(1) > 0, lam[:, 0] / lam.sum(1), 0.0)
    clear = live & ((lam[:, 1] - lam[:, 0]) >= CLEAR * lam[:, 2]) & (lam[:, 2] > 0)
    ang = co.angle(n64, c["oracle"][0])
    return dict(live=live, clear=clear, finite=bool(np.isfinite(n64).all() and np.isfinite(curv).all()),
                residual=np.where(live, ratio, 0.0), length=np.where(live, np.abs(np.linalg.norm(n64, axis=1) - 1), 0.0),
                curvature=np.where(live, np.abs(curv.astype(np.float64) - want_curv), 0.0),
                negative=live & ((curv < 0) | np.signbit(curv)), angle=np.where(clear, ang, 0.0),
                dead_zero=bool(not n64[~live].any() and not np.asarray(curv)[~live].any()))


def summary(f):
    return (f"{int(f['live'].sum())} points with m >= 3 ({int(f['clear'].sum())} clear): residual / bound {f['residual'].max():.3e}, "
            f"angle {f['angle'].max():.3e} rad, curvature off by {f['curvature'].max():.3e}, length off by {f['length'].max():.3e}")


def failures(f):
    """the names of the bounds the figures miss (empty: the criterion holds)"""
    bad = []
    if not f["finite"]:
        bad.append("finite")
    if not (f["residual"] <= 1.0).all():
        bad.append("residual")
    if not (f["length"] <= LENGTH).all():
        bad.append("length")
    if not (f["curvature"] <= CURVATURE).all():
        bad.append("curvature")
    if f["negative"].any():
        bad.append("negative curvature")
    if not (f["angle"] <= ANGLE).all():
        bad.append("angle")
    if not f["dead_zero"]:
        bad.append("m < 3 not zero")
    return bad


def exact_failures(c, nrm, curv):
    """cases with `expect`: the same axis and the same sign as stated, exactly, in every live row"""
    if c.get("expect") is None:
        return []
    live = c["m"] >= 3
    bad = [] if np.array_equal(np.asarray(nrm, np.float64)[live], c["expect"][live]) else ["expected normal"]
    if c.get("expect_curv") is not None and not np.array_equal(np.asarray(curv, np.float64)[live], c["expect_curv"][live]):
        bad.append("expected curvature")
    return bad


def signed_failures(c, nrm):
    """cases with centres: on the clear points whose facing is not within rounding of 0, the oracle's sign"""
    if c["centres"] is None:
        return []
    want, facing = c["oracle"][0], c["oracle"][3]
    sure = (c["m"] >= 3) & ((c["lam"][:, 1] - c["lam"][:, 0]) >= CLEAR * c["lam"][:, 2]) & (np.abs(facing) > 1e-9)
    return [] if (co.angle(np.asarray(nrm, np.float64)[sure], want[sure], signed=True) <= ANGLE).all() else ["facing"]


# ---- the kernel, restated in its operation order -----------------------------------------------------------------------------
def _rotate(a, v, P, Q):
    apq = a[P][Q]
    go = apq != 0.0
    theta = (a[Q][Q] - a[P][P]) / (2.0 * np.where(go, apq, 1.0))
    t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    tt = np.where(np.abs(theta) > 1e150, 0.5 / np.where(theta == 0.0, 1.0, theta), t)
    c = 1.0 / np.sqrt(tt * tt + 1.0)
    s = tt * c
    R = 3 - P - Q
    app, aqq, arp, arq = a[P][P], a[Q][Q], a[R][P], a[R][Q]

    def put(r, q, new):
        a[r][q] = a[q][r] = np.where(go, new, a[r][q])
    put(P, P, app - tt * apq)
    put(Q, Q, aqq + tt * apq)
    put(P, Q, np.zeros_like(apq))
    put(R, P, c * arp - s * arq)
    put(R, Q, s * arp + c * arq)
    for i in range(3):
        vip, viq = v[i][P], v[i][Q]
        v[i][P] = np.where(go, c * vip - s * viq, vip)
        v[i][Q] = np.where(go, s * vip + c * viq, viq)


def kernel_normals(pts, idx, include_self=True, view_index=None, centres=None, mut=frozenset(), raw=False, sweeps=8):
    """-> (normals (n,3) float32, curvature (n,) float32 [, dict(lmin, trace, m, dot) before clamp and flip]); sweeps: the
    kernel's kJacobiSweeps"""
    mut = frozenset(mut)
    assert mut <= set(MUTANTS)
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    idx = np.asarray(idx, np.int64).reshape(n, -1)
    k = idx.shape[1]
    valid = (idx >= 0) & (idx < n)
    nb = pts[np.where(valid, idx, 0)]                                      # (n,k,3)
    p = [pts[:, a].copy() for a in range(3)]
    s = [p[a].copy() if include_self else np.zeros(n) for a in range(3)]
    m = np.full(n, 1 if include_self else 0)
    for t in range(k):
        s = [np.where(valid[:, t], s[a] + nb[:, t, a], s[a]) for a in range(3)]
        m = m + valid[:, t]
    inv_m = 1.0 / np.maximum(m, 1)
    mean = [s[a] * inv_m for a in range(3)]
    if "first_centroid" in mut:
        first = nb[np.arange(n), np.argmax(valid, 1)]
        mean = [p[a] if include_self else first[:, a] for a in range(3)]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    e = [p[a] - mean[a] for a in range(3)]
    cov = [e[a] * e[b] if include_self else np.zeros(n) for a, b in pairs]
    for t in range(k):
        e = [nb[:, t, a] - mean[a] for a in range(3)]
        cov = [np.where(valid[:, t], cov[q] + e[a] * e[b], cov[q]) for q, (a, b) in enumerate(pairs)]
    a = [[None] * 3 for _ in range(3)]
    for q, (r, c) in enumerate(pairs):
        a[r][c] = a[c][r] = cov[q] * inv_m
    v = [[np.full(n, 1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    with np.errstate(all="ignore"):
        for _ in range(2 if "sweeps2" in mut else sweeps):
            _rotate(a, v, 0, 1)
            _rotate(a, v, 0, 2)
            _rotate(a, v, 1, 2)
    l0, l1, l2 = a[0][0], a[1][1], a[2][2]
    pick1 = (l1 < l0) & ((l1 < l2) if "pick_lt" in mut else (l1 <= l2))
    pick2 = (l2 < l0) & (l2 < l1)
    ex, ey, ez = (np.where(pick2, v[r][2], np.where(pick1, v[r][1], v[r][0])) for r in range(3))
    lmin = np.where(pick2, l2, np.where(pick1, l1, l0))
    trace = l0 + l1 + l2
    with np.errstate(all="ignore"):
        top = lmin if "no_clamp" in mut else np.where(lmin > 0.0, lmin, 0.0)
        curv = np.where(trace > 0.0, (top / np.where(trace > 0.0, trace, 1.0)).astype(np.float32), np.float32(0.0))
    length = np.sqrt(ex * ex + ey * ey + ez * ez)
    div = np.where(length > 0.0, length, 1.0)
    ex, ey, ez = (np.where(length > 0.0, w / div, w) for w in (ex, ey, ez))
    dot = np.full(n, np.nan)
    if centres is not None:
        C = np.asarray(centres, np.float64).reshape(-1, 3)
        if view_index is not None:
            ci = np.clip(np.asarray(view_index, np.int64), 0, len(C) - 1)
        else:
            best, ci = np.full(n, 1e300), np.zeros(n, np.int64)
            for w in range(len(C)):
                dx, dy, dz = C[w, 0] - p[0], C[w, 1] - p[1], C[w, 2] - p[2]
                d2 = dx * dx + dy * dy + dz * dz
                closer = (d2 <= best) if "nearest_le" in mut else (d2 < best)
                best, ci = np.where(closer, d2, best), np.where(closer, w, ci)
        dot = ex * (C[ci, 0] - p[0]) + ey * (C[ci, 1] - p[1]) + ez * (C[ci, 2] - p[2])
        flip = (dot <= 0.0) if "dot_le" in mut else (dot < 0.0)
        ex, ey, ez = (np.where(flip, -w, w) for w in (ex, ey, ez))
    live = m >= 3
    nrm = np.where(live[:, None], np.stack([ex, ey, ez], 1), 0.0).astype(np.float32)
    curv = np.where(live, curv, np.float32(0.0)).astype(np.float32)
    return (nrm, curv, dict(lmin=lmin, trace=trace, m=m, dot=dot)) if raw else (nrm, curv)


# ---- building blocks ---------------------------------------------------------------------------------------------------------
def _finish(name, family, pts, idx, include_self=True, view_index=None, centres=None, **extra):
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    idx = np.ascontiguousarray(idx, np.int32).reshape(len(pts), -1)
    if view_index is not None:
        view_index = np.ascontiguousarray(view_index, np.int32)
    if centres is not None:
        centres = np.ascontiguousarray(centres, np.float64).reshape(-1, 3)
    assert len(pts) <= 1300
    C, m = reference_covariance(pts, idx, include_self)
    c = dict(name=name, family=family, pts=pts, idx=idx, include_self=include_self, view_index=view_index, centres=centres,
             C=C, m=m, lam=np.linalg.eigvalsh(C), oracle=co.normals(pts, idx, include_self, view_index, centres))
    c.update(extra)
    return c


def blocks_table(sizes, k=None):
    """idx of a cloud made of blocks of the given sizes: every point's slots hold the other points of its block, in order"""
    k = max(sizes) - 1 if k is None else k
    idx = np.full((sum(sizes), k), -1, np.int32)
    a = 0
    for size in sizes:
        for i in range(size):
            idx[a + i, :size - 1] = [a + j for j in range(size) if j != i]
        a += size
    return idx


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def _axis_rows(expect, n):
    return np.tile(np.asarray(expect, np.float64), (n, 1))


# ---- the families ------------------------------------------------------------------------------------------------------------
def _base_cloud(cloud):
    return co.noisy_sphere(1000, 0) if cloud == "sphere" else co.noisy_plane(1000, 1)


def _scan(cloud, scale):
    s, t = SCALES[scale]
    pts = s * _base_cloud(cloud) + np.array(t)
    _, idx, _ = co.knn(pts, pts, K, RADIUS * s, exclude_same_index=True)
    view = np.random.default_rng(5).integers(0, 3, len(pts)).astype(np.int32)
    return _finish(f"scan-{cloud}-{scale}", "scan", pts, idx, True, view, s * CENTRES + np.array(t), k=K, radius=RADIUS * s,
                   base=f"scan-{cloud}-unit", s=s)


def _ladder(rung):
    """64 neighbourhoods of 17 points: a box cloud whitened to the identity covariance, its axes scaled to the rung's
    eigenvalues, turned by a rotation of its own.  Every point of a block sees the same set in another order."""
    r1, r0 = RUNGS[rung]
    rng = np.random.default_rng(100 + list(RUNGS).index(rung))
    blocks = []
    for _ in range(64):
        X = rng.uniform(-1, 1, (17, 3))
        X -= X.mean(0)
        w, V = np.linalg.eigh(X.T @ X / 17)
        blocks.append((X @ V / np.sqrt(w)) * np.sqrt([1.0, r1, r0]) @ rotation(rng).T)
    return _finish(f"ladder-{rung}", "ladder", np.concatenate(blocks), blocks_table([17] * 64), ratios=(r1, r0))


def _lattice(nx, ny, nz):
    g = np.stack(np.meshgrid(*[np.arange(v, dtype=np.float64) - (v - 1) / 2 for v in (nx, ny, nz)], indexing="ij"), -1)
    return g.reshape(-1, 3)


def _star(sx, sy, sz):
    """a lattice node at the origin and its two neighbours along every axis, at the given steps"""
    return np.array([[0, 0, 0], [sx, 0, 0], [-sx, 0, 0], [0, sy, 0], [0, -sy, 0], [0, 0, sz], [0, 0, -sz]], np.float64)


# tilted integer lattice: i (1,0,1) + j (0,1,2) + a shear -- exactly coplanar (normal (1,2,-1)), no axis special
_TILTED = np.array([[i + 3 * j, j - 2 * i, i + 3 * j + 2 * (j - 2 * i)] for i in (-1, 0, 1) for j in (-1, 0, 1)], np.float64)

EXACT = {
    # name: (points of the one block, spectrum ascending or None, normal or None)
    "lattice331": (_lattice(3, 3, 1), (0.0, 6.0 / 9, 6.0 / 9), (0, 0, 1)),
    "collinear_x": (_lattice(5, 1, 1), (0.0, 0.0, 2.0), (0, 1, 0)),
    "collinear_z": (_lattice(1, 1, 5), (0.0, 0.0, 2.0), (1, 0, 0)),
    "star111": (_star(1, 1, 1), (2.0 / 7, 2.0 / 7, 2.0 / 7), (1, 0, 0)),
    "star211": (_star(2, 1, 1), (2.0 / 7, 2.0 / 7, 8.0 / 7), (0, 1, 0)),
    "star112": (_star(1, 1, 2), (2.0 / 7, 2.0 / 7, 8.0 / 7), (1, 0, 0)),
    "star121": (_star(1, 2, 1), (2.0 / 7, 2.0 / 7, 8.0 / 7), (1, 0, 0)),
    "coincident": (np.tile([[3.0, -5.0, 0.375]], (4, 1)), (0.0, 0.0, 0.0), (1, 0, 0)),
    "tilted_lattice": (_TILTED, None, None),
}


def _exact(name):
    block, spectrum, normal = EXACT[name]
    extra = dict(spectrum=spectrum)
    if normal is not None:
        extra.update(expect=_axis_rows(normal, len(block)))
    if spectrum is not None and spectrum[0] == 0.0:
        extra.update(expect_curv=np.zeros(len(block)))
    return _finish(f"exact-{name}", "exact", block, blocks_table([len(block)]), **extra)


def _slots(name):
    """explicit tables on a small random cloud: what a slot may hold and where the valid ones sit"""
    n = 40
    pts = co.random_cloud(n, 77)
    rng = np.random.default_rng(78)
    BIG = 2 ** 31 - 1

    def others(i, count):
        return rng.permutation([j for j in range(n) if j != i])[:count]
    if name == "k2_self":                                    # include_self with two valid slots: m == 3; one: m == 2
        idx = np.array([list(others(i, 2)) if i % 4 else [[-1, others(i, 1)[0]], [others(i, 1)[0], n], [BIG, -1],
                                                          [others(i, 1)[0], -7]][(i // 4) % 4] for i in range(n)])
        return _finish("slots-k2_self", "slots", pts, idx, True, m_values={1, 2, 3})
    if name == "k3_noself":                                  # without the point: three valid slots, m == 3; two: m == 2
        idx = np.array([list(others(i, 3)) if i % 3 else ([-1] + list(others(i, 2)) if i % 2 else list(others(i, 2)) + [n + i])
                        for i in range(n)])
        return _finish("slots-k3_noself", "slots", pts, idx, False, m_values={2, 3})
    if name == "k2_noself":                                  # two slots without the point: never a plane
        return _finish("slots-k2_noself", "slots", pts, np.array([others(i, 2) for i in range(n)]), False, m_values={2})
    idx = np.full((n, 32), -1, np.int64)
    for i in range(n):
        kind = i % 5
        if kind == 0:                                        # valid slots between -1 and indices >= n
            idx[i, 0::3], idx[i, 1::3] = others(i, 11), rng.choice([n, n + 1, BIG], 11)
        elif kind == 1:                                      # the valid slots only at the end
            idx[i, :28], idx[i, 28:] = rng.choice([-1, n, BIG], 28), others(i, 4)
        elif kind == 2:                                      # two valid slots at the very end: m == 3 (or 2 without self)
            idx[i, 30:] = others(i, 2)
        elif kind == 3:                                      # a full row
            idx[i] = others(i, 32)
        # kind 4: nothing valid
    if name == "k32_self":
        return _finish("slots-k32_self", "slots", pts, idx, True, m_values={1, 3, 5, 12, 33})
    return _finish("slots-k32_noself", "slots", pts, idx, False, m_values={0, 2, 4, 11, 32})


def _facing(name):
    if name == "view_clamp":                                 # view indices below 0 and at / beyond n_views
        pts = co.noisy_sphere(300, 3)
        _, idx, _ = co.knn(pts, pts, K, 1.0, exclude_same_index=True)
        view = np.random.default_rng(9).choice([-1, -2 ** 31, 0, 1, 2, 3, 4, 2 ** 31 - 1], len(pts)).astype(np.int32)
        clamped = np.clip(view, 0, 2)
        return _finish("facing-view_clamp", "facing", pts, idx, True, view, CENTRES, clamped=clamped)
    lattice = _lattice(3, 3, 1)                              # the plane z = 0: the solver gives (0,0,1) exactly
    n = len(lattice)
    table = {
        # centres, view index, the normal every row must have
        "tangent": ([[5.0, 3.0, 0.0]], None, (0, 0, 1)),                     # dot == 0 for every point of the plane: no flip
        "tangent_by_view": ([[9.0, 9.0, 9.0], [5.0, 3.0, 0.0]], np.ones(n, np.int32), (0, 0, 1)),
        "below": ([[5.0, 3.0, -1.0]], None, (0, 0, -1)),                     # the flip itself
        "above": ([[5.0, 3.0, 1.0]], None, (0, 0, 1)),
        "nearest_tie_down": ([[0.0, 0.0, -4.0], [0.0, 0.0, 4.0]], None, (0, 0, -1)),    # equal distances: the first centre
        "nearest_tie_up": ([[0.0, 0.0, 4.0], [0.0, 0.0, -4.0]], None, (0, 0, 1)),
    }
    centres, view, normal = table[name]
    return _finish(f"facing-{name}", "facing", lattice, blocks_table([n]), True, view, np.array(centres),
                   expect=_axis_rows(normal, n), expect_curv=np.zeros(n))


def _count(n):
    s, t = SCALES["dtu"]
    pts = s * co.noisy_sphere(n, 40 + n) + np.array(t)
    _, idx, _ = co.knn(pts, pts, K, 1.0 * s, exclude_same_index=True)
    return _finish(f"count-{n}", "count", pts, idx, True, n_points=n)


FAMILIES = {
    "scan": {f"scan-{cloud}-{scale}": functools.partial(_scan, cloud, scale) for cloud in ("sphere", "plane") for scale in SCALES},
    "ladder": {f"ladder-{rung}": functools.partial(_ladder, rung) for rung in RUNGS},
    "exact": {f"exact-{name}": functools.partial(_exact, name) for name in EXACT},
    "slots": {f"slots-{name}": functools.partial(_slots, name) for name in ("k2_self", "k2_noself", "k3_noself", "k32_self",
                                                                           "k32_noself")},
    "facing": {f"facing-{name}": functools.partial(_facing, name) for name in ("view_clamp", "tangent", "tangent_by_view", "below",
                                                                             "above", "nearest_tie_down", "nearest_tie_up")},
    "count": {f"count-{n}": functools.partial(_count, n) for n in COUNTS},
}
NAMES = {family: list(makers) for family, makers in FAMILIES.items()}
ALL = [name for names in NAMES.values() for name in names]


@functools.lru_cache(maxsize=None)
def case(name):
    """the case of that name, built once and shared: treat it as read-only"""
    return FAMILIES[name.split("-")[0]][name]()


def all_failures(c, nrm, curv):
    """everything a case asks of a pair of outputs -> (figures, the names of what is missed)"""
    f = figures(c, nrm, curv)
    return f, failures(f) + exact_failures(c, nrm, curv) + signed_failures(c, nrm)
