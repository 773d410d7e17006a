"""The screened rule of svs_hip.poisson (include/svolsdf_hip.h, "point constraints and a preconditioned solve") restated in
float64 numpy on top of tests/poisson_oracle.py: the operator A + diag(weight W), the Jacobi-preconditioned recurrence
(float64, and with float32 storage emulated by casts), a scipy.sparse direct solve of the same system as the independent
check of it, the density rule that turns a `screen` value into a weight, the cloud of uneven density the CPU and GPU tests
share, and the radial-probe error of a level set.  Nothing here runs on the GPU."""
import functools

import numpy as np

import poisson_oracle as po

SCREENS = (0.0, 1.0, 4.0, 16.0)
KEEP_SHARE = 0.15                                            # of the points on the thin side of the uneven cloud
PROBE_RAYS = 2000
PROBE_REACH = 3.0                                            # voxels either side of the sphere a ray is searched over
PROBE_STEP = 0.05


# ---- the operator and the preconditioned recurrence -----------------------------------------------------------------------------
def _w64(W):
    return np.asarray(W, np.float32).astype(np.float64)


def diagonal(W, h, weight):
    """d = 6 / (h h) + weight * W"""
    return 6.0 / (float(h) * float(h)) + float(weight) * _w64(W)


def apply(x, W, h, weight):
    """a = (6 x - s) / (h h) as `po.apply` forms it, b = (weight * W) * x, y = a + b"""
    x = np.asarray(x, np.float64)
    return po.apply(x, h) + (float(weight) * _w64(W)) * x


def pcg(rhs, W, h, weight, tol=1e-4, max_iter=None, check_every=1, storage=np.float64):
    """The header's preconditioned recurrence from x = 0; z = r / d is never stored.  storage=np.float32: vectors rounded to
    float32 on every store.  -> x (float64 array of the stored values), dict(iterations, residual, converged).  ValueError
    "no normal field" for a zero right-hand side."""
    st = lambda a: a.astype(storage).astype(np.float64)
    rhs = np.asarray(rhs, np.float32).astype(np.float64)
    max_iter = 4 * max(rhs.shape) if max_iter is None else int(max_iter)
    d = diagonal(W, h, weight)
    x = np.zeros_like(rhs)
    r = rhs.copy()
    p = st(r / d)
    rz = float(np.vdot(r, r / d))
    bb = rn = float(np.vdot(r, r))
    if not (bb > 0 and np.isfinite(bb)):
        raise ValueError("svs_screened_pcg: no normal field")
    it, conv = 0, False
    while it < max_iter:
        q = st(apply(p, W, h, weight))
        pq = float(np.vdot(p, q))
        alpha = rz / pq if pq > 0 else 0.0
        x = st(x + alpha * p)
        r = st(r - alpha * q)
        rn = float(np.vdot(r, r))
        rzn = float(np.vdot(r, r / d))
        beta = rzn / rz if rz > 0 else 0.0
        rz = rzn
        p = st(r / d + beta * p)
        it += 1
        if it % check_every == 0 or it == max_iter:
            if rn <= tol * tol * bb:
                conv = True
                break
    return x, dict(iterations=it, residual=float(np.sqrt(rn / bb)), converged=conv)


def true_residual(x, rhs, W, h, weight):
    """|rhs - (A + weight W) x| / |rhs| in float64"""
    rhs = np.asarray(rhs, np.float64)
    return float(np.linalg.norm(rhs - apply(np.asarray(x, np.float64), W, h, weight)) / np.linalg.norm(rhs))


def direct_solve(rhs, W, h, weight):
    """(A + diag(weight W)) x = rhs by a sparse LU of the Kronecker-sum matrix plus the diagonal: shares nothing with `apply`
    but the definition"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    rhs = np.asarray(rhs, np.float64)
    n0, n1, n2 = rhs.shape
    lap = lambda n: sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    eye = sp.identity
    A = (sp.kron(sp.kron(lap(n0), eye(n1)), eye(n2)) + sp.kron(sp.kron(eye(n0), lap(n1)), eye(n2))
         + sp.kron(sp.kron(eye(n0), eye(n1)), lap(n2))) / (float(h) * float(h))
    A = A + sp.diags(float(weight) * _w64(W).reshape(-1))
    return spl.splu(sp.csc_matrix(A)).solve(rhs.reshape(-1)).reshape(rhs.shape)


def screen_weight(W, counted, screen, voxel):
    """-> (weight, density): density = counted / the number of nodes the splat touched (W != 0), the points per touched node;
    weight = screen / (density * voxel * voxel)"""
    density = float(counted) / float(np.count_nonzero(np.asarray(W)))
    return float(screen) / (density * float(voxel) * float(voxel)), density


# ---- the cloud of uneven density ---------------------------------------------------------------------------------------------------
def uneven_cloud(n=3000, dims=po.DIMS):
    """`po.sphere_cloud(n, dims=dims)` thinned: a point stays if x > the centre's, or if default_rng(1).random(n) < 0.15
    (1699 of 3000) -> pts, normals"""
    pts, nrm = po.sphere_cloud(n, dims=dims)
    centre = po.sphere_of(dims)[0]
    keep = (pts[:, 0] > centre[0]) | (np.random.default_rng(1).random(len(pts)) < KEEP_SHARE)
    return pts[keep], nrm[keep]


@functools.lru_cache(maxsize=None)
def uneven_system(dims=po.DIMS):
    """the oracle's splat and divergence of `uneven_cloud` on dims, voxel 1, origin 0 (computed once, shared, not to be
    changed) -> dict(pts, normals, field, rhs (float32), W (float32), counted)"""
    pts, nrm = uneven_cloud(dims=dims)
    field, counted, skipped = po.splat(pts, nrm, dims, np.zeros(3), 1.0)
    field = field.astype(np.float32)
    return dict(pts=pts, normals=nrm, field=field, rhs=po.divergence(field, 1.0).astype(np.float32), W=field[3], counted=counted)


@functools.lru_cache(maxsize=None)
def uneven_solution(dims=po.DIMS, screen=0.0, storage="float32", even=False):
    """the oracle's own screened solve (tol 1e-4, check_every 1) -> dict(x (float64 array of the stored values), info, level,
    weight, density); even=True: the clean `po.sphere_cloud` in place of the uneven one"""
    if even:
        s = po.sphere_solution(dims=dims)
        sys_ = dict(pts=s["pts"], rhs=s["rhs"], W=s["field"][3], counted=s["counted"])
    else:
        sys_ = uneven_system(dims)
    weight, density = screen_weight(sys_["W"], sys_["counted"], screen, 1.0)
    x, info = pcg(sys_["rhs"], sys_["W"], 1.0, weight, tol=1e-4, storage=np.dtype(storage).type)
    level = po.sample(x.astype(np.float32), sys_["pts"], dims, np.zeros(3), 1.0)[1]
    return dict(x=x, info=info, level=level, weight=weight, density=density)


# ---- the radial probe ----------------------------------------------------------------------------------------------------------------
def _trilinear(x, q):
    """x at the positions q (m,3) in node units, clamped into the grid's cells"""
    n = np.asarray(x.shape, np.float64)
    q = np.clip(q, 0.0, n - 1.0)
    b = np.minimum(np.floor(q), n - 2).astype(np.int64)
    t = q - b
    w = po.corner_weights(t)
    v = np.zeros(len(q))
    for c in range(8):
        v = v + w[:, c] * x[b[:, 0] + (c >> 2), b[:, 1] + ((c >> 1) & 1), b[:, 2] + (c & 1)]
    return v


def radial_error(x, level, rays=PROBE_RAYS, seed=0):
    """PROBE_RAYS seeded directions from the sphere's centre: along each, the crossing of the trilinear x with the level
    nearest to the sphere (searched PROBE_REACH voxels either side in steps of PROBE_STEP, linear between steps; a ray with
    no crossing counts PROBE_REACH) -> dict(rms, max) of |crossing - RADIUS| in voxels"""
    x = np.asarray(x, np.float64)
    d = np.random.default_rng(seed).normal(size=(rays, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    radii = po.RADIUS + np.arange(-PROBE_REACH, PROBE_REACH + PROBE_STEP / 2, PROBE_STEP)
    vals = np.stack([_trilinear(x, po.CENTRE + r * d) for r in radii], 1) - level            # (rays, steps)
    a, b = vals[:, :-1], vals[:, 1:]
    cross = (a < 0) != (b < 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        at = radii[:-1] + PROBE_STEP * np.where(cross, a / (a - b), 0.0)
    off = np.where(cross, np.abs(at - po.RADIUS), PROBE_REACH)
    err = off.min(1)
    return dict(rms=float(np.sqrt(np.mean(err * err))), max=float(err.max()))
