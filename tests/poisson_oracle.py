"""The rule of svs_hip.poisson (include/svolsdf_hip.h, "a surface from an oriented point cloud") restated in float64 numpy:
the six stages in the header's order of sums, the conjugate-gradient recurrence (float64, and with float32 storage emulated by
casts), a scipy.sparse direct solve as the independent check of it, the synthetic clouds and input tables the CPU and GPU
tests share, and the checks of the issue's end-to-end properties.  Nothing here runs on the GPU."""
import functools

import numpy as np

SEGMENT = 64
THREADS = 256


# ---- stage 1: splat ----------------------------------------------------------------------------------------------------------
def locate(pts, dims, origin, h):
    """-> counted (n,) bool, b (n,3) int64 (0 where not counted), t (n,3): g = (p - origin) / h, b = floor(g), t = g - b; a
    point counts iff its coordinates are finite and 0 <= b <= n - 2 on every axis"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        g = (pts - np.asarray(origin, np.float64)) / float(h)
        f = np.floor(g)
        ok = np.isfinite(pts).all(1) & np.isfinite(f).all(1) & (f >= 0).all(1) & (f <= np.asarray(dims, np.float64) - 2).all(1)
        t = g - f
    b = np.where(ok[:, None], f, 0).astype(np.int64)
    return ok, b, np.where(ok[:, None], t, 0.0)


def corner_weights(t):
    """(n,3) -> (n,8): corner c = 4 di + 2 dj + dk has (wx * wy) * wz, w = t for d = 1 and 1 - t for d = 0"""
    w = np.empty((len(t), 8))
    for c in range(8):
        wx = t[:, 0] if c & 4 else 1.0 - t[:, 0]
        wy = t[:, 1] if c & 2 else 1.0 - t[:, 1]
        wz = t[:, 2] if c & 1 else 1.0 - t[:, 2]
        w[:, c] = (wx * wy) * wz
    return w


def splat(pts, normals, dims, origin, h, segment=SEGMENT):
    """-> field (4,n0,n1,n2) float64 (compare float32(field)), counted, skipped.  The order of the sums is the header's: a
    cell's counted points ascending by index in segments of `segment`, each from zero; the segment sums from zero; a node adds
    the corner sums of the cells around it in ascending corner order from zero."""
    n0, n1, n2 = (int(d) for d in dims)
    nrm = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    ok, b, t = locate(pts, dims, origin, h)
    ok &= np.isfinite(nrm).all(1)
    field = np.zeros((4, n0, n1, n2))
    idx = np.flatnonzero(ok)
    if len(idx) == 0:
        return field, 0, len(ok)
    key = (b[idx, 0] * (n1 - 1) + b[idx, 1]) * (n2 - 1) + b[idx, 2]
    order = np.argsort(key, kind="stable")
    idx, key = idx[order], key[order]
    w = corner_weights(t[idx])
    contrib = np.empty((len(idx), 8, 4))
    for p in range(3):
        contrib[:, :, p] = w * nrm[idx, p][:, None]
    contrib[:, :, 3] = w
    head = np.r_[True, key[1:] != key[:-1]]
    run_first = np.flatnonzero(head)
    run_of = np.cumsum(head) - 1
    pos = np.arange(len(idx)) - run_first[run_of]
    seg_head = pos % segment == 0
    seg_start = np.flatnonzero(seg_head)
    seg_end = np.r_[seg_start[1:], len(idx)]
    seg_sum = np.zeros((len(seg_start), 8, 4))
    for j in range(segment):                                   # every segment left to right from zero
        live = seg_start + j < seg_end
        if not live.any():
            break
        seg_sum[live] = seg_sum[live] + contrib[seg_start[live] + j]
    seg_run = run_of[seg_start]
    first_seg = np.flatnonzero(np.r_[True, seg_run[1:] != seg_run[:-1]])
    n_seg = np.diff(np.r_[first_seg, len(seg_start)])
    cell_sum = np.zeros((len(run_first), 8, 4))
    for s in range(int(n_seg.max())):                          # the segment sums left to right from zero
        live = n_seg > s
        cell_sum[live] = cell_sum[live] + seg_sum[first_seg[live] + s]
    cell_key = key[run_first]
    ck = cell_key % (n2 - 1)
    cj = (cell_key // (n2 - 1)) % (n1 - 1)
    ci = cell_key // ((n2 - 1) * (n1 - 1))
    for c in range(8):                                         # per node: ascending corner order (one cell per corner)
        ni, nj, nk = ci + (c >> 2), cj + ((c >> 1) & 1), ck + (c & 1)
        for p in range(4):
            field[p, ni, nj, nk] = field[p, ni, nj, nk] + cell_sum[:, c, p]
    return field, len(idx), len(ok) - len(idx)


# ---- stages 2, 3: divergence and the operator ------------------------------------------------------------------------------------
def _shift(a, axis, step):
    """a[index + step] along axis, 0 beyond the grid"""
    out = np.zeros_like(a)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if step > 0:
        src[axis], dst[axis] = slice(step, None), slice(None, -step)
    else:
        src[axis], dst[axis] = slice(None, step), slice(-step, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def divergence(field, h):
    f = np.asarray(field, np.float32).astype(np.float64)
    d = [_shift(f[a], a, 1) - _shift(f[a], a, -1) for a in range(3)]
    return -((d[0] + d[1]) + d[2]) / (2.0 * float(h))


def apply(x, h):
    """A x = (6 x - ((((((i-1) + (i+1)) + (j-1)) + (j+1)) + (k-1)) + (k+1))) / (h h), 0 beyond the grid"""
    x = np.asarray(x, np.float64)
    s = _shift(x, 0, -1) + _shift(x, 0, 1)
    for a in (1, 2):
        s = s + _shift(x, a, -1)
        s = s + _shift(x, a, 1)
    return (6.0 * x - s) / (float(h) * float(h))


# ---- stage 4: conjugate gradients -------------------------------------------------------------------------------------------------
def cg(rhs, h, tol=1e-4, max_iter=None, check_every=1, storage=np.float64):
    """The header's recurrence from x = 0.  storage=np.float32: vectors rounded to float32 on every store, as the kernels
    store them; per-element arithmetic and dot products float64 either way.  -> x (float64 array of the stored values),
    dict(iterations, residual, converged).  ValueError "no normal field" for a zero right-hand side."""
    st = lambda a: a.astype(storage).astype(np.float64)
    rhs = np.asarray(rhs, np.float32).astype(np.float64)
    max_iter = 4 * max(rhs.shape) if max_iter is None else int(max_iter)
    x = np.zeros_like(rhs)
    r = rhs.copy()
    p = r.copy()
    rr = bb = rn = float(np.vdot(r, r))
    if not (bb > 0 and np.isfinite(bb)):
        raise ValueError("svs_poisson_cg: no normal field")
    it, conv = 0, False
    while it < max_iter:
        q = st(apply(p, h))
        pq = float(np.vdot(p, q))
        alpha = rr / pq if pq > 0 else 0.0
        x = st(x + alpha * p)
        r = st(r - alpha * q)
        rn = float(np.vdot(r, r))
        beta = rn / rr if rr > 0 else 0.0
        rr = rn
        p = st(r + beta * p)
        it += 1
        if it % check_every == 0 or it == max_iter:
            if rn <= tol * tol * bb:
                conv = True
                break
    return x, dict(iterations=it, residual=float(np.sqrt(rn / bb)), converged=conv)


def true_residual(x, rhs, h):
    """|rhs - A x| / |rhs| in float64"""
    rhs = np.asarray(rhs, np.float64)
    return float(np.linalg.norm(rhs - apply(np.asarray(x, np.float64), h)) / np.linalg.norm(rhs))


def direct_solve(rhs, h):
    """A x = rhs by a sparse LU of the Kronecker-sum matrix: shares nothing with `apply` but the definition"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    rhs = np.asarray(rhs, np.float64)
    n0, n1, n2 = rhs.shape
    lap = lambda n: sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    eye = sp.identity
    A = (sp.kron(sp.kron(lap(n0), eye(n1)), eye(n2)) + sp.kron(sp.kron(eye(n0), lap(n1)), eye(n2))
         + sp.kron(sp.kron(eye(n0), eye(n1)), lap(n2))) / (float(h) * float(h))
    return spl.splu(sp.csc_matrix(A)).solve(rhs.reshape(-1)).reshape(rhs.shape)


# ---- stages 5, 6: sample, level, trim ------------------------------------------------------------------------------------------------
def _tree(v):
    """the workgroup's binary tree over 256 values, in place on a copy: s[t] += s[t + d] for d = 128, 64, ... 1"""
    s = np.array(v, np.float64)
    d = THREADS // 2
    while d > 0:
        s[:d] = s[:d] + s[d:2 * d]
        d //= 2
    return s[0]


def fixed_order_sum(values):
    """the device's order: workgroups of 256 consecutive values by `_tree`; thread t of the last pass adds the partials t,
    t + 256, ... from zero; `_tree` again"""
    v = np.asarray(values, np.float64)
    nb = (len(v) + THREADS - 1) // THREADS
    v = np.r_[v, np.zeros(nb * THREADS - len(v))].reshape(nb, THREADS)
    partial = np.array([_tree(row) for row in v])
    acc = np.zeros(THREADS)
    for first in range(0, nb, THREADS):
        chunk = partial[first:first + THREADS]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    return _tree(acc)


def sample(x, pts, dims, origin, h):
    """-> vals (n,) float64 (NaN where the point does not count), level: the mean over the counted points, counted"""
    x = np.asarray(x, np.float32).astype(np.float64)
    ok, b, t = locate(pts, dims, origin, h)
    w = corner_weights(t)
    v = np.zeros(len(ok))
    for c in range(8):
        v = v + w[:, c] * x[b[:, 0] + (c >> 2), b[:, 1] + ((c >> 1) & 1), b[:, 2] + (c & 1)]
    counted = int(ok.sum())
    level = fixed_order_sum(np.where(ok, v, 0.0)) / counted if counted else 0.0
    return np.where(ok, v, np.nan), float(level), counted


def cell_density(W):
    """(n0-1,n1-1,n2-1): the float64 sum of W over a cell's eight nodes in corner order from zero"""
    W = np.asarray(W, np.float32).astype(np.float64)
    n0, n1, n2 = W.shape
    s = np.zeros((n0 - 1, n1 - 1, n2 - 1))
    for c in range(8):
        di, dj, dk = c >> 2, (c >> 1) & 1, c & 1
        s = s + W[di:n0 - 1 + di, dj:n1 - 1 + dj, dk:n2 - 1 + dk]
    return s


def face_keep(W, cells, min_density):
    """keep (F,) uint8; cells: node indices (i*n1 + j)*n2 + k; a node on an upper face or out of range keeps nothing"""
    n0, n1, n2 = np.asarray(W).shape
    cells = np.asarray(cells, np.int64)
    ok = (cells >= 0) & (cells < n0 * n1 * n2)
    c = np.where(ok, cells, 0)
    k, j, i = c % n2, (c // n2) % n1, c // (n1 * n2)
    ok &= (i + 1 < n0) & (j + 1 < n1) & (k + 1 < n2)
    dens = cell_density(W)
    return (ok & (dens[np.minimum(i, n0 - 2), np.minimum(j, n1 - 2), np.minimum(k, n2 - 2)] >= float(min_density))).astype(np.uint8)


def crossing_cells(x, level):
    """node indices (i*n1 + j)*n2 + k of the cells whose eight nodes are not all on one side of the level (x < level is
    inside, as `mesh.marching_cubes` takes it)"""
    inside = np.asarray(x, np.float64) < level
    n0, n1, n2 = inside.shape
    cnt = np.zeros((n0 - 1, n1 - 1, n2 - 1), np.int64)
    for c in range(8):
        di, dj, dk = c >> 2, (c >> 1) & 1, c & 1
        cnt += inside[di:n0 - 1 + di, dj:n1 - 1 + dj, dk:n2 - 1 + dk]
    i, j, k = np.nonzero((cnt > 0) & (cnt < 8))
    return (i * n1 + j) * n2 + k


# ---- the whole pipeline on the host --------------------------------------------------------------------------------------------------
def reconstruct(pts, normals, dims, origin, h, tol=1e-4, storage=np.float32):
    """stages 1 to 5 -> dict(field, rhs, x, info, level, counted, skipped); float32 wherever the device stores float32"""
    field, counted, skipped = splat(pts, normals, dims, origin, h)
    field = field.astype(np.float32)
    rhs = divergence(field, h).astype(np.float32)
    x, info = cg(rhs, h, tol=tol, storage=storage)
    x = x.astype(np.float32)
    _, level, _ = sample(x, pts, dims, origin, h)
    return dict(field=field, rhs=rhs, x=x, info=info, level=level, counted=counted, skipped=skipped)


# ---- synthetic clouds ----------------------------------------------------------------------------------------------------------------
RADIUS = 8.0                                                 # voxels
CENTRE = np.array([11.8, 11.6, 11.7])                        # off the nodes by a fraction of a voxel, in a 24^3 grid
DIMS = (24, 24, 24)
CG_GRIDS = ((12, 13, 14), (24, 24, 24))
# With float32 vectors the recursive residual passes 1e-9 after 66 and 97 iterations on CG_GRIDS (test_poisson_cpu.py), while
# the true one stalls near 2e-6: a solve asked for tol = 1e-9 within this many iterations ends at max_iter, unconverged.
STALL_ITERATIONS = 40


def sphere_of(dims):
    """-> centre, radius in voxels: DIMS holds the sphere of the end-to-end checks; a smaller grid one scaled to its shortest
    axis, as far off the middle node"""
    dims = np.asarray(dims, np.float64)
    return (dims - 1) / 2 + (CENTRE - (np.asarray(DIMS) - 1) / 2), RADIUS * dims.min() / min(DIMS)


def sphere_cloud(n=3000, seed=0, upper=False, dims=DIMS):
    """n seeded points on the sphere `sphere_of(dims)` (voxel 1, origin 0) with exact outward normals -> (pts (n,3) float64,
    normals (n,3) float32); upper: only the points with z >= the centre's (the open hemisphere)"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if upper:
        d = d[d[:, 2] >= 0]
    centre, radius = sphere_of(dims)
    return centre + radius * d, d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def sphere_solution(n=3000, upper=False, dims=DIMS):
    """the oracle's own reconstruction of `sphere_cloud` (computed once, shared, not to be changed)"""
    pts, nrm = sphere_cloud(n, upper=upper, dims=dims)
    out = reconstruct(pts, nrm, dims, np.zeros(3), 1.0)
    out.update(pts=pts, normals=nrm)
    return out


def node_distance(dims=DIMS):
    """signed distance of every node to the sphere in voxels (negative inside)"""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing="ij"), -1)
    return np.linalg.norm(g - CENTRE, axis=-1) - RADIUS


def worst_misclassified(x, level, dims=DIMS):
    """the largest |distance to the sphere| among the nodes whose sign of x - level is not their side's (0 when none)"""
    d = node_distance(dims)
    wrong = (np.asarray(x, np.float64) - level < 0) != (d < 0)
    return float(np.abs(d[wrong]).max()) if wrong.any() else 0.0


def check_closed_surface(x, level, verts, faces, h=1.0, origin=np.zeros(3)):
    """the issue's check 5 on a solution and its mesh (verts in world units) -> dict of the measured figures; asserts"""
    import mesh_oracle as mo
    worst = worst_misclassified(x, level)
    v = (np.asarray(verts, np.float64) - origin) / h
    off = np.abs(np.linalg.norm(v - CENTRE, axis=1) - RADIUS)
    vol = mo.signed_volume(v, faces)
    want = 4.0 / 3.0 * np.pi * RADIUS ** 3
    fig = dict(worst_misclassified=worst, euler=int(mo.euler_characteristic(faces)), worst_vertex=float(off.max()), volume_ratio=vol / want)
    assert worst <= 0.5, fig
    assert fig["euler"] == 2, fig
    assert off.max() <= 1.0, fig
    assert vol > 0 and abs(vol / want - 1.0) <= 0.05, fig
    return fig


def check_open_surface(x, level, W, keep_cells, min_density=2.0):
    """the issue's check 6: keep_cells = the node indices of the cells that still have a face after the trim -> figures"""
    n0, n1, n2 = np.asarray(x).shape
    kept = np.unique(np.asarray(keep_cells, np.int64))
    centre = lambda c: np.stack([c // (n1 * n2), (c // n2) % n1, c % n2], 1) + 0.5
    kc = centre(kept)
    rim = CENTRE[2]
    kd = np.abs(np.linalg.norm(kc - CENTRE, axis=1) - RADIUS)
    cross = crossing_cells(x, level)
    cc = centre(cross)
    must = (np.abs(np.linalg.norm(cc - CENTRE, axis=1) - RADIUS) <= 1.0) & (cc[:, 2] > rim + 1.0)
    share = float(np.isin(cross[must], kept).mean())
    fig = dict(kept=len(kept), lowest=float(rim - kc[:, 2].min()), farthest=float(kd.max()), must=int(must.sum()), share=share,
               crossing=len(cross))
    assert (kc[:, 2] >= rim - 1.0).all(), fig
    assert kd.max() <= 1.5, fig
    assert share >= 0.95, fig
    return fig


# ---- the input tables of the parity tests ----------------------------------------------------------------------------------------------
SPLAT_GRIDS = {"9x10x11": (9, 10, 11), "2x2x2": (2, 2, 2), "7x6x13": (7, 6, 13)}
VOLUME_SHAPES = [(2, 2, 2), (3, 5, 64), (65, 7, 9)]


def splat_case(name, seed=0):
    """-> pts (n,3) float64, normals (n,3) float32, dims, origin, h: random points, points on nodes and cell walls, points with
    b == n - 1, b == -1 and far outside, NaN / inf coordinates and normals, one-cell runs of 63, 64, 65 and 4097 points"""
    dims = SPLAT_GRIDS[name]
    rng = np.random.default_rng(seed + sum(dims))
    origin, h = np.array([-0.75, 0.5, 2.0]), 0.25            # dyadic: a point built as origin + m h sits on node m exactly
    d = np.asarray(dims, np.float64)
    parts = [origin + rng.uniform(0, 1, (2000, 3)) * (d - 1) * h]                       # inside the cells
    nodes = np.stack([rng.integers(0, n, 64) for n in dims], 1).astype(np.float64)
    parts.append(origin + nodes * h)                                                     # exactly on nodes (b == n - 1 among them)
    wall = origin + rng.uniform(0, 1, (64, 3)) * (d - 1) * h
    wall[:, 1] = origin[1] + np.floor(rng.uniform(0, dims[1] - 1, 64)) * h             # t == 0 on one axis
    parts.append(wall)
    parts.append(origin + (d - 1) * h * np.array([[1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, 1.0]]))   # b == n - 1
    parts.append(origin + np.array([[-0.5, 0.5, 0.5], [0.5, -1e-9, 0.5], [0.5, 0.5, -1.0]]) * h)         # b == -1
    parts.append(np.array([[1e9, 0, 0], [0, -1e300, 0], [3e18, 3e18, 3e18]]))                             # far outside
    bad = origin + rng.uniform(0, 1, (6, 3)) * (d - 1) * h
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    parts.append(bad)                                        # rows 3..5 get bad normals below
    for k, run in enumerate((63, 64, 65, 4097)):             # one-cell runs, spread over the cells the grid has
        cell = np.array([k % (dims[0] - 1), (k // 2) % (dims[1] - 1), (3 * k) % (dims[2] - 1)], np.float64)
        parts.append(origin + (cell + rng.uniform(0.01, 0.99, (run, 3))) * h)
    pts = np.concatenate(parts)
    nrm = rng.normal(size=pts.shape).astype(np.float32)
    at = sum(len(p) for p in parts[:6])
    nrm[at + 3, 0], nrm[at + 4, 1], nrm[at + 5, 2] = np.nan, np.inf, -np.inf
    perm = rng.permutation(len(pts))
    return pts[perm], nrm[perm], dims, origin, h


def segment_case():
    """128 points at the centre of one cell (every weight 1/8) whose x normals are 2^80, 63 ones, -2^80, 63 ones: summed in
    segments of 64 the ones are absorbed twice and Vx is 0 at all eight nodes; any other segment length leaves some of them
    (7.875 for one segment of 128).  -> pts, normals, dims, origin, h"""
    dims, origin, h = (3, 4, 5), np.zeros(3), 1.0
    pts = np.tile(np.array([[1.5, 2.5, 3.5]]), (128, 1))
    nrm = np.zeros((128, 3), np.float32)
    nrm[:, 0] = 1.0
    nrm[0, 0], nrm[64, 0] = 2.0 ** 80, -2.0 ** 80
    return pts, nrm, dims, origin, h


def tile_shapes(tile):
    """one shape straddling each extent of the stencil tile by -1, 0, +1 (the other axes small and odd)"""
    t0, t1, t2 = tile
    out = []
    for d in (-1, 0, 1):
        out += [(t0 + d, 5, 8), (3, t1 + d, 12), (3, 5, t2 + d)]
    out.append((2 * t0 + 1, t1 + 1, t2 + 4))               # more than one workgroup along every axis
    return out


def random_volume(shape, seed, planes=None):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(shape if planes is None else (planes,) + tuple(shape))).astype(np.float32)


def dyadic_keep_case():
    """W whose cell sums are exact: cell (1,1,1) sums to exactly 2.0, cell (0,0,0) to 1.75, cell (2,1,1) to 2.25 ->
    W (4,4,4) float32, cells (node indices, with one on an upper face and one out of range), min_density"""
    W = np.zeros((4, 4, 4), np.float32)
    W[1:3, 1:3, 1:3] = 0.25
    W[0, 0, 0] = 1.5
    W[3, 1, 1] = 1.25
    idx = lambda i, j, k: (i * 4 + j) * 4 + k
    cells = np.array([idx(1, 1, 1), idx(0, 0, 0), idx(2, 1, 1), idx(3, 1, 1), idx(1, 3, 1), 64, -1, idx(1, 1, 1)], np.int32)
    return W, cells, 2.0
