"""The rule of svs_hip.meshsimplify (include/svolsdf_hip.h, "a mesh made smaller") restated in float64 numpy, and the small
meshes its tests run on.  Same cells, same pair order (f, then k), same segments of 64 pairs summed left to right, then the
segment sums left to right; np.linalg.eigh takes the place of the kernel's cyclic Jacobi, as in cloudclean_oracle.normals.
A cell is CLEAR when no eigenvalue ratio lies within a factor two of `tol` and the solved offset is not within 10 % of the
clamp: the two eigen solvers can only disagree about a decision in cells that are not clear."""
import math

import numpy as np

CELL_BITS = 21
SEGMENT = 64


# ---- the rule ------------------------------------------------------------------------------------------------------------
def default_origin(verts):
    """the cloud operators' origin rule over the finite vertices: their per-axis minimum - 1e-6 (zeros when there are none)"""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    return v.min(0) - 1e-6 if len(v) else np.zeros(3)


def face_geometry(verts, faces):
    """-> valid (F,) bool, corners (F,3,3) float64 (zeros where the indices are bad), n (F,3), L (F,)"""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < len(v))).all(1)
    P = np.zeros((len(f), 3, 3))
    P[inside] = v[f[inside]]
    with np.errstate(all="ignore"):
        finite = np.isfinite(P).all((1, 2))
        u, w = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        L = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        valid = inside & finite & np.isfinite(L) & (L > 0)
    return valid, P, n, L


def cell_index(p, origin, h):
    """(...,3) float64 -> (...,3) int64: floor((p - origin) * (1 / h)) clamped to [0, 2^21)"""
    c = np.floor((p - origin) * (1.0 / h))
    return np.clip(c, 0, (1 << CELL_BITS) - 1).astype(np.int64)


def cell_keys(idx):
    return idx[..., 0] | (idx[..., 1] << CELL_BITS) | (idx[..., 2] << (2 * CELL_BITS))


def cells(verts, faces, h, origin):
    """-> vert_cell (V,) int32, n_cells, index (n_cells,3) int64: the occupied cells ranked by ascending key"""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid = face_geometry(verts, faces)[0]
    used = np.zeros(len(v), bool)
    used[f[valid].reshape(-1)] = True
    vert_cell = np.full(len(v), -1, np.int32)
    idx = cell_index(v[used], np.asarray(origin, np.float64), float(h))
    keys, inverse = np.unique(cell_keys(idx), return_inverse=True)
    vert_cell[used] = inverse.reshape(-1)
    index = np.zeros((len(keys), 3), np.int64)
    index[inverse.reshape(-1)] = idx
    return vert_cell, len(keys), index


def _left_to_right(rows):
    return np.add.accumulate(rows, axis=0)[-1]


def remap_faces(verts, faces, vert_cell):
    """the ranks of the valid faces' corners in corner order, without the collapsed ones and the duplicates (the same set of
    three ranks: the lowest input index stays) -> (faces (M,3) int32 in input order, their input indices)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid = face_geometry(verts, faces)[0]
    at = np.nonzero(valid)[0]
    r = vert_cell[f[at]].astype(np.int64)
    distinct = (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2])
    at, r = at[distinct], r[distinct]
    s = np.sort(r, 1)
    _, first = np.unique(s[:, 0] | (s[:, 1] << CELL_BITS) | (s[:, 2] << (2 * CELL_BITS)), return_index=True)
    first = np.sort(first)
    return r[first].astype(np.int32).reshape(-1, 3), at[first]


def count_faces(verts, faces, h, origin=None):
    origin = default_origin(verts) if origin is None else origin
    return len(remap_faces(verts, faces, cells(verts, faces, h, origin)[0])[0])


def cluster(verts, faces, h, origin=None, colors=None, tol=1e-3):
    """-> dict(verts (C,3) float32, faces (M,3) int32, colors (C,3) uint8 or None, vert_cell, n_cells, info (C,) int32, err (C,),
    clear (C,) bool, centre (C,3): the cells' centres, trace (C,): trace of A, origin)"""
    origin = np.asarray(default_origin(verts) if origin is None else origin, np.float64)
    h = float(h)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid, P, n, L = face_geometry(verts, faces)
    vert_cell, n_cells, index = cells(verts, faces, h, origin)
    centre = origin + (index.astype(np.float64) + 0.5) * h
    # per pair (f, k), valid faces only, in the order f then k
    fv = np.nonzero(valid)[0]
    pf = np.repeat(fv, 3)
    pk = np.tile(np.arange(3), len(fv))
    rank = vert_cell[f[pf, pk]].astype(np.int64)
    c = centre[rank] if len(pf) else np.zeros((0, 3))
    nn, LL, P0, Pk = n[pf], L[pf], P[pf, 0], P[pf, pk]
    d = -((nn[:, 0] * (P0[:, 0] - c[:, 0]) + nn[:, 1] * (P0[:, 1] - c[:, 1])) + nn[:, 2] * (P0[:, 2] - c[:, 2]))
    terms = np.stack([nn[:, 0] * nn[:, 0] / LL, nn[:, 0] * nn[:, 1] / LL, nn[:, 0] * nn[:, 2] / LL, nn[:, 1] * nn[:, 1] / LL,
                      nn[:, 1] * nn[:, 2] / LL, nn[:, 2] * nn[:, 2] / LL, nn[:, 0] * d / LL, nn[:, 1] * d / LL, nn[:, 2] * d / LL,
                      d * d / LL, Pk[:, 0] - c[:, 0], Pk[:, 1] - c[:, 1], Pk[:, 2] - c[:, 2]], 1) if len(pf) else np.zeros((0, 13))
    codes = None if colors is None else np.asarray(colors, np.uint8).reshape(-1, 3).astype(np.int64)[f[pf, pk]]
    order = np.argsort(rank, kind="stable")
    begin = np.searchsorted(rank[order], np.arange(n_cells + 1))
    out = np.zeros((n_cells, 3), np.float32)
    info = np.zeros(n_cells, np.int32)
    err = np.zeros(n_cells)
    clear = np.ones(n_cells, bool)
    trace = np.zeros(n_cells)
    out_colors = None if colors is None else np.zeros((n_cells, 3), np.uint8)
    for r in range(n_cells):
        rows = terms[order[begin[r]:begin[r + 1]]]
        count = len(rows)
        segs = np.stack([_left_to_right(rows[a:a + SEGMENT]) for a in range(0, count, SEGMENT)])
        q = _left_to_right(np.concatenate([np.zeros((1, 13)), segs]))
        A = np.array([[q[0], q[1], q[2]], [q[1], q[3], q[4]], [q[2], q[4], q[5]]])
        b, e, mean = q[6:9], q[9], q[10:13] / float(count)
        lam, vec = np.linalg.eigh(A)
        lmax = lam.max()
        g = np.array([-b[i] - ((A[i, 0] * mean[0] + A[i, 1] * mean[1]) + A[i, 2] * mean[2]) for i in range(3)])
        x = mean.copy()
        kept = 0
        for i in range(3):
            if lam[i] > tol * lmax:
                x = x + vec[:, i] * ((vec[:, i] @ g) / lam[i])
                kept += 1
        ratio = lam / lmax
        reach = np.abs(x).max() if np.isfinite(x).all() else np.inf
        clear[r] = not ((ratio >= tol / 2) & (ratio <= 2 * tol)).any() and not (0.9 * h <= reach <= 1.1 * h)
        fallback = not np.isfinite(x).all() or reach > h
        if fallback:
            x = mean.copy()
        err[r] = x @ (A @ x) + 2.0 * (b @ x) + e
        out[r] = (centre[r] + x).astype(np.float32)
        info[r] = kept | (4 if fallback else 0)
        trace[r] = q[0] + q[3] + q[5]
        if codes is not None:
            total = codes[order[begin[r]:begin[r + 1]]].sum(0)
            out_colors[r] = (2 * total + count) // (2 * count)
    new_faces, source = remap_faces(verts, faces, vert_cell)
    return dict(verts=out, faces=new_faces, colors=out_colors, vert_cell=vert_cell, n_cells=n_cells, info=info, err=err, clear=clear,
                centre=centre, trace=trace, origin=origin, source=source)


def bisect(count, lo, hi, target, tries=16):
    """The search of `svs_hip.meshsimplify.simplify`: log(cell) bisected between lo and hi; count(h) = faces at cell size h.
    -> (the finest cell tried whose count meets the target or None, [(h, count)] in the order tried)"""
    a, b = math.log(lo), math.log(hi)
    best, tried = None, []
    for _ in range(int(tries)):
        mid = 0.5 * (a + b)
        h = float(math.exp(mid))
        n = int(count(h))
        tried.append((h, n))
        if n <= target:
            best = h if best is None or h < best else best
            b = mid
        else:
            a = mid
    return best, tried


# ---- what the tests measure ----------------------------------------------------------------------------------------------
def edges(faces):
    """-> (directed edges (3F,2), unique undirected edges (E,2))"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return d, np.unique(np.sort(d, 1), axis=0)


def euler(n_verts, faces):
    return n_verts - len(edges(faces)[1]) + len(faces)


def closed_oriented_manifold(faces):
    """every directed edge once, and its reverse once"""
    d = edges(faces)[0]
    keys = d[:, 0] * (1 << 32) + d[:, 1]
    back = d[:, 1] * (1 << 32) + d[:, 0]
    return len(np.unique(keys)) == len(keys) and np.array_equal(np.sort(keys), np.sort(back))


# ---- the meshes (coordinates rounded to float32 first) -------------------------------------------------------------------
def _grid_faces(nu, nv, wrap_u=False, wrap_v=False):
    """two triangles per quad of an nu x nv vertex grid, vertex (i, j) = i * nv + j"""
    f = []
    for i in range(nu if wrap_u else nu - 1):
        for j in range(nv if wrap_v else nv - 1):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
            f += [[a, b, d], [a, d, c]]
    return np.array(f, np.int32).reshape(-1, 3)


def uv_sphere(n_lon=48, n_lat=24, radius=1.0, centre=(0.13, 0.21, 0.34)):
    """two poles and n_lat - 1 rings of n_lon vertices: 2 + (n_lat - 1) n_lon vertices, 2 n_lon (n_lat - 1) faces, outward"""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None],
                     np.cos(th)[:, None] * np.ones(n_lon)[None]], -1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]) * radius + np.asarray(centre)
    f = []
    last = 1 + (n_lat - 1) * n_lon
    for j in range(n_lon):
        k = (j + 1) % n_lon
        f.append([0, 1 + j, 1 + k])
        for i in range(n_lat - 2):
            a, b = 1 + i * n_lon + j, 1 + i * n_lon + k
            c, d = a + n_lon, b + n_lon
            f += [[a, c, d], [a, d, b]]
        f.append([last, 1 + (n_lat - 2) * n_lon + k, 1 + (n_lat - 2) * n_lon + j])
    return v.astype(np.float32), np.array(f, np.int32)


def torus(n_major=64, n_minor=24, R=1.0, r=0.4):
    u = 2 * np.pi * np.arange(n_major) / n_major
    w = 2 * np.pi * np.arange(n_minor) / n_minor
    x = (R + r * np.cos(w)[None]) * np.cos(u)[:, None]
    y = (R + r * np.cos(w)[None]) * np.sin(u)[:, None]
    z = r * np.sin(w)[None] * np.ones(n_major)[:, None]
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32), _grid_faces(n_major, n_minor, True, True)


def sheet(n, corner, du, dv):
    """n x n quads: vertex (i, j) = corner + i du / n + j dv / n"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.asarray(corner, np.float64) + i[..., None] * np.asarray(du, np.float64) / n + j[..., None] * np.asarray(dv, np.float64) / n
    return v.reshape(-1, 3), _grid_faces(n + 1, n + 1)


def join(parts):
    """[(verts, faces)] -> one mesh, nothing welded"""
    v, f, at = [], [], 0
    for pv, pf in parts:
        v.append(np.asarray(pv, np.float64)); f.append(np.asarray(pf, np.int32) + at); at += len(pv)
    return np.concatenate(v).astype(np.float32), np.concatenate(f).astype(np.int32)


def cube(n=10):
    """the surface of [-1,1]^3 as six unwelded sheets of n x n quads, outward"""
    parts = []
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for side in (-1.0, 1.0):
            corner = np.full(3, -1.0); corner[axis] = side
            du, dv = np.zeros(3), np.zeros(3)
            du[a], dv[b] = 2.0, 2.0
            parts.append(sheet(n, corner, du, dv) if side > 0 else sheet(n, corner, dv, du))
    return join(parts)


def plane(n=12):
    """a tilted planar sheet"""
    du, dv = np.array([2.0, 0.3, 0.5]), np.array([-0.2, 2.0, 0.7])
    return join([sheet(n, (-1.0, -1.0, -0.4), du, dv)])


def wedge(n=8):
    """two sheets z = +-0.05 (x - 10) over [-1,1]^2: they meet at x = 10, far outside any cell that holds them"""
    parts = []
    for sign in (1.0, -1.0):
        v, f = sheet(n, (-1.0, -1.0, 0.0), (2.0, 0, 0), (0, 2.0, 0))
        v[:, 2] = sign * 0.05 * (v[:, 0] - 10.0)
        parts.append((v, f))
    return join(parts)


def slab(h, n=6):
    """two identically triangulated sheets 0.1 h apart inside one layer of cells of size h (origin (0,0,0)): the second
    sheet's faces all repeat the first's"""
    a = sheet(n, (0.05 * h, 0.07 * h, 0.3 * h), (3.1 * h, 0, 0), (0, 2.9 * h, 0))
    b = (a[0] + np.array([0, 0, 0.1 * h]), a[1])
    return join([a, b]), len(a[1])


def fan(n_faces, radius=1.0, height=0.6):
    """a cone: hub 0 at (0, 0, height), n_faces rim vertices on the circle of `radius` in z = 0, faces (hub, i, i + 1)"""
    ph = 2 * np.pi * np.arange(n_faces) / n_faces
    v = np.concatenate([[[0, 0, height]], np.stack([radius * np.cos(ph), radius * np.sin(ph), np.zeros(n_faces)], 1)])
    f = np.stack([np.zeros(n_faces, np.int64), 1 + np.arange(n_faces), 1 + (np.arange(n_faces) + 1) % n_faces], 1)
    return v.astype(np.float32), f.astype(np.int32)


# ---- the cases both test files run -------------------------------------------------------------------------------------------
def grid_origin(verts, h, pad=0.2):
    """the grid's corner the cases use: `pad` cells below the box of the finite vertices, which keeps the meshes' many axis-
    aligned vertices off the cell walls (exact in float64 for none of them)"""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    return v[np.isfinite(v).all(1)].min(0) - pad * float(h)


CASES = {                                                     # name -> (mesh, cell size, pad of grid_origin)
    "sphere_0.5": (uv_sphere, 0.5, 0.2),
    "sphere_0.3": (uv_sphere, 0.3, 0.2),
    "sphere_one_cell": (uv_sphere, 8.0, 0.2),
    "torus_0.4": (torus, 0.4, 0.2),
    "cube_0.5": (cube, 0.5, 0.2),
    "plane_0.45": (plane, 0.45, 0.2),
    "wedge_2.5": (wedge, 2.5, 0.1),
    "wedge_1.0": (wedge, 1.0, 0.1),
}
FAN_CELL = 2.5
FAN_ORIGIN = (-2.5, -1.1, -2.5 / 3)                          # two rim cells (x < 0, x >= 0), the hub at z = 2 alone in a third


def case(name):
    """-> verts, faces, cell size, origin"""
    if name.startswith("fan_"):
        v, f = fan(int(name[4:]), 1.0, 2.0)
        return v, f, FAN_CELL, np.array(FAN_ORIGIN)
    mesh, h, pad = CASES[name]
    v, f = mesh()
    return v, f, h, grid_origin(v, h, pad)


def threshold_case():
    """Two triangles inside one cell whose quadric is diagonal in exact arithmetic: A = diag(0.75, 0.1875, 0), every term a
    dyadic number.  With tol = 0.25 the middle eigenvalue EQUALS tol * the largest: the rule's strict `>` leaves one direction.
    -> verts, faces, cell size, origin, tol"""
    v = np.array([[0.5, 0.25, 0.25], [0.5, 0.75, 0.25], [0.5, 0.25, 0.75],          # in x = 0.5, |n| = 0.25
                  [1.0, 0.25, 1.0], [1.0, 0.25, 1.25], [1.25, 0.25, 1.0]], np.float32)   # in y = 0.25, |n| = 0.0625
    return v, np.array([[0, 1, 2], [3, 4, 5]], np.int32), 2.0, np.zeros(3), 0.25
