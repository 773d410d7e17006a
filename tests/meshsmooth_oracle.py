"""The rule of svs_hip.meshsmooth (include/svolsdf_hip.h, "a mesh made smoother") restated in float64 numpy, and the small
meshes its tests run on.  Same validity test, same neighbour and face lists (ascending), every sum taken left to right from
zero over a vertex's (or a face's) own list: numpy's elementwise float64 operations are the device's IEEE operations, so the
float64 results agree to the bit and the float32 outputs are compared for equality (at most one step)."""
import numpy as np

from meshsimplify_oracle import face_geometry

USED, BOUNDARY, NONMANIFOLD = 1, 2, 4
FIXED, CURVE, FREE = 0, 1, 2
MODES = dict(fixed=FIXED, curve=CURVE, free=FREE)


# ---- the rule ------------------------------------------------------------------------------------------------------------
def adjacency(verts, faces):
    """-> dict(nbr_start (V+1,), nbr, nbr_boundary, face_start (V+1,), vert_face, face_valid (F,) uint8, flags (V,) int32,
    counts [edges, boundary edges, non-manifold edges, valid faces])"""
    V = len(np.asarray(verts).reshape(-1, 3))
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid = face_geometry(verts, faces)[0]
    at = np.nonzero(valid)[0]
    fv = f[at]
    a, b = fv.reshape(-1), fv[:, [1, 2, 0]].reshape(-1)
    key = np.concatenate([a << 32 | b, b << 32 | a])
    uniq, use = np.unique(key, return_counts=True)
    ua, ub = uniq >> 32, uniq & 0xffffffff
    flags = np.zeros(V, np.int32)
    flags[a] |= USED
    flags[ua[use == 1]] |= BOUNDARY
    flags[ua[use > 2]] |= NONMANIFOLD
    once = ua < ub
    corner_f = np.repeat(at, 3)
    order = np.argsort(a, kind="stable")                      # a is in (f, k) order: a vertex's faces stay ascending
    return dict(nbr_start=np.searchsorted(ua, np.arange(V + 1)).astype(np.int32), nbr=ub.astype(np.int32),
                nbr_boundary=(use == 1).astype(np.uint8), face_start=np.searchsorted(a[order], np.arange(V + 1)).astype(np.int32),
                vert_face=corner_f[order].astype(np.int32), face_valid=valid.astype(np.uint8), flags=flags,
                counts=[int(once.sum()), int((once & (use == 1)).sum()), int((once & (use > 2)).sum()), int(valid.sum())])


def _ordered_add(acc, start, terms, keep=None):
    """acc[r] += terms[start[r]], terms[start[r] + 1], ... one after the other (entries with keep == False left out)
    -> how many were added per row"""
    length = np.diff(start)
    count = np.zeros(len(length), np.int64)
    for t in range(int(length.max()) if len(length) else 0):
        rows = np.nonzero(length > t)[0]
        pos = start[rows] + t
        if keep is not None:
            rows, pos = rows[keep[pos]], pos[keep[pos]]
        acc[rows] = acc[rows] + terms[pos]
        count[rows] += 1
    return count


def taubin_pass(x, adj, s, boundary):
    flags, start = adj["flags"], adj["nbr_start"].astype(np.int64)
    edge = (flags & BOUNDARY) != 0
    along = edge & (boundary == CURVE)
    row = np.repeat(np.arange(len(x)), np.diff(start))
    keep = ~along[row] | (adj["nbr_boundary"] != 0)
    m = np.zeros_like(x)
    count = _ordered_add(m, start, x[adj["nbr"]], keep)
    move = ((flags & USED) != 0) & ~(edge & (boundary == FIXED)) & (count > 0)
    y = x.copy()
    c = count[move].astype(np.float64)[:, None]
    y[move] = x[move] + s * (m[move] / c - x[move])
    return y


def taubin64(x, adj, iters=10, lam=0.5, mu=-0.53, boundary=FIXED):
    for _ in range(iters):
        x = taubin_pass(x, adj, lam, boundary)
        if mu != 0:
            x = taubin_pass(x, adj, mu, boundary)
    return x


def face_frames(x, faces, adj):
    """-> normals (F,3), areas (F,), centroids (F,3); zeros for an invalid face"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = adj["face_valid"] != 0
    normals, areas, cent = np.zeros((len(f), 3)), np.zeros(len(f)), np.zeros((len(f), 3))
    P = x[f[ok]]
    u, w = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    with np.errstate(all="ignore"):
        L = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        normals[ok] = n / L[:, None]
    areas[ok] = 0.5 * L
    cent[ok] = ((P[:, 0] + P[:, 1]) + P[:, 2]) / 3.0
    return normals, areas, cent


def _visits(faces, adj):
    """the faces g a valid face f visits, in its order (corner, then ascending g, g != f) -> (first visit of every face
    (F+1,), g per visit)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    at = np.nonzero(adj["face_valid"])[0]
    fs = adj["face_start"].astype(np.int64)
    cf, cv = np.repeat(at, 3), f[at].reshape(-1)
    lens = fs[cv + 1] - fs[cv]
    total = int(lens.sum())
    vf = np.repeat(cf, lens)
    pos = np.repeat(fs[cv], lens) + (np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens))
    vg = adj["vert_face"].astype(np.int64)[pos]
    vf, vg = vf[vg != vf], vg[vg != vf]
    return np.searchsorted(vf, np.arange(len(f) + 1)), vf, vg


def normal_filter(normals, areas, cent, faces, adj, iters, rs, rn):
    start, vf, vg = _visits(faces, adj)
    ok = adj["face_valid"] != 0
    d = cent[vg] - cent[vf]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    a = 1.0 - d2 / (rs * rs)
    n = normals
    for _ in range(iters):
        q = n[vf] - n[vg]
        with np.errstate(all="ignore"):
            q2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
            b = 1.0 - q2 / (rn * rn)
            keep = (a > 0) & (b > 0)
            w = (areas[vg] * (a * a)) * (b * b)
            terms = w[:, None] * n[vg]
            s = areas[:, None] * n
            _ordered_add(s, start, terms, keep)
            Ls = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
            new = ok & np.isfinite(Ls) & (Ls > 0)
            out = n.copy()
            out[new] = s[new] / Ls[new, None]
        n = out
    return n


def vertex_update(x, normals, faces, adj, iters, boundary):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    flags, start = adj["flags"], adj["face_start"].astype(np.int64)
    vf = adj["vert_face"].astype(np.int64)
    row = np.repeat(np.arange(len(x)), np.diff(start))
    move = ((flags & USED) != 0) & ~(((flags & BOUNDARY) != 0) & (boundary == FIXED))
    nn = normals[vf]
    for _ in range(iters):
        P = x[f[vf]]
        with np.errstate(all="ignore"):
            d = ((P[:, 0] + P[:, 1]) + P[:, 2]) / 3.0 - x[row]
            t = (nn[:, 0] * d[:, 0] + nn[:, 1] * d[:, 1]) + nn[:, 2] * d[:, 2]
            acc = np.zeros_like(x)
            count = _ordered_add(acc, start, nn * t[:, None])
            y = x.copy()
            go = move & (count > 0)
            y[go] = x[go] + acc[go] / count[go].astype(np.float64)[:, None]
        x = y
    return x


def _widen(verts):
    return np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)


def taubin(verts, faces, iters=10, lam=0.5, mu=-0.53, boundary="fixed"):
    """-> (V,3) float32"""
    return taubin64(_widen(verts), adjacency(verts, faces), iters, lam, mu, MODES[boundary]).astype(np.float32)


def mean_edge(verts, faces):
    v, f = _widen(verts), np.asarray(faces, np.int64).reshape(-1, 3)
    tri = v[f[((f >= 0) & (f < len(v))).all(1)]]
    tri = tri[np.isfinite(tri).all((1, 2))]
    return float(np.mean([np.linalg.norm(tri[:, a] - tri[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))]))


def denoise(verts, faces, normal_iters=5, vertex_iters=10, rn=0.6, rs=None, boundary="fixed"):
    """-> (V,3) float32"""
    x, adj = _widen(verts), adjacency(verts, faces)
    rs = 2.0 * mean_edge(verts, faces) if rs is None else rs
    normals, areas, cent = face_frames(x, faces, adj)
    normals = normal_filter(normals, areas, cent, faces, adj, normal_iters, rs, rn)
    return vertex_update(x, normals, faces, adj, vertex_iters, MODES[boundary]).astype(np.float32)


# ---- measures ------------------------------------------------------------------------------------------------------------
def volume(verts, faces):
    P = _widen(verts)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", P[:, 0], np.cross(P[:, 1], P[:, 2])).sum() / 6.0)


def unit_normals(verts, faces):
    P = _widen(verts)[np.asarray(faces, np.int64)]
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def mean_angle(verts, faces, clean_verts):
    """the mean angle in degrees between the face normals and those of the clean mesh"""
    c = np.einsum("ij,ij->i", unit_normals(verts, faces), unit_normals(clean_verts, faces))
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))).mean())


# ---- meshes --------------------------------------------------------------------------------------------------------------
def icosphere(level=3):
    """(V,3) float32 on the unit sphere, (F,3) int32, outward: 642 vertices and 1280 faces at level 3"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def cube(n=8):
    """the surface of [-1,1]^3, n x n quads per side cut along one diagonal, outward: 386 vertices and 768 faces at n = 8"""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append([2.0 * c / n - 1.0 for c in p])
        return index[p]
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def at(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        return vid(tuple(p))
                    q = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]
                    if side == 0:
                        q = q[::-1]
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)


def patch(n=8):
    """an open n x n planar patch over [0,1]^2 at z = 0: 32 boundary vertices and 32 boundary edges at n = 8"""
    g = np.arange(n + 1) / n
    verts = np.stack([np.repeat(g, n + 1), np.tile(g, n + 1), np.zeros((n + 1) ** 2)], 1)
    faces = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            faces += [(a, b, c), (a, c, d)]
    return verts.astype(np.float32), np.asarray(faces, np.int32)


def bipyramid(n):
    """a ring of n vertices and two apexes of valence n: closed, 2 n faces"""
    ang = 2 * np.pi * np.arange(n) / n
    verts = np.concatenate([np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(3 * ang)], 1), [[0, 0, 1.0], [0, 0, -1.0]]])
    i, j = np.arange(n), (np.arange(n) + 1) % n
    faces = np.concatenate([np.stack([i, j, np.full(n, n)], 1), np.stack([j, i, np.full(n, n + 1)], 1)])
    return verts.astype(np.float32), faces.astype(np.int32)


def fin():
    """three faces on the edge {0, 1}, each with a further face: a non-manifold edge between open sheets"""
    verts = [[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [-0.5, 0.9, 0.5], [-0.5, -0.9, 0.5], [1, 0.1, 1.5], [-0.6, 0.9, 1.5], [-0.6, -0.9, 1.5]]
    faces = [[0, 1, 2], [0, 1, 3], [0, 1, 4], [1, 5, 2], [1, 6, 3], [1, 7, 4]]
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)


def noisy(verts, faces, amount, seed, axes=(0, 1, 2)):
    """Gaussian noise of `amount` mean edges on the coordinates `axes`, seeded -> float32.  (The open patch gets noise along z
    alone: noise in the plane would widen the x-y extent the boundary tests measure, and removing it would count as shrinking.)"""
    rng = np.random.default_rng(seed)
    noise = rng.normal(0.0, amount * mean_edge(verts, faces), np.shape(verts))
    out = np.asarray(verts, np.float64).copy()
    out[:, list(axes)] += noise[:, list(axes)]
    return out.astype(np.float32)


def bad_input():
    """the level-2 icosphere with vertices that are not finite or unused, and faces with bad indices, NaN corners or no area
    -> (verts, faces, the number of clean vertices)"""
    v, f = icosphere(2)
    n = len(v)
    bad_v = np.concatenate([v, [[np.nan, 0, 0], [np.inf, 0, 0], [0.5, 0.5, 0.5], [0, -np.inf, np.nan]]]).astype(np.float32)
    bad_f = np.concatenate([[[0, 1, n]], f[:100], [[0, n + 1, 2], [0, 1, n + 4], [-1, 0, 1], [5, 5, 9], [0, 0, 0], [2 ** 31 - 1, 0, 1],
                                                   [-2 ** 31, 0, 1], [n + 3, 1, 2]], f[100:], [[3, 4, n + 9]]]).astype(np.int32)
    return bad_v, bad_f, n


SMALL = {
    "triangle": ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]]),
    "two_triangles": ([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.3]], [[0, 1, 2], [2, 1, 3]]),
    "tetrahedron": ([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]),
    "three_on_an_edge": ([[0, 0, 0], [0, 0, 1], [1, 0, 0], [-1, 1, 0], [-1, -1, 0]], [[0, 1, 2], [0, 1, 3], [0, 1, 4]]),
    "face_twice": ([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], [[0, 1, 2], [2, 1, 3], [0, 1, 2]]),
    "unused_vertex": ([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], [[0, 1, 2]]),
    "bad_faces": ([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [2, 0, 0]], [[0, 1, 2], [0, 1, 5], [0, 1, 3], [0, 1, 4], [-1, 0, 1], [1, 1, 2]]),
    "no_valid_face": ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 1], [0, 1, 7]]),      # every sorted key is the sentinel
}


def small(name):
    v, f = SMALL[name]
    return np.asarray(v, np.float32), np.asarray(f, np.int32).reshape(-1, 3)


EMPTY = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
