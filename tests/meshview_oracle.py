"""Float64 numpy restatements of svs_hip.meshview for the tests (include/svolsdf_hip.h, the section on a mesh seen from a
scan's cameras): the rasteriser with its `fragile` pixels, the resolve step, the vertex visibility with its fragile
vertices, the cull rule, and the two-sphere scene the tests share.  numpy only; every expression is written in the order
the header gives, so that float64 without contraction gives the same bits on both sides."""
import numpy as np

from tsdf_oracle import look_at

FRAGILE = 1e-9
CLOSE = 2.0 ** -21                   # two covering depths this close (relative) may round to one float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def project(verts, K, E, near):
    """`project_points` of the vertices as the device has them: float32, widened"""
    return project_points(np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3), K, E, near)


def project_points(p, K, E, near):
    """float64 points p (N,3) -> cam (3 arrays), x, y, ok: cam = E (p,1), pix = K cam, x = pix.x / pix.z, y = pix.y / pix.z; ok:
    z > near and z, x, y finite"""
    K, E = np.asarray(K, np.float64), np.asarray(E, np.float64)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        cam = [E[r, 0] * px + E[r, 1] * py + E[r, 2] * pz + E[r, 3] for r in range(3)]
        q = [K[r, 0] * cam[0] + K[r, 1] * cam[1] + K[r, 2] * cam[2] for r in range(3)]
        x, y = q[0] / q[2], q[1] / q[2]
        ok = (cam[2] > near) & np.isfinite(cam[2]) & np.isfinite(x) & np.isfinite(y)
    return cam, x, y, ok


def _edges(xs, ys, cx, cy):
    """e_k(c) = (x_q-x_p)(c.y-y_p) - (y_q-y_p)(c.x-x_p), (p,q) = (k+1,k+2) mod 3"""
    return [(xs[(k + 2) % 3] - xs[(k + 1) % 3]) * (cy - ys[(k + 1) % 3]) - (ys[(k + 2) % 3] - ys[(k + 1) % 3]) * (cx - xs[(k + 1) % 3])
            for k in range(3)]


def _face_setup(verts, faces, K, E, near):
    """rules 1-3 -> (ids of the faces drawn, xs, ys, zs: three arrays each over those faces, A)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n_verts = len(np.asarray(verts).reshape(-1, 3))
    cam, x, y, ok = project(verts, K, E, near)
    valid = ((faces >= 0) & (faces < n_verts)).all(1)
    fs = np.where(valid[:, None], faces, 0)
    valid &= ok[fs].all(1) if n_verts else False
    ids = np.nonzero(valid)[0]
    f = faces[ids]
    xs, ys, zs = [x[f[:, k]] for k in range(3)], [y[f[:, k]] for k in range(3)], [cam[2][f[:, k]] for k in range(3)]
    with np.errstate(all="ignore"):
        A = (xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0])
    keep = np.isfinite(A) & (A != 0)
    return ids[keep], [a[keep] for a in xs], [a[keep] for a in ys], [a[keep] for a in zs], A[keep]


def _box(xs, ys, H, W, margin=0.0):
    """rules 4-5: ceil(min) .. floor(max), clamped in float64 -> lx, hx, ly, hy as int64 (an empty box has lx > hx or ly > hy)"""
    lx = np.maximum(np.ceil(np.minimum(xs[0], np.minimum(xs[1], xs[2])) - margin), 0.0)
    hx = np.minimum(np.floor(np.maximum(xs[0], np.maximum(xs[1], xs[2])) + margin), W - 1.0)
    ly = np.maximum(np.ceil(np.minimum(ys[0], np.minimum(ys[1], ys[2])) - margin), 0.0)
    hy = np.minimum(np.floor(np.maximum(ys[0], np.maximum(ys[1], ys[2])) + margin), H - 1.0)
    empty = (lx > hx) | (ly > hy)
    lx, hx, ly, hy = (np.where(empty, 0.0, a).astype(np.int64) for a in (lx, hx, ly, hy))
    hx = np.where(empty, -1, hx)
    return lx, hx, ly, hy


def box_pixels(verts, faces, K, E, H, W, near=1e-6):
    """pixels of every face's clamped box (0 for a face that is skipped): what decides the rasteriser's path"""
    ids, xs, ys, zs, A = _face_setup(verts, faces, K, E, near)
    lx, hx, ly, hy = _box(xs, ys, H, W)
    out = np.zeros(len(np.asarray(faces).reshape(-1, 3)), np.int64)
    out[ids] = np.maximum(hx - lx + 1, 0) * np.maximum(hy - ly + 1, 0)
    return out


def raster_view(zbuf, verts, faces, K, E, near=1e-6, face_base=0):
    """One view of svs_mesh_raster: folds the faces into zbuf (H,W) uint64 in place -> fragile (H,W) bool: pixels where, for
    a face whose box holds them (the box taken 1e-9 wider), some |e_k| <= 1e-9 max(1, |A|) while the other edges do not
    exclude them, or where the two smallest covering float64 depths of this call differ by at most 2**-21 relative"""
    H, W = zbuf.shape
    fragile = np.zeros((H, W), bool)
    ids, xs, ys, zs, A = _face_setup(verts, faces, K, E, near)
    lx, hx, ly, hy = _box(xs, ys, H, W, FRAGILE)
    tx = _box(xs, ys, H, W)
    bw = hx - lx + 1
    n = np.maximum(bw, 0) * np.maximum(hy - ly + 1, 0)
    if n.sum() == 0:
        return fragile
    fi = np.repeat(np.arange(len(n)), n)
    off = np.arange(int(n.sum())) - (np.cumsum(n) - n)[fi]
    ix, iy = lx[fi] + off % bw[fi], ly[fi] + off // bw[fi]
    inbox = (ix >= tx[0][fi]) & (ix <= tx[1][fi]) & (iy >= tx[2][fi]) & (iy <= tx[3][fi])
    fx, fy, fz, fA = [a[fi] for a in xs], [a[fi] for a in ys], [a[fi] for a in zs], A[fi]
    e = _edges(fx, fy, ix.astype(np.float64), iy.astype(np.float64))
    pos = fA > 0
    cov = inbox & np.where(pos, (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0), (e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
    s = np.where(pos, 1.0, -1.0)
    tol = FRAGILE * np.maximum(1.0, np.abs(fA))
    near_edge = ((np.abs(e[0]) <= tol) | (np.abs(e[1]) <= tol) | (np.abs(e[2]) <= tol)) & \
                (s * e[0] >= -tol) & (s * e[1] >= -tol) & (s * e[2] >= -tol)
    fragile[iy[near_edge], ix[near_edge]] = True
    with np.errstate(all="ignore"):
        b = [e[k] / fA for k in range(3)]
        zc = 1.0 / (b[0] / fz[0] + b[1] / fz[1] + b[2] / fz[2])
        zf = zc.astype(np.float32)
        cov &= (zf > 0) & np.isfinite(zf)
    ix, iy, zc, zf, fid = ix[cov], iy[cov], zc[cov], zf[cov], ids[fi[cov]]
    key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (fid + face_base).astype(np.uint64)
    np.minimum.at(zbuf, (iy, ix), key)
    # the two smallest covering depths per pixel
    pix = iy * W + ix
    order = np.lexsort((zc, pix))
    pix, zc = pix[order], zc[order]
    pair = np.nonzero(pix[1:] == pix[:-1])[0]
    first = pair[np.concatenate([[True], pix[pair[1:]] != pix[pair[:-1]]])] if len(pair) else pair
    close = (zc[first + 1] - zc[first]) <= zc[first] * CLOSE
    fragile.reshape(-1)[pix[first[close]]] = True
    return fragile


def raster(verts, faces, views, H, W, near=1e-6, face_base=0, zbuf=None):
    """svs_mesh_raster over views (dicts of K, E) -> zbuf (n_views,H,W) uint64 (a given one is folded into), fragile"""
    if zbuf is None:
        zbuf = np.full((len(views), H, W), EMPTY, np.uint64)
    fragile = np.zeros((len(views), H, W), bool)
    for v, view in enumerate(views):
        fragile[v] = raster_view(zbuf[v], verts, faces, view["K"], view["E"], near, face_base)
    return zbuf, fragile


def resolve(zbuf, verts, faces, views, face_base=0, colors=None):
    """svs_mesh_raster_resolve -> depth (n,H,W) float32, face (n,H,W) int32, normal (n,H,W,3) float64 (not rounded), shade
    (n,H,W,3) uint8.  Ids outside [face_base, face_base + n_faces) keep normal 0 and shade 0 here (the device leaves them)."""
    n, H, W = zbuf.shape
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    empty = zbuf == EMPTY
    depth = np.where(empty, np.uint32(0), (zbuf >> np.uint64(32)).astype(np.uint32)).view(np.float32)
    face = np.where(empty, -1, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    normal = np.zeros((n, H, W, 3))
    shade = np.zeros((n, H, W, 3), np.uint8)
    shade[empty] = 255
    iy, ix = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for v, view in enumerate(views):
        cam, x, y, _ = project(verts, view["K"], view["E"], 0.0)
        local = face[v].astype(np.int64) - face_base
        own = ~empty[v] & (local >= 0) & (local < len(faces))
        f = np.clip(faces[np.where(own, local, 0)], 0, len(cam[0]) - 1)          # (H,W,3); a winner's indices are valid
        P = [[cam[a][f[..., k]] for a in range(3)] for k in range(3)]
        u = [P[1][a] - P[0][a] for a in range(3)]
        w = [P[2][a] - P[0][a] for a in range(3)]
        nrm = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
        with np.errstate(all="ignore"):
            length = np.sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2])
            unit = (length > 0) & np.isfinite(length)
            nrm = [np.where(unit, c / length, 0.0) for c in nrm]
        flip = nrm[2] > 0
        nrm = np.stack([np.where(flip, -c, c) for c in nrm], -1)
        normal[v][own] = nrm[own]
        g = 0.2 + 0.8 * np.abs(nrm[..., 2])
        col = np.ones((H, W, 3))
        if colors is not None:
            c = np.asarray(colors, np.uint8).astype(np.float64) / 255.0
            xs, ys, zs = [x[f[..., k]] for k in range(3)], [y[f[..., k]] for k in range(3)], [cam[2][f[..., k]] for k in range(3)]
            with np.errstate(all="ignore"):
                A = (xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0])
                e = _edges(xs, ys, ix, iy)
                b = [e[k] / A for k in range(3)]
                zc = 1.0 / (b[0] / zs[0] + b[1] / zs[1] + b[2] / zs[2])
                wk = [b[k] / zs[k] * zc for k in range(3)]
                col = wk[0][..., None] * c[f[..., 0]] + wk[1][..., None] * c[f[..., 1]] + wk[2][..., None] * c[f[..., 2]]
        with np.errstate(all="ignore"):
            code = np.floor(255.0 * (g[..., None] * col) + 0.5)
        code = np.clip(np.where(np.isnan(code), 0.0, code), 0, 255).astype(np.uint8)
        shade[v][own] = code[own]
    return depth, face, normal, shade


def visibility(verts, views, depth, masks=None, rel=0.01, abs_tol=0.0, near=1e-6, fragile_pixels=None):
    """svs_mesh_vertex_visibility over all views -> seen (V,) int32, off_mask (V,) int32, fragile (V,) bool: vertices where
    x + 0.5 or y + 0.5 is within 1e-9 of an integer, |z - (d (1 + rel) + abs_tol)| <= 1e-9 z, or whose pixel is fragile"""
    n_verts = len(np.asarray(verts).reshape(-1, 3))
    seen, off = np.zeros(n_verts, np.int32), np.zeros(n_verts, np.int32)
    fragile = np.zeros(n_verts, bool)
    for v, view in enumerate(views):
        d32 = np.asarray(depth[v], np.float32)
        H, W = d32.shape
        cam, x, y, ok = project(verts, view["K"], view["E"], near)
        z = cam[2]
        with np.errstate(all="ignore"):
            u, w = x + 0.5, y + 0.5
            fu, fv = np.floor(u), np.floor(w)
            ok = ok & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            fragile |= ok & ((np.abs(u - np.rint(u)) <= FRAGILE) | (np.abs(w - np.rint(w)) <= FRAGILE))
        iu, iv = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
        masked = np.zeros(n_verts, bool)
        if masks is not None and masks[v] is not None:
            masked = ok & (np.asarray(masks[v])[iv, iu] == 0)
        off += masked
        d = d32[iv, iu].astype(np.float64)
        lim = d * (1.0 + rel) + abs_tol
        live = ok & ~masked
        with np.errstate(all="ignore"):
            seen += live & ((d == 0) | (z <= lim))
            fragile |= live & (d != 0) & (np.abs(z - lim) <= FRAGILE * z)
        if fragile_pixels is not None:
            fragile |= live & np.asarray(fragile_pixels[v])[iv, iu]
    return seen, off, fragile


def cull(verts, faces, seen, off_mask=None, min_views=1, max_off_mask=None, mode="all", colors=None):
    """a vertex survives iff seen >= min_views and (with max_off_mask) off_mask <= max_off_mask; a face iff all of its
    vertices do ("any": one of them); the unused vertices dropped -> verts, faces[, colors], kept faces (F,) bool"""
    verts, faces = np.asarray(verts), np.asarray(faces, np.int64).reshape(-1, 3)
    alive = np.asarray(seen) >= min_views
    if max_off_mask is not None:
        alive &= np.asarray(off_mask) <= max_off_mask
    keep = alive[faces].all(1) if mode == "all" else alive[faces].any(1)
    used = np.zeros(len(verts), bool)
    used[faces[keep].reshape(-1)] = True
    remap = np.cumsum(used) - 1
    out = (verts[used], remap[faces[keep]])
    if colors is not None:
        out += (np.asarray(colors)[used],)
    return out + (keep,)


# ---- the scene -------------------------------------------------------------------------------------------------------
SCENE_K = np.array([[70.0, 0, 31.3], [0, 70.0, 23.6], [0, 0, 1]], np.float64)
SCENE_EYES = ((2.2, 0.3, 0.9), (-0.4, 2.1, 1.1), (-1.6, -1.5, 0.7))
BIG_CENTRE, BIG_RADIUS = np.array([0.013, -0.021, 0.007]), 0.6
SMALL_CENTRE, SMALL_RADIUS = np.array([0.55, 0.35, 0.3]), 0.25
FLOOR_Z = -0.62


def uv_sphere(n_lat, n_lon, radius, centre):
    """a latitude-longitude sphere: (n_lat + 1) rings of n_lon vertices (the poles repeated), 2 n_lat n_lon faces, the
    degenerate ones at the poles included"""
    th = np.pi * np.arange(n_lat + 1) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    v = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(n_lon))], -1)
    i, j = np.meshgrid(np.arange(n_lat), np.arange(n_lon), indexing="ij")
    a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
    c, d = a + n_lon, b + n_lon
    f = np.stack([np.stack([a, c, b], -1), np.stack([b, c, d], -1)], 2).reshape(-1, 3)
    return radius * v.reshape(-1, 3) + np.asarray(centre, np.float64), f


def scene(n_lat, n_lon):
    """the two spheres, the two-triangle floor and one triangle with a vertex behind every camera -> verts (V,3) float32,
    faces (F,3) int32; the floor is faces F-3 and F-2, the triangle behind the cameras F-1"""
    v1, f1 = uv_sphere(n_lat, n_lon, BIG_RADIUS, BIG_CENTRE)
    v2, f2 = uv_sphere(max(4, n_lat // 2), max(6, n_lon // 2), SMALL_RADIUS, SMALL_CENTRE)
    extra = np.array([[-1.5, -1.5, FLOOR_Z], [1.5, -1.5, FLOOR_Z], [1.5, 1.5, FLOOR_Z], [-1.5, 1.5, FLOOR_Z],
                      [0.1, 0.2, -5.0], [0.3, 0.1, 9.0], [0.2, 0.4, 9.0]])
    fe = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]])
    verts = np.concatenate([v1, v2, extra]).astype(np.float32)
    faces = np.concatenate([f1, f2 + len(v1), fe + len(v1) + len(v2)]).astype(np.int32)
    return verts, faces


def cameras(n_views=3, seed=0, zoom=1.0):
    """the scene's three cameras, then perturbed copies of them -> dicts of K, E.  zoom: K's first two rows scaled (an image
    that many times as large)"""
    rng = np.random.default_rng(seed)
    eyes = [np.asarray(SCENE_EYES[i % 3]) + (0.0 if i < 3 else 1.0) * rng.uniform(-0.15, 0.15, 3) for i in range(n_views)]
    return [dict(K=np.diag([zoom, zoom, 1.0]) @ SCENE_K, E=look_at(tuple(e))) for e in eyes]


def vertex_colors(n_verts, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n_verts, 3)).astype(np.uint8)


# ---- the exact case ----------------------------------------------------------------------------------------------------
# a square at z = 2 in front of a camera at the origin; pixel = 4 X + 4: the square covers pixels 2..6 in x and y, its
# diagonal runs through the pixel centres (2,2) .. (6,6); every figure is dyadic, so every operation is exact
EXACT_K = np.array([[8.0, 0, 4.0], [0, 8.0, 4.0], [0, 0, 1]])
EXACT_VERTS = np.array([[-0.5, -0.5, 2], [0.5, -0.5, 2], [0.5, 0.5, 2], [-0.5, 0.5, 2]], np.float32)
EXACT_FACES = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def exact_case_expectation():
    """-> depth, face (9,9) of the square drawn with face_base 5"""
    depth, face = np.zeros((9, 9), np.float32), np.full((9, 9), -1, np.int32)
    iy, ix = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    inside = (ix >= 2) & (ix <= 6) & (iy >= 2) & (iy <= 6)
    depth[inside] = 2.0
    face[inside & (iy <= ix)] = 5                            # face 0 holds the corner (6,2): x >= y, the diagonal included
    face[inside & (iy > ix)] = 6
    return depth, face
