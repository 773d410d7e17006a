"""Float64 numpy restatements of svs_hip.meshtexture for the tests (include/svolsdf_hip.h, the section on a texture atlas baked
from a scan's photographs): slots and rotations, the layout, the per-texel barycentrics, the bake with its `fragile` texels,
the conversion to codes with its vertex-colour branch, and the renderer with its fragile pixels.  numpy only; every
expression is written in the order the header gives, so that float64 without contraction gives the same bits on both sides.

The gather.  A texel's point and normal are float64 combinations that no float32 holds; `bake` hands them to
`meshpaint_oracle.gather`, the one restatement of the device's gather, which `meshpaint_oracle.paint` calls on widened
float32 vertices.  tests/test_meshtexture_cpu.py checks that widening: on points that float32 holds, `gather` returns `paint`'s
accumulators and fragile flags bit for bit; tests/test_paint_gather_golden.py holds both to what they returned as two loops."""
import numpy as np

from meshpaint_oracle import _near_int, agreement, codes, gather
from meshview_oracle import _edges, project_points

MIN_CELL = 6


# ---- slots, layout ---------------------------------------------------------------------------------------------------------
def valid_faces(verts, faces):
    """the face rule of csrc/svs_mesh_face.h -> valid (F,) bool, corners (F,3,3) float64 (zeros where an index is out of range)"""
    p = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((faces >= 0) & (faces < len(p))).all(1)
    P = np.zeros((len(faces), 3, 3))
    if inside.any():
        P[inside] = p[faces[inside]]
    with np.errstate(all="ignore"):
        u, w = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        L = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        valid = inside & np.isfinite(P).all((1, 2)) & np.isfinite(L) & (L > 0)
    return valid, P


def slots(verts, faces):
    """svs_mesh_atlas_slots -> chart (F,) int32, counts [valid, not valid]"""
    valid, P = valid_faces(verts, faces)
    with np.errstate(all="ignore"):
        d = []
        for k in range(3):
            e = P[:, (k + 2) % 3] - P[:, (k + 1) % 3]
            d.append(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        d = np.stack(d, 1)
        r = np.zeros(len(P), np.int64)
        r = np.where(d[:, 1] > d[np.arange(len(P)), r], 1, r)
        r = np.where(d[:, 2] > d[np.arange(len(P)), r], 2, r)
    slot = np.cumsum(valid) - valid
    chart = np.where(valid, slot * 4 + r, -1).astype(np.int32)
    return chart, [int(valid.sum()), int((~valid).sum())]


def corners(h, c):
    """chart corners A_0, A_1, A_2 of half h in a cell of c texels, local texel coordinates -> (3,2) ints (x, y)"""
    return np.array([[1, 1], [c - 4, 1], [1, c - 4]] if h == 0 else [[c - 2, c - 2], [2, c - 2], [c - 2, 2]], np.int64)


def owner(i, j, c):
    """the half that local texel (i, j) belongs to"""
    return np.where(np.asarray(i) + np.asarray(j) <= c - 2, 0, 1)


def check_layout(n_slots, S, c):
    if c < MIN_CELL or S < c or 2 * (S // c) ** 2 < n_slots:
        raise ValueError(f"{n_slots} charts, an atlas of {S}, cells of {c}")


def corner_texels(chart, S, c):
    """-> T (F,3,2) int64: the atlas texel (x, y) of every face corner (zeros for chart -1)"""
    chart = np.asarray(chart, np.int64)
    n = S // c
    T = np.zeros((len(chart), 3, 2), np.int64)
    for f in np.nonzero(chart >= 0)[0]:
        slot, r = chart[f] >> 2, chart[f] & 3
        q, h = slot >> 1, slot & 1
        A = corners(h, c)
        for k in range(3):
            T[f, (r + k) % 3] = [(q % n) * c + A[k, 0], (q // n) * c + A[k, 1]]
    return T


def layout(chart, S, c):
    """svs_mesh_atlas_uv -> uv (F,3,2) float32, slot_face (n_slots,) int32"""
    chart = np.asarray(chart, np.int64)
    n_slots = int((chart >= 0).sum())
    check_layout(n_slots, S, c)
    T = corner_texels(chart, S, c).astype(np.float64)
    uv = np.stack([(T[..., 0] + 0.5) / float(S), 1.0 - (T[..., 1] + 0.5) / float(S)], -1)
    uv[chart < 0] = 0.0
    slot_face = np.zeros(n_slots, np.int32)
    slot_face[chart[chart >= 0] >> 2] = np.nonzero(chart >= 0)[0]
    return uv.astype(np.float32), slot_face


def rows_of(n_slots, S, c):
    """ceil(ceil(n_slots / 2) / n) c: the rows that hold charts"""
    n = S // c
    return ((n_slots + 1) // 2 + n - 1) // n * c


def texels(faces, n_verts, chart, slot_face, S, c):
    """per texel of the rows that hold charts -> has (rows,S) bool, idx (rows,S,3) int64: the vertices at A_0, A_1, A_2 (face
    corners r, r+1, r+2), b (rows,S,3): the clamped barycentrics"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    chart, slot_face = np.asarray(chart, np.int64), np.asarray(slot_face, np.int64)
    n_slots, n = len(slot_face), S // c
    rows = rows_of(n_slots, S, c)
    j, i = np.meshgrid(np.arange(rows), np.arange(S), indexing="ij")
    qx, qy = i // c, j // c
    li, lj = i - qx * c, j - qy * c
    h = owner(li, lj, c)
    slot = 2 * (qy * n + qx) + h
    has = (i < n * c) & (slot < n_slots)
    f = slot_face[np.where(has, slot, 0)] if n_slots else np.zeros_like(slot)
    has &= (f >= 0) & (f < len(faces))
    f = np.where(has, f, 0)
    ch = chart[f] if len(chart) else np.full_like(f, -1)
    has &= ch >= 0
    r = np.where(has, ch & 3, 0)
    tri = faces[f] if len(faces) else np.zeros(f.shape + (3,), np.int64)
    has &= ((tri >= 0) & (tri < n_verts)).all(-1)
    idx = np.stack([np.take_along_axis(tri, ((r + k) % 3)[..., None], -1)[..., 0] for k in range(3)], -1)
    idx = np.where(has[..., None], idx, 0)
    lo = h == 0
    b1 = np.where(lo, (li - 1).astype(np.float64) / float(c - 5), ((c - 2) - li).astype(np.float64) / float(c - 4))
    b2 = np.where(lo, (lj - 1).astype(np.float64) / float(c - 5), ((c - 2) - lj).astype(np.float64) / float(c - 4))
    b0 = 1.0 - b1 - b2
    b0, b1, b2 = np.maximum(b0, 0.0), np.maximum(b1, 0.0), np.maximum(b2, 0.0)
    s = b0 + b1 + b2
    return has, idx, np.stack([b0 / s, b1 / s, b2 / s], -1)


# ---- bake, finish ------------------------------------------------------------------------------------------------------------
def bake(verts, normals, faces, chart, slot_face, S, c, views, depth, images, masks=None, **rules):
    """svs_mesh_atlas_bake over all views in index order.  normals: (V,3) float32 as the device gets them, or None; depth:
    (n_views,H,W) float32.  -> acc (rows,S,4) float64 (zeros where nothing is touched), fragile (rows,S) bool"""
    p = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    has, idx, b = texels(faces, len(p), chart, slot_face, S, c)
    rows = has.shape[0]
    acc, fragile = np.zeros((rows, S, 4)), np.zeros((rows, S), bool)
    at = np.nonzero(has)
    if not len(at[0]):
        return acc, fragile
    idx, b = idx[at], b[at]
    with np.errstate(all="ignore"):
        pts = b[:, 0:1] * p[idx[:, 0]] + b[:, 1:2] * p[idx[:, 1]] + b[:, 2:3] * p[idx[:, 2]]
        nrm, lit = None, None
        if normals is not None:
            m = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
            m = b[:, 0:1] * m[idx[:, 0]] + b[:, 1:2] * m[idx[:, 1]] + b[:, 2:3] * m[idx[:, 2]]
            L = np.sqrt(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1] + m[:, 2] * m[:, 2])
            lit = np.isfinite(m).all(1) & (L > 0) & np.isfinite(L)
            nrm = m / L[:, None]
    got, frag = gather(pts, nrm, lit, views, depth, images, masks, **rules)
    acc[at], fragile[at] = got, frag
    return acc, fragile


def finish(acc, faces, n_verts, chart, slot_face, S, c, vert_rgb=None, mode="blend", fill=(128, 128, 128)):
    """svs_mesh_atlas_finish -> atlas (S,S,3) uint8, covered (S,S) uint8; acc None: every texel takes the vertex-colour branch"""
    has, idx, b = texels(faces, n_verts, chart, slot_face, S, c)
    rows = has.shape[0]
    atlas = np.tile(np.asarray(fill, np.uint8), (S, S, 1))
    covered = np.zeros((S, S), np.uint8)
    acc = np.zeros((rows, S, 4)) if acc is None else np.asarray(acc, np.float64)
    seen = has & (acc[..., 3] > 0)
    atlas[:rows][seen] = codes(acc, mode)[seen]
    covered[:rows][seen] = 1
    if vert_rgb is not None:
        col = np.asarray(vert_rgb, np.uint8).astype(np.float64).reshape(-1, 3)
        rest = has & ~seen
        mix = b[..., 0:1] * col[idx[..., 0]] + b[..., 1:2] * col[idx[..., 1]] + b[..., 2:3] * col[idx[..., 2]]
        mix = np.clip(np.floor(mix + 0.5), 0, 255).astype(np.uint8)
        atlas[:rows][rest] = mix[rest]
        covered[:rows][rest] = 2
    return atlas, covered


# ---- render ----------------------------------------------------------------------------------------------------------------
def render(face, verts, faces, chart, views, atlas, c, fill=(255, 255, 255), face_base=0):
    """svs_mesh_atlas_render -> rgb (n,H,W,3) uint8 (`fill` where nothing is drawn), fragile (n,H,W) bool: a pixel where an
    atlas coordinate is within 1e-9 of an integer (the tap floor; the clamp bounds are integers too) or is not finite, or a
    channel within 1e-9 of a rounding boundary"""
    p = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    chart = np.asarray(chart, np.int64)
    tex = np.asarray(atlas, np.uint8).astype(np.float64)
    S = tex.shape[0]
    face = np.asarray(face, np.int64)
    n, H, W = face.shape
    rgb = np.tile(np.asarray(fill, np.uint8), (n, H, W, 1))
    fragile = np.zeros((n, H, W), bool)
    if not len(faces) or not len(p):
        return rgb, fragile
    T = corner_texels(chart, S, c).astype(np.float64)
    iy, ix = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for v, view in enumerate(views):
        cam, x, y, _ = project_points(p, view["K"], view["E"], 0.0)
        local = face[v] - face_base
        own = (face[v] >= 0) & (local >= 0) & (local < len(faces))
        local = np.where(own, local, 0)
        own &= chart[local] >= 0
        tri = faces[local]
        own &= ((tri >= 0) & (tri < len(p))).all(-1)
        tri = np.where(own[..., None], tri, 0)
        xs, ys, zs = [x[tri[..., k]] for k in range(3)], [y[tri[..., k]] for k in range(3)], [cam[2][tri[..., k]] for k in range(3)]
        with np.errstate(all="ignore"):
            A = (xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0])
            e = _edges(xs, ys, ix, iy)
            b = [e[k] / A for k in range(3)]
            zc = 1.0 / (b[0] / zs[0] + b[1] / zs[1] + b[2] / zs[2])
            wk = [b[k] / zs[k] * zc for k in range(3)]
            X = wk[0] * T[local, 0, 0] + wk[1] * T[local, 1, 0] + wk[2] * T[local, 2, 0]
            Y = wk[0] * T[local, 0, 1] + wk[1] * T[local, 1, 1] + wk[2] * T[local, 2, 1]
            frag = _near_int(X) | _near_int(Y) | ~np.isfinite(X) | ~np.isfinite(Y)      # the clamp bounds are integers too
            X = np.where(X >= 0.0, X, 0.0); X = np.where(X > S - 1.0, S - 1.0, X)
            Y = np.where(Y >= 0.0, Y, 0.0); Y = np.where(Y > S - 1.0, S - 1.0, Y)
        x0, y0 = np.floor(X), np.floor(Y)
        fx, fy = (X - x0)[..., None], (Y - y0)[..., None]
        ix0, iy0 = x0.astype(np.int64), y0.astype(np.int64)
        ix1, iy1 = np.minimum(ix0 + 1, S - 1), np.minimum(iy0 + 1, S - 1)
        col = ((1.0 - fx) * tex[iy0, ix0] + fx * tex[iy0, ix1]) * (1.0 - fy) + ((1.0 - fx) * tex[iy1, ix0] + fx * tex[iy1, ix1]) * fy
        frag |= _near_int(col + 0.5).any(-1)
        code = np.clip(np.floor(col + 0.5), 0, 255).astype(np.uint8)
        rgb[v][own] = code[own]
        fragile[v] = own & frag
    return rgb, fragile


def score(rgb, face, chart, images, masks=None):
    """svs_hip.meshtexture.score -> dict(n, mad, psnr)"""
    chart = np.asarray(chart, np.int64)
    face = np.asarray(face, np.int64)
    at = (face >= 0) & (face < len(chart))
    at &= chart[np.clip(face, 0, max(len(chart) - 1, 0))] >= 0 if len(chart) else False
    for v in range(len(face)):
        if masks is not None and masks[v] is not None:
            at[v] &= np.asarray(masks[v]) != 0
    return agreement(np.asarray(rgb, np.uint8)[at].astype(np.float64) - np.stack([np.asarray(im, np.uint8) for im in images])[at].astype(np.float64))
