"""Float64 numpy restatements of svs_hip.meshpaint for the tests (include/svolsdf_hip.h, the section on a mesh painted from a
scan's photographs): the vertex normals, the paint accumulation with its `fragile` vertices, the conversion to codes, the
hole filling and the photo-consistency score.  numpy only; every expression is written in the order the header gives, so
that float64 without contraction gives the same bits on both sides."""
import numpy as np

from meshview_oracle import FRAGILE, project_points

DEGENERATE = 1e-6                    # |sum| < this * sum of |cross|: a normal that cancellation decides


def vertex_normals(verts, faces):
    """svs_mesh_vertex_normals -> normals (V,3) float64 (not rounded to float32), accum (V,3), fragile (V,) bool: vertices
    whose |sum| < 1e-6 * the sum of their |cross| (the order of the device's atomic adds shows there)"""
    p = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n_verts = len(p)
    accum, total = np.zeros((n_verts, 3)), np.zeros(n_verts)
    valid = ((faces >= 0) & (faces < n_verts)).all(1)
    f = faces[valid]
    f = f[np.isfinite(p[f]).all((1, 2))] if len(f) else f
    if len(f):
        u, w = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
        with np.errstate(all="ignore"):
            cross = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                              u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
            size = np.sqrt((cross * cross).sum(1))
            for k in range(3):
                np.add.at(accum, f[:, k], cross)
                np.add.at(total, f[:, k], size)
    with np.errstate(all="ignore"):
        length = np.sqrt(accum[:, 0] * accum[:, 0] + accum[:, 1] * accum[:, 1] + accum[:, 2] * accum[:, 2])
        unit = np.isfinite(accum).all(1) & (length > 0) & np.isfinite(length)
        normals = np.where(unit[:, None], accum / length[:, None], 0.0)
        fragile = (total > 0) & ~(length >= DEGENERATE * total)
    return normals, accum, fragile


def _near_int(a):
    return np.abs(a - np.rint(a)) <= FRAGILE


def paint(verts, normals, views, depth, images, masks=None, **rules):
    """svs_mesh_paint over all views in index order (what several calls of at most 16 views accumulate): `gather` on the
    vertices and normals (V,3) as the device gets them, float32 widened (normals None: every view weighs 1); a vertex whose
    normal is zero or not finite is not lit.  -> acc (V,4) float64, fragile (V,) bool"""
    n, lit = None, None
    if normals is not None:
        n = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
        lit = np.isfinite(n).all(1) & ~(n == 0).all(1)
    return gather(np.asarray(verts, np.float32).astype(np.float64), n, lit, views, depth, images, masks, **rules)


def gather(p, n, lit, views, depth, images, masks=None, mode="blend", cos_min=0.1, power=2, one_sided=False, rel=0.01,
           abs_tol=0.0, near=1e-6, acc=None):
    """Steps 1 to 7 of svs_mesh_paint for float64 points p (N,3) with float64 normals n (N,3) or None and lit (N,) bool or
    None (a point that is not lit is skipped in every view), the one restatement of csrc/svs_paint_gather.h: `paint` calls
    it per vertex, `meshtexture_oracle.bake` per texel.  depth: (n_views,H,W) float32; images: per view (H,W,3) uint8; masks:
    None or per view None / (H,W); acc: what earlier calls left.  -> acc (N,4) float64, fragile (N,) bool: a point where, in
    some view, z is within 1e-9 of near, x or y within 1e-9 of the image bounds, x + 0.5 or y + 0.5 within 1e-9 of an
    integer, |z - (d (1 + rel) + abs_tol)| <= 1e-9 z, or c within 1e-9 of cos_min; in best mode where the two largest weights
    are within 1e-9 relative (an exact tie of weights that are 1 by construction is not fragile: the earlier view wins it);
    and where a channel's mean is within 1e-9 of a rounding boundary."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    n_verts = len(p)
    acc = np.zeros((n_verts, 4)) if acc is None else np.array(acc, np.float64)
    fragile = np.zeros(n_verts, bool)
    best = mode == "best"
    lit = np.ones(n_verts, bool) if lit is None else np.asarray(lit, bool)
    top = np.stack([acc[:, 3], np.zeros(n_verts)], 1)          # the two largest weights met so far
    for v, view in enumerate(views):
        d32 = np.asarray(depth[v], np.float32)
        img = np.asarray(images[v], np.uint8).astype(np.float64)
        H, W = d32.shape
        cam, x, y, ok = project_points(p, view["K"], view["E"], near)
        z = cam[2]
        with np.errstate(all="ignore"):
            fragile |= lit & np.isfinite(z) & (np.abs(z - near) <= FRAGILE)
            ok = ok & lit
            inside = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
            fragile |= ok & ((np.abs(x) <= FRAGILE) | (np.abs(x - (W - 1)) <= FRAGILE)) & (y >= -FRAGILE) & (y <= H - 1 + FRAGILE)
            fragile |= ok & ((np.abs(y) <= FRAGILE) | (np.abs(y - (H - 1)) <= FRAGILE)) & (x >= -FRAGILE) & (x <= W - 1 + FRAGILE)
            ok = ok & inside
            fragile |= ok & (_near_int(x + 0.5) | _near_int(y + 0.5))
        xs, ys = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
        iu, iv = np.floor(xs + 0.5).astype(np.int64), np.floor(ys + 0.5).astype(np.int64)
        if masks is not None and masks[v] is not None:
            ok = ok & (np.asarray(masks[v])[iv, iu] != 0)
        d = d32[iv, iu].astype(np.float64)
        lim = d * (1.0 + rel) + abs_tol
        with np.errstate(all="ignore"):
            fragile |= ok & (d != 0) & (np.abs(z - lim) <= FRAGILE * z)
            ok = ok & ((d == 0) | (z <= lim))
        w = np.ones(n_verts)
        if n is not None:
            E = np.asarray(view["E"], np.float64)
            eye = [-(E[0, k] * E[0, 3] + E[1, k] * E[1, 3] + E[2, k] * E[2, 3]) for k in range(3)]
            t = [eye[k] - p[:, k] for k in range(3)]
            with np.errstate(all="ignore"):
                c = (n[:, 0] * t[0] + n[:, 1] * t[1] + n[:, 2] * t[2]) / np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
                if not one_sided:
                    c = np.abs(c)
                fragile |= ok & (np.abs(c - cos_min) <= FRAGILE)
                ok = ok & (c >= cos_min)
                for _ in range(int(power)):
                    w = w * c
        x0, y0 = np.floor(xs), np.floor(ys)
        fx, fy = xs - x0, ys - y0
        ix0, iy0 = x0.astype(np.int64), y0.astype(np.int64)
        ix1, iy1 = np.minimum(ix0 + 1, W - 1), np.minimum(iy0 + 1, H - 1)
        col = ((1.0 - fx)[:, None] * img[iy0, ix0] + fx[:, None] * img[iy0, ix1]) * (1.0 - fy)[:, None] + \
              ((1.0 - fx)[:, None] * img[iy1, ix0] + fx[:, None] * img[iy1, ix1]) * fy[:, None]
        if best:
            take = ok & (w > acc[:, 3])
            acc[take, :3] = col[take]
            acc[take, 3] = w[take]
            both = np.sort(np.stack([top[:, 0], top[:, 1], np.where(ok, w, 0.0)], 1), 1)[:, ::-1]
            top = both[:, :2]
        else:
            acc[ok, :3] = acc[ok, :3] + w[ok, None] * col[ok]
            acc[ok, 3] = acc[ok, 3] + w[ok]
    if best:
        by_construction = n is None or int(power) == 0
        close = (top[:, 1] > 0) & (top[:, 0] - top[:, 1] <= FRAGILE * top[:, 0])
        if by_construction:
            close &= top[:, 0] != top[:, 1]
        fragile |= close
    seen = acc[:, 3] > 0
    with np.errstate(all="ignore"):
        mean = acc[:, :3] if best else acc[:, :3] / acc[:, 3:4]
        fragile |= seen & _near_int(mean + 0.5).any(1)
    return acc, fragile


def codes(acc, mode="blend"):
    """accumulators (...,4) -> codes (...,3) uint8: the rule both finish kernels share (meaningless where acc.w is 0)"""
    with np.errstate(all="ignore"):
        mean = acc[..., :3] if mode == "best" else acc[..., :3] / acc[..., 3:4]
        code = np.floor(mean + 0.5)
    return np.clip(np.where(np.isnan(code), 0.0, code), 0, 255).astype(np.uint8)


def agreement(diff):
    """differences (n,3) float64, channels pooled -> dict(n, mad, psnr); NaN for n = 0"""
    if not len(diff):
        return dict(n=0, mad=float("nan"), psnr=float("nan"))
    mse = float((diff * diff).mean())
    return dict(n=len(diff), mad=float(np.abs(diff).mean()), psnr=float("inf") if mse == 0 else float(10.0 * np.log10(255.0 ** 2 / mse)))


def finish(acc, mode="blend", fill=(128, 128, 128)):
    """svs_mesh_paint_finish -> rgb (V,3) uint8, painted (V,) int32"""
    acc = np.asarray(acc, np.float64)
    rgb = np.tile(np.asarray(fill, np.uint8), (len(acc), 1))
    seen = acc[:, 3] > 0
    rgb[seen] = codes(acc, mode)[seen]
    return rgb, seen.astype(np.int32)


def spread_round(faces, n_verts, round, rgb, painted):
    """one call of svs_mesh_paint_spread on copies -> rgb, painted, changed (bool)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    rgb, painted = np.array(rgb, np.uint8), np.array(painted, np.int32)
    work = np.zeros((n_verts, 4), np.int64)
    f = faces[((faces >= 0) & (faces < n_verts)).all(1)]
    for i in range(3):
        for j in range(3):
            if i == j:
                continue
            a, b = f[:, i], f[:, j]
            go = (painted[a] > 0) & (painted[a] <= round) & (painted[b] == 0)
            np.add.at(work, b[go], np.concatenate([rgb[a[go]].astype(np.int64), np.ones((int(go.sum()), 1), np.int64)], 1))
    got = work[:, 3] > 0
    count = work[got, 3:4]
    rgb[got] = ((2 * work[got, :3] + count) // (2 * count)).astype(np.uint8)
    painted[got] = round + 1
    return rgb, painted, bool(got.any())


def spread(faces, n_verts, rgb, painted, rounds=None):
    """rounds of `spread_round` from round 1, until one changes nothing (rounds=None) or `rounds` have run
    -> rgb, painted, rounds run (rounds=None: those that filled something)"""
    done = 0
    while rounds is None or done < rounds:
        rgb, painted, changed = spread_round(faces, n_verts, 1 + done, rgb, painted)
        if rounds is None and not changed:
            break
        done += 1
    return np.array(rgb, np.uint8), np.array(painted, np.int32), done


def consistency(colors, acc):
    """`colors` (V,3) uint8 against the blend of held-out views in `acc`, over the vertices with acc.w > 0, channels pooled
    -> dict(n, mad, psnr)"""
    acc = np.asarray(acc, np.float64)
    at = acc[:, 3] > 0
    return agreement(np.asarray(colors, np.uint8)[at].astype(np.float64) - acc[at, :3] / acc[at, 3:4])
