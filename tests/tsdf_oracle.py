"""Float64 numpy restatements of svs_hip.tsdf for the tests (include/svolsdf_hip.h, the TSDF section): the integration with
its `fragile` mask, the face rule, the vertex colours, and the sphere scene the tests share.  numpy only."""
import numpy as np

from svs_hip import mc_table

FRAGILE = 1e-9


def integrate(tsdf, weight, rgb, origin, voxel, trunc, views):
    """One launch.  tsdf, weight (n0,n1,n2), rgb (3,n0,n1,n2) or None: float64 copies of the stored float32 values.
    views: dicts of K (3,3), E (4,4), depth (H,W) [, mask (H,W), img (H,W,3)].
    -> tsdf, weight, rgb (float64, NOT rounded: the caller rounds where it stores), fragile (n0,n1,n2) bool: voxels where a
    view has u or v within 1e-9 of an integer, z within 1e-9 of 0, or sdf + trunc within 1e-9 * trunc of 0 -- a decision
    that float64 noise in the camera arithmetic may take either way."""
    tsdf, weight = np.array(tsdf, np.float64), np.array(weight, np.float64)
    rgb = None if rgb is None else np.array(rgb, np.float64)
    shape = tsdf.shape
    origin = np.asarray(origin, np.float64)
    idx = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    p = origin + idx * float(voxel)
    n_vox = len(p)
    st, sn = np.zeros(n_vox), np.zeros(n_vox)
    sc = np.zeros((n_vox, 3))
    fragile = np.zeros(n_vox, bool)
    for view in views:
        K, E = np.asarray(view["K"], np.float64), np.asarray(view["E"], np.float64)
        depth = np.asarray(view["depth"], np.float32)
        H, W = depth.shape
        cam = p @ E[:3, :3].T + E[:3, 3]
        z = cam[:, 2]
        fragile |= np.abs(z) <= FRAGILE
        ok = z > 0
        pix = cam @ K.T
        with np.errstate(all="ignore"):
            u, v = pix[:, 0] / pix[:, 2] + 0.5, pix[:, 1] / pix[:, 2] + 0.5
        fin = ok & np.isfinite(u) & np.isfinite(v)
        fragile[fin] |= (np.abs(u[fin] - np.rint(u[fin])) <= FRAGILE) | (np.abs(v[fin] - np.rint(v[fin])) <= FRAGILE)
        fu, fv = np.floor(u), np.floor(v)
        ok = fin & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        iu, iv = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
        d = depth[iv, iu]
        if view.get("mask") is not None:
            ok &= np.asarray(view["mask"])[iv, iu] != 0
        with np.errstate(all="ignore"):
            ok &= np.isfinite(d) & (d > 0)
        d = np.where(ok, d, 1.0).astype(np.float64)
        sdf = d - z
        fragile |= ok & (np.abs(sdf + trunc) <= FRAGILE * trunc)
        ok &= ~(sdf < -trunc)
        t = np.minimum(1.0, sdf / trunc)
        st += np.where(ok, t, 0.0)
        sn += ok
        if rgb is not None:
            img = np.asarray(view["img"], np.float32).astype(np.float64)
            sc += np.where(ok[:, None], img[iv, iu], 0.0)
    seen = (sn > 0).reshape(shape)
    st, sn = st.reshape(shape), sn.reshape(shape)
    w_new = weight + sn
    with np.errstate(all="ignore"):
        tsdf = np.where(seen, (weight * tsdf + st) / w_new, tsdf)
        if rgb is not None:
            sc = np.moveaxis(sc.reshape(shape + (3,)), -1, 0)
            rgb = np.where(seen[None], (weight[None] * rgb + sc) / w_new[None], rgb)
    return tsdf, np.where(seen, w_new, weight), rgb, fragile.reshape(shape)


def integrate_f32(shape, origin, voxel, trunc, launches, colors=True):
    """The volume after `launches` (a list of view lists), stored as float32 between them as the device stores it.
    -> tsdf, weight, rgb (float32), fragile (any launch)"""
    tsdf, weight = np.ones(shape, np.float32), np.zeros(shape, np.float32)
    rgb = np.zeros((3,) + tuple(shape), np.float32) if colors else None
    fragile = np.zeros(shape, bool)
    for views in launches:
        t, w, c, fr = integrate(tsdf, weight, rgb, origin, voxel, trunc, views)
        tsdf, weight = t.astype(np.float32), w.astype(np.float32)
        rgb = None if c is None else c.astype(np.float32)
        fragile |= fr
    return tsdf, weight, rgb, fragile


def _cell_corners(weight, cells):
    n0, n1, n2 = weight.shape
    i, j, k = np.unravel_index(np.asarray(cells, np.int64), (n0, n1, n2))
    return [(i + a, j + b, k + c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]


def face_keep(weight, cells, min_weight):
    """keep (F,) bool: all eight nodes of the face's cell have weight >= min_weight"""
    weight = np.asarray(weight)
    keep = np.ones(len(cells), bool)
    for at in _cell_corners(weight, cells):
        keep &= weight[at] >= min_weight
    return keep


def vertex_colors(rgb, weight, verts):
    """verts (V,3) in index units -> (V,3) float64: trilinear over the observed nodes (weight > 0) around the vertex, base
    index clamped to [0, n-2], normalised by the sum of their trilinear weights, 0 where that sum is 0"""
    rgb, weight = np.asarray(rgb, np.float64), np.asarray(weight)
    x = np.asarray(verts, np.float64)
    n = np.asarray(weight.shape)
    base = np.clip(np.floor(x), 0, n - 2)
    f = x - base
    b = base.astype(np.int64)
    acc, wsum = np.zeros((len(x), 3)), np.zeros(len(x))
    for c in range(8):
        d = np.array([c >> 2, (c >> 1) & 1, c & 1])
        at = tuple((b + d).T)
        w = np.prod(np.where(d, f, 1.0 - f), 1) * (weight[at] > 0)
        wsum += w
        acc += w[:, None] * rgb[(slice(None),) + at].T
    with np.errstate(all="ignore"):
        return np.where(wsum[:, None] != 0, acc / wsum[:, None], 0.0)


def mc_cells(vol, level):
    """per face of mesh_oracle.marching_cubes(vol, level), the node index of its cell (faces come by cell, then table order)"""
    vol = np.asarray(vol, np.float64)
    n0, n1, n2 = vol.shape
    inside = vol < level
    case = np.zeros((n0 - 1, n1 - 1, n2 - 1), np.int64)
    for c in range(8):
        o = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
        case |= inside[o[0]:n0 - 1 + o[0], o[1]:n1 - 1 + o[1], o[2]:n2 - 1 + o[2]].astype(np.int64) << c
    i, j, k = np.nonzero((case != 0) & (case != 255))
    n_tri = np.asarray([len(mc_table.TRIANGLES[c]) for c in case[i, j, k]], np.int64)
    return np.repeat((i * n1 + j) * n2 + k, n_tri)


def compact(verts, faces):
    """drops the vertices no face uses -> verts, faces re-indexed, used (V,) bool"""
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return verts[used], remap[faces], used


def colors_u8(c):
    return np.clip(np.floor(np.asarray(c, np.float64) * 255.0 + 0.5), 0, 255).astype(np.uint8)


# ---- the sphere scene ------------------------------------------------------------------------------------------------
SPHERE_K = np.array([[61.3, 0, 31.7], [0, 60.9, 23.4], [0, 0, 1]], np.float64)
SPHERE_CENTRE = np.array([0.07, -0.04, 0.11])
SPHERE_RADIUS = 0.5
SPHERE_EYES = ((2.03, 0.31, 0.42), (-0.87, 1.79, 0.55), (-0.93, -1.71, -0.38))


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """world-to-camera E (4,4): +z looks at the target, +x right, +y down"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    E = np.eye(4)
    E[:3, :3] = np.stack([right, down, fwd])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def sphere_depth(K, E, H, W, centre=SPHERE_CENTRE, radius=SPHERE_RADIUS):
    """camera-z of the first hit of every pixel centre's ray with the sphere, 0 on a miss -> (H,W) float32"""
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T        # camera frame, z = 1
    c = E[:3, :3] @ np.asarray(centre, np.float64) + E[:3, 3]
    a = (rays * rays).sum(-1)
    b = rays @ c
    disc = b * b - a * (c @ c - radius * radius)
    s = (b - np.sqrt(np.maximum(disc, 0.0))) / a
    return np.where((disc > 0) & (s > 0), s, 0.0).astype(np.float32)


def sphere_image(K, E, depth):
    """a smooth colour per pixel in [0,1]: the world position of the hit, scaled; grey on a miss -> (H,W,3) float32"""
    H, W = depth.shape
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    cam = (np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T) * depth[..., None].astype(np.float64)
    world = (cam - E[:3, 3]) @ E[:3, :3]
    img = np.clip(0.5 + 0.8 * (world - SPHERE_CENTRE), 0.0, 1.0)
    img[depth <= 0] = 0.25
    return img.astype(np.float32)


def sphere_scene(shape=(33, 35, 67), voxel=0.05, H=48, W=64, eyes=SPHERE_EYES):
    """-> dict(views=[dict(K, E, depth, img)], origin (3,), shape, voxel, trunc = 3 * voxel, centre, radius)"""
    views = []
    for eye in eyes:
        E = look_at(eye)
        depth = sphere_depth(SPHERE_K, E, H, W)
        views.append(dict(K=SPHERE_K.copy(), E=E, depth=depth, img=sphere_image(SPHERE_K, E, depth)))
    origin = -voxel * (np.asarray(shape, np.float64) - 1) / 2 + np.array([0.003, -0.002, 0.001])
    return dict(views=views, origin=origin, shape=tuple(shape), voxel=float(voxel), trunc=3.0 * voxel,
                centre=SPHERE_CENTRE, radius=SPHERE_RADIUS)
