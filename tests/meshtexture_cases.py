"""The cases tests/test_meshtexture_cpu.py and tests/test_gpu_meshtexture.py share: the scene of test_gpu_meshpaint.py with its
photographs, the table of bake cases, and the patterned scene of the held-out comparison.  numpy only; everything is computed
once and cached."""
import numpy as np

import meshtexture_oracle as mt
import meshview_oracle as mv

H, W = 48, 64
_CACHE = {}

# the list of tests/test_gpu_meshpaint.py (test_gpu_meshtexture.py checks that the two are the same)
RULES = [dict(), dict(mode="best"), dict(use_normals=False), dict(use_normals=False, mode="best"), dict(one_sided=True),
         dict(one_sided=True, mode="best", power=1), dict(power=0), dict(power=0, mode="best"), dict(cos_min=0.5, power=8),
         dict(cos_min=0.0, power=3), dict(cos_min=1.0)]


def scene(n_lat=12, n_lon=24):
    key = ("scene", n_lat, n_lon)
    if key not in _CACHE:
        verts, faces = mv.scene(n_lat, n_lon)
        chart, counts = mt.slots(verts, faces)
        _CACHE[key] = dict(verts=verts, faces=faces, colors=mv.vertex_colors(len(verts)), chart=chart, n_valid=counts[0])
    return _CACHE[key]


def atlas_size(n_valid, cell):
    """the smallest atlas of whole cells that holds n_valid charts, and an unused margin of 2 texels"""
    n = 1
    while 2 * n * n < n_valid:
        n += 1
    return n * cell + 2


def _key(views, h, w):
    return (np.stack([np.concatenate([v["K"].ravel(), v["E"].ravel()]) for v in views]).tobytes(), h, w)


def rastered(s, views, h=H, w=W):
    """the oracle's depth (n,h,w) float32 and face (n,h,w) int32 maps of the scene, once per set of cameras"""
    key = ("raster", len(s["verts"])) + _key(views, h, w)
    if key not in _CACHE:
        zbuf, _ = mv.raster(s["verts"], s["faces"], views, h, w)
        depth, face, _, shade = mv.resolve(zbuf, s["verts"], s["faces"], views, colors=s.get("colors"))
        _CACHE[key] = dict(depth=depth, face=face, shade=shade)
    return _CACHE[key]


def photographs(s, views, h=H, w=W):
    """photographs of the scene in its vertex colours, drawn by the meshview oracle (test_gpu_meshpaint.py's `_rendered`)"""
    return list(rastered(s, views, h, w)["shade"])


def masks_for(n_views, seed=11):
    rng = np.random.default_rng(seed)
    return [None if v == 1 else (rng.random((H, W)) > 0.3).astype(np.uint8) for v in range(n_views)]


def _name(c):
    rules = "-".join(f"{k}={v}" for k, v in c["rules"].items()) or "defaults"
    return f"{c['n_views']}views-c{c['cell']}-{rules}" + ("-masked" if c["masked"] else "")


def _table():
    out = [dict(n_views=n, seed=3, rules={}, masked=False, cell=16) for n in (1, 3, 16, 17)]
    out += [dict(n_views=3, seed=0, rules=r, masked=m, cell=16) for r in RULES for m in (False, True)]
    out += [dict(n_views=3, seed=0, rules=r, masked=m, cell=6) for r in (RULES[0], RULES[1], RULES[2]) for m in (False, True)]
    for c in out:
        c["name"] = _name(c)
    return out


BAKE_CASES = _table()


def case_inputs(c):
    """-> dict(s, views, images, masks, size, cell, rules, mode)"""
    s = scene()
    views = mv.cameras(c["n_views"], seed=c["seed"])
    return dict(s=s, views=views, images=photographs(s, views), masks=masks_for(c["n_views"]) if c["masked"] else None,
                size=atlas_size(s["n_valid"], c["cell"]), cell=c["cell"], rules=dict(c["rules"]), mode=c["rules"].get("mode", "blend"))


# ---- the patterned scene: what a texture is for ------------------------------------------------------------------------------
WAVES = ((0.12, (1.0, 0.3, 0.2)), (0.13, (-0.2, 1.0, 0.4)), (0.14, (0.3, -0.4, 1.0)))   # wavelength, direction per channel
BACKGROUND = 128


def pattern(p):
    """an analytic pattern of the surface point p (...,3) -> codes (...,3) uint8; its period is a few pixels of the 48 x 64
    views (a pixel spans about 0.03 at the scene's distance) and under a face of the 12 x 24 sphere (about 0.16)"""
    out = []
    for lam, d in WAVES:
        d = np.asarray(d) / np.linalg.norm(d)
        out.append(127.5 + 100.0 * np.sin(2.0 * np.pi * (p @ d) / lam))
    return np.clip(np.floor(np.stack(out, -1) + 0.5), 0, 255).astype(np.uint8)


def surface_points(face, verts, faces, view):
    """the world point under every pixel centre of one view: the perspective-correct combination of the winner's corners"""
    p = np.asarray(verts, np.float32).astype(np.float64)
    cam, x, y, _ = mv.project_points(p, view["K"], view["E"], 0.0)
    tri = np.asarray(faces, np.int64)[np.maximum(face, 0)]
    h, w = face.shape
    iy, ix = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    xs, ys, zs = [x[tri[..., k]] for k in range(3)], [y[tri[..., k]] for k in range(3)], [cam[2][tri[..., k]] for k in range(3)]
    with np.errstate(all="ignore"):
        A = (xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0])
        e = mv._edges(xs, ys, ix, iy)
        b = [e[k] / A for k in range(3)]
        zc = 1.0 / (b[0] / zs[0] + b[1] / zs[1] + b[2] / zs[2])
        return sum((b[k] / zs[k] * zc)[..., None] * p[tri[..., k]] for k in range(3))


def pattern_scene():
    """`scene(12, 24)` photographed per pixel in the pattern: four views bake, two are held out.
    -> dict(verts, faces, colors (the pattern at the vertices), bake / held: dict(views, images, masks, depth, face))"""
    if "pattern" not in _CACHE:
        s = scene()
        views = mv.cameras(6, seed=7)
        r = rastered(s, views)
        images, masks = [], []
        for v, view in enumerate(views):
            seen = r["face"][v] >= 0
            img = np.full((H, W, 3), BACKGROUND, np.uint8)
            img[seen] = pattern(surface_points(r["face"][v], s["verts"], s["faces"], view)[seen])
            images.append(img)
            masks.append(seen.astype(np.uint8))
        part = lambda a, b: dict(views=views[a:b], images=images[a:b], masks=masks[a:b], depth=r["depth"][a:b], face=r["face"][a:b])
        _CACHE["pattern"] = dict(verts=s["verts"], faces=s["faces"], chart=s["chart"], n_valid=s["n_valid"],
                                 colors=pattern(s["verts"].astype(np.float64)), bake=part(0, 4), held=part(4, 6))
    return _CACHE["pattern"]
