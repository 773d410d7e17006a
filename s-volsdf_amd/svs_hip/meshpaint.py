"""A mesh's vertices coloured from a scan's photographs on the HIP path (csrc/svs_meshpaint.hip), and how well a coloured
surface agrees with photographs it was not painted from.

    python -m svs_hip.meshpaint --ply exps_mvs/mesh/scan106.ply --scan-folder exps_mvs/scan106 --views 25 22 28 \\
        --ply-out exps_mvs/mesh/scan106_painted.ply [--holdout 23 24] [--mode best] [--cos-min C --power P --one-sided \\
        --no-normals --rel R --abs-tol T --spread-rounds N --fill R G B] [--data-dir-root D --dataset DTU]

Every view projects into the mesh, the depth maps `meshview.rasterize` draws decide occlusion, views are weighted by the
cosine between the vertex normal and the direction to the camera, vertices no view sees are filled from their neighbours
over the mesh's edges.  `svs_hip.meshview` then renders the file in colour.

OURS throughout: the reference writes its checkpoint mesh without colours and has no such step.  The arithmetic is fixed in
include/svolsdf_hip.h and restated in float64 in tests/meshpaint_oracle.py.  SETTINGS, all choices and none of them tuned:
`mode` (blend: the weighted mean of all views; best: the view with the largest weight), `cos_min` (default 0.1), `power`
(default 2: weight = cos^2), `one_sided` (a normal that points away from the camera does not count), `use_normals`, the
visibility tolerances `rel` (default 0.01) and `abs_tol` of `meshview.visibility`, `near`, `spread_rounds` (default: until
nothing changes), `fill` (the colour of what is never reached).  `svs_hip.meshtexture` takes from here what the two share:
`check_rules`, `view_inputs`, `view_chunks` (not in `svs_hip.views`, which launches nothing), `filled`, `agreement`, and the command
lines' `add_painter_args`, `check_painter_args`, `painter_rules`; both read a scan folder through `views.scan_folder_inputs`.
"""
import argparse
import os
import time
from collections import OrderedDict

import numpy as np
import torch

from . import lib as _lib
from . import meshview as _mv
from . import ply as _ply
from .images import seconds_line, tick, to_device
from .ops import _ptr, _ptr_array, _stream
from .views import (MAX_VIEWS, add_eval_mask_args, check_eval_mask_args, chunks, device_masks, folder_images, launches_since,
                    mesh_args, scan_folder_inputs)

FACE_CHUNK = 1 << 24                 # faces per call of svs_mesh_vertex_normals
ENTRY_CALLS = {"normals": 0, "paint": 0, "finish": 0, "spread": 0}  # C entry points called, not kernels
RULES = dict(cos_min=0.1, power=2, one_sided=False, use_normals=True, rel=0.01, abs_tol=0.0, near=1e-6)


def check_rules(rules, name="svs_mesh_paint"):
    """The caller's rules over RULES and mode="blend", for the painter and for `svs_hip.meshtexture`: TypeError in `name` for a
    rule that is not known, ValueError for a mode or a range that is not allowed -> (the rules without mode, flags)"""
    unknown = sorted(set(rules) - set(RULES) - {"mode"})
    if unknown:
        raise TypeError(f"{name}: unknown rules {unknown} (known: {sorted(list(RULES) + ['mode'])})")
    r = dict(RULES, **rules)
    mode = r.pop("mode", "blend")
    if mode not in ("blend", "best"):
        raise ValueError(f"svs_mesh_paint: mode 'blend' or 'best', got {mode!r}")
    if not (0 <= r["cos_min"] <= 1) or int(r["power"]) != r["power"] or not (0 <= r["power"] <= 8):
        raise ValueError(f"svs_mesh_paint: cos_min in [0,1] and power an integer in [0,8], got {r['cos_min']} and {r['power']}")
    if r["rel"] < 0 or r["abs_tol"] < 0 or not (r["near"] > 0):
        raise ValueError(f"svs_mesh_paint: near must be positive, rel and abs_tol not negative, got {r['near']}, {r['rel']}, {r['abs_tol']}")
    return r, (_lib.PAINT_BEST if mode == "best" else 0) | (_lib.PAINT_ONE_SIDED if r["one_sided"] else 0)


def flags_of(mode="blend", one_sided=False):
    return check_rules(dict(mode=mode, one_sided=one_sided))[1]


def normals_raw(verts, faces, accum, normals):
    """One call of svs_mesh_vertex_normals on device tensors -> its return code"""
    rc = _lib.load().svs_mesh_vertex_normals(_ptr(verts), int(verts.shape[0]), _ptr(faces), int(faces.shape[0]), _ptr(accum),
                                             _ptr(normals), _stream())
    ENTRY_CALLS["normals"] += 1
    return rc


def vertex_normals(verts, faces, chunk=FACE_CHUNK, accum=None):
    """verts (V,3), faces (F,3): arrays or device tensors -> (V,3) float32 device tensor: the area-weighted unit normal of
    every vertex, (0,0,0) where no valid face meets it.  The faces go in chunks of `chunk`; accum: a zeroed (V,3) float64
    device tensor that keeps the unnormalised sums."""
    verts, faces, _ = mesh_args(verts, faces)
    if accum is None:
        accum = torch.zeros((verts.shape[0], 3), dtype=torch.float64, device=verts.device)
    normals = torch.zeros((verts.shape[0], 3), dtype=torch.float32, device=verts.device)
    n_faces = int(faces.shape[0])
    for at in range(0, max(1, n_faces), int(chunk)):
        last = at + int(chunk) >= n_faces
        _lib.check(normals_raw(verts, faces[at:at + int(chunk)], accum, normals if last else None), "svs_mesh_vertex_normals")
    return normals


def paint_raw(verts, normals, mats, n_views, H, W, depth, images, masks, acc, near=1e-6, rel=0.01, abs_tol=0.0, cos_min=0.1,
              power=2, flags=0):
    """One call of svs_mesh_paint on device tensors (images, masks: lists) -> its return code (`accumulate` is the checked form)."""
    rc = _lib.load().svs_mesh_paint(_ptr(verts), int(verts.shape[0]), _ptr(normals), _ptr(mats), int(n_views), int(H), int(W),
                                    float(near), _ptr(depth), _ptr_array(images) if images is not None else None,
                                    _ptr_array(masks) if masks is not None else None, float(rel), float(abs_tol), float(cos_min),
                                    int(power), int(flags), _ptr(acc), _stream())
    ENTRY_CALLS["paint"] += 1
    return rc


def _check_rules(cos_min, power, rel, abs_tol, near):
    check_rules(dict(cos_min=cos_min, power=power, rel=rel, abs_tol=abs_tol, near=near))


def _images(images, n_views):
    out = [to_device(im, torch.uint8, "meshpaint", "image", ndim=(3,), cast=False) for im in images]
    if len(out) != n_views:
        raise ValueError(f"svs_mesh_paint: {len(out)} images for {n_views} views")
    sizes = sorted({tuple(im.shape) for im in out})
    if len(sizes) > 1 or (sizes and sizes[0][2] != 3):
        raise ValueError(f"svs_mesh_paint: the images are (H,W,3) of one size, got {sizes}")
    return out


def view_inputs(name, verts, views, images, masks, depth, normals):
    """What `accumulate` and `meshtexture.bake` are given per view, checked in the name of the entry `name` and on the device
    -> views (a list), images, masks, depth (n_views,H,W) or None, normals (V,3) or None, H, W"""
    views = list(views)
    if not views:
        raise ValueError(f"{name}: no views")
    images = _images(images, len(views))
    H, W = int(images[0].shape[0]), int(images[0].shape[1])
    masks = device_masks(masks, len(views), H, W, verts.device, name)
    if depth is not None:
        depth = to_device(depth, torch.float32, "meshpaint", "depth", ndim=(3,))
        if tuple(depth.shape) != (len(views), H, W):
            raise ValueError(f"{name}: depth maps of {tuple(depth.shape)} for {len(views)} views of {(H, W)}")
    if normals is not None:
        normals = to_device(normals, torch.float32, "meshpaint", "normals")
        if tuple(normals.shape) != tuple(verts.shape):
            raise ValueError(f"{name}: normals of {tuple(normals.shape)} for {verts.shape[0]} vertices")
    return views, images, masks, depth, normals, H, W


def view_chunks(verts, faces, views, H, W, masks, depth, near, timers, phase):
    """yields (at, to, mats, depth maps, masks or None) of views[at:to] per chunk of MAX_VIEWS.  A chunk is rasterised when it is
    asked for (`meshview.rasterize`, unless depth has the maps; ticks "raster"), so the device holds MAX_VIEWS z-buffers at a
    time; what the caller does with it ticks `phase`."""
    t0 = time.perf_counter()
    for at, to, mats in chunks(views, verts.device):
        part = depth[at:to] if depth is not None else _mv.rasterize(verts, faces, views[at:to], H, W, near=near)["depth"]
        t0 = tick(timers, "raster", t0)
        yield at, to, mats, part, masks[at:to] if masks is not None else None
        t0 = tick(timers, phase, t0)


def accumulate(verts, faces, views, images, masks=None, *, normals=None, flags=0, cos_min=0.1, power=2, rel=0.01, abs_tol=0.0,
               near=1e-6, depth=None, seen=None, timers=None):
    """The views painted chunk by chunk (`view_chunks`; depth: (n_views,H,W) when the caller has the maps).  normals: (V,3)
    float32 or None (every view weighs 1).  seen: a zeroed (V,) int32 tensor that gets `meshview.visibility`'s count of the
    views that pass the mask and the depth test.  -> acc (V,4) float64: (r, g, b, w) as svs_mesh_paint leaves them."""
    verts, faces, _ = mesh_args(verts, faces)
    _check_rules(cos_min, power, rel, abs_tol, near)
    views, images, masks, depth, normals, H, W = view_inputs("svs_mesh_paint", verts, views, images, masks, depth, normals)
    acc = torch.zeros((verts.shape[0], 4), dtype=torch.float64, device=verts.device)
    for at, to, mats, part, part_masks in view_chunks(verts, faces, views, H, W, masks, depth, near, timers, "paint"):
        _lib.check(paint_raw(verts, normals, mats, to - at, H, W, part, images[at:to], part_masks, acc, near, rel, abs_tol,
                             cos_min, power, flags), "svs_mesh_paint")
        if seen is not None:
            off = torch.zeros_like(seen)
            _lib.check(_mv.visibility_raw(verts, mats, to - at, H, W, part, part_masks, rel, abs_tol, seen, off, near),
                       "svs_mesh_vertex_visibility")
    return acc


def filled(fill, shape, dev):
    """a uint8 tensor of shape + (3,) on dev that holds the colour `fill` everywhere"""
    return torch.tensor([int(c) for c in fill], dtype=torch.uint8, device=dev).repeat(*shape, 1).contiguous()


def finish(acc, flags=0, fill=(128, 128, 128)):
    """svs_mesh_paint_finish -> colors (V,3) uint8 (`fill` where acc.w is 0), painted (V,) int32 (1 or 0)"""
    n = int(acc.shape[0])
    colors = filled(fill, (n,), acc.device)
    painted = torch.zeros(n, dtype=torch.int32, device=acc.device)
    rc = _lib.load().svs_mesh_paint_finish(_ptr(acc), n, int(flags), _ptr(colors), _ptr(painted), _stream())
    ENTRY_CALLS["finish"] += 1
    _lib.check(rc, "svs_mesh_paint_finish")
    return colors, painted


def spread(faces, colors, painted, rounds=None):
    """Hole filling in place: svs_mesh_paint_spread round after round, until a round fills nothing (rounds=None; the host
    reads one int per round) or `rounds` have run.  -> rounds run (rounds=None: those that filled something)"""
    n_verts, n_faces = int(colors.shape[0]), int(faces.shape[0])
    if n_verts == 0 or n_faces == 0 or rounds == 0:
        return 0
    work = torch.empty((n_verts, 4), dtype=torch.int32, device=colors.device)
    changed = torch.zeros(1, dtype=torch.int32, device=colors.device)
    done = 0
    while rounds is None or done < rounds:
        rc = _lib.load().svs_mesh_paint_spread(_ptr(faces), n_faces, n_verts, 1 + done, _ptr(colors), _ptr(painted),
                                               _ptr(work), _ptr(changed), _stream())
        ENTRY_CALLS["spread"] += 1
        _lib.check(rc, "svs_mesh_paint_spread")
        if rounds is None and int(changed.item()) == 0:
            break
        done += 1
    return done


def paint(verts, faces, views, images, masks=None, *, mode="blend", cos_min=0.1, power=2, one_sided=False, use_normals=True,
          rel=0.01, abs_tol=0.0, near=1e-6, spread_rounds=None, fill=(128, 128, 128), depth=None, stats=None):
    """verts (V,3), faces (F,3): arrays or device tensors; views: dicts of K (3,3), E (4,4); images: per view an (H,W,3)
    uint8 array or tensor, all of one size; masks: None or per view None / an (H,W) array, non-zero = inside; depth: the
    mesh's depth maps (n_views,H,W) when the caller has them.
    -> colors (V,3) uint8, painted (V,) int32 on the device: 1 = painted by a view, r + 1 = filled in round r of the
    hole filling, 0 = never reached (its colour is `fill`).
    stats: a dict that gets acc (V,4) float64, normals, seen (V,) int32 (views that pass the mask and depth test),
    rounds, and seconds per phase (which makes every phase wait for the device)."""
    verts, faces, _ = mesh_args(verts, faces)
    flags = check_rules(dict(mode=mode, cos_min=cos_min, power=power, one_sided=one_sided, rel=rel, abs_tol=abs_tol, near=near))[1]
    timers = None
    if stats is not None:
        timers = stats.setdefault("seconds", OrderedDict())
        for k in ("normals", "raster", "paint", "spread"):
            timers.setdefault(k, 0.0)
    t0 = time.perf_counter()
    normals = vertex_normals(verts, faces) if use_normals else None
    t0 = tick(timers, "normals", t0)
    seen = torch.zeros(verts.shape[0], dtype=torch.int32, device=verts.device) if stats is not None else None
    acc = accumulate(verts, faces, views, images, masks, normals=normals, flags=flags, cos_min=cos_min, power=power, rel=rel,
                     abs_tol=abs_tol, near=near, depth=depth, seen=seen, timers=timers)
    t0 = time.perf_counter()
    colors, painted = finish(acc, flags, fill)
    t0 = tick(timers, "paint", t0)
    rounds = spread(faces, colors, painted, spread_rounds)
    tick(timers, "spread", t0)
    if stats is not None:
        stats.update(acc=acc, normals=normals, seen=seen, rounds=rounds)
    return colors, painted


def consistency(verts, faces, colors, views, images, masks=None, *, cos_min=0.1, power=2, one_sided=False, use_normals=True,
                rel=0.01, abs_tol=0.0, near=1e-6, depth=None):
    """How well `colors` (V,3) uint8 agree with views they were not painted from: those views are blended into fresh
    accumulators by the same rules, and over the vertices they see (acc.w > 0), channels pooled:
    -> dict(n = those vertices, mad = mean |colors - acc.rgb / acc.w| in codes, psnr = 10 log10(255^2 / mean square))"""
    verts, faces, colors = mesh_args(verts, faces, colors)
    if colors is None:
        raise ValueError("svs_mesh_paint: consistency needs colours")
    normals = vertex_normals(verts, faces) if use_normals else None
    acc = accumulate(verts, faces, views, images, masks, normals=normals, flags=flags_of("blend", one_sided), cos_min=cos_min,
                     power=power, rel=rel, abs_tol=abs_tol, near=near, depth=depth)
    at = acc[:, 3] > 0
    return agreement(colors[at].to(torch.float64) - acc[at, :3] / acc[at, 3:4])


def agreement(diff):
    """diff (n,3) float64, channels pooled -> dict(n, mad = mean |diff|, psnr = 10 log10(255^2 / mean square)), NaN for n = 0"""
    if not len(diff):
        return dict(n=0, mad=float("nan"), psnr=float("nan"))
    mse = float((diff * diff).mean())
    return dict(n=len(diff), mad=float(diff.abs().mean()), psnr=float("inf") if mse == 0 else float(10.0 * np.log10(255.0 ** 2 / mse)))


def paint_folder(ply, scan_folder, view_ids, ply_out, holdout=(), *, mode="blend", cos_min=0.1, power=2, one_sided=False,
                 use_normals=True, rel=0.01, abs_tol=0.0, near=1e-6, spread_rounds=None, fill=(128, 128, 128),
                 eval_mask_root=None, dataset=None, eval_mask_radius=12, log=None):
    """Paints the mesh file `ply` from the views of a scan folder (cameras from cams/{id:08}_cam.txt, photographs from
    images/{id:08}.jpg at their own size) and writes it, coloured, to ply_out.  holdout: view ids that are not painted
    from; `consistency` scores the result against them.  With eval_mask_root and dataset the evaluation masks cut the
    photographs, as `meshview.view_folder` takes them (the scan's name is the last component of scan_folder).
    -> colors, painted (device tensors), stats: dict(files, n_verts, n_faces, painted per round ([0]: by a view), unpainted,
    views (histogram of the views that see a vertex), holdout (`consistency`'s dict or None), launches, seconds per phase)."""
    sec = OrderedDict((k, 0.0) for k in ("read", "upload", "normals", "raster", "paint", "spread", "download", "write"))
    calls = dict(ENTRY_CALLS)
    view_ids, holdout = list(view_ids), list(holdout)
    rules = dict(cos_min=cos_min, power=power, one_sided=one_sided, use_normals=use_normals, rel=rel, abs_tol=abs_tol, near=near)
    t0 = time.perf_counter()
    verts, faces, _, views, images, masks, (H, W) = scan_folder_inputs(ply, scan_folder, view_ids + holdout, eval_mask_root, dataset,
                                                                       eval_mask_radius)
    t0 = tick(sec, "read", t0)
    verts_d, faces_d, _ = mesh_args(verts, faces)
    images_d = [to_device(im, torch.uint8, "meshpaint", "image") for im in images]
    t0 = tick(sec, "upload", t0)
    n = len(view_ids)
    stats = dict(seconds=sec)
    colors, painted = paint(verts_d, faces_d, views[:n], images_d[:n], None if masks is None else masks[:n], mode=mode,
                            spread_rounds=spread_rounds, fill=fill, stats=stats, **rules)
    score = None
    if holdout:
        t0 = time.perf_counter()
        score = consistency(verts_d, faces_d, colors, views[n:], images_d[n:], None if masks is None else masks[n:], **rules)
        tick(sec, "paint", t0)
    t0 = time.perf_counter()
    host_c, host_p, host_seen = colors.cpu().numpy(), painted.cpu().numpy(), stats.pop("seen").cpu().numpy()
    t0 = tick(sec, "download", t0)
    os.makedirs(os.path.dirname(ply_out) or ".", exist_ok=True)
    _ply.write(ply_out, verts_d, host_c, faces_d)
    tick(sec, "write", t0)
    for k in ("acc", "normals"):
        stats.pop(k)
    stats.update(files=dict(ply=ply_out), n_verts=len(verts), n_faces=len(faces), painted=np.bincount(host_p)[1:].tolist(),
                 unpainted=int((host_p == 0).sum()), views=np.bincount(host_seen, minlength=n + 1).tolist(), holdout=score,
                 launches=launches_since(ENTRY_CALLS, calls))
    if log is not None:
        log(f"meshpaint: {ply} ({len(verts)} vertices, {len(faces)} faces) from {n} views of {H} x {W}: painted per round "
            + " ".join(map(str, stats["painted"])) + f", {stats['unpainted']} never reached; seen by k views: "
            + " ".join(map(str, stats["views"])) + f" -> {ply_out}")
        if score is not None:
            log(f"held-out views {' '.join(map(str, holdout))}: {score['n']} vertices, mean |difference| {score['mad']:.3f} codes, "
                f"PSNR {score['psnr']:.2f} dB")
        log(seconds_line(sec))
    return colors, painted, stats


def add_painter_args(p, verb, point, holdout_use):
    """the options `svs_hip.meshpaint` and `svs_hip.meshtexture` share: the views and the rules"""
    p.add_argument("--views", type=int, nargs="+", required=True, help=f"view ids to {verb} from, e.g. 25 22 28")
    p.add_argument("--holdout", type=int, nargs="*", default=[], help=f"view ids kept back: {holdout_use}")
    p.add_argument("--mode", default="blend", choices=("blend", "best"), help="the weighted mean of all views, or the best view alone")
    p.add_argument("--cos-min", type=float, default=RULES["cos_min"], help="a view counts from this cosine between normal and viewing direction")
    p.add_argument("--power", type=int, default=RULES["power"], help="weight = cosine ** power, 0..8")
    p.add_argument("--one-sided", action="store_true", help="a normal that points away from the camera does not count")
    p.add_argument("--no-normals", action="store_true", help=f"every view that sees a {point} weighs 1")
    p.add_argument("--rel", type=float, default=RULES["rel"], help="relative depth tolerance of the visibility test")
    p.add_argument("--abs-tol", type=float, default=RULES["abs_tol"], help="absolute depth tolerance of the visibility test")
    p.add_argument("--fill", type=int, nargs=3, default=[128, 128, 128], metavar=("R", "G", "B"), help="the colour of what is never reached")
    add_eval_mask_args(p, "the evaluation masks cut the photographs")


def check_painter_args(p, a, also, also_ok=True):
    """`check_rules`' ranges in the parsers' words; also, also_ok: the module's own options that the second message names"""
    check_eval_mask_args(p, a)
    rest_ok = also_ok and all(0 <= c <= 255 for c in a.fill)
    for names, ok, text in ((("cos_min", "power"), True, "--cos-min lies in [0,1] and --power in [0,8]"),
                            (("rel", "abs_tol"), rest_ok, f"{also} are not negative, --fill holds codes in [0,255]")):
        try:
            check_rules({k: getattr(a, k) for k in names})
        except ValueError:
            ok = False
        if not ok:
            p.error(text)


def painter_rules(a):
    return dict(mode=a.mode, cos_min=a.cos_min, power=a.power, one_sided=a.one_sided, use_normals=not a.no_normals, rel=a.rel,
                abs_tol=a.abs_tol)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Colours a mesh's vertices from a scan's photographs on the GPU and scores the result "
                                            "against held-out views")
    p.add_argument("--ply", required=True, help="the mesh (a PLY with faces; colours it has are ignored)")
    p.add_argument("--scan-folder", required=True, help="holds cams/{id:08}_cam.txt and images/{id:08}.jpg; its last component names the scan")
    p.add_argument("--ply-out", required=True, help="the coloured mesh")
    add_painter_args(p, "paint", "vertex", "the photo-consistency score is taken against them")
    p.add_argument("--spread-rounds", type=int, default=None, help="rounds of hole filling (default: until nothing changes; 0: none)")
    a = p.parse_args(argv)
    check_painter_args(p, a, "--rel, --abs-tol and --spread-rounds", a.spread_rounds is None or a.spread_rounds >= 0)
    if set(a.views) & set(a.holdout):
        p.error("--holdout names views that --views paints from")
    return a


def main(argv=None):
    a = parse_args(argv)
    return paint_folder(a.ply, a.scan_folder, a.views, a.ply_out, a.holdout, spread_rounds=a.spread_rounds, fill=tuple(a.fill),
                        eval_mask_root=a.data_dir_root, dataset=a.dataset, log=print, **painter_rules(a))


if __name__ == "__main__":
    main()
