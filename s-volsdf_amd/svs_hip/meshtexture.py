"""A texture atlas for a mesh, baked from a scan's photographs on the HIP path (csrc/svs_meshtexture.hip), the mesh rendered
through that atlas, and how well the result agrees with photographs it was not baked from.

    python -m svs_hip.meshtexture --ply exps_mvs/tsdf_simple/mvsnet106_l3.ply --scan-folder exps_mvs/scan106 --views 25 22 28 \\
        --obj-out exps_mvs/tsdf_texture/mvsnet106_l3.obj [--size 4096] [--cell C] [--holdout 23 24] [--mode best] \\
        [--cos-min C --power P --one-sided --no-normals --rel R --abs-tol T --fill R G B] [--data-dir-root D --dataset DTU]

One chart per valid face, two charts per square cell of the atlas (`cell_for` picks the largest cell that holds them all);
every texel gathers the photographs exactly as `svs_hip.meshpaint` gathers them per vertex (one device function serves
both); texels no view sees take the interpolated vertex colours.  `svs_hip.obj` writes the OBJ, MTL and PNG.

OURS throughout: the reference has no such step.  The arithmetic is fixed in include/svolsdf_hip.h and restated in float64 in
tests/meshtexture_oracle.py (the gather: tests/meshpaint_oracle.py).  SETTINGS: `size` (the atlas is size x size texels), `cell`
(texels per cell side, >= 6; default: `cell_for`), and the painter's `mode`, `cos_min`, `power`, `one_sided`, `use_normals`, `rel`,
`abs_tol`, `near`, `fill`; its rules record, checked view inputs, loop over launches and command-line options are `svs_hip.meshpaint`'s.
"""
import argparse
import time
from collections import OrderedDict

import torch

from . import lib as _lib
from . import meshpaint as _mp
from . import meshview as _mv
from . import obj as _obj
from .images import seconds_line, tick, to_device
from .ops import _ptr, _ptr_array, _stream
from .views import chunks, launches_since, mesh_args, scan_folder_inputs

MIN_CELL = 6
MAX_SIZE = 32768
ENTRY_CALLS = {"slots": 0, "uv": 0, "bake": 0, "finish": 0, "render": 0}  # C entry points called, not kernels
RULES = dict(_mp.RULES, mode="blend")
LANE_ORDER = "cell"                  # how svs_mesh_atlas_bake's lanes walk the atlas: "cell" (the faster, NOTES/meshtexture.md) or "row"; same bytes


def _rules(rules):
    """`meshpaint.check_rules` -> (rules without mode, flags)"""
    return _mp.check_rules(rules, "svs_mesh_atlas_bake")


def slots(verts, faces):
    """svs_mesh_atlas_slots -> chart (F,) int32 on the device (slot * 4 + rotation, -1 for a face that is not valid), the
    number of valid faces (the host reads four bytes)"""
    verts, faces, _ = mesh_args(verts, faces)
    n_faces = int(faces.shape[0])
    chart = torch.empty(n_faces, dtype=torch.int32, device=verts.device)
    work = torch.empty(n_faces, dtype=torch.uint8, device=verts.device)
    counts = torch.zeros(2, dtype=torch.int32, device=verts.device)
    rc = _lib.load().svs_mesh_atlas_slots(_ptr(verts), int(verts.shape[0]), _ptr(faces), n_faces, _ptr(work), _ptr(chart),
                                          _ptr(counts), _stream())
    ENTRY_CALLS["slots"] += 1
    _lib.check(rc, "svs_mesh_atlas_slots")
    return chart, int(counts[0].item())


def cell_for(n_valid, size):
    """the largest cell side c >= 6 with 2 (size // c)^2 >= n_valid; ValueError naming both numbers when there is none"""
    n_valid, size = int(n_valid), int(size)
    for c in range(size, MIN_CELL - 1, -1):
        if 2 * (size // c) ** 2 >= n_valid:
            return c
    raise ValueError(f"svs_mesh_atlas_uv: {n_valid} charts do not fit an atlas of {size} x {size} texels with cells of {MIN_CELL} "
                     f"({2 * (size // MIN_CELL) ** 2} fit)")


def rows_for(n_slots, size, cell):
    """the atlas rows that hold charts: what svs_mesh_atlas_bake's acc has"""
    n, cells = int(size) // int(cell), (int(n_slots) + 1) // 2
    return (cells + n - 1) // n * int(cell) if n else 0


def layout(chart, n_slots, size, cell):
    """svs_mesh_atlas_uv -> uv (F,3,2) float32 per face corner in the OBJ convention, slot_face (n_slots,) int32"""
    n_faces = int(chart.shape[0])
    uv = torch.zeros((n_faces, 3, 2), dtype=torch.float32, device=chart.device)
    slot_face = torch.full((int(n_slots),), -1, dtype=torch.int32, device=chart.device)
    rc = _lib.load().svs_mesh_atlas_uv(_ptr(chart), n_faces, int(n_slots), int(size), int(cell), _ptr(uv), _ptr(slot_face), _stream())
    ENTRY_CALLS["uv"] += 1
    _lib.check(rc, "svs_mesh_atlas_uv")
    return uv, slot_face


def bake_raw(verts, normals, faces, chart, slot_face, size, cell, mats, n_views, H, W, depth, images, masks, acc, near=1e-6,
             rel=0.01, abs_tol=0.0, cos_min=0.1, power=2, flags=0):
    """One call of svs_mesh_atlas_bake on device tensors (images, masks: lists) -> its return code (`bake` is the checked form)"""
    rc = _lib.load().svs_mesh_atlas_bake(_ptr(verts), int(verts.shape[0]), _ptr(normals), _ptr(faces), int(faces.shape[0]),
                                         _ptr(chart), _ptr(slot_face), int(slot_face.shape[0]), int(size), int(cell), _ptr(mats),
                                         int(n_views), int(H), int(W), float(near), _ptr(depth),
                                         _ptr_array(images) if images is not None else None,
                                         _ptr_array(masks) if masks is not None else None, float(rel), float(abs_tol),
                                         float(cos_min), int(power), int(flags), _ptr(acc), _stream())
    ENTRY_CALLS["bake"] += 1
    return rc


def bake(verts, faces, chart, slot_face, size, cell, views, images, masks=None, *, normals=None, flags=0, cos_min=0.1, power=2,
         rel=0.01, abs_tol=0.0, near=1e-6, depth=None, timers=None, order=None):
    """The views baked chunk by chunk, as `meshpaint.accumulate` paints them (`meshpaint.view_chunks`).  order: "row" or "cell"
    (default: LANE_ORDER).  -> acc (rows,size,4) float64: (r, g, b, w) per texel of the rows that hold charts"""
    verts, faces, _ = mesh_args(verts, faces)
    order = LANE_ORDER if order is None else order
    if order not in ("row", "cell"):
        raise ValueError(f"svs_mesh_atlas_bake: order 'row' or 'cell', got {order!r}")
    flags = int(flags) | (_lib.ATLAS_CELL_MAJOR if order == "cell" else 0)
    _mp._check_rules(cos_min, power, rel, abs_tol, near)
    views, images, masks, depth, normals, H, W = _mp.view_inputs("svs_mesh_atlas_bake", verts, views, images, masks, depth, normals)
    acc = torch.zeros((rows_for(slot_face.shape[0], size, cell), int(size), 4), dtype=torch.float64, device=verts.device)
    for at, to, mats, part, part_masks in _mp.view_chunks(verts, faces, views, H, W, masks, depth, near, timers, "bake"):
        _lib.check(bake_raw(verts, normals, faces, chart, slot_face, size, cell, mats, to - at, H, W, part, images[at:to], part_masks,
                            acc, near, rel, abs_tol, cos_min, power, flags), "svs_mesh_atlas_bake")
    return acc


def finish(acc, faces, n_verts, chart, slot_face, size, cell, vert_colors=None, flags=0, fill=(128, 128, 128)):
    """svs_mesh_atlas_finish -> atlas (size,size,3) uint8 (`fill` where nothing was written), covered (size,size) uint8: 1 =
    baked from a view, 2 = from the vertex colours, 0 = left as filled.  acc None: the vertex-colour atlas"""
    size = int(size)
    atlas = _mp.filled(fill, (size, size), chart.device)
    covered = torch.zeros((size, size), dtype=torch.uint8, device=chart.device)
    if acc is not None and tuple(acc.shape) != (rows_for(slot_face.shape[0], size, cell), size, 4):
        raise ValueError(f"svs_mesh_atlas_finish: acc of {tuple(acc.shape)} for {rows_for(slot_face.shape[0], size, cell)} rows of {size}")
    rc = _lib.load().svs_mesh_atlas_finish(_ptr(acc), _ptr(faces), int(faces.shape[0]), int(n_verts), _ptr(chart), _ptr(slot_face),
                                           int(slot_face.shape[0]), size, int(cell), _ptr(vert_colors), int(flags), _ptr(atlas),
                                           _ptr(covered), _stream())
    ENTRY_CALLS["finish"] += 1
    _lib.check(rc, "svs_mesh_atlas_finish")
    return atlas, covered


def render_raw(face, verts, faces, chart, mats, atlas, cell, rgb, face_base=0):
    """One call of svs_mesh_atlas_render on device tensors -> its return code"""
    n_views, H, W = (int(s) for s in face.shape)
    rc = _lib.load().svs_mesh_atlas_render(_ptr(face), _ptr(verts), int(verts.shape[0]), _ptr(faces), int(faces.shape[0]),
                                           int(face_base), _ptr(chart), _ptr(mats), n_views, H, W, _ptr(atlas), int(atlas.shape[0]),
                                           int(cell), _ptr(rgb), _stream())
    ENTRY_CALLS["render"] += 1
    return rc


def render(verts, faces, chart, atlas, cell, views, H, W, fill=(255, 255, 255), near=1e-6, face=None):
    """The textured mesh seen from `views`: -> rgb (n_views,H,W,3) uint8 (`fill` where no textured face is seen; no shading
    factor: the picture is meant to be compared with photographs), face (n_views,H,W) int32 as `meshview.rasterize` gives it
    (or as given)."""
    verts, faces, _ = mesh_args(verts, faces)
    views = list(views)
    if not views:
        raise ValueError("svs_mesh_atlas_render: no views")
    if face is None:
        face = _mv.rasterize(verts, faces, views, H, W, near=near)["face"]
    rgb = _mp.filled(fill, (len(views), int(H), int(W)), verts.device)
    for at, to, mats in chunks(views, verts.device):
        _lib.check(render_raw(face[at:to], verts, faces, chart, mats, atlas, cell, rgb[at:to]), "svs_mesh_atlas_render")
    return rgb, face


def texture(verts, faces, views, images, masks=None, *, size=4096, cell=None, vert_colors=None, depth=None, stats=None,
            fill=(128, 128, 128), **rules):
    """verts (V,3), faces (F,3): arrays or device tensors; views, images, masks, depth: as `meshpaint.paint` takes them;
    vert_colors: (V,3) uint8 for the texels no view sees (None: they keep `fill`); rules: `meshpaint.RULES` and mode.
    -> dict(atlas (size,size,3) uint8, covered (size,size) uint8, uv (F,3,2) float32, chart (F,) int32, cell) on the device.
    stats: a dict that gets acc, normals, slot_face, n_slots and seconds per phase (which makes every phase wait)."""
    verts, faces, vert_colors = mesh_args(verts, faces, vert_colors)
    r, flags = _rules(rules)
    size = int(size)
    if not (MIN_CELL <= size <= MAX_SIZE):
        raise ValueError(f"svs_mesh_atlas_uv: an atlas of {MIN_CELL} to {MAX_SIZE} texels a side, got {size}")
    timers = None
    if stats is not None:
        timers = stats.setdefault("seconds", OrderedDict())
        for k in ("slots", "normals", "raster", "bake", "finish"):
            timers.setdefault(k, 0.0)
    t0 = time.perf_counter()
    chart, n_slots = slots(verts, faces)
    cell = cell_for(n_slots, size) if cell is None else int(cell)
    uv, slot_face = layout(chart, n_slots, size, cell)
    t0 = tick(timers, "slots", t0)
    r.pop("one_sided")
    normals = _mp.vertex_normals(verts, faces) if r.pop("use_normals") else None
    t0 = tick(timers, "normals", t0)
    acc = bake(verts, faces, chart, slot_face, size, cell, views, images, masks, normals=normals, flags=flags, depth=depth,
               timers=timers, **r)
    t0 = time.perf_counter()
    atlas, covered = finish(acc, faces, verts.shape[0], chart, slot_face, size, cell, vert_colors, flags, fill)
    tick(timers, "finish", t0)
    if stats is not None:
        stats.update(acc=acc, normals=normals, slot_face=slot_face, n_slots=n_slots)
    return dict(atlas=atlas, covered=covered, uv=uv, chart=chart, cell=cell)


def vertex_atlas(faces, n_verts, chart, slot_face, size, cell, vert_colors, fill=(128, 128, 128)):
    """the atlas of the interpolated vertex colours alone: the baseline `consistency` scores a baked atlas against"""
    return finish(None, faces, n_verts, chart, slot_face, size, cell, vert_colors, 0, fill)[0]


def score(rgb, face, chart, images, masks=None):
    """rendered rgb (n,H,W,3) against the photographs over the pixels with a face, a chart and the mask, channels pooled
    -> dict(n = those pixels, mad = mean |difference| in codes, psnr = 10 log10(255^2 / mean square))"""
    photo = torch.stack([to_device(im, torch.uint8, "meshtexture", "image") for im in images])
    at = (face >= 0) & (face < int(chart.shape[0]))
    if chart.numel():
        at &= chart[face.clamp(0, int(chart.shape[0]) - 1).long()] >= 0
    if masks is not None:
        for v, m in enumerate(masks):
            if m is not None:
                at[v] &= torch.as_tensor(m).to(at.device) != 0
    return _mp.agreement(rgb[at].to(torch.float64) - photo[at].to(torch.float64))


def consistency(verts, faces, tex, vert_colors, views, images, masks=None, near=1e-6):
    """How well a textured mesh agrees with views it was not baked from: those views are rendered through tex["atlas"] and
    through the atlas of the interpolated vertex colours (the same layout), and both are scored by `score`, the three figures
    of `meshpaint.consistency` per pixel.  -> dict(baked=dict(n, mad, psnr), vertex=dict(n, mad, psnr))"""
    verts, faces, vert_colors = mesh_args(verts, faces, vert_colors)
    if vert_colors is None:
        raise ValueError("svs_mesh_atlas_render: consistency needs vertex colours for its baseline")
    images = _mp._images(images, len(list(views)))
    H, W = int(images[0].shape[0]), int(images[0].shape[1])
    size, cell, chart = int(tex["atlas"].shape[0]), int(tex["cell"]), tex["chart"]
    n_slots = int((chart >= 0).sum())
    slot_face = layout(chart, n_slots, size, cell)[1]
    plain = vertex_atlas(faces, verts.shape[0], chart, slot_face, size, cell, vert_colors)
    rgb, face = render(verts, faces, chart, tex["atlas"], cell, views, H, W, near=near)
    base = render(verts, faces, chart, plain, cell, views, H, W, near=near, face=face)[0]
    return dict(baked=score(rgb, face, chart, images, masks), vertex=score(base, face, chart, images, masks))


def texture_folder(ply, scan_folder, view_ids, obj_out, holdout=(), *, size=4096, cell=None, fill=(128, 128, 128),
                   eval_mask_root=None, dataset=None, eval_mask_radius=12, log=None, **rules):
    """Textures the mesh file `ply` from the views of a scan folder (cameras, photographs and evaluation masks as
    `meshpaint.paint_folder` takes them) and writes obj_out with its .mtl and .png.  The PLY's own vertex colours fill the
    texels no view sees; a PLY without colours is painted first (`meshpaint.paint`, same views and rules, with its hole
    filling).  holdout: view ids that are not baked from; `consistency` scores the result against them.
    -> dict(atlas, covered, uv, chart, cell) on the device, stats: dict(files, n_verts, n_faces, faces_written, faces_left_out,
    size, cell, texels_baked, texels_from_vertices, holdout (`consistency`'s dict or None), launches, seconds per phase)."""
    sec = OrderedDict((k, 0.0) for k in ("read", "upload", "paint", "slots", "normals", "raster", "bake", "finish", "score",
                                         "download", "write"))
    calls = dict(ENTRY_CALLS)
    view_ids, holdout = list(view_ids), list(holdout)
    _rules(rules)
    t0 = time.perf_counter()
    verts, faces, colors, views, images, masks, (H, W) = scan_folder_inputs(ply, scan_folder, view_ids + holdout, eval_mask_root,
                                                                            dataset, eval_mask_radius)
    t0 = tick(sec, "read", t0)
    verts_d, faces_d, colors_d = mesh_args(verts, faces, colors)
    images_d = [to_device(im, torch.uint8, "meshtexture", "image") for im in images]
    t0 = tick(sec, "upload", t0)
    n = len(view_ids)
    part_masks = None if masks is None else masks[:n]
    if colors_d is None:
        colors_d = _mp.paint(verts_d, faces_d, views[:n], images_d[:n], part_masks, fill=fill, **rules)[0]
        t0 = tick(sec, "paint", t0)
    stats = dict(seconds=sec)
    tex = texture(verts_d, faces_d, views[:n], images_d[:n], part_masks, size=size, cell=cell, vert_colors=colors_d, stats=stats,
                  fill=fill, **rules)
    held = None
    if holdout:
        t0 = time.perf_counter()
        held = consistency(verts_d, faces_d, tex, colors_d, views[n:], images_d[n:], None if masks is None else masks[n:],
                           near=dict(RULES, **rules)["near"])
        tick(sec, "score", t0)
    t0 = time.perf_counter()
    host = {k: tex[k].cpu().numpy() for k in ("atlas", "covered", "uv", "chart")}
    t0 = tick(sec, "download", t0)
    left_out = _obj.write(obj_out, verts, faces, host["uv"], host["chart"], host["atlas"])
    tick(sec, "write", t0)
    for k in ("acc", "normals", "slot_face"):
        stats.pop(k)
    stats.update(files=dict(obj=obj_out, mtl=obj_out[:-4] + ".mtl", png=obj_out[:-4] + ".png"), n_verts=len(verts),
                 n_faces=len(faces), faces_written=len(faces) - left_out, faces_left_out=left_out, size=int(size), cell=tex["cell"],
                 texels_baked=int((host["covered"] == 1).sum()), texels_from_vertices=int((host["covered"] == 2).sum()),
                 holdout=held, launches=launches_since(ENTRY_CALLS, calls))
    if log is not None:
        log(f"meshtexture: {ply} ({len(verts)} vertices, {len(faces)} faces, {left_out} without a chart) from {n} views of {H} x {W}: "
            f"atlas {size} x {size}, cell {tex['cell']}, {stats['texels_baked']} texels baked, {stats['texels_from_vertices']} from "
            f"vertex colours -> {obj_out}")
        if held is not None:
            log(f"held-out views {' '.join(map(str, holdout))}: {held['baked']['n']} pixels, baked atlas PSNR {held['baked']['psnr']:.2f} dB "
                f"(mean |difference| {held['baked']['mad']:.3f} codes), vertex colours {held['vertex']['psnr']:.2f} dB "
                f"({held['vertex']['mad']:.3f} codes)")
        log(seconds_line(sec))
    return tex, stats


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Bakes a texture atlas for a mesh from a scan's photographs on the GPU, writes OBJ, MTL "
                                            "and PNG, and scores the result against held-out views")
    p.add_argument("--ply", required=True, help="the mesh (a PLY with faces; its vertex colours fill what no view sees)")
    p.add_argument("--scan-folder", required=True, help="holds cams/{id:08}_cam.txt and images/{id:08}.jpg; its last component names the scan")
    p.add_argument("--obj-out", required=True, help="the textured mesh; the .mtl and .png go beside it")
    p.add_argument("--size", type=int, default=4096, help="the atlas is size x size texels")
    p.add_argument("--cell", type=int, default=None, help="texels per cell side, at least 6 (default: the largest that holds every face)")
    _mp.add_painter_args(p, "bake", "texel", "the rendered mesh is scored against them")
    a = p.parse_args(argv)
    _mp.check_painter_args(p, a, "--rel and --abs-tol")
    if not (MIN_CELL <= a.size <= MAX_SIZE) or (a.cell is not None and not (MIN_CELL <= a.cell <= a.size)):
        p.error(f"--size lies in [{MIN_CELL}, {MAX_SIZE}] and --cell in [{MIN_CELL}, size]")
    if not a.obj_out.lower().endswith(".obj"):
        p.error("--obj-out names an .obj file")
    if set(a.views) & set(a.holdout):
        p.error("--holdout names views that --views bakes from")
    return a


def main(argv=None):
    a = parse_args(argv)
    return texture_folder(a.ply, a.scan_folder, a.views, a.obj_out, a.holdout, size=a.size, cell=a.cell, fill=tuple(a.fill),
                          eval_mask_root=a.data_dir_root, dataset=a.dataset, log=print, **_mp.painter_rules(a))


if __name__ == "__main__":
    main()
