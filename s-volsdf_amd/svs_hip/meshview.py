"""A mesh seen from a scan's own cameras on the HIP path (csrc/svs_meshview.hip): its depth map beside depth_est/, a shaded
picture of it on a headless machine, and the mesh cut to what the cameras and the evaluation masks see.

    python -m svs_hip.meshview --ply exps_mvs/tsdf/mvsnet106_l3.ply --scan-folder exps_mvs/scan106 --out-folder exps_mvs/scan106 \\
        --views 25 22 28 [--size H W] [--cull --min-views K --max-off-mask N --any --rel R --abs-tol T --ply-out P] \\
        [--data-dir-root D --dataset DTU]

writes {out_folder}/mesh_depth/{id:08}.pfm and {out_folder}/mesh_shade/{id:08}.png, and with --cull the pruned mesh
(`svs_hip.run ... +tsdf_voxel=1.5 +tsdf_views=true` renders every scan's TSDF mesh under {outdir}/tsdf/scanNNN/).

OURS throughout: the reference has no such step.  The arithmetic is fixed in include/svolsdf_hip.h and restated in float64 in
tests/meshview_oracle.py.  LIMIT: a face with a vertex at or behind `near` is dropped, not clipped.  SETTINGS: `near`
(default 1e-6), the visibility tolerances `rel` (default 0.01, the relative depth test of the fusion's filter_diff) and
`abs_tol`, the cull rule's `min_views`, `max_off_mask` and `mode`.
"""
import argparse
import os
import time
from collections import OrderedDict

import numpy as np
import torch

from . import lib as _lib
from . import mesh as _mesh
from . import ply as _ply
from .images import device as _device, seconds_line, tick, to_device
from .ops import _ptr, _ptr_array, _stream
from .views import (MAX_VIEWS, add_eval_mask_args, check_eval_mask_args, chunks, device_masks, folder_cameras, folder_masks,
                    folder_size, launches_since, mesh_args)

FACE_CHUNK = 1 << 22                 # faces per call of svs_mesh_raster: bounds the list of the large path (256 MiB at 16 views)
WORK_HEAD = 4                        # ints of the work buffer in front of that list
FLAG_COUNT, FLAG_SMALL_ONLY, FLAG_LARGE_ONLY = 1, 2, 4
ENTRY_CALLS = {"raster": 0, "resolve": 0, "visibility": 0}  # C entry points called, not kernels


def small_box():
    """pixels of a clamped bounding box up to which the lane that set a face up walks it (kSmallBox)"""
    return int(_lib.load().svs_mesh_raster_small_box())


def new_zbuf(n_views, H, W, device=None):
    """(n_views,H,W) int64 device tensor of all-ones bits: the empty buffer svs_mesh_raster folds faces into"""
    dev = _device("meshview") if device is None else torch.device(device)
    return torch.full((int(n_views), int(H), int(W)), -1, dtype=torch.int64, device=dev)


def raster_raw(zbuf, verts, faces, mats, n_views, H, W, near=1e-6, face_base=0, work=None, flags=0):
    """One call of svs_mesh_raster on device tensors -> (its return code, the work buffer: [0] = (view, face) pairs that
    took the large path).  `raster_into` is the checked form."""
    n_faces = int(faces.shape[0])
    if work is None:
        alloc = torch.empty if n_faces and n_views else torch.zeros           # the entry zeroes the head unless the mesh is empty
        work = alloc(WORK_HEAD + max(0, min(int(n_views), MAX_VIEWS)) * n_faces, dtype=torch.int32, device=zbuf.device)
    rc = _lib.load().svs_mesh_raster(_ptr(verts), int(verts.shape[0]), _ptr(faces), n_faces, _ptr(mats), int(n_views), int(H),
                                     int(W), float(near), int(face_base), _ptr(zbuf), _ptr(work), int(work.numel()), int(flags),
                                     _stream())
    ENTRY_CALLS["raster"] += 1
    return rc, work


def raster_into(zbuf, verts, faces, mats, near=1e-6, face_base=0, flags=0, stats=None):
    """Folds a mesh into zbuf (n_views <= MAX_VIEWS, H, W), FACE_CHUNK faces per call.  stats: a dict whose "large" (pairs on
    the large path) and, under FLAG_COUNT, "small" and "atomics" are added to -- reading them waits for the device."""
    n_views, H, W = (int(s) for s in zbuf.shape)
    for at in range(0, max(1, int(faces.shape[0])), FACE_CHUNK):
        part = faces[at:at + FACE_CHUNK]
        rc, work = raster_raw(zbuf, verts, part, mats, n_views, H, W, near, face_base + at, flags=flags)
        _lib.check(rc, "svs_mesh_raster")
        if stats is not None:
            head = work[:WORK_HEAD].cpu().numpy()
            stats["large"] = stats.get("large", 0) + int(head[0])
            stats["small"] = stats.get("small", 0) + int(head[1])
            stats["atomics"] = stats.get("atomics", 0) + int(head[2:4].view(np.uint64)[0])
    return zbuf


def resolve(zbuf, verts, faces, mats, face_base=0, colors=None, normals=False, shade=False, out=None):
    """svs_mesh_raster_resolve -> dict(depth (n,H,W) float32, face (n,H,W) int32[, normal (n,H,W,3) float32, shade (n,H,W,3)
    uint8]).  out: a dict of earlier results whose normal / shade are written into (ids of another call's mesh stay)."""
    n_views, H, W = (int(s) for s in zbuf.shape)
    dev = zbuf.device
    res = dict(depth=torch.empty((n_views, H, W), dtype=torch.float32, device=dev),
               face=torch.empty((n_views, H, W), dtype=torch.int32, device=dev))
    if normals:
        res["normal"] = out["normal"] if out is not None else torch.zeros((n_views, H, W, 3), dtype=torch.float32, device=dev)
    if shade:
        res["shade"] = out["shade"] if out is not None else torch.full((n_views, H, W, 3), 255, dtype=torch.uint8, device=dev)
    rc = _lib.load().svs_mesh_raster_resolve(_ptr(zbuf), _ptr(verts), int(verts.shape[0]), _ptr(faces), int(faces.shape[0]),
                                             _ptr(mats), n_views, H, W, int(face_base), _ptr(colors), _ptr(res["depth"]),
                                             _ptr(res["face"]), _ptr(res.get("normal")), _ptr(res.get("shade")), _stream())
    ENTRY_CALLS["resolve"] += 1
    _lib.check(rc, "svs_mesh_raster_resolve")
    return res


def rasterize(verts, faces, views, H, W, near=1e-6, colors=None, normals=False, shade=False, stats=None):
    """verts (V,3), faces (F,3), colors (V,3) uint8 or None: arrays or device tensors; views: dicts of K (3,3), E (4,4).
    -> dict of device tensors: depth (n,H,W) float32 (camera z, 0 where empty), face (n,H,W) int32 (-1 where empty)
    [, normal (n,H,W,3) float32 towards the camera, shade (n,H,W,3) uint8].  MAX_VIEWS views per launch."""
    verts, faces, colors = mesh_args(verts, faces, colors)
    views = list(views)
    if not (near > 0):
        raise ValueError(f"svs_mesh_raster: near must be positive, got {near}")
    H, W = int(H), int(W)
    parts = []
    for at, to, mats in chunks(views, verts.device):
        zbuf = raster_into(new_zbuf(to - at, H, W, verts.device), verts, faces, mats, near, stats=stats)
        parts.append(resolve(zbuf, verts, faces, mats, colors=colors, normals=normals, shade=shade))
    if not parts:
        raise ValueError("svs_mesh_raster: no views")
    return {k: torch.cat([p[k] for p in parts], 0) if len(parts) > 1 else parts[0][k] for k in parts[0]}


def visibility_raw(verts, mats, n_views, H, W, depth, masks, rel, abs_tol, seen, off_mask, near=1e-6):
    """One call of svs_mesh_vertex_visibility on device tensors -> its return code (`visibility` is the checked form)."""
    rc = _lib.load().svs_mesh_vertex_visibility(_ptr(verts), int(verts.shape[0]), _ptr(mats), int(n_views), int(H), int(W),
                                                float(near), _ptr(depth), _ptr_array(masks) if masks is not None else None,
                                                float(rel), float(abs_tol), _ptr(seen), _ptr(off_mask), _stream())
    ENTRY_CALLS["visibility"] += 1
    return rc


def visibility(verts, views, depth, masks=None, rel=0.01, abs_tol=0.0, near=1e-6):
    """depth: (n_views,H,W) float32 as `rasterize` returns it; masks: None or per view None / an (H,W) array, non-zero =
    inside.  -> (seen, off_mask): (V,) int32 device tensors, the views in which a vertex is not hidden behind the depth map
    (z <= d (1 + rel) + abs_tol, or nothing drawn there) and those in which it falls on a zero of the mask."""
    verts = to_device(verts, torch.float32, "meshview", "verts")
    views = list(views)
    depth = to_device(depth, torch.float32, "meshview", "depth", ndim=(3,))
    if depth.shape[0] != len(views):
        raise ValueError(f"svs_mesh_vertex_visibility: {depth.shape[0]} depth maps for {len(views)} views")
    if rel < 0 or abs_tol < 0 or not (near > 0):
        raise ValueError(f"svs_mesh_vertex_visibility: near must be positive, rel and abs_tol not negative, got {near}, {rel}, {abs_tol}")
    H, W = int(depth.shape[1]), int(depth.shape[2])
    dev_masks = device_masks(masks, len(views), H, W, verts.device, "svs_mesh_vertex_visibility")
    seen = torch.zeros(verts.shape[0], dtype=torch.int32, device=verts.device)
    off_mask = torch.zeros_like(seen)
    for at, to, mats in chunks(views, verts.device):
        rc = visibility_raw(verts, mats, to - at, H, W, depth[at:to], dev_masks[at:to] if dev_masks is not None else None,
                            rel, abs_tol, seen, off_mask, near)
        _lib.check(rc, "svs_mesh_vertex_visibility")
    return seen, off_mask


def cull(verts, faces, seen, off_mask=None, min_views=1, max_off_mask=None, mode="all", colors=None):
    """A vertex survives iff seen >= min_views and, when max_off_mask is given, off_mask <= max_off_mask; a face iff all of its
    vertices do (mode="any": one of them); then `mesh.compact`.  Tensors on one device (the host will do).
    -> verts, faces[, colors] of the surviving mesh"""
    if mode not in ("all", "any"):
        raise ValueError(f"cull: mode 'all' or 'any', got {mode!r}")
    if max_off_mask is not None and off_mask is None:
        raise ValueError("cull: max_off_mask needs off_mask")
    verts, faces, seen = torch.as_tensor(verts), torch.as_tensor(faces), torch.as_tensor(seen)
    alive = seen >= min_views
    if max_off_mask is not None:
        alive &= torch.as_tensor(off_mask).to(alive.device) <= max_off_mask
    corner = alive[faces.long()]
    faces = faces[corner.all(1) if mode == "all" else corner.any(1)]
    out = _mesh.compact(verts, faces)
    if colors is not None:
        used = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
        used[faces.reshape(-1).long()] = True
        out += (torch.as_tensor(colors).to(verts.device)[used].contiguous(),)
    return out


_cull = cull                         # view_folder's switch has the rule's name


def view_folder(ply, scan_folder, out_folder, view_ids, size=None, cull=False, min_views=1, max_off_mask=None, mode="all",
                rel=0.01, abs_tol=0.0, near=1e-6, ply_out=None, *, eval_mask_root=None, dataset=None, eval_mask_radius=12,
                log=None):
    """Renders the mesh file `ply` into the views of a scan folder: cameras from cams/{id:08}_cam.txt, the image size from
    images/{id:08}.jpg unless size = (H, W) is given (the cameras are taken as they are: they belong to that size).  Writes
    {out_folder}/mesh_depth/{id:08}.pfm (camera z, 0 where nothing is drawn) and {out_folder}/mesh_shade/{id:08}.png.
    cull=True: the mesh pruned by `visibility` and `cull` goes to ply_out (default {out_folder}/mesh_culled.ply); with
    eval_mask_root and dataset the evaluation masks count towards off_mask, as `fusion.scan_inputs` takes them.
    -> result (`rasterize`'s dict), stats: dict(files, n_faces, covered per view, faces_kept, launches, seconds per phase)."""
    from datasets.data_io import save_pfm
    from PIL import Image
    sec = OrderedDict((k, 0.0) for k in ("read", "upload", "raster", "visibility", "download", "write"))
    calls = dict(ENTRY_CALLS)
    view_ids = list(view_ids)
    t0 = time.perf_counter()
    verts, faces, colors = _ply.read_mesh_colors(ply)
    views = folder_cameras(scan_folder, view_ids)
    if size is None:
        size = folder_size(scan_folder, view_ids, "svs_mesh_raster")
    H, W = int(size[0]), int(size[1])
    masks = folder_masks(eval_mask_root, dataset, os.path.normpath(out_folder).split(os.sep)[-1], view_ids, H, W,
                         eval_mask_radius)
    t0 = tick(sec, "read", t0)
    verts_d, faces_d, colors_d = mesh_args(verts, faces, colors)
    t0 = tick(sec, "upload", t0)
    res = rasterize(verts_d, faces_d, views, H, W, near=near, colors=colors_d, shade=True)
    t0 = tick(sec, "raster", t0)
    kept = None
    if cull:
        seen, off = visibility(verts_d, views, res["depth"], masks, rel, abs_tol, near)
        kept = _cull(verts_d, faces_d, seen, off, min_views, max_off_mask, mode, colors=colors_d)
        t0 = tick(sec, "visibility", t0)
    depth, shade = res["depth"].cpu().numpy(), res["shade"].cpu().numpy()
    if kept is not None:
        kept = tuple(k.cpu().numpy() if k is not None else None for k in (kept + (None,))[:3])
    t0 = tick(sec, "download", t0)
    files = OrderedDict(depth=[], shade=[])
    for sub in ("mesh_depth", "mesh_shade"):
        os.makedirs(os.path.join(out_folder, sub), exist_ok=True)
    for i, v in enumerate(view_ids):
        files["depth"].append(os.path.join(out_folder, "mesh_depth", "{:0>8}.pfm".format(v)))
        save_pfm(files["depth"][-1], depth[i])
        files["shade"].append(os.path.join(out_folder, "mesh_shade", "{:0>8}.png".format(v)))
        Image.fromarray(shade[i]).save(files["shade"][-1], compress_level=1)
    if kept is not None:
        ply_out = os.path.join(out_folder, "mesh_culled.ply") if ply_out is None else ply_out
        os.makedirs(os.path.dirname(ply_out) or ".", exist_ok=True)
        _ply.write(ply_out, kept[0], kept[2], kept[1])
        files["ply"] = ply_out
    tick(sec, "write", t0)
    stats = dict(files=files, n_verts=len(verts), n_faces=len(faces), covered=[int((d > 0).sum()) for d in depth],
                 faces_kept=None if kept is None else len(kept[1]),
                 launches=launches_since(ENTRY_CALLS, calls), seconds=sec)
    if log is not None:
        log(f"meshview: {ply} ({len(verts)} vertices, {len(faces)} faces) into {len(view_ids)} views of {H} x {W}: covered "
            + " ".join(str(c) for c in stats["covered"]) + (f"; {stats['faces_kept']} faces kept -> {files['ply']}" if kept else ""))
        log(seconds_line(sec))
    return res, stats


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Renders a mesh into a scan's own views on the GPU: depth PFMs and shaded PNGs, "
                                            "and with --cull the mesh cut to what the views and the evaluation masks see")
    p.add_argument("--ply", required=True, help="the mesh (a PLY with faces; vertex colours are used when it has them)")
    p.add_argument("--scan-folder", required=True, help="holds cams/{id:08}_cam.txt and images/{id:08}.jpg")
    p.add_argument("--out-folder", required=True, help="mesh_depth/ and mesh_shade/ are written here; its last component names the scan")
    p.add_argument("--views", type=int, nargs="+", required=True, help="view ids, e.g. 25 22 28")
    p.add_argument("--size", type=int, nargs=2, default=None, metavar=("H", "W"), help="the views' size (default: the JPEGs')")
    p.add_argument("--cull", action="store_true", help="write the mesh without the faces no view sees")
    p.add_argument("--min-views", type=int, default=1, help="a vertex survives when this many views see it")
    p.add_argument("--max-off-mask", type=int, default=None, help="and when at most this many views have it off their mask")
    p.add_argument("--any", action="store_true", help="a face survives with one surviving vertex (default: all three)")
    p.add_argument("--rel", type=float, default=0.01, help="relative depth tolerance of the visibility test")
    p.add_argument("--abs-tol", type=float, default=0.0, help="absolute depth tolerance of the visibility test")
    p.add_argument("--ply-out", default=None, help="the culled mesh (default: {out_folder}/mesh_culled.ply)")
    add_eval_mask_args(p, "the evaluation masks count towards --max-off-mask")
    a = p.parse_args(argv)
    check_eval_mask_args(p, a)
    return a


def main(argv=None):
    a = parse_args(argv)
    return view_folder(a.ply, a.scan_folder, a.out_folder, a.views, size=a.size, cull=a.cull, min_views=a.min_views,
                       max_off_mask=a.max_off_mask, mode="any" if a.any else "all", rel=a.rel, abs_tol=a.abs_tol,
                       ply_out=a.ply_out, eval_mask_root=a.data_dir_root, dataset=a.dataset, log=print)


if __name__ == "__main__":
    main()
