"""A scan's depth maps meshed on the HIP path: truncated signed distance (TSDF) fusion (csrc/svs_tsdf.hip).

`svs_hip.run` ends in a point cloud (`fusion.filter_depth_folder`) and `svs_hip.mesh` meshes a checkpoint's SDF network.
This module is the link between the two for runs without a checkpoint (filter_only, the MVS backbones alone): the filtered
depth maps of `fusion.fuse_view` are integrated into a TSDF volume, `mesh.marching_cubes` meshes it, the faces between
observed and never-observed space are dropped, and the vertices take the views' colours:

    python -m svs_hip.tsdf --scan-folder exps_mvs/scan106 --out-folder exps_mvs/scan106 --views 25 22 28 --voxel 1.5 \\
        [--trunc T] [--bounds x0 y0 z0 x1 y1 z1] [--raw] [--largest] [--ply P] [--data-dir-root D --dataset DTU]

writes {out_folder}/tsdf.ply (or --ply), which `evals.eval_dtu.evaluate_scan_files(mode="mesh")` scores once it is named
mvsnet{scan:03}_l3.ply (`svs_hip.run ... +tsdf_voxel=1.5` does that under {outdir}/tsdf/).

OURS throughout: the reference has no TSDF.  The arithmetic is fixed in include/svolsdf_hip.h and restated in float64 in
tests/tsdf_oracle.py.  SETTINGS: `trunc` (default `TRUNC_VOXELS` = 3 voxels), `min_weight` of the face rule (default 1: a
face survives when every node of its cell was observed at least once), `max_voxels` (default 2**30).
"""
import argparse
import ctypes
import os
import time
from collections import OrderedDict

import numpy as np
import torch

from . import lib as _lib
from . import fusion
from . import mesh as _mesh
from . import ply as _ply
from .images import device as _device, seconds_line, tick, to_device
from .ops import _f32, _ptr, _ptr_array, _stream
from .views import MAX_VIEWS, add_eval_mask_args, check_eval_mask_args, chunks, device_masks, view_matrices

TRUNC_VOXELS = 3.0                   # the default truncation distance in voxels
MAX_VOXELS = 1 << 30
ENTRY_CALLS = {"integrate": 0, "keep": 0, "colors": 0}      # C entry points called, not kernels
_D3 = ctypes.c_double * 3


def integrate_raw(tsdf, weight, rgb, origin, voxel, trunc, depths, masks, images, mats, H, W):
    """One call of svs_tsdf_integrate on device tensors -> its return code (`Volume.integrate` is the checked form)."""
    L = _lib.load()
    n0, n1, n2 = (int(s) for s in tsdf.shape)
    rc = L.svs_tsdf_integrate(_ptr(tsdf), _ptr(weight), _ptr(rgb), n0, n1, n2, _D3(*[float(o) for o in origin]), float(voxel),
                              float(trunc), _ptr_array(depths), _ptr_array(masks) if masks is not None else None,
                              _ptr_array(images) if images is not None else None, _ptr(mats), len(depths), int(H), int(W),
                              _stream())
    ENTRY_CALLS["integrate"] += 1
    return rc


def face_keep(weight, cells, min_weight=1.0):
    """keep (F,) uint8: 1 where all eight nodes of the face's cell have weight >= min_weight.  cells: (F,) int32 node
    indices (`mesh.marching_cubes(..., return_cells=True)`)."""
    n0, n1, n2 = (int(s) for s in weight.shape)
    cells = cells.to(torch.int32).contiguous()
    keep = torch.empty(cells.shape[0], dtype=torch.uint8, device=weight.device)
    _lib.check(_lib.load().svs_tsdf_face_keep(_ptr(weight), n0, n1, n2, _ptr(cells), int(cells.shape[0]), float(min_weight),
                                              _ptr(keep), _stream()), "svs_tsdf_face_keep")
    ENTRY_CALLS["keep"] += 1
    return keep


def vertex_colors(rgb, weight, verts):
    """verts (V,3) float32 in volume index units -> (V,3) float32: trilinear over the observed nodes around each vertex"""
    n0, n1, n2 = (int(s) for s in weight.shape)
    verts = _f32(verts)
    out = torch.empty(verts.shape[0], 3, dtype=torch.float32, device=weight.device)
    _lib.check(_lib.load().svs_tsdf_vertex_colors(_ptr(rgb), _ptr(weight), n0, n1, n2, _ptr(verts), int(verts.shape[0]), _ptr(out),
                                                  _stream()), "svs_tsdf_vertex_colors")
    ENTRY_CALLS["colors"] += 1
    return out


def colors_u8(c):
    """floor(c * 255 + 0.5) clamped to [0, 255] -> uint8"""
    return torch.floor(c.double() * 255.0 + 0.5).clamp_(0, 255).to(torch.uint8)


class Volume:
    """A TSDF volume on the GPU: node (i,j,k) sits at origin + (i,j,k) * voxel.  tsdf (n0,n1,n2) float32 starts at 1, weight
    at 0, rgb planar (3,n0,n1,n2) at 0 (colors=False: no rgb).  trunc: the truncation distance, a setting; default
    TRUNC_VOXELS = 3 voxels."""

    def __init__(self, origin, shape, voxel, trunc=None, colors=True, device=None):
        self.origin = np.asarray(origin, np.float64).reshape(3)
        self.shape = tuple(int(s) for s in shape)
        self.voxel = float(voxel)
        self.trunc = TRUNC_VOXELS * self.voxel if trunc is None else float(trunc)
        if len(self.shape) != 3 or min(self.shape) < 1:
            raise ValueError(f"Volume: shape must be three positive sizes, got {shape}")
        if not (self.voxel > 0 and self.trunc > 0):
            raise ValueError(f"Volume: voxel and trunc must be positive, got {voxel} and {trunc}")
        dev = _device("tsdf") if device is None else torch.device(device)
        self.tsdf = torch.ones(self.shape, dtype=torch.float32, device=dev)
        self.weight = torch.zeros(self.shape, dtype=torch.float32, device=dev)
        self.rgb = torch.zeros((3,) + self.shape, dtype=torch.float32, device=dev) if colors else None
        self.launches = 0

    def integrate(self, views):
        """views: dicts of K (3,3), E (4,4), depth (H,W) [, mask (H,W), img (H,W,3) float32 in [0,1]]; arrays or device
        tensors.  All of one size (AssertionError otherwise, as `fusion.fuse_view`); MAX_VIEWS views per launch."""
        views = list(views)
        if not views:
            return self
        depths = [to_device(v["depth"], torch.float32, "tsdf") for v in views]
        H, W = depths[0].shape
        images = []
        for v, d in zip(views, depths):
            if tuple(d.shape) != (H, W):
                raise AssertionError("depth map shapes differ between the views")
            if self.rgb is not None:
                if v.get("img") is None:
                    raise ValueError("a volume with colours needs every view's img")
                img = to_device(v["img"], torch.float32, "tsdf")
                if tuple(img.shape) != (H, W, 3):
                    raise AssertionError("image shape differs from its depth map's")
                images.append(img)
        masks = device_masks([v.get("mask") for v in views], len(views), H, W, self.tsdf.device, "svs_tsdf_integrate",
                             AssertionError)
        for at, to, mats_d in chunks(views, self.tsdf.device):
            rc = integrate_raw(self.tsdf, self.weight, self.rgb, self.origin, self.voxel, self.trunc, depths[at:to], masks[at:to],
                               images[at:to] if self.rgb is not None else None, mats_d, H, W)
            _lib.check(rc, "svs_tsdf_integrate")
            self.launches += 1
        return self

    def mesh(self, min_weight=1, largest=False, timers=None):
        """-> verts (V,3) float32 world positions, faces (F,3) int32, rgb (V,3) uint8 (None without colours), on the device.
        `mesh.marching_cubes` at level 0, the faces whose cell has a node with weight < min_weight dropped, the unused
        vertices dropped; largest=True: the largest component by area.  ValueError when nothing crosses zero or nothing is kept."""
        sp = (self.voxel,) * 3
        verts, faces, cells = _mesh.marching_cubes(self.tsdf, 0.0, sp, timers=timers, return_cells=True)
        t0 = time.perf_counter()
        keep = face_keep(self.weight, cells, min_weight)
        faces = faces[keep.bool()]
        if faces.shape[0] == 0:
            raise ValueError(f"tsdf: no face is kept at min_weight {min_weight} ({int(keep.numel())} faces cross zero)")
        verts, faces = _mesh.compact(verts, faces)
        if largest:
            verts, faces = _mesh.largest_component(verts, faces)
        t0 = tick(timers, "keep", t0)
        rgb = None
        if self.rgb is not None:
            rgb = colors_u8(vertex_colors(self.rgb, self.weight, (verts.double() / self.voxel).float()))
        origin = torch.as_tensor(self.origin, dtype=torch.float64, device=verts.device)
        verts = (verts.double() + origin).float()
        tick(timers, "colors", t0)
        return verts, faces, rgb


def bounds_from_points(xyz, voxel, pad, max_voxels=MAX_VOXELS):
    """-> origin (3,) float64, shape (3 ints): origin = floor((min - pad) / voxel) * voxel, shape = ceil((max + pad - origin)
    / voxel) + 1, on the host in float64.  ValueError naming the voxel count when it exceeds max_voxels."""
    xyz = np.asarray(xyz.detach().cpu() if torch.is_tensor(xyz) else xyz, np.float64).reshape(-1, 3)
    if len(xyz) == 0:
        raise ValueError("bounds_from_points: no points")
    voxel, pad = float(voxel), float(pad)
    if not voxel > 0:
        raise ValueError(f"bounds_from_points: voxel must be positive, got {voxel}")
    lo, hi = xyz.min(0), xyz.max(0)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("bounds_from_points: points are not finite")
    origin = np.floor((lo - pad) / voxel) * voxel
    shape = tuple(int(n) for n in np.ceil((hi + pad - origin) / voxel) + 1)
    count = shape[0] * shape[1] * shape[2]
    if count > max_voxels:
        raise ValueError(f"bounds_from_points: {shape[0]} x {shape[1]} x {shape[2]} = {count} voxels exceed the budget of "
                         f"{max_voxels}: choose a larger voxel or tighter bounds")
    return origin, shape


def fuse_folder(scan_folder, out_folder, view_ids, voxel, trunc=None, ply=None, bounds=None, depth="averaged", conf=0.0,
                filter_dist=1, filter_diff=0.01, thres_view=1, *, eval_mask_root=None, dataset=None, eval_mask_radius=12,
                min_weight=1, largest=False, max_voxels=MAX_VOXELS, log=None):
    """Reads what `fusion.filter_depth_folder` reads, runs `fusion.fuse_view` per view against the others, integrates every
    view and writes the coloured mesh to `ply` (default {out_folder}/tsdf.ply).
    depth="averaged": depth_avg cast to float32 under final_mask; "raw": the view's depth map under photo_mask.
    bounds: (x0,y0,z0,x1,y1,z1); default: the fused points of all views padded by trunc + voxel.  The evaluation masks as
    filter_depth_folder takes them.  -> verts (V,3) float32, faces (F,3) int32, rgb (V,3) uint8 (numpy), stats: dict(file,
    shape, origin, n_verts, n_faces, launches, seconds per phase)."""
    if depth not in ("averaged", "raw"):
        raise ValueError(f"depth: 'averaged' or 'raw', got {depth!r}")
    voxel = float(voxel)
    trunc = TRUNC_VOXELS * voxel if trunc is None else float(trunc)
    sec = OrderedDict((k, 0.0) for k in ("read", "filter", "bounds", "integrate", "scan", "classify", "emit", "keep", "colors",
                                         "download", "write"))
    t0 = time.perf_counter()
    views, pairs, eval_masks = fusion.scan_inputs(scan_folder, out_folder, view_ids, eval_mask_root, dataset, eval_mask_radius)
    t0 = tick(sec, "read", t0)
    tviews, clouds = [], []
    for v, out in fusion.fuse_views(views, pairs, eval_masks, conf=conf, filter_dist=filter_dist, filter_diff=filter_diff,
                                    thres_view=thres_view, points=bounds is None):
        if bounds is None:
            clouds.append(out["xyz"])
        d, m = (out["depth_avg"].float(), out["final_mask"]) if depth == "averaged" else (views[v]["depth"], out["photo_mask"])
        tviews.append(dict(K=views[v]["K"], E=views[v]["E"], depth=d, mask=m, img=views[v]["img"]))
    t0 = tick(sec, "filter", t0)
    if bounds is None:
        pts = torch.cat(clouds, 0)
        if pts.shape[0] == 0:
            raise ValueError("tsdf: no pixel survives the filter, so there is nothing to bound the volume with")
        corners = torch.stack([pts.min(0)[0], pts.max(0)[0]]).cpu().numpy()
        origin, shape = bounds_from_points(corners, voxel, trunc + voxel, max_voxels)
    else:
        b = np.asarray(bounds, np.float64).reshape(2, 3)
        origin, shape = bounds_from_points(b, voxel, 0.0, max_voxels)
    t0 = tick(sec, "bounds", t0)
    vol = Volume(origin, shape, voxel, trunc)
    vol.integrate(tviews)
    t0 = tick(sec, "integrate", t0)
    verts, faces, rgb = vol.mesh(min_weight=min_weight, largest=largest, timers=sec)
    sec.pop("workspace_bytes", None)
    t0 = time.perf_counter()
    v, f, c = verts.cpu().numpy(), faces.cpu().numpy(), rgb.cpu().numpy()
    t0 = tick(sec, "download", t0)
    ply = os.path.join(out_folder, "tsdf.ply") if ply is None else ply
    os.makedirs(os.path.dirname(ply) or ".", exist_ok=True)
    _ply.write(ply, v, c, f)
    tick(sec, "write", t0)
    stats = dict(file=ply, shape=shape, origin=origin, n_verts=len(v), n_faces=len(f), launches=vol.launches, seconds=sec)
    if log is not None:
        log(f"tsdf: {ply} ({len(v)} vertices, {len(f)} faces, volume {shape[0]} x {shape[1]} x {shape[2]})")
        log(seconds_line(sec))
    return v, f, c, stats


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Meshes a scan's filtered depth maps on the GPU: TSDF fusion, marching cubes, "
                                            "vertex colours -> a PLY that evals.eval_dtu --mode mesh reads")
    p.add_argument("--scan-folder", required=True, help="holds cams/{id:08}_cam.txt and images/{id:08}.jpg")
    p.add_argument("--out-folder", required=True, help="holds depth_est/ and confidence/ PFMs")
    p.add_argument("--views", type=int, nargs="+", required=True, help="view ids, e.g. 25 22 28")
    p.add_argument("--voxel", type=float, required=True, help="voxel size in world units")
    p.add_argument("--trunc", type=float, default=None, help="truncation distance (default: 3 voxels)")
    p.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                   help="the volume's box (default: the fused points, padded by trunc + voxel)")
    p.add_argument("--raw", action="store_true", help="integrate the depth maps under the photometric mask instead of the "
                                                      "averaged depth under the final mask")
    p.add_argument("--largest", action="store_true", help="keep the largest component by area")
    p.add_argument("--ply", default=None, help="output file (default: {out_folder}/tsdf.ply)")
    p.add_argument("--min-weight", type=float, default=1.0, help="a face survives when every node of its cell has this weight")
    add_eval_mask_args(p, "cut every view by its evaluation mask")
    a = p.parse_args(argv)
    check_eval_mask_args(p, a)
    return a


def main(argv=None):
    a = parse_args(argv)
    return fuse_folder(a.scan_folder, a.out_folder, a.views, a.voxel, trunc=a.trunc, ply=a.ply, bounds=a.bounds,
                       depth="raw" if a.raw else "averaged", eval_mask_root=a.data_dir_root, dataset=a.dataset,
                       min_weight=a.min_weight, largest=a.largest, log=print)


if __name__ == "__main__":
    main()
