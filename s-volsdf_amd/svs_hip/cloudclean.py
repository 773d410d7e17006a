"""Cleaning a fused point cloud on the GPU: statistical outlier removal and oriented normals (csrc/svs_cloudknn.hip through
`svs_hip.clouds`).

The fused cloud of `fusion.filter_depth` keeps every pixel that passes the photometric and geometric tests; the isolated
points among them count against the accuracy half of the Chamfer distance, and the file carries no normals.  Here a point's
score is the mean distance to its k nearest other points, a point is kept when score <= mean + std_ratio * std of all scores
(the common remove_statistical_outlier recipe), and the kept points get the PCA normal of their normal_k neighbourhood,
turned towards the camera the point was fused from -- which this pipeline knows, so the orientation is exact, not propagated.

    clean_cloud(xyz, rgb, view_index, centres, ...)        arrays or tensors in, a dict of host arrays out
    clean_folder(scan_folder, out_folder, view_ids, ply)   a fused scan folder: `fusion.scan_inputs` + `fusion.fuse_views`
    clean_ply(ply_in, ply_out, centres=None)               a cloud without provenance: towards the nearest centre, or unoriented

    python -m svs_hip.cloudclean --scan-folder S --out-folder O --views 25 22 28 --ply-out P [--k 20 --std-ratio 2
        --normal-k 16 --max-radius R --no-outliers --no-normals] [--data-dir-root D --dataset DTU]
    python -m svs_hip.cloudclean --ply IN --ply-out P [...]

The arithmetic is this project's own (include/svolsdf_hip.h section f4c); tests/cloudclean_oracle.py restates it in numpy.
"""
import argparse
import time

import numpy as np
import torch

from . import clouds, ply
from .images import seconds_line, tick, to_device

PHASES = ("read", "fuse", "outliers", "compact", "normals", "download", "write")


def camera_centre(E):
    """-R^T t of a world-to-camera E (4,4) -> (3,) float64"""
    E = np.asarray(E, np.float64)
    return -E[:3, :3].T @ E[:3, 3]


def clean_cloud(xyz, rgb, view_index, centres, k=20, std_ratio=2.0, normal_k=16, max_radius=None, outliers=True, normals=True,
                seconds=None):
    """xyz (n,3), rgb (n,3) uint8 or None, view_index (n,) (the row of `centres` a point was fused from) or None, centres
    (n_views,3) or None; arrays or tensors, host or device.  Outliers are removed first, the normals are estimated on the
    KEPT points.  max_radius: the neighbour search radius of both steps (default `clouds.default_radius` of each).
    -> dict(xyz (m,3) float32, rgb (m,3) uint8 or None, normals (m,3) float32 or None, curvature (m,) float32 or None,
    keep (n,) bool, view_index (m,) int32 or None: the kept points', stats: `clouds.outlier_mask`'s dict plus points_in,
    points_kept), host arrays."""
    t0 = time.perf_counter()
    pts = to_device(xyz, torch.float64, "cloudclean").reshape(-1, 3)
    n = pts.shape[0]
    if outliers and n:
        keep, stats = clouds.outlier_mask(pts, k=k, std_ratio=std_ratio, max_radius=max_radius)
    else:
        keep, stats = torch.ones(n, dtype=torch.bool, device=pts.device), dict(count=n, mean=0.0, std=0.0, threshold=float("inf"))
    t0 = tick(seconds, "outliers", t0)
    kept = clouds.compact(pts, keep) if n else pts
    where = torch.nonzero(keep).reshape(-1)
    t0 = tick(seconds, "compact", t0)
    nrm = curv = None
    vi = None if view_index is None else to_device(view_index, torch.int32, "cloudclean").reshape(-1)[where].contiguous()
    if normals:
        nrm, curv = clouds.estimate_normals(kept, k=normal_k, max_radius=max_radius, view_index=None if centres is None else vi,
                                            centres=centres)
    t0 = tick(seconds, "normals", t0)
    sel = where.cpu().numpy()
    xyz_h = np.asarray(xyz.detach().cpu() if torch.is_tensor(xyz) else xyz).reshape(-1, 3)
    out = dict(xyz=np.ascontiguousarray(xyz_h[sel], np.float32), rgb=None, normals=None, curvature=None, keep=keep.cpu().numpy(),
               view_index=None if vi is None else vi.cpu().numpy())
    if rgb is not None:
        out["rgb"] = np.asarray(rgb.detach().cpu() if torch.is_tensor(rgb) else rgb, np.uint8).reshape(-1, 3)[sel]
    if normals:
        out["normals"], out["curvature"] = nrm.cpu().numpy(), curv.cpu().numpy()
    stats.update(points_in=n, points_kept=int(len(sel)))
    out["stats"] = stats
    tick(seconds, "download", t0)
    return out


def clean_folder(scan_folder, out_folder, view_ids, plyfilename, k=20, std_ratio=2.0, normal_k=16, max_radius=None, outliers=True,
                 normals=True, conf=0.0, filter_dist=1, filter_diff=0.01, thres_view=1, eval_mask_root=None, dataset=None):
    """A fused scan folder (cams/ and images/ under scan_folder, depth_est/ and confidence/ under out_folder) -> the cleaned
    cloud in plyfilename (x y z nx ny nz red green blue).  The views are fused as `fusion.filter_depth_folder` fuses them
    (same settings, same evaluation masks), which is where a point's view comes from; the camera centres are -R^T t of
    every view's E.  -> `clean_cloud`'s dict, stats with `seconds` per phase and `file`."""
    from . import fusion
    seconds = {k_: 0.0 for k_ in PHASES}
    t0 = time.perf_counter()
    view_ids = list(view_ids)
    views, pairs, eval_masks = fusion.scan_inputs(scan_folder, out_folder, view_ids, eval_mask_root, dataset)
    centres = np.stack([camera_centre(views[v]["E"]) for v in view_ids])
    t0 = tick(seconds, "read", t0)
    xyz, rgb, vidx = [], [], []
    for ref_view, out in fusion.fuse_views(views, pairs, eval_masks, conf=conf, filter_dist=filter_dist, filter_diff=filter_diff,
                                           thres_view=thres_view):
        xyz.append(out["xyz"])
        rgb.append(out["rgb"])
        vidx.append(torch.full((out["xyz"].shape[0],), view_ids.index(ref_view), dtype=torch.int32, device=out["xyz"].device))
    xyz, rgb, vidx = torch.cat(xyz, 0), torch.cat(rgb, 0), torch.cat(vidx, 0)
    t0 = tick(seconds, "fuse", t0)
    res = clean_cloud(xyz, rgb, vidx, centres, k=k, std_ratio=std_ratio, normal_k=normal_k, max_radius=max_radius,
                      outliers=outliers, normals=normals, seconds=seconds)
    t0 = time.perf_counter()
    ply.write(plyfilename, res["xyz"], res["rgb"], normals=res["normals"])
    tick(seconds, "write", t0)
    res["stats"].update(seconds=seconds, file=plyfilename)
    return res


def clean_ply(ply_in, ply_out, centres=None, k=20, std_ratio=2.0, normal_k=16, max_radius=None, outliers=True, normals=True):
    """A cloud someone brings (any PLY `ply.read_points` reads) -> ply_out.  There is no provenance: with centres (m,3) a
    normal faces the centre nearest to its point, without them it keeps the solver's sign.  -> `clean_cloud`'s dict."""
    seconds = {k_: 0.0 for k_ in PHASES}
    t0 = time.perf_counter()
    xyz, rgb = ply.read_points(ply_in)
    t0 = tick(seconds, "read", t0)
    res = clean_cloud(xyz, rgb, None, centres, k=k, std_ratio=std_ratio, normal_k=normal_k, max_radius=max_radius,
                      outliers=outliers, normals=normals, seconds=seconds)
    t0 = time.perf_counter()
    ply.write(ply_out, res["xyz"], res["rgb"], normals=res["normals"])
    tick(seconds, "write", t0)
    res["stats"].update(seconds=seconds, file=ply_out)
    return res


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Cleans a fused point cloud on the GPU: statistical outlier removal over k nearest "
                                            "neighbours, PCA normals turned towards the cameras -> a PLY with nx ny nz")
    p.add_argument("--scan-folder", default=None, help="holds cams/{id:08}_cam.txt and images/{id:08}.jpg")
    p.add_argument("--out-folder", default=None, help="holds depth_est/ and confidence/ PFMs")
    p.add_argument("--views", type=int, nargs="+", default=None, help="view ids, e.g. 25 22 28")
    p.add_argument("--ply", default=None, help="instead of a scan folder: a point cloud to clean (no provenance)")
    p.add_argument("--ply-out", required=True, help="output file")
    p.add_argument("--k", type=int, default=20, help="neighbours of the outlier score")
    p.add_argument("--std-ratio", type=float, default=2.0, help="kept: score <= mean + std_ratio * std")
    p.add_argument("--normal-k", type=int, default=16, help="neighbours of a normal")
    p.add_argument("--max-radius", type=float, default=None, help="neighbour search radius (default: four grid cells)")
    p.add_argument("--no-outliers", action="store_true", help="keep every point")
    p.add_argument("--no-normals", action="store_true", help="write no normals")
    p.add_argument("--data-dir-root", default=None, help="with --dataset: cut every view by its evaluation mask")
    p.add_argument("--dataset", default=None, choices=("DTU", "BlendedMVS"))
    a = p.parse_args(argv)
    if a.ply is None and (a.scan_folder is None or a.out_folder is None or a.views is None):
        p.error("give --ply IN, or --scan-folder, --out-folder and --views")
    if a.ply is not None and (a.scan_folder is not None or a.out_folder is not None or a.views is not None):
        p.error("--ply excludes --scan-folder, --out-folder and --views")
    if (a.data_dir_root is None) != (a.dataset is None):
        p.error("--data-dir-root and --dataset go together")
    return a


def main(argv=None):
    a = parse_args(argv)
    kw = dict(k=a.k, std_ratio=a.std_ratio, normal_k=a.normal_k, max_radius=a.max_radius, outliers=not a.no_outliers,
              normals=not a.no_normals)
    if a.ply is not None:
        res = clean_ply(a.ply, a.ply_out, **kw)
    else:
        res = clean_folder(a.scan_folder, a.out_folder, a.views, a.ply_out, eval_mask_root=a.data_dir_root, dataset=a.dataset, **kw)
    s = res["stats"]
    print(f"points in {s['points_in']}, points kept {s['points_kept']}, threshold {s['threshold']:.6g}", flush=True)
    print(seconds_line(s["seconds"]), flush=True)
    print(f"saving the cleaned cloud to {s['file']}", flush=True)
    return res


if __name__ == "__main__":
    main()
