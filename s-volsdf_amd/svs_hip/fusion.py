"""Depth-map fusion on the HIP path (csrc/svs_fusion.hip).

`fuse_view` is one iteration of the reference's filter_depth loop (runner.py:312-386): geometric consistency of a
reference view against its source views, photometric mask, depth averaging and the coloured world-space points of the
surviving pixels.  `filter_depth` is the whole function on in-memory views or on a scan folder, ending in the same
binary PLY (`ply.write`).  The small camera matrices are formed on the host exactly as the reference forms them
(float32 inverses / products), everything per pixel runs on the GPU.
"""
import os

import numpy as np
import torch

from . import lib as _lib
from . import ply
from .images import device, to_device
from .ops import _ptr, _ptr_array, _stream


def pair_matrices(K_ref, E_ref, K_src, E_src):
    """The six matrices of reproject_with_depth (helpers/utils.py:82-111) for one (ref, src) pair, float64 (68,):
    inv(K_ref), E_src @ inv(E_ref), K_src, inv(K_src), E_ref @ inv(E_src), K_ref.  Inverses and products are taken
    in the dtype of the inputs (float32 from read_camera_parameters), as numpy does in the reference."""
    K_ref, E_ref, K_src, E_src = (np.asarray(m) for m in (K_ref, E_ref, K_src, E_src))
    mats = (np.linalg.inv(K_ref), np.matmul(E_src, np.linalg.inv(E_ref)), K_src, np.linalg.inv(K_src),
            np.matmul(E_ref, np.linalg.inv(E_src)), K_ref)
    return np.concatenate([np.asarray(m, np.float64).reshape(-1) for m in mats])


def fuse_view(ref, srcs, conf=0.0, filter_dist=1, filter_diff=0.01, thres_view=1, extra_mask=None, per_source=False,
              points=True):
    """ref / srcs[i]: dict(K (3,3), E (4,4), depth (H,W) [, confidence (H,W), img (H,W,3) float32 in [0,1]]); arrays or
    device tensors.  Returns device tensors: depth_avg (H,W) float64, photo_mask / geo_mask / final_mask (H,W) uint8,
    and with points=True xyz (n,3) float32, rgb (n,3) uint8 (row-major order of the surviving pixels); with
    per_source=True also src_mask, src_depth_reproj, src_x, src_y (n_src,H,W)."""
    L = _lib.load()
    dev = device("fusion")
    depth = to_device(ref["depth"], torch.float32, "fusion")
    H, W = depth.shape
    confidence = to_device(ref["confidence"], torch.float32, "fusion") if "confidence" in ref else torch.full((H, W), float("inf"), device=dev)
    n_src = len(srcs)
    src_depths = [to_device(s["depth"], torch.float32, "fusion") for s in srcs]
    for d in src_depths:
        if tuple(d.shape) != (H, W):
            raise AssertionError("source depth map shape differs from the reference view's")     # runner.py:334
    per = L.svs_fuse_mats_per_src()
    mats = np.zeros((max(n_src, 1), per), np.float64)
    for v, s in enumerate(srcs):
        mats[v] = pair_matrices(ref["K"], ref["E"], s["K"], s["E"])
    mats_d = torch.from_numpy(mats).to(dev)
    out = dict(depth_avg=torch.empty(H, W, dtype=torch.float64, device=dev))
    for k in ("photo_mask", "geo_mask", "final_mask"):
        out[k] = torch.empty(H, W, dtype=torch.uint8, device=dev)
    if per_source:
        out["src_mask"] = torch.empty(n_src, H, W, dtype=torch.uint8, device=dev)
        for k in ("src_depth_reproj", "src_x", "src_y"):
            out[k] = torch.empty(n_src, H, W, dtype=torch.float32, device=dev)
    em = None if extra_mask is None else (to_device(extra_mask, torch.float32, "fusion") > 0).to(torch.uint8).contiguous()
    _lib.check(L.svs_fuse_view(_ptr(depth), _ptr(confidence), _ptr_array(src_depths), _ptr(mats_d), n_src, H, W,
                               float(conf), float(filter_dist), float(filter_diff), int(thres_view), _ptr(em),
                               _ptr(out["depth_avg"]), _ptr(out["photo_mask"]), _ptr(out["geo_mask"]), _ptr(out["final_mask"]),
                               _ptr(out.get("src_mask")), _ptr(out.get("src_depth_reproj")), _ptr(out.get("src_x")),
                               _ptr(out.get("src_y")), _stream()), "svs_fuse_view")
    if points:
        K, E = np.asarray(ref["K"]), np.asarray(ref["E"])
        pm = np.concatenate([np.asarray(np.linalg.inv(K), np.float64).reshape(-1), np.asarray(np.linalg.inv(E), np.float64).reshape(-1)])
        pm_d = torch.from_numpy(pm).to(dev)
        img = to_device(ref["img"], torch.float32, "fusion") if "img" in ref else None
        if img is not None and tuple(img.shape) != (H, W, 3):
            raise AssertionError("reference image shape differs from its depth map's")            # runner.py:322
        ws = torch.empty(H * W, dtype=torch.int32, device=dev)
        xyz = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
        rgb = torch.empty(H * W, 3, dtype=torch.uint8, device=dev) if img is not None else None
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.svs_fuse_points(_ptr(out["depth_avg"]), _ptr(out["final_mask"]), _ptr(img), _ptr(pm_d), H, W, _ptr(ws),
                                     _ptr(xyz), _ptr(rgb), _ptr(count), _stream()), "svs_fuse_points")
        n = int(count.item())
        out["xyz"] = xyz[:n]
        if rgb is not None:
            out["rgb"] = rgb[:n]
    return out


def fuse_views(views, pairs, eval_masks=None, **kw):
    """(ref_view, fuse_view's dict) per pair of `pairs` = [(ref_view, [src_view, ...]), ...], every reference view cut by
    its entry of eval_masks when there are any; kw: fuse_view's settings"""
    for ref_view, src_views in pairs:
        yield ref_view, fuse_view(views[ref_view], [views[s] for s in src_views],
                                  extra_mask=None if eval_masks is None else eval_masks[ref_view], **kw)


def filter_depth(views, pairs, conf=0.0, filter_dist=1, filter_diff=0.01, thres_view=1, plyfilename=None, eval_masks=None,
                 mask_dir=None):
    """filter_depth (runner.py:301-401) on in-memory views.  views: {view_id: dict(K, E, img, depth, confidence)},
    pairs: [(ref_view, [src_view, ...]), ...] (runner.py:303-305 builds all-vs-all pairs of the training views),
    eval_masks: optional {view_id: (H,W) mask}, dilated and resized (runner.py:349-368): arrays, or the device tensors of
    `svs_hip.mvsout.eval_mask`, which does both on the GPU.
    Returns (vertices (n,3) float32, colours (n,3) uint8, per-view stats); writes the PLY if plyfilename is given and
    the three masks per view under mask_dir."""
    from helpers.utils import save_mask
    vertexs, colors, stats = [], [], []
    for ref_view, out in fuse_views(views, pairs, eval_masks, conf=conf, filter_dist=filter_dist, filter_diff=filter_diff,
                                    thres_view=thres_view):
        vertexs.append(out["xyz"])
        colors.append(out["rgb"])
        m = torch.stack([out[k].float().mean() for k in ("photo_mask", "geo_mask", "final_mask")]).cpu().numpy()
        stats.append((ref_view, float(m[0]), float(m[1]), float(m[2])))
        if mask_dir is not None:
            os.makedirs(mask_dir, exist_ok=True)
            for k, tag in (("photo_mask", "photo"), ("geo_mask", "geo"), ("final_mask", "final")):
                save_mask(os.path.join(mask_dir, "{:0>8}_{}.png".format(ref_view, tag)), out[k].cpu().numpy().astype(bool))
    xyz = torch.cat(vertexs, 0).cpu().numpy() if vertexs else np.zeros((0, 3), np.float32)
    rgb = torch.cat(colors, 0).cpu().numpy() if colors else np.zeros((0, 3), np.uint8)
    if plyfilename is not None:
        ply.write(plyfilename, xyz, rgb)
    return xyz, rgb, stats


def folder_views(scan_folder, out_folder, view_ids):
    """{view: dict(K, E, img, depth, confidence)} of a scan folder: cams/{id:08}_cam.txt and images/{id:08}.jpg under
    scan_folder, depth_est/ and confidence/ PFMs under out_folder (runner.py:312-332)"""
    from datasets.data_io import read_pfm
    from helpers.utils import read_camera_parameters, read_img
    views = {}
    for v in view_ids:
        K, E = read_camera_parameters(os.path.join(scan_folder, "cams/{:0>8}_cam.txt".format(v)))
        views[v] = dict(K=K, E=E, img=read_img(os.path.join(scan_folder, "images/{:0>8}.jpg".format(v))),
                        depth=np.ascontiguousarray(read_pfm(os.path.join(out_folder, "depth_est/{:0>8}.pfm".format(v)))[0]),
                        confidence=np.ascontiguousarray(read_pfm(os.path.join(out_folder, "confidence/{:0>8}.pfm".format(v)))[0]))
    return views


def scan_inputs(scan_folder, out_folder, view_ids, eval_mask_root=None, dataset=None, eval_mask_radius=12):
    """What a fused scan folder gives -> (views: `folder_views`, pairs: every view against all the others, eval_masks).
    eval_masks: None without eval_mask_root (the reference's data_dir_root; `dataset` 'DTU' or 'BlendedMVS'), else per view
    the file of `svs_hip.mvsout.eval_mask_path` for the scan named by out_folder's last component, dilated by
    disk(eval_mask_radius) and resized to the depth map on the GPU (runner.py:350-368)."""
    view_ids = list(view_ids)
    views = folder_views(scan_folder, out_folder, view_ids)
    pairs = [(v, [x for x in view_ids if x != v]) for v in view_ids]
    eval_masks = None
    if eval_mask_root is not None:
        from . import mvsout
        scan_name = os.path.normpath(out_folder).split(os.sep)[-1]
        eval_masks = mvsout.folder_eval_masks(eval_mask_root, dataset, scan_name, view_ids,
                                              {v: views[v]["depth"].shape for v in view_ids}, radius=eval_mask_radius)
    return views, pairs, eval_masks


def filter_depth_folder(scan_folder, out_folder, plyfilename, view_ids, conf=0.0, filter_dist=1, filter_diff=0.01,
                        thres_view=1, *, eval_mask_root=None, dataset=None, eval_mask_radius=12):
    """The file-level form (runner.py:301-332): cams/{id:08}_cam.txt and images/{id:08}.jpg under scan_folder,
    depth_est/ and confidence/ PFMs under out_folder; all-vs-all pairs of view_ids.  With eval_mask_root every view's
    final mask is cut by its evaluation mask, as with the reference's default eval_mask: true (`scan_inputs`)."""
    views, pairs, eval_masks = scan_inputs(scan_folder, out_folder, view_ids, eval_mask_root, dataset, eval_mask_radius)
    return filter_depth(views, pairs, conf, filter_dist, filter_diff, thres_view, plyfilename, eval_masks=eval_masks,
                        mask_dir=os.path.join(out_folder, "mask"))
