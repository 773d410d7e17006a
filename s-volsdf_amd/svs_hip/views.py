"""The shared parts of `tsdf`, `meshview`, `meshpaint` and `meshtexture`: a view's matrices as the kernels of csrc/svs_views.h read
them, the launch chunks, the checked upload of masks and of a mesh, a scan folder's cameras, photographs and evaluation masks (all of
them with the mesh file: `scan_folder_inputs`), the command lines' evaluation-mask options.  Host code only; nothing here launches a kernel."""
import os

import numpy as np
import torch

from . import ply
from .images import read_rgb8, to_device

MAX_VIEWS = 16                       # views per launch (csrc/svs_views.h kMaxViews)


def view_matrices(K, E):
    """(21,) float64: K row-major, then the top three rows of E"""
    K, E = np.asarray(K, np.float64), np.asarray(E, np.float64)
    if K.shape != (3, 3) or E.shape != (4, 4):
        raise ValueError(f"a view has K (3,3) and E (4,4), got {K.shape} and {E.shape}")
    return np.concatenate([K.reshape(-1), E[:3].reshape(-1)])


def mats(views, dev):
    return torch.from_numpy(np.ascontiguousarray(np.stack([view_matrices(v["K"], v["E"]) for v in views]))).to(dev)


def chunks(views, dev):
    """yields (at, to, mats of views[at:to] on dev) per launch of at most MAX_VIEWS views"""
    for at in range(0, len(views), MAX_VIEWS):
        to = min(at + MAX_VIEWS, len(views))
        yield at, to, mats(views[at:to], dev)


def device_masks(masks, n_views, H, W, dev, name, error=ValueError):
    """per view None or an (H,W) array, non-zero = inside -> uint8 tensors of 0 / 1 on dev; `error` names the entry `name`"""
    if masks is None:
        return None
    out = [m if m is None else (torch.as_tensor(m).to(dev) != 0).to(torch.uint8).contiguous() for m in masks]
    for m in out:
        if m is not None and tuple(m.shape) != (H, W):
            raise error(f"{name}: a mask of {tuple(m.shape)} for views of {(H, W)}")
    if len(out) != n_views:
        raise error(f"{name}: {len(out)} masks for {n_views} views")
    return out


def mesh_args(verts, faces, colors=None):
    """arrays or tensors -> verts (V,3) float32, faces (F,3) int32, colors (V,3) uint8 or None, contiguous on the GPU"""
    verts = to_device(verts, torch.float32, "views", "verts")
    faces = to_device(faces, torch.int32, "views", "faces")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"a mesh is verts (V,3) and faces (F,3), got {tuple(verts.shape)} and {tuple(faces.shape)}")
    if colors is not None:
        colors = to_device(colors, torch.uint8, "views", "colors")
        if tuple(colors.shape) != (verts.shape[0], 3):
            raise ValueError(f"svs_mesh_raster_resolve: {tuple(colors.shape)} colours for {verts.shape[0]} vertices")
    return verts, faces, colors


def folder_cameras(scan_folder, view_ids):
    """[dict(K, E)] from cams/{id:08}_cam.txt"""
    from helpers.utils import read_camera_parameters
    cams = (read_camera_parameters(os.path.join(scan_folder, "cams/{:0>8}_cam.txt".format(v))) for v in view_ids)
    return [dict(K=K, E=E) for K, E in cams]


def folder_images(scan_folder, view_ids):
    """[(H,W,3) uint8] from images/{id:08}.jpg at their own size; ValueError when the sizes differ"""
    out = [read_rgb8(os.path.join(scan_folder, "images/{:0>8}.jpg".format(v))) for v in view_ids]
    sizes = sorted({im.shape[:2] for im in out})
    if len(sizes) > 1:
        raise ValueError(f"svs_mesh_paint: the views have different sizes {sizes}")
    return out


def folder_size(scan_folder, view_ids, name):
    """(H, W) of images/{id:08}.jpg, read from the headers alone; ValueError in `name` when the sizes differ"""
    from PIL import Image
    sizes = set()
    for v in view_ids:
        with Image.open(os.path.join(scan_folder, "images/{:0>8}.jpg".format(v))) as im:
            sizes.add((im.height, im.width))
    if len(sizes) != 1:
        raise ValueError(f"{name}: the views have different sizes {sorted(sizes)}")
    return sizes.pop()


def folder_masks(eval_mask_root, dataset, scan_name, view_ids, H, W, radius):
    """the evaluation masks of `mvsout.folder_eval_masks` as a per-view list, or None when eval_mask_root is None"""
    if eval_mask_root is None:
        return None
    from . import mvsout
    by_view = mvsout.folder_eval_masks(eval_mask_root, dataset, scan_name, view_ids, {v: (H, W) for v in view_ids}, radius=radius)
    return [by_view[v] for v in view_ids]


def scan_folder_inputs(ply_file, scan_folder, view_ids, eval_mask_root, dataset, eval_mask_radius):
    """The mesh file (`ply.read_mesh_colors`), the cameras and photographs of view_ids and their evaluation masks under the scan's
    name, the last component of scan_folder -> verts, faces, colors or None, views, images, masks or None, (H, W): host arrays"""
    verts, faces, colors = ply.read_mesh_colors(ply_file)
    views, images = folder_cameras(scan_folder, view_ids), folder_images(scan_folder, view_ids)
    H, W = images[0].shape[:2]
    masks = folder_masks(eval_mask_root, dataset, os.path.normpath(scan_folder).split(os.sep)[-1], view_ids, H, W, eval_mask_radius)
    return verts, faces, colors, views, images, masks, (H, W)


def add_eval_mask_args(parser, effect):
    parser.add_argument("--data-dir-root", default=None, help=f"with --dataset: {effect}")
    parser.add_argument("--dataset", default=None, choices=("DTU", "BlendedMVS"))


def check_eval_mask_args(parser, args):
    if (args.data_dir_root is None) != (args.dataset is None):
        parser.error("--data-dir-root and --dataset come together")


def launches_since(entry_calls, before):
    return {k: entry_calls[k] - before[k] for k in entry_calls}
