"""Image-based rendering of evaluation views on the HIP path (simple_ibr.py:116-235; csrc/svs_ibr.hip).

`blend_view` is one iteration of the reference's image_based_render loop: the source (training) images warped into an
evaluation view through the rendered depths, weighted by geometric consistency and ray-direction agreement, and
Laplacian-blended with the volume render of that view.  `image_based_render` is the file-level form that writes the
eval_blend_XXX.png files the evaluation scores with --result_from blend.  The geometry reuses svs_fuse_view (float64,
per-source maps and masks) and svs_rays_from_uv (the reference's get_dir_loc); the small camera matrices are formed on
the host as the reference forms them.

    python -m svs_hip.ibr --scan-folder SCAN --out-folder RENDERING --ref-views 23 24 --src-views 25 22 28
"""
import argparse
import os

import numpy as np
import torch

from . import lib as _lib
from .fusion import fuse_view
from .images import device, to_device
from .ops import _ptr, _ptr_array, _stream

_UV = {}


def _shape(a):
    return tuple(a.shape)


def _uv_grid(H, W):
    """(H*W, 2) float32 pixel (x, y) at integer positions, row-major (get_dir_loc's flipped mgrid); cached per size."""
    key = (H, W, torch.cuda.current_device())
    if key not in _UV:
        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
        _UV[key] = torch.from_numpy(np.stack([x.ravel(), y.ravel()], 1)).to(device("ibr"))
    return _UV[key]


def ray_dirs(K, E, H, W):
    """get_dir_loc (simple_ibr.py:75-88): unit ray directions (H,W,3) float32 of the camera at every integer pixel.
    pose = inv(E) in float32 and the intrinsics in a 4x4, as the reference forms them."""
    L = _lib.load()
    dev = device("ibr")
    intr = np.eye(4)
    intr[:3, :3] = np.asarray(K)
    pose = np.linalg.inv(np.asarray(E, np.float32))
    pose_d = torch.from_numpy(np.ascontiguousarray(pose, np.float32)).to(dev)
    intr_d = torch.from_numpy(intr.astype(np.float32)).to(dev)
    dirs = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    cam = torch.empty(3, dtype=torch.float32, device=dev)
    ds = torch.empty(H * W, dtype=torch.float32, device=dev)
    _lib.check(L.svs_rays_from_uv(_ptr(_uv_grid(H, W)), _ptr(pose_d), _ptr(intr_d), H * W, _ptr(dirs), _ptr(cam), _ptr(ds),
                                  _stream()), "svs_rays_from_uv")
    return dirs


def check_shapes(ref, srcs, pred_img):
    """The shape rules of blend_view, checked before any GPU work: (H, W) for every depth map, (H, W, 3) for the images,
    1..16 sources, H and W positive multiples of 8 (Laplacian_Blending's pyramids need them)."""
    H, W = _shape(ref["depth"])
    if not 1 <= len(srcs) <= 16:
        raise ValueError(f"image-based rendering takes 1..16 source views, got {len(srcs)}")
    for s in srcs:
        if _shape(s["depth"]) != (H, W):
            raise AssertionError("source depth map shape differs from the reference view's")       # simple_ibr.py:170
        if _shape(s["img"]) != (H, W, 3):
            raise AssertionError("source image shape differs from the reference view's depth map")
    if _shape(pred_img) != (H, W, 3):
        raise AssertionError("the rendered image's shape differs from the reference view's depth map")
    if H < 8 or W < 8 or H % 8 or W % 8:
        raise ValueError(f"Laplacian blending needs H and W to be multiples of 8, got {(H, W)}")
    return H, W


def blend_view(ref, srcs, pred_img, return_stages=False):
    """One evaluation view of image_based_render (simple_ibr.py:150-235).  ref / srcs[i]: dict(K (3,3), E (4,4),
    depth (H,W)), srcs[i] also img (H,W,3) float32 in [0,1]; pred_img: the view's rendered RGB (H,W,3) float32.
    Arrays or device tensors.  -> device (H,W,3) float32 blend in [0,1]; with return_stages also the fusion outputs,
    the fill images (n+1,H,W,3) and masks (n+1,H,W)."""
    H, W = check_shapes(ref, srcs, pred_img)
    L = _lib.load()
    dev = device("ibr")
    n = len(srcs)
    geo = fuse_view(ref, srcs, filter_dist=2, per_source=True, points=False)
    ref_dir = ray_dirs(ref["K"], ref["E"], H, W)
    src_dirs = [ray_dirs(s["K"], s["E"], H, W) for s in srcs]
    src_imgs = [to_device(s["img"], torch.float32, "ibr") for s in srcs]
    pred = to_device(pred_img, torch.float32, "ibr")
    ws = torch.empty(int(L.svs_ibr_workspace_bytes(n, H, W)), dtype=torch.uint8, device=dev)
    fill = torch.empty(n + 1, H, W, 3, dtype=torch.float32, device=dev)
    masks = torch.empty(n + 1, H, W, dtype=torch.float32, device=dev)
    out = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    _lib.check(L.svs_ibr_weights(_ptr_array(src_imgs), _ptr_array(src_dirs), _ptr(ref_dir), _ptr(pred), _ptr(geo["src_mask"]),
                                 _ptr(geo["src_x"]), _ptr(geo["src_y"]), n, H, W, _ptr(ws), _ptr(fill), _ptr(masks),
                                 _stream()), "svs_ibr_weights")
    _lib.check(L.svs_ibr_laplacian_blend(_ptr(fill), _ptr(masks), n, H, W, _ptr(ws), _ptr(out), _stream()),
               "svs_ibr_laplacian_blend")
    if return_stages:
        return out, dict(geo, fill=fill, masks=masks, ref_dir=ref_dir, src_dirs=src_dirs)
    return out


def to_png_array(blend):
    """(blend_image * 255).astype(np.uint8) of simple_ibr.py:232 (the reference's blend is float64)."""
    b = blend.cpu().numpy() if torch.is_tensor(blend) else np.asarray(blend)
    return (b.astype(np.float64) * 255).astype(np.uint8)


def image_based_render(scan_folder, out_folder, ref_views, src_views):
    """image_based_render (simple_ibr.py:150-235) for explicit view ids: reads cams/{:08d}_cam.txt and
    images/{:08d}.png under scan_folder, eval_{:03d}.png and depth_est/{:08d}.pfm under out_folder, and writes
    out_folder/eval_blend_{:03d}.png for every reference view.  Returns the written paths."""
    from PIL import Image
    from datasets.data_io import read_pfm
    from helpers.utils import read_camera_parameters, read_img

    def cam(v):
        return read_camera_parameters(os.path.join(scan_folder, "cams/{:0>8}_cam.txt".format(v)))

    def depth(v):
        return np.ascontiguousarray(read_pfm(os.path.join(out_folder, "depth_est/{:0>8}.pfm".format(v)))[0])

    srcs = []
    for v in src_views:
        K, E = cam(v)
        srcs.append(dict(K=K, E=E, depth=depth(v), img=read_img(os.path.join(scan_folder, "images/{:0>8}.png".format(v)))))
    written = []
    for v in ref_views:
        K, E = cam(v)
        pred = read_img(os.path.join(out_folder, "eval_{:0>3}.png".format(v)))
        blend = blend_view(dict(K=K, E=E, depth=depth(v)), srcs, pred)
        fn = os.path.join(out_folder, "eval_blend_{:0>3}.png".format(v))
        Image.fromarray(to_png_array(blend)).save(fn)
        written.append(fn)
    return written


def main(argv=None):
    p = argparse.ArgumentParser(description="GPU image-based rendering of evaluation views (the reference's simple_ibr.py): "
                                            "writes OUT_FOLDER/eval_blend_XXX.png for every reference view.")
    p.add_argument("--scan-folder", required=True, help="holds cams/{:08d}_cam.txt and images/{:08d}.png")
    p.add_argument("--out-folder", required=True, help="holds eval_{:03d}.png and depth_est/{:08d}.pfm; receives the blends")
    p.add_argument("--ref-views", type=int, nargs="+", required=True, help="evaluation view ids")
    p.add_argument("--src-views", type=int, nargs="+", required=True, help="training view ids (1..16)")
    a = p.parse_args(argv)
    for fn in image_based_render(a.scan_folder, a.out_folder, a.ref_views, a.src_views):
        print(fn)


if __name__ == "__main__":
    main()
