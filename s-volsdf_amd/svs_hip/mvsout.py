"""From the MVS network's outputs to the default-config point cloud on the GPU (csrc/svs_mvsout.hip): what the
reference's runner does on the host with OpenCV and scikit-image between `CascadeMVSNet` and `filter_depth`.

    final_confidence(outputs)           conf_1 * conf_2 * photometric_confidence, each resized to the depth map's size
                                        with cv2.resize (INTER_LINEAR) -- the map filter_depth thresholds (runner.py:267-271)
    save_view(out_folder, view, ...)    the files later steps read: depth_est/ and confidence/ PFMs, cams/, images/
                                        (runner.py:261-295 without the colour previews)
    eval_mask(image, H, W, radius=12)   read_img's mask -> last channel -> binary_dilation(disk(12)) -> cv2.resize(.. * 1.,
                                        (W,H)) > 0. (runner.py:362-368), = resize_any(dilate_disk(image != 0), H, W)
    eval_mask_path(root, dataset, scan_name, view)      the file rule of runner.py:351-360

`fusion.filter_depth_folder(..., eval_mask_root=..., dataset=...)` applies the masks, which is the reference's default
configuration (eval_mask: true).  Every operator runs on the device; there is no CPU fallback (`SvsError` without the
library or a GPU).  The dilation and the thresholded resize are boolean functions of their input and bit-exact; the
float32 bilinear resize of the confidence maps is restated and UNPINNED against OpenCV (INTEGRATION.md gives the call to
check it against).  JPEG files are written by PIL at quality 95 (OpenCV's default): the decoded images are close to, not
byte-identical with, what cv2.imwrite stores.

    python -m svs_hip.mvsout --scan-folder S --out-folder O --ply P --views 25 22 28 [--data-dir-root D --dataset DTU]
"""
import argparse
import os

import numpy as np
import torch

from . import lib as _lib
from .images import linear_table, tables_device, to_device
from .ops import _ptr, _stream
from .scans import view_mask_file as eval_mask_path        # the file rule of runner.py:351-360, decided per file

MAX_RADIUS = 32
LAUNCHES = {"dilate": 0, "resize": 0, "confidence": 0}      # entry-point calls made by this process (tests, bench_mvsout.py)
KERNELS_PER_CALL = {"dilate": 3, "resize": 1, "confidence": 1}


def _mask_dev(mask, what):
    """(Hs,Ws) or (V,Hs,Ws) array / tensor of any numeric type -> uint8 device tensor (V,Hs,Ws) of its codes (a bool or
    float input: 1 where non-zero), and whether a view axis was added"""
    t = mask if torch.is_tensor(mask) else np.asarray(mask)
    if "uint8" not in str(t.dtype):
        t = t != 0
    t = to_device(t, torch.uint8, "mvsout", what, ndim=(2, 3), expect="(Hs,Ws) or (V,Hs,Ws)", non_blocking=True)
    single = t.dim() == 2
    return (t[None] if single else t).contiguous(), single


def _tables(H, W, Hs, Ws, dev):
    return [None] * 4 if (Hs, Ws) == (H, W) else tables_device(linear_table, H, W, Hs, Ws, dev)


def dilate_disk(mask, radius=12):
    """skimage.morphology.binary_dilation(mask, disk(radius)) (runner.py:365).  mask: (Hs,Ws) or (V,Hs,Ws), set where
    non-zero -> uint8 device tensor of 0/1, same shape."""
    L = _lib.load()
    d, single = _mask_dev(mask, "mask")
    V, Hs, Ws = d.shape
    out = torch.empty_like(d)
    ws = torch.empty(max(int(L.svs_mask_dilate_workspace_bytes(V, Hs, Ws)), 8) // 8, dtype=torch.int64, device=d.device)
    _lib.check(L.svs_mask_dilate_disk(_ptr(d), V, Hs, Ws, int(radius), _ptr(ws), _ptr(out), _stream()), "svs_mask_dilate_disk")
    LAUNCHES["dilate"] += 1
    return out[0] if single else out


def resize_any(mask, H, W):
    """cv2.resize(mask * 1., (W,H)) > 0. of a 0/1 mask (runner.py:366-368).  mask: (Hs,Ws) or (V,Hs,Ws) -> uint8 device
    tensor of 0/1, (H,W) or (V,H,W)."""
    L = _lib.load()
    H, W = int(H), int(W)
    d, single = _mask_dev(mask, "mask")
    V, Hs, Ws = d.shape
    out = torch.empty(V, max(H, 0), max(W, 0), dtype=torch.uint8, device=d.device)
    tabs = _tables(H, W, Hs, Ws, d.device) if H >= 1 and W >= 1 else [None] * 4
    _lib.check(L.svs_mask_resize_any(_ptr(d), V, Hs, Ws, H, W, *[_ptr(t) for t in tabs], _ptr(out), _stream()),
               "svs_mask_resize_any")
    LAUNCHES["resize"] += 1
    return out[0] if single else out


def eval_mask(image, H, W, radius=12):
    """The evaluation mask of one view as filter_depth applies it (runner.py:362-368).  image: what read_img returns for
    the mask file, or its uint8 codes: (Hs,Ws) or (Hs,Ws,C) -- the last channel is taken.  -> uint8 device tensor (H,W)
    of 0/1, which `fusion.fuse_view(extra_mask=...)` / `fusion.filter_depth(eval_masks=...)` take as it is."""
    a = image if torch.is_tensor(image) else np.asarray(image)
    if a.ndim == 3:
        a = a[:, :, -1]
    if a.ndim != 2:
        raise ValueError(f"image: expected (Hs,Ws) or (Hs,Ws,C), got {tuple(a.shape)}")
    return resize_any(dilate_disk(a, radius), H, W)


def _map_dev(a, what):
    t = a if torch.is_tensor(a) else np.asarray(a)
    if t.ndim == 3:
        t = t[0]                                                  # batch entry 0, like the loop at runner.py:261-262
    return to_device(t, torch.float32, "mvsout", what, ndim=(2,), expect="(H,W) or (B,H,W)")


def confidence_product(conf1, conf2, conf3, H, W):
    """cv2.resize(conf1, (W,H)) * cv2.resize(conf2, (W,H)) * cv2.resize(conf3, (W,H)) (runner.py:267-271): float32 maps of
    any sizes -> float32 device tensor (H,W)."""
    L = _lib.load()
    H, W = int(H), int(W)
    maps = [_map_dev(c, f"conf{k + 1}") for k, c in enumerate((conf1, conf2, conf3))]
    dev = maps[0].device
    out = torch.empty(max(H, 0), max(W, 0), dtype=torch.float32, device=dev)
    args, keep = [], []
    for m in maps:
        tabs = _tables(H, W, m.shape[0], m.shape[1], dev) if H >= 1 and W >= 1 else [None] * 4
        keep.append(tabs)
        args += [_ptr(m), m.shape[0], m.shape[1]] + [_ptr(t) for t in tabs]
    _lib.check(L.svs_mvs_confidence(*args, H, W, _ptr(out), _stream()), "svs_mvs_confidence")
    LAUNCHES["confidence"] += 1
    return out


def final_confidence(outputs):
    """outputs: the dict CascadeMVSNet returns for one view (device tensors or arrays).  -> conf_final of runner.py:267-271,
    float32 device tensor of the depth map's size: outputs['stage1'] / ['stage2'] / the top-level
    'photometric_confidence', batch entry 0, resized to the top-level map's size and multiplied."""
    c3 = _map_dev(outputs["photometric_confidence"], "photometric_confidence")
    H, W = _map_dev(outputs["depth"], "depth").shape if "depth" in outputs else c3.shape
    return confidence_product(outputs["stage1"]["photometric_confidence"], outputs["stage2"]["photometric_confidence"], c3,
                              H, W)


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def save_view(out_folder, view, outputs, cam, img, cam_near_far=None):
    """The files of one view that later steps read (runner.py:261-295): depth_est/{view:08}.pfm (outputs['depth'], batch
    entry 0), confidence/{view:08}.pfm (`final_confidence`), cams/{view:08}_cam.txt (cam: (2,4,4) extrinsic, intrinsic),
    images/{view:08}.jpg (img: (3,H,W) float in [0,1]; clip(img * 255, 0, 255) as uint8, JPEG quality 95).  The colour
    previews of the reference (depth_est*.png, confidence_final.png) are not written: nothing reads them.
    -> dict of the four file names."""
    from datasets.data_io import save_pfm
    from helpers.utils import write_cam
    from PIL import Image
    names = {k: os.path.join(out_folder, k, "{:0>8}{}".format(view, ext))
             for k, ext in (("depth_est", ".pfm"), ("confidence", ".pfm"), ("cams", "_cam.txt"), ("images", ".jpg"))}
    for f in names.values():
        os.makedirs(os.path.dirname(f), exist_ok=True)
    depth = _host(outputs["depth"]).astype(np.float32, copy=False)
    save_pfm(names["depth_est"], depth[0] if depth.ndim == 3 else depth)
    save_pfm(names["confidence"], final_confidence(outputs).cpu().numpy())
    write_cam(names["cams"], _host(cam), cam_near_far)
    rgb = np.clip(np.transpose(_host(img), (1, 2, 0)) * 255, 0, 255).astype(np.uint8)
    Image.fromarray(rgb).save(names["images"], quality=95)
    return names


def folder_eval_masks(eval_mask_root, dataset, scan_name, views, shapes, radius=12):
    """{view: eval_mask of its file, resized to shapes[view]} -- what filter_depth_folder hands to filter_depth"""
    from helpers.utils import read_img
    return {v: eval_mask(read_img(eval_mask_path(eval_mask_root, dataset, scan_name, v)), *shapes[v], radius=radius)
            for v in views}


def main(argv=None):
    p = argparse.ArgumentParser(description="The reference's filter_only run for one scan: fuses the depth maps of a scan "
                                            "folder into a PLY, with the evaluation masks when --data-dir-root is given.")
    p.add_argument("--scan-folder", required=True, help="holds cams/{view:08}_cam.txt and images/{view:08}.jpg")
    p.add_argument("--out-folder", required=True, help="holds depth_est/ and confidence/ PFMs; its last component names the scan")
    p.add_argument("--ply", required=True)
    p.add_argument("--views", type=int, nargs="+", required=True)
    p.add_argument("--data-dir-root", help="holds <dataset>/eval_mask/<scan>/...: apply the evaluation masks (eval_mask: true)")
    p.add_argument("--dataset", choices=("DTU", "BlendedMVS"), help="with --data-dir-root")
    p.add_argument("--conf", type=float, default=0.0)
    p.add_argument("--filter-dist", type=float, default=1)
    p.add_argument("--filter-diff", type=float, default=0.01)
    p.add_argument("--thres-view", type=int, default=1)
    p.add_argument("--eval-mask-radius", type=int, default=12)
    a = p.parse_args(argv)
    if a.data_dir_root and not a.dataset:
        p.error("--data-dir-root needs --dataset")
    from . import fusion
    xyz, _, stats = fusion.filter_depth_folder(a.scan_folder, a.out_folder, a.ply, a.views, conf=a.conf,
                                               filter_dist=a.filter_dist, filter_diff=a.filter_diff, thres_view=a.thres_view,
                                               eval_mask_root=a.data_dir_root, dataset=a.dataset,
                                               eval_mask_radius=a.eval_mask_radius)
    for v, photo, geo, final in stats:
        print("processing {}, ref-view{:0>2}, photo/geo/final-mask:{:.3f}/{:.3f}/{:.3f}".format(a.scan_folder, v, photo, geo, final))
    print(f"saving the final MVS result to {a.ply}: {len(xyz)} points")


if __name__ == "__main__":
    main()
