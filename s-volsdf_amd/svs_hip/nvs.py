"""Novel-view scores on the HIP path (eval_vsdf.py:186-212, `--result_from blend|default`; csrc/svs_nvs.hip).

`score_views` is the reference's masked PSNR and scikit-image 0.17.2 SSIM for a stack of evaluation views in one
`svs_nvs_score` call.  `load_gt` reads the ground truth and masks the reference's SceneDataset reads for those views, and
`score_scan` scores the eval_blend_XXX.png (or eval_XXX.png) files of one scan.  The view ids are explicit: the
reference's id tables stay in its dataset module.  LPIPS, the reference's third metric, is svs_hip.lpips: it is computed
and printed when the two public weight files are given (--lpips-vgg / --lpips-lin), not otherwise.

    python -m svs_hip.nvs --data-dir-root data_s_volsdf --dataset DTU --scan 106 \\
        --rendering-dir exps_result/ours_106/rendering_1562 --views 1 2 9 --result-from blend [--json scores.json] \\
        [--lpips-vgg vgg16.pth --lpips-lin vgg_lin.pth]
"""
import argparse
import json
import os

import numpy as np
import torch

from . import lib as _lib
from .images import alpha_inside, read_bmvs_alpha, read_dtu_mask, read_rgb8, to_device
from .scans import DATASETS, DTU_UNMASKED_SCANS, IMG_RES, glob_images, scan_mask_files
from .ops import _ptr, _stream

def score_views(pred, gt, mask):
    """pred, gt: (V,H,W,3) uint8 codes (the rendered PNGs, the 8-bit ground truth); mask: (V,H,W,3) uint8, nonzero
    inside.  Arrays or tensors, host or device.  -> psnr[V], ssim[V] float64 numpy: the reference's masked PSNR over the
    whole image (+inf for a perfect match, NaN for an empty mask) and SSIM of the white-composited images."""
    shape = tuple(pred.shape)
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError(f"expected (V,H,W,3) images, got {shape}")
    if tuple(gt.shape) != shape or tuple(mask.shape) != shape:
        raise ValueError(f"pred {shape}, gt {tuple(gt.shape)} and mask {tuple(mask.shape)} differ")
    V, H, W, _ = shape
    if V < 1 or H < 7 or W < 7:
        raise ValueError(f"need at least one view of at least 7x7 pixels (the SSIM window), got {shape}")
    L = _lib.load()
    p, g, m = (to_device(a, torch.uint8, "nvs", what, cast=False) for a, what in ((pred, "pred"), (gt, "gt"), (mask, "mask")))
    ws = torch.empty(int(L.svs_nvs_workspace_bytes(V, H, W)), dtype=torch.uint8, device=p.device)
    out = torch.empty(V, 3, dtype=torch.float64, device=p.device)
    _lib.check(L.svs_nvs_score(_ptr(p), _ptr(g), _ptr(m), V, H, W, _ptr(ws), _ptr(out), _stream()), "svs_nvs_score")
    res = out.cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        psnr = -10.0 * np.log10(res[:, 0] / (255.0 * 255.0) / res[:, 1])
    return psnr, res[:, 2].copy()


def _check_size(a, img_res, path):
    if tuple(a.shape[:2]) != tuple(img_res):
        raise NotImplementedError(f"{path}: {a.shape[:2]} differs from img_res {tuple(img_res)}; the reference resizes it "
                                  f"with cv2.resize, which is not ported")


def _gt_from_scene(scene, views, img_res, mask):
    """gt codes and masks of `views` from a loaded svs_hip.scene.SceneDataset (its images are float32 (H*W,3) in the
    reference's units; a native-size image is code * (1/255), so rint(rgb * 255) is the file's code exactly)."""
    H, W = int(img_res[0]), int(img_res[1])
    if (int(scene.img_res[0]), int(scene.img_res[1])) != (H, W):
        raise ValueError(f"the dataset was loaded at {tuple(scene.img_res)}, img_res is {(H, W)}")
    gts, masks = [], []
    for v in views:
        v = int(v)
        if not 0 <= v < scene.n_images:
            raise IndexError(f"view {v}: the scan holds {scene.n_images} images")
        rgb = scene.rgb_images[v].numpy().astype(np.float64).reshape(H, W, 3)
        gts.append(np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8))
        if mask:
            masks.append((scene.masks[v].numpy().reshape(H, W, 3) == 1.0).astype(np.uint8))
        else:
            masks.append(np.ones((H, W, 3), np.uint8))
    return np.stack(gts), np.stack(masks)


def load_gt(data_dir_root, dataset, scan, views, img_res=IMG_RES, mask=None, scene=None):
    """The ground truth and masks SceneDataset (scene_dataset.py:113-206) holds for the given views of one scan.
    -> gt (V,H,W,3) uint8 codes (load_rgb's values are code / 255), mask (V,H,W,3) uint8 0/1.

    Image v is file number v of sorted(glob_imgs({root}/{dataset}/scan{scan}/image)), 8-bit RGB.  Masks: DTU reads
    eval_mask/scan{S}/mask/{v:03d}.png (or eval_mask/scan{S}/{v:03d}.png when mask/000.png does not exist, decided once
    for the scan), inside where a channel is 255; BlendedMVS reads eval_mask/scan{S}/mask/{v:08d}.png (RGBA), inside
    where alpha / 255 > 0.5, for all three channels.  mask=None follows the reference: masked, except the DTU scans
    1, 4, 11, 13 and 48 (all ones); True / False force it.  The views are the scored (evaluation) views: the reference
    reads DTU masks only for its evaluation ids and BlendedMVS masks for its evaluation and training ids.

    scene: a svs_hip.scene.SceneDataset of that scan loaded at img_res.  Images and masks are then taken from it instead
    of the files, which covers ground truth that is not stored at img_res (the dataset resizes it as the reference does).
    The scorer works on 8-bit codes: a resized image is rounded to the nearest code (at most 0.5 / 255 from the float
    ground truth the reference scores against); a native-size image gives the file's codes exactly."""
    if dataset not in DATASETS:
        raise NotImplementedError(f"dataset {dataset!r}: only {DATASETS}")
    scan = int(scan)
    if scene is not None:
        if mask is None:
            mask = not (dataset == "DTU" and scan in DTU_UNMASKED_SCANS)
        return _gt_from_scene(scene, views, img_res, mask)
    inst = os.path.join(data_dir_root, dataset, f"scan{scan}")
    paths = glob_images(os.path.join(inst, "image"))
    if mask is None:
        mask = not (dataset == "DTU" and scan in DTU_UNMASKED_SCANS)
    mask_fn = scan_mask_files(data_dir_root, dataset, scan)
    H, W = img_res
    gts, masks = [], []
    for v in views:
        v = int(v)
        if not 0 <= v < len(paths):
            raise IndexError(f"view {v}: {inst}/image holds {len(paths)} images")
        img = read_rgb8(paths[v])
        _check_size(img, img_res, paths[v])
        gts.append(img)
        if not mask:
            masks.append(np.ones((H, W, 3), np.uint8))
            continue
        fn = mask_fn(v)
        if dataset == "DTU":
            m = read_dtu_mask(fn)                                                # per channel: they need not agree here
            _check_size(m, img_res, fn)
            masks.append(m.astype(np.uint8))
        else:
            m = read_bmvs_alpha(fn)
            _check_size(m, img_res, fn)
            masks.append(np.repeat(alpha_inside(m)[:, :, None], 3, axis=2).astype(np.uint8))
    return np.stack(gts), np.stack(masks)


def prediction_path(rendering_dir, view, result_from="blend"):
    """eval_blend_{v:03d}.png for 'blend', eval_{v:03d}.png for 'default' (eval_vsdf.py:191-194)"""
    if result_from == "blend":
        return os.path.join(rendering_dir, f"eval_blend_{int(view):03d}.png")
    if result_from == "default":
        return os.path.join(rendering_dir, f"eval_{int(view):03d}.png")
    raise NotImplementedError(f"result_from {result_from!r}: 'blend' or 'default'")


def score_scan(rendering_dir, data_dir_root, dataset, scan, views, result_from="blend", img_res=IMG_RES, mask=None,
               scene=None, lpips=None):
    """Scores the rendered views of one scan against its ground truth (eval_vsdf.py:186-212 for explicit view ids).
    scene: see load_gt.  lpips: a svs_hip.lpips.LpipsNet adds `lpips`.  -> dict(views, psnr, ssim[, lpips]): float64
    arrays in view order."""
    views = [int(v) for v in views]
    if not views:
        raise ValueError("no views to score")
    preds = []
    for v in views:
        fn = prediction_path(rendering_dir, v, result_from)
        p = read_rgb8(fn)
        _check_size(p, img_res, fn)
        preds.append(p)
    gt, m = load_gt(data_dir_root, dataset, scan, views, img_res=img_res, mask=mask, scene=scene)
    preds = np.stack(preds)
    psnr, ssim = score_views(preds, gt, m)
    res = dict(views=np.asarray(views), psnr=psnr, ssim=ssim)
    if lpips is not None:
        res["lpips"] = lpips.score_views(preds, gt, m)
    return res


def scan_lines(scan, psnr, ssim, lpips=None):
    """The reference's per-scan block (eval_vsdf.py:273-277); its LPIPS line only when `lpips` is given."""
    psnr, ssim = np.asarray(psnr, np.float64), np.asarray(ssim, np.float64)
    lines = [f"SCAN {scan}:",
             "    psnr mean = {0}, std {1}".format("%.4f" % psnr.mean(), "%.4f" % psnr.std()),
             "    ssim mean = {0}, std {1}".format("%.4f" % ssim.mean(), "%.4f" % ssim.std())]
    if lpips is not None:
        lpips = np.asarray(lpips, np.float64)
        lines.append("    lpips mean = {0}, std {1}".format("%.4f" % lpips.mean(), "%.4f" % lpips.std()))
    return lines


def add_lpips_arguments(p, required=False):
    p.add_argument("--lpips-vgg", required=required, help="VGG-16 state dict (.pth or .npz: torchvision's vgg16, or one "
                                                         "file with the lin layers too): adds the LPIPS line")
    p.add_argument("--lpips-lin", help="the lin layers (.pth or .npz: the lpips package's vgg.pth)")


def lpips_from_arguments(a):
    """-> a svs_hip.lpips.LpipsNet, or None without --lpips-vgg"""
    if a.lpips_vgg is None:
        if a.lpips_lin is not None:
            raise SystemExit("--lpips-lin needs --lpips-vgg")
        return None
    from . import lpips as _lpips
    return _lpips.LpipsNet(_lpips.load_weights(a.lpips_vgg, a.lpips_lin))


def main(argv=None, require_lpips=False):
    p = argparse.ArgumentParser(description="GPU novel-view scores (the reference's eval_vsdf.py --result_from): masked "
                                            "PSNR and SSIM of the rendered evaluation views of one scan.")
    p.add_argument("--data-dir-root", required=True, help="holds {DTU|BlendedMVS}/scanN/image and .../eval_mask")
    p.add_argument("--dataset", required=True, choices=DATASETS)
    p.add_argument("--scan", type=int, required=True)
    p.add_argument("--rendering-dir", required=True, help="holds eval_blend_{:03d}.png / eval_{:03d}.png")
    p.add_argument("--views", type=int, nargs="+", required=True, help="evaluation view ids (training views excluded)")
    p.add_argument("--result-from", default="blend", choices=("blend", "default"))
    p.add_argument("--img-res", type=int, nargs=2, default=IMG_RES, metavar=("H", "W"))
    p.add_argument("--mask", choices=("auto", "on", "off"), default="auto",
                   help="auto: the reference's rule (DTU scans 1, 4, 11, 13, 48 unmasked)")
    p.add_argument("--json", help="write the per-view values here")
    add_lpips_arguments(p, required=require_lpips)
    a = p.parse_args(argv)
    mask = {"auto": None, "on": True, "off": False}[a.mask]
    r = score_scan(a.rendering_dir, a.data_dir_root, a.dataset, a.scan, a.views, result_from=a.result_from,
                   img_res=tuple(a.img_res), mask=mask, lpips=lpips_from_arguments(a))
    for line in scan_lines(a.scan, r["psnr"], r["ssim"], r.get("lpips")):
        print(line)
    if a.json:
        rec = dict(scan=a.scan, dataset=a.dataset, result_from=a.result_from, views=r["views"].tolist(),
                   psnr=[float(x) for x in r["psnr"]], ssim=[float(x) for x in r["ssim"]])
        if "lpips" in r:
            rec["lpips"] = [float(x) for x in r["lpips"]]
        with open(a.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
