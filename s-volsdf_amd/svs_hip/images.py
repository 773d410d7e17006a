"""What the evaluation-side modules (fusion, ibr, nvs, scene, evalviews, mvsout) share: the GPU and the upload of an
array to it, PNG decoding with the reference's mask rules, the dataset's constants and file layout, and the per-axis
tables of the resize kernels.  Host code only; nothing here launches a kernel.
"""
import glob
import os

import numpy as np
import torch

from . import lib as _lib

# ---- dataset facts ---------------------------------------------------------------------------------------------------
IMG_RES = (576, 768)                                   # dataset.img_res of config/confs/dtu.conf and bmvs.conf
DATASETS = ("DTU", "BlendedMVS")
DTU_UNMASKED_SCANS = (1, 4, 11, 13, 48)                # scene_dataset.py:172: scored without eval masks
BMVS_ALPHA_DIVISOR = 255.0                             # a BlendedMVS mask is the alpha channel / 255


def glob_images(image_dir):
    """sorted(glob_imgs(image_dir)) (volsdf/utils/general.py:18-22)"""
    paths = []
    for ext in ("*.png", "*.jpg", "*.JPEG", "*.JPG"):
        paths.extend(glob.glob(os.path.join(image_dir, ext)))
    return sorted(paths)


# Two rules name a view's evaluation-mask file, and they differ for a DTU scan that holds both layouts in part.
def scan_mask_files(data_dir_root, dataset, scan):
    """The dataset's rule (scene_dataset.py:130-138,178,190-191), decided ONCE PER SCAN: DTU reads
    eval_mask/scan{S}/mask/{v:03d}.png when mask/000.png exists and eval_mask/scan{S}/{v:03d}.png otherwise; BlendedMVS
    reads eval_mask/scan{S}/mask/{v:08d}.png.  -> the function view -> file"""
    mask_dir = os.path.join(data_dir_root, dataset, "eval_mask", f"scan{scan}")
    if dataset == "DTU":
        sub = "mask" if os.path.exists(os.path.join(mask_dir, "mask", "000.png")) else ""
        return lambda v: os.path.join(mask_dir, sub, f"{v:03d}.png")
    return lambda v: os.path.join(mask_dir, "mask", f"{v:08d}.png")


def view_mask_file(data_dir_root, dataset, scan_name, view):
    """The runner's rule (runner.py:351-360), decided PER FILE: BlendedMVS eval_mask/<scan>/mask/{view:08}.png; DTU
    eval_mask/<scan>/mask/{view:03}.png, else eval_mask/<scan>/{view:03}.png.  -> the file, which exists"""
    mask_dir = os.path.join(data_dir_root, dataset, "eval_mask", scan_name)
    if dataset == "BlendedMVS":
        path = os.path.join(mask_dir, "mask", "{:0>8}.png".format(view))
    elif dataset == "DTU":
        path = os.path.join(mask_dir, "mask", "{:0>3}.png".format(view))
        if not os.path.exists(path):
            path = os.path.join(mask_dir, "{:0>3}.png".format(view))
    else:
        raise NotImplementedError(f"dataset {dataset!r}: only DTU and BlendedMVS have evaluation masks")
    if not os.path.exists(path):
        raise FileNotFoundError(f"evaluation mask of view {view} not found: {path}")
    return path


# ---- the GPU ---------------------------------------------------------------------------------------------------------
def device(module):
    """The current GPU, or SvsError in the name of svs_hip.<module>."""
    if not torch.cuda.is_available():
        raise _lib.SvsError(f"svs_hip.{module} needs the GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def to_device(a, dtype, module, what="array", ndim=None, expect=None, cast=True, non_blocking=False):
    """a: array or tensor, host or device.  -> contiguous tensor of `dtype` on the current GPU.  ndim: the numbers of
    dimensions that are taken (ValueError otherwise; `expect` words it).  cast=False: another dtype is a TypeError
    instead of being converted."""
    name = str(dtype).replace("torch.", "")
    if not torch.is_tensor(a):
        a = np.asarray(a)
    if not cast and str(a.dtype).replace("torch.", "") != name:
        raise TypeError(f"{what} must be {name}, got {a.dtype}")
    if ndim is not None and a.ndim not in ndim:
        raise ValueError(f"{what}: expected {expect or ' or '.join(map(str, ndim)) + ' dimensions'}, got {tuple(a.shape)}")
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=name))
    return a.detach().to(device=device(module), dtype=dtype, non_blocking=non_blocking).contiguous()


# ---- PNG files -------------------------------------------------------------------------------------------------------
def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def read_rgb8(path):
    """-> (H,W,3) uint8, or ValueError"""
    a = read_png(path)
    if a.dtype != np.uint8:
        raise ValueError(f"{path}: {a.dtype} image; only 8-bit images are supported")
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{path}: expected an RGB image, got shape {a.shape}")
    return a


def read_dtu_mask(path):
    """-> (H,W,3) bool: inside where a channel's code is 255 ((png / 255.) == 1, scene_dataset.py:181-182)"""
    m = read_png(path)
    if m.ndim != 3 or m.shape[2] < 3 or m.dtype != np.uint8:
        raise ValueError(f"{path}: expected an 8-bit RGB(A) mask, got {m.dtype} {m.shape}")
    return m[:, :, :3] == 255


def read_bmvs_alpha(path):
    """-> (H,W) uint8: the alpha codes of an RGBA mask (scene_dataset.py:195-197); see alpha_inside"""
    m = read_png(path)
    if m.ndim != 3 or m.shape[2] != 4 or m.dtype != np.uint8:
        raise AssertionError(f"{path}: expected an 8-bit RGBA mask, got {m.dtype} {m.shape}")
    return np.ascontiguousarray(m[:, :, 3])


def alpha_inside(alpha):
    """alpha * 1. / 255. > 0.5 (scene_dataset.py:197) of unresized alpha codes -> bool"""
    return alpha.astype(np.float32) / np.float32(BMVS_ALPHA_DIVISOR) > 0.5


# ---- the per-axis tables of the resize kernels -------------------------------------------------------------------------
def source_coords(dst, src):
    """OpenCV's split of the source coordinate: fx = (float)((d + 0.5) * scale - 0.5) with scale = 1 / (dst / src) in
    double, s = floor(fx), t = fx - s (exact in float32).  -> s int32 (dst,), t float32 (dst,)"""
    scale = 1.0 / (float(dst) / float(src))
    fx = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(fx)
    return s.astype(np.int32), (fx - s).astype(np.float32)


def cubic_table(dst, src):
    """-> first tap index (s - 1; taps are clamped by the kernel) int32 (dst,), Keys' cubic weights for A = -0.75 at t,
    float32 (dst,4): evaluated in float64 from the float32 t and rounded once (OpenCV evaluates the same polynomials in
    float32: up to ~1e-7 apart)."""
    s, t = source_coords(dst, src)
    t = t.astype(np.float64)
    A = -0.75

    def near(x):                                        # |x| <= 1
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

    def far(x):                                         # 1 < |x| < 2
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    coef = np.stack([far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t)], -1)
    return (s - 1).astype(np.int32), coef.astype(np.float32)


def linear_table(dst, src):
    """-> first tap index s int32 (dst,), weights (1 - t, t) float32 (dst,2)"""
    s, t = source_coords(dst, src)
    return s, np.stack([np.float32(1.0) - t, t], -1).astype(np.float32)


def tables_device(builder, H, W, Hs, Ws, dev):
    """-> [x index, x weights, y index, y weights] of an (Hs,Ws) -> (H,W) resize as device tensors, in the order the
    entry points take them"""
    xo, xc = builder(W, Ws)
    yo, yc = builder(H, Hs)
    return [torch.from_numpy(t).to(dev) for t in (xo, xc, yo, yc)]
