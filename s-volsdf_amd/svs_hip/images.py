"""What the evaluation-side modules (fusion, ibr, nvs, scene, mvsdata, evalviews, mvsout) share: the GPU and the upload
of an array to it, the phase clock of a loader, PNG decoding with the reference's mask rules, and the per-axis tables of
the resize kernels.  Host code only; nothing here launches a kernel.  (What is known about a scan -- constants, file
layout, view ids -- is svs_hip/scans.py.)
"""
import time
from collections import OrderedDict

import numpy as np
import torch

from . import lib as _lib
from .scans import BMVS_ALPHA_DIVISOR

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


class Phases:
    """seconds per named phase (default: a loader's four); with sync=True the device is drained at every boundary so that
    they add up"""

    def __init__(self, names=("decode", "upload", "kernels", "download"), sync=False):
        self.sync, self.s = sync, OrderedDict((k, 0.0) for k in names)
        self.bytes_up = self.bytes_down = 0

    def add(self, name, t0):
        if self.sync and torch.cuda.is_available():
            torch.cuda.synchronize()
        self.s[name] += time.perf_counter() - t0
        return time.perf_counter()

    def summary(self, total):
        return seconds_line(self.s) + f", total {total:.3f}; {self.bytes_up / 1e6:.1f} MB up, {self.bytes_down / 1e6:.1f} MB down"


def seconds_line(timers):
    return "seconds: " + ", ".join(f"{k} {v:.3f}" for k, v in timers.items())


def tick(timers, name, t0):
    """adds the seconds since t0 to timers[name] after a device synchronise -> the new t0; without timers nothing waits"""
    if timers is None:
        return t0
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    timers[name] = timers.get(name, 0.0) + (t1 - t0)
    return t1


def upload_codes(stack, phases):
    """a stack of uint8 codes from the host -> the current GPU (the host tensor itself without one), counted in `phases`"""
    t = torch.from_numpy(stack)
    phases.bytes_up += t.numel()
    return t.to("cuda", non_blocking=True) if torch.cuda.is_available() else t


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
