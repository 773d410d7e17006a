"""numpy / scipy restatements of what the reference's runner does between the MVS network and the point cloud
(runner.py:267-271 and :350-368) -- what csrc/svs_mvsout.hip and svs_hip/mvsout.py are tested against.

    disk(r)                 skimage.morphology.disk: x^2 + y^2 <= r^2 on the (2r+1)x(2r+1) integer grid
    dilate(mask, r)         skimage.morphology.binary_dilation(mask, disk(r)) = scipy.ndimage.binary_dilation of mask != 0
                            with that structure, border value 0
    dilate_brute / dilate_spans     second opinions: "some set pixel within the footprint", and the OR of the footprint's
                            2r+1 horizontal spans
    resize_any(mask, H, W)  cv2.resize(mask * 1., (W,H)) > 0. as a boolean rule on the taps of svs_hip.images.linear_table
    resize_any_float64      the same through the interpolated float64 values (tests/scene_oracle.py::resize_linear)
    final_confidence        cv2.resize(c1) * cv2.resize(c2) * cv2.resize(c3) in float32, every product and sum rounded on
                            its own (numpy never contracts); final_confidence64: the same taps and weights, float64 arithmetic
    filter_depth            oracle/fusion_oracle.py::fuse_view(extra_mask=...) per (ref, sources) pair

scikit-image and OpenCV are not installed where this project is built: the three statements are restated, and the float32
resize is UNPINNED against OpenCV (INTEGRATION.md lists the one-line calls to check it with).
"""
import math

import numpy as np
from scipy import ndimage

import scene_oracle as so

F32 = np.float32
CONF_BOUND = 14 * 2.0 ** -24            # |float32 final confidence - float64 one|: derived in tests/test_gpu_mvsout.py


def disk(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return x * x + y * y <= r * r


def half_widths(r):
    """half-width of the footprint's row |dy| = 0..r: isqrt(r^2 - dy^2)"""
    return [math.isqrt(r * r - dy * dy) for dy in range(r + 1)]


def dilate(mask, r):
    """mask (..., Hs, Ws), set where non-zero -> uint8 0/1 of the same shape"""
    m = np.asarray(mask) != 0
    if m.ndim == 2:
        return ndimage.binary_dilation(m, structure=disk(r)).astype(np.uint8)
    return np.stack([dilate(s, r) for s in m])


def dilate_brute(mask, r):
    m = np.asarray(mask) != 0
    H, W = m.shape
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            hit = False
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    if dx * dx + dy * dy <= r * r and 0 <= y + dy < H and 0 <= x + dx < W and m[y + dy, x + dx]:
                        hit = True
            out[y, x] = hit
    return out


def dilate_spans(mask, r):
    """OR over dy of (row y + dy dilated horizontally by its half-width): the horizontal dilation through a prefix sum"""
    m = np.asarray(mask) != 0
    H, W = m.shape
    out = np.zeros((H, W), bool)
    pre = np.concatenate([np.zeros((H, 1), np.int64), np.cumsum(m, 1)], 1)           # pre[:, x] = set pixels left of x
    x = np.arange(W)
    for dy, w in enumerate(half_widths(r)):
        wide = (pre[:, np.minimum(x + w + 1, W)] - pre[:, np.maximum(x - w, 0)]) > 0
        for s in ({dy, -dy}):
            lo, hi = max(0, -s), min(H, H - s)                                        # out[y] |= wide[y + s]
            if lo < hi:
                out[lo:hi] |= wide[lo + s:hi + s]
    return out.astype(np.uint8)


def linear_table(dst, src):
    from svs_hip.images import linear_table as table
    return table(dst, src)


def resize_any(mask, H, W):
    """mask (..., Hs, Ws) 0/1 -> uint8 0/1 (..., H, W): set iff one of the 2x2 taps is set and both of that tap's
    weights are non-zero; equal sizes: mask != 0"""
    m = np.asarray(mask) != 0
    Hs, Ws = m.shape[-2:]
    if (Hs, Ws) == (H, W):
        return m.astype(np.uint8)
    xo, xc = linear_table(W, Ws)
    yo, yc = linear_table(H, Hs)
    out = np.zeros(m.shape[:-2] + (H, W), bool)
    for i in range(2):
        rows = np.take(m, np.clip(yo + i, 0, Hs - 1), axis=-2) & (yc[:, i] != 0)[:, None]
        for j in range(2):
            out |= np.take(rows, np.clip(xo + j, 0, Ws - 1), axis=-1) & (xc[:, j] != 0)[None, :]
    return out.astype(np.uint8)


def resize_any_float64(mask, H, W):
    """bilinear_float64(mask) > 0 from the coordinate formula (float32 source coordinate, float64 weights and sums)"""
    m = (np.asarray(mask) != 0).astype(np.float64)
    if m.shape == (H, W):
        return (m > 0).astype(np.uint8)
    return (so.resize_linear(m, (H, W)) > 0.0).astype(np.uint8)


def eval_mask(image, H, W, r=12):
    a = np.asarray(image)
    if a.ndim == 3:
        a = a[:, :, -1]
    return resize_any(dilate(a, r), H, W)


def _resize_f(c, H, W, dtype):
    c = np.asarray(c, F32)
    if c.shape == (H, W):
        return c.astype(dtype)
    xo, xc = linear_table(W, c.shape[1])
    yo, yc = linear_table(H, c.shape[0])
    c, xc, yc = c.astype(dtype), xc.astype(dtype), yc.astype(dtype)
    x0, x1 = np.clip(xo, 0, c.shape[1] - 1), np.clip(xo + 1, 0, c.shape[1] - 1)
    y0, y1 = np.clip(yo, 0, c.shape[0] - 1), np.clip(yo + 1, 0, c.shape[0] - 1)
    rows = c[:, x0] * xc[None, :, 0] + c[:, x1] * xc[None, :, 1]                     # horizontal pass, every source row
    out = rows[y0] * yc[:, 0, None] + rows[y1] * yc[:, 1, None]
    assert out.dtype == dtype
    return out


def final_confidence(c1, c2, c3, H, W):
    """float32, every operation rounded on its own -> float32 (H,W)"""
    r = [_resize_f(c, H, W, F32) for c in (c1, c2, c3)]
    out = (r[0] * r[1]) * r[2]
    assert out.dtype == F32
    return out


def final_confidence64(c1, c2, c3, H, W):
    r = [_resize_f(c, H, W, np.float64) for c in (c1, c2, c3)]
    return (r[0] * r[1]) * r[2]


def filter_depth(views, pairs, eval_masks=None, **kw):
    """-> list of fusion_oracle.fuse_view results, one per pair, the final masks cut by eval_masks[ref]"""
    import fusion_oracle as forc
    return [forc.fuse_view(views[v], [views[s] for s in src], extra_mask=None if eval_masks is None else eval_masks[v], **kw)
            for v, src in pairs]


def blobs(rng, hw, density):
    """a random mask with codes 0 / 1..255: seeds at `density`, every second one grown into a 3x2 blob"""
    seeds = rng.random(hw) < density
    grown = seeds & (rng.random(hw) < 0.5)
    m = seeds.copy()
    for dy, dx in ((0, 1), (1, 0), (1, 1), (2, 0), (2, 1)):
        m[dy:, dx:] |= grown[:hw[0] - dy, :hw[1] - dx]
    return (m * rng.integers(1, 256, hw)).astype(np.uint8)
