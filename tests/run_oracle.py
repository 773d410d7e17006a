"""Numpy restatements for svs_hip.run's save tail (csrc/svs_preview.hip, svs_hip/mvsout.py): what the GPU tests compare
against, themselves checked on the CPU against the reference's own function (tests/golden/depth_preview.npz) and against
numpy (tests/test_run_cpu.py)."""
import numpy as np


def visualize_depth(depth, lo=None, hi=None, direct=False, table=None):
    """helpers/utils.py:197-224 without the in-place clamp of the caller's array; lo / hi None: the 5th / 95th percentile
    of the valid pixels.  table (256,3) uint8: what cv2.applyColorMap looks up.  hi <= lo: zeros (the reference's result is
    platform-defined there)."""
    depth = np.array(depth, dtype=np.float32)
    invalid = np.logical_or(np.isnan(depth), np.logical_not(np.isfinite(depth)))
    if lo is None:
        lo = np.percentile(depth[~invalid], 5)
    if hi is None:
        hi = np.percentile(depth[~invalid], 95)
    lo, hi = np.float32(lo), np.float32(hi)
    if not hi > lo:
        return np.zeros(depth.shape + (() if direct else (3,)), np.uint8)
    with np.errstate(invalid="ignore"):
        depth[depth < lo] = lo
        depth[depth > hi] = hi
    depth[invalid] = hi
    codes = np.uint8((depth - lo) / (hi - lo) * 255)
    if direct:
        codes[invalid] = 0
        return codes
    color = np.asarray(table, np.uint8)[255 - codes]
    color[invalid, :] = 0
    return color


def sort_select(values, ranks):
    """the stand-in for svs_hip.mvsout.select_sorted_pairs on the host: np.sort"""
    a = np.asarray(values.cpu() if hasattr(values, "cpu") else values, dtype=np.float32).reshape(-1)
    s = np.sort(a)
    n = s.size
    pairs = np.array([[s[k], s[min(k + 1, n - 1)]] for k in ranks], np.float32).reshape(len(ranks), 2)
    return pairs, dict(nan=int(np.isnan(a).sum()), posinf=int(np.isposinf(a).sum()), neginf=int(np.isneginf(a).sum()))


def key_order(values):
    """the kernel's total order: -inf < negatives < -0.0 < +0.0 < positives < +inf < NaN -> the sorted array"""
    a = np.asarray(values, np.float32).reshape(-1)
    u = a.view(np.uint32)
    key = np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000))
    key = np.where(np.isnan(a), np.uint32(0xffffffff), key)
    return a[np.argsort(key, kind="stable")]


def same_bits(got, want):
    """bit for bit, NaN matching NaN, and a zero matching a zero of either sign (np.sort and np.quantile leave the sign of a
    zero among -0.0 and +0.0 to their algorithm)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    zero = (got == 0) & (want == 0)
    nan = np.isnan(got) & np.isnan(want)
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | zero | nan))
