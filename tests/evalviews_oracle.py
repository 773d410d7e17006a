"""numpy restatement of the per-view finish of evaluation rendering (eval_vsdf.py:230-262) and of the depth colouring it
calls (volsdf/utils/plots.py:392-468: visualize_depth, visualize_cmap, weighted_percentile, matte), written from the
reference's behaviour.  Test-side only.

Two evaluations of the colour step:
  mode "f32": the number formats the reference's statements end up with -- the depth is a float32 torch tensor, so the
      curve, the normalisation and matplotlib's index are float32; the percentile's cumulative sum is float32 (acc is);
      the colour table, the checker and the matte are float64, except (1 - acc), which stays float32.  This reproduces
      tests/golden/evalviews_finish.npz code for code.
  mode "f64": every step in float64 from the float32 inputs (only (1 - acc) stays float32: it is an input-side
      rounding, not an evaluation error).  This is what the kernel is compared against.
"""
import numpy as np

F32 = np.float32
EPS = np.finfo(np.float32).eps
CHECKER = 8
DARK, LIGHT = 0.8, 1.0


def to_code(x):
    """x86 numpy's float -> uint8 cast: truncation toward zero to int32, the low 8 bits kept (-1.5 -> 255, 300.7 -> 44,
    1e6 -> 64); outside the int32 range and for NaN the conversion's result is 0x80000000: code 0."""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        ok = np.abs(x) < 2147483648.0
        t = np.trunc(np.where(ok, x, 0.0)).astype(np.int64)
    return (t & 255).astype(np.uint8)


def finish(rgb_values, normal_map, depth_values, weights, scale_factor):
    """-> rgb_codes (N,3) uint8, normal_codes (N,3) uint8, depth_est (N,) float32 -- each step the float32 operation the
    reference performs -- and acc (N,) float64: the exact row sums, with acc_bound (N,) = (S-1) 2^-24 sum|w|, the
    bound of any float32 summation order of S terms."""
    rgb = np.asarray(rgb_values, F32)
    n = np.asarray(normal_map, F32)
    w = np.asarray(weights, F32).astype(np.float64)
    return dict(rgb_codes=to_code(rgb * F32(255)),
                normal_codes=to_code(((n + F32(1)) / F32(2)) * F32(255)),
                depth_est=np.asarray(depth_values, F32).reshape(-1) * F32(scale_factor),
                acc=w.sum(1), acc_bound=(w.shape[1] - 1) * 2.0 ** -24 * np.abs(w).sum(1))


def weighted_percentile(x, w, ps, dtype=np.float64):
    """plots.py:399-407: sort by value, cumulative weights in `dtype`, linear interpolation at ps percent of the total."""
    x, w = np.asarray(x).reshape(-1), np.asarray(w).reshape(-1)
    order = np.argsort(x)
    x, w = x[order], w[order].astype(dtype)
    cw = np.cumsum(w)
    return np.interp(np.array(ps) * (cw[-1] / 100), cw, x)


def depth_bounds(depth, acc, mode="f64", percentile=99.0):
    """The two bounds visualize_cmap renders between, in depth units: the weighted percentiles 0.5 and 99.5 of the depth,
    moved outwards by float32 eps (plots.py:444-450)."""
    lo, hi = weighted_percentile(depth, acc, [50 - percentile / 2, 50 + percentile / 2],
                                 dtype=np.float32 if mode == "f32" else np.float64)
    return float(lo - EPS), float(hi + EPS)


def checker(H, W):
    """matte's background (plots.py:411-414): 8-pixel squares, 0.8 where the two parities agree, 1.0 elsewhere"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where(np.logical_xor(yy % (2 * CHECKER) // CHECKER, xx % (2 * CHECKER) // CHECKER), LIGHT, DARK)


def depth_colors(depth, acc, lo, hi, table, hw, mode="f64", return_values=False):
    """depth, acc: (H*W,) float32; lo, hi: depth_bounds; table: (L,3) float64.  -> codes (H,W,3) uint8; with
    return_values also the index value v * L and the final value * 255 (H,W,3), in the mode's arithmetic."""
    H, W = hw
    T = np.float32 if mode == "f32" else np.float64
    table = np.asarray(table, np.float64)
    L = table.shape[0]
    d = np.asarray(depth, F32).reshape(-1)
    a = np.asarray(acc, F32).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cl, ch = -np.log(np.float64(lo) + EPS), -np.log(np.float64(hi) + EPS)
        if mode == "f32":
            c = -np.log(d + EPS)                                      # float32 + float32 eps, float32 log
        else:
            c = -np.log(d.astype(np.float64) + np.float64(EPS))
        v = (c - T(np.minimum(cl, ch))) / T(np.abs(ch - cl))
        v = np.nan_to_num(np.clip(v, 0, 1)).astype(T)
    xa = v * T(L)                                                     # matplotlib: v = 1 belongs to the last entry
    xa = np.where(xa == L, T(L - 1), xa)
    idx = np.clip(xa.astype(np.int64), 0, L - 1)
    col = table[idx]                                                  # (N,3) float64
    bg = checker(H, W).reshape(-1)
    final = (col * a.astype(np.float64)[:, None] + (bg * (F32(1) - a).astype(np.float64))[:, None]) * 255.0
    codes = to_code(final).reshape(H, W, 3)
    if return_values:
        return codes, xa.astype(np.float64).reshape(H, W), final.reshape(H, W, 3)
    return codes


def near_boundary(xa, final, acc, tol=1e-5):
    """(H,W) bool: pixels whose table index value or whose final value (any channel) lies within tol of an integer.
    Narrower than that where the value is exact in any arithmetic and so no hazard: an index value clipped to 0 or to the
    last entry does not count, nor does the final value of a pixel with acc == 0 (the checker alone: 0.8 * 255, 255)."""
    def close(z):
        return np.abs(z - np.rint(z)) <= tol
    free = (xa > 0) & (xa < np.floor(xa.max()))
    return (close(xa) & free) | (close(final).any(-1) & (np.asarray(acc).reshape(xa.shape) != 0))


def turbo_table():
    """matplotlib's 256-entry turbo table, float64 (256,3); taken from matplotlib at run time, never stored"""
    import matplotlib
    return np.asarray(matplotlib.colormaps["turbo"](np.arange(256))[:, :3], np.float64)


def seeded_view(seed, hw, n_samples=98):
    """per-ray arrays of one view in merge_output's shapes (the generator's recipe, any size)"""
    from make_evalviews_fixture import make_inputs
    return make_inputs(seed=seed, hw=hw, n_samples=n_samples)
