"""TEST INFRASTRUCTURE ONLY -- CPU restatement (numpy + scipy.ndimage) of the reference's novel-view scores,
eval_vsdf.py:186-212 (`--result_from blend|default`), in float64 on the reference's float32 values.

Pinning status:
  * Ground-truth and mask loading (SceneDataset, volsdf/datasets/scene_dataset.py:113-206: file order, the DTU mask
    layouts and `== 1` rule, the BlendedMVS alpha `> 0.5` rule), the prediction file names, the view exclusion, the
    white compositing and the float32 PSNR: PINNED by tests/golden/nvs_scores.npz -- the reference's own SceneDataset and
    the scoring branch of evaluate(), taken from eval_vsdf.py with `ast` and executed unmodified on a synthetic
    data_s_volsdf tree (tests/golden/make_nvs_fixture.py).
  * The two scikit-image pieces (scikit-image is not installed, so they cannot be compared against the library):
    RESTATED, NOT PINNED -- the fixture's SSIM values are this module's `structural_similarity`, called by the reference's
    statements on the arrays they build:
      - img_as_float32 of an 8-bit image: code / 255 in float32.  scikit-image 0.17.2 may form code * (1 / 255) in
        float32 instead; the two differ by at most one float32 ulp.  The division is what the prediction path
        (np.array(png, float32) / 255.) computes, so equal codes give equal values and a perfect match gives +inf.
      - structural_similarity(im1, im2, multichannel=True) of 0.17.2: each channel scored alone (converted to float64)
        and the results averaged; uniform_filter(size=7) of x, y, x^2, y^2, xy; cov_norm = 49/48; C1 = (0.01 R)^2,
        C2 = (0.03 R)^2; S averaged over the map with 3 pixels cropped from every side.  data_range is not passed, so
        for float32 input R = dtype_range[float32] = (-1, 1) -> R = 2, not the 1 most reimplementations use.  The
        crop keeps only windows wholly inside the image, so the filter's border mode never reaches the result.
Only tests/ and tools/bench_nvs.py may import this module.
"""
import numpy as np
from scipy.ndimage import uniform_filter

F32 = np.float32
WIN = 7
K1, K2 = 0.01, 0.03
DATA_RANGE_F32 = 2.0          # dtype_range[np.float32] = (-1, 1) in scikit-image 0.17.2


def img_as_float32(img):
    """skimage.img_as_float32 of an 8-bit image (restated, see the module docstring)."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise ValueError(f"only 8-bit images are restated, got {a.dtype}")
    return a.astype(F32) / F32(255.0)


def _ssim_channel(x, y, data_range):
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    n = WIN ** x.ndim
    cov_norm = n / (n - 1)
    ux = uniform_filter(x, size=WIN)
    uy = uniform_filter(y, size=WIN)
    uxx = uniform_filter(x * x, size=WIN)
    uyy = uniform_filter(y * y, size=WIN)
    uxy = uniform_filter(x * y, size=WIN)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    c1 = (K1 * data_range) ** 2
    c2 = (K2 * data_range) ** 2
    a1, a2, b1, b2 = 2 * ux * uy + c1, 2 * vxy + c2, ux ** 2 + uy ** 2 + c1, vx + vy + c2
    s = (a1 * a2) / (b1 * b2)
    pad = (WIN - 1) // 2
    return s[pad:-pad, pad:-pad].mean()


def structural_similarity(im1, im2, multichannel=False):
    """skimage.metrics.structural_similarity(im1, im2, multichannel=...) of scikit-image 0.17.2 with every other
    argument at its default, for float32 / float64 images (restated, see the module docstring)."""
    im1, im2 = np.asarray(im1), np.asarray(im2)
    if im1.shape != im2.shape:
        raise ValueError("Input images must have the same dimensions.")
    if im1.dtype not in (np.float32, np.float64):
        raise ValueError(f"only float images are restated, got {im1.dtype}")
    if multichannel:
        mssim = np.empty(im1.shape[-1])
        for ch in range(im1.shape[-1]):
            mssim[ch] = structural_similarity(im1[..., ch], im2[..., ch])
        return mssim.mean()
    if np.any(np.asarray(im1.shape) - WIN < 0):
        raise ValueError("win_size exceeds image extent.")
    return _ssim_channel(im1, im2, DATA_RANGE_F32)


def composite(x, mask):
    """x * mask + (1 - mask) in float32, as eval_vsdf.py:200-201 forms rgb_fg / rgb_hat_fg."""
    x, mask = np.asarray(x, F32), np.asarray(mask, F32)
    return x * mask + (F32(1.0) - mask)


def psnr_masked(rgb_pred, gt, mask):
    """-10 log10(mean((pred - gt)[mask == 1] ** 2)) in float64 on the float32 values (eval_vsdf.py:204-205):
    +inf for a perfect match, NaN for an empty mask."""
    d = np.asarray(rgb_pred, F32).astype(np.float64) - np.asarray(gt, F32).astype(np.float64)
    sel = np.asarray(mask) == 1
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = (d[sel] ** 2).sum() / sel.sum()
        return float(-10.0 * np.log10(mse))


def score_view(pred_codes, gt, mask):
    """One view of the scoring branch: pred_codes (H,W,3) uint8 PNG codes, gt (H,W,3) float32 as load_rgb returns it
    (or uint8 codes), mask (H,W,3) 0/1.  -> (psnr, ssim) float64."""
    pred = np.asarray(pred_codes).astype(F32) / F32(255.0)
    g = np.asarray(gt)
    g = img_as_float32(g) if g.dtype == np.uint8 else g.astype(F32)
    m = np.asarray(mask).astype(F32)
    return psnr_masked(pred, g, m), float(structural_similarity(composite(pred, m), composite(g, m), multichannel=True))


def score_views(pred, gt, mask):
    """score_view over (V,H,W,3) stacks.  -> psnr[V], ssim[V] float64."""
    res = [score_view(p, g, m) for p, g, m in zip(pred, gt, mask)]
    return np.array([r[0] for r in res]), np.array([r[1] for r in res])


def fixture_tree(golden, root):
    """Writes the input files of tests/golden/nvs_scores.npz under root.  -> {case: dict(data_dir_root, rendering_dir,
    dataset, scan, img_res, views)}."""
    import os
    for k in golden:
        if k.startswith("file/"):
            fn = os.path.join(str(root), k[len("file/"):])
            os.makedirs(os.path.dirname(fn), exist_ok=True)
            with open(fn, "wb") as f:
                f.write(np.asarray(golden[k]).tobytes())
    out = {}
    for case in golden["cases"]:
        case = str(case)
        out[case] = dict(data_dir_root=os.path.join(str(root), "data"),
                         rendering_dir=os.path.join(str(root), str(golden[f"{case}/rendering_dir"])),
                         dataset=str(golden[f"{case}/dataset"]), scan=int(golden[f"{case}/scan"]),
                         img_res=tuple(int(x) for x in golden[f"{case}/img_res"]),
                         views=[int(v) for v in golden[f"{case}/views"]])
    return out


def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)
