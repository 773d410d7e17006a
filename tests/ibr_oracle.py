"""TEST INFRASTRUCTURE ONLY -- CPU restatement (numpy) of the reference's image-based rendering of evaluation views,
simple_ibr.py:116-235 (image_based_render after its file reads, get_dir_loc, Laplacian_Blending, get_lpIMG), keeping
numpy's dtypes: float32 up to the blend, float64 pyramids (`astype("float")`).

Pinning status:
  * image_based_render's per-view arithmetic, get_dir_loc / get_camera_params / lift, Laplacian_Blending, get_lpIMG and
    the PNG it writes: PINNED by tests/golden/ibr_blend.npz -- the reference's own functions, taken from simple_ibr.py with
    `ast` and executed unmodified on a synthetic scan folder (tests/golden/make_ibr_fixture.py) with real
    scipy.special.softmax and `cv2` bound to the restatements below.  tests/test_ibr_cpu.py checks that this module
    reproduces every captured array bit for bit.
  * check_geometric_consistency: fusion_oracle's, pinned by tests/golden/fusion_geo.npz.
  * The OpenCV pieces (cv2 is not installed, so they cannot be compared against the library itself): PARITY UNPINNED,
    restated from OpenCV's documented algorithms and checked on their own properties in tests/test_ibr_cpu.py:
      - remap_cubic: cv2.remap(INTER_CUBIC, BORDER_CONSTANT 0) on float32: maps rounded to 5 fractional bits
        (cvRound(x * 32), half to even), taps ix-1..ix+2, 1-D weights interpolateCubic(k / 32) with A = -0.75, 2-D weight
        wy[i] * wx[j] in float32; inside the image each row is summed left to right and the rows added, at the border the
        in-image taps are added one by one from 0; a window wholly outside gives 0.
      - erode: cv2.erode(src, ones(5,5)) with the default border: a minimum over the in-image neighbourhood.
      - pyr_down / pyr_up: cv2.pyrDown / cv2.pyrUp, 5x5 [1 4 6 4 1]^2 kernel (/256, x4 /256 for pyrUp), BORDER_REFLECT_101
        (pyrUp: on the upsampled grid), OpenCV's operation order.
      - cv2.subtract / cv2.add of float arrays: element-wise.
Only tests/ and tools/bench_ibr.py may import this module.
"""
import types

import numpy as np
import torch
import torch.nn.functional as F

import fusion_oracle as forc

F32 = np.float32
NUM_LEVELS = 4


# ---- OpenCV restatements ----------------------------------------------------------------------------------------------
def cubic_coeffs(x):
    """interpolateCubic (imgwarp.cpp) in float32: the four weights of taps -1..2 at fraction x."""
    x = np.asarray(x, F32)
    A, one = F32(-0.75), F32(1.0)
    x1 = (x + one).astype(F32)
    c0 = (((A * x1 - F32(5.0) * A) * x1 + F32(8.0) * A) * x1 - F32(4.0) * A).astype(F32)
    c1 = ((((A + F32(2.0)) * x - (A + F32(3.0))) * x) * x + one).astype(F32)
    xm = (one - x).astype(F32)
    c2 = ((((A + F32(2.0)) * xm - (A + F32(3.0))) * xm) * xm + one).astype(F32)
    c3 = (((one - c0) - c1) - c2).astype(F32)
    return np.stack([c0, c1, c2, c3], -1)


CUBIC_TAB = cubic_coeffs(np.arange(32, dtype=F32) * F32(1.0 / 32.0))       # (32, 4): OpenCV's INTER_TAB_SIZE table


def remap_cubic(img, mapx, mapy):
    """cv2.remap(img, mapx, mapy, interpolation=cv2.INTER_CUBIC): float32 image (H,W) or (H,W,C), float32 maps."""
    img = np.asarray(img, F32)
    squeeze = img.ndim == 2
    if squeeze:
        img = img[..., None]
    H, W, C = img.shape
    fx = (np.asarray(mapx, F32) * F32(32.0)).astype(F32)
    fy = (np.asarray(mapy, F32) * F32(32.0)).astype(F32)
    bad = ~((fx > -2.1e9) & (fx < 2.1e9) & (fy > -2.1e9) & (fy < 2.1e9))
    sx = np.rint(np.where(bad, 0, fx)).astype(np.int64)            # cvRound: half to even
    sy = np.rint(np.where(bad, 0, fy)).astype(np.int64)
    x0 = np.clip(sx >> 5, -32768, 32767) - 1
    y0 = np.clip(sy >> 5, -32768, 32767) - 1
    wx, wy = CUBIC_TAB[sx & 31], CUBIC_TAB[sy & 31]                 # (..., 4)
    w = (wy[..., :, None] * wx[..., None, :]).astype(F32)           # (..., 4, 4): w[i, j] = wy[i] * wx[j]
    outside = bad | (x0 >= W) | (x0 + 4 <= 0) | (y0 >= H) | (y0 + 4 <= 0)
    inside = (x0 >= 0) & (x0 < max(W - 3, 0)) & (y0 >= 0) & (y0 < max(H - 3, 0))
    taps, valid = {}, {}
    for i in range(4):
        for j in range(4):
            xx, yy = x0 + j, y0 + i
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            valid[i, j] = ok
            taps[i, j] = np.where(ok[..., None], img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], F32(0.0)).astype(F32)
    prod = {k: (taps[k] * w[..., k[0], k[1]][..., None]).astype(F32) for k in taps}
    interior = None
    for i in range(4):
        row = (((prod[i, 0] + prod[i, 1]) + prod[i, 2]) + prod[i, 3]).astype(F32)
        interior = row if interior is None else (interior + row).astype(F32)
    border = np.zeros_like(interior)
    for i in range(4):
        for j in range(4):
            border = np.where(valid[i, j][..., None], (border + prod[i, j]).astype(F32), border)
    out = np.where(inside[..., None], interior, border)
    out = np.where(outside[..., None], F32(0.0), out).astype(F32)
    return out[..., 0] if squeeze else out


def erode(src, kernel):
    """cv2.erode(src, kernel) with a full rectangular kernel and the default border (outside pixels take no part)."""
    kh, kw = np.asarray(kernel).shape
    assert np.all(np.asarray(kernel) != 0), "full rectangular kernels only"
    src = np.asarray(src)
    H, W = src.shape[:2]
    ry, rx = kh // 2, kw // 2
    pad = np.full((H + 2 * ry, W + 2 * rx) + src.shape[2:], np.inf)
    pad[ry:ry + H, rx:rx + W] = src
    out = np.full(src.shape, np.inf)
    for dy in range(kh):
        for dx in range(kw):
            out = np.minimum(out, pad[dy:dy + H, dx:dx + W])
    return out.astype(src.dtype)


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101) for an integer array p."""
    p = np.array(p, np.int64, copy=True)
    if n == 1:
        return np.zeros_like(p)
    while True:
        out = (p < 0) | (p >= n)
        if not out.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def pyr_down(src):
    """cv2.pyrDown on a float64 (H,W[,C]) image: [1 4 6 4 1]^2 / 256 at the even rows and columns, BORDER_REFLECT_101."""
    src = np.asarray(src, np.float64)
    H, W = src.shape[:2]
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    cx = [reflect101(2 * np.arange(w2) - 2 + k, W) for k in range(5)]
    ry = [reflect101(2 * np.arange(h2) - 2 + k, H) for k in range(5)]
    s = [src[:, c] for c in cx]
    row = ((s[2] * 6 + (s[1] + s[3]) * 4) + s[0]) + s[4]                 # every source row, at the destination columns
    r = [row[i] for i in ry]
    return (((r[2] * 6 + (r[1] + r[3]) * 4) + r[0]) + r[4]) * (1.0 / 256)


def pyr_up(src):
    """cv2.pyrUp on a float64 (h,w[,C]) image -> (2h, 2w[,C]).  Zeros injected, 4 x the pyrDown kernel, BORDER_REFLECT_101
    on the upsampled grid: rows reflect at the top and replicate at the bottom; columns 6 c + 2 r at the left edge,
    l + 7 c and 8 c at the right edge; a single column gives 8 c for both."""
    src = np.asarray(src, np.float64)
    h, w = src.shape[:2]
    row = np.empty((h, 2 * w) + src.shape[2:])
    if w == 1:
        row[:, 0] = row[:, 1] = src[:, 0] * 8
    else:
        row[:, 0] = src[:, 0] * 6 + src[:, 1] * 2
        row[:, 1] = (src[:, 0] + src[:, 1]) * 4
        row[:, 2 * w - 2] = src[:, w - 2] + src[:, w - 1] * 7
        row[:, 2 * w - 1] = src[:, w - 1] * 8
        if w > 2:
            x = np.arange(1, w - 1)
            row[:, 2 * x] = (src[:, x - 1] + src[:, x] * 6) + src[:, x + 1]
            row[:, 2 * x + 1] = (src[:, x] + src[:, x + 1]) * 4
    y = np.arange(h)
    up, dn = reflect101(2 * (y - 1), 2 * h) // 2, reflect101(2 * (y + 1), 2 * h) // 2
    out = np.empty((2 * h, 2 * w) + src.shape[2:])
    out[0::2] = ((row[up] + row[y] * 6) + row[dn]) * (1.0 / 64)
    out[1::2] = ((row[y] + row[dn]) * 4) * (1.0 / 64)
    return out


INTER_LINEAR, INTER_CUBIC = 1, 2


def _remap(src, mapx, mapy, interpolation):
    if interpolation == INTER_LINEAR:
        return forc.remap_linear(src, mapx, mapy)
    if interpolation == INTER_CUBIC:
        return remap_cubic(src, mapx, mapy)
    raise NotImplementedError(interpolation)


# what the reference's functions see as `cv2` when the fixture is made
cv2 = types.SimpleNamespace(INTER_LINEAR=INTER_LINEAR, INTER_CUBIC=INTER_CUBIC, remap=_remap, erode=erode,
                            pyrDown=pyr_down, pyrUp=pyr_up, subtract=lambda a, b: a - b, add=lambda a, b: a + b)


# ---- simple_ibr.py ----------------------------------------------------------------------------------------------------
def get_dir_loc(K, E, hw):
    """get_dir_loc + get_camera_params + lift (simple_ibr.py:31-88) with torch on the CPU, as the reference runs them:
    pose = inv(E) in E's dtype (float32), intrinsics in a float64 4x4 then float32.  -> (h,w,3) float32, (3,) float32."""
    h, w = hw
    intr = np.eye(4)
    intr[:3, :3] = K
    pose = np.linalg.inv(E)
    uv = np.flip(np.mgrid[0:h, 0:w].astype(np.int32), axis=0).copy().reshape(2, -1).transpose(1, 0)
    uv = torch.from_numpy(uv[None]).float()
    p = torch.from_numpy(pose[None]).float()
    intr = torch.from_numpy(intr[None]).float()
    cam_loc = p[:, :3, 3]
    x, y, z = uv[:, :, 0].view(1, -1), uv[:, :, 1].view(1, -1), torch.ones((1, uv.shape[1])).view(1, -1)
    fx, fy, cx, cy, sk = intr[:, 0, 0], intr[:, 1, 1], intr[:, 0, 2], intr[:, 1, 2], intr[:, 0, 1]
    x_lift = (x - cx.unsqueeze(-1) + cy.unsqueeze(-1) * sk.unsqueeze(-1) / fy.unsqueeze(-1)
              - sk.unsqueeze(-1) * y / fy.unsqueeze(-1)) / fx.unsqueeze(-1) * z
    y_lift = (y - cy.unsqueeze(-1)) / fy.unsqueeze(-1) * z
    pts = torch.stack((x_lift, y_lift, z, torch.ones_like(z)), dim=-1).permute(0, 2, 1)
    world = (torch.bmm(p[:, :3, :3], pts[:, :3, :]) + p[:, :3, 3:]).permute(0, 2, 1)
    dirs = F.normalize(world - cam_loc[:, None, :], dim=2)
    return dirs.squeeze().reshape(h, w, 3).numpy(), cam_loc.squeeze().numpy()


def softmax0(x):
    """scipy.special.softmax(x, axis=0)."""
    x_max = np.amax(x, axis=0, keepdims=True)
    e = np.exp(x - x_max)
    return e / np.sum(e, axis=0, keepdims=True)


def get_lp_img(img, num_levels=NUM_LEVELS, is_mask=False):
    """get_lpIMG (simple_ibr.py:90-110)."""
    G = img.copy().astype("float")
    gp = [G]
    for _ in range(num_levels):
        G = pyr_down(G)
        gp.append(G)
    if is_mask:
        return [gp[num_levels - 1]] + [gp[i] for i in range(num_levels - 2, -1, -1)]
    lp = [gp[num_levels - 1]]
    for i in range(num_levels - 1, 0, -1):
        lp.append(gp[i - 1] - pyr_up(gp[i]))
    return lp


def laplacian_blending(imgs, masks, num_levels=NUM_LEVELS):
    """Laplacian_Blending (simple_ibr.py:112-136): imgs, masks (N+1,H,W,3) -> float64 (H,W,3) in [0, 1]."""
    assert imgs.shape == masks.shape
    lp_imgs = [get_lp_img(i, num_levels) for i in imgs]
    lp_masks = [get_lp_img(m, num_levels, is_mask=True) for m in masks]
    LS = []
    for i in range(num_levels):
        ls = 0
        for j in range(len(masks)):
            ls += lp_masks[j][i] * lp_imgs[j][i]
        LS.append(ls)
    out = LS[0]
    for i in range(1, num_levels):
        out = pyr_up(out) + LS[i]
    return np.clip(out, 0.0, 1.0)


def weights_stage(src_imgs, src_dirs, ref_dir, pred_img, geo, x2d, y2d):
    """simple_ibr.py:171-214 from the geometric masks and maps: -> (softmax weights (N+1,H,W) float32, fill images
    (N+1,H,W,3) float32, masks (N+1,H,W,3) float32) -- the arrays handed to Laplacian_Blending."""
    weight_masks, sampled = [], []
    for img, d, g, x, y in zip(src_imgs, src_dirs, geo, x2d, y2d):
        sampled.append(remap_cubic(img, x, y))
        sd = remap_cubic(d, x, y)
        with np.errstate(invalid="ignore", divide="ignore"):
            sd /= np.linalg.norm(sd, axis=2, keepdims=True)
        wm = np.nan_to_num((sd * ref_dir).sum(axis=2))
        wm *= np.asarray(g).astype(np.int32)
        weight_masks.append(wm)
    weight_masks.append(0.2 * np.ones_like(weight_masks[0]))
    sampled.append(pred_img)
    w = softmax0(20 * np.stack(weight_masks))
    w3 = w[..., None].repeat(3, -1)
    sampled = np.stack(sampled)
    fill = sampled * w3 + sampled[-1:] * (1 - w3)
    m = w3.copy()
    kernel = np.ones((5, 5), np.uint8)
    for i in range(m.shape[0] - 1):
        m[i] = erode((m[i] > 0.2) * 1.0, kernel) * 1.0 * m[i]
    m[-1] += 1e-2
    m /= m.sum(0, keepdims=True)
    return w, fill, m


def blend_view(ref, srcs, pred_img):
    """One reference view of image_based_render (simple_ibr.py:150-235).  ref / srcs[i]: dict(K (3,3), E (4,4), depth
    (H,W)) float32, srcs also img (H,W,3) float32; pred_img (H,W,3) float32.  -> dict(geo (N,H,W) bool, x2d, y2d
    (N,H,W) float32, weights, fill, masks (see weights_stage), blend (H,W,3) float64, png (H,W,3) uint8)."""
    H, W = ref["depth"].shape
    ref_dir, _ = get_dir_loc(ref["K"], ref["E"], (H, W))
    geo, xs, ys, dirs = [], [], [], []
    for s in srcs:
        assert s["depth"].shape == ref["depth"].shape
        g, _, x, y = forc.check_geometric_consistency(ref["depth"], ref["K"], ref["E"], s["depth"], s["K"], s["E"],
                                                      filter_dist=2)
        geo.append(g); xs.append(x); ys.append(y)
        dirs.append(get_dir_loc(s["K"], s["E"], s["depth"].shape)[0])
    w, fill, m = weights_stage([s["img"] for s in srcs], dirs, ref_dir, pred_img, geo, xs, ys)
    blend = laplacian_blending(fill, m)
    return dict(geo=np.stack(geo), x2d=np.stack(xs), y2d=np.stack(ys), ref_dir=ref_dir, src_dirs=np.stack(dirs),
                weights=w, fill=fill, masks=m, blend=blend, png=(blend * 255).astype(np.uint8))


def fixture_views(g, tmp_path):
    """Writes the fixture's input files under tmp_path and reads them the way image_based_render does:
    -> (scan_folder, out_folder, {eval id: (ref dict, [src dicts], pred_img)})."""
    from datasets.data_io import read_pfm
    from helpers.utils import read_camera_parameters, read_img
    scan, out = tmp_path / "scan24", tmp_path / "out"
    for key in g:
        if key.startswith("file/"):
            fn = (out if key[5:].startswith(("eval_", "depth_est")) else scan) / key[5:]
            fn.parent.mkdir(parents=True, exist_ok=True)
            fn.write_bytes(g[key].tobytes())

    def view(vid, with_img):
        K, E = read_camera_parameters(str(scan / "cams/{:0>8}_cam.txt".format(vid)))
        d = dict(K=K, E=E, depth=np.ascontiguousarray(read_pfm(str(out / "depth_est/{:0>8}.pfm".format(vid)))[0]))
        if with_img:
            d["img"] = read_img(str(scan / "images/{:0>8}.png".format(vid)))
        return d

    srcs = [view(v, True) for v in g["src_ids"]]
    views = {int(v): (view(v, False), srcs, read_img(str(out / "eval_{:0>3}.png".format(v)))) for v in g["eval_ids"]}
    return str(scan), str(out), views
