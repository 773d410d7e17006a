"""Float64 numpy restatements of the image and camera work of the reference's SceneDataset
(volsdf/datasets/scene_dataset.py:113-206) -- what csrc/svs_scene.hip and svs_hip/scene.py are tested against.

    resize_cubic     cv2.resize(img, (W,H), interpolation=cv2.INTER_CUBIC): separable 4 taps, Keys' cubic with A = -0.75,
                     source coordinate (d + 0.5) * scale - 0.5, taps clamped to the image one by one, no prefilter
    resize_linear    cv2.resize(img, (W,H)) (INTER_LINEAR): 2 taps, the same coordinate rule and clamping
    gaussian_smooth  cv2.GaussianBlur(img, (31,31), 90): 31 weights exp(-(i-15)^2 / (2 90^2)) normalised in float64 and
                     rounded to float32, BORDER_REFLECT_101, rows then columns
    mask_resize      the reference's cv2.resize(mask, (W,H), cv2.INTER_NEAREST) -- the third positional parameter is dst, so
                     INTER_LINEAR runs -- followed by > 0.5
    load_K_Rt_from_P cv2.decomposeProjectionMatrix: RQ with a positive diagonal, the camera centre from P's null vector

coord="f32" (the default, the parity definition) rounds the source coordinate to float32 before it is split into index
and fraction, as OpenCV does (`fx = (float)((dx+0.5)*scale_x - 0.5); sx = cvFloor(fx); fx -= sx`); coord="f64" keeps it
exact, which is what torch's float64 interpolate evaluates (tests/test_scene_cpu.py).  Everything after the split --
weights, products, sums -- is float64 here.

None of OpenCV, imageio or scikit-image is installed where this project is built, so the three cv2 statements above are
UNPINNED (INTEGRATION.md lists the one-line calls to check them with).
"""
import glob
import os

import numpy as np

A = -0.75
KSIZE, SIGMA = 31, 90.0


def split_coords(dst, src, coord="f32"):
    """-> s int64 (dst,), t float64 (dst,): floor and fraction of the source coordinate of every destination index"""
    scale = 1.0 / (float(dst) / float(src))                 # OpenCV: inv_scale = dst / src, scale = 1 / inv_scale
    fx = (np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5
    if coord == "f32":
        fx = fx.astype(np.float32).astype(np.float64)
    elif coord != "f64":
        raise ValueError(coord)
    s = np.floor(fx)
    return s.astype(np.int64), fx - s


def cubic_weights(t):
    """Keys' cubic convolution weights of the taps at s-1, s, s+1, s+2 for the fraction t (float64) -> (...,4)"""
    def w(x):
        x = np.abs(x)
        return np.where(x <= 1.0, ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0,
                        np.where(x < 2.0, ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A, 0.0))
    return np.stack([w(t + 1.0), w(t), w(1.0 - t), w(2.0 - t)], -1)


def cubic_table(dst, src, coord="f32"):
    s, t = split_coords(dst, src, coord)
    return s - 1, cubic_weights(t)


def linear_table(dst, src, coord="f32"):
    s, t = split_coords(dst, src, coord)
    return s, np.stack([1.0 - t, t], -1)


def _resample_axis(img, axis, first, coef):
    """sum_k coef[:, k] * img[clip(first + k)] along `axis`"""
    n = img.shape[axis]
    out = 0.0
    shape = [1] * img.ndim
    shape[axis] = -1
    for k in range(coef.shape[1]):
        idx = np.clip(first + k, 0, n - 1)
        out = out + np.take(img, idx, axis=axis) * coef[:, k].reshape(shape)
    return out


def _resize(img, hw, table, coord):
    img = np.asarray(img, np.float64)
    H, W = hw
    xo, xc = table(W, img.shape[1], coord)
    yo, yc = table(H, img.shape[0], coord)
    return _resample_axis(_resample_axis(img, 1, xo, xc), 0, yo, yc)


def resize_cubic(img, hw, coord="f32"):
    """img (Hs,Ws[,C]) -> (H,W[,C]) float64"""
    return _resize(img, hw, cubic_table, coord)


def resize_linear(img, hw, coord="f32"):
    return _resize(img, hw, linear_table, coord)


def gaussian_kernel():
    """cv2.getGaussianKernel(31, 90, CV_32F) -> float32 (31,)"""
    i = np.arange(KSIZE, dtype=np.float64) - (KSIZE - 1) / 2
    g = np.exp(-(i * i) / (2.0 * SIGMA * SIGMA))
    return (g * (1.0 / g.sum())).astype(np.float32)


def gaussian_smooth(img):
    """img (H,W[,C]), H and W >= 16 -> float64, the intermediate rounded to float32 as the row filter's output is"""
    img = np.asarray(img, np.float64)
    k = gaussian_kernel().astype(np.float64)
    r = KSIZE // 2

    def one_axis(a, axis):
        n = a.shape[axis]
        assert n > r
        out = 0.0
        for j in range(KSIZE):
            idx = np.arange(n) + j - r
            idx = np.where(idx < 0, -idx, np.where(idx >= n, 2 * n - 2 - idx, idx))     # BORDER_REFLECT_101
            out = out + k[j] * np.take(a, idx, axis=axis)
        return out
    rows = one_axis(img, 1).astype(np.float32).astype(np.float64)
    return one_axis(rows, 0)


def mask_resize(mask, hw, coord="f32", return_values=False):
    """mask (Hs,Ws) float values -> (H,W) 0/1 float64 (and the interpolated values before the threshold)"""
    v = resize_linear(mask, hw, coord)
    m = (v > 0.5).astype(np.float64)
    return (m, v) if return_values else m


def load_K_Rt_from_P(P):
    """rend_util.load_K_Rt_from_P(None, P) -> intrinsics (4,4) float64, pose (4,4) float32.  RQ by Gram-Schmidt on the
    rows from the last one up (independent of numpy's QR, which svs_hip/scene.py uses)."""
    P = np.asarray(P, np.float64)
    M = P[:, :3]
    r3 = M[2] / np.linalg.norm(M[2])
    k12 = M[1] @ r3
    r2 = M[1] - k12 * r3
    k11 = np.linalg.norm(r2)
    r2 = r2 / k11
    k02, k01 = M[0] @ r3, M[0] @ r2
    r1 = M[0] - k02 * r3 - k01 * r2
    k00 = np.linalg.norm(r1)
    r1 = r1 / k00
    K = np.array([[k00, k01, k02], [0.0, k11, k12], [0.0, 0.0, np.linalg.norm(M[2])]])
    R = np.stack([r1, r2, r3])
    c = -np.linalg.solve(M, P[:, 3])                        # P (c, 1) = 0
    intrinsics = np.eye(4)
    intrinsics[:3, :3] = K / K[2, 2]
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = R.T
    pose[:3, 3] = c
    return intrinsics, pose


# ---- the whole folder ------------------------------------------------------------------------------------------------
def read_image(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def load_rgb(path):
    """imageio.imread + skimage.img_as_float32 of an 8-bit image: code * (1/255) in float32"""
    return read_image(path).astype(np.float32) * np.float32(1.0 / 255.0)


def load_scene(data_dir_root, data_dir, scan_id, img_res, ids, coord="f32"):
    """scene_dataset.py:113-206 for one folder, cv2 bound to the restatements above.  `ids`: the module that provides
    get_eval_ids / get_trains_ids (the id tables are inputs here, not under test).
    -> dict(rgb, rgb_smooth, masks: lists of float64 (H*W,3); mask_values: {view: interpolated values (H*W,) or None};
            intrinsics, pose: lists of float32 (4,4); scale_factor; n_images; cam_file)"""
    H, W = img_res
    instance_dir = os.path.join(data_dir_root, data_dir, f"scan{scan_id}")
    cam_file = f"{instance_dir}/cameras.npz"
    if not os.path.exists(cam_file) and int(scan_id) < 200:
        cam_file = os.path.join(data_dir_root, data_dir, "scan114", "cameras.npz")
    paths = []
    for ext in ("*.png", "*.jpg", "*.JPEG", "*.JPG"):
        paths.extend(glob.glob(os.path.join(f"{instance_dir}/image", ext)))
    paths = sorted(paths)
    n = len(paths)
    cams = np.load(cam_file)
    scale_mats = [cams[f"scale_mat_{i}"].astype(np.float32) for i in range(n)]
    world_mats = [cams[f"world_mat_{i}"].astype(np.float32) for i in range(n)]
    first = load_rgb(paths[0])
    scale_h, scale_w = H * 1. / first.shape[0], W * 1. / first.shape[1]
    resize = scale_h != 1 or scale_w != 1

    mask_path = os.path.join(data_dir_root, data_dir, "eval_mask")
    if data_dir == "DTU":
        maskf = lambda x: os.path.join(mask_path, f"scan{scan_id}", "mask", f"{x:03d}.png")         # noqa: E731
        if not os.path.exists(maskf(0)):
            maskf = lambda x: os.path.join(mask_path, f"scan{scan_id}", f"{x:03d}.png")             # noqa: E731
    elif data_dir == "BlendedMVS":
        maskf = lambda x: os.path.join(mask_path, f"scan{scan_id}", "mask", f"{x:08d}.png")         # noqa: E731
    else:
        raise NotImplementedError

    out = dict(rgb=[], rgb_smooth=[], masks=[], mask_values={}, intrinsics=[], pose=[], n_images=n, cam_file=cam_file)
    out["scale_factor"] = scale_mats[0][0, 0]
    if int(scan_id) == 5 and data_dir == "BlendedMVS":
        out["scale_factor"] = 1.0
    for i, path in enumerate(paths):
        P = (world_mats[i] @ scale_mats[i])[:3, :4]
        K, pose = load_K_Rt_from_P(P)
        K[0, :] *= scale_w
        K[1, :] *= scale_h
        out["intrinsics"].append(K.astype(np.float32))
        out["pose"].append(pose.astype(np.float32))
        img = load_rgb(path)
        if resize:
            img = resize_cubic(img, (H, W), coord)
        out["rgb"].append(np.asarray(img, np.float64).reshape(-1, 3))
        # the smoothing reads the float32 image the resize wrote
        out["rgb_smooth"].append(gaussian_smooth(np.asarray(img, np.float32)).reshape(-1, 3))
        if data_dir == "DTU" and i in ids.get_eval_ids(data_dir=data_dir) and scan_id not in [1, 4, 11, 13, 48]:
            m = read_image(maskf(i)).astype(np.float32)[:, :, :3] / 255.
            m = (m == 1).astype(np.float32)
            vals = None
            if resize:
                chans = [mask_resize(m[..., c], (H, W), coord, return_values=True) for c in range(3)]
                m = np.stack([c[0] for c in chans], -1)
                vals = chans[0][1].reshape(-1)
            out["masks"].append(np.asarray(m, np.float64).reshape(-1, 3))
            out["mask_values"][i] = vals
        elif data_dir == "BlendedMVS" and i in (ids.get_eval_ids(data_dir=data_dir, scan_id=scan_id)
                                                + ids.get_trains_ids(data_dir=data_dir, scan=f"scan{scan_id}", num_views=3)):
            m = read_image(maskf(i)).astype(np.float32)
            assert m.ndim == 3 and m.shape[2] == 4
            alpha = m[:, :, -1] * np.float32(1.) / np.float32(255.)
            m, vals = mask_resize(alpha, (H, W), coord, return_values=True)
            out["masks"].append(np.repeat(m.reshape(-1, 1), 3, 1))
            out["mask_values"][i] = vals.reshape(-1)
        else:
            out["masks"].append(np.ones((H * W, 3)))
    return out


# ---- synthetic inputs for the tests ----------------------------------------------------------------------------------
def synthetic_image(H, W, seed):
    """uint8 (H,W,3): a gradient, hard-edged blocks and stripes, and noise -- a wrong tap or border rule shows"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = (60 + 120.0 * yy / H + 40 * np.sin(xx / 7.0))[..., None] + rng.normal(0, 12, (H, W, 3))
    img[H // 5:H // 2, W // 6:W // 3] = (250, 10, 128)
    img[(xx // 3) % 2 == 0, 1] += 60                        # 3-pixel stripes in one channel
    img[:2], img[-2:], img[:, :2], img[:, -2:] = 255, 0, 0, 255          # distinct borders
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def synthetic_mask(H, W):
    """uint8 (H,W) 0/1: an ellipse plus a block in the corner (so the border clamp matters)"""
    yy, xx = np.mgrid[0:H, 0:W]
    inside = ((yy - 0.5 * H) / (0.36 * H)) ** 2 + ((xx - 0.45 * W) / (0.4 * W)) ** 2 <= 1.0
    inside[:H // 6, :W // 5] = True
    return inside.astype(np.uint8)


def random_camera(rng, size):
    """a proper camera with skew: K (K[2,2] = 1), R (det +1), centre c"""
    H, W = size
    K = np.array([[W * rng.uniform(1.0, 2.0), rng.uniform(-2.0, 2.0), W * rng.uniform(0.4, 0.6)],
                  [0.0, W * rng.uniform(1.0, 2.0), H * rng.uniform(0.4, 0.6)], [0.0, 0.0, 1.0]])
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(Q) < 0:
        Q[0] = -Q[0]
    return K, Q, rng.uniform(-2.0, 2.0, 3)


def write_scan(root, dataset, scan, n_images, size, mask_views=(), mask_layout="mask", mask_size=None, seed=0,
               own_cameras=True):
    """Writes {root}/{dataset}/scan{scan}/image/*.png, cameras.npz (under scan114 when own_cameras is False) and the
    masks of `mask_views`: DTU 'mask' (eval_mask/scanS/mask/NNN.png) or 'flat' (eval_mask/scanS/NNN.png) RGB 0/255,
    BlendedMVS RGBA with a soft-edged alpha."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    inst = os.path.join(root, dataset, f"scan{scan}")
    os.makedirs(os.path.join(inst, "image"), exist_ok=True)
    cams = {}
    for i in range(n_images):
        name = f"{i:06d}.png" if dataset == "DTU" else f"{i:08d}.png"
        Image.fromarray(synthetic_image(size[0], size[1], seed * 1000 + i)).save(os.path.join(inst, "image", name))
        K, R, c = random_camera(rng, size)
        world = np.eye(4)
        world[:3, :4] = K @ np.concatenate([R, -(R @ c)[:, None]], 1) * rng.uniform(0.5, 2.0)
        scale = np.diag([1.7 + scan, 1.7 + scan, 1.7 + scan, 1.0])
        scale[:3, 3] = rng.uniform(-0.3, 0.3, 3)
        cams[f"world_mat_{i}"], cams[f"scale_mat_{i}"] = world, scale
    cam_dir = inst if own_cameras else os.path.join(root, dataset, "scan114")
    os.makedirs(cam_dir, exist_ok=True)
    np.savez(os.path.join(cam_dir, "cameras.npz"), **cams)
    mh, mw = mask_size or size
    mdir = os.path.join(root, dataset, "eval_mask", f"scan{scan}")
    if dataset == "BlendedMVS" or mask_layout == "mask":
        mdir = os.path.join(mdir, "mask")
    os.makedirs(mdir, exist_ok=True)
    for v in mask_views:
        m = np.roll(synthetic_mask(mh, mw), 2 * v, axis=1)
        if dataset == "DTU":
            Image.fromarray(np.repeat((m * 255)[..., None], 3, 2).astype(np.uint8)).save(os.path.join(mdir, f"{v:03d}.png"))
        else:
            alpha = m.astype(np.float64) * 255
            alpha[1:-1, 1:-1] = (alpha[1:-1, 1:-1] * 2 + alpha[:-2, 1:-1] + alpha[2:, 1:-1] + alpha[1:-1, :-2]
                                 + alpha[1:-1, 2:]) / 6.0            # soft edge: the order of resize and threshold matters
            rgba = np.concatenate([np.zeros((mh, mw, 3)), alpha[..., None]], -1)
            Image.fromarray(np.rint(rgba).astype(np.uint8), "RGBA").save(os.path.join(mdir, f"{v:08d}.png"))
    return inst
