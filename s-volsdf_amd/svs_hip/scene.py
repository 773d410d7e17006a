"""A scan folder loaded on the GPU: `SceneDataset` with the surface of the reference's class
(volsdf/datasets/scene_dataset.py:94-282) and no OpenCV, imageio or scikit-image underneath (csrc/svs_scene.hip).

The reference's class turns every image of the folder into `rgb` (cv2.resize INTER_CUBIC of code / 255), `rgb_smooth`
(cv2.GaussianBlur (31,31), 90), `mask` (cv2.resize + threshold) and `intrinsics` / `pose`
(cv2.decomposeProjectionMatrix).  Here PIL decodes the files, the 8-bit codes are uploaded, three kernels do the image
work for a chunk of views per call, and one copy per chunk brings the float32 results back into a pinned host tensor
whose rows the lists `rgb_images` / `rgb_smooth` / `masks` are views of -- CPU float32 (H*W,3) tensors as the
reference's, so `VolOpt`, `CachedItems`, `DeviceBatches` and a `DataLoader` take the class unchanged:

    VolOpt(..., dataset_class=svs_hip.scene.SceneDataset)      or      train.dataset_class = svs_hip.scene.SceneDataset

The default dataset class stays the reference's.  `VolOpt` builds the dataset of one scan five times with the same
arguments (four at full size); a process-wide cache keyed by the folder, `img_res` and every file's size and mtime does
the image work once and hands out the same READ-ONLY tensors (SVS_SCENE_CACHE=0 turns it off).

What is restated rather than called, and so UNPINNED against OpenCV (INTEGRATION.md gives the one-line cv2 call to check
each against): the coordinate rule of the cubic / linear resize, the reference's mask call
`cv2.resize(mask, (W,H), cv2.INTER_NEAREST)` -- whose third positional parameter is `dst`, so INTER_LINEAR runs -- and
`load_K_Rt_from_P` for anything but a proper camera.

View ids (`get_trains_ids`, `get_eval_ids`, `get_near_id`, `register_blendedmvs_ids`) and the opening of the folder are
svs_hip/scans.py's; the names stay importable from here.  A BlendedMVS scan whose id tables nobody supplied is a
LookupError that says how to.

    python -m svs_hip.scene --data-dir-root data_s_volsdf --dataset DTU --scan 106 [--img-res 576 768]
"""
import argparse
import os
import random
import time
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import lib as _lib
from .images import (Phases, cubic_table, linear_table, read_bmvs_alpha, read_dtu_mask, read_rgb8, tables_device, to_device,
                     upload_codes)
from .ops import _ptr, _stream
from .scans import (_BMVS, BMVS_ALPHA_DIVISOR, DATASETS, DTU_EXCLUDE_IDS, DTU_TRAIN_IDS, DTU_UNMASKED_SCANS, IMG_RES,
                    get_eval_ids, get_near_id, get_trains_ids, open_scan, read_cameras, register_blendedmvs_ids,
                    scan_mask_files)                      # _BMVS: the one registry, under the name it had here

CHUNK = 8                      # views per kernel call: bounds device memory (8 x 1200x1600 codes + 3 float images of 576x768)
MAX_DECODERS = 16
CACHE_ENTRIES = 4              # (scan, img_res) results kept: the full-size and the plot-size build of two scans
LAUNCHES = {"resize": 0, "smooth": 0, "mask": 0}       # entry-point calls made by this process (tests, bench_scene.py)

# ---- the kernels -----------------------------------------------------------------------------------------------------
def prepare_images(codes, img_res):
    """codes: (V,Hs,Ws,3) uint8 RGB codes, array or tensor, host or device.  -> rgb, rgb_smooth: float32 DEVICE tensors
    (V,H*W,3): cv2.resize(code * (1/255), (W,H), INTER_CUBIC) (code * (1/255) itself at equal sizes) and
    cv2.GaussianBlur(rgb, (31,31), 90) of it (scene_dataset.py:163-175)."""
    H, W = int(img_res[0]), int(img_res[1])
    d = to_device(codes, torch.uint8, "scene", "codes", ndim=(4,), cast=False, non_blocking=True)
    V, Hs, Ws, C = d.shape
    if C != 3:
        raise ValueError(f"codes: expected (V,Hs,Ws,3), got {tuple(d.shape)}")
    L = _lib.load()
    rgb = torch.empty(V, H * W, 3, dtype=torch.float32, device=d.device)
    smooth = torch.empty_like(rgb)
    tabs = [None] * 4 if (Hs, Ws) == (H, W) else tables_device(cubic_table, H, W, Hs, Ws, d.device)
    _lib.check(L.svs_scene_resize_cubic(_ptr(d), V, Hs, Ws, H, W, *[_ptr(t) for t in tabs], _ptr(rgb), _stream()),
               "svs_scene_resize_cubic")
    LAUNCHES["resize"] += 1
    ws = torch.empty(int(L.svs_scene_workspace_bytes(V, H, W)), dtype=torch.uint8, device=d.device)
    _lib.check(L.svs_scene_smooth(_ptr(rgb), V, H, W, _ptr(ws), _ptr(smooth), _stream()), "svs_scene_smooth")
    LAUNCHES["smooth"] += 1
    return rgb, smooth


def prepare_masks(masks01, img_res, divisor=1.0):
    """masks01: (V,Hs,Ws) uint8, read as code / divisor (0/1 codes with divisor 1; an alpha channel with divisor 255).
    -> float32 DEVICE tensor (V,H*W,3) of 0/1: the reference's cv2.resize(mask, (W,H), cv2.INTER_NEAREST) -- which runs
    INTER_LINEAR, its third positional parameter being dst -- and > 0.5, in all three channels (scene_dataset.py:178-202)."""
    H, W = int(img_res[0]), int(img_res[1])
    d = to_device(masks01, torch.uint8, "scene", "masks01", ndim=(3,), cast=False, non_blocking=True)
    V, Hs, Ws = d.shape
    L = _lib.load()
    out = torch.empty(V, H * W, 3, dtype=torch.float32, device=d.device)
    tabs = tables_device(linear_table, H, W, Hs, Ws, d.device)
    _lib.check(L.svs_scene_mask(_ptr(d), float(divisor), V, Hs, Ws, H, W, *[_ptr(t) for t in tabs], _ptr(out), _stream()),
               "svs_scene_mask")
    LAUNCHES["mask"] += 1
    return out


# ---- cameras ---------------------------------------------------------------------------------------------------------
def load_K_Rt_from_P(P, P_=None):
    """rend_util.load_K_Rt_from_P (volsdf/utils/rend_util.py:36-57) for a given 3x4 P (also callable as the reference's
    `(None, P)`).  -> intrinsics float64 (4,4), pose float32 (4,4).

    P[:, :3] = K R by an RQ decomposition with K's diagonal made positive, intrinsics[:3,:3] = K / K[2,2],
    pose[:3,:3] = R.T, pose[:3,3] = the null vector of P de-homogenised (the camera centre).  Computed in float64.
    cv2.decomposeProjectionMatrix reaches its RQ with Givens rotations; for a proper camera (positive focal lengths,
    det R = +1) the factorisation is unique and any RQ agrees.  UNPINNED for other inputs (a negative determinant, a
    zero on K's diagonal)."""
    P = np.asarray(P if P_ is None else P_, dtype=np.float64)
    if P.shape != (3, 4):
        raise ValueError(f"P must be 3x4, got {P.shape}")
    M = P[:, :3]
    Q, U = np.linalg.qr(np.flipud(M).T)                # RQ of M from the QR of its row-reversed transpose
    K = np.flipud(np.fliplr(U.T))
    R = np.flipud(Q.T)
    sgn = np.where(np.diag(K) < 0, -1.0, 1.0)
    K, R = K * sgn[None, :], R * sgn[:, None]
    v = np.linalg.svd(P)[2][-1]
    intrinsics = np.eye(4)
    intrinsics[:3, :3] = K / K[2, 2]
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = R.T
    pose[:3, 3] = v[:3] / v[3]
    return intrinsics, pose


# ---- files -----------------------------------------------------------------------------------------------------------
def _decode_dtu_mask(path):
    """one 0/1 mask per pixel: the three channels must agree"""
    inside = read_dtu_mask(path)
    if not (np.array_equal(inside[..., 0], inside[..., 1]) and np.array_equal(inside[..., 0], inside[..., 2])):
        raise ValueError(f"{path}: the mask's three channels differ; one mask per pixel is supported")
    return inside[..., 0].astype(np.uint8)


def _mask_files(data_dir_root, data_dir, scan_id, n_images):
    """{view: mask file} for the views whose mask the reference reads (scene_dataset.py:130-138,178,190-191), and the
    divisor of their codes (the BlendedMVS alpha codes are divided by 255 on the device)."""
    fn = scan_mask_files(data_dir_root, data_dir, scan_id)
    if data_dir == "DTU":
        if int(scan_id) in DTU_UNMASKED_SCANS:
            return {}, 1.0
        return {v: fn(v) for v in get_eval_ids("DTU") if v < n_images}, 1.0
    views = get_eval_ids("BlendedMVS", scan_id=scan_id) + get_trains_ids("BlendedMVS", scan=f"scan{scan_id}", num_views=3)
    files = {v: fn(v) for v in views if v < n_images}
    for f in files.values():
        assert os.path.exists(f), f
    return files, BMVS_ALPHA_DIVISOR


def _chunks(n, size):
    return [range(a, min(a + size, n)) for a in range(0, n, size)]


def _to_host(dst, src, ph):
    dst.copy_(src, non_blocking=True)
    ph.bytes_down += dst.numel() * dst.element_size()


def _host_tensor(*shape):
    return torch.empty(*shape, dtype=torch.float32, pin_memory=torch.cuda.is_available())


def load_images(image_paths, mask_files, mask_divisor, img_res, phases=None):
    """The image work of one scan.  -> rgb, rgb_smooth, masks: lists of CPU float32 (H*W,3) tensors, one per image, views
    of pinned host tensors; `resized`.  Views without a mask file share one tensor of ones."""
    ph = phases or Phases()
    H, W = int(img_res[0]), int(img_res[1])
    n = len(image_paths)
    host = _host_tensor(2, n, H * W, 3)
    size = None
    with ThreadPoolExecutor(max_workers=min(MAX_DECODERS, os.cpu_count() or 1)) as pool:
        chunks = _chunks(n, CHUNK)
        ahead = [pool.submit(read_rgb8, image_paths[i]) for i in chunks[0]] if chunks else []
        for c, ids in enumerate(chunks):
            cur, t0 = ahead, time.perf_counter()
            ahead = [pool.submit(read_rgb8, image_paths[i]) for i in chunks[c + 1]] if c + 1 < len(chunks) else []
            imgs = [f.result() for f in cur]
            size = size or imgs[0].shape[:2]
            for i, a in zip(ids, imgs):
                if a.shape[:2] != size:
                    raise ValueError(f"{image_paths[i]}: {a.shape[:2]} differs from the first image's {size}")
            stack = np.stack(imgs)
            t0 = ph.add("decode", t0)
            d = upload_codes(stack, ph)
            t0 = ph.add("upload", t0)
            rgb, smooth = prepare_images(d, (H, W))
            t0 = ph.add("kernels", t0)
            _to_host(host[0, ids.start:ids.stop], rgb, ph)
            _to_host(host[1, ids.start:ids.stop], smooth, ph)
            if torch.cuda.is_available():
                torch.cuda.synchronize()                 # the device buffers are reused by the next chunk
            ph.add("download", t0)
        resized = size != (H, W)

        ones = torch.ones(H * W, 3)
        masks = [ones] * n
        views = sorted(mask_files)
        if views:
            decode = _decode_dtu_mask if mask_divisor == 1.0 else read_bmvs_alpha
            mhost = _host_tensor(len(views), H * W, 3)
            msize = None
            for ids in _chunks(len(views), CHUNK):
                t0 = time.perf_counter()
                ms = list(pool.map(decode, [mask_files[views[k]] for k in ids]))
                msize = msize or ms[0].shape
                for k, m in zip(ids, ms):
                    if m.shape != msize:
                        raise ValueError(f"{mask_files[views[k]]}: {m.shape} differs from the first mask's {msize}")
                if mask_divisor == 1.0 and not resized and msize != (H, W):
                    raise ValueError(f"{mask_files[views[ids[0]]]}: {msize} mask for {(H, W)} images that are not resized")
                stack = np.stack(ms)
                t0 = ph.add("decode", t0)
                d = upload_codes(stack, ph)
                t0 = ph.add("upload", t0)
                out = prepare_masks(d, (H, W), divisor=mask_divisor)
                t0 = ph.add("kernels", t0)
                _to_host(mhost[ids.start:ids.stop], out, ph)
                if torch.cuda.is_available():
                    torch.cuda.synchronize()
                ph.add("download", t0)
            masks = list(masks)
            for k, v in enumerate(views):
                masks[v] = mhost[k]
    return [host[0, i] for i in range(n)], [host[1, i] for i in range(n)], masks, resized


_CACHE = OrderedDict()


def _stat_key(path):
    st = os.stat(path)
    return (path, st.st_size, st.st_mtime_ns)


def cache_clear():
    _CACHE.clear()


def _cached_images(instance_dir, image_paths, mask_files, mask_divisor, img_res, phases=None):
    if os.environ.get("SVS_SCENE_CACHE", "1") == "0":
        return load_images(image_paths, mask_files, mask_divisor, img_res, phases) + (False,)
    key = (os.path.realpath(instance_dir), int(img_res[0]), int(img_res[1]), mask_divisor,
           tuple(_stat_key(p) for p in image_paths), tuple((v, _stat_key(f)) for v, f in sorted(mask_files.items())))
    hit = key in _CACHE
    if hit:
        _CACHE.move_to_end(key)
    else:
        _CACHE[key] = load_images(image_paths, mask_files, mask_divisor, img_res, phases)
        while len(_CACHE) > CACHE_ENTRIES:
            _CACHE.popitem(last=False)
    rgb, smooth, masks, resized = _CACHE[key]
    return list(rgb), list(smooth), list(masks), resized, hit


# ---- the dataset -----------------------------------------------------------------------------------------------------
class SceneDataset(torch.utils.data.Dataset):
    """The reference's SceneDataset (scene_dataset.py:94-282): same arguments, attributes, items and file conventions.
    The image tensors are shared between the datasets of one scan and READ-ONLY."""

    def __init__(self, data_dir, img_res, scan_id=0, num_views=-1, data_dir_root=None, phases=None):
        if data_dir not in DATASETS:
            raise NotImplementedError(f"dataset {data_dir!r}: only {DATASETS}")
        self.data_dir, self.scan_id, self.num_views = data_dir, scan_id, num_views
        self.total_pixels = img_res[0] * img_res[1]
        self.img_res = img_res
        assert num_views in [-1, 3, 4, 5, 6, 9]
        self.mode, self.plot_id = 'train', 0
        self.sampling_idx = None
        self.use_pixel_centers = False

        instance_dir, image_dir, self.cam_file, image_paths = open_scan(data_dir_root, data_dir, scan_id)
        assert os.path.exists(image_dir), "Data directory is empty"
        assert os.path.exists(self.cam_file), "Data directory is empty"
        self.n_images = len(image_paths)
        assert self.n_images > 0, "Data directory is empty"
        scale_mats, world_mats = read_cameras(self.cam_file, self.n_images)

        from PIL import Image
        with Image.open(image_paths[0]) as im:
            w0, h0 = im.size
        scale_h, scale_w = img_res[0] * 1. / h0, img_res[1] * 1. / w0

        self.scale_factor = scale_mats[0][0, 0]
        if int(scan_id) == 5 and data_dir == "BlendedMVS":                   # that scan's scale_mat is wrong: 1 instead
            self.scale_factor = 1.0

        self.intrinsics_all, self.pose_all = [], []
        for scale_mat, world_mat in zip(scale_mats, world_mats):
            intrinsics, pose = load_K_Rt_from_P((world_mat @ scale_mat)[:3, :4])
            intrinsics[0, :] *= scale_w
            intrinsics[1, :] *= scale_h
            self.intrinsics_all.append(torch.from_numpy(intrinsics).float())
            self.pose_all.append(torch.from_numpy(pose).float())

        mask_files, divisor = _mask_files(data_dir_root, data_dir, scan_id, self.n_images)
        self.rgb_images, self.rgb_smooth, self.masks, self.resized, self.cache_hit = _cached_images(
            instance_dir, image_paths, mask_files, divisor, img_res, phases)
        self.mask_views = sorted(mask_files)

    def __len__(self):
        return self.n_images

    def trains_ids(self):
        return get_trains_ids(data_dir=self.data_dir, scan=f"scan{self.scan_id}", num_views=self.num_views)

    def __getitem__(self, idx):
        """(view index, sample, ground truth) of scene_dataset.py:211-253: with num_views >= 1 a random training view in
        train mode and the next evaluation view in plot mode; the rows of `sampling_idx` when one is set."""
        if self.num_views >= 1:
            train_ids = self.trains_ids()
            if self.mode == 'train':
                idx = train_ids[random.randint(0, self.num_views - 1)]
            elif self.mode == 'plot':
                eval_ids = get_eval_ids(data_dir=self.data_dir, scan_id=self.scan_id)
                if len(eval_ids) == 0:
                    eval_ids = [x for x in range(self.n_images) if x not in train_ids]
                idx = eval_ids[self.plot_id]
                self.plot_id = (self.plot_id + 1) % len(eval_ids)
        H, W = self.img_res[0], self.img_res[1]
        uv = np.mgrid[0:H, 0:W].astype(np.int32)
        uv = torch.from_numpy(np.flip(uv, axis=0).copy()).float().reshape(2, -1).transpose(1, 0)      # (x, y) rows
        if self.use_pixel_centers:
            uv += 0.5
        sample = {"uv": uv, "intrinsics": self.intrinsics_all[idx], "pose": self.pose_all[idx]}
        if self.data_dir == "BlendedMVS":
            sample["near_pose"] = self.pose_all[get_near_id(data_dir=self.data_dir, scan_id=self.scan_id, idx=idx)]
        gt = {"rgb": self.rgb_images[idx], "rgb_smooth": self.rgb_smooth[idx], "mask": self.masks[idx]}
        if self.sampling_idx is not None:
            gt["rgb"] = self.rgb_images[idx][self.sampling_idx, :]
            gt["rgb_smooth"] = self.rgb_smooth[idx][self.sampling_idx, :]
            sample["uv"] = uv[self.sampling_idx, :]
        return idx, sample, gt

    def collate_fn(self, batch_list):
        """dictionaries stacked key by key, indices as a LongTensor (scene_dataset.py:258-273)"""
        out = []
        for entry in zip(*batch_list):
            if type(entry[0]) is dict:
                out.append({k: torch.stack([o[k] for o in entry]) for k in entry[0].keys()})
            else:
                out.append(torch.LongTensor(entry))
        return tuple(out)

    def change_sampling_idx(self, sampling_size):
        self.sampling_idx = None if sampling_size == -1 else torch.randperm(self.total_pixels)[:sampling_size]

    def get_scale_mat(self):
        return np.load(self.cam_file)['scale_mat_0']


# ---- command line ----------------------------------------------------------------------------------------------------
def main(argv=None):
    p = argparse.ArgumentParser(description="Loads one scan folder on the GPU (the reference's SceneDataset) and reports "
                                            "what it found: a quick check that a folder loads.")
    p.add_argument("--data-dir-root", required=True, help="holds {DTU|BlendedMVS}/scanN/{image,cameras.npz} and .../eval_mask")
    p.add_argument("--dataset", required=True, choices=DATASETS)
    p.add_argument("--scan", type=int, required=True)
    p.add_argument("--img-res", type=int, nargs=2, default=IMG_RES, metavar=("H", "W"))
    a = p.parse_args(argv)
    ph = Phases(sync=True)
    t0 = time.perf_counter()
    ds = SceneDataset(a.dataset, tuple(a.img_res), scan_id=a.scan, data_dir_root=a.data_dir_root, phases=ph)
    total = time.perf_counter() - t0
    print(f"{a.dataset} scan{a.scan}: {ds.n_images} images -> {a.img_res[0]}x{a.img_res[1]} "
          f"({'resized (cubic)' if ds.resized else 'native size, no resize'}), cameras {ds.cam_file}, "
          f"scale_factor {float(ds.scale_factor):.6g}")
    print(f"rgb in [{min(float(t.min()) for t in ds.rgb_images):.4f}, {max(float(t.max()) for t in ds.rgb_images):.4f}], "
          f"{len(ds.mask_views)} views with a mask file")
    for v in ds.mask_views:
        print(f"  view {v:3d}: mask covers {100.0 * float(ds.masks[v].mean()):6.2f} %")
    print(f"{ph.summary(total)}, launches {dict(LAUNCHES)}")


if __name__ == "__main__":
    main()
