"""The MVS inputs of a scan loaded on the GPU: `MVSDataset` with the surface of the reference's class
(datasets/general_eval.py:12-273) and no OpenCV or loguru underneath (csrc/svs_mvsdata.hip), and `create_scene`, the
folder of cameras and images that image-based rendering reads (runner.py:74-108).

The reference's class decodes every view of every sample each time the sample is asked for and resizes it on the host,
twice with `x2_mvsres` (1200x1600 -> 576x768 -> 1152x1536): a 3-view scan iterated four times per run costs 36 decodes
and 72 `cv2.resize` calls for 3 distinct images.  Here a view id is decoded ONCE per dataset (PIL), its 8-bit codes are
uploaded, one or two kernels turn them into the planes `imgs` (3,H,W) and `masks` (1,H,W), and those stay on the device;
a sample is a stack of cached views.  `decoded_views` counts the real decodes.

    ds = svs_hip.mvsdata.MVSDataset(mvs_datapath, [scan], "test", num_view, data_dir, numdepth, interval_scale,
                                    max_h=576, max_w=768, trains_i=trains_i, args=args)
    loop.cost_volumes(stage_idx, ds.device_samples(), outs_samples, view_extra)

`ds[i]` is the reference's dict of numpy arrays, so a `DataLoader` plus `tocuda` takes the class unchanged;
`ds.device_sample(i)` is what those two would deliver, without the round trip through the host.  The class is selected
explicitly: `datasets.general_eval.MVSDataset` stays the reference's.

What is restated rather than called, and so UNPINNED against OpenCV (INTEGRATION.md gives the one-line cv2 calls): the
coordinate rule of the cubic resize and `load_K_Rt_from_P` for anything but a proper camera -- both inherited from
svs_hip.scene.  A code's value here is read_img's `np.float32(code) / 255.`, a float32 division; svs_hip.scene follows
load_rgb and multiplies by float32(1/255).  The two differ by one ulp at some codes.

BlendedMVS keeps its MVS files under a folder named by a hash: `scan2hash` and `register_blendedmvs_hash` are
svs_hip/scans.py's and stay importable from here; a BlendedMVS scan whose folder name nobody supplied is a LookupError.

    python -m svs_hip.mvsdata --data-dir-root data_s_volsdf --dataset DTU --scan 106 \\
        [--max-h 576 --max-w 768 --no-x2] [--create-scene data_ibr]
"""
import argparse
import copy
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import lib as _lib
from . import scene as _scene
from .images import Phases, cubic_table, read_png, tables_device, to_device, upload_codes
from .ops import _ptr, _stream
from .scans import _BMVS as _HASH                       # the one registry, under the name its folder names had here
from .scans import DATASETS, get_eval_ids, get_trains_ids, open_scan, read_cameras, register_blendedmvs_hash, scan2hash

NVIEWS_MAX = 5                 # general_eval.py:19
X2_SIZE = (1152, 1536)         # general_eval.py:226-229
MAX_DECODERS = 16
LAUNCHES = {"resize": 0, "pack": 0, "codes": 0}        # entry-point calls made by this process (tests, bench_mvsdata.py)
CODE_VALUES = np.arange(256, dtype=np.float32) / 255.  # np.array(img, dtype=np.float32) / 255. of every code (utils.py:27)

# ---- the kernels -----------------------------------------------------------------------------------------------------
_CODE_TABLES = {}


def _code_table(dev):
    if dev not in _CODE_TABLES:
        _CODE_TABLES[dev] = torch.from_numpy(CODE_VALUES).to(dev)
    return _CODE_TABLES[dev]


def _resize_args(src, H, W):
    """the arguments both resize entry points share, for a source tensor (V,Hs,Ws,C) of codes or float32"""
    V, Hs, Ws, C = src.shape
    tabs = [None] * 4 if (Hs, Ws) == (H, W) else tables_device(cubic_table, H, W, Hs, Ws, src.device)
    is_float = src.dtype == torch.float32
    table = None if is_float else _code_table(src.device)
    return (_ptr(src), int(is_float), _ptr(table), V, Hs, Ws, C, H, W, *[_ptr(t) for t in tabs]), (tabs, table)


def prepare_views(codes, sizes, png=False):
    """The image work of V views of one size (general_eval.py:220-232, 254, 267-268): read_img's code / 255., then
    cv2.resize(img, (W,H), interpolation=cv2.INTER_CUBIC) to every (H,W) of `sizes` in turn (one size, or the two of the
    x2_mvsres chain), the transpose and the alpha split.

    codes: (V,Hs,Ws,C) uint8, C = 3 (RGB) or 4 (RGBA), array or tensor, host or device.
    -> imgs (V,3,H,W), masks (V,1,H,W): float32 DEVICE tensors; RGBA: rgb * alpha and alpha, both after the resize;
       RGB: rgb and ones.  png=True: also (V,H,W,3) uint8 on the device, np.clip(imgs * 255, 0, 255).astype(np.uint8) as
       create_scene writes them (runner.py:106)."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    if not sizes or min(min(s) for s in sizes) < 1:
        raise ValueError(f"sizes: at least one (H,W), each size >= 1, got {sizes}")
    d = to_device(codes, torch.uint8, "mvsdata", "codes", ndim=(4,), cast=False, non_blocking=True)
    if d.shape[3] not in (3, 4):
        raise ValueError(f"codes: expected (V,Hs,Ws,3) or (V,Hs,Ws,4), got {tuple(d.shape)}")
    L = _lib.load()
    V, C = d.shape[0], d.shape[3]
    for H, W in sizes[:-1]:                                  # the channel-last passes before the last one
        out = torch.empty(V, H, W, C, dtype=torch.float32, device=d.device)
        args, keep = _resize_args(d, H, W)
        _lib.check(L.svs_mvs_resize_cubic(*args, _ptr(out), _stream()), "svs_mvs_resize_cubic")
        LAUNCHES["resize"] += 1
        d = out
    H, W = sizes[-1]
    imgs = torch.empty(V, 3, H, W, dtype=torch.float32, device=d.device)
    masks = torch.empty(V, 1, H, W, dtype=torch.float32, device=d.device)
    args, keep = _resize_args(d, H, W)
    _lib.check(L.svs_mvs_resize_pack(*args, _ptr(imgs), _ptr(masks), _stream()), "svs_mvs_resize_pack")
    LAUNCHES["pack"] += 1
    if not png:
        return imgs, masks
    return imgs, masks, to_codes(imgs)


def to_codes(imgs):
    """imgs: (V,3,H,W) float32 planes on the device, contiguous.  -> (V,H,W,3) uint8 on the device:
    np.clip(imgs * 255, 0, 255).astype(np.uint8), channel-last (runner.py:106); one launch per view."""
    V, _, H, W = imgs.shape
    L = _lib.load()
    out = torch.empty(V, H, W, 3, dtype=torch.uint8, device=imgs.device)
    for v in range(V):
        _lib.check(L.svs_mvs_codes(_ptr(imgs[v]), H, W, _ptr(out[v]), _stream()), "svs_mvs_codes")
        LAUNCHES["codes"] += 1
    return out


# ---- host arithmetic -------------------------------------------------------------------------------------------------
def scaled_size(h, w, max_w, max_h, base=32):
    """scale_mvs_input's size arithmetic (general_eval.py:160-170) in Python floats, exactly as written.
    -> new_h, new_w (ints), scale_h, scale_w (the factors of the intrinsics' rows)"""
    if h != max_h or w != max_w:
        scale = 1.0 * max_h / h
        if scale * w > max_w:
            scale = 1.0 * max_w / w
        new_w, new_h = scale * w // base * base, scale * h // base * base
    else:
        new_w, new_h = 1.0 * w // base * base, 1.0 * h // base * base
    return int(new_h), int(new_w), 1.0 * new_h / h, 1.0 * new_w / w


def _arg(args, name, default=None):
    """`args` is the hydra object or a plain dict"""
    if args is None:
        return default
    if hasattr(args, "get"):
        return args.get(name, default)
    return getattr(args, name, default)


def read_view_codes(path):
    """-> (H,W,3) or (H,W,4) uint8, or ValueError: 8-bit RGB and RGBA files only"""
    a = read_png(path)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"{path}: expected an 8-bit RGB or RGBA image, got {a.dtype} {a.shape}")
    return a


class MVSDataset(torch.utils.data.Dataset):
    """The reference's MVSDataset (general_eval.py:12-273): same arguments, asserts, attributes and items.  The cached
    views are shared between the samples and READ-ONLY."""

    def __init__(self, datapath, listfile, mode, nviews, data_dir, ndepths=192, interval_scale=1.06, *, max_h, max_w,
                 trains_i=None, args=None, phases=None):
        super().__init__()
        self.datapath, self.listfile, self.mode, self.nviews = datapath, listfile, mode, nviews
        self.nviews_max = NVIEWS_MAX
        self.ndepths, self.interval_scale, self.data_dir = ndepths, interval_scale, data_dir
        self._max_h, self._max_w = max_h, max_w
        self.hparams = args if args is not None else dict()
        self.trains_i = trains_i
        self.fix_wh = False
        self.phases = phases or Phases()
        self.decoded_views = 0
        self._views, self._png, self._src_size = {}, {}, {}

        assert len(listfile) == 1                            # one scan at a time
        assert self.mode == "test"
        if self.data_dir != 'DTU':
            assert interval_scale == 1
        assert self.data_dir in DATASETS
        assert self.trains_i is not None

        self.meta_from_idr(listfile[0], self.data_dir)
        self.metas = self.build_list()
        assert self.trains_i == [x[1] for x in self.metas]

    # ---- general_eval.py:40-81 ----
    def meta_from_idr(self, scan, data_dir):
        """camera matrices, the scale matrix and the image paths of the IDR-format folder"""
        _, image_dir, cam_file, self.image_paths_idr = open_scan(_arg(self.hparams, "data_dir_root"), data_dir, scan[4:])
        assert os.path.exists(image_dir), f"{image_dir} is empty"
        assert os.path.exists(cam_file), f"{cam_file} is empty"
        scale_mats, world_mats = read_cameras(cam_file, len(self.image_paths_idr))
        self.intrinsics_idr, self.pose_idr = [], []
        scan5 = scan == 'scan5'                              # that scan's scale_mat is wrong: 1 instead
        for scale_mat, world_mat in zip(scale_mats, world_mats):
            P = world_mat @ scale_mat if scan5 else world_mat
            intrinsics, pose = _scene.load_K_Rt_from_P(None, P[:3, :4])
            self.intrinsics_idr.append(intrinsics)
            self.pose_idr.append(pose)
        if scan5:
            self.scale_mat, self.scale_factor = None, 1.0
            self._scale_mvs = scale_mats[0][0, 0]
        else:
            self.scale_mat = scale_mats[0]                   # first image of the scene
            self.scale_factor = scale_mats[0][0, 0]

    # ---- general_eval.py:83-125 ----
    def build_list(self):
        """(scan, reference view, its source views in the order of the pair file, scan) per id of trains_i"""
        metas, interval_scale_dict = [], {}
        for scan in self.listfile:
            interval_scale_dict[scan] = self.interval_scale if isinstance(self.interval_scale, float) \
                else self.interval_scale[scan]
            if self.data_dir == 'DTU':
                pair_file = f"{scan}/pair.txt"
                if not os.path.exists(os.path.join(self.datapath, pair_file)):
                    pair_file = "scan1/pair.txt"
            else:
                pair_file = f"{scan2hash(scan)}/cams/pair.txt"
            assert os.path.exists(os.path.join(self.datapath, pair_file))
            with open(os.path.join(self.datapath, pair_file)) as f:
                for _ in range(int(f.readline())):
                    ref_view = int(f.readline().rstrip())
                    src_views = [int(x) for x in f.readline().rstrip().split()[1::2]]
                    if len(src_views) > 0 and ref_view in self.trains_i:
                        metas.append((scan, ref_view, src_views, scan))
        metas = [metas[[x[1] for x in metas].index(y)] for y in self.trains_i]     # ValueError: an id without a pair entry
        self.interval_scale = interval_scale_dict
        return metas

    def __len__(self):
        return len(self.metas)

    # ---- general_eval.py:130-155 ----
    def read_cam_file(self, filename, interval_scale):
        with open(filename) as f:
            lines = [line.rstrip() for line in f.readlines()]
        extrinsics = np.array(' '.join(lines[1:5]).split(), dtype=np.float32).reshape((4, 4))
        intrinsics = np.array(' '.join(lines[7:10]).split(), dtype=np.float32).reshape((3, 3))
        intrinsics[:2, :] /= 4.0
        depth_min = float(lines[11].split()[0])
        depth_interval = float(lines[11].split()[1])
        if self.data_dir == 'BlendedMVS':
            depth_max = float(lines[11].split()[-1])
            depth_interval = float(depth_max - depth_min) / self.ndepths
            return intrinsics, extrinsics, depth_min, depth_interval
        elif len(lines[11].split()) >= 3:                    # num_depth != 192 (default value)
            num_depth = lines[11].split()[2]
            depth_max = depth_min + int(float(num_depth)) * depth_interval
            depth_interval = (depth_max - depth_min) / self.ndepths
        depth_interval *= interval_scale
        return intrinsics, extrinsics, depth_min, depth_interval

    # ---- general_eval.py:178-273, without the images ----
    def view_ids(self, idx):
        """the reference view, its sources among trains_i in pair order, the remaining trains_i; at most 5"""
        _, ref_view, src_views, _ = self.metas[idx]
        srcs = [x for x in src_views if x in self.trains_i]
        ids = [ref_view] + srcs
        ids += [x for x in self.trains_i if x not in ids]
        assert ref_view not in srcs and set(ids) == set(self.trains_i)
        return ids[:self.nviews_max]

    def _depth_range(self, scan, scene_name, vid):
        if self.data_dir == 'BlendedMVS':
            cam = os.path.join(self.datapath, '{}/cams/{:0>8}_cam.txt'.format(scan2hash(scan), vid))
            _, _, depth_min, depth_interval = self.read_cam_file(cam, interval_scale=self.interval_scale[scene_name])
            if scan == 'scan5':
                depth_min, depth_interval = depth_min / self._scale_mvs, depth_interval / self._scale_mvs
            if scan in ['scan4', 'scan5']:
                depth_max = depth_min + self.ndepths * depth_interval
                depth_max = min(depth_max, depth_min * 2.197)
                depth_interval = float(depth_max - depth_min) / self.ndepths
            return depth_min, depth_interval
        return 425, 2.5 * self.interval_scale[scene_name]

    def source_size(self, vid):
        """(h, w) of a view's file, from its header"""
        if vid not in self._src_size:
            from PIL import Image
            with Image.open(self.image_paths_idr[vid]) as im:
                self._src_size[vid] = (im.size[1], im.size[0])
        return self._src_size[vid]

    def passes(self, h, w, intrinsics=None):
        """The sizes a (h,w) image goes through (general_eval.py:225-232) and, when given, its intrinsics after them.
        -> [(H,W), ...] (one entry, or two with x2_mvsres), intrinsics"""
        sizes = []
        if _arg(self.hparams, "x2_mvsres", False):
            _s_hw = 1536 / self._max_w
            assert self._max_w * _s_hw == 1536 and self._max_h * _s_hw == 1152
            chain = [(self._max_w, self._max_h, 1), (X2_SIZE[1], X2_SIZE[0], 32)]
        else:
            chain = [(self._max_w, self._max_h, 32)]
        for max_w, max_h, base in chain:
            new_h, new_w, scale_h, scale_w = scaled_size(h, w, max_w, max_h, base)
            if intrinsics is not None:
                intrinsics = copy.deepcopy(intrinsics)
                intrinsics[0, :] *= scale_w
                intrinsics[1, :] *= scale_h
            sizes.append((new_h, new_w))
            h, w = new_h, new_w
        return sizes, intrinsics

    def sample_meta(self, idx):
        """Everything of sample `idx` but `imgs` and `masks`, on the host, with the reference's dtypes."""
        scan, ref_view, _, scene_name = self.metas[idx]
        ids = self.view_ids(idx)
        proj_matrices, size = [], None
        for vid in ids:
            intrinsics = copy.deepcopy(self.intrinsics_idr[vid][:3, :3])
            intrinsics[:2, :] /= 4.0
            extrinsics = np.linalg.inv(self.pose_idr[vid])
            sizes, intrinsics = self.passes(*self.source_size(vid), intrinsics)
            size = size or sizes[-1]
            assert sizes[-1] == size                         # all images have the same size
            proj_mat = np.zeros(shape=(2, 4, 4), dtype=np.float32)
            proj_mat[0, :4, :4] = extrinsics
            proj_mat[1, :3, :3] = intrinsics
            proj_matrices.append(proj_mat)
        depth_min, depth_interval = self._depth_range(scan, scene_name, ids[0])
        depth_values = np.arange(depth_min, depth_interval * (self.ndepths - 0.5) + depth_min, depth_interval,
                                 dtype=np.float32)
        cam_near_far = np.array([depth_min, depth_interval, self.ndepths, depth_interval * self.ndepths + depth_min])
        proj_matrices = np.stack(proj_matrices)
        stage2 = proj_matrices.copy()
        stage2[:, 1, :2, :] = proj_matrices[:, 1, :2, :] * 2
        stage3 = proj_matrices.copy()
        stage3[:, 1, :2, :] = proj_matrices[:, 1, :2, :] * 4
        return {"proj_matrices": {"stage1": proj_matrices, "stage2": stage2, "stage3": stage3},
                "depth_values": depth_values, "cam_near_far": cam_near_far,
                "filename": scan + '/{}/' + '{:0>8}'.format(ids[0]) + "{}"}

    # ---- the views: decoded and resized once, kept on the device ----
    def _load(self, vids, png=False):
        """Brings the views `vids` into the cache (and their PNG codes with png=True); files are decoded on a thread
        pool, views of one source shape go through the kernels together."""
        want = [v for v in dict.fromkeys(vids) if v not in self._views or (png and v not in self._png)]
        if not want:
            return
        ph, t0 = self.phases, time.perf_counter()
        with ThreadPoolExecutor(max_workers=min(MAX_DECODERS, len(want), os.cpu_count() or 1)) as pool:
            decoded = list(pool.map(read_view_codes, [self.image_paths_idr[v] for v in want]))
        self.decoded_views += len(want)
        groups = {}
        for v, a in zip(want, decoded):
            groups.setdefault(a.shape, []).append((v, a))
        t0 = ph.add("decode", t0)
        for shape, members in groups.items():
            stack = upload_codes(np.stack([a for _, a in members]), ph)
            t0 = ph.add("upload", t0)
            out = prepare_views(stack, self.passes(shape[0], shape[1])[0], png=png)
            t0 = ph.add("kernels", t0)
            for k, (v, _) in enumerate(members):
                self._views[v] = (out[0][k], out[1][k])
                if png:
                    self._png[v] = out[2][k]

    def view(self, vid):
        """-> imgs (3,H,W), masks (1,H,W) of view id `vid`: float32 tensors on the device, READ-ONLY"""
        self._load([vid])
        return self._views[vid]

    def png_codes(self, vid):
        """-> (H,W,3) uint8 numpy array: np.clip(imgs * 255, 0, 255).astype(np.uint8) of view `vid`, channel-last, as
        create_scene writes it (a view that was cached without its codes is decoded again)"""
        self._load([vid], png=True)
        t0 = time.perf_counter()
        out = self._png[vid].cpu().numpy()
        self.phases.bytes_down += out.size
        self.phases.add("download", t0)
        return out

    def _stacked(self, idx):
        ids = self.view_ids(idx)
        self._load(ids)
        imgs = torch.stack([self._views[v][0] for v in ids])
        masks = torch.stack([self._views[v][1] for v in ids])
        return imgs, masks

    def __getitem__(self, idx):
        """the reference's dict, numpy arrays (general_eval.py:267-273)"""
        imgs, masks = self._stacked(idx)
        t0 = time.perf_counter()
        out = {"imgs": imgs.cpu().numpy(), "masks": masks.cpu().numpy()}
        self.phases.bytes_down += out["imgs"].nbytes + out["masks"].nbytes
        self.phases.add("download", t0)
        out.update(self.sample_meta(idx))
        return out

    def device_sample(self, idx):
        """Sample `idx` as `DataLoader(batch_size=1)` plus `tocuda` deliver it, the images never leaving the device:
        imgs (1,N,3,H,W), masks (1,N,1,H,W), proj_matrices[stage] (1,N,2,4,4), depth_values (1,D) float32,
        cam_near_far (1,4) float64, filename [str]."""
        imgs, masks = self._stacked(idx)
        meta = self.sample_meta(idx)
        dev = imgs.device

        def put(a):
            return torch.from_numpy(a)[None].to(dev)
        return {"imgs": imgs[None], "masks": masks[None],
                "proj_matrices": {k: put(v) for k, v in meta["proj_matrices"].items()},
                "depth_values": put(meta["depth_values"]), "cam_near_far": put(meta["cam_near_far"]),
                "filename": [meta["filename"]]}

    def device_samples(self):
        self._load([v for i in range(len(self)) for v in self.view_ids(i)])          # one decode pool, one kernel call
        return [self.device_sample(i) for i in range(len(self))]


# ---- runner.py:74-108 ------------------------------------------------------------------------------------------------
def create_scene(out_folder, dataset, evals_i=None):
    """The folder image-based rendering reads (svs_hip.ibr, `evalviews --ibr`): {out_folder}/{scan}/cams/{id:08d}_cam.txt
    for every sample of `dataset` -- built with trains_i + evals_i -- and images/{id:08d}.png for the ids that are not
    evaluation views (`evals_i`; default: the scan's evaluation ids).  Only the images that are written are decoded.
    -> the ids whose image was written"""
    from PIL import Image
    from helpers.utils import write_cam
    scan = dataset.listfile[0]
    if evals_i is None:
        evals_i = get_eval_ids(dataset.data_dir, int(scan[4:]))
    os.makedirs(os.path.join(out_folder, scan), exist_ok=True)
    metas = [dataset.sample_meta(i) for i in range(len(dataset))]
    ids = [int(m["filename"].split('/')[-1][:8]) for m in metas]
    dataset._load([i for i in ids if i not in evals_i], png=True)
    written = []
    for id_, meta in zip(ids, metas):
        cam_filename = os.path.join(out_folder, meta["filename"].format('cams', '_cam.txt'))
        img_filename = os.path.join(out_folder, meta["filename"].format('images', '.png'))
        os.makedirs(os.path.dirname(cam_filename), exist_ok=True)
        os.makedirs(os.path.dirname(img_filename), exist_ok=True)
        write_cam(cam_filename, meta["proj_matrices"]["stage3"][0], meta["cam_near_far"])
        if id_ not in evals_i:
            Image.fromarray(dataset.png_codes(id_), "RGB").save(img_filename)
            written.append(id_)
    return written


# ---- command line ----------------------------------------------------------------------------------------------------
def main(argv=None):
    p = argparse.ArgumentParser(description="Loads the MVS inputs of one scan on the GPU (the reference's MVSDataset) and "
                                            "reports what it found; with --create-scene it writes the folder of cameras "
                                            "and images that image-based rendering reads.")
    p.add_argument("--data-dir-root", required=True, help="holds {DTU|BlendedMVS}/{scanN/{image,cameras.npz},mvs_data}")
    p.add_argument("--dataset", required=True, choices=DATASETS)
    p.add_argument("--scan", type=int, required=True)
    p.add_argument("--num-view", type=int, default=3)
    p.add_argument("--max-h", type=int, default=576)
    p.add_argument("--max-w", type=int, default=768)
    p.add_argument("--no-x2", action="store_true", help="x2_mvsres off: one resize to at most max-h x max-w")
    p.add_argument("--ndepths", type=int, default=192)
    p.add_argument("--interval-scale", type=float, help="default: 1.06 for DTU, 1 for BlendedMVS")
    p.add_argument("--create-scene", metavar="OUT", help="write OUT/scanN/{cams,images}")
    a = p.parse_args(argv)
    scan = f"scan{a.scan}"
    interval = a.interval_scale if a.interval_scale is not None else (1.06 if a.dataset == "DTU" else 1.0)
    args = dict(data_dir_root=a.data_dir_root, x2_mvsres=not a.no_x2)
    datapath = os.path.join(a.data_dir_root, a.dataset, "mvs_data")
    trains_i = get_trains_ids(a.dataset, scan, a.num_view)

    def dataset(ids):
        return MVSDataset(datapath, [scan], "test", a.num_view, a.dataset, a.ndepths, interval, max_h=a.max_h,
                          max_w=a.max_w, trains_i=list(ids), args=args, phases=Phases(sync=True))

    t0 = time.perf_counter()
    ds = dataset(trains_i)
    samples = ds.device_samples()
    total = time.perf_counter() - t0
    h, w = ds.source_size(trains_i[0])
    print(f"{a.dataset} {scan}: {len(ds)} samples, {ds.decoded_views} views decoded, {h}x{w} -> "
          + " -> ".join(f"{s[0]}x{s[1]}" for s in ds.passes(h, w)[0])
          + f", depth {float(samples[0]['depth_values'][0, 0]):.4g} .. {float(samples[0]['depth_values'][0, -1]):.4g} "
          f"({ds.ndepths} values), scale_factor {float(ds.scale_factor):.6g}")
    for i in range(len(ds)):
        print(f"  sample {i}: views {ds.view_ids(i)}, imgs {tuple(samples[i]['imgs'].shape)}, "
              f"mask covers {100.0 * float(samples[i]['masks'][0, 0].mean()):6.2f} %")
    print(ds.phases.summary(total))
    if a.create_scene:
        evals_i = get_eval_ids(a.dataset, a.scan)
        t0 = time.perf_counter()
        both = dataset(list(trains_i) + [i for i in evals_i if i not in trains_i])
        written = create_scene(a.create_scene, both, evals_i)
        total = time.perf_counter() - t0
        print(f"{os.path.join(a.create_scene, scan)}: {len(both)} cams, images {written} ({both.decoded_views} decoded)")
        print(both.phases.summary(total))
    print(f"launches {dict(LAUNCHES)}")


if __name__ == "__main__":
    main()
