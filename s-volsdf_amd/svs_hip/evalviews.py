"""Evaluation views of a checkpoint on the HIP path (eval_vsdf.py --eval_rendering; csrc/svs_evalviews.hip).

The reference renders every evaluation view of a scan from a checkpoint, moves the merged per-ray outputs to the host and
finishes them in numpy: eval_XXX.png, normal_XXX.png, dep_XXX.png and depth_est/XXXXXXXX.pfm (eval_vsdf.py:156-262).  Its
script imports TensorFlow, lpips_tf, pyhocon, cv2 and scikit-image.  Here `renderer.render_image` renders on the device,
`finish_view` turns its tensors into the four images with two kernels (one pass over the (N,S) weights), and only those
leave the device; a writer thread encodes view k while view k+1 renders.  The folder is what `svs_hip.ibr` and
`svs_hip.nvs` read, and `--ibr` / `--score` run them right after:

    python -m svs_hip.evalviews --ckpt exps_vsdf/ours_106/2026_01_01_00_00_00/checkpoints --checkpoint latest \\
        --data-dir-root data_s_volsdf --dataset DTU --scan 106 [--img-res 576 768] [--evals-folder exps_result] \\
        [--expname ours] [--split-n-pixels 512] [--views 1 2 9 ...] [--ibr MVS_SCAN_FOLDER] [--score]
        [--lpips-vgg vgg16.pth --lpips-lin vgg_lin.pth]

dep_XXX.png needs matplotlib's `turbo` colour table, which is read from matplotlib at run time; without matplotlib that
one file is skipped with one warning.  LPIPS is not computed; the mesh is `svs_hip.mesh`.
"""
import argparse
import os
import time
import warnings
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import lib as _lib
from . import scene as _scene
from .images import device, seconds_line
from .ops import _f32, _ptr, _stream
from .renderer import render_image
from .scans import DATASETS, IMG_RES, get_eval_ids, get_trains_ids

RENDER_KEYS = ("rgb_values", "normal_map", "depth_values", "weights")      # what eval_vsdf.py:220-225 keeps per chunk
EPS_F32 = float(np.finfo(np.float32).eps)
LAUNCHES = {"finish": 0, "colors": 0}                   # entry-point calls made by this process (tests, bench_evalviews.py)
_TABLES = {}
_WARNED = []


def turbo_table():
    """matplotlib's 256-entry `turbo` table as float64 (256,3) (what cm.get_cmap('turbo') looks colours up in), or None
    with ONE warning when matplotlib does not import."""
    if "turbo" not in _TABLES:
        try:
            import matplotlib
            _TABLES["turbo"] = np.ascontiguousarray(matplotlib.colormaps["turbo"](np.arange(256))[:, :3], dtype=np.float64)
        except Exception as e:                          # noqa: BLE001  (no matplotlib, or one without the table)
            _TABLES["turbo"] = None
            if not _WARNED:
                _WARNED.append(True)
                warnings.warn(f"matplotlib's turbo colour table is not available ({e}): dep_XXX.png is not written")
    return _TABLES["turbo"]


def _table_dev(cmap, dev):
    if cmap is None:
        cmap = turbo_table()
        if cmap is None:
            return None
        key = ("turbo", dev)
        if key not in _TABLES:
            _TABLES[key] = torch.from_numpy(cmap).to(dev)
        return _TABLES[key]
    t = cmap if torch.is_tensor(cmap) else torch.from_numpy(np.ascontiguousarray(np.asarray(cmap, dtype=np.float64)))
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError(f"cmap: expected an (L,3) colour table, got {tuple(t.shape)}")
    return t.detach().to(device=dev, dtype=torch.float64).contiguous()


def depth_bounds(depth, acc, percentile=99.0):
    """The bounds visualize_cmap renders between (plots.py:399-407,444-450), on the device: the weighted percentiles
    50 -/+ percentile / 2 of `depth` under the weights `acc` -- sort, cumulative weights, np.interp's rule -- moved
    outwards by float32 eps.  The cumulative sum runs in float64 (numpy's runs in acc's float32).  -> (lo, hi) floats."""
    x, order = torch.sort(depth.reshape(-1))
    n = x.numel()
    cw = torch.cumsum(acc.reshape(-1)[order].double(), 0)
    x = x.double()
    t = torch.tensor([50.0 - percentile / 2, 50.0 + percentile / 2], dtype=torch.float64, device=x.device) * (cw[-1] / 100)
    j = (torch.searchsorted(cw, t, right=True) - 1).clamp(0, n - 1)               # the last j with cw[j] <= t
    j1 = (j + 1).clamp(max=n - 1)
    step = cw[j1] - cw[j]
    slope = (x[j1] - x[j]) / torch.where(step > 0, step, torch.ones_like(step))
    val = torch.where((j == n - 1) | (step <= 0), x[j], slope * (t - cw[j]) + x[j])
    val = torch.where(t < cw[0], x[0], val)
    lo, hi = val.tolist()
    return lo - EPS_F32, hi + EPS_F32


def finish_arrays(rgb_values, normal_map, depth_values, weights, scale_factor):
    """svs_view_finish on per-ray device tensors: rgb_values, normal_map (N,3), depth_values (N) or (N,1), weights (N,S).
    -> rgb_codes (N,3) uint8, normal_codes (N,3) uint8, depth_est (N) float32, acc (N) float32."""
    rgb, nrm, dep, w = _f32(rgb_values), _f32(normal_map), _f32(depth_values), _f32(weights)
    if w.dim() != 2:
        raise ValueError(f"weights: expected (N,S), got {tuple(w.shape)}")
    N, S = w.shape
    if tuple(rgb.shape) != (N, 3) or tuple(nrm.shape) != (N, 3) or dep.numel() != N:
        raise ValueError(f"rgb_values {tuple(rgb.shape)}, normal_map {tuple(nrm.shape)} and depth_values {tuple(dep.shape)} "
                         f"do not belong to {N} rays")
    L = _lib.load()
    rgb_codes = torch.empty(N, 3, dtype=torch.uint8, device=w.device)
    normal_codes = torch.empty_like(rgb_codes)
    depth_est = torch.empty(N, dtype=torch.float32, device=w.device)
    acc = torch.empty_like(depth_est)
    _lib.check(L.svs_view_finish(_ptr(rgb), _ptr(nrm), _ptr(dep), _ptr(w), N, S, float(scale_factor), _ptr(rgb_codes),
                                 _ptr(normal_codes), _ptr(depth_est), _ptr(acc), _stream()), "svs_view_finish")
    LAUNCHES["finish"] += 1
    return rgb_codes, normal_codes, depth_est, acc


def depth_colors(depth_values, acc, img_res, lo, hi, table):
    """svs_view_depth_colors: depth_values (N) float32 unscaled, acc (N) float32, lo / hi from depth_bounds, table (L,3)
    float64 on the device.  -> (H,W,3) uint8 device tensor."""
    H, W = int(img_res[0]), int(img_res[1])
    dep, a = _f32(depth_values).reshape(-1), _f32(acc).reshape(-1)
    if dep.numel() != H * W or a.numel() != H * W:
        raise ValueError(f"depth {tuple(dep.shape)} / acc {tuple(a.shape)} are not {H}x{W} images")
    codes = torch.empty(H, W, 3, dtype=torch.uint8, device=dep.device)
    _lib.check(_lib.load().svs_view_depth_colors(_ptr(dep), _ptr(a), H * W, W, float(lo), float(hi), _ptr(table),
                                                 int(table.shape[0]), _ptr(codes), _stream()), "svs_view_depth_colors")
    LAUNCHES["colors"] += 1
    return codes


def finish_view(outputs, img_res, scale_factor, cmap=None):
    """The finish of one rendered view (eval_vsdf.py:230-262).  outputs: what renderer.render_image returns (device
    tensors; rgb_values, normal_map, depth_values and weights are read).  cmap: an (L,3) colour table, None for
    matplotlib's turbo (depth_vis is None when matplotlib is missing), False for no depth_vis.
    -> dict of device tensors: rgb (H,W,3) uint8, normal (H,W,3) uint8, depth_est (H,W) float32, acc (H,W) float32,
    depth_vis (H,W,3) uint8 or None."""
    H, W = int(img_res[0]), int(img_res[1])
    if outputs["weights"].shape[0] != H * W:
        raise ValueError(f"outputs hold {outputs['weights'].shape[0]} rays, img_res {H}x{W} has {H * W}")
    rgb, nrm, depth_est, acc = finish_arrays(outputs["rgb_values"], outputs["normal_map"], outputs["depth_values"],
                                             outputs["weights"], scale_factor)
    table = None if cmap is False else _table_dev(cmap, acc.device)
    vis = None
    if table is not None:
        dep = _f32(outputs["depth_values"]).reshape(-1)
        lo, hi = depth_bounds(dep, acc)
        vis = depth_colors(dep, acc, (H, W), lo, hi, table)
    return dict(rgb=rgb.view(H, W, 3), normal=nrm.view(H, W, 3), depth_est=depth_est.view(H, W), acc=acc.view(H, W),
                depth_vis=vis)


# ---- files -----------------------------------------------------------------------------------------------------------
def view_files(out_folder, view):
    """The reference's names for one view (eval_vsdf.py:241,246,255,262)."""
    v = int(view)
    return dict(rgb=os.path.join(out_folder, "eval_%03d.png" % v), normal=os.path.join(out_folder, "normal_%03d.png" % v),
                depth_vis=os.path.join(out_folder, "dep_%03d.png" % v),
                depth_est=os.path.join(out_folder, "depth_est", "%08d.pfm" % v))


def write_view(out_folder, view, host):
    """host: finish_view's dict as numpy arrays.  Writes the view's files; -> the paths written."""
    from PIL import Image
    from datasets.data_io import save_pfm
    names = view_files(out_folder, view)
    save_pfm(names["depth_est"], np.ascontiguousarray(host["depth_est"], dtype=np.float32))
    written = [names["depth_est"]]
    for k in ("rgb", "normal", "depth_vis"):
        if host.get(k) is not None:
            Image.fromarray(host[k]).save(names[k])
            written.append(names[k])
    return written


def _to_device(model_input, dev):
    keep = ("intrinsics", "uv", "pose", "near_pose")
    return {k: v.to(dev) for k, v in model_input.items() if k in keep}


def render_views(model, dataset, view_ids, out_folder, split_n_pixels=512, fast=-1, rank=0, world=1, cmap=None,
                 seconds=None):
    """Renders the views `view_ids` of `dataset` (a SceneDataset) with `model` (eval mode, on the GPU) and writes
    eval_%03d.png, normal_%03d.png, dep_%03d.png and depth_est/%08d.pfm under out_folder (eval_vsdf.py:179-262).  The
    files of view k are written by a helper thread while view k+1 renders; at most one view is in flight.  world > 1:
    every rank renders its share of each view (renderer.shard_pixels) and rank 0 finishes and writes.  `seconds`, when
    given, receives the seconds per phase (render, finish, write: the time the loop waited for the writer).
    -> the list of written paths (rank 0)."""
    if model.training:
        raise ValueError("render_views renders in eval mode: call model.eval()")
    sec = seconds if seconds is not None else OrderedDict()
    for k in ("render", "finish", "write"):
        sec.setdefault(k, 0.0)
    dev = next(model.parameters()).device
    H, W = int(dataset.img_res[0]), int(dataset.img_res[1])
    if rank == 0:
        os.makedirs(os.path.join(out_folder, "depth_est"), exist_ok=True)
    written, pending = [], None
    with ThreadPoolExecutor(max_workers=1) as writer:
        for v in view_ids:
            v = int(v)
            if not 0 <= v < len(dataset):
                raise IndexError(f"view {v}: the scan holds {len(dataset)} images")
            t0 = time.perf_counter()
            _, model_input, _ = dataset.collate_fn([dataset[v]])
            out = render_image(model, _to_device(model_input, dev), H * W, split_n_pixels=split_n_pixels, fast=fast,
                               keys=RENDER_KEYS, rank=rank, world=world)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            sec["render"] += t1 - t0
            if rank != 0:
                continue
            res = finish_view(out, (H, W), dataset.scale_factor, cmap=cmap)
            host = {k: (t.cpu().numpy() if t is not None else None) for k, t in res.items()}
            del out, res
            t2 = time.perf_counter()
            sec["finish"] += t2 - t1
            if pending is not None:
                written += pending.result()
            pending = writer.submit(write_view, out_folder, v, host)
            sec["write"] += time.perf_counter() - t2
        t2 = time.perf_counter()
        if pending is not None:
            written += pending.result()
        sec["write"] += time.perf_counter() - t2
    return written


# ---- checkpoint -> folder ---------------------------------------------------------------------------------------------
def find_checkpoint(ckpt, checkpoint="latest"):
    """--ckpt: a ModelParameters/*.pth file, an experiment's `checkpoints` folder (or the run folder that holds it) plus
    the checkpoint's name (eval_vsdf.py:103).  -> the .pth path."""
    if os.path.isfile(ckpt):
        return ckpt
    for base in (ckpt, os.path.join(ckpt, "checkpoints")):
        fn = os.path.join(base, "ModelParameters", f"{checkpoint}.pth")
        if os.path.isfile(fn):
            return fn
    raise FileNotFoundError(f"no checkpoint {checkpoint!r} under {ckpt}: expected a .pth file or a folder holding "
                            f"ModelParameters/{checkpoint}.pth")


def default_views(dataset, scan):
    """The views the reference renders (eval_vsdf.py:162-172): the evaluation ids, then the first three training ids (the
    sources of image-based rendering).  -> (views, train ids)"""
    test = list(get_eval_ids(dataset, scan_id=scan))
    train = list(get_trains_ids(dataset, f"scan{scan}", num_views=3))[:3]
    if dataset == "BlendedMVS":
        assert test == [i for i in test if i not in train]
    return test + train, train


def build_model(dataset):
    """The mirror model with the model section VolOpt runs for that dataset (volsdf/utils/conf.py)."""
    from volsdf.utils.conf import bmvs_model_conf, dtu_model_conf
    if dataset == "DTU":
        from volsdf.model.network import VolSDFNetwork
        return VolSDFNetwork(conf=dtu_model_conf())
    if dataset == "BlendedMVS":
        from volsdf.model.network_bg import VolSDFNetworkBG
        return VolSDFNetworkBG(conf=bmvs_model_conf())
    raise NotImplementedError(f"dataset {dataset!r}: only {DATASETS}")


def load_model(ckpt_file, dataset, device):
    """-> (model in eval mode on `device`, the checkpoint's epoch).  The state dict is loaded strictly."""
    saved = torch.load(ckpt_file, map_location="cpu")
    model = build_model(dataset)
    model.load_state_dict(saved["model_state_dict"], strict=True)
    model.to(device).eval()
    if hasattr(model, "invalidate_packed"):
        model.invalidate_packed()
    return model, saved["epoch"]


def evaluate(ckpt, data_dir_root, dataset, scan, img_res=IMG_RES, evals_folder="exps_result", expname="ours",
             checkpoint="latest", split_n_pixels=512, views=None, src_views=None, ibr=None, score=False, fast=-1,
             rank=0, world=1, log=print, lpips=None):
    """Checkpoint -> {evals_folder}/{expname}_{scan}/rendering_{epoch} (eval_vsdf.py:157) with the files of every view.
    views: explicit ids, or None for default_views().  ibr: the scan's MVS folder (cams/, images/): blends every view that
    is not a source from `src_views` (default: the training ids among the views) with svs_hip.ibr; score: svs_hip.nvs
    on those views ('blend' after ibr, 'default' otherwise), with the LPIPS line when `lpips` is a svs_hip.lpips.LpipsNet.
    -> dict(folder, epoch, views, written, seconds, scores)."""
    dev = device("evalviews")
    sec = OrderedDict((k, 0.0) for k in ("load", "render", "finish", "write"))
    t0 = time.perf_counter()
    if views is None:
        views, train = default_views(dataset, scan)
    else:
        views = [int(v) for v in views]
        try:
            train = list(get_trains_ids(dataset, f"scan{scan}", num_views=3))[:3]
        except LookupError:
            train = []
    src = [int(v) for v in src_views] if src_views is not None else [v for v in views if v in train]
    ckpt_file = find_checkpoint(ckpt, checkpoint)
    model, epoch = load_model(ckpt_file, dataset, dev)
    ds = _scene.SceneDataset(dataset, [int(img_res[0]), int(img_res[1])], scan_id=int(scan), data_dir_root=data_dir_root)
    folder = os.path.join(evals_folder, f"{expname}_{scan}", f"rendering_{epoch}")
    sec["load"] = time.perf_counter() - t0
    log(f"rendered images dir: {folder}")
    log(f"{len(views)} images (including train)")
    written = render_views(model, ds, views, folder, split_n_pixels=split_n_pixels, fast=fast, rank=rank, world=world,
                           seconds=sec)
    log(seconds_line(sec))
    res = dict(folder=folder, epoch=epoch, views=views, written=written, seconds=sec, scores=None)
    if rank != 0:
        return res
    refs = [v for v in views if v not in src]
    if ibr:
        from . import ibr as _ibr
        if not src:
            raise ValueError("--ibr needs source views: none of the rendered views is a training view (give --src-views)")
        t0 = time.perf_counter()
        res["written"] = written + _ibr.image_based_render(ibr, folder, refs, src)
        sec["ibr"] = time.perf_counter() - t0
    if score:
        from . import nvs as _nvs
        t0 = time.perf_counter()
        res["scores"] = _nvs.score_scan(folder, data_dir_root, dataset, scan, refs, result_from="blend" if ibr else "default",
                                        img_res=tuple(int(x) for x in img_res), scene=ds, **({} if lpips is None else dict(lpips=lpips)))
        sec["score"] = time.perf_counter() - t0
        for line in _nvs.scan_lines(scan, res["scores"]["psnr"], res["scores"]["ssim"], res["scores"].get("lpips")):
            log(line)
    return res


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Renders the evaluation views of a scan from a checkpoint on the GPU (the "
                                            "reference's eval_vsdf.py --eval_rendering): eval_XXX.png, normal_XXX.png, "
                                            "dep_XXX.png and depth_est/XXXXXXXX.pfm per view.")
    p.add_argument("--ckpt", required=True, help="a ModelParameters/*.pth file, or an experiment's checkpoints folder")
    p.add_argument("--checkpoint", default="latest", help="the checkpoint's name when --ckpt is a folder")
    p.add_argument("--data-dir-root", required=True, help="holds {DTU|BlendedMVS}/scanN/{image,cameras.npz} and .../eval_mask")
    p.add_argument("--dataset", required=True, choices=DATASETS)
    p.add_argument("--scan", type=int, required=True)
    p.add_argument("--img-res", type=int, nargs=2, default=IMG_RES, metavar=("H", "W"))
    p.add_argument("--evals-folder", default="exps_result", help="the evaluation folder (created)")
    p.add_argument("--expname", default="ours")
    p.add_argument("--split-n-pixels", type=int, default=512, help="rays per sampler decision (the reference's chunk)")
    p.add_argument("--views", type=int, nargs="+", default=None,
                   help="view ids; default: the evaluation ids and the first three training ids")
    p.add_argument("--src-views", type=int, nargs="+", default=None,
                   help="source views of --ibr; default: the training ids among the views")
    p.add_argument("--ibr", metavar="MVS_SCAN_FOLDER", default=None,
                   help="blend the views with svs_hip.ibr; the folder holds cams/{:08d}_cam.txt and images/{:08d}.png")
    p.add_argument("--score", action="store_true", help="print the SCAN block of svs_hip.nvs for the rendered views")
    from .nvs import add_lpips_arguments
    add_lpips_arguments(p)
    return p.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    from .nvs import lpips_from_arguments
    net = lpips_from_arguments(a) if a.score else None
    return evaluate(a.ckpt, a.data_dir_root, a.dataset, a.scan, img_res=tuple(a.img_res), evals_folder=a.evals_folder,
                    expname=a.expname, checkpoint=a.checkpoint, split_n_pixels=a.split_n_pixels, views=a.views,
                    src_views=a.src_views, ibr=a.ibr, score=a.score, lpips=net)


if __name__ == "__main__":
    main()
