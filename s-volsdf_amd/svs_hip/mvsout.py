"""From the MVS network's outputs to the default-config point cloud on the GPU (csrc/svs_mvsout.hip): what the
reference's runner does on the host with OpenCV and scikit-image between `CascadeMVSNet` and `filter_depth`.

    final_confidence(outputs)           conf_1 * conf_2 * photometric_confidence, each resized to the depth map's size
                                        with cv2.resize (INTER_LINEAR) -- the map filter_depth thresholds (runner.py:267-271)
    save_view(out_folder, view, ...)    the files later steps read: depth_est/ and confidence/ PFMs, cams/, images/
                                        (runner.py:261-295); previews=True: the four colour previews as well
    select_sorted_pairs(map, ranks)     exact order statistics of a float32 map (csrc/svs_preview.hip)
    quantile(map, q), percentile(map, p)   np.quantile / np.percentile (method linear) of a float32 map, from them
    depth_preview(maps, lo, hi, ...)    helpers.utils.visualize_depth per pixel, for the maps of a view that share bounds
    eval_mask(image, H, W, radius=12)   read_img's mask -> last channel -> binary_dilation(disk(12)) -> cv2.resize(.. * 1.,
                                        (W,H)) > 0. (runner.py:362-368), = resize_any(dilate_disk(image != 0), H, W)
    eval_mask_path(root, dataset, scan_name, view)      the file rule of runner.py:351-360

`fusion.filter_depth_folder(..., eval_mask_root=..., dataset=...)` applies the masks, which is the reference's default
configuration (eval_mask: true).  Every operator runs on the device; there is no CPU fallback (`SvsError` without the
library or a GPU).  The dilation and the thresholded resize are boolean functions of their input and bit-exact; the
float32 bilinear resize of the confidence maps is restated and UNPINNED against OpenCV (INTEGRATION.md gives the call to
check it against).  JPEG files are written by PIL at quality 95 (OpenCV's default): the decoded images are close to, not
byte-identical with, what cv2.imwrite stores.

    python -m svs_hip.mvsout --scan-folder S --out-folder O --ply P --views 25 22 28 [--data-dir-root D --dataset DTU]
"""
import argparse
import ctypes
import os

import numpy as np
import torch

from . import lib as _lib
from .images import linear_table, tables_device, to_device
from .ops import _ptr, _stream
from .scans import view_mask_file as eval_mask_path        # the file rule of runner.py:351-360, decided per file

MAX_RADIUS = 32
# entry-point calls made by this process (tests, bench_mvsout.py, bench_run.py)
LAUNCHES = {"dilate": 0, "resize": 0, "confidence": 0, "select": 0, "preview": 0}
KERNELS_PER_CALL = {"dilate": 3, "resize": 1, "confidence": 1, "select": 8, "preview": 1}
SELECT_MAX_RANKS = 4
BYTES_DOWN = {"select": 0, "maps": 0, "previews": 0}       # what save_view and the order statistics brought to the host


def _mask_dev(mask, what):
    """(Hs,Ws) or (V,Hs,Ws) array / tensor of any numeric type -> uint8 device tensor (V,Hs,Ws) of its codes (a bool or
    float input: 1 where non-zero), and whether a view axis was added"""
    t = mask if torch.is_tensor(mask) else np.asarray(mask)
    if "uint8" not in str(t.dtype):
        t = t != 0
    t = to_device(t, torch.uint8, "mvsout", what, ndim=(2, 3), expect="(Hs,Ws) or (V,Hs,Ws)", non_blocking=True)
    single = t.dim() == 2
    return (t[None] if single else t).contiguous(), single


def _tables(H, W, Hs, Ws, dev):
    return [None] * 4 if (Hs, Ws) == (H, W) else tables_device(linear_table, H, W, Hs, Ws, dev)


def dilate_disk(mask, radius=12):
    """skimage.morphology.binary_dilation(mask, disk(radius)) (runner.py:365).  mask: (Hs,Ws) or (V,Hs,Ws), set where
    non-zero -> uint8 device tensor of 0/1, same shape."""
    L = _lib.load()
    d, single = _mask_dev(mask, "mask")
    V, Hs, Ws = d.shape
    out = torch.empty_like(d)
    ws = torch.empty(max(int(L.svs_mask_dilate_workspace_bytes(V, Hs, Ws)), 8) // 8, dtype=torch.int64, device=d.device)
    _lib.check(L.svs_mask_dilate_disk(_ptr(d), V, Hs, Ws, int(radius), _ptr(ws), _ptr(out), _stream()), "svs_mask_dilate_disk")
    LAUNCHES["dilate"] += 1
    return out[0] if single else out


def resize_any(mask, H, W):
    """cv2.resize(mask * 1., (W,H)) > 0. of a 0/1 mask (runner.py:366-368).  mask: (Hs,Ws) or (V,Hs,Ws) -> uint8 device
    tensor of 0/1, (H,W) or (V,H,W)."""
    L = _lib.load()
    H, W = int(H), int(W)
    d, single = _mask_dev(mask, "mask")
    V, Hs, Ws = d.shape
    out = torch.empty(V, max(H, 0), max(W, 0), dtype=torch.uint8, device=d.device)
    tabs = _tables(H, W, Hs, Ws, d.device) if H >= 1 and W >= 1 else [None] * 4
    _lib.check(L.svs_mask_resize_any(_ptr(d), V, Hs, Ws, H, W, *[_ptr(t) for t in tabs], _ptr(out), _stream()),
               "svs_mask_resize_any")
    LAUNCHES["resize"] += 1
    return out[0] if single else out


def eval_mask(image, H, W, radius=12):
    """The evaluation mask of one view as filter_depth applies it (runner.py:362-368).  image: what read_img returns for
    the mask file, or its uint8 codes: (Hs,Ws) or (Hs,Ws,C) -- the last channel is taken.  -> uint8 device tensor (H,W)
    of 0/1, which `fusion.fuse_view(extra_mask=...)` / `fusion.filter_depth(eval_masks=...)` take as it is."""
    a = image if torch.is_tensor(image) else np.asarray(image)
    if a.ndim == 3:
        a = a[:, :, -1]
    if a.ndim != 2:
        raise ValueError(f"image: expected (Hs,Ws) or (Hs,Ws,C), got {tuple(a.shape)}")
    return resize_any(dilate_disk(a, radius), H, W)


def _map_dev(a, what):
    t = a if torch.is_tensor(a) else np.asarray(a)
    if t.ndim == 3:
        t = t[0]                                                  # batch entry 0, like the loop at runner.py:261-262
    return to_device(t, torch.float32, "mvsout", what, ndim=(2,), expect="(H,W) or (B,H,W)")


def confidence_product(conf1, conf2, conf3, H, W):
    """cv2.resize(conf1, (W,H)) * cv2.resize(conf2, (W,H)) * cv2.resize(conf3, (W,H)) (runner.py:267-271): float32 maps of
    any sizes -> float32 device tensor (H,W)."""
    L = _lib.load()
    H, W = int(H), int(W)
    maps = [_map_dev(c, f"conf{k + 1}") for k, c in enumerate((conf1, conf2, conf3))]
    dev = maps[0].device
    out = torch.empty(max(H, 0), max(W, 0), dtype=torch.float32, device=dev)
    args, keep = [], []
    for m in maps:
        tabs = _tables(H, W, m.shape[0], m.shape[1], dev) if H >= 1 and W >= 1 else [None] * 4
        keep.append(tabs)
        args += [_ptr(m), m.shape[0], m.shape[1]] + [_ptr(t) for t in tabs]
    _lib.check(L.svs_mvs_confidence(*args, H, W, _ptr(out), _stream()), "svs_mvs_confidence")
    LAUNCHES["confidence"] += 1
    return out


def final_confidence(outputs):
    """outputs: the dict CascadeMVSNet returns for one view (device tensors or arrays).  -> conf_final of runner.py:267-271,
    float32 device tensor of the depth map's size: outputs['stage1'] / ['stage2'] / the top-level
    'photometric_confidence', batch entry 0, resized to the top-level map's size and multiplied."""
    c3 = _map_dev(outputs["photometric_confidence"], "photometric_confidence")
    H, W = _map_dev(outputs["depth"], "depth").shape if "depth" in outputs else c3.shape
    return confidence_product(outputs["stage1"]["photometric_confidence"], outputs["stage2"]["photometric_confidence"], c3,
                              H, W)


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


# ---- order statistics and colour previews (csrc/svs_preview.hip) ---------------------------------------------------------
def select_sorted_pairs(values, ranks):
    """Exact order statistics of a float32 map on the device.  values: array or tensor of any shape (n elements); ranks: up
    to 4 zero-based ranks k in 0..n-1.  -> pairs float32 (len(ranks),2): the k-th and the min(k+1, n-1)-th smallest
    element, bit for bit what np.sort places there (but -0.0 orders before +0.0, which np.sort leaves open; NaNs last);
    counts: dict(nan, posinf, neginf).  One call, whatever the number of ranks; its 8 + 3 words are the only download."""
    L = _lib.load()
    t = values if torch.is_tensor(values) else np.asarray(values)
    d = to_device(t.reshape(-1), torch.float32, "mvsout", "values", cast=False)
    n = d.numel()
    ranks = [int(k) for k in ranks]
    if not 1 <= len(ranks) <= SELECT_MAX_RANKS:
        raise ValueError(f"ranks: 1..{SELECT_MAX_RANKS} ranks per call, got {len(ranks)}")
    if n < 1 or any(not 0 <= k < n for k in ranks):
        raise ValueError(f"ranks {ranks} outside 0..{n - 1}")
    ws = torch.empty((int(L.svs_select_workspace_bytes()) + 7) // 8, dtype=torch.int64, device=d.device)
    out = torch.empty(2 * SELECT_MAX_RANKS + 4, dtype=torch.int32, device=d.device)
    arr = (ctypes.c_longlong * len(ranks))(*ranks)
    _lib.check(L.svs_select_sorted_pairs(_ptr(d), n, arr, len(ranks), _ptr(ws), _ptr(out), _ptr(out[2 * SELECT_MAX_RANKS:]),
                                         _stream()), "svs_select_sorted_pairs")
    LAUNCHES["select"] += 1
    host = out.cpu().numpy()
    BYTES_DOWN["select"] += host.nbytes
    pairs = host[:2 * len(ranks)].view(np.float32).reshape(len(ranks), 2).copy()
    c = host[2 * SELECT_MAX_RANKS:].view(np.uint32)
    return pairs, dict(nan=int(c[0]), posinf=int(c[1]), neginf=int(c[2]))


def quantile_ranks(n, q):
    """numpy's `linear` rule for n float32 values (numpy 2: lib/_function_base_impl.py::_quantile, _get_indexes,
    _get_gamma), evaluated with numpy's own scalar arithmetic: a Python-number q is taken in the array's dtype, so the
    virtual index (n - 1) * q, its floor and the weight gamma are float32.  q: float32 scalars in [0,1].
    -> ranks (ints; n - 1 where the index reaches the end), gamma (float32 array)"""
    q = np.asarray(q, dtype=np.float32).reshape(-1)
    if not np.all((q >= 0) & (q <= 1)):
        raise ValueError("Quantiles must be in the range [0, 1]")
    virtual = np.asanyarray((n - 1) * q)
    previous = np.floor(virtual)
    above = virtual >= n - 1
    previous[above] = -1
    gamma = np.asanyarray(virtual - previous, dtype=virtual.dtype)
    ranks = previous.astype(np.intp)
    ranks[above] = n - 1
    return [int(k) for k in ranks], gamma


def lerp(a, b, t):
    """numpy's _lerp in the operands' float32: a + (b - a) t for t < 0.5, b - (b - a)(1 - t) otherwise"""
    a, b, t = (np.asarray(v, dtype=np.float32) for v in (a, b, t))
    with np.errstate(invalid="ignore"):
        diff = np.subtract(b, a)
        out = np.asanyarray(np.add(a, diff * t))
        np.subtract(b, diff * (1 - t), out=out, where=t >= 0.5)
    return out


def _quantiles(values, q, valid_only=False, select=None):
    """np.quantile(values, q) for float32 scalars q (a list of up to 4) -> float32 array.  valid_only: of the finite
    elements only, np.quantile(values[isfinite(values)], q): the ranks are asked for as if every element were finite and
    asked for again when the counts say otherwise (finite elements sit between the -inf and the +inf / NaN in the order)."""
    select = select or select_sorted_pairs
    n = int(values.numel() if torch.is_tensor(values) else np.asarray(values).size)
    ranks, gamma = quantile_ranks(n, q)
    pairs, counts = select(values, ranks)
    bad = counts["nan"] + counts["posinf"] + counts["neginf"]
    if valid_only and bad:
        m = n - bad
        if m < 1:
            raise ValueError("no finite value to take a percentile of")
        ranks, gamma = quantile_ranks(m, q)
        pairs, _ = select(values, [min(k + counts["neginf"], n - 1) for k in ranks])
        last = [k == m - 1 for k in ranks]
        pairs[last, 1] = pairs[last, 0]                  # (the element after the last finite one is not finite)
    elif counts["nan"]:
        return np.full(len(ranks), np.nan, np.float32)   # numpy: a slice with a NaN gives NaN
    return lerp(pairs[:, 0], pairs[:, 1], gamma)


def quantile(values, q, select=None):
    """np.quantile(values, q) (method linear) of a float32 map on the device, bit for bit (the sign of a zero result
    aside: see select_sorted_pairs).  q: a number, or up to 4 of them -> np.float32, or a float32 array.  A map with a
    NaN gives NaN, as numpy does."""
    out = _quantiles(values, np.asarray(q, dtype=np.float32), select=select)
    return out[0] if np.ndim(q) == 0 else out


def percentile(values, p, valid_only=False, select=None):
    """np.percentile(values, p): `quantile` at p / float32(100), numpy's division."""
    q = np.true_divide(p, np.float32(100))
    out = _quantiles(values, np.asarray(q, dtype=np.float32), valid_only=valid_only, select=select)
    return out[0] if np.ndim(p) == 0 else out


_JET = {}


def jet_table():
    """matplotlib's `jet` sampled at 256 entries as uint8 (256,3) RGB codes -- the stand-in for cv2.COLORMAP_JET, UNPINNED
    against it (INTEGRATION.md gives the cv2.applyColorMap call to check it with) -- or None, with one warning, when
    matplotlib does not import."""
    if "table" not in _JET:
        try:
            import matplotlib
            _JET["table"] = np.ascontiguousarray(matplotlib.colormaps["jet"](np.arange(256), bytes=True)[:, :3], dtype=np.uint8)
        except Exception as e:                          # noqa: BLE001  (no matplotlib, or one without the table)
            import warnings
            _JET["table"] = None
            warnings.warn(f"matplotlib's jet colour table is not available ({e}): the colour previews are not written")
    return _JET["table"]


def depth_preview(maps, lo, hi, direct=False, table=None):
    """helpers.utils.visualize_depth(map, depth_min=lo, depth_max=hi, direct=direct) (helpers/utils.py:197-224) of up to 3
    float32 maps that share the bounds, in one launch.  maps: (H,W) arrays or device tensors, each of its own size.
    direct=False: -> uint8 device tensors (H,W,3), row 255 - code of `table` (256,3) uint8 (default: `jet_table()`, RGB; the
    channel order of the result is the table's); direct=True: -> (H,W) grey codes.  Invalid pixels (NaN, infinite) are 0.
    hi <= lo, or a bound that is NaN: the reference divides by zero and casts NaN to uint8, which is platform-defined;
    here the image is all zeros."""
    L = _lib.load()
    maps = [_map_dev(m, f"maps[{k}]") for k, m in enumerate(maps)]
    if not 1 <= len(maps) <= 3:
        raise ValueError(f"maps: 1..3 maps per call, got {len(maps)}")
    dev = maps[0].device
    tab = None
    if not direct:
        if table is None:
            table = jet_table()
            if table is None:
                raise _lib.SvsError("no colour table: matplotlib is missing and none was passed")
        tab = to_device(table, torch.uint8, "mvsout", "table", ndim=(2,), expect="(256,3) uint8", cast=False)
        if tuple(tab.shape) != (256, 3):
            raise ValueError(f"table: expected (256,3), got {tuple(tab.shape)}")
    outs = [torch.empty(m.shape + (() if direct else (3,)), dtype=torch.uint8, device=dev) for m in maps]
    args = []
    for k in range(3):
        args += [_ptr(maps[k]), maps[k].numel(), _ptr(outs[k])] if k < len(maps) else [None, 0, None]
    if any(m.numel() < 1 for m in maps):
        raise ValueError("maps: an empty map")
    _lib.check(L.svs_depth_preview(*args, len(maps), float(lo), float(hi), int(bool(direct)), _ptr(tab), _stream()),
               "svs_depth_preview")
    LAUNCHES["preview"] += 1
    return outs


def save_view(out_folder, view, outputs, cam, img, cam_near_far=None, previews=False, dep_max=None, table=None):
    """The files of one view that later steps read (runner.py:261-295): depth_est/{view:08}.pfm (outputs['depth'], batch
    entry 0), confidence/{view:08}.pfm (`final_confidence`), cams/{view:08}_cam.txt (cam: (2,4,4) extrinsic, intrinsic),
    images/{view:08}.jpg (img: (3,H,W) float in [0,1]; clip(img * 255, 0, 255) as uint8, JPEG quality 95).
    previews=True: the four colour previews of runner.py:283-290 as well -- depth_est/{view:08}.png, _1.png, _2.png
    (outputs['depth'], ['stage1']['depth'], ['stage2']['depth'] between quantile(depth, 0.01) and dep_max, the sample's
    depth_values.max(), through `table`, default jet) and confidence/{view:08}_final.png (the grey codes of the
    confidence between the 5th and 95th percentile of its finite pixels).  PNGs are RGB through PIL; cv2.imwrite of the
    BGR map shows the same colours.  Without a table (no matplotlib) the three colour previews are skipped.  Depth,
    confidence and previews are formed on the device and only what a file holds is downloaded: two float32 maps and four
    uint8 images; `prob_volume` never is.
    -> dict of the file names."""
    from datasets.data_io import save_pfm
    from helpers.utils import write_cam
    from PIL import Image
    names = {k: os.path.join(out_folder, k, "{:0>8}{}".format(view, ext))
             for k, ext in (("depth_est", ".pfm"), ("confidence", ".pfm"), ("cams", "_cam.txt"), ("images", ".jpg"))}
    for f in names.values():
        os.makedirs(os.path.dirname(f), exist_ok=True)
    if not previews:
        depth = _host(outputs["depth"]).astype(np.float32, copy=False)
        save_pfm(names["depth_est"], depth[0] if depth.ndim == 3 else depth)
        save_pfm(names["confidence"], final_confidence(outputs).cpu().numpy())
    else:
        if dep_max is None:
            raise ValueError("previews=True needs dep_max, the sample's depth_values.max()")
        depth = _map_dev(outputs["depth"], "depth")
        conf = final_confidence(outputs)
        shots = {}
        if table is None:
            table = jet_table()
        if table is not None:
            lo = quantile(depth, 0.01)
            col = depth_preview([depth, outputs["stage1"]["depth"], outputs["stage2"]["depth"]], lo, np.float32(dep_max),
                                table=table)
            shots.update(zip(("depth_png", "depth_1_png", "depth_2_png"), col))
        c_lo, c_hi = percentile(conf, [5, 95], valid_only=True)
        shots["confidence_png"] = depth_preview([conf], c_lo, c_hi, direct=True)[0]
        for k, f in (("depth_est", depth), ("confidence", conf)):
            a = f.cpu().numpy()
            BYTES_DOWN["maps"] += a.nbytes
            save_pfm(names[k], a)
        for k, (sub, ext) in dict(depth_png=("depth_est", ".png"), depth_1_png=("depth_est", "_1.png"),
                                  depth_2_png=("depth_est", "_2.png"), confidence_png=("confidence", "_final.png")).items():
            if k in shots:
                names[k] = os.path.join(out_folder, sub, "{:0>8}{}".format(view, ext))
                a = shots[k].cpu().numpy()
                BYTES_DOWN["previews"] += a.nbytes
                Image.fromarray(a).save(names[k], compress_level=1)       # (cv2.imwrite's default PNG level)
    write_cam(names["cams"], _host(cam), cam_near_far)
    rgb = np.clip(np.transpose(_host(img), (1, 2, 0)) * 255, 0, 255).astype(np.uint8)
    Image.fromarray(rgb).save(names["images"], quality=95)
    return names


def folder_eval_masks(eval_mask_root, dataset, scan_name, views, shapes, radius=12):
    """{view: eval_mask of its file, resized to shapes[view]} -- what filter_depth_folder hands to filter_depth"""
    from helpers.utils import read_img
    return {v: eval_mask(read_img(eval_mask_path(eval_mask_root, dataset, scan_name, v)), *shapes[v], radius=radius)
            for v in views}


def main(argv=None):
    p = argparse.ArgumentParser(description="The reference's filter_only run for one scan: fuses the depth maps of a scan "
                                            "folder into a PLY, with the evaluation masks when --data-dir-root is given.")
    p.add_argument("--scan-folder", required=True, help="holds cams/{view:08}_cam.txt and images/{view:08}.jpg")
    p.add_argument("--out-folder", required=True, help="holds depth_est/ and confidence/ PFMs; its last component names the scan")
    p.add_argument("--ply", required=True)
    p.add_argument("--views", type=int, nargs="+", required=True)
    p.add_argument("--data-dir-root", help="holds <dataset>/eval_mask/<scan>/...: apply the evaluation masks (eval_mask: true)")
    p.add_argument("--dataset", choices=("DTU", "BlendedMVS"), help="with --data-dir-root")
    p.add_argument("--conf", type=float, default=0.0)
    p.add_argument("--filter-dist", type=float, default=1)
    p.add_argument("--filter-diff", type=float, default=0.01)
    p.add_argument("--thres-view", type=int, default=1)
    p.add_argument("--eval-mask-radius", type=int, default=12)
    a = p.parse_args(argv)
    if a.data_dir_root and not a.dataset:
        p.error("--data-dir-root needs --dataset")
    from . import fusion
    xyz, _, stats = fusion.filter_depth_folder(a.scan_folder, a.out_folder, a.ply, a.views, conf=a.conf,
                                               filter_dist=a.filter_dist, filter_diff=a.filter_diff, thres_view=a.thres_view,
                                               eval_mask_root=a.data_dir_root, dataset=a.dataset,
                                               eval_mask_radius=a.eval_mask_radius)
    for v, photo, geo, final in stats:
        print("processing {}, ref-view{:0>2}, photo/geo/final-mask:{:.3f}/{:.3f}/{:.3f}".format(a.scan_folder, v, photo, geo, final))
    print(f"saving the final MVS result to {a.ply}: {len(xyz)} points")


if __name__ == "__main__":
    main()
