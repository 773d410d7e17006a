"""Builds tests/golden/ibr_blend.npz: the reference's image-based rendering of evaluation views (simple_ibr.py:116-235)
run end to end on a synthetic scan folder.

    python tests/golden/make_ibr_fixture.py          (needs the reference checkout, see ref_shim.REFERENCE_ROOT)

simple_ibr.py cannot be imported (hydra's get_config() runs at import), so image_based_render, Laplacian_Blending,
get_lpIMG, get_dir_loc, get_camera_params and lift are taken from the file with `ast`, compiled and executed -- unmodified --
in a namespace that binds the names they use: the reference's own helpers (read_camera_parameters, read_img, read_pfm,
check_geometric_consistency), numpy / torch / PIL / copy / os / Path, real scipy.special.softmax, fixed view-id lists for
get_trains_ids / get_eval_ids, and `cv2` bound to tests/ibr_oracle.py's restatements (the image lacks OpenCV):
cv2.remap dispatches on `interpolation`, INTER_LINEAR to fusion_oracle.remap_linear (check_geometric_consistency) and
INTER_CUBIC to ibr_oracle.remap_cubic.  Laplacian_Blending and check_geometric_consistency are wrapped to capture what
they receive and return.

Stored: the input files exactly as the function reads them (cams/*.txt, images/*.png, eval_*.png, depth_est/*.pfm), the
per-source geometric masks, the PNG pixels written, and for the arrays handed to Laplacian_Blending (fill images, masks)
and its float64 result a sha256 of their bytes plus every 8th row of the result.  The full arrays (2 x 1.8 MB per view at
96x128) would not fit the 1 MiB limit of a committed file; ibr_oracle reproduces them bit for bit from the stored inputs
(tests/test_ibr_cpu.py), and the GPU tests take them from there.
"""
import ast
import copy
import hashlib
import io
import os
import shutil
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import ref_shim  # noqa: E402
import synth     # noqa: E402

SEED, HW, SRC_IDS, EVAL_IDS = 41, (96, 128), [25, 22, 28], [23, 27]
SRC_OF_VIEW = {0: 25, 1: 23, 2: 22, 3: 27, 4: 28}          # synth view -> id: the eval views sit between the sources
ROW_STEP = 8


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def main():
    ref_shim.install()
    import torch
    import torch.nn.functional as F
    from PIL import Image
    from scipy.special import softmax
    import ibr_oracle
    import cv2
    for k, v in vars(ibr_oracle.cv2).items():
        setattr(cv2, k, v)
    import helpers.utils as hu
    from datasets.data_io import read_pfm, save_pfm

    src = open(os.path.join(ref_shim.REFERENCE_ROOT, "simple_ibr.py")).read()
    names = ("lift", "get_camera_params", "get_dir_loc", "get_lpIMG", "Laplacian_Blending", "image_based_render")
    fns = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in fns) == sorted(names)
    args = SimpleNamespace(vol=SimpleNamespace(dataset=SimpleNamespace(data_dir="DTU")), num_view=3)
    captured = {"geo": [], "lap": []}

    def geo_capture(*a, **k):
        out = hu.check_geometric_consistency(*a, **k)
        captured["geo"].append(out[0].copy())
        return out

    ns = dict(np=np, os=os, Path=Path, torch=torch, F=F, copy=copy, cv2=cv2, softmax=softmax, Image=Image, args=args,
              logger=ref_shim._NoLog(), get_trains_ids=lambda data_dir, scan, n: list(SRC_IDS)[:n],
              get_eval_ids=lambda data_dir, scan_id: list(EVAL_IDS), read_pfm=read_pfm,
              read_camera_parameters=hu.read_camera_parameters, read_img=hu.read_img,
              check_geometric_consistency=geo_capture)
    exec(compile(ast.Module(body=fns, type_ignores=[]), "simple_ibr.py", "exec"), ns)
    lap = ns["Laplacian_Blending"]

    def lap_capture(imgs, masks, num_levels=4):
        out = lap(imgs, masks, num_levels=num_levels)
        captured["lap"].append((imgs.copy(), masks.copy(), out.copy()))
        return out
    ns["Laplacian_Blending"] = lap_capture

    views = synth.make_fusion_views(SEED, hw=HW, n_views=5)
    root = tempfile.mkdtemp(prefix="svs_ibr_")
    arr = dict(seed=np.asarray(SEED), hw=np.asarray(HW), src_ids=np.asarray(SRC_IDS), eval_ids=np.asarray(EVAL_IDS),
               row_step=np.asarray(ROW_STEP))
    try:
        scan, out = os.path.join(root, "scan24"), os.path.join(root, "out")
        for d in (os.path.join(scan, "cams"), os.path.join(scan, "images"), os.path.join(out, "depth_est")):
            os.makedirs(d)
        files = {}
        for v, vid in SRC_OF_VIEW.items():
            view = views[v]
            K4 = np.eye(4, dtype=np.float32)
            K4[:3, :3] = view["K"]
            files["cams/{:0>8}_cam.txt".format(vid)] = os.path.join(scan, "cams/{:0>8}_cam.txt".format(vid))
            hu.write_cam(files["cams/{:0>8}_cam.txt".format(vid)], [view["E"], K4], cam_near_far=(1.0, 0.01, 192, 3.0))
            png = Image.fromarray(np.rint(view["img"] * 255).astype(np.uint8))
            key = "images/{:0>8}.png".format(vid) if vid in SRC_IDS else "eval_{:0>3}.png".format(vid)
            files[key] = os.path.join(scan if vid in SRC_IDS else out, key)
            png.save(files[key])
            files["depth_est/{:0>8}.pfm".format(vid)] = os.path.join(out, "depth_est/{:0>8}.pfm".format(vid))
            save_pfm(files["depth_est/{:0>8}.pfm".format(vid)], view["depth"])
        for key, fn in files.items():
            arr["file/" + key] = np.frombuffer(open(fn, "rb").read(), np.uint8)
        ns["image_based_render"](scan, out)
        assert len(captured["lap"]) == len(EVAL_IDS) and len(captured["geo"]) == len(EVAL_IDS) * len(SRC_IDS)
        for n, vid in enumerate(EVAL_IDS):
            imgs, masks, blend = captured["lap"][n]
            assert imgs.dtype == np.float32 and masks.dtype == np.float32 and blend.dtype == np.float64
            assert np.array_equal(masks, np.repeat(masks[..., :1], 3, -1))
            geo = np.stack(captured["geo"][n * len(SRC_IDS):(n + 1) * len(SRC_IDS)])
            arr[f"geo_{vid}"] = geo
            arr[f"sha_fill_{vid}"] = np.asarray(digest(imgs))
            arr[f"sha_masks_{vid}"] = np.asarray(digest(masks))
            arr[f"sha_blend_{vid}"] = np.asarray(digest(blend))
            arr[f"blend_rows_{vid}"] = blend[::ROW_STEP]
            arr[f"png_{vid}"] = np.array(Image.open(os.path.join(out, "eval_blend_{:0>3}.png".format(vid))))
            print(f"  view {vid}: geo mean {geo.mean():.3f}, masks > 0 {(masks[:-1] > 0).mean():.3f}, "
                  f"blend [{blend.min():.3f}, {blend.max():.3f}]")
        path = os.path.join(HERE, "ibr_blend.npz")
        np.savez_compressed(path, **arr)
        print(f"  wrote ibr_blend.npz ({os.path.getsize(path) / 1024:.1f} KiB)")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
