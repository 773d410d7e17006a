"""Builds tests/golden/nvs_scores.npz: the reference's novel-view scoring (eval_vsdf.py:186-212, --result_from blend and
default) run on a synthetic data_s_volsdf tree.

    python tests/golden/make_nvs_fixture.py          (needs the reference checkout, see ref_shim.REFERENCE_ROOT)

eval_vsdf.py cannot be imported (TensorFlow, lpips_tf, GPUtil and scikit-image at module level), so the statement of
evaluate() that holds the scoring branch -- `if opt.eval_rendering:` with the view selection, the dataloader loop and the
per-scan print (eval_vsdf.py:157-283) -- is taken from the file with `ast`, wrapped unmodified in a function and executed
with: the reference's own SceneDataset, DataLoader and id tables (get_eval_ids / get_trains_ids), numpy / torch / PIL,
`structural_similarity` bound to tests/nvs_oracle.py's restatement, and the TensorFlow session and lpips_tf stubbed (their
LPIPS values are not stored).  SceneDataset runs through ref_shim's stubs with imageio.imread bound to a PIL reader,
skimage.img_as_float32 to nvs_oracle.img_as_float32, cv2.GaussianBlur to a pass-through (rgb_smooth is unused here),
cv2.decomposeProjectionMatrix to an identity camera (poses are unused here) and cv2.resize to a pass-through that asserts
the size already matches (only the BlendedMVS mask path calls it, always with the same size).

Cases: DTU scan 106 (masks under eval_mask/scan106/mask/), DTU scan 24 (masks directly under eval_mask/scan24/), DTU
scan 4 (one of the scans the reference scores unmasked) and BlendedMVS scan 7 (RGBA masks): every image file of each scan
(49 / 31), the masks, and eval_blend / eval PNGs that differ from the ground truth by noise with a share of exact pixels.

Stored: every input file (`file/<path>`), per case the reference's ground truth and mask arrays of the scored views
(float32, (V,H,W,3)), the scored view ids in loop order, and per result_from the reference's psnrs / ssims and the SCAN
lines it printed (without the LPIPS line).  This pins file naming, sorting, the mask rules, the view exclusion, the
compositing and the float32 PSNR; the SSIM values are pinned only to nvs_oracle's restatement.
"""
import ast
import contextlib
import gc
import io
import os
import shutil
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import ref_shim  # noqa: E402

SEED = 17
# case -> (dataset, scan, (H, W), number of images, DTU mask layout)
CASES = {
    "dtu106": ("DTU", 106, (24, 32), 49, "mask"),
    "dtu24": ("DTU", 24, (16, 20), 49, "flat"),
    "dtu4": ("DTU", 4, (12, 16), 49, "mask"),
    "bmvs7": ("BlendedMVS", 7, (16, 24), 31, None),
}
RESULT_FROM = ("blend", "default")


def gt_image(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 40 + 150 * (yy / H) + 50 * np.sin(xx / 3.0)
    img = base[..., None] + rng.normal(0, 20, (H, W, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def rendered(rng, gt, sigma):
    noise = np.rint(rng.normal(0, sigma, gt.shape)).astype(int)
    noise[rng.random(gt.shape[:2]) < 0.3] = 0                                  # exact pixels
    return np.clip(gt.astype(int) + noise, 0, 255).astype(np.uint8)


def dtu_mask_png(rng, H, W):
    """RGB: 255 inside a disc, 0 outside, some 254 (not == 1 after / 255) and per-channel differences"""
    yy, xx = np.mgrid[0:H, 0:W]
    inside = (yy - H / 2) ** 2 + (xx - W / 2) ** 2 < (0.4 * min(H, W)) ** 2
    m = np.where(inside[..., None], 255, 0).repeat(3, -1).astype(np.uint8)
    m[rng.random((H, W, 3)) < 0.05] = 254
    m[rng.random((H, W, 3)) < 0.05] = 255
    return m


def bmvs_mask_png(rng, H, W):
    """RGBA: alpha spread around the 0.5 threshold (127 / 128) plus 0 / 255"""
    rgba = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    rgba[..., 3] = rng.choice(np.array([0, 127, 128, 255, 200, 60], np.uint8), (H, W))
    return rgba


def main():
    ref_shim.install()
    import torch
    from PIL import Image
    import nvs_oracle
    import cv2
    import imageio
    import skimage

    def resize_same(img, dsize, *a, **k):
        assert tuple(dsize) == (img.shape[1], img.shape[0]), "the fixture keeps every image at img_res"
        return np.array(img, copy=True)

    imageio.imread = lambda path: np.array(Image.open(path))
    skimage.img_as_float32 = nvs_oracle.img_as_float32
    cv2.GaussianBlur = lambda img, ksize, sigma: img
    cv2.resize = resize_same
    cv2.decomposeProjectionMatrix = lambda P: (np.eye(3), np.eye(3), np.array([[0.0], [0.0], [0.0], [1.0]]))
    cv2.INTER_CUBIC, cv2.INTER_NEAREST = 2, 0
    import volsdf.utils.general as utils
    from volsdf.datasets import scene_dataset as sd

    src = open(os.path.join(ref_shim.REFERENCE_ROOT, "eval_vsdf.py")).read()
    evaluate = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "evaluate"][0]
    blocks = [n for n in evaluate.body if isinstance(n, ast.If) and ast.unparse(n.test) == "opt.eval_rendering"
              and "psnrs" in ast.unparse(n)]
    assert len(blocks) == 1
    fn = ast.parse("def scoring_branch(model):\n    pass\n").body[0]
    fn.body = blocks
    code = compile(ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[])), "eval_vsdf.py", "exec")

    class _Session:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def run(self, *a, **k):
            return np.zeros(1)

    tf = SimpleNamespace(float32=None, placeholder=lambda *a, **k: None, Session=_Session)
    lpips_tf = SimpleNamespace(lpips=lambda *a, **k: None)

    rng = np.random.default_rng(SEED)
    root = tempfile.mkdtemp(prefix="svs_nvs_")
    arr = dict(seed=np.asarray(SEED), cases=np.asarray(list(CASES)), result_from=np.asarray(RESULT_FROM))
    files = []
    try:
        for case, (dataset, scan, (H, W), n_img, layout) in CASES.items():
            inst = os.path.join(root, "data", dataset, f"scan{scan}")
            os.makedirs(os.path.join(inst, "image"))
            mats = {}
            for i in range(n_img):
                fn = os.path.join(inst, "image", f"{i:06d}.png")
                Image.fromarray(gt_image(rng, H, W)).save(fn)
                files.append(fn)
                mats[f"scale_mat_{i}"] = np.eye(4)
                mats[f"world_mat_{i}"] = np.eye(4)
            np.savez(os.path.join(inst, "cameras.npz"), **mats)
            files.append(os.path.join(inst, "cameras.npz"))
            if dataset == "DTU":
                ids = sd.get_eval_ids("DTU")
                mdir = os.path.join(root, "data", "DTU", "eval_mask", f"scan{scan}")
                mdir = os.path.join(mdir, "mask") if layout == "mask" else mdir
                if scan not in (1, 4, 11, 13, 48):
                    os.makedirs(mdir)
                    # 000.png (a training view) decides the layout: written in the mask/ layout only
                    for i in ([0] if layout == "mask" else []) + ids:
                        fn = os.path.join(mdir, f"{i:03d}.png")
                        Image.fromarray(dtu_mask_png(rng, H, W)).save(fn)
                        files.append(fn)
            else:
                ids = sd.get_eval_ids("BlendedMVS", scan) + sd.get_trains_ids("BlendedMVS", f"scan{scan}", num_views=3)
                mdir = os.path.join(root, "data", "BlendedMVS", "eval_mask", f"scan{scan}", "mask")
                os.makedirs(mdir)
                for i in ids:
                    fn = os.path.join(mdir, f"{i:08d}.png")
                    Image.fromarray(bmvs_mask_png(rng, H, W), "RGBA").save(fn)
                    files.append(fn)
            ds = sd.SceneDataset(data_dir=dataset, img_res=[H, W], scan_id=scan, num_views=-1,
                                 data_dir_root=os.path.join(root, "data"))
            evaldir = os.path.join(root, "render", case)
            images_dir = os.path.join(evaldir, "rendering_0")
            os.makedirs(images_dir)
            for i in range(n_img):
                gt = (ds.rgb_images[i].numpy().reshape(H, W, 3) * 255).round().astype(np.uint8)
                for rf, sigma in (("blend", 5.0), ("default", 9.0)):
                    name = f"eval_blend_{i:03d}.png" if rf == "blend" else f"eval_{i:03d}.png"
                    Image.fromarray(rendered(rng, gt, sigma)).save(os.path.join(images_dir, name))
            for rf in RESULT_FROM:
                opened = []

                class _Image:
                    @staticmethod
                    def open(path):
                        opened.append(path)
                        return Image.open(path)

                loader = torch.utils.data.DataLoader(ds, batch_size=1, num_workers=0, shuffle=False, collate_fn=ds.collate_fn)
                ns = dict(np=np, torch=torch, os=os, gc=gc, Image=_Image, utils=utils, logger=ref_shim._NoLog(),
                          opt=SimpleNamespace(conf="./config/confs/{}.conf".format("dtu" if dataset == "DTU" else "bmvs"),
                                              result_from=rf, eval_rendering=True),
                          evaldir=evaldir, epoch=0, scan_id=scan, eval_dataloader=loader, img_res=[H, W],
                          total_pixels=H * W, get_eval_ids=sd.get_eval_ids, get_trains_ids=sd.get_trains_ids,
                          structural_similarity=nvs_oracle.structural_similarity, tf=tf, lpips_tf=lpips_tf,
                          plt=None, save_pfm=None, tqdm=None)
                exec(code, ns)
                out = io.StringIO()
                with contextlib.redirect_stdout(out):
                    psnrs, ssims, _ = ns["scoring_branch"](model=None)
                views = [int(os.path.basename(p).split("_")[-1][:3]) for p in opened]
                arr[f"{case}/{rf}/psnr"] = np.asarray(psnrs, np.float64).ravel()
                arr[f"{case}/{rf}/ssim"] = np.asarray(ssims, np.float64).ravel()
                arr[f"{case}/{rf}/lines"] = np.asarray([ln for ln in out.getvalue().splitlines() if "lpips" not in ln])
                if rf == "blend":
                    arr[f"{case}/views"] = np.asarray(views)
                    arr[f"{case}/gt"] = np.stack([ds.rgb_images[v].numpy().reshape(H, W, 3) for v in views])
                    arr[f"{case}/mask"] = np.stack([ds.masks[v].numpy().reshape(H, W, 3) for v in views])
                else:
                    assert views == list(arr[f"{case}/views"])
                for v in views:
                    name = f"eval_blend_{v:03d}.png" if rf == "blend" else f"eval_{v:03d}.png"
                    files.append(os.path.join(images_dir, name))
                print(f"  {case} {rf}: {len(views)} views, psnr {arr[f'{case}/{rf}/psnr'].mean():.3f}, "
                      f"ssim {arr[f'{case}/{rf}/ssim'].mean():.4f}")
            arr[f"{case}/dataset"] = np.asarray(dataset)
            arr[f"{case}/scan"] = np.asarray(scan)
            arr[f"{case}/img_res"] = np.asarray([H, W])
            arr[f"{case}/rendering_dir"] = np.asarray(os.path.relpath(images_dir, root))
        for fn in files:
            arr["file/" + os.path.relpath(fn, root)] = np.frombuffer(open(fn, "rb").read(), np.uint8)
        path = os.path.join(HERE, "nvs_scores.npz")
        np.savez_compressed(path, **arr)
        print(f"  wrote nvs_scores.npz ({os.path.getsize(path) / 1024:.1f} KiB)")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
