"""Numpy restatements of the image work of the reference's MVSDataset (datasets/general_eval.py:157-176, 220-232, 254,
267-268) and of create_scene's PNG codes (runner.py:106) -- what csrc/svs_mvsdata.hip and svs_hip/mvsdata.py are tested
against -- and the synthetic scan folders the tests and tests/golden/make_mvsdata_fixture.py run on.

The resize is tests/scene_oracle.py::resize_cubic (cv2.resize INTER_CUBIC, UNPINNED: no OpenCV here).  Two precisions:

    float32 flow   what the reference computes with cv2.resize bound to the oracle: every pass's result rounded to float32
                   (cv2.resize of a float32 image returns float32), the alpha product in float32.  `prepare_views` -- the
                   stand-in for svs_hip.mvsdata.prepare_views in the CPU tests.
    float64 chain  no rounding between the passes or before the product: what the GPU results are bounded against.
"""
import os

import numpy as np

import scene_oracle as so


def code_values(codes):
    """helpers/utils.py:27 read_img: np.array(img, dtype=np.float32) / 255."""
    return np.array(codes, dtype=np.float32) / 255.


def resize_chain(img, sizes, dtype=np.float64):
    """img (Hs,Ws,C) -> (H,W,C) after cv2.resize(..., INTER_CUBIC) to every size in turn; a resize to the same size
    copies.  dtype float32: each pass rounded, as cv2 returns it."""
    img = np.asarray(img, dtype)
    for hw in sizes:
        if img.shape[:2] != tuple(hw):
            img = so.resize_cubic(img, tuple(hw)).astype(dtype)
    return img


def pack(img):
    """(H,W,C) -> imgs (3,H,W), masks (1,H,W) (general_eval.py:254, 267-268) in img's dtype"""
    planes = img.transpose(2, 0, 1)
    if planes.shape[0] == 4:
        return planes[:3] * planes[3:], planes[3:].copy()
    return planes.copy(), np.ones_like(planes[:1])


def views64(codes, sizes):
    """the float64 chain of V views: codes (V,Hs,Ws,C) uint8 -> imgs (V,3,H,W), masks (V,1,H,W), and the resized
    channel-last image (V,H,W,C), float64"""
    out = [resize_chain(code_values(c), sizes) for c in codes]
    packed = [pack(o) for o in out]
    return np.stack([p[0] for p in packed]), np.stack([p[1] for p in packed]), np.stack(out)


def png_codes(img):
    """runner.py:106 for planes (3,H,W) float32 -> (H,W,3) uint8"""
    assert img.dtype == np.float32
    return np.clip(np.transpose(img, (1, 2, 0)) * 255, 0, 255).astype(np.uint8)


def prepare_views(codes, sizes, png=False):
    """The float32 flow with the signature of svs_hip.mvsdata.prepare_views; CPU tensors."""
    import torch
    imgs, masks = [], []
    for c in np.asarray(codes):
        i, m = pack(resize_chain(code_values(c), sizes, np.float32))
        imgs.append(i)
        masks.append(m)
    out = (torch.from_numpy(np.stack(imgs)), torch.from_numpy(np.stack(masks)))
    return out + (torch.from_numpy(np.stack([png_codes(i) for i in imgs])),) if png else out


def decompose_projection_matrix(P):
    """cv2.decomposeProjectionMatrix(P)[:3] from scene_oracle.load_K_Rt_from_P: K, R and the homogeneous camera centre
    (4,1), in float64"""
    K, pose = so.load_K_Rt_from_P(np.asarray(P, np.float64))
    c = -np.linalg.solve(np.asarray(P, np.float64)[:, :3], np.asarray(P, np.float64)[:, 3])
    return K[:3, :3], pose[:3, :3].astype(np.float64).T, np.concatenate([c, [1.0]])[:, None]


def all_codes(H, W, C, seed):
    """uint8 (H,W,C) that holds every code in every channel"""
    rng = np.random.default_rng(seed)
    assert H * W >= 512
    return np.stack([rng.permutation(np.resize(np.arange(256, dtype=np.uint8), H * W)).reshape(H, W) for _ in range(C)], -1)


# ---- synthetic scan folders --------------------------------------------------------------------------------------------
def rgba_image(H, W, seed):
    """uint8 (H,W,4): scene_oracle's image with a soft-edged, partly transparent alpha channel"""
    rng = np.random.default_rng(seed + 7)
    alpha = np.roll(so.synthetic_mask(H, W), seed % 5, axis=1).astype(np.float64) * 255
    alpha[1:-1, 1:-1] = (alpha[1:-1, 1:-1] * 2 + alpha[:-2, 1:-1] + alpha[2:, 1:-1] + alpha[1:-1, :-2] + alpha[1:-1, 2:]) / 6.0
    alpha = alpha * rng.uniform(0.6, 1.0, (H, W))
    return np.concatenate([so.synthetic_image(H, W, seed), np.rint(alpha).astype(np.uint8)[..., None]], -1)


def pair_text(pairs):
    """{ref: [src, ...]} -> the text of a pair.txt (ids with made-up scores)"""
    lines = [str(len(pairs))]
    for ref, srcs in pairs.items():
        lines += [str(ref), " ".join([str(len(srcs))] + [f"{s} {100.0 - k:.1f}" for k, s in enumerate(srcs)])]
    return "\n".join(lines) + "\n"


def write_mvs_scan(root, dataset, scan, n_images, size, pairs, folder=None, rgba=False, seed=0, own_cameras=True,
                   own_pairs=True, depth_line=lambda v: f"{300.0 + 7 * v} 2.5 128 {900.0 + 11 * v}"):
    """so.write_scan's folder plus what MVSDataset reads below {root}/{dataset}/mvs_data: DTU {scan}/pair.txt (scan1's when
    own_pairs is False); BlendedMVS {folder}/cams/pair.txt and {folder}/cams/{v:08d}_cam.txt with `depth_line(v)` as the
    depth range.  rgba: the images are rewritten as RGBA.  -> mvs_data's path"""
    from PIL import Image
    inst = so.write_scan(root, dataset, scan, n_images, size, seed=seed, own_cameras=own_cameras)
    if rgba:
        for i in range(n_images):
            name = f"{i:06d}.png" if dataset == "DTU" else f"{i:08d}.png"
            Image.fromarray(rgba_image(size[0], size[1], seed * 1000 + i), "RGBA").save(os.path.join(inst, "image", name))
    mvs = os.path.join(root, dataset, "mvs_data")
    if dataset == "DTU":
        d = os.path.join(mvs, f"scan{scan}" if own_pairs else "scan1")
        os.makedirs(d, exist_ok=True)
        open(os.path.join(d, "pair.txt"), "w").write(pair_text(pairs))
    else:
        d = os.path.join(mvs, folder, "cams")
        os.makedirs(d, exist_ok=True)
        open(os.path.join(d, "pair.txt"), "w").write(pair_text(pairs))
        for v in range(n_images):
            with open(os.path.join(d, f"{v:08d}_cam.txt"), "w") as f:
                f.write("extrinsic\n" + "1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n" + "\nintrinsic\n"
                        + "800 0 80\n0 800 60\n0 0 1\n" + "\n" + depth_line(v) + "\n")
    return mvs


class Args(dict):
    """stands for the hydra object: attribute access and .get"""
    __getattr__ = dict.__getitem__


# The folders of tests/golden/mvsdata_ref.npz: name -> (write_mvs_scan arguments, MVSDataset arguments)
PAIRS = {0: [1, 2, 3, 4, 5], 1: [0, 2, 5, 4, 3], 2: [4, 1, 0, 3, 5], 3: [2, 4, 0], 4: [2, 3, 1, 5, 0], 5: [1, 0, 4]}
CASES = {
    # 120x160 -> 64x64: the height sets the scale, 85.33 columns round down to 64.  scan114's cameras, scan1's pairs.
    "dtu": dict(scan=dict(dataset="DTU", scan=24, n_images=6, size=(120, 160), pairs=PAIRS, seed=3, own_cameras=False,
                          own_pairs=False),
                ds=dict(nviews=3, ndepths=48, interval_scale=1.06, max_h=64, max_w=96, trains_i=[4, 1, 2]), x2=False),
    # RGBA, 100x160 -> 32x96: the width-limited branch; scan5: the depth range is divided by scale_mat's and capped
    "bmvs": dict(scan=dict(dataset="BlendedMVS", scan=5, n_images=6, size=(100, 160), pairs=PAIRS, seed=5, rgba=True),
                 ds=dict(nviews=3, ndepths=32, interval_scale=1.0, max_h=64, max_w=96, trains_i=[2, 5, 0]), x2=False),
    # x2_mvsres at the real sizes (metadata and sizes only), four training views: cut to five does not bite, order does
    "x2": dict(scan=dict(dataset="DTU", scan=106, n_images=4, size=(1200, 1600), pairs={k: [s for s in v if s < 4] for k, v
                                                                                         in PAIRS.items() if k < 4}, seed=9),
               ds=dict(nviews=3, ndepths=192, interval_scale=1.06, max_h=576, max_w=768, trains_i=[3, 0, 2, 1]), x2=True),
}


def build_case(name, root, cls, folder=None):
    """writes the folder of CASES[name] under `root` and constructs `cls` (an MVSDataset class) on it"""
    case = CASES[name]
    kw = dict(case["scan"])
    if kw["dataset"] == "BlendedMVS":
        kw["folder"] = folder
    mvs = write_mvs_scan(root, **kw)
    d = dict(case["ds"])
    return cls(mvs, [f"scan{kw['scan']}"], "test", d.pop("nviews"), kw["dataset"], d.pop("ndepths"), d.pop("interval_scale"),
               args=Args(data_dir_root=root, x2_mvsres=case["x2"]), **d)


def flatten(ds, images=True):
    """every array of every sample of `ds` as {key: array} (the layout of the fixture): sample{i}/<key>, the images once per
    view id as view{id}/imgs|masks after checking that every sample holds exactly those"""
    out, views = {"n_samples": np.asarray(len(ds))}, {}
    for i in range(len(ds)):
        s = ds[i] if images else ds.sample_meta(i)
        for st, p in s["proj_matrices"].items():
            out[f"sample{i}/proj_matrices/{st}"] = p
        out[f"sample{i}/depth_values"] = s["depth_values"]
        out[f"sample{i}/cam_near_far"] = s["cam_near_far"]
        out[f"sample{i}/filename"] = np.asarray(s["filename"])
        if images:
            ids = view_order(ds, i)
            out[f"sample{i}/view_ids"] = np.asarray(ids)
            assert s["imgs"].shape[0] == s["masks"].shape[0] == len(ids)
            for k, v in enumerate(ids):
                got = (np.asarray(s["imgs"][k]), np.asarray(s["masks"][k]))
                if v in views:
                    assert np.array_equal(views[v][0], got[0]) and np.array_equal(views[v][1], got[1])
                views[v] = got
    for v, (img, mask) in views.items():
        out[f"view{v}/imgs"], out[f"view{v}/masks"] = img, mask
    return out


def view_order(ds, idx):
    """general_eval.py:181-191 from the attributes both classes have"""
    _, ref_view, src_views, _ = ds.metas[idx]
    ids = [ref_view] + [x for x in src_views if x in ds.trains_i]
    ids += [x for x in ds.trains_i if x not in ids]
    return ids[:ds.nviews_max]
