"""The scene loader without a GPU: the oracle (tests/scene_oracle.py) against independent implementations (torch's float64
interpolate, scipy's correlate1d and rq), the host-side tables and camera decomposition of svs_hip/scene.py against the
oracle, the dataset surface on synthetic scan folders with the image work bound to the oracle, and the argument checks of
the C entry points (nothing is launched)."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import scene_oracle as so

IDENTITY_TOL = 1e-12            # float64 against float64
REFERENCE = os.environ.get("SVOLSDF_REFERENCE_ROOT", "/root/reference")
SIZES = [((50, 66), (24, 32)), ((24, 32), (57, 70)), ((150, 200), (72, 96))]


@pytest.fixture()
def scene():
    from svs_hip import scene as sc
    saved = dict(sc._BMVS)
    sc.cache_clear()
    yield sc
    sc._BMVS.clear()
    sc._BMVS.update(saved)
    sc.cache_clear()


# ---- the oracle against independent implementations ----
@pytest.mark.parametrize("src,dst", SIZES)
def test_oracle_resizes_are_torch_float64_interpolate(src, dst):
    img = np.random.default_rng(src[0]).random(src + (3,))
    t = torch.from_numpy(img).permute(2, 0, 1)[None]
    for mode, fn in (("bicubic", so.resize_cubic), ("bilinear", so.resize_linear)):
        want = torch.nn.functional.interpolate(t, size=dst, mode=mode, align_corners=False)[0].permute(1, 2, 0).numpy()
        err = float(np.abs(fn(img, dst, coord="f64") - want).max())
        print(f"{mode} {src}->{dst}: max |oracle - torch| {err:.3g}")
        assert err <= IDENTITY_TOL
    # the float32 coordinate of the parity definition moves the result by what the issue measured (1e-5 .. 1e-4 scale)
    d = float(np.abs(so.resize_cubic(img, dst) - so.resize_cubic(img, dst, coord="f64")).max())
    assert d < 1e-3


def test_oracle_smoothing_is_two_mirrored_correlations():
    from scipy.ndimage import correlate1d
    img = np.random.default_rng(2).random((40, 53, 3))
    k = so.gaussian_kernel()
    assert k.dtype == np.float32 and k.shape == (31,) and abs(float(k.min()) - 0.03197) < 1e-5 \
        and abs(float(k.max()) - 0.03242) < 1e-5
    rows = correlate1d(img, k.astype(np.float64), axis=1, mode="mirror").astype(np.float32).astype(np.float64)
    want = correlate1d(rows, k.astype(np.float64), axis=0, mode="mirror")
    err = float(np.abs(so.gaussian_smooth(img) - want).max())
    print(f"smoothing: max |oracle - scipy| {err:.3g}")
    assert err <= IDENTITY_TOL


def test_oracle_mask_check_shapes_leave_no_pixel_near_the_threshold():
    """the shapes the GPU test uses: no interpolated value within 1e-5 of 0.5, the mask neither empty nor full"""
    for src, dst in (((150, 200), (72, 96)), ((300, 400), (144, 192)), ((72, 96), (144, 192)), ((100, 130), (72, 96))):
        m, v = so.mask_resize(so.synthetic_mask(*src), dst, return_values=True)
        assert int((np.abs(v - 0.5) <= 1e-5).sum()) == 0
        assert 0.3 < m.mean() < 0.6


# ---- the host code of svs_hip/scene.py ----
def _ulps(a, b):
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("src,dst", [(1600, 768), (1200, 576), (800, 192), (96, 192), (130, 96), (200, 96), (64, 64)])
def test_tables_match_the_oracle(scene, src, dst):
    ofs, coef = scene.cubic_table(dst, src)
    want_ofs, want = so.cubic_table(dst, src)
    assert ofs.dtype == np.int32 and coef.dtype == np.float32 and coef.shape == (dst, 4)
    assert np.array_equal(ofs, want_ofs)
    assert float(_ulps(coef, want).max()) <= 2.0
    ofs, coef = scene.linear_table(dst, src)
    want_ofs, want = so.linear_table(dst, src)
    assert ofs.dtype == np.int32 and coef.dtype == np.float32 and coef.shape == (dst, 2)
    assert np.array_equal(ofs, want_ofs)
    assert float(_ulps(coef, want).max()) <= 2.0
    if src == dst:
        assert np.array_equal(ofs, np.arange(dst)) and np.array_equal(coef[:, 0], np.ones(dst))


def test_camera_decomposition_round_trip_and_scipy(scene):
    from scipy.linalg import rq
    rng = np.random.default_rng(11)
    for _ in range(50):
        K, R, c = so.random_camera(rng, (1200, 1600))
        P = (K @ np.concatenate([R, -(R @ c)[:, None]], 1) * rng.uniform(0.1, 10.0)).astype(np.float32)
        for fn in (scene.load_K_Rt_from_P, so.load_K_Rt_from_P):
            intr, pose = fn(P)
            assert intr.shape == (4, 4) and pose.shape == (4, 4) and pose.dtype == np.float32 and intr.dtype == np.float64
            assert intr[2, 2] == 1.0 and np.array_equal(intr[3], [0, 0, 0, 1]) and np.array_equal(pose[3], [0, 0, 0, 1])
            # K's entries are O(1000): 1e-5 relative to the focal length
            assert np.abs(intr[:3, :3] - K).max() <= 1e-5 * K[0, 0]
            assert np.abs(pose[:3, :3] - R.T).max() <= 1e-5
            assert np.abs(pose[:3, 3] - c).max() <= 1e-5
        intr2, pose2 = scene.load_K_Rt_from_P(None, P)            # the reference's calling form
        assert np.array_equal(intr2, scene.load_K_Rt_from_P(P)[0])
        Ks, Rs = rq(P[:, :3].astype(np.float64))
        sgn = np.sign(np.diag(Ks))
        Ks, Rs = Ks * sgn[None, :], Rs * sgn[:, None]
        intr, pose = scene.load_K_Rt_from_P(P)
        assert np.abs(intr[:3, :3] - Ks / Ks[2, 2]).max() <= 1e-9 * K[0, 0]
        assert np.abs(pose[:3, :3] - Rs.T).max() <= 1e-6           # pose is stored in float32


def test_dtu_id_tables(scene):
    assert scene.get_trains_ids("DTU", "scan24", 3) == [25, 22, 28]
    assert scene.get_trains_ids("DTU", "scan24", 49) == list(range(49))
    ev = scene.get_eval_ids("DTU")
    assert len(ev) == 25 and not set(ev) & set(scene.DTU_TRAIN_IDS) and not set(ev) & set(scene.DTU_EXCLUDE_IDS)
    with pytest.raises(NotImplementedError):
        scene.get_trains_ids("DTU", "scan24", 0)
    scene.register_blendedmvs_ids(77, [4, 1, 2], [0, 3], {i: [4, 1, 2][i % 3] for i in range(6)})
    assert scene.get_trains_ids("BlendedMVS", "scan77", 3) == [4, 1, 2] and scene.get_eval_ids("BlendedMVS", 77) == [0, 3]
    assert scene.get_near_id("BlendedMVS", 77, 5) == 2


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "volsdf", "vsdf.py")),
                    reason=f"needs a checkout of the reference at {REFERENCE} (SVOLSDF_REFERENCE_ROOT)")
def test_id_tables_equal_the_reference_checkout(scene, monkeypatch):
    monkeypatch.setenv("SVOLSDF_REFERENCE_ROOT", REFERENCE)
    from svs_hip import scans
    monkeypatch.setattr(scans, "_REF_FUNCS", None)
    ref = scans._reference_functions()
    assert set(ref) == {"get_trains_ids", "get_eval_ids", "get_near_id", "scan2hash"}
    for n in (3, 4, 5, 6, 9, 49):
        assert scene.get_trains_ids("DTU", "scan24", n) == ref["get_trains_ids"]("DTU", "scan24", n)
    assert scene.get_eval_ids("DTU") == ref["get_eval_ids"]("DTU")
    assert scene.get_trains_ids("BlendedMVS", "scan3", 3) == ref["get_trains_ids"]("BlendedMVS", "scan3", 3)
    assert len(scene.get_eval_ids("BlendedMVS", 3)) == 12 and scene.get_near_id("BlendedMVS", 3, 0) in \
        scene.get_trains_ids("BlendedMVS", "scan3", 3)


# ---- the dataset surface, image work bound to the oracle ----
def _oracle_image_work(scene, monkeypatch):
    calls = dict(images=0, masks=0)

    def prepare_images(codes, img_res):
        calls["images"] += 1
        codes = np.asarray(codes)
        rgb, smooth = [], []
        for c in codes:
            img = c.astype(np.float32) * np.float32(1.0 / 255.0)
            if c.shape[:2] != tuple(img_res):
                img = so.resize_cubic(img, img_res).astype(np.float32)
            rgb.append(img.reshape(-1, 3))
            smooth.append(so.gaussian_smooth(img).astype(np.float32).reshape(-1, 3))
        return torch.from_numpy(np.stack(rgb)), torch.from_numpy(np.stack(smooth))

    def prepare_masks(masks, img_res, divisor=1.0):
        calls["masks"] += 1
        out = [so.mask_resize(np.asarray(m).astype(np.float32) / np.float32(divisor), img_res) for m in masks]
        return torch.from_numpy(np.repeat(np.stack(out).reshape(len(out), -1, 1), 3, 2).astype(np.float32))
    monkeypatch.setattr(scene, "prepare_images", prepare_images)
    monkeypatch.setattr(scene, "prepare_masks", prepare_masks)
    return calls


def _check_against_oracle(ds, want, tol=0.0):
    n = want["n_images"]
    assert len(ds) == ds.n_images == n
    for name, key in (("rgb_images", "rgb"), ("rgb_smooth", "rgb_smooth"), ("masks", "masks")):
        got = getattr(ds, name)
        assert isinstance(got, list) and len(got) == n
        for g, w in zip(got, want[key]):
            assert g.dtype == torch.float32 and tuple(g.shape) == (ds.total_pixels, 3) and g.device.type == "cpu"
            assert float(np.abs(g.numpy() - w).max()) <= tol + 1e-7           # (float32 rounding of the float64 oracle)
    for g, w in zip(ds.intrinsics_all, want["intrinsics"]):
        assert g.dtype == torch.float32 and tuple(g.shape) == (4, 4)
        assert np.abs(g.numpy() - w).max() <= 1e-5 * max(1.0, float(np.abs(w).max()))
    for g, w in zip(ds.pose_all, want["pose"]):
        assert g.dtype == torch.float32 and np.abs(g.numpy() - w).max() <= 1e-5
    assert ds.scale_factor == want["scale_factor"] and ds.cam_file == want["cam_file"]


@pytest.mark.parametrize("layout,own_cameras", [("mask", True), ("flat", False)])
def test_dtu_folder(scene, monkeypatch, tmp_path, layout, own_cameras):
    calls = _oracle_image_work(scene, monkeypatch)
    root, res = str(tmp_path), (36, 48)
    so.write_scan(root, "DTU", 24, 4, (50, 66), mask_views=(0, 1, 2), mask_layout=layout, mask_size=(60, 80),
                  own_cameras=own_cameras)
    ds = scene.SceneDataset("DTU", res, scan_id=24, num_views=3, data_dir_root=root)
    for a in ("rgb_images", "rgb_smooth", "masks", "intrinsics_all", "pose_all", "scale_factor", "n_images", "total_pixels",
              "img_res", "mode", "plot_id", "sampling_idx", "cam_file", "num_views", "data_dir", "scan_id"):
        assert hasattr(ds, a), a
    assert (ds.mode, ds.plot_id, ds.sampling_idx, ds.total_pixels, ds.resized) == ("train", 0, None, 36 * 48, True)
    assert ("scan114" in ds.cam_file) == (not own_cameras)
    _check_against_oracle(ds, so.load_scene(root, "DTU", 24, res, scene))
    assert ds.mask_views == [1, 2] and 0.3 < float(ds.masks[1].mean()) < 0.6 and bool((ds.masks[0] == 1).all())
    assert ds.get_scale_mat().shape == (4, 4)
    # a second dataset of the same folder: the same tensors, no image work
    n = dict(calls)
    ds2 = scene.SceneDataset("DTU", res, scan_id=24, num_views=3, data_dir_root=root)
    assert calls == n and ds2.cache_hit and not ds.cache_hit
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(ds.rgb_images + ds.rgb_smooth + ds.masks,
                                                            ds2.rgb_images + ds2.rgb_smooth + ds2.masks))
    assert scene.SceneDataset("DTU", (18, 24), scan_id=24, num_views=3, data_dir_root=root).cache_hit is False
    monkeypatch.setenv("SVS_SCENE_CACHE", "0")
    ds3 = scene.SceneDataset("DTU", res, scan_id=24, num_views=3, data_dir_root=root)
    assert calls["images"] > n["images"] and ds3.rgb_images[0].data_ptr() != ds.rgb_images[0].data_ptr()
    assert all(torch.equal(a, b) for a, b in zip(ds.rgb_images + ds.masks, ds3.rgb_images + ds3.masks))


def test_unmasked_dtu_scan_and_native_size(scene, monkeypatch, tmp_path):
    _oracle_image_work(scene, monkeypatch)
    root = str(tmp_path)
    so.write_scan(root, "DTU", 4, 3, (20, 28))
    ds = scene.SceneDataset("DTU", (20, 28), scan_id=4, num_views=3, data_dir_root=root)
    assert not ds.resized and ds.mask_views == [] and all(bool((m == 1).all()) for m in ds.masks)
    code = so.read_image(os.path.join(root, "DTU", "scan4", "image", "000001.png"))
    assert torch.equal(ds.rgb_images[1], torch.from_numpy(code.astype(np.float32) * np.float32(1 / 255.0)).reshape(-1, 3))
    _check_against_oracle(ds, so.load_scene(root, "DTU", 4, (20, 28), scene))


def test_blendedmvs_folder_items_and_cached_items(scene, monkeypatch, tmp_path):
    from svs_hip.batches import CachedItems
    _oracle_image_work(scene, monkeypatch)
    root, res, n = str(tmp_path), (24, 32), 6
    scene.register_blendedmvs_ids(5, train=[4, 1, 2], eval=[0, 3], near={i: [4, 1, 2][i % 3] for i in range(n)})
    so.write_scan(root, "BlendedMVS", 5, n, (40, 52), mask_views=(0, 1, 2, 3, 4))
    ds = scene.SceneDataset("BlendedMVS", res, scan_id=5, num_views=3, data_dir_root=root)
    _check_against_oracle(ds, so.load_scene(root, "BlendedMVS", 5, res, scene))
    assert ds.scale_factor == 1.0 and ds.mask_views == [0, 1, 2, 3, 4] and bool((ds.masks[5] == 1).all())
    assert ds.trains_ids() == [4, 1, 2]

    # item and batch layouts: what tests/test_cached_items_cpu.py expects of the reference's class
    random.seed(3)
    idx, sample, gt = ds[0]
    assert idx in (4, 1, 2) and list(sample) == ["uv", "intrinsics", "pose", "near_pose"] and list(gt) == ["rgb", "rgb_smooth", "mask"]
    assert tuple(sample["uv"].shape) == (24 * 32, 2) and sample["uv"][33].tolist() == [1.0, 1.0]
    assert torch.equal(sample["near_pose"], ds.pose_all[scene.get_near_id("BlendedMVS", 5, idx)])
    assert gt["rgb"] is ds.rgb_images[idx] and gt["mask"] is ds.masks[idx]
    ds.change_sampling_idx(37)
    idx, sample, gt = ds[0]
    assert tuple(sample["uv"].shape) == (37, 2) and tuple(gt["rgb"].shape) == (37, 3) and tuple(gt["mask"].shape) == (768, 3)
    assert torch.equal(gt["rgb_smooth"], ds.rgb_smooth[idx][ds.sampling_idx])
    b = ds.collate_fn([ds[0], ds[0]])
    assert b[0].dtype == torch.long and tuple(b[1]["uv"].shape) == (2, 37, 2) and tuple(b[2]["mask"].shape) == (2, 768, 3)
    ds.change_sampling_idx(-1)
    ds.mode = "plot"
    assert [ds[0][0] for _ in range(3)] == [0, 3, 0]
    ds.mode = "train"

    def loop(items, seed=3):
        torch.manual_seed(seed); random.seed(seed)
        loader = torch.utils.data.DataLoader(items, batch_size=1, shuffle=True, collate_fn=items.collate_fn)
        out = []
        for _ in range(3):
            ds.change_sampling_idx(29)
            for batch in loader:
                out.append(batch)
                ds.change_sampling_idx(29)
        return out
    plain = loop(ds)
    ci = CachedItems(ds)
    fast = loop(ci)
    assert ci.reason is None and ci.own_items == 3 and ci.fast_items == len(fast) - 3
    for a, b in zip(plain, fast):
        assert torch.equal(a[0], b[0])
        for x, y in zip(a[1:], b[1:]):
            assert list(x) == list(y) and all(torch.equal(x[k], y[k]) for k in x)


def test_blendedmvs_without_tables_says_so(scene, monkeypatch, tmp_path):
    monkeypatch.setattr("svs_hip.scans._REF_FUNCS", {})
    monkeypatch.delenv("SVS_SCENE_IDS", raising=False)
    so.write_scan(str(tmp_path), "BlendedMVS", 8, 2, (20, 28))
    with pytest.raises(LookupError, match="register_blendedmvs_ids"):
        scene.SceneDataset("BlendedMVS", (20, 28), scan_id=8, num_views=3, data_dir_root=str(tmp_path))


def test_bad_files_raise(scene, monkeypatch, tmp_path):
    from PIL import Image
    _oracle_image_work(scene, monkeypatch)
    root = str(tmp_path)
    inst = so.write_scan(root, "DTU", 4, 2, (20, 28))
    Image.fromarray(np.zeros((20, 28), np.uint16)).save(os.path.join(inst, "image", "000001.png"))
    with pytest.raises(ValueError):
        scene.SceneDataset("DTU", (16, 16), scan_id=4, data_dir_root=root)
    with pytest.raises(NotImplementedError):
        scene.SceneDataset("Other", (16, 16), scan_id=4, data_dir_root=root)


# ---- the C entry points reject bad arguments before any launch ----
def test_entry_points_check_their_arguments():
    from svs_hip import lib
    L = lib.load()
    d = ctypes.c_void_p(64)                      # never dereferenced
    EINVAL, ESHAPE = -1, -2

    def cubic(codes=d, V=2, Hs=40, Ws=50, H=20, W=30, tabs=(d, d, d, d), out=d):
        return L.svs_scene_resize_cubic(codes, V, Hs, Ws, H, W, *tabs, out, None)

    def smooth(img=d, V=2, H=20, W=30, ws=d, out=d):
        return L.svs_scene_smooth(img, V, H, W, ws, out, None)

    def mask(m=d, div=1.0, V=2, Hs=40, Ws=50, H=20, W=30, tabs=(d, d, d, d), out=d):
        return L.svs_scene_mask(m, div, V, Hs, Ws, H, W, *tabs, out, None)
    for fn, name, nulls in ((cubic, b"svs_scene_resize_cubic", [dict(codes=None), dict(out=None), dict(tabs=(None, d, d, d))]),
                            (smooth, b"svs_scene_smooth", [dict(img=None), dict(ws=None), dict(out=None)]),
                            (mask, b"svs_scene_mask", [dict(m=None), dict(out=None), dict(tabs=(d, d, None, d))])):
        for kw in nulls:
            assert fn(**kw) == EINVAL, (name, kw)
            assert name in L.svs_last_error_string()
        for v in (0, -1):
            assert fn(V=v) == EINVAL and name in L.svs_last_error_string()
        for hw in (dict(H=15), dict(W=15), dict(H=0, W=0), dict(H=-20)):
            assert fn(**hw) == ESHAPE and name in L.svs_last_error_string(), (name, hw)
    assert cubic(Hs=0) == ESHAPE and mask(Ws=0) == ESHAPE and mask(div=0.0) == EINVAL
    assert L.svs_scene_workspace_bytes(2, 20, 30) == 2 * 20 * 30 * 3 * 4
    assert L.svs_scene_workspace_bytes(2, 15, 30) == 0 and L.svs_scene_workspace_bytes(0, 20, 30) == 0
