"""GPU parity of the scene loader (csrc/svs_scene.hip, svs_hip/scene.py) against the float64 oracle of
tests/scene_oracle.py with the float32 source coordinate of the parity definition (coord="f32").  Synthetic arrays and
folders only.

Bounds (derived, not measured):
  rgb         1e-5 absolute.  Values lie in about [-0.2, 1.2]; each pass is 4 products and 3 sums with sum|c| <= 1.375, both
              passes give at most (gamma_4 + 2u) 1.375^2 1.2 ~ 1e-6 with u = 2^-24; a factor of ten is left for the float32
              rounding of the coefficients.  A wrong tap, border rule or A costs 1e-3 or more.
  rgb_smooth  2e-5 absolute: the resize bound plus two 31-tap passes of positive weights summing to 1, gamma_32 2 1.2 ~ 5e-6.
  mask        exact wherever the oracle's interpolated value is farther than 1e-5 from 0.5; at most 1 % of the pixels may
              be left out on that ground.
Observed maxima are printed by each test (pytest -s)."""
import numpy as np
import pytest
import torch

import scene_oracle as so

pytestmark = pytest.mark.gpu
RGB_TOL, SMOOTH_TOL = 1e-5, 2e-5
MASK_BAND, MASK_MAX_LEFT_OUT = 1e-5, 0.01


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def scene(dev):
    from svs_hip import scene as sc
    saved = dict(sc._BMVS)
    sc.cache_clear()
    yield sc
    sc._BMVS.clear()
    sc._BMVS.update(saved)
    sc.cache_clear()


def _oracle_images(code, hw):
    img = code.astype(np.float32) * np.float32(1.0 / 255.0)
    rgb = so.resize_cubic(img, hw) if code.shape[:2] != tuple(hw) else img.astype(np.float64)
    return rgb, so.gaussian_smooth(rgb.astype(np.float32))


@pytest.mark.parametrize("src,dst,V", [((1200, 1600), (576, 768), 2), ((600, 800), (144, 192), 3), ((72, 96), (144, 192), 3),
                                       ((100, 130), (72, 96), 3), ((144, 192), (144, 192), 2), ((100, 130), (100, 96), 1),
                                       ((40, 50), (16, 16), 2), ((33, 47), (67, 259), 1)])
def test_prepare_images(scene, src, dst, V):
    codes = np.stack([so.synthetic_image(src[0], src[1], 100 + v) for v in range(V)])
    rgb, smooth = scene.prepare_images(codes, dst)
    assert rgb.is_cuda and rgb.dtype == torch.float32 and tuple(rgb.shape) == tuple(smooth.shape) == (V, dst[0] * dst[1], 3)
    rgb, smooth = rgb.cpu().numpy().reshape(V, *dst, 3), smooth.cpu().numpy().reshape(V, *dst, 3)
    e_rgb = e_smooth = 0.0
    for v in range(V):
        want_rgb, want_smooth = _oracle_images(codes[v], dst)
        e_rgb = max(e_rgb, float(np.abs(rgb[v] - want_rgb).max()))
        e_smooth = max(e_smooth, float(np.abs(smooth[v] - want_smooth).max()))
    print(f"{src}->{dst}: max |rgb - oracle| {e_rgb:.3g}, max |rgb_smooth - oracle| {e_smooth:.3g}")
    assert e_rgb <= RGB_TOL and e_smooth <= SMOOTH_TOL
    if src == dst:
        assert np.array_equal(rgb, codes.astype(np.float32) * np.float32(1.0 / 255.0))         # the pass-through is exact
    # a device tensor goes the same way, bit for bit
    again = scene.prepare_images(torch.from_numpy(codes).to("cuda:0"), dst)
    assert np.array_equal(again[0].cpu().numpy().reshape(rgb.shape), rgb)
    assert np.array_equal(again[1].cpu().numpy().reshape(smooth.shape), smooth)


@pytest.mark.parametrize("src,dst", [((33, 47), (67, 259)),    # neither ratio rational, upscale, W: two workgroups, ragged tail
                                     ((40, 50), (16, 16)),     # the smallest destination, taps clamp on all four borders
                                     ((32, 64), (32, 64))])    # equal sizes, every code in every channel
def test_cubic_resize_is_one_arithmetic(scene, dev, src, dst):
    """The two loaders' resizes differ in the code-to-float rule and in nothing else: the MVS entry point, given the
    scene loader's rule as its code table, returns the scene loader's bits."""
    from svs_hip import lib
    from svs_hip.images import cubic_table, tables_device
    from svs_hip.ops import _ptr, _stream
    from mvsdata_oracle import all_codes
    V, (H, W) = 2, dst
    image = (lambda v: all_codes(src[0], src[1], 3, v)) if src == dst else (lambda v: so.synthetic_image(src[0], src[1], 7 + v))
    codes = torch.from_numpy(np.stack([image(v) for v in range(V)])).to(dev)
    if src == dst:
        assert all(len(np.unique(codes[v, ..., c].cpu().numpy())) == 256 for v in range(V) for c in range(3))
    rgb = scene.prepare_images(codes, dst)[0]
    table = torch.from_numpy(np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0)).to(dev)
    tabs = [None] * 4 if src == dst else tables_device(cubic_table, H, W, src[0], src[1], dev)
    out = torch.full((V, H, W, 3), 7.0, device=dev)
    assert lib.load().svs_mvs_resize_cubic(_ptr(codes), 0, _ptr(table), V, src[0], src[1], 3, H, W, *[_ptr(t) for t in tabs],
                                           _ptr(out), _stream()) == 0
    assert torch.equal(rgb.reshape(V, H, W, 3), out)


@pytest.mark.parametrize("src,dst", [((150, 200), (72, 96)), ((300, 400), (144, 192)), ((72, 96), (144, 192)),
                                     ((100, 130), (72, 96)), ((72, 96), (72, 96))])
def test_prepare_masks(scene, src, dst):
    masks = np.stack([np.roll(so.synthetic_mask(*src), 3 * v, axis=1) for v in range(3)])
    got = scene.prepare_masks(masks, dst)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, dst[0] * dst[1], 3)
    got = got.cpu().numpy().reshape(3, *dst, 3)
    assert set(np.unique(got)) == {0.0, 1.0}
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    left_out = 0
    for v in range(3):
        want, vals = so.mask_resize(masks[v], dst, return_values=True)
        sure = np.abs(vals - 0.5) > MASK_BAND
        left_out += int((~sure).sum())
        assert np.array_equal(got[v, ..., 0][sure], want[sure])
    print(f"{src}->{dst}: {left_out} pixels within {MASK_BAND} of the threshold, {100 * got.mean():.1f} % inside")
    assert left_out <= MASK_MAX_LEFT_OUT * got[..., 0].size
    assert 0.0 < got.mean() < 1.0


def test_alpha_masks_are_interpolated_before_the_threshold(scene):
    """the BlendedMVS alpha channel: code / 255 is resized, THEN thresholded"""
    rng = np.random.default_rng(4)
    alpha = np.clip(np.rint(so.synthetic_mask(90, 120) * 255 * rng.uniform(0.3, 1.0, (90, 120))), 0, 255).astype(np.uint8)
    got = scene.prepare_masks(alpha[None], (48, 64), divisor=255.0).cpu().numpy().reshape(48, 64, 3)[..., 0]
    want, vals = so.mask_resize(alpha.astype(np.float32) / np.float32(255.0), (48, 64), return_values=True)
    sure = np.abs(vals - 0.5) > MASK_BAND
    assert (~sure).sum() <= MASK_MAX_LEFT_OUT * sure.size and np.array_equal(got[sure], want[sure])
    assert 0.0 < got.mean() < 1.0
    first = so.mask_resize((alpha.astype(np.float32) / np.float32(255.0) > 0.5).astype(np.float32), (48, 64))
    assert not np.array_equal(first, want)                   # the other order is a different mask


def test_rejected_calls_write_nothing(scene, dev):
    from svs_hip import lib
    from svs_hip.ops import _ptr, _stream
    L = lib.load()
    img = torch.rand(1, 20, 30, 3, device=dev)
    out = torch.full((1, 20, 30, 3), 7.0, device=dev)
    ws = torch.full((int(L.svs_scene_workspace_bytes(1, 20, 30)),), 7, dtype=torch.uint8, device=dev)
    assert L.svs_scene_smooth(_ptr(img), 1, 15, 30, _ptr(ws), _ptr(out), _stream()) == -2
    assert L.svs_scene_smooth(_ptr(img), 0, 20, 30, _ptr(ws), _ptr(out), _stream()) == -1
    assert L.svs_scene_smooth(_ptr(img), 1, 20, 30, None, _ptr(out), _stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 7).all())
    assert L.svs_scene_smooth(_ptr(img), 1, 20, 30, _ptr(ws), _ptr(out), _stream()) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
    with pytest.raises(TypeError):
        scene.prepare_images(np.zeros((1, 20, 30, 3), np.float32), (16, 16))
    with pytest.raises(lib.SvsError):
        scene.prepare_images(np.zeros((1, 20, 30, 3), np.uint8), (15, 16))


def _check_dataset(ds, want):
    e = dict(rgb=0.0, smooth=0.0, left_out=0)
    for v in range(want["n_images"]):
        assert ds.rgb_images[v].device.type == "cpu" and ds.rgb_images[v].dtype == torch.float32
        e["rgb"] = max(e["rgb"], float(np.abs(ds.rgb_images[v].numpy() - want["rgb"][v]).max()))
        e["smooth"] = max(e["smooth"], float(np.abs(ds.rgb_smooth[v].numpy() - want["rgb_smooth"][v]).max()))
        vals = want["mask_values"].get(v)
        sure = np.ones(ds.total_pixels, bool) if vals is None else np.abs(vals - 0.5) > MASK_BAND
        e["left_out"] += int((~sure).sum())
        assert np.array_equal(ds.masks[v].numpy()[sure], want["masks"][v][sure])
        assert np.abs(ds.intrinsics_all[v].numpy() - want["intrinsics"][v]).max() <= 1e-5 * max(
            1.0, float(np.abs(want["intrinsics"][v]).max()))
        assert np.abs(ds.pose_all[v].numpy() - want["pose"][v]).max() <= 1e-5
    print(f"dataset: max |rgb - oracle| {e['rgb']:.3g}, max |rgb_smooth - oracle| {e['smooth']:.3g}, "
          f"{e['left_out']} mask pixels near the threshold")
    assert e["rgb"] <= RGB_TOL and e["smooth"] <= SMOOTH_TOL
    assert e["left_out"] <= MASK_MAX_LEFT_OUT * ds.total_pixels * max(1, len(want["mask_values"]))
    assert ds.scale_factor == want["scale_factor"] and ds.n_images == want["n_images"] and ds.cam_file == want["cam_file"]


def test_dtu_folder_cache_and_device_batches(scene, tmp_path, monkeypatch):
    import random
    from svs_hip.batches import DeviceBatches
    root, res = str(tmp_path), (72, 96)
    so.write_scan(root, "DTU", 24, 11, (150, 200), mask_views=(0, 1, 2, 9, 10), mask_size=(150, 200))
    ds = scene.SceneDataset("DTU", res, scan_id=24, num_views=3, data_dir_root=root)
    assert ds.resized and not ds.cache_hit and ds.mask_views == [1, 2, 9, 10] and ds.rgb_images[0].is_pinned()
    _check_dataset(ds, so.load_scene(root, "DTU", 24, res, scene))
    assert 0.0 < float(ds.masks[9].mean()) < 1.0 and bool((ds.masks[0] == 1).all())

    # a second construction: the same storage, nothing launched
    before = dict(scene.LAUNCHES)
    ds2 = scene.SceneDataset("DTU", res, scan_id=24, num_views=3, data_dir_root=root)
    assert ds2.cache_hit and scene.LAUNCHES == before
    for a, b in zip(ds.rgb_images + ds.rgb_smooth + ds.masks, ds2.rgb_images + ds2.rgb_smooth + ds2.masks):
        assert a.data_ptr() == b.data_ptr()
    # the cache off: recomputed, bit-identical
    monkeypatch.setenv("SVS_SCENE_CACHE", "0")
    ds3 = scene.SceneDataset("DTU", res, scan_id=24, num_views=3, data_dir_root=root)
    assert not ds3.cache_hit and scene.LAUNCHES["resize"] > before["resize"] and scene.LAUNCHES["mask"] > before["mask"]
    for a, b in zip(ds.rgb_images + ds.rgb_smooth + ds.masks, ds3.rgb_images + ds3.rgb_smooth + ds3.masks):
        assert torch.equal(a, b)
    assert ds3.rgb_images[0].data_ptr() != ds.rgb_images[0].data_ptr()

    # end to end: a device train batch holds the dataset's rows at the drawn pixels (a real 3-view run trains on views
    # 25, 22, 28; this folder has 11 images, so num_views = -1: every image is a training image)
    ds4 = scene.SceneDataset("DTU", res, scan_id=24, num_views=-1, data_dir_root=root)
    db = DeviceBatches(ds4, 64, "cuda:0")
    torch.manual_seed(0); random.seed(0)
    for _ in range(3):
        idx, sample, gt = db.batch()
        v = int(idx[0])
        uv = sample["uv"][0].cpu()
        pix = (uv[:, 1] * res[1] + uv[:, 0]).long()
        assert pix.unique().numel() == 64
        assert torch.equal(gt["rgb"][0].cpu(), ds4.rgb_images[v][pix])
        assert torch.equal(gt["rgb_smooth"][0].cpu(), ds4.rgb_smooth[v][pix])
        assert torch.equal(sample["pose"][0].cpu(), ds4.pose_all[v])


def test_blendedmvs_folder_with_near_pose(scene, tmp_path):
    import random
    from svs_hip.batches import DeviceBatches
    root, res, n = str(tmp_path), (72, 96), 6
    scene.register_blendedmvs_ids(3, train=[4, 1, 2], eval=[0, 3], near={i: [4, 1, 2][i % 3] for i in range(n)})
    so.write_scan(root, "BlendedMVS", 3, n, (100, 130), mask_views=(0, 1, 2, 3, 4), mask_size=(100, 130))
    ds = scene.SceneDataset("BlendedMVS", res, scan_id=3, num_views=3, data_dir_root=root)
    _check_dataset(ds, so.load_scene(root, "BlendedMVS", 3, res, scene))
    assert ds.mask_views == [0, 1, 2, 3, 4] and 0.0 < float(ds.masks[3].mean()) < 1.0
    random.seed(1)
    idx, sample, gt = ds[0]
    assert torch.equal(sample["near_pose"], ds.pose_all[scene.get_near_id("BlendedMVS", 3, idx)])
    db = DeviceBatches(ds, 32, "cuda:0")
    idx, sample, gt = db.batch()
    v = int(idx[0])
    assert v in (4, 1, 2) and torch.equal(sample["near_pose"][0].cpu(), ds.pose_all[scene.get_near_id("BlendedMVS", 3, v)])
    pix = (sample["uv"][0, :, 1] * res[1] + sample["uv"][0, :, 0]).long().cpu()
    assert torch.equal(gt["rgb"][0].cpu(), ds.rgb_images[v][pix])


def test_a_scan_larger_than_one_chunk_and_the_command_line(scene, tmp_path, capsys):
    root = str(tmp_path)
    n = 2 * scene.CHUNK + 3
    so.write_scan(root, "DTU", 4, n, (60, 80))
    ds = scene.SceneDataset("DTU", (32, 48), scan_id=4, data_dir_root=root)
    want = so.load_scene(root, "DTU", 4, (32, 48), scene)
    _check_dataset(ds, want)
    scene.cache_clear()
    scene.main(["--data-dir-root", root, "--dataset", "DTU", "--scan", "4", "--img-res", "32", "48"])
    out = capsys.readouterr().out
    assert f"{n} images" in out and "resized (cubic)" in out and "kernels" in out
