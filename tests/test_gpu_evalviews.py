"""GPU checks of evaluation-view rendering (csrc/svs_evalviews.hip, svs_hip/evalviews.py) against the reference-made
fixture evalviews_finish.npz and the numpy oracle (tests/evalviews_oracle.py, which reproduces the fixture:
tests/test_evalviews_cpu.py).

svs_view_finish: rgb codes, normal codes and depth_est EQUAL (each is one IEEE float32 operation chain and a
truncation); acc within (S-1) 2^-24 sum|w| of the float64 row sum and bit-identical between two runs.
svs_view_depth_colors: the percentile bounds within 2^-23 relative of the oracle's float64 ones (both sum the weights in
float64; a float32 ulp of the bound is the scale the colours can resolve); codes equal to the float64 oracle's given the
same bounds, except pixels whose table index value or final value lies within 1e-5 of an integer in the oracle's
evaluation, which may differ by one code; at most 0.5 % of the pixels may be excused (observed share printed; on these
inputs test_evalviews_cpu.py measures 0.0047 % and 0 %).
End to end: synthetic DTU folder + geometrically initialised model + checkpoint -> main() -> files -> blend -> scores."""
import ctypes
import os

import numpy as np
import pytest
import torch

import evalviews_oracle as eo
import scene_oracle as so

pytestmark = pytest.mark.gpu
SVS_EINVAL, SVS_ESHAPE = -1, -2
CAP = 0.005
KEYS = ("rgb_values", "normal_map", "depth_values", "weights")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ev(dev):
    from svs_hip import evalviews
    return evalviews


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "evalviews_finish.npz")))


def _finish(ev, dev, inp, scale):
    out = ev.finish_arrays(*[torch.from_numpy(inp[k]).to(dev) for k in KEYS], scale)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check_finish(ev, dev, inp, scale):
    o = eo.finish(*[inp[k] for k in KEYS], scale)
    rgb, nrm, dep, acc = _finish(ev, dev, inp, scale)
    assert rgb.dtype == np.uint8 and nrm.dtype == np.uint8 and dep.dtype == np.float32 and acc.dtype == np.float32
    assert np.array_equal(rgb, o["rgb_codes"])
    assert np.array_equal(nrm, o["normal_codes"])
    assert np.array_equal(dep.view(np.uint32), o["depth_est"].view(np.uint32))
    err = np.abs(acc.astype(np.float64) - o["acc"])
    print(f"N = {acc.size}: acc max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(o['acc_bound'], 1e-300)):.3f}")
    assert (err <= o["acc_bound"]).all()
    again = _finish(ev, dev, inp, scale)[3]
    assert np.array_equal(acc.view(np.uint32), again.view(np.uint32))
    return rgb, nrm, dep, acc


def test_finish_matches_the_reference_fixture(ev, dev, golden):
    g = golden
    H, W = (int(v) for v in g["img_res"])
    rgb, nrm, dep, acc = _check_finish(ev, dev, g, float(g["scale_factor"]))
    assert np.array_equal(rgb.reshape(H, W, 3), g["rgb_codes"]) and np.array_equal(nrm.reshape(H, W, 3), g["normal_codes"])
    assert np.array_equal(dep.reshape(H, W).view(np.uint32), g["depth_est"].view(np.uint32))
    S = g["weights"].shape[1]
    bound = (S - 1) * 2.0 ** -24 * np.abs(g["weights"].astype(np.float64)).sum(1)
    assert (np.abs(acc.astype(np.float64) - g["acc"].reshape(-1)) <= 2 * bound).all()      # two float32 orders


@pytest.mark.parametrize("seed,hw,S", [(11, (576, 768), 98), (12, (61, 75), 98), (13, (33, 21), 97), (14, (16, 17), 4),
                                       (15, (5, 3), 1), (16, (9, 7), 131)])
def test_finish_vs_oracle(ev, dev, seed, hw, S):
    """576x768, and sizes that are not multiples of the wavefront (nor of the 4-row set), odd and tiny S"""
    _check_finish(ev, dev, eo.seeded_view(seed, hw, S), 1.7)


def test_finish_takes_unaligned_weights(ev, dev):
    """weights that do not start on a 16-byte boundary are read with 4-byte loads: the same elements in the same order"""
    inp = eo.seeded_view(17, (40, 23), 98)
    args = [torch.from_numpy(inp[k]).to(dev) for k in KEYS]
    want = [t.cpu().numpy() for t in ev.finish_arrays(*args, 2.0)]
    flat = torch.empty(args[3].numel() + 1, dtype=torch.float32, device=dev)
    flat[1:].copy_(args[3].reshape(-1))
    shifted = flat[1:].view_as(args[3])
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    got = [t.cpu().numpy() for t in ev.finish_arrays(args[0], args[1], args[2], shifted, 2.0)]
    for a, b in zip(want, got):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_colors(ev, dev, depth, acc, hw):
    table = eo.turbo_table()
    d, a = torch.from_numpy(depth).to(dev), torch.from_numpy(acc).to(dev)
    lo, hi = ev.depth_bounds(d, a)
    lo64, hi64 = eo.depth_bounds(depth, acc, mode="f64")
    print(f"{hw}: bounds {lo!r}, {hi!r}; oracle {lo64!r}, {hi64!r}")
    assert abs(lo - lo64) <= 2.0 ** -23 * abs(lo64) and abs(hi - hi64) <= 2.0 ** -23 * abs(hi64)
    codes = ev.depth_colors(d, a, hw, lo64, hi64, torch.from_numpy(table).to(dev)).cpu().numpy()
    want, xa, final = eo.depth_colors(depth, acc, lo64, hi64, table, hw, mode="f64", return_values=True)
    assert codes.shape == want.shape and codes.dtype == np.uint8
    excused = eo.near_boundary(xa, final, acc)
    diff = np.abs(codes.astype(int) - want.astype(int)).max(-1)
    print(f"{hw}: {100 * excused.mean():.4f} % of pixels excused, {int((diff != 0).sum())} pixels differ")
    assert excused.mean() <= CAP
    assert (diff[~excused] == 0).all() and (diff[excused] <= 1).all()
    return codes


def test_depth_colors_on_the_fixture(ev, dev, golden):
    g = golden
    H, W = (int(v) for v in g["img_res"])
    codes = _check_colors(ev, dev, g["depth_values"], g["acc"].reshape(-1), (H, W))
    # against the reference's own image (float32 curve and index, float32 cumulative weights): the few pixels whose
    # index lands in the neighbouring table row
    differ = (codes != g["depth_codes"]).any(-1).mean()
    print(f"fixture: {100 * differ:.4f} % of pixels differ from the reference's dep image")
    assert differ <= CAP


@pytest.mark.parametrize("seed,hw", [(11, (576, 768)), (12, (61, 75))])
def test_depth_colors_vs_oracle(ev, dev, seed, hw):
    inp = eo.seeded_view(seed, hw)
    acc = eo.finish(*[inp[k] for k in KEYS], 1.0)["acc"].astype(np.float32)
    _check_colors(ev, dev, inp["depth_values"], acc, hw)


def test_finish_view_shapes_and_the_table_argument(ev, dev, golden):
    g = golden
    H, W = (int(v) for v in g["img_res"])
    out = {k: torch.from_numpy(g[k]).to(dev) for k in KEYS}
    out["depth_values"] = out["depth_values"].reshape(-1, 1)              # as render_image returns it
    res = ev.finish_view(out, (H, W), float(g["scale_factor"]))
    assert {k: (tuple(v.shape), v.dtype) for k, v in res.items()} == {
        "rgb": ((H, W, 3), torch.uint8), "normal": ((H, W, 3), torch.uint8), "depth_est": ((H, W), torch.float32),
        "acc": ((H, W), torch.float32), "depth_vis": ((H, W, 3), torch.uint8)}
    assert all(v.is_cuda for v in res.values())
    assert np.array_equal(res["rgb"].cpu().numpy(), g["rgb_codes"])
    assert ev.finish_view(out, (H, W), 1.0, cmap=False)["depth_vis"] is None
    grey = np.repeat(np.linspace(0, 1, 7)[:, None], 3, 1)
    vis = ev.finish_view(out, (H, W), 1.0, cmap=grey)["depth_vis"].cpu().numpy()
    acc = res["acc"].cpu().numpy().reshape(-1)
    lo, hi = ev.depth_bounds(out["depth_values"].reshape(-1), res["acc"].reshape(-1))
    assert np.array_equal(vis, eo.depth_colors(g["depth_values"], acc, lo, hi, grey, (H, W), mode="f64"))
    with pytest.raises(ValueError):
        ev.finish_view(out, (H, W + 1), 1.0)


def test_rejected_calls_write_nothing(dev):
    from svs_hip import lib
    L = lib.load()
    N, S = 200, 10
    f = lambda *s: torch.rand(*s, device=dev)                              # noqa: E731
    rgb, nrm, dep, w = f(N, 3), f(N, 3), f(N), f(N, S)
    outs = [torch.full((N, 3), 7, dtype=torch.uint8, device=dev), torch.full((N, 3), 7, dtype=torch.uint8, device=dev),
            torch.full((N,), -3.0, device=dev), torch.full((N,), -3.0, device=dev)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())                            # noqa: E731
    good = [p(rgb), p(nrm), p(dep), p(w), N, S, 1.0] + [p(t) for t in outs] + [None]
    for i, val, code in [(0, None, SVS_EINVAL), (3, None, SVS_EINVAL), (7, None, SVS_EINVAL), (10, None, SVS_EINVAL),
                         (4, 0, SVS_ESHAPE), (4, -5, SVS_ESHAPE), (5, 0, SVS_ESHAPE), (5, 1 << 20, SVS_ESHAPE)]:
        args = list(good)
        args[i] = val
        assert L.svs_view_finish(*args) == code and b"svs_view_finish" in L.svs_last_error_string()
    table = torch.rand(256, 3, dtype=torch.float64, device=dev)
    codes = torch.full((N, 3), 7, dtype=torch.uint8, device=dev)
    good2 = [p(dep), p(dep), N, 20, 0.5, 2.0, p(table), 256, p(codes), None]
    for i, val, code in [(0, None, SVS_EINVAL), (6, None, SVS_EINVAL), (8, None, SVS_EINVAL), (2, 0, SVS_ESHAPE),
                         (3, 0, SVS_ESHAPE), (3, 7, SVS_ESHAPE), (7, 0, SVS_ESHAPE)]:
        args = list(good2)
        args[i] = val
        assert L.svs_view_depth_colors(*args) == code and b"svs_view_depth_colors" in L.svs_last_error_string()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs[:2] + [codes]) and all(bool((t == -3.0).all()) for t in outs[2:])
    assert L.svs_view_finish(*good) == 0 and L.svs_view_depth_colors(*good2) == 0
    torch.cuda.synchronize()
    assert not bool((outs[3] == -3.0).any()) and not bool((codes == 7).all())


def _write_mvs_folder(root, ds, n):
    """cams/{:08d}_cam.txt and images/{:08d}.png of the scan in the layout svs_hip.ibr reads, from the dataset's own
    cameras (world units: the scale matrix folded back in, as depth_est is depth * scale_factor)"""
    from PIL import Image
    from helpers.utils import write_cam
    from svs_hip.scene import load_K_Rt_from_P
    cams = np.load(ds.cam_file)
    os.makedirs(os.path.join(root, "cams"))
    os.makedirs(os.path.join(root, "images"))
    H, W = ds.img_res
    for i in range(n):
        K, pose = load_K_Rt_from_P(cams[f"world_mat_{i}"][:3, :4])
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0] = np.linalg.inv(pose.astype(np.float64))
        cam[1, :3, :3] = K[:3, :3]
        cam[1, 3] = (0.1, 0.01, 192, 10.0)
        write_cam(os.path.join(root, "cams", f"{i:08d}_cam.txt"), cam)
        img = (ds.rgb_images[i].numpy().reshape(H, W, 3).astype(np.float64) * 255).round().astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "images", f"{i:08d}.png"))


def test_checkpoint_to_scores_end_to_end(ev, dev, tmp_path, capsys):
    from PIL import Image
    from datasets.data_io import read_pfm
    from svs_hip import nvs, scene
    from svs_hip.renderer import render_image
    root, size, n, scan = str(tmp_path / "data"), (96, 128), 6, 24
    so.write_scan(root, "DTU", scan, n, size, mask_views=(0, 1, 2))
    torch.manual_seed(5)
    model = ev.build_model("DTU")                                          # geometric initialisation: a sphere
    mp = tmp_path / "exps" / f"ours_{scan}" / "2026_01_01_00_00_00" / "checkpoints" / "ModelParameters"
    os.makedirs(mp)
    torch.save({"epoch": 42, "model_state_dict": model.state_dict(), "iter_step": 7}, mp / "latest.pth")
    ds = scene.SceneDataset("DTU", list(size), scan_id=scan, data_dir_root=root)
    mvs = str(tmp_path / "mvs")
    _write_mvs_folder(mvs, ds, n)
    views, src = [1, 2, 0, 3], [0, 3]
    evals = str(tmp_path / "result")
    res = ev.main(["--ckpt", str(mp.parent), "--checkpoint", "latest", "--data-dir-root", root, "--dataset", "DTU",
                   "--scan", str(scan), "--img-res", str(size[0]), str(size[1]), "--evals-folder", evals,
                   "--views"] + [str(v) for v in views] + ["--src-views"] + [str(v) for v in src] +
                  ["--ibr", mvs, "--score", "--split-n-pixels", "512"])
    folder = os.path.join(evals, f"ours_{scan}", "rendering_42")
    printed = capsys.readouterr().out
    assert res["folder"] == folder and res["epoch"] == 42 and folder in printed and "seconds: load" in printed
    assert f"SCAN {scan}:" in printed and "psnr mean" in printed and "ssim mean" in printed
    for v in views:
        names = ev.view_files(folder, v)
        for k in ("rgb", "normal", "depth_vis"):
            img = np.array(Image.open(names[k]))
            assert img.shape == size + (3,) and img.dtype == np.uint8, names[k]
        depth = np.asarray(read_pfm(names["depth_est"])[0])
        assert depth.shape == size and depth.dtype == np.float32 and np.isfinite(depth).all()
    # the files hold exactly finish_view's products of a direct render of the same view
    model2, epoch = ev.load_model(str(mp / "latest.pth"), "DTU", dev)
    assert epoch == 42
    v = views[0]
    _, model_input, _ = ds.collate_fn([ds[v]])
    out = render_image(model2, {k: t.to(dev) for k, t in model_input.items()}, size[0] * size[1], split_n_pixels=512,
                       keys=ev.RENDER_KEYS)
    direct = ev.finish_view(out, size, ds.scale_factor)
    names = ev.view_files(folder, v)
    assert np.array_equal(np.array(Image.open(names["rgb"])), direct["rgb"].cpu().numpy())
    assert np.array_equal(np.array(Image.open(names["normal"])), direct["normal"].cpu().numpy())
    assert np.array_equal(np.array(Image.open(names["depth_vis"])), direct["depth_vis"].cpu().numpy())
    assert np.array_equal(np.asarray(read_pfm(names["depth_est"])[0]).view(np.uint32),
                          direct["depth_est"].cpu().numpy().view(np.uint32))
    # blends and scores
    refs = [1, 2]
    for r in refs:
        blend = np.array(Image.open(os.path.join(folder, f"eval_blend_{r:03d}.png")))
        assert blend.shape == size + (3,) and blend.dtype == np.uint8
    assert np.isfinite(res["scores"]["psnr"]).all() and np.isfinite(res["scores"]["ssim"]).all()
    for rf in ("default", "blend"):
        s = nvs.score_scan(folder, root, "DTU", scan, refs, result_from=rf, img_res=size)
        assert s["psnr"].shape == (2,) and np.isfinite(s["psnr"]).all() and np.isfinite(s["ssim"]).all()
        if rf == "blend":                                                  # the scene= path scored the same arrays
            assert np.array_equal(s["psnr"], res["scores"]["psnr"]) and np.array_equal(s["ssim"], res["scores"]["ssim"])
