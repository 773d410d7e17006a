"""CPU checks of evaluation-view rendering (svs_hip/evalviews.py): the numpy oracle reproduces the reference-made
fixture evalviews_finish.npz (codes equal, float32 products to the last bit), the cast rule, how far the oracle's
float32 evaluation of the colour step strays from its float64 one on the inputs the GPU test uses, and the host side of
the module: arguments, default view lists, file names, checkpoint discovery, nvs.load_gt(scene=)."""
import os
import types

import numpy as np
import pytest
import torch

import evalviews_oracle as eo
import scene_oracle as so
import svs_oracle as orc

CAP = 0.005                                    # the share of pixels the GPU colour test may excuse
GPU_CASES = ((11, (576, 768)), (12, (61, 75)))           # (seed, size) of tests/test_gpu_evalviews.py's colour cases


def table_step(table):
    """the most codes a pixel moves when its index lands in the neighbouring table row (plus one for the truncation)"""
    return int(np.ceil(255.0 * np.abs(np.diff(table, axis=0)).max())) + 1


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "evalviews_finish.npz")))


@pytest.fixture(scope="module")
def ev():
    from svs_hip import evalviews
    return evalviews


def test_cast_rule():
    """the values the issue lists for x86 numpy's float32 -> uint8 cast"""
    x = np.array([-1.5, -0.2, 255.9, 256.0, 300.7, -256.5, 1e6], np.float32)
    assert eo.to_code(x).tolist() == [255, 0, 255, 0, 44, 0, 64]
    assert eo.to_code(np.array([np.nan, 3e9, -3e9, np.inf], np.float32)).tolist() == [0, 0, 0, 0]
    assert eo.to_code(np.array([-1.5, 300.7, 2147483000.0])).tolist() == [255, 44, 2147483000 & 255]


def test_oracle_reproduces_the_reference_fixture(golden):
    g = golden
    H, W = (int(v) for v in g["img_res"])
    o = eo.finish(g["rgb_values"], g["normal_map"], g["depth_values"], g["weights"], g["scale_factor"])
    assert np.array_equal(o["rgb_codes"].reshape(H, W, 3), g["rgb_codes"])
    assert np.array_equal(o["normal_codes"].reshape(H, W, 3), g["normal_codes"])
    wrapped = (np.abs(g["normal_map"]) > 1.0).any(-1).mean()
    assert wrapped > 0.2                                                   # the wrap-around rule is exercised
    assert o["depth_est"].dtype == np.float32
    assert np.array_equal(o["depth_est"].reshape(H, W).view(np.uint32), g["depth_est"].view(np.uint32))
    # acc: the reference sums with torch.sum (ATen's cascade, restated in oracle/svs_oracle.py): equal to the last bit;
    # the exact sums lie within the bound any float32 order obeys
    acc_ref = g["acc"].reshape(-1)
    assert np.array_equal(orc.aten_sum(g["weights"])[:, 0].view(np.uint32), acc_ref.view(np.uint32))
    assert (np.abs(acc_ref.astype(np.float64) - o["acc"]) <= o["acc_bound"]).all()
    assert (acc_ref < 0.2).mean() > 0.05 and acc_ref.max() > 1.0
    # the two percentile bounds and the colour codes, in the reference's number formats
    table = eo.turbo_table()
    lo, hi = eo.depth_bounds(g["depth_values"], acc_ref, mode="f32")
    assert (lo + float(eo.EPS), hi - float(eo.EPS)) == tuple(g["bounds"].tolist())
    codes = eo.depth_colors(g["depth_values"], acc_ref, lo, hi, table, (H, W), mode="f32")
    assert np.array_equal(codes, g["depth_codes"])
    # float64 evaluation: the same codes except near an integer boundary
    lo64, hi64 = eo.depth_bounds(g["depth_values"], acc_ref, mode="f64")
    assert abs(lo64 - lo) <= 2.0 ** -20 * abs(lo) and abs(hi64 - hi) <= 2.0 ** -20 * abs(hi)
    c64 = eo.depth_colors(g["depth_values"], acc_ref, lo, hi, table, (H, W), mode="f64")
    assert (c64 != codes).any(-1).mean() <= CAP
    assert np.abs(c64.astype(int) - codes.astype(int)).max() <= table_step(table)


@pytest.mark.parametrize("seed,hw", GPU_CASES)
def test_float32_colours_stay_under_the_cap_on_the_gpu_inputs(seed, hw):
    """The GPU test excuses pixels whose table index or final value lies within 1e-5 of an integer in the float64
    evaluation, at most 0.5 % of them.  On its inputs: that share, and the share of pixels where the oracle's float32
    evaluation (the reference's formats) gives another code than its float64 one, both under the cap."""
    inp = eo.seeded_view(seed, hw)
    o = eo.finish(**{k: inp[k] for k in ("rgb_values", "normal_map", "depth_values", "weights")}, scale_factor=1.0)
    acc = o["acc"].astype(np.float32)
    table = eo.turbo_table()
    lo, hi = eo.depth_bounds(inp["depth_values"], acc, mode="f64")
    c64, xa, final = eo.depth_colors(inp["depth_values"], acc, lo, hi, table, hw, mode="f64", return_values=True)
    c32 = eo.depth_colors(inp["depth_values"], acc, lo, hi, table, hw, mode="f32")
    excused = eo.near_boundary(xa, final, acc).mean()
    differ = (c32 != c64).any(-1).mean()
    print(f"{hw}: {100 * excused:.4f} % of pixels within 1e-5 of a boundary, float32 vs float64 codes differ at "
          f"{100 * differ:.4f} %")
    assert excused <= CAP and differ <= CAP
    assert np.abs(c32.astype(int) - c64.astype(int)).max() <= table_step(table)


def test_weighted_percentile_is_np_interp_on_cumulative_weights():
    rng = np.random.default_rng(3)
    x, w = rng.random(1000).astype(np.float32), rng.random(1000).astype(np.float32)
    w[::7] = 0.0
    lo, hi = eo.weighted_percentile(x, w, [0.5, 99.5])
    order = np.argsort(x)
    cw = np.cumsum(w[order].astype(np.float64))
    for p, got in ((0.5, lo), (99.5, hi)):
        k = np.searchsorted(cw, p * cw[-1] / 100, side="right")
        assert x[order][k - 1] <= got <= x[order][k]


# ---- the host side of svs_hip.evalviews ------------------------------------------------------------------------------
def test_arguments(ev):
    a = ev.parse_args(["--ckpt", "c", "--data-dir-root", "d", "--dataset", "DTU", "--scan", "106"])
    assert (a.ckpt, a.checkpoint, a.data_dir_root, a.dataset, a.scan) == ("c", "latest", "d", "DTU", 106)
    assert tuple(a.img_res) == (576, 768) and a.evals_folder == "exps_result" and a.expname == "ours"
    assert a.split_n_pixels == 512 and a.views is None and a.src_views is None and a.ibr is None and a.score is False
    a = ev.parse_args(["--ckpt", "c", "--data-dir-root", "d", "--dataset", "BlendedMVS", "--scan", "3", "--img-res", "96",
                       "128", "--views", "1", "2", "0", "--src-views", "0", "--ibr", "mvs/scan3", "--score",
                       "--split-n-pixels", "1000", "--evals-folder", "out", "--expname", "x", "--checkpoint", "500"])
    assert a.views == [1, 2, 0] and a.src_views == [0] and a.ibr == "mvs/scan3" and a.score and a.img_res == [96, 128]
    assert (a.split_n_pixels, a.evals_folder, a.expname, a.checkpoint) == (1000, "out", "x", "500")
    for bad in (["--dataset", "DTU"], ["--ckpt", "c", "--data-dir-root", "d", "--dataset", "Tanks", "--scan", "1"]):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)


def test_default_views(ev, monkeypatch):
    from svs_hip import scene
    views, train = ev.default_views("DTU", 106)
    assert train == [25, 22, 28] and views[-3:] == train
    assert views[:-3] == [i for i in range(49) if i not in scene.DTU_TRAIN_IDS + scene.DTU_EXCLUDE_IDS] and len(views) == 28
    scene.register_blendedmvs_ids(91, train=[4, 1, 2], eval=[0, 3, 5], near={i: 4 for i in range(6)})
    assert ev.default_views("BlendedMVS", 91) == ([0, 3, 5, 4, 1, 2], [4, 1, 2])
    monkeypatch.setattr("svs_hip.scans._REF_FUNCS", {})
    monkeypatch.delenv("SVS_SCENE_IDS", raising=False)
    with pytest.raises(LookupError, match="register_blendedmvs_ids"):
        ev.default_views("BlendedMVS", 92)


def test_file_names(ev, tmp_path):
    names = ev.view_files("out", 7)
    assert names == dict(rgb=os.path.join("out", "eval_007.png"), normal=os.path.join("out", "normal_007.png"),
                         depth_vis=os.path.join("out", "dep_007.png"),
                         depth_est=os.path.join("out", "depth_est", "00000007.pfm"))
    from datasets.data_io import read_pfm
    from PIL import Image
    rng = np.random.default_rng(0)
    host = dict(rgb=rng.integers(0, 256, (6, 8, 3), dtype=np.uint8), normal=rng.integers(0, 256, (6, 8, 3), dtype=np.uint8),
                depth_vis=None, depth_est=rng.random((6, 8)).astype(np.float32), acc=np.ones((6, 8), np.float32))
    os.makedirs(tmp_path / "depth_est")
    written = ev.write_view(str(tmp_path), 123, host)
    assert sorted(os.path.relpath(p, tmp_path) for p in written) == ["depth_est/00000123.pfm", "eval_123.png",
                                                                       "normal_123.png"]
    assert np.array_equal(np.array(Image.open(tmp_path / "eval_123.png")), host["rgb"])
    assert np.array_equal(np.array(Image.open(tmp_path / "normal_123.png")), host["normal"])
    back = np.asarray(read_pfm(str(tmp_path / "depth_est" / "00000123.pfm"))[0])
    assert back.dtype == np.float32 and np.array_equal(back, host["depth_est"])


def test_checkpoint_discovery(ev, tmp_path):
    run = tmp_path / "exps" / "ours_24" / "2026_01_01_00_00_00"
    mp = run / "checkpoints" / "ModelParameters"
    os.makedirs(mp)
    for name in ("latest", "500"):
        torch.save({"epoch": 500, "model_state_dict": {}, "iter_step": 1}, mp / f"{name}.pth")
    assert ev.find_checkpoint(str(mp / "500.pth")) == str(mp / "500.pth")
    assert ev.find_checkpoint(str(run / "checkpoints")) == str(mp / "latest.pth")
    assert ev.find_checkpoint(str(run / "checkpoints"), "500") == str(mp / "500.pth")
    assert ev.find_checkpoint(str(run), "latest") == str(mp / "latest.pth")
    with pytest.raises(FileNotFoundError):
        ev.find_checkpoint(str(run), "700")
    with pytest.raises(RuntimeError):                       # a strict load: a checkpoint of another model is an error
        ev.load_model(str(mp / "latest.pth"), "DTU", "cpu")


def test_models_follow_the_dataset(ev):
    from volsdf.model.network import VolSDFNetwork
    from volsdf.model.network_bg import VolSDFNetworkBG
    assert type(ev.build_model("DTU")) is VolSDFNetwork and type(ev.build_model("BlendedMVS")) is VolSDFNetworkBG
    with pytest.raises(NotImplementedError):
        ev.build_model("Tanks")


def test_load_gt_from_a_scene(tmp_path):
    """nvs.load_gt(scene=): a native-size scan gives the default path's arrays exactly; the default path is unchanged."""
    from svs_hip import nvs
    root, size = str(tmp_path), (20, 28)
    so.write_scan(root, "DTU", 24, 3, size, mask_views=(0, 1, 2))
    gt, m = nvs.load_gt(root, "DTU", 24, [1, 2], img_res=size)
    rgb = [torch.from_numpy(so.load_rgb(os.path.join(root, "DTU", "scan24", "image", f"{i:06d}.png")).reshape(-1, 3))
           for i in range(3)]
    masks = [torch.ones(size[0] * size[1], 3)] + [torch.from_numpy(m[k].reshape(-1, 3).astype(np.float32)) for k in (0, 1)]
    scene = types.SimpleNamespace(img_res=list(size), n_images=3, rgb_images=rgb, masks=masks)
    gt2, m2 = nvs.load_gt(root, "DTU", 24, [1, 2], img_res=size, scene=scene)
    assert gt2.dtype == np.uint8 and m2.dtype == np.uint8 and np.array_equal(gt, gt2) and np.array_equal(m, m2)
    assert 0 < m.mean() < 1
    _, m3 = nvs.load_gt(root, "DTU", 24, [0], img_res=size, scene=scene, mask=False)
    assert (m3 == 1).all()
    with pytest.raises(ValueError):
        nvs.load_gt(root, "DTU", 24, [1], img_res=(10, 14), scene=scene)
    with pytest.raises(IndexError):
        nvs.load_gt(root, "DTU", 24, [3], img_res=size, scene=scene)
    with pytest.raises(NotImplementedError):                # without a scene a size mismatch still says so
        nvs.load_gt(root, "DTU", 24, [1], img_res=(10, 14))
