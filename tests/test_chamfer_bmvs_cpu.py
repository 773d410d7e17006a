"""CPU-side checks of the BlendedMVS Chamfer evaluator (evals/eval_bmvs.py): the oracle the GPU tests compare against is
pinned to the reference scripts' own outputs (fixture chamfer_bmvs_ref.npz), and everything of the module that needs no
device -- the scale table, the file rules, the command line, the PLY writer, the argument checks of the two entry points."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import bmvs_chamfer_oracle as borc
import synth
import synth_bmvs
from evals import eval_bmvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "chamfer_bmvs_ref.npz")))


def _shuffled(sc, seed):
    perm = np.arange(len(sc["data_pcd"]))
    np.random.default_rng(seed).shuffle(perm)
    return sc["data_pcd"][perm]


def _check_colors(fx, prefix, rgb):
    every = int(fx["every"])
    assert len(rgb) == int(fx[prefix + "_n"])
    np.testing.assert_array_equal(rgb[::every], fx[prefix + "_rows"])
    np.testing.assert_array_equal(borc.color_classes(rgb), fx[prefix + "_classes"])
    np.testing.assert_allclose(rgb.sum(0), fx[prefix + "_colsum"], rtol=1e-12)


@pytest.mark.parametrize("scan", [4, 5])
def test_oracle_equals_reference_script(fx, scan):
    """Scan 4: the prepared cloud, all distances and the colours bit for bit.  Scan 5 goes through the script's BLAS dot:
    cloud to 1e-13, distances to 1e-12."""
    k = f"s{scan}"
    sc = synth_bmvs.make_bmvs_scan(int(fx[k + "_seed"]), scan)
    means, d = borc.evaluate_scan(_shuffled(sc, int(fx[k + "_shuffle_seed"])), sc["gt_pcd"], sc["relative_scale"], sc["scale_mat"])
    assert len(d["data_pcd"]) == int(fx[k + "_n_data"])
    head = d["data_pcd"][:len(fx[k + "_data_head"])]
    if scan == 4:
        np.testing.assert_array_equal(head, fx[k + "_data_head"])
        for side in ("d2s", "s2d"):
            np.testing.assert_array_equal(d["dist_" + side], fx[f"{k}_dist_{side}"])
            _check_colors(fx, f"{k}_color_{side}", borc.error_colors(d["dist_" + side])[0])
    else:
        np.testing.assert_allclose(head, fx[k + "_data_head"], rtol=1e-13, atol=0)
        for side in ("d2s", "s2d"):
            np.testing.assert_allclose(d["dist_" + side], fx[f"{k}_dist_{side}"], rtol=1e-12, atol=0)
            np.testing.assert_array_equal(borc.color_classes(borc.error_colors(d["dist_" + side])[0]), fx[f"{k}_color_{side}_classes"])
    np.testing.assert_allclose(means, fx[k + "_means"], rtol=1e-12)
    assert str(fx[k + "_row"]) == 'scan{:0>3} {:.2f} {:.2f} {:.2f}'.format(scan, *means)


def test_oracle_colors_equal_reference_dtu_script(fx):
    """The scatter to a partly evaluated cloud (eval_dtu.py:178-187): the oracle's colours of the DTU fixture scan."""
    import chamfer_oracle as corc
    sc = synth.make_dtu_scan(int(fx["dtu_seed"]))
    data = sc["data_pcd"].copy()
    np.random.default_rng(int(fx["dtu_shuffle_seed"])).shuffle(data, axis=0)
    means, d = corc.evaluate_scan(data, sc["stl"], sc["ObsMask"], sc["BB"], sc["Res"], sc["P"], n_jobs=2)
    np.testing.assert_allclose(means, fx["dtu_means"], rtol=1e-12)
    _, in_obs = corc.obs_filter(d["data_down"], sc["ObsMask"], sc["BB"], sc["Res"], 60)
    stl_hom = np.concatenate([sc["stl"], np.ones_like(sc["stl"][:, :1])], -1)
    above = (sc["P"].reshape((1, 4)) * stl_hom).sum(-1) > 0
    vis = float(fx["dtu_vis_dist"])
    _check_colors(fx, "dtu_color_d2s", borc.error_colors(d["dist_d2s"], 20, vis, select=in_obs)[0])
    _check_colors(fx, "dtu_color_s2d", borc.error_colors(d["dist_s2d"], 20, vis, select=above)[0])


def test_index_shuffle_is_the_scripts_row_shuffle():
    """shuffle_rows draws what `default_rng().shuffle(float32 array, axis=0)` draws (eval_bmvs.py:201-202)."""
    pts = np.random.default_rng(3).normal(0, 1, (1001, 3)).astype(np.float32)
    want = pts.copy()
    np.random.default_rng(11).shuffle(want, axis=0)
    np.testing.assert_array_equal(eval_bmvs.shuffle_rows(pts, np.random.default_rng(11)), want)
    assert eval_bmvs.shuffle_rows(pts, False) is pts


def test_uint8_rule():
    """(uint8) rint(min(1, max(0, c)) * 255) at its edges; the expected bytes come from exact rational arithmetic: the
    float64 product correctly rounded, then round-half-to-even."""
    def exact(c):
        c = min(1.0, max(0.0, c))
        prod = float(Fraction(c) * 255)                                  # float() of a Fraction rounds correctly
        lo = int(Fraction(prod) // 1)
        frac = Fraction(prod) - lo
        return lo + (1 if frac > Fraction(1, 2) or (frac == Fraction(1, 2) and lo % 2) else 0)
    cases = [0.0, 1.0, np.nextafter(1.0, 2.0), 0.5 / 255, 1.5 / 255, -0.25, 0.999]
    got = borc.colors_u8(np.array(cases))
    assert got.dtype == np.uint8
    assert got.tolist() == [exact(float(c)) for c in cases]
    assert got[:3].tolist() == [0, 255, 255]


def test_relative_scale_table_and_get_scales(tmp_path):
    assert sorted(eval_bmvs.RELATIVE_SCALE) == list(range(1, 10)) == list(eval_bmvs.SCANS)
    assert eval_bmvs.RELATIVE_SCALE[5] == 0.007349738091050388 and eval_bmvs.RELATIVE_SCALE[9] == 0.022978406132555827
    rng = np.random.default_rng(5)
    dtu = 312.5 + rng.uniform()

    def cameras(folder, s):
        os.makedirs(folder)
        m0, m1 = np.eye(4), np.eye(4)
        m0[:3, :3] *= s; m1[:3, :3] *= s
        m0[:3, 3] = rng.normal(0, 1, 3)
        np.savez(os.path.join(folder, "cameras.npz"), scale_mat_0=m0, scale_mat_1=m1, world_mat_0=np.eye(4))
    cameras(tmp_path / "DTU" / "scan114", dtu)
    scales = {s: float(rng.uniform(0.2, 8.0)) for s in range(1, 10)}
    for s, v in scales.items():
        cameras(tmp_path / "BlendedMVS" / f"scan{s}", v)
    got_dtu, got_bmvs, got_rel = eval_bmvs.get_scales(str(tmp_path))
    assert got_dtu == dtu and got_bmvs == scales
    assert got_rel == {s: v / dtu for s, v in scales.items()}
    # scale_mat_0 and scale_mat_1 have to agree (eval_bmvs.py:62,73)
    m = np.eye(4) * 2.0
    np.savez(tmp_path / "BlendedMVS" / "scan3" / "cameras.npz", scale_mat_0=np.eye(4), scale_mat_1=m)
    with pytest.raises(AssertionError):
        eval_bmvs.get_scales(str(tmp_path))


def _write_ply(fn, pts):
    with open(fn, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\n"
                 "property double z\nend_header\n" % len(pts)).encode())
        np.ascontiguousarray(pts, "<f8").tofile(f)


def test_file_rules(tmp_path, monkeypatch):
    """Which files a scan reads: the cropped ground truth unless no_crop, scale_mat_0 for scan 5 only, the table's ratio."""
    rng = np.random.default_rng(9)
    root, pred = tmp_path / "root" / "BlendedMVS", tmp_path / "pred"
    (root / "stl").mkdir(parents=True); (root / "scan5").mkdir(); (root / "scan4").mkdir(); pred.mkdir()
    clouds = {}
    for scan in (4, 5):
        for name in (f"scan{scan}_crop.ply", f"scan{scan}.ply"):
            clouds[name] = rng.normal(0, 1, (7 + len(clouds), 3))
            _write_ply(root / "stl" / name, clouds[name])
        clouds[f"pred{scan}"] = rng.normal(0, 1, (20 + scan, 3))
        _write_ply(pred / f"mvsnet{scan:03}_l3.ply", clouds[f"pred{scan}"])
        mat = np.eye(4) * (scan + 0.5)
        np.savez(root / f"scan{scan}" / "cameras.npz", scale_mat_0=mat, scale_mat_1=mat)
    calls = []

    def fake(data_pcd, gt_pcd, relative_scale, scale_mat=None, **kw):
        calls.append(dict(data_pcd=data_pcd, gt_pcd=gt_pcd, relative_scale=relative_scale, scale_mat=scale_mat, kw=kw))
        return (1.0, 2.0, 1.5), {}
    monkeypatch.setattr(eval_bmvs, "evaluate_scan", fake)
    assert eval_bmvs.evaluate_scan_files(4, str(pred), str(tmp_path / "root"), shuffle_rng=False) == (1.0, 2.0, 1.5)
    c = calls[-1]
    np.testing.assert_array_equal(c["data_pcd"], clouds["pred4"]); np.testing.assert_array_equal(c["gt_pcd"], clouds["scan4_crop.ply"])
    assert c["scale_mat"] is None and c["relative_scale"] == eval_bmvs.RELATIVE_SCALE[4] and c["kw"]["shuffle_rng"] is False
    eval_bmvs.evaluate_scan_files(4, str(pred), str(tmp_path / "root"), no_crop=True)
    np.testing.assert_array_equal(calls[-1]["gt_pcd"], clouds["scan4.ply"])
    eval_bmvs.evaluate_scan_files(5, str(pred), str(tmp_path / "root"))
    c = calls[-1]
    np.testing.assert_array_equal(c["scale_mat"], np.eye(4) * 5.5)
    np.testing.assert_array_equal(c["gt_pcd"], clouds["scan5_crop.ply"])
    assert c["relative_scale"] == eval_bmvs.RELATIVE_SCALE[5]
    with pytest.raises(OSError):
        eval_bmvs.evaluate_scan_files(6, str(pred), str(tmp_path / "root"))          # no prediction


def test_command_line(monkeypatch, capsys):
    seen = []

    def fake(scan, datadir, data_dir_root, no_crop=False, visualize_error=False, **kw):
        seen.append((scan, datadir, data_dir_root, no_crop, visualize_error))
        if scan == 3:
            raise ValueError("Found array with 0 sample(s)")                         # an empty cloud: skipped
        if scan == 7:
            raise FileNotFoundError("mvsnet007_l3.ply")                              # a missing one too
        return scan + 0.123, scan + 0.456, scan + 0.2895
    monkeypatch.setattr(eval_bmvs, "evaluate_scan_files", fake)
    res = eval_bmvs.main(["--datadir", "p", "--data_dir_root", "r", "--scan", "77", "--no_crop"])      # unknown scan: all nine
    assert [s[0] for s in seen] == list(range(1, 10)) and all(s[1:] == ("p", "r", True, False) for s in seen)
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0] == "ply_name, chamfer(mm)"
    assert lines[1:] == ['scan{:0>3} {:.2f} {:.2f} {:.2f}'.format(s, s + 0.123, s + 0.456, s + 0.2895) for s in (1, 2, 4, 5, 6, 8, 9)]
    assert sorted(res) == [1, 2, 4, 5, 6, 8, 9]
    del seen[:]
    eval_bmvs.main(["--scan", "4", "-ve", "--sample", "10", "--dataset_dir", "x"])
    assert seen == [(4, "", "data_s_volsdf", False, True)]
    with pytest.raises(SystemExit) as e:
        eval_bmvs.main(["--save_gt"])
    assert "not provided" in str(e.value.code)
    assert eval_bmvs.scan2hash.__module__ == "svs_hip.scans"


def test_dtu_command_line_keeps_its_flags_and_gains_two():
    from evals import eval_dtu
    import inspect
    sig = inspect.signature(eval_dtu.evaluate_scan)
    assert sig.parameters["visualize"].default is None and sig.parameters["details"].default is False
    with pytest.raises(SystemExit):
        eval_dtu.main(["--no_such_flag"])


def test_vis_pcd_round_trip(tmp_path):
    from svs_hip import ply
    from svs_hip.ply import read_points
    rng = np.random.default_rng(2)
    pts = rng.normal(0, 100, (257, 3))
    pts[0] = [1e30, -0.0, np.nextafter(1.0, 2.0)]                                    # float64 survives the file
    rgb = rng.integers(0, 256, (257, 3)).astype(np.uint8)
    fn = str(tmp_path / "cloud.ply")
    ply.write(fn, pts, rgb, coords="double")
    got_pts, got_rgb = read_points(fn)
    np.testing.assert_array_equal(got_pts, pts); np.testing.assert_array_equal(got_rgb, rgb)
    header = open(fn, "rb").read(400).split(b"end_header\n")[0].decode().split("\n")
    assert header[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 257"]
    assert header[3:9] == ["property double x", "property double y", "property double z", "property uchar red",
                           "property uchar green", "property uchar blue"]
    assert os.path.getsize(fn) == len("\n".join(header)) + len("end_header\n") + 257 * 27
    ply.write(fn, np.zeros((0, 3)), np.zeros((0, 3), np.uint8), coords="double")
    assert read_points(fn)[0].shape == (0, 3)


def test_argument_errors_come_back_as_codes():
    """Both entry points validate before they touch the device: nothing is launched here."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("svs_build", os.path.join(ROOT, "s-volsdf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from svs_hip import lib
    L = lib.load()
    d = ctypes.c_void_p(64)                          # never dereferenced
    for scale in (0.0, -1.0, float("nan")):
        assert L.svs_cloud_prepare(d, 0, 4, None, scale, d, None) < 0 and b"svs_cloud_prepare" in L.svs_last_error_string()
    assert L.svs_cloud_prepare(None, 0, 4, None, 1.0, d, None) < 0 and L.svs_cloud_prepare(d, 1, 4, None, 1.0, None, None) < 0
    assert L.svs_cloud_prepare(d, 0, -1, None, 1.0, d, None) < 0
    assert L.svs_cloud_prepare(None, 0, 0, None, 1.0, None, None) == 0              # an empty cloud is not an error
    assert L.svs_cloud_error_colors(None, 3, None, None, 3, 20.0, 10.0, d, d, None) < 0
    assert b"svs_cloud_error_colors" in L.svs_last_error_string()
    assert L.svs_cloud_error_colors(d, 3, None, None, 4, 20.0, 10.0, d, d, None) < 0          # no select: n_full == n_dist
    assert L.svs_cloud_error_colors(d, 3, d, None, 4, 20.0, 10.0, d, d, None) < 0             # select without rank
    assert L.svs_cloud_error_colors(d, 5, d, d, 4, 20.0, 10.0, d, d, None) < 0                # more distances than rows
    assert L.svs_cloud_error_colors(d, 3, None, None, 3, 20.0, 0.0, d, d, None) < 0
    assert L.svs_cloud_error_colors(None, 0, None, None, 0, 20.0, 10.0, None, None, None) == 0
