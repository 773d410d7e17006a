"""GPU parity of the BlendedMVS Chamfer evaluator and of the error clouds of both evaluators (csrc/svs_chamfer.hip,
evals/eval_bmvs.py, the additions to evals/eval_dtu.py): against the reference scripts' outputs (fixture
chamfer_bmvs_ref.npz) and against the numpy + sklearn oracle (tests/bmvs_chamfer_oracle.py) on edge values and sizes.
Bars: the prepared clouds and the colours bit for bit (both kernels are IEEE operations in numpy's order); distances closer
than the search radius bit-equal to the kd-tree's; means to 1e-12 relative (summation order); scan 5, whose matrix product
the reference leaves to its BLAS, to 1e-13 (cloud) and 1e-12 (distances)."""
import os

import numpy as np
import pytest
import torch

import bmvs_chamfer_oracle as borc
import synth
import synth_bmvs
from evals import eval_bmvs, eval_dtu
from svs_hip import clouds

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 4097]                      # below, at and above a wavefront; more than one block, not a multiple


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "chamfer_bmvs_ref.npz")))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype == np.uint8 else np.int64)


def _cloud(n, dtype, seed):
    rng = np.random.default_rng(seed)
    pts = rng.normal(0, 1, (n, 3)) * rng.choice([1e-3, 1.0, 250.0], (n, 1))
    edge = np.array([0.0, -0.0, 1e30, -1e30, -7.25, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -23, 1.0 / 3.0])
    flat = pts.reshape(-1)
    flat[rng.permutation(flat.size)[:min(len(edge), flat.size)]] = edge[:min(len(edge), flat.size)]
    return pts.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", SIZES)
def test_prepare_scale_mode_vs_oracle(dev, n, dtype):
    pts = _cloud(n, dtype, n)
    for scan, scale in eval_bmvs.RELATIVE_SCALE.items():
        got = clouds.prepare_cloud(pts, scale).cpu().numpy()
        want = borc.prepare(pts, scale)
        assert got.dtype == np.float64 and got.shape == (n, 3)
        assert np.array_equal(_bits(got), _bits(want)), (scan, np.abs(got - want).max())      # signed zeros included


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", SIZES)
def test_prepare_matrix_mode_vs_oracle(dev, n, dtype):
    """t_a = ((m_a0 p_0 + m_a1 p_1) + m_a2 p_2) + m_a3 then / scale, float64, nothing contracted: a full matrix, so that every
    term counts."""
    pts = _cloud(n, dtype, 100 + n)
    mat = np.random.default_rng(7).normal(0, 1, (4, 4)); mat[3] = [0, 0, 0, 1]
    for scale in (eval_bmvs.RELATIVE_SCALE[5], 1.0 / 3.0):
        got = clouds.prepare_cloud(pts, scale, mat).cpu().numpy()
        want = borc.prepare(pts, scale, mat)
        assert np.array_equal(_bits(got), _bits(want)), np.abs(got - want).max()
    got = clouds.prepare_cloud(torch.from_numpy(pts).to(dev), 0.5, mat).cpu().numpy()      # a device tensor is taken as is
    assert np.array_equal(_bits(got), _bits(borc.prepare(pts, 0.5, mat)))


def test_prepare_empty_and_bad_arguments(dev):
    assert clouds.prepare_cloud(np.zeros((0, 3), np.float32), 0.5).shape == (0, 3)
    from svs_hip.lib import SvsError
    with pytest.raises(SvsError):
        clouds.prepare_cloud(np.zeros((4, 3)), 0.0)
    with pytest.raises(ValueError):
        clouds.prepare_cloud(np.zeros((4, 3)), 1.0, np.eye(3))


def _distances(n, seed, max_dist=20.0, vis_dist=10.0):
    rng = np.random.default_rng(seed)
    d = np.abs(rng.normal(0, 12, n))
    edge = np.array([0.0, vis_dist, np.nextafter(vis_dist, 0), np.nextafter(vis_dist, np.inf), max_dist, np.nextafter(max_dist, 0),
                     np.inf, 1e300, 5.0, 1e-300])
    d[rng.permutation(n)[:min(len(edge), n)]] = edge[:min(len(edge), n)]
    return d


@pytest.mark.parametrize("n", SIZES)
def test_error_colors_vs_oracle(dev, n):
    """select = none, all, a random mask, and the same mask as a view one byte off a 16-byte boundary."""
    rng = np.random.default_rng(n)
    masks = [None, np.ones(n, np.uint8), (rng.uniform(0, 1, n) < 0.6).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)]
    for k, mask in enumerate(masks + [masks[2]]):
        n_dist = n if mask is None else int((mask != 0).sum())
        d = _distances(n_dist, 10 * n + k)
        for max_dist, vis_dist in ((20, 10), (20.0, 7.3)):
            d[:1] = vis_dist                                                             # the threshold itself is always in
            sel = None
            if mask is not None:
                sel = torch.from_numpy(mask).to(dev)
                if k == 3:
                    buf = torch.zeros(n + 32, dtype=torch.uint8, device=dev)
                    off = (1 - buf.data_ptr()) % 16
                    sel = buf[off:off + n]
                    sel.copy_(torch.from_numpy(mask))
                    assert sel.data_ptr() % 16 == 1
            rgb, u8 = clouds.error_colors(torch.from_numpy(d).to(dev), max_dist, vis_dist, select=sel)
            want, want_u8 = borc.error_colors(d, max_dist, vis_dist, select=mask)
            assert rgb.shape == u8.shape == (n, 3) and rgb.dtype == torch.float64 and u8.dtype == torch.uint8
            assert np.array_equal(_bits(rgb.cpu().numpy()), _bits(want)), (k, n)
            assert np.array_equal(u8.cpu().numpy(), want_u8), (k, n)


def test_error_colors_edges(dev):
    """inf is green, the thresholds fall on the side the script puts them, nothing evaluated is all blue, bool masks."""
    d = np.array([np.inf, 1e300, 20.0, np.nextafter(20.0, 0), 10.0, 0.0, 3.3])
    rgb, u8 = clouds.error_colors(torch.from_numpy(d).to(dev))
    rgb = rgb.cpu().numpy()
    np.testing.assert_array_equal(rgb[:3], [[0, 1, 0]] * 3)
    np.testing.assert_array_equal(rgb[3:5], [[1, 0, 0]] * 2)
    np.testing.assert_array_equal(rgb[5], [1, 1, 1])
    a = 3.3 / 10
    np.testing.assert_array_equal(rgb[6], [a + (1 - a), 1 - a, 1 - a])
    np.testing.assert_array_equal(u8.cpu().numpy()[:6], [[0, 255, 0]] * 3 + [[255, 0, 0]] * 2 + [[255, 255, 255]])
    for n in (1, 65, 4097):
        rgb, u8 = clouds.error_colors(torch.zeros(0, dtype=torch.float64, device=dev), select=torch.zeros(n, dtype=torch.uint8, device=dev))
        assert (rgb.cpu().numpy() == [0, 0, 1]).all() and (u8.cpu().numpy() == [0, 0, 255]).all() and len(rgb) == n
    mask = torch.tensor([True, False, True, True, False], device=dev)
    d = np.array([1.0, 25.0, 12.0])
    rgb, _ = clouds.error_colors(torch.from_numpy(d).to(dev), select=mask)
    np.testing.assert_array_equal(rgb.cpu().numpy(), borc.error_colors(d, select=mask.cpu().numpy())[0])
    assert clouds.error_colors(torch.zeros(0, dtype=torch.float64, device=dev))[0].shape == (0, 3)


def _check_u8_classes(u8, classes):
    """In bytes a graded colour within 1/510 of pure red IS pure red: blue, green and the sum of the two others are what a
    stored cloud can be counted by."""
    got = borc.color_classes(u8)
    assert (got[0], got[1], got[2] + got[3]) == (classes[0], classes[1], classes[2] + classes[3]) and got[2] >= classes[2]


def _check_colors(fx, prefix, rgb, u8):
    every = int(fx["every"])
    rgb, u8 = rgb.cpu().numpy(), u8.cpu().numpy()
    assert len(rgb) == len(u8) == int(fx[prefix + "_n"])
    assert np.array_equal(_bits(rgb[::every]), _bits(fx[prefix + "_rows"]))              # == the script's colours
    np.testing.assert_array_equal(borc.color_classes(rgb), fx[prefix + "_classes"])
    _check_u8_classes(u8, fx[prefix + "_classes"])
    np.testing.assert_array_equal(u8[::every], borc.colors_u8(fx[prefix + "_rows"]))
    np.testing.assert_allclose(rgb.sum(0), fx[prefix + "_colsum"], rtol=1e-12)


def test_fixture_covers_every_colour_branch(fx):
    """classes = (blue, green, saturated, graded): each branch holds enough rows of the reference's own clouds that none can
    go untested."""
    for scan in (4, 5):
        for side in ("d2s", "s2d"):
            blue, green, sat, graded = fx[f"s{scan}_color_{side}_classes"] / float(fx[f"s{scan}_color_{side}_n"])
            assert blue == 0 and min(green, sat, graded) >= 0.01, (scan, side, green, sat, graded)
    for side in ("d2s", "s2d"):
        blue, green, sat, graded = fx[f"dtu_color_{side}_classes"] / float(fx[f"dtu_color_{side}_n"])
        assert blue >= 0.10 and sat >= 0.01 and graded >= 0.01, (side, blue, sat, graded)


def _run_scan(fx, scan):
    k = f"s{scan}"
    sc = synth_bmvs.make_bmvs_scan(int(fx[k + "_seed"]), scan)
    res, d = eval_bmvs.evaluate_scan(sc["data_pcd"], sc["gt_pcd"], sc["relative_scale"], scale_mat=sc["scale_mat"],
                                     shuffle_rng=np.random.default_rng(int(fx[k + "_shuffle_seed"])), details=True)
    assert len(d["data_pcd"]) == int(fx[k + "_n_data"])
    return sc, res, d


def test_scan4_matches_reference_script(dev, fx):
    sc, res, d = _run_scan(fx, 4)
    head = d["data_pcd"][:len(fx["s4_data_head"])].cpu().numpy()
    assert np.array_equal(_bits(head), _bits(fx["s4_data_head"]))                        # the shuffled, prepared cloud
    for side in ("d2s", "s2d"):
        got, want = d["dist_" + side].cpu().numpy(), fx["s4_dist_" + side]
        near = want < 20
        np.testing.assert_array_equal(got[near], want[near])
        assert (got[~near] >= 20).all()
        _check_colors(fx, f"s4_color_{side}", *clouds.error_colors(d["dist_" + side], 20, 10))
    np.testing.assert_allclose(res, fx["s4_means"], rtol=1e-12)
    assert 'scan{:0>3} {:.2f} {:.2f} {:.2f}'.format(4, *res) == str(fx["s4_row"])
    # the oracle on the same order: the whole prepared cloud, not the stored head only
    perm = np.arange(len(sc["data_pcd"]))
    np.random.default_rng(int(fx["s4_shuffle_seed"])).shuffle(perm)
    assert np.array_equal(_bits(d["data_pcd"].cpu().numpy()), _bits(borc.prepare(sc["data_pcd"][perm], sc["relative_scale"])))
    assert np.array_equal(_bits(d["gt_pcd"].cpu().numpy()), _bits(borc.prepare(sc["gt_pcd"], sc["relative_scale"])))


def test_scan5_matches_reference_script(dev, fx):
    """The scan that goes through scale_mat_0: the reference's product is a BLAS dot, hence tolerances instead of bits."""
    sc, res, d = _run_scan(fx, 5)
    head = d["data_pcd"][:len(fx["s5_data_head"])].cpu().numpy()
    np.testing.assert_allclose(head, fx["s5_data_head"], rtol=1e-13, atol=0)
    for side in ("d2s", "s2d"):
        got, want = d["dist_" + side].cpu().numpy(), fx["s5_dist_" + side]
        near = want < 20
        np.testing.assert_allclose(got[near], want[near], rtol=1e-12, atol=0)
        assert (got[~near] >= 20 * (1 - 1e-12)).all()
        rgb, u8 = clouds.error_colors(d["dist_" + side], 20, 10)
        np.testing.assert_array_equal(borc.color_classes(rgb.cpu().numpy()), fx[f"s5_color_{side}_classes"])
        _check_u8_classes(u8.cpu().numpy(), fx[f"s5_color_{side}_classes"])
    np.testing.assert_allclose(res, fx["s5_means"], rtol=1e-12)
    # scale_mat belongs to the prediction only
    assert np.array_equal(_bits(d["gt_pcd"].cpu().numpy()), _bits(borc.prepare(sc["gt_pcd"], sc["relative_scale"])))


def test_empty_clouds(dev):
    gt = np.random.default_rng(0).normal(0, 1, (50, 3))
    with pytest.raises(ValueError):
        eval_bmvs.evaluate_scan(np.zeros((0, 3)), gt, 0.01)
    far = gt + 1e4                                                                        # nothing within max_dist: nan, like numpy
    res = eval_bmvs.evaluate_scan(far, gt, 1.0, shuffle_rng=False)
    assert all(np.isnan(r) for r in res)


@pytest.fixture(scope="module")
def dtu_run(dev, fx):
    sc = synth.make_dtu_scan(int(fx["dtu_seed"]))
    res, d = eval_dtu.evaluate_scan(sc["data_pcd"], sc["stl"], sc["ObsMask"], sc["BB"], sc["Res"], sc["P"],
                                    shuffle_rng=np.random.default_rng(int(fx["dtu_shuffle_seed"])), visualize=float(fx["dtu_vis_dist"]))
    return sc, res, d


def test_dtu_error_clouds_match_reference_script(dtu_run, fx):
    sc, res, d = dtu_run
    np.testing.assert_allclose(res, fx["dtu_means"], rtol=1e-12)
    assert len(d["in_obs"]) == len(d["data_down"]) and len(d["above"]) == len(sc["stl"]) == len(d["stl"])
    assert int(d["in_obs"].ne(0).sum()) == len(d["dist_d2s"]) and int(d["above"].ne(0).sum()) == len(d["dist_s2d"])
    _check_colors(fx, "dtu_color_d2s", d["data_color"], d["data_color_u8"])
    _check_colors(fx, "dtu_color_s2d", d["stl_color"], d["stl_color_u8"])


def _write_ply(fn, pts):
    with open(fn, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\n"
                 "property double z\nend_header\n" % len(pts)).encode())
        np.ascontiguousarray(pts, "<f8").tofile(f)


def test_file_layout_and_command_line(dev, fx, tmp_path, capsys):
    from svs_hip.ply import read_points
    root, pred = tmp_path / "root" / "BlendedMVS", tmp_path / "pred"
    (root / "stl").mkdir(parents=True); pred.mkdir()
    scans = {}
    for scan in (4, 5):
        sc = scans[scan] = synth_bmvs.make_bmvs_scan(int(fx[f"s{scan}_seed"]), scan)
        _write_ply(root / "stl" / f"scan{scan}_crop.ply", sc["gt_pcd"])
        _write_ply(root / "stl" / f"scan{scan}.ply", sc["gt_pcd"][::2])
        _write_ply(pred / f"mvsnet{scan:03}_l3.ply", sc["data_pcd"])
        if sc["scale_mat"] is not None:
            (root / f"scan{scan}").mkdir()
            np.savez(root / f"scan{scan}" / "cameras.npz", scale_mat_0=sc["scale_mat"], scale_mat_1=sc["scale_mat"])
    res = eval_bmvs.main(["--data_dir_root", str(tmp_path / "root"), "--datadir", str(pred), "-ve"])       # all nine: seven are missing
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0] == "ply_name, chamfer(mm)" and len(lines) == 3 and sorted(res) == [4, 5]
    for line, scan in zip(lines[1:], (4, 5)):
        name, *vals = line.split()
        assert name == f"scan{scan:03}" and len(vals) == 3
        # the command line shuffles unseeded like the script: the order moves the means in their last digits only
        np.testing.assert_allclose([float(v) for v in vals], fx[f"s{scan}_means"], rtol=0.02)
        np.testing.assert_allclose(res[scan], fx[f"s{scan}_means"], rtol=0.02)
        for side, n in (("d2s", int(fx[f"s{scan}_n_data"])), ("s2d", len(scans[scan]["gt_pcd"]))):
            pts, rgb = read_points(str(pred / "result" / f"{scan}_{side}.ply"))
            assert pts.shape == (n, 3) and rgb.shape == (n, 3) and rgb.dtype == np.uint8
            _check_u8_classes(rgb, fx[f"s{scan}_color_{side}_classes"])
        gt, _ = read_points(str(pred / "result" / f"{scan}_s2d.ply"))                 # the cloud the search saw
        assert np.array_equal(_bits(gt), _bits(borc.prepare(scans[scan]["gt_pcd"], scans[scan]["relative_scale"])))
    # --no_crop reads scan4.ply (half the ground truth here); the result is a tuple of three again
    r = eval_bmvs.evaluate_scan_files(4, str(pred), str(tmp_path / "root"), no_crop=True, visualize_error=True)
    assert len(r) == 3 and read_points(str(pred / "result" / "4_s2d.ply"))[0].shape == ((len(scans[4]["gt_pcd"]) + 1) // 2, 3)


def test_dtu_command_line_writes_error_clouds(dev, dtu_run, fx, tmp_path, capsys):
    from scipy.io import savemat
    from svs_hip.ply import read_points
    sc, _, d = dtu_run
    scan = 24
    ds = tmp_path / "root" / "DTU" / "DTU_MVS_Data"
    (ds / "ObsMask").mkdir(parents=True); (ds / "Points" / "stl").mkdir(parents=True); (tmp_path / "pred").mkdir()
    savemat(str(ds / "ObsMask" / f"ObsMask{scan}_10.mat"), dict(ObsMask=sc["ObsMask"], BB=sc["BB"], Res=sc["Res"]))
    savemat(str(ds / "ObsMask" / f"Plane{scan}.mat"), dict(P=sc["P"]))
    _write_ply(ds / "Points" / "stl" / f"stl{scan:03}_total.ply", sc["stl"])
    _write_ply(tmp_path / "pred" / f"mvsnet{scan:03}_l3.ply", sc["data_pcd"])
    res = eval_dtu.main(["--data_dir_root", str(tmp_path / "root"), "--datadir", str(tmp_path / "pred"), "--scan", str(scan), "-ve"])
    np.testing.assert_allclose(res, fx["dtu_means"], rtol=0.02)
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0] == "ply_name, accuracy(mm), completeness(mm), overall(mm)" and lines[1].startswith("scan024 ") and \
        lines[2].startswith("mean_err ")
    stl, rgb = read_points(str(tmp_path / "pred" / "result" / f"vis_{scan:03}_s2d.ply"))
    np.testing.assert_array_equal(stl, sc["stl"])
    np.testing.assert_array_equal(borc.color_classes(rgb)[0], fx["dtu_color_s2d_classes"][0])      # the plane side: order-free
    pts, rgb = read_points(str(tmp_path / "pred" / "result" / f"vis_{scan:03}_d2s.ply"))
    assert pts.shape == rgb.shape and abs(len(pts) - int(fx["dtu_color_d2s_n"])) <= 0.02 * int(fx["dtu_color_d2s_n"])
