"""csrc/svs_cloudknn.hip on the GPU against tests/cloudclean_oracle.py: k nearest neighbours (bit for bit), the outlier
statistics and mask, the oriented normals, and `svs_hip.cloudclean` end to end on a toy scan folder and through the runner.

Neighbours are compared exactly: the kernel and the oracle evaluate the same float64 expression and order by (d2, index).
The oracle lists 32 neighbours per query once per cloud; a smaller k is a prefix of that list."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest
import torch

import cloudclean_oracle as co
import tsdf_oracle as to

pytestmark = pytest.mark.gpu
FAR = 10.0                                                   # a radius that cuts nothing in the unit-size clouds below


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def H(t):
    return t.cpu().numpy()


def same(got, want):
    """equal element for element, infinities included"""
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


@functools.lru_cache(maxsize=None)
def random_case(n):
    """the cloud, queries that reach outside its box, and the oracle's 32 neighbours: of the cloud against itself with and
    without the point itself, and of the queries"""
    ref, query = co.random_cloud(n, 10 + n), co.random_cloud(min(n, 300) + 3, 20 + n, scale=1.3)
    return dict(ref=ref, query=query, self_excl=co.knn(ref, ref, 32, exclude_same_index=True), self_incl=co.knn(ref, ref, 32),
                outside=co.knn(ref, query, 32))


def check_prefix(got, want32, k, what):
    dist, idx, mean = (H(t) for t in got)
    assert same(dist, want32[0][:, :k]) and same(idx, want32[1][:, :k]), what
    assert same(mean, co.row_means(want32[0][:, :k])), what


# ---- neighbours ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8, 20, 32])
@pytest.mark.parametrize("n", [1, 5, 257, 2049])
def test_knn_is_the_oracles(n, k):
    from svs_hip import clouds
    c = random_case(n)
    ref = G(c["ref"])
    check_prefix(clouds.knn(ref, ref, k, FAR, exclude_same_index=True, return_mean=True), c["self_excl"], k, "self, excluded")
    check_prefix(clouds.knn(ref, ref, k, FAR, return_mean=True), c["self_incl"], k, "self")
    check_prefix(clouds.knn(ref, c["query"], k, FAR, return_mean=True), c["outside"], k, "queries outside the box")
    if n < k:                                                # the fill: slots that do not exist
        dist, idx = clouds.knn(ref, ref, k, FAR)
        assert np.isinf(H(dist)[:, n:]).all() and (H(idx)[:, n:] == -1).all() and (H(idx)[:, :n] >= 0).all()


@pytest.mark.parametrize("k", [1, 7, 32])
def test_knn_ties_go_to_the_lower_index(k):
    from svs_hip import clouds
    pts = co.lattice_cloud()
    for excl in (False, True):
        want = co.knn(pts, pts, k, exclude_same_index=excl)
        if k > 1:
            assert (np.diff(want[0], axis=1) == 0).mean() > 0.3                   # equal distances all over
        got = clouds.knn(G(pts), G(pts), k, FAR, exclude_same_index=excl, return_mean=True)      # two uploads: the plain walk
        check_prefix(got, want, k, excl)
        p = G(pts)
        check_prefix(clouds.knn(p, p, k, FAR, exclude_same_index=excl, return_mean=True), want, k, excl)     # the sorted walk
    # cells of one lattice step: walls between equal candidates
    check_prefix(clouds.knn(p, p, k, FAR, exclude_same_index=True, return_mean=True, cell=1.0), want, k, "cell 1")


def test_knn_does_not_depend_on_the_cell():
    """the 8 neighbours lie about 0.4 away: one cell holds everything, or the answer needs one, three and more rings"""
    from svs_hip import clouds
    c = random_case(257)
    ref = G(c["ref"])
    kth = np.median(c["self_excl"][0][:, 7])
    assert 0.1 < kth < 0.5
    for cell in (8.0, 0.5, 0.12, 0.05):
        check_prefix(clouds.knn(ref, ref, 8, FAR, exclude_same_index=True, return_mean=True, cell=cell), c["self_excl"], 8, cell)
        check_prefix(clouds.knn(ref, c["query"], 8, FAR, return_mean=True, cell=cell), c["outside"], 8, cell)


def test_knn_radius_cuts_lists_short():
    from svs_hip import clouds
    c = random_case(257)
    ref = G(c["ref"])
    for radius in (float(np.median(c["self_excl"][0][:, 4])), float(c["self_excl"][0][:, 0].min()), float(c["self_excl"][0][3, 2])):
        want = co.knn(c["ref"], c["ref"], 20, radius, exclude_same_index=True)
        got = clouds.knn(ref, ref, 20, radius, exclude_same_index=True, return_mean=True)
        check_prefix(got, want, 20, radius)
        d = H(got[0])
        assert (d[np.isfinite(d)] < radius).all()                                  # strictly closer
        assert same(H(clouds.knn_mean(ref, 20, radius)), want[2])                  # the scores alone
    assert np.isinf(want[0][3, 2]) and np.isfinite(want[0][3, 1])                  # a neighbour AT the radius is not listed
    assert np.isinf(co.knn(c["ref"], c["ref"], 20, float(c["self_excl"][0][:, 0].min()), exclude_same_index=True)[2]).all()


def test_knn_one_neighbour_is_nearest_neighbor():
    from svs_hip import clouds
    c = random_case(2049)
    ref, query = G(c["ref"]), G(c["query"])
    dist, idx = clouds.knn(ref, query, 1, FAR)
    d1, i1 = clouds.nearest_neighbor(ref, query, FAR, return_index=True)
    assert torch.equal(dist[:, 0].view(torch.int64), d1.view(torch.int64)) and torch.equal(idx[:, 0], i1)
    lat = G(co.lattice_cloud())
    dist, idx = clouds.knn(lat, lat, 1, FAR)
    d1, i1 = clouds.nearest_neighbor(lat, lat, FAR, return_index=True)
    assert torch.equal(dist[:, 0], d1) and torch.equal(idx[:, 0], i1)


def test_knn_chunks_and_repeats():
    from svs_hip import clouds
    c = random_case(257)
    ref = G(c["ref"])
    check_prefix(clouds.knn(ref, ref, 20, FAR, exclude_same_index=True, return_mean=True, chunk=100), c["self_excl"], 20, "chunks")
    check_prefix(clouds.knn(ref, c["query"], 20, FAR, return_mean=True, chunk=100), c["outside"], 20, "chunks")
    assert same(H(clouds.knn_mean(ref, 20, FAR, chunk=100)), co.row_means(c["self_excl"][0][:, :20]))
    big = G(random_case(2049)["ref"])
    first = clouds.knn(big, big, 32, FAR, exclude_same_index=True, return_mean=True)
    again = clouds.knn(big, big, 32, FAR, exclude_same_index=True, return_mean=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    with pytest.raises(ValueError):
        clouds.knn(ref, ref, 33, FAR)
    with pytest.raises(ValueError):
        clouds.knn(ref, ref, 4, 0.0)
    empty = clouds.knn(ref, ref[:0], 4, FAR, return_mean=True)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 4) and empty[2].shape == (0,)


# ---- outliers --------------------------------------------------------------------------------------------------------------
OUT_K, OUT_RADIUS, OUT_RATIO = 20, 0.6, 2.0


@functools.lru_cache(maxsize=None)
def floater_case():
    pts, planted = co.surface_with_floaters(1500, 12, seed=0)
    keep, scores, stats = co.clean_scores(pts, OUT_K, OUT_RADIUS, OUT_RATIO)
    return dict(pts=pts, planted=planted, keep=keep, scores=scores, stats=stats)


def test_outlier_stats_are_the_oracles():
    from svs_hip import clouds
    c = floater_case()
    for scores in (c["scores"], c["scores"][:1], np.array([np.inf, 2.5, np.nan]), np.array([np.inf]), np.zeros(0)):       # (n = 0: no call)
        got = clouds.outlier_stats(G(scores))
        count, mean, std = co.outlier_stats(scores)
        n = max(len(scores), 1)
        print(f"n {len(scores)}: count {got['count']} / {count}, mean {got['mean']!r} / {mean!r}, std {got['std']!r} / {std!r}")
        assert got["count"] == count
        assert abs(got["mean"] - mean) <= 4 * n * 2.0 ** -53 * abs(mean) and abs(got["std"] - std) <= 4 * n * 2.0 ** -53 * abs(std)
    assert not np.isfinite(c["scores"]).all()                                      # the planted points without neighbours


def test_outlier_mask_is_the_oracles():
    from svs_hip import clouds
    c = floater_case()
    fin = np.isfinite(c["scores"])
    thr = c["stats"]["threshold"]
    assert (np.abs(c["scores"][fin] - thr) > 1e-9 * thr).all()                     # no score at the threshold: nothing to excuse
    keep, stats = clouds.outlier_mask(G(c["pts"]), OUT_K, OUT_RATIO, OUT_RADIUS)
    assert keep.dtype == torch.bool and same(H(keep), c["keep"])
    assert stats["count"] == c["stats"]["count"] and abs(stats["threshold"] - thr) <= 1e-11 * thr
    assert same(H(clouds.threshold_mask(G(c["scores"]), thr)), c["keep"])
    edge = np.array([thr, np.nextafter(thr, 1), np.inf, -np.inf, np.nan, 0.0])
    assert same(H(clouds.threshold_mask(G(edge), thr)), np.array([True, False, False, False, False, True]))


def test_planted_points_are_dropped():
    from svs_hip import clouds
    c = floater_case()
    keep = H(clouds.outlier_mask(G(c["pts"]), OUT_K, OUT_RATIO, OUT_RADIUS)[0])
    assert not keep[c["planted"]].any() and (~keep[~c["planted"]]).mean() <= 0.05
    assert not c["keep"][c["planted"]].any() and (~c["keep"][~c["planted"]]).mean() <= 0.05        # the recipe's, not the kernel's
    keep = H(clouds.outlier_mask(G(c["pts"]))[0])                                  # the default radius: four grid cells
    assert not keep[c["planted"]].any() and (~keep[~c["planted"]]).mean() <= 0.05


# ---- normals ---------------------------------------------------------------------------------------------------------------
NRM_K, NRM_RADIUS = 16, 0.5
CENTRES = np.array([[4.0, 0.3, 0.2], [-0.5, 3.5, 1.0], [0.2, -0.4, -3.8]])


@functools.lru_cache(maxsize=None)
def normal_case(name):
    pts = co.noisy_sphere(2000, 0) if name == "sphere" else co.noisy_plane(2000, 1)
    _, idx, _ = co.knn(pts, pts, NRM_K, NRM_RADIUS, exclude_same_index=True)
    view = np.random.default_rng(5).integers(0, 3, len(pts)).astype(np.int32)
    return dict(pts=pts, idx=idx, view=view, plain=co.normals(pts, idx, True), by_view=co.normals(pts, idx, True, view, CENTRES),
                nearest=co.normals(pts, idx, True, None, CENTRES))


@pytest.mark.parametrize("name", ["sphere", "plane"])
def test_normals_are_the_oracles(name):
    from svs_hip import clouds
    c = normal_case(name)
    pts = G(c["pts"])
    _, idx = clouds.knn(pts, pts, NRM_K, NRM_RADIUS, exclude_same_index=True)
    assert same(H(idx), c["idx"])
    lam = c["plain"][2]
    clear = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-3
    assert clear.mean() >= 0.95
    for mode, kw in (("plain", dict()), ("by_view", dict(view_index=c["view"], centres=CENTRES)), ("nearest", dict(centres=CENTRES))):
        want_n, want_c, _, facing = c[mode]
        n, curv = clouds.normals_from_neighbors(pts, idx, **kw)
        n, curv = H(n), H(curv)
        assert n.dtype == np.float32 and curv.dtype == np.float32
        ang = co.angle(n, want_n)
        print(f"{name} {mode}: largest angle {ang[clear].max():.3e} rad, curvature off by {np.abs(curv - want_c).max():.3e}")
        # float32 output: a unit vector's components are rounded to 2^-24 relative, an angle of at most 2^-24 sqrt(3) ~ 1e-7
        assert (ang[clear] <= 1e-6).all()
        assert (np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1) <= 1e-6).all()
        assert (np.abs(curv - want_c) <= 1e-6).all()
        if mode != "plain":
            sure = clear & (np.abs(facing) > 1e-9)
            assert sure.mean() > 0.9 and (co.angle(n[sure], want_n[sure], signed=True) <= 1e-6).all()
            C = CENTRES[c["view"]] if mode == "by_view" else CENTRES[np.argmin(((c["pts"][:, None] - CENTRES[None]) ** 2).sum(-1), 1)]
            assert ((n[sure] * (C - c["pts"])[sure]).sum(1) > 0).all()
    # the whole function: its own neighbour search
    n2, curv2 = clouds.estimate_normals(pts, NRM_K, NRM_RADIUS, view_index=c["view"], centres=CENTRES)
    n1, curv1 = clouds.normals_from_neighbors(pts, idx, view_index=c["view"], centres=CENTRES)
    assert torch.equal(n1, n2) and torch.equal(curv1, curv2)


def test_normals_need_three_points():
    from svs_hip import clouds
    two = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    n, curv = clouds.estimate_normals(two, 16, FAR)
    assert not H(n).any() and not H(curv).any()
    # a radius that leaves some points with fewer than two neighbours
    c = normal_case("sphere")
    radius = float(np.sort(co.knn(c["pts"], c["pts"], 2, exclude_same_index=True)[0][:, 1])[1000])
    want_idx = co.knn(c["pts"], c["pts"], NRM_K, radius, exclude_same_index=True)[1]
    few = (want_idx >= 0).sum(1) < 2
    assert 0.2 < few.mean() < 0.8
    n, curv = clouds.estimate_normals(c["pts"], NRM_K, radius)
    n, curv = H(n), H(curv)
    assert not n[few].any() and not curv[few].any()
    assert (np.abs(np.linalg.norm(n[~few].astype(np.float64), axis=1) - 1) <= 1e-6).all()
    with pytest.raises(ValueError):
        clouds.normals_from_neighbors(c["pts"], want_idx, view_index=c["view"])


# ---- end to end ------------------------------------------------------------------------------------------------------------
VIEW_IDS = (25, 22, 28)                                      # the runner's training views of a DTU scan
NEAR_EYES = ((2.03, 0.31, 0.42), (1.9, 0.62, 0.5), (1.95, 0.0, 0.28))


@pytest.fixture(scope="module")
def scan_folder(tmp_path_factory):
    """{root}/scan106 with cams/, images/, depth_est/, confidence/ of three neighbouring views of a sphere, written by the
    project's own writers"""
    from datasets.data_io import save_pfm
    from helpers.utils import write_cam
    from PIL import Image
    root = tmp_path_factory.mktemp("fused")
    folder = root / "scan106"
    for sub in ("cams", "images", "depth_est", "confidence"):
        os.makedirs(folder / sub)
    sc = to.sphere_scene(eyes=NEAR_EYES)
    for vid, v in zip(VIEW_IDS, sc["views"]):
        cam = np.zeros((2, 4, 4))
        cam[0] = v["E"]
        cam[1, :3, :3] = v["K"]
        write_cam(str(folder / "cams" / f"{vid:08}_cam.txt"), cam, (1.0, 0.01, 192, 3.0))
        save_pfm(str(folder / "depth_est" / f"{vid:08}.pfm"), v["depth"])
        save_pfm(str(folder / "confidence" / f"{vid:08}.pfm"), (v["depth"] > 0).astype(np.float32))
        Image.fromarray(np.clip(v["img"] * 255, 0, 255).astype(np.uint8)).save(folder / "images" / f"{vid:08}.jpg", quality=95)
    return dict(root=root, folder=folder, scene=sc)


def test_clean_folder(scan_folder):
    from svs_hip import cloudclean, fusion, ply
    folder, sc = str(scan_folder["folder"]), scan_folder["scene"]
    out = str(scan_folder["root"] / "cleaned.ply")
    res = cloudclean.clean_folder(folder, folder, VIEW_IDS, out)
    stats = res["stats"]
    plain = fusion.filter_depth_folder(folder, folder, None, VIEW_IDS)[0]
    assert stats["points_in"] == len(plain) == len(res["keep"]) and stats["file"] == out
    assert 0.9 * len(plain) <= stats["points_kept"] == int(res["keep"].sum()) < len(plain) <= 4096
    assert list(stats["seconds"]) == list(cloudclean.PHASES) and all(v >= 0 for v in stats["seconds"].values())
    pts, col = ply.read_points(out)
    nrm = ply.read_point_normals(out)
    assert len(pts) == len(nrm) == len(col) == stats["points_kept"]
    assert np.array_equal(pts.astype(np.float32), plain[res["keep"]]) and np.array_equal(nrm, res["normals"])
    assert (np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1) <= 1e-6).all()
    # every normal faces its source camera: the centres the folder's camera files give; the float32 a normal is stored in
    # moves n . (c - p) by at most 2^-24 sqrt(3) |c - p|
    from helpers.utils import read_camera_parameters
    centres = np.stack([cloudclean.camera_centre(read_camera_parameters(os.path.join(folder, f"cams/{v:08}_cam.txt"))[1])
                        for v in VIEW_IDS])
    assert np.allclose(centres, NEAR_EYES, atol=1e-4)
    towards = centres[res["view_index"]] - pts
    assert ((nrm * towards).sum(1) >= -1e-6 * np.linalg.norm(towards, axis=1)).all()
    assert ((nrm * towards).sum(1) > 0).mean() > 0.99
    # and is the sphere's: the surface the depth maps sample
    radial = (pts - sc["centre"]) / np.linalg.norm(pts - sc["centre"], axis=1, keepdims=True)
    print(f"{len(pts)} of {len(plain)} points, median angle to the sphere's normal {np.median(co.angle(nrm, radial, True)):.3f} rad")
    assert np.median(co.angle(nrm, radial, signed=True)) < 0.2
    # the command, on the folder and on the plain cloud
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        again = cloudclean.main(["--scan-folder", folder, "--out-folder", folder, "--views", *map(str, VIEW_IDS), "--ply-out",
                                 str(scan_folder["root"] / "cmd.ply")])
    assert open(out, "rb").read() == open(scan_folder["root"] / "cmd.ply", "rb").read() and again["stats"]["points_kept"] == len(pts)
    assert f"points in {len(plain)}, points kept {len(pts)}, threshold " in text.getvalue() and "seconds: read " in text.getvalue()
    ply.write(str(scan_folder["root"] / "plain.ply"), plain, col[:1].repeat(len(plain), 0))
    with contextlib.redirect_stdout(io.StringIO()):
        bare = cloudclean.main(["--ply", str(scan_folder["root"] / "plain.ply"), "--ply-out", str(scan_folder["root"] / "bare.ply"),
                                "--no-outliers"])
    assert bare["stats"]["points_kept"] == len(plain) and bare["view_index"] is None
    assert np.median(co.angle(ply.read_point_normals(str(scan_folder["root"] / "bare.ply"))[res["keep"]], nrm)) < 0.05


def test_runner_switch(scan_folder):
    from svs_hip import ply, run
    root = scan_folder["root"] / "run"
    os.makedirs(root)
    os.symlink(scan_folder["folder"], root / "scan106")
    base = [f"outdir={root}", "filter_only=true", "eval_mask=false", "testlist=scan106"]
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base)
    assert "clean" not in res and "cloud clean" not in text.getvalue()
    assert sorted(os.listdir(root)) == ["mvsnet106_l3.ply", "scan106"]                # what the run writes today
    assert sorted(os.listdir(root / "scan106")) == ["cams", "confidence", "depth_est", "images", "mask"]
    cloud = open(root / "mvsnet106_l3.ply", "rb").read()
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base + ["+cloud_clean=true", "+cloud_k=12", "+cloud_std_ratio=1.5", "+cloud_normal_k=10"])
    assert sorted(os.listdir(root)) == ["clean", "mvsnet106_l3.ply", "scan106"] and os.listdir(root / "clean") == ["mvsnet106_l3.ply"]
    assert open(root / "mvsnet106_l3.ply", "rb").read() == cloud
    stats = res["clean"]["scan106"]
    assert (stats["k"], stats["std_ratio"]) == (12, 1.5) and text.getvalue().count("scan106 cloud clean seconds: read ") == 1
    pts, _ = ply.read_points(str(root / "clean" / "mvsnet106_l3.ply"))
    nrm = ply.read_point_normals(str(root / "clean" / "mvsnet106_l3.ply"))
    assert 0 < len(pts) == len(nrm) == stats["points_kept"] < stats["points_in"] == len(ply.read_points(str(root / "mvsnet106_l3.ply"))[0])
