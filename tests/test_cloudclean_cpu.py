"""CPU-side checks of the cloud cleaning: the oracle's neighbours against sklearn's kd-tree, the PLY writer's normals, the
argument checks of the four entry points of csrc/svs_cloudknn.hip (nothing is launched), the runner's keys, the command's
defaults and the build flags."""
import ctypes
import os

import numpy as np
import pytest

import cloudclean_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESHAPE = -1, -2


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def test_oracle_neighbours_are_sklearns():
    neighbors = pytest.importorskip("sklearn.neighbors")
    ref, query = co.random_cloud(700, 1), co.random_cloud(90, 2, scale=1.3)
    for k in (1, 8, 20):
        dist, idx, mean = co.knn(ref, query, k)
        want_d, want_i = neighbors.NearestNeighbors(n_neighbors=k, algorithm="kd_tree").fit(ref).kneighbors(query)
        assert len(np.unique(want_d)) == want_d.size                              # tie-free: the order is the distances' alone
        assert np.array_equal(dist, want_d) and np.array_equal(idx, want_i)       # to the last bit
        assert np.allclose(mean, want_d.mean(1), rtol=1e-14, atol=0)
    # a cloud against itself: sklearn lists the point first, the oracle leaves it out
    dist, idx, _ = co.knn(ref, ref, 5, exclude_same_index=True)
    want_d, want_i = neighbors.NearestNeighbors(n_neighbors=6, algorithm="kd_tree").fit(ref).kneighbors(ref)
    assert np.array_equal(want_i[:, 0], np.arange(len(ref)))
    assert np.array_equal(dist, want_d[:, 1:]) and np.array_equal(idx, want_i[:, 1:])


def test_oracle_fill_ties_radius_and_mean():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [3, 0, 0]], np.float64)
    dist, idx, mean = co.knn(pts, pts[:2], 7)
    assert np.array_equal(idx[0], [0, 3, 1, 2, 4, -1, -1]) and np.array_equal(dist[0, :5], [0, 0, 1, 1, 3])
    assert np.isinf(dist[:, 5:]).all() and np.array_equal(idx[1, :5], [1, 0, 3, 2, 4])
    assert mean[0] == (((0.0 + 0.0) + 1.0) + 1.0 + 3.0) / 5
    dist, idx, mean = co.knn(pts, pts, 3, max_radius=1.0, exclude_same_index=True)       # strictly closer than 1: the twin only
    assert np.array_equal(idx[0], [3, -1, -1]) and np.array_equal(idx[3], [0, -1, -1]) and (idx[[1, 2, 4]] == -1).all()
    assert np.array_equal(mean, [0, np.inf, np.inf, 0, np.inf])
    dist, idx, _ = co.knn(pts, pts[3:], 1, exclude_same_index=True, first_row=3)
    assert np.array_equal(idx[:, 0], [0, 1])
    c, m, s = co.outlier_stats([1.0, np.inf, 3.0, np.nan])
    assert (c, m) == (2, 2.0) and s == np.sqrt(2.0) and co.outlier_stats([5.0]) == (1, 5.0, 0.0) and co.outlier_stats([]) == (0, 0.0, 0.0)
    assert np.array_equal(co.outlier_mask([1.0, 2.0, np.inf, np.nan, 2.5], 2.0), [True, True, False, False, False])


def test_oracle_normals_on_exact_shapes():
    rng = np.random.default_rng(3)
    flat = np.concatenate([rng.uniform(-1, 1, (40, 2)), np.zeros((40, 1))], 1)
    _, idx, _ = co.knn(flat, flat, 8, exclude_same_index=True)
    centres = np.array([[0.0, 0.0, 5.0], [0.0, 0.0, -5.0]])
    n, curv, lam, facing = co.normals(flat, idx, True, np.ones(40, np.int32), centres)
    assert np.allclose(n, [0, 0, -1]) and np.allclose(curv, 0) and (np.abs(facing) > 0.9).all()
    n, _, _, _ = co.normals(flat + [0, 0, 1.0], idx, True, None, centres)                  # nearest centre: the upper one
    assert np.allclose(n, [0, 0, 1])
    n, curv, _, _ = co.normals(flat[:2], np.array([[1], [0]]), True)
    assert not n.any() and not curv.any()                                                  # two points: no plane
    assert np.allclose(co.angle([[1, 0, 0]], [[-1, 1e-9, 0]]), 1e-9) and np.allclose(co.angle([[1, 0, 0]], [[-1, 0, 0]], True), np.pi)


# ---- ply -------------------------------------------------------------------------------------------------------------------
def test_ply_normals_round_trip(tmp_path):
    from svs_hip import ply
    rng = np.random.default_rng(5)
    xyz = rng.normal(size=(7, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (7, 3), dtype=np.uint8)
    nrm = rng.normal(size=(7, 3)).astype(np.float32)
    f = str(tmp_path / "n.ply")
    ply.write(f, xyz, rgb, normals=nrm)
    raw = open(f, "rb").read()
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
            "property uchar blue\nend_header\n").encode("ascii")
    assert raw.startswith(head) and len(raw) == len(head) + 7 * 27
    assert raw[len(head):len(head) + 27] == xyz[0].tobytes() + nrm[0].tobytes() + rgb[0].tobytes()
    pts, col = ply.read_points(f)
    assert np.array_equal(pts, xyz.astype(np.float64)) and np.array_equal(col, rgb)
    assert np.array_equal(ply.read_point_normals(f), nrm) and ply.read_point_normals(f).dtype == np.float32
    # without the argument: the bytes of a call that does not name it, and no normals to read
    for kw in (dict(), dict(coords="double"), dict(faces=np.array([[0, 1, 2], [2, 3, 4]]))):
        a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
        ply.write(a, xyz, rgb, **kw)
        ply.write(b, xyz, rgb, normals=None, **kw)
        assert open(a, "rb").read() == open(b, "rb").read()
        assert ply.read_point_normals(a) is None
    old = ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
           "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode("ascii")
    ply.write(a, xyz, rgb)
    assert open(a, "rb").read() == old + b"".join(xyz[i].tobytes() + rgb[i].tobytes() for i in range(7))
    # normals without colours, double coordinates, a mesh with normals
    ply.write(f, xyz, normals=nrm, coords="double", faces=np.array([[0, 1, 2]]))
    assert np.array_equal(ply.read_point_normals(f), nrm) and ply.read_points(f)[1] is None
    assert np.array_equal(ply.read_mesh(f)[1], [[0, 1, 2]])
    with pytest.raises(ValueError, match="6 normals for 7 vertices"):
        ply.write(f, xyz, rgb, normals=nrm[:6])


# ---- the entry points' argument checks ----------------------------------------------------------------------------------------
def _lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("svs_build", os.path.join(ROOT, "s-volsdf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from svs_hip import lib
    return mod, lib.load()


def test_build_flags_and_version():
    mod, L = _lib()
    assert mod.UNITS["svs_cloudknn.hip"] == ["-ffp-contract=off"] and mod.UNITS["svs_cloud.hip"] == ["-ffp-contract=off"]
    assert L.svs_version() == 101
    assert L.svs_cloud_outlier_workspace_bytes() >= 2 * 8


def test_argument_errors_come_back_as_codes():
    _, L = _lib()
    d = ctypes.c_void_p(64)                                  # never dereferenced: the checks come first
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)

    def knn(ref=d, n_ref=5, query=d, n_query=5, origin=org, cell=1.0, k=4, max_radius=2.0, excl=0, ws=d, dist=d, idx=d, mean=d):
        return L.svs_cloud_knn(ref, n_ref, query, n_query, origin, cell, k, max_radius, excl, ws, dist, idx, mean, None)

    def named(rc, code, name):
        assert rc == code, (name, rc)
        assert L.svs_last_error_string().startswith(name.encode()), L.svs_last_error_string()

    for bad in (dict(ref=None), dict(query=None), dict(ws=None), dict(origin=None), dict(dist=None, idx=None, mean=None),
                dict(k=0), dict(k=33), dict(n_ref=-1), dict(n_query=-1), dict(excl=-1)):
        named(knn(**bad), EINVAL, "svs_cloud_knn")
    for bad in (dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(max_radius=0.0), dict(max_radius=1e9)):
        named(knn(**bad), ESHAPE, "svs_cloud_knn")
    assert knn(n_query=0) == 0                                # no queries: nothing to do, nothing launched
    named(L.svs_cloud_outlier_stats(None, 5, d, d, None), EINVAL, "svs_cloud_outlier_stats")
    named(L.svs_cloud_outlier_stats(d, 5, None, d, None), EINVAL, "svs_cloud_outlier_stats")
    named(L.svs_cloud_outlier_stats(d, 5, d, None, None), EINVAL, "svs_cloud_outlier_stats")
    named(L.svs_cloud_outlier_stats(d, -1, d, d, None), EINVAL, "svs_cloud_outlier_stats")
    named(L.svs_cloud_outlier_mask(None, 5, 1.0, d, None), EINVAL, "svs_cloud_outlier_mask")
    named(L.svs_cloud_outlier_mask(d, 5, 1.0, None, None), EINVAL, "svs_cloud_outlier_mask")
    named(L.svs_cloud_outlier_mask(d, -1, 1.0, d, None), EINVAL, "svs_cloud_outlier_mask")
    assert L.svs_cloud_outlier_mask(d, 0, 1.0, d, None) == 0

    def normals(pts=d, n=5, idx=d, k=8, view_index=None, centres=None, n_views=0, out=d):
        return L.svs_cloud_normals(pts, n, idx, k, 1, view_index, centres, n_views, out, d, None)

    for bad in (dict(pts=None), dict(idx=None), dict(out=None), dict(n=-1), dict(k=0), dict(k=33), dict(view_index=d),
                dict(centres=d, n_views=0)):
        named(normals(**bad), EINVAL, "svs_cloud_normals")
    assert normals(n=0) == 0 and normals(n=0, centres=d, n_views=3, view_index=d) == 0


# ---- runner and command -------------------------------------------------------------------------------------------------------
def test_runner_parses_the_cloud_keys():
    from svs_hip import run
    args = run.apply_overrides(run.default_args("dtu"), ["+cloud_clean=true", "+cloud_k=12", "+cloud_std_ratio=1.5",
                                                         "+cloud_normal_k=24"])
    assert args["cloud_clean"] is True and args["cloud_k"] == 12 and args["cloud_std_ratio"] == 1.5 and args["cloud_normal_k"] == 24
    assert "cloud_clean" not in run.default_args("dtu")       # off unless asked for
    with pytest.raises(KeyError, match="cloud_clean"):
        run.apply_overrides(run.default_args("dtu"), ["cloud_clean=true"])       # a new key takes the +
    assert run.clean_ply_name("exps_mvs", "scan106") == os.path.join("exps_mvs", "clean", "mvsnet106_l3.ply")
    assert callable(run.clean_clouds)


def test_command_defaults():
    from svs_hip import cloudclean
    a = cloudclean.parse_args(["--scan-folder", "S", "--out-folder", "O", "--views", "25", "22", "28", "--ply-out", "P"])
    assert (a.scan_folder, a.out_folder, a.views, a.ply_out, a.ply) == ("S", "O", [25, 22, 28], "P", None)
    assert (a.k, a.std_ratio, a.normal_k, a.max_radius) == (20, 2.0, 16, None)
    assert not a.no_outliers and not a.no_normals and a.data_dir_root is None and a.dataset is None
    b = cloudclean.parse_args(["--ply", "IN", "--ply-out", "P", "--k", "8", "--std-ratio", "1", "--normal-k", "10", "--max-radius",
                               "0.5", "--no-outliers", "--no-normals"])
    assert (b.ply, b.k, b.std_ratio, b.normal_k, b.max_radius, b.no_outliers, b.no_normals) == ("IN", 8, 1.0, 10, 0.5, True, True)
    for bad in (["--ply-out", "P"], ["--ply", "IN", "--views", "1", "--ply-out", "P"], ["--ply", "IN"],
                ["--ply", "IN", "--ply-out", "P", "--dataset", "DTU"]):
        with pytest.raises(SystemExit):
            cloudclean.parse_args(bad)
    E = np.eye(4)
    E[:3, :3] = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]]
    E[:3, 3] = [1, 2, 3]
    assert np.allclose(cloudclean.camera_centre(E), -E[:3, :3].T @ E[:3, 3]) and np.allclose(
        E[:3, :3] @ cloudclean.camera_centre(E) + E[:3, 3], 0)


def test_default_cell_rule():
    from svs_hip import clouds
    lo, hi = np.zeros(3), np.array([2.0, 1.0, 0.5])
    assert clouds.knn_cell(lo, hi, 10000, 1) == 2.0 / 100 and clouds.knn_cell(lo, hi, 10000, 16) == 2.0 * 4 / 100
    assert clouds.knn_cell(lo, hi, 10000, 16, max_radius=0.01) == 0.01
    assert clouds.knn_cell(lo, hi, 10 ** 14, 1) == 2.0 / (1 << 20)
