"""svs_hip.meshsimplify without a GPU: the float64 oracle (tests/meshsimplify_oracle.py) on the meshes the GPU tests use, the
entries' argument checks with dummy pointers, the build list, the command line and the runner's key."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import meshsimplify_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results():
    return {name: so.cluster(*so.case(name)) for name in so.CASES}


def _ranks(r):
    return np.bincount(r["info"] & 3, minlength=4).tolist()


def test_oracle_on_the_sphere(results):
    for name, cells, faces in (("sphere_0.5", 67, 130), ("sphere_0.3", 170, 336)):
        r = results[name]
        assert r["n_cells"] == cells and len(r["faces"]) == faces and r["clear"].all()
        assert _ranks(r) == [0, 0, 0, cells] and not (r["info"] >> 2).any()
        assert so.euler(cells, r["faces"]) == 2 and so.closed_oriented_manifold(r["faces"])
        # a sphere's planes meet near its surface: every output vertex is within a twentieth of a cell of it
        dist = np.abs(np.linalg.norm(r["verts"].astype(np.float64) - [0.13, 0.21, 0.34], axis=1) - 1.0)
        print(f"{name}: worst distance to the sphere {dist.max():.4f}")
        assert dist.max() < 0.05 * float(name[7:]) + 0.01
    one = results["sphere_one_cell"]
    assert one["n_cells"] == 1 and len(one["faces"]) == 0 and one["clear"].all()


def test_oracle_on_the_torus_cube_plane_and_wedge(results):
    t = results["torus_0.4"]
    assert t["n_cells"] == 131 and len(t["faces"]) == 262 and so.euler(131, t["faces"]) == 0 and so.closed_oriented_manifold(t["faces"])
    assert 0.75 < t["clear"].mean() < 0.85                      # used for integers only
    c = results["cube_0.5"]
    assert c["clear"].all() and all(n > 0 for n in _ranks(c)[1:]) and _ranks(c)[0] == 0 and _ranks(c)[3] == 8
    # corners, edges and faces land on the cube: a rank-3 cell gives the corner itself
    corners = c["verts"][(c["info"] & 3) == 3].astype(np.float64)
    assert np.abs(np.abs(corners) - 1.0).max() < 1e-6
    p = results["plane_0.45"]
    assert p["clear"].all() and _ranks(p) == [0, p["n_cells"], 0, 0] and np.abs(p["err"]).max() < 1e-12
    w = results["wedge_2.5"]
    assert w["n_cells"] == 1 and w["clear"].all() and w["info"].tolist() == [2 | 4] and len(w["faces"]) == 0
    w = results["wedge_1.0"]
    assert w["clear"].all() and (w["info"] == 1).all()


def test_oracle_rules_on_small_cases():
    # the order of the sums: one cell of 65 pairs = a segment of 64 and one of 1
    v, f, h, o = so.case("fan_65")
    r = so.cluster(v, f, h, o)
    hub = r["vert_cell"][0]
    assert (r["vert_cell"] == hub).sum() == 1 and r["clear"].all() and r["n_cells"] == 3
    assert np.abs(r["verts"][hub].astype(np.float64) - [0, 0, 2.0]).max() < 1e-6     # the apex of the cone
    # a face with two corners in one cell counts twice there; duplicates keep the lowest index, whatever the orientation
    assert len(r["faces"]) == 1 and r["source"][0] == min(r["source"])
    both = np.concatenate([f, f[:, ::-1]])
    assert np.array_equal(so.cluster(v, both, h, o)["faces"], r["faces"])
    # the slab: the second sheet repeats the first
    (sv, sf), n1 = so.slab(0.5)
    s = so.cluster(sv, sf, 0.5, np.zeros(3))
    assert (s["source"] < n1).all() and np.array_equal(s["faces"], so.cluster(sv[:len(sv) // 2], sf[:n1], 0.5, np.zeros(3))["faces"])
    # bad input is ignored: the valid faces alone give the same
    v, f, h, o = so.case("sphere_0.5")
    bad_v = np.concatenate([v, [[np.nan, 0, 0], [np.inf, 0, 0], [0.5, 0.5, 0.5]]]).astype(np.float32)
    n = len(v)
    bad_f = np.concatenate([[[0, 1, n]], f[:100], [[0, n + 1, 2], [0, 1, n + 3], [-1, 0, 1], [5, 5, 9], [0, 0, 0]], f[100:]]).astype(np.int32)
    a, b = so.cluster(bad_v, bad_f, h, o), so.cluster(v, f, h, o)
    assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(a["verts"], b["verts"]) and (a["vert_cell"][n:] == -1).all()
    empty = so.cluster(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0)
    assert empty["n_cells"] == 0 and empty["faces"].shape == (0, 3)
    # colours: the rounded integer mean over the pairs
    col = np.random.default_rng(0).integers(0, 256, (len(v), 3)).astype(np.uint8)
    c = so.cluster(v, f, h, o, colors=col)
    r0 = np.nonzero(c["vert_cell"][f] == 0)
    total, count = col[f[r0]].astype(np.int64).sum(0), len(r0[0])
    assert np.array_equal(c["colors"][0], (2 * total + count) // (2 * count))
    # the threshold is strict: an eigenvalue equal to tol * the largest is not kept
    tv, tf, th, to_, tol = so.threshold_case()
    t = so.cluster(tv, tf, th, to_, tol=tol)
    assert t["n_cells"] == 1 and t["trace"][0] == 0.9375 and (t["info"][0] & 3) == 1 and not t["clear"][0]
    assert (so.cluster(tv, tf, th, to_, tol=0.2499)["info"][0] & 3) == 2
    # the search
    best, tried = so.bisect(lambda x: so.count_faces(v, f, x), 0.1, 3.0, 200, tries=8)
    assert len(tried) == 8 and best == min(x for x, k in tried if k <= 200) and so.count_faces(v, f, best) <= 200


def _build():
    spec = importlib.util.spec_from_file_location("svs_build", os.path.join(ROOT, "s-volsdf_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build


def test_symbols_unit_and_command_line():
    from svs_hip import lib, meshsimplify
    for name, nargs in (("svs_mesh_cluster_workspace_bytes", 2), ("svs_mesh_cluster_cells", 10), ("svs_mesh_cluster_solve", 16),
                        ("svs_mesh_cluster_faces_count", 11), ("svs_mesh_cluster_faces_emit", 7)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
    assert lib.ABI_VERSION == 101
    assert lib.SIGNATURES["svs_mesh_cluster_cells"][1][8] is ctypes.POINTER(ctypes.c_int)
    assert _build().UNITS["svs_meshsimplify.hip"] == ["-ffp-contract=off"]
    base = ["--ply", "in.ply", "--ply-out", "out.ply"]
    a = meshsimplify.parse_args(base + ["--cell", "0.5"])
    assert a.cell == 0.5 and a.faces is None and a.ratio is None and a.tol == 1e-3 and not a.report and a.tries == 16
    a = meshsimplify.parse_args(base + ["--faces", "1000", "--tol", "0.01", "--report"])
    assert a.faces == 1000 and a.cell is None and a.tol == 0.01 and a.report
    assert meshsimplify.parse_args(base + ["--ratio", "0.1"]).ratio == 0.1
    for bad in ([], ["--cell", "0.5", "--faces", "10"], ["--cell", "0.5", "--ratio", "0.5"], ["--faces", "10", "--ratio", "0.5"],
                ["--cell", "0"], ["--cell", "-1"], ["--ratio", "1.0"], ["--ratio", "0"], ["--faces", "-1"], ["--cell", "1", "--tol", "1"],
                ["--cell", "1", "--tol", "0"], ["--cell", "1", "--tries", "0"]):
        with pytest.raises(SystemExit):
            meshsimplify.parse_args(base + bad)
    with pytest.raises(SystemExit):
        meshsimplify.parse_args(["--ply", "in.ply", "--cell", "1"])              # --ply-out is required
    v, f = np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32)
    for kw in (dict(), dict(cell=1.0, ratio=0.5), dict(target_faces=3, ratio=0.5), dict(cell=1.0, target_faces=3, ratio=0.5)):
        with pytest.raises(ValueError, match="exactly one"):
            meshsimplify.simplify(v, f, **kw)
    assert meshsimplify.bisect(lambda h: 10 if h < 1 else 2, 0.1, 10.0, 5, tries=6) == so.bisect(lambda h: 10 if h < 1 else 2, 0.1, 10.0, 5, tries=6)


def test_runner_carries_the_key(tmp_path):
    from svs_hip import run
    args = run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", "+tsdf_simplify=0.25"])
    assert args["tsdf_simplify"] == 0.25 and run.check_tsdf_simplify(args) == 0.25
    assert "tsdf_simplify" not in run.default_args() and run.check_tsdf_simplify(run.default_args()) is None
    with pytest.raises(KeyError):
        run.apply_overrides(run.default_args(), ["tsdf_simplify=0.25"])
    alone = run.apply_overrides(run.default_args(), ["+tsdf_simplify=0.25", f"outdir={tmp_path / 'out'}"])
    with pytest.raises(ValueError, match="tsdf_simplify.*tsdf_voxel"):
        run.run_help(alone, select_device=False)
    assert not os.path.exists(tmp_path / "out")                                   # refused before anything is made
    for bad in ("1.5", "0", "-0.1", "1", "true", "half"):
        with pytest.raises(ValueError, match="tsdf_simplify"):
            run.check_tsdf_simplify(run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", f"+tsdf_simplify={bad}"]))
    assert run.tsdf_simple_ply_name("o", "scan106") == os.path.join("o", "tsdf_simple", "mvsnet106_l3.ply")


def test_argument_errors_name_the_entry():
    """the checks come before any device work: no GPU needed, dummy pointers are never dereferenced"""
    from svs_hip import lib
    _build().build(verbose=False)
    L = lib.load()
    d = ctypes.c_void_p(64)
    ESHAPE, EINVAL = -2, -1
    org = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    nan_org = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    n_cells = ctypes.c_int(7)
    msg = L.svs_last_error_string

    def cells(nv=5, nf=4, verts=d, faces=d, origin=org, h=0.5, ws=d, vert_cell=d, out=ctypes.byref(n_cells)):
        return L.svs_mesh_cluster_cells(verts, nv, faces, nf, origin, h, ws, vert_cell, out, None)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nf=(2 ** 31 - 1) // 3 + 1)):
        assert cells(**kw) == ESHAPE and msg().startswith(b"svs_mesh_cluster_cells: "), kw
    for kw in (dict(verts=None), dict(faces=None), dict(origin=None), dict(ws=None), dict(vert_cell=None), dict(out=None), dict(h=0.0),
               dict(h=-1.0), dict(h=float("inf")), dict(h=float("nan")), dict(origin=nan_org)):
        assert cells(**kw) == EINVAL and msg().startswith(b"svs_mesh_cluster_cells: "), kw
    assert cells(nv=0, nf=0) == 0 and n_cells.value == 0                          # an empty mesh is not an error

    def solve(nv=5, nf=4, verts=d, faces=d, colors=None, origin=org, h=0.5, tol=1e-3, vert_cell=d, nc=3, ws=d, out=d, out_colors=None,
              info=d, err=d):
        return L.svs_mesh_cluster_solve(verts, nv, faces, nf, colors, origin, h, tol, vert_cell, nc, ws, out, out_colors, info, err, None)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nc=-1), dict(nc=6), dict(nv=1 << 22, nc=(1 << 21) + 1)):
        assert solve(**kw) == ESHAPE and msg().startswith(b"svs_mesh_cluster_solve: "), kw
    for kw in (dict(verts=None), dict(faces=None), dict(vert_cell=None), dict(ws=None), dict(out=None), dict(info=None), dict(err=None),
               dict(colors=d), dict(out_colors=d), dict(origin=None), dict(h=0.0), dict(h=float("nan")), dict(tol=0.0), dict(tol=1.0),
               dict(tol=-0.5), dict(tol=float("nan"))):
        assert solve(**kw) == EINVAL and msg().startswith(b"svs_mesh_cluster_solve: "), kw
    assert solve(nc=0) == 0 and solve(nv=0, nf=0, nc=0) == 0

    def count(nv=5, nf=4, verts=d, faces=d, vert_cell=d, nc=3, ws=d, keep=d, offsets=d, out=d):
        return L.svs_mesh_cluster_faces_count(verts, nv, faces, nf, vert_cell, nc, ws, keep, offsets, out, None)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nc=-1), dict(nc=(1 << 21) + 1)):
        assert count(**kw) == ESHAPE and msg().startswith(b"svs_mesh_cluster_faces_count: "), kw
    assert b"21" in msg()
    for kw in (dict(verts=None), dict(faces=None), dict(vert_cell=None), dict(ws=None), dict(keep=None), dict(offsets=None), dict(out=None)):
        assert count(**kw) == EINVAL and msg().startswith(b"svs_mesh_cluster_faces_count: "), kw

    def emit(nf=4, faces=d, vert_cell=d, keep=d, offsets=d, out=d):
        return L.svs_mesh_cluster_faces_emit(faces, nf, vert_cell, keep, offsets, out, None)
    assert emit(nf=-1) == ESHAPE and msg().startswith(b"svs_mesh_cluster_faces_emit: ")
    for kw in (dict(faces=None), dict(vert_cell=None), dict(keep=None), dict(offsets=None), dict(out=None)):
        assert emit(**kw) == EINVAL and msg().startswith(b"svs_mesh_cluster_faces_emit: "), kw
    assert emit(nf=0) == 0
    assert L.svs_mesh_cluster_workspace_bytes(1000, 2000) > L.svs_mesh_cluster_workspace_bytes(10, 20) > 0
    assert L.svs_mesh_cluster_workspace_bytes(-1, -1) == L.svs_mesh_cluster_workspace_bytes(0, 0)
