"""svs_hip.meshsmooth without a GPU: the float64 oracle (tests/meshsmooth_oracle.py) on the meshes the GPU tests use -- what
the two smoothers are for, stated as inequalities --, the rules on small cases, the entries' argument checks with dummy
pointers, the build list, the command line and the runner's key."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import meshsmooth_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _radius_error(v):
    return float(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0).mean())


def _extent(v):
    return float((v[:, :2].max(0) - v[:, :2].min(0)).astype(np.float64).mean())


# ---- what the smoothers are for ----------------------------------------------------------------------------------------------
def test_taubin_keeps_the_volume_of_a_noisy_sphere_and_a_laplacian_does_not():
    v, f = mo.icosphere(3)
    assert v.shape == (642, 3) and f.shape == (1280, 3) and mo.adjacency(v, f)["counts"] == [1920, 0, 0, 1280]
    noisy = mo.noisy(v, f, 0.1, seed=1)
    out = mo.taubin(noisy, f, iters=10)
    ratio = mo.volume(out, f) / mo.volume(v, f)
    print(f"sphere: mean | |x| - 1 | {_radius_error(noisy):.4f} -> {_radius_error(out):.4f}, volume ratio {ratio:.4f}")
    assert _radius_error(out) < 0.5 * _radius_error(noisy)
    assert abs(ratio - 1.0) < 0.02
    shrunk = mo.volume(mo.taubin(noisy, f, iters=10, mu=0.0), f) / mo.volume(v, f)
    print(f"sphere: volume ratio with mu = 0: {shrunk:.4f}")
    assert shrunk < 0.9


def test_denoise_keeps_the_edges_of_a_noisy_cube_and_taubin_does_not():
    v, f = mo.cube(8)
    assert v.shape == (386, 3) and f.shape == (768, 3) and mo.adjacency(v, f)["counts"] == [1152, 0, 0, 768]
    noisy = mo.noisy(v, f, 0.1 * 0.25 / mo.mean_edge(v, f), seed=2)            # 0.1 of the quad size
    before = mo.mean_angle(noisy, f, v)
    out = mo.denoise(noisy, f, 5, 10, rn=0.6)
    after = mo.mean_angle(out, f, v)
    by_taubin = [mo.mean_angle(mo.taubin(noisy, f, iters=k), f, v) for k in (5, 10)]
    ratio = mo.volume(out, f) / mo.volume(noisy, f)
    print(f"cube: mean normal angle {before:.2f} -> {after:.2f} degrees (taubin 5, 10: {by_taubin[0]:.2f}, {by_taubin[1]:.2f}), volume ratio {ratio:.5f}")
    assert after < 0.25 * before
    assert all(a > 0.5 * before for a in by_taubin)
    assert abs(ratio - 1.0) < 0.01


def test_boundary_modes_on_an_open_patch():
    v, f = mo.patch(8)
    adj = mo.adjacency(v, f)
    edge = (adj["flags"] & mo.BOUNDARY) != 0
    assert adj["counts"] == [208, 32, 0, 128] and edge.sum() == 32 and not (adj["flags"] & mo.NONMANIFOLD).any()
    noisy = mo.noisy(v, f, 0.1, seed=3, axes=(2,))
    fixed = mo.taubin(noisy, f, iters=10, boundary="fixed")
    assert np.array_equal(fixed[edge].view(np.uint32), noisy[edge].view(np.uint32)) and not np.array_equal(fixed[~edge], noisy[~edge])
    free = _extent(mo.taubin(noisy, f, iters=10, mu=0.0, boundary="free")) / _extent(noisy)
    curve = _extent(mo.taubin(noisy, f, iters=10, mu=0.0, boundary="curve")) / _extent(noisy)
    print(f"patch: x-y extent with mu = 0: free {free:.4f}, curve {curve:.4f}")
    assert free < 0.8
    assert 0.95 < curve <= 1.0
    # denoising a flat patch with noise along z flattens it, with its boundary held
    out = mo.denoise(noisy, f, 5, 10, rs=0.3)
    assert np.array_equal(out[edge], noisy[edge]) and np.abs(out[~edge, 2]).mean() < 0.5 * np.abs(noisy[~edge, 2]).mean()


# ---- the rules ---------------------------------------------------------------------------------------------------------------
def test_rules_on_small_cases():
    e = mo.adjacency(*mo.EMPTY)
    assert e["counts"] == [0, 0, 0, 0] and e["nbr_start"].tolist() == [0] and e["face_start"].tolist() == [0] and len(e["nbr"]) == 0
    assert mo.taubin(*mo.EMPTY).shape == (0, 3) and mo.denoise(*mo.EMPTY, rs=1.0).shape == (0, 3)
    # one triangle: all boundary, fixed under FIXED, moving under FREE
    v, f = mo.small("triangle")
    a = mo.adjacency(v, f)
    assert a["counts"] == [3, 3, 0, 1] and a["flags"].tolist() == [3, 3, 3] and a["nbr"].tolist() == [1, 2, 0, 2, 0, 1]
    assert a["nbr_boundary"].all() and a["vert_face"].tolist() == [0, 0, 0]
    assert np.array_equal(mo.taubin(v, f), v) and np.array_equal(mo.denoise(v, f, rs=1.0), v)
    moved = mo.taubin(v, f, iters=1, mu=0.0, boundary="free")
    assert np.array_equal(moved[0], (v[0] + 0.5 * ((v[1].astype(np.float64) + v[2]) / 2 - v[0])).astype(np.float32))
    # two triangles on an edge: the shared edge is no boundary edge, its ends are still boundary vertices
    a = mo.adjacency(*mo.small("two_triangles"))
    assert a["counts"] == [5, 4, 0, 2] and a["flags"].tolist() == [3, 3, 3, 3]
    assert a["nbr_start"].tolist() == [0, 2, 5, 8, 10] and a["nbr_boundary"].tolist() == [1, 1, 1, 0, 1, 1, 0, 1, 1, 1]
    assert a["vert_face"].tolist() == [0, 0, 1, 0, 1, 1]
    # a tetrahedron: closed
    v, f = mo.small("tetrahedron")
    a = mo.adjacency(v, f)
    assert a["counts"] == [6, 0, 0, 4] and a["flags"].tolist() == [1, 1, 1, 1] and not a["nbr_boundary"].any()
    assert mo.volume(v, f) == pytest.approx(1 / 6)
    one = mo.taubin(v, f, iters=1, mu=0.0)
    mean = np.stack([v[[j for j in range(4) if j != i]].astype(np.float64).sum(0) / 3 for i in range(4)])
    assert np.array_equal(one, (v + 0.5 * (mean - v)).astype(np.float32))
    # three faces on one edge
    a = mo.adjacency(*mo.small("three_on_an_edge"))
    assert a["counts"] == [7, 6, 1, 3] and a["flags"].tolist() == [7, 7, 3, 3, 3] and a["nbr_boundary"][0] == 0
    # a face listed twice: its edges are used twice (or, next to the other face, three times), and vert_face holds both copies
    a = mo.adjacency(*mo.small("face_twice"))
    assert a["counts"] == [5, 2, 1, 3] and a["flags"].tolist() == [1, 7, 7, 3]
    assert a["nbr_boundary"].tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 1, 1] and a["vert_face"].tolist() == [0, 2, 0, 1, 2, 0, 1, 2, 1]
    # a vertex no face uses, and faces that are not valid: nothing comes of them, and their vertices keep their bits
    for name, bits in (("unused_vertex", [3, 3, 3, 0]), ("bad_faces", [3, 3, 3, 0, 0])):
        v, f = mo.small(name)
        a = mo.adjacency(v, f)
        assert a["counts"] == [3, 3, 0, 1] and a["flags"].tolist() == bits and a["face_valid"].tolist() == [1] + [0] * (len(f) - 1)
        for out in (mo.taubin(v, f, boundary="free"), mo.denoise(v, f, rs=1.0, boundary="free")):
            assert np.array_equal(out[3:].view(np.uint32), v[3:].view(np.uint32))
    # the non-manifold fin and the bad-input sphere the GPU tests use
    assert mo.adjacency(*mo.fin())["counts"] == [13, 9, 1, 6]
    bv, bf, n = mo.bad_input()
    a, clean = mo.adjacency(bv, bf), mo.adjacency(*mo.icosphere(2))
    assert a["counts"] == clean["counts"] == [480, 0, 0, 320] and (a["flags"][n:] == 0).all() and np.array_equal(a["nbr"], clean["nbr"])
    out = mo.taubin(bv, bf)
    assert np.array_equal(out[:n], mo.taubin(*mo.icosphere(2))) and np.array_equal(out[n:].view(np.uint32), bv[n:].view(np.uint32))
    # iters = 0 and the bipyramids: apexes of valence n, closed
    assert np.array_equal(mo.taubin(*mo.icosphere(1), iters=0), mo.icosphere(1)[0])
    for k in (63, 64, 65):
        a = mo.adjacency(*mo.bipyramid(k))
        assert a["counts"] == [3 * k, 0, 0, 2 * k] and np.diff(a["nbr_start"]).tolist() == [4] * k + [k, k]


def test_the_filter_counts_an_edge_neighbour_twice_and_skips_beyond_its_supports():
    v, f = mo.small("two_triangles")
    adj = mo.adjacency(v, f)
    x = v.astype(np.float64)
    n, area, c = mo.face_frames(x, f, adj)
    assert np.allclose(np.linalg.norm(n, axis=1), 1) and area[0] == 0.5
    d2, q2 = ((c[0] - c[1]) ** 2).sum(), ((n[0] - n[1]) ** 2).sum()
    rs, rn = 1.0, 1.0
    w = area[1] * (1 - d2 / rs ** 2) ** 2 * (1 - q2 / rn ** 2) ** 2
    s = area[0] * n[0] + 2 * w * n[1]                          # face 1 is met at vertices 1 and 2
    got = mo.normal_filter(n, area, c, f, adj, 1, rs, rn)
    assert np.allclose(got[0], s / np.linalg.norm(s), rtol=0, atol=1e-15)
    # supports too small to see the neighbour: the normals come back as they were
    assert np.array_equal(mo.normal_filter(n, area, c, f, adj, 3, 1e-3, rn), n)
    assert np.array_equal(mo.normal_filter(n, area, c, f, adj, 3, rs, q2 ** 0.5 * 0.99), n)


# ---- no device work -----------------------------------------------------------------------------------------------------------
def _build():
    spec = importlib.util.spec_from_file_location("svs_build", os.path.join(ROOT, "s-volsdf_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    return build


def test_symbols_unit_and_command_line():
    from svs_hip import lib, meshsmooth
    for name, nargs in (("svs_mesh_smooth_workspace_bytes", 2), ("svs_mesh_adjacency", 14), ("svs_mesh_taubin", 12), ("svs_mesh_face_frames", 9),
                        ("svs_mesh_normal_filter", 14), ("svs_mesh_vertex_update", 12)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
    assert lib.ABI_VERSION == 101
    assert lib.SIGNATURES["svs_mesh_adjacency"][1][12] is ctypes.POINTER(ctypes.c_int)
    assert (lib.SMOOTH_FIXED, lib.SMOOTH_CURVE, lib.SMOOTH_FREE) == (mo.FIXED, mo.CURVE, mo.FREE) == (0, 1, 2)
    assert (lib.MESH_USED, lib.MESH_BOUNDARY, lib.MESH_NONMANIFOLD) == (mo.USED, mo.BOUNDARY, mo.NONMANIFOLD) == (1, 2, 4)
    assert _build().UNITS["svs_meshsmooth.hip"] == ["-ffp-contract=off"]
    base = ["--ply", "in.ply", "--ply-out", "out.ply"]
    a = meshsmooth.parse_args(base)
    assert (a.method, a.iters, a.lam, a.mu, a.boundary, a.report) == ("taubin", 10, 0.5, -0.53, "fixed", False)
    assert (a.normal_iters, a.vertex_iters, a.rn, a.rs) == (5, 10, 0.6, None)
    a = meshsmooth.parse_args(base + ["--method", "denoise", "--normal-iters", "3", "--vertex-iters", "7", "--rn", "0.4", "--rs", "0.1",
                                      "--boundary", "free", "--report"])
    assert (a.method, a.normal_iters, a.vertex_iters, a.rn, a.rs, a.boundary, a.report) == ("denoise", 3, 7, 0.4, 0.1, "free", True)
    a = meshsmooth.parse_args(base + ["--iters", "0", "--lambda", "1", "--mu", "0", "--boundary", "curve"])
    assert (a.iters, a.lam, a.mu, a.boundary) == (0, 1.0, 0.0, "curve")
    for bad in (["--method", "laplace"], ["--iters", "-1"], ["--lambda", "0"], ["--lambda", "1.5"], ["--mu", "0.1"], ["--mu", "-2.5"],
                ["--normal-iters", "-1"], ["--vertex-iters", "-2"], ["--rn", "0"], ["--rn", "2.5"], ["--rs", "0"], ["--rs", "-1"],
                ["--boundary", "loose"], ["--method", "denoise", "--boundary", "curve"], ["--iters", "1.5"]):
        with pytest.raises(SystemExit):
            meshsmooth.parse_args(base + bad)
    with pytest.raises(SystemExit):
        meshsmooth.parse_args(["--ply", "in.ply"])                                # --ply-out is required


def test_runner_carries_the_key(tmp_path):
    from svs_hip import run
    args = run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", "+tsdf_smooth=4"])
    assert args["tsdf_smooth"] == 4 and run.check_tsdf_smooth(args) == (4, "taubin")
    args = run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", "+tsdf_smooth=4", "+tsdf_smooth_method=denoise"])
    assert run.check_tsdf_smooth(args) == (4, "denoise")
    assert "tsdf_smooth" not in run.default_args() and run.check_tsdf_smooth(run.default_args()) is None
    with pytest.raises(KeyError):
        run.apply_overrides(run.default_args(), ["tsdf_smooth=4"])
    alone = run.apply_overrides(run.default_args(), ["+tsdf_smooth=4", f"outdir={tmp_path / 'out'}"])
    with pytest.raises(ValueError, match="tsdf_smooth.*tsdf_voxel"):
        run.run_help(alone, select_device=False)
    assert not os.path.exists(tmp_path / "out")                                   # refused before anything is made
    for bad in ("1.5", "0", "-3", "true", "many"):
        with pytest.raises(ValueError, match="tsdf_smooth"):
            run.check_tsdf_smooth(run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", f"+tsdf_smooth={bad}"]))
    for bad in ("laplace", "3", "true"):
        with pytest.raises(ValueError, match="tsdf_smooth_method"):
            run.check_tsdf_smooth(run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", "+tsdf_smooth=4", f"+tsdf_smooth_method={bad}"]))
    with pytest.raises(ValueError, match="tsdf_smooth_method"):
        run.check_tsdf_smooth(run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", "+tsdf_smooth_method=taubin"]))
    assert run.tsdf_smooth_ply_name("o", "scan106") == os.path.join("o", "tsdf_smooth", "mvsnet106_l3.ply")


def test_python_refuses_bad_parameters_before_any_call():
    """ValueError naming the entry, raised before the library is loaded or a tensor is made"""
    from svs_hip import meshsmooth as sm
    for fn, kw, entry in ((sm._iters, dict(entry="svs_mesh_taubin", what="iters", n=-1), "svs_mesh_taubin"),
                          (sm._iters, dict(entry="svs_mesh_vertex_update", what="vertex_iters", n=1.5), "svs_mesh_vertex_update"),
                          (sm._mode, dict(entry="svs_mesh_vertex_update", boundary="curve", allowed=("fixed", "free")), "svs_mesh_vertex_update"),
                          (sm._mode, dict(entry="svs_mesh_taubin", boundary="loose", allowed=("fixed", "curve", "free")), "svs_mesh_taubin")):
        with pytest.raises(ValueError, match=entry):
            fn(**kw)
    assert sm._mode("svs_mesh_taubin", "curve", ("fixed", "curve", "free")) == 1 and sm._iters("svs_mesh_taubin", "iters", 0) == 0
    with pytest.raises(ValueError, match="method"):
        sm.smooth_ply("in.ply", "out.ply", "laplace")


def test_argument_errors_name_the_entry():
    """the checks come before any device work: no GPU needed, dummy pointers are never dereferenced"""
    from svs_hip import lib
    _build().build(verbose=False)
    L = lib.load()
    d = ctypes.c_void_p(64)
    ESHAPE, EINVAL = -2, -1
    counts = (ctypes.c_int * 4)(7, 7, 7, 7)
    msg = L.svs_last_error_string
    too_many = (2 ** 31 - 1) // 6 + 1

    def adjacency(nv=5, nf=4, verts=d, faces=d, ws=d, nbr_start=d, nbr=d, nbr_boundary=d, face_start=d, vert_face=d, face_valid=d, flags=d,
                  out=counts):
        return L.svs_mesh_adjacency(verts, nv, faces, nf, ws, nbr_start, nbr, nbr_boundary, face_start, vert_face, face_valid, flags, out, None)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nf=too_many)):
        assert adjacency(**kw) == ESHAPE and msg().startswith(b"svs_mesh_adjacency: "), kw
    for kw in (dict(verts=None), dict(faces=None), dict(ws=None), dict(nbr_start=None), dict(nbr=None), dict(nbr_boundary=None),
               dict(face_start=None), dict(vert_face=None), dict(face_valid=None), dict(flags=None), dict(out=None)):
        assert adjacency(**kw) == EINVAL and msg().startswith(b"svs_mesh_adjacency: "), kw
    assert list(counts) == [7, 7, 7, 7]

    def taubin(x=d, tmp=d, nv=5, nbr_start=d, nbr=d, nbr_boundary=d, flags=d, iters=2, lam=0.5, mu=-0.53, boundary=0):
        return L.svs_mesh_taubin(x, tmp, nv, nbr_start, nbr, nbr_boundary, flags, iters, lam, mu, boundary, None)
    assert taubin(nv=-1) == ESHAPE and msg().startswith(b"svs_mesh_taubin: ")
    for kw in (dict(x=None), dict(tmp=None), dict(nbr_start=None), dict(flags=None), dict(iters=-1), dict(lam=0.0), dict(lam=1.5),
               dict(lam=float("nan")), dict(mu=0.1), dict(mu=-2.5), dict(mu=float("nan")), dict(boundary=3), dict(boundary=-1)):
        assert taubin(**kw) == EINVAL and msg().startswith(b"svs_mesh_taubin: "), kw
    assert taubin(nv=0) == 0 and taubin(iters=0) == 0         # nothing to do is not an error, and touches nothing

    def frames(x=d, nv=5, faces=d, face_valid=d, nf=4, normals=d, areas=d, cent=d):
        return L.svs_mesh_face_frames(x, nv, faces, face_valid, nf, normals, areas, cent, None)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nf=too_many)):
        assert frames(**kw) == ESHAPE and msg().startswith(b"svs_mesh_face_frames: "), kw
    for kw in (dict(x=None), dict(faces=None), dict(face_valid=None), dict(normals=None), dict(areas=None), dict(cent=None)):
        assert frames(**kw) == EINVAL and msg().startswith(b"svs_mesh_face_frames: "), kw
    assert frames(nf=0) == 0

    def nfilter(faces=d, face_valid=d, nf=4, nv=5, face_start=d, vert_face=d, areas=d, cent=d, normals=d, tmp=d, iters=2, rs=0.5, rn=0.6):
        return L.svs_mesh_normal_filter(faces, face_valid, nf, nv, face_start, vert_face, areas, cent, normals, tmp, iters, rs, rn, None)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nf=too_many)):
        assert nfilter(**kw) == ESHAPE and msg().startswith(b"svs_mesh_normal_filter: "), kw
    for kw in (dict(faces=None), dict(face_valid=None), dict(face_start=None), dict(areas=None), dict(cent=None),
               dict(normals=None), dict(tmp=None), dict(iters=-1), dict(rs=0.0), dict(rs=float("inf")), dict(rs=float("nan")), dict(rn=0.0),
               dict(rn=2.5), dict(rn=float("nan"))):
        assert nfilter(**kw) == EINVAL and msg().startswith(b"svs_mesh_normal_filter: "), kw
    assert nfilter(nf=0) == 0 and nfilter(iters=0) == 0

    def update(x=d, tmp=d, nv=5, faces=d, nf=4, face_start=d, vert_face=d, flags=d, normals=d, iters=2, boundary=0):
        return L.svs_mesh_vertex_update(x, tmp, nv, faces, nf, face_start, vert_face, flags, normals, iters, boundary, None)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nf=too_many)):
        assert update(**kw) == ESHAPE and msg().startswith(b"svs_mesh_vertex_update: "), kw
    for kw in (dict(x=None), dict(tmp=None), dict(faces=None), dict(face_start=None), dict(flags=None), dict(normals=None),
               dict(iters=-1), dict(boundary=1), dict(boundary=3)):
        assert update(**kw) == EINVAL and msg().startswith(b"svs_mesh_vertex_update: "), kw
    assert update(nv=0) == 0 and update(nf=0) == 0 and update(iters=0) == 0
    assert L.svs_mesh_smooth_workspace_bytes(1000, 2000) > L.svs_mesh_smooth_workspace_bytes(10, 20) > 0
    assert L.svs_mesh_smooth_workspace_bytes(-1, -1) == L.svs_mesh_smooth_workspace_bytes(0, 0)
