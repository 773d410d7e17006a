"""svs_hip.tsdf without a GPU: the float64 oracle's own mesh of the sphere scene (tests/tsdf_oracle.py), the host arithmetic
of the bounds, the coloured PLY, the runner's key and the ctypes table."""
import numpy as np
import pytest

import mesh_oracle as mo
import tsdf_oracle as to

CASES = {0.05: ((33, 35, 67), 6272, 2266), 0.1: ((17, 18, 35), 1344, 432)}       # voxel -> shape, faces before / after keep
_CACHE = {}


def _oracle_mesh(voxel):
    if voxel not in _CACHE:
        shape = CASES[voxel][0]
        sc = to.sphere_scene(shape, voxel)
        tsdf, weight, rgb, fragile = to.integrate_f32(shape, sc["origin"], voxel, sc["trunc"], [sc["views"]])
        verts, faces, _ = mo.marching_cubes(tsdf.astype(np.float64), 0.0, (voxel,) * 3)
        keep = to.face_keep(weight, to.mc_cells(tsdf, 0.0), 1.0)
        _CACHE[voxel] = dict(scene=sc, tsdf=tsdf, weight=weight, rgb=rgb, fragile=fragile, verts=verts, faces=faces, keep=keep)
    return _CACHE[voxel]


@pytest.mark.parametrize("voxel", list(CASES))
def test_oracle_mesh_of_the_sphere_scene(voxel):
    m = _oracle_mesh(voxel)
    sc = m["scene"]
    shape, n_all, n_kept = CASES[voxel]
    assert int(m["fragile"].sum()) == 0                       # the comparison rule's cap costs nothing on these inputs
    assert len(m["faces"]) == n_all and int(m["keep"].sum()) == n_kept
    kept = np.unique(m["faces"][m["keep"]])
    dist = np.abs(np.linalg.norm(m["verts"][kept] + sc["origin"] - sc["centre"], axis=1) - sc["radius"])
    print(f"voxel {voxel}: {n_all} -> {n_kept} faces, kept vertices within {dist.max() / voxel:.2f} voxel of the sphere, "
          f"min |tsdf| {np.abs(m['tsdf']).min():.2e}")
    assert dist.max() <= voxel
    assert np.abs(m["tsdf"]).min() >= 1e-4                    # no node near the level: the GPU's topology is the oracle's
    # the sphere's three seen caps, not its unseen rest: every kept vertex has a colour from a view
    col = to.vertex_colors(m["rgb"], m["weight"], m["verts"][kept] / voxel)
    assert (col.sum(1) > 0).all()


def test_oracle_arithmetic_on_one_voxel():
    """a voxel on the optical axis of a camera at the origin looking down +z: every figure by hand"""
    K = np.array([[10.0, 0, 2.0], [0, 10.0, 1.0], [0, 0, 1]])
    depth = np.full((3, 5), 2.0, np.float32)
    img = np.full((3, 5, 3), 0.5, np.float32)
    view = dict(K=K, E=np.eye(4), depth=depth, img=img)
    # nodes at z = 1.5, 1.75, 2, 2.25, 2.5 along the axis; trunc 0.3
    t, w, c, fr = to.integrate_f32((1, 1, 5), (0.0, 0.0, 1.5), 0.25, 0.3, [[view]])
    np.testing.assert_array_equal(w[0, 0], [1, 1, 1, 1, 0])                     # sdf = -0.5 < -trunc: skipped
    np.testing.assert_allclose(t[0, 0], [1.0, 0.25 / 0.3, 0.0, -0.25 / 0.3, 1.0], rtol=1e-6)
    np.testing.assert_allclose(c[:, 0, 0, :4], 0.5)
    assert c[:, 0, 0, 4].sum() == 0 and not fr.any()
    # a second launch of two views averages with the stored weight
    t2, w2, _, _ = to.integrate_f32((1, 1, 5), (0.0, 0.0, 1.5), 0.25, 0.3, [[view], [view, view]])
    np.testing.assert_array_equal(w2[0, 0], [3, 3, 3, 3, 0])
    np.testing.assert_allclose(t2[0, 0], t[0, 0], rtol=1e-6)
    # masked out, non-finite or non-positive depth: unobserved
    for bad in (0.0, -1.0, np.inf, np.nan):
        v = dict(view, depth=np.full((3, 5), bad, np.float32))
        assert to.integrate_f32((1, 1, 5), (0.0, 0.0, 1.5), 0.25, 0.3, [[v]])[1].sum() == 0
    v = dict(view, mask=np.zeros((3, 5), np.uint8))
    assert to.integrate_f32((1, 1, 5), (0.0, 0.0, 1.5), 0.25, 0.3, [[v]])[1].sum() == 0
    # u = 10 * x / z + 2.5 lands exactly on an integer at x = 0.15 z -> 0.05 z ... : flagged
    fr = to.integrate_f32((1, 1, 1), (0.1, 0.0, 2.0), 0.25, 0.3, [[view]])[3]
    assert fr.all()                                                             # u = 10 * 0.1 / 2 + 2.5 = 3


def test_bounds_from_points():
    from svs_hip import tsdf
    pts = np.array([[0.2, -1.3, 4.0], [3.9, 2.2, 5.05], [1.0, 0.0, 4.5]])
    origin, shape = tsdf.bounds_from_points(pts, 0.5, 0.75)
    np.testing.assert_array_equal(origin, [-1.0, -2.5, 3.0])                   # floor((min - pad) / voxel) * voxel
    assert shape == (13, 12, 7)                                                 # ceil((max + pad - origin) / voxel) + 1
    top = origin + (np.asarray(shape) - 1) * 0.5
    assert (top >= pts.max(0) + 0.75).all() and (origin <= pts.min(0) - 0.75).all()
    with pytest.raises(ValueError, match=str(13 * 12 * 7)):
        tsdf.bounds_from_points(pts, 0.5, 0.75, max_voxels=1000)
    assert tsdf.bounds_from_points(pts, 0.5, 0.75, max_voxels=13 * 12 * 7)[1] == shape
    with pytest.raises(ValueError):
        tsdf.bounds_from_points(np.zeros((0, 3)), 0.5, 0.75)
    # the default budget is 2**30 voxels
    with pytest.raises(ValueError, match="voxels"):
        tsdf.bounds_from_points(np.array([[0.0, 0, 0], [1100.0, 1100, 1100]]), 1.0, 0.0)


def _mesh():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, 0.5, 1.5]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [1, 3, 2]], np.int32)
    colors = np.array([[0, 1, 2], [255, 254, 253], [10, 20, 30], [128, 0, 77]], np.uint8)
    return verts, faces, colors


def test_coloured_ply_round_trips(tmp_path):
    from svs_hip import ply
    verts, faces, colors = _mesh()
    f = str(tmp_path / "c.ply")
    ply.write(f, verts, colors, faces)
    v, t = ply.read_mesh(f)
    np.testing.assert_array_equal(v, verts.astype(np.float64))
    np.testing.assert_array_equal(t, faces)
    p, c = ply.read_points(f)
    np.testing.assert_array_equal(p, verts.astype(np.float64))
    np.testing.assert_array_equal(c, colors)
    with pytest.raises(ValueError):
        ply.write(f, verts, colors[:3], faces)


def test_ply_without_colours_is_unchanged(tmp_path):
    from svs_hip import ply
    verts, faces, _ = _mesh()
    f = str(tmp_path / "m.ply")
    ply.write(f, verts, faces=faces)
    want = (b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
            b"element face 3\nproperty list uchar int vertex_indices\nend_header\n" + verts.astype("<f4").tobytes()
            + b"".join(b"\x03" + row.astype("<i4").tobytes() for row in faces))
    assert open(f, "rb").read() == want


def test_runner_carries_the_key():
    from svs_hip import run
    args = run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", "+tsdf_trunc=4.5"])
    assert args["tsdf_voxel"] == 1.5 and args["tsdf_trunc"] == 4.5
    assert "tsdf_voxel" not in run.default_args()                               # without the key nothing new runs
    with pytest.raises(KeyError):
        run.apply_overrides(run.default_args(), ["tsdf_voxel=1.5"])
    assert run.tsdf_ply_name("o", "scan106").replace("\\", "/") == "o/tsdf/mvsnet106_l3.ply"


def test_symbols_are_in_the_ctypes_table():
    from svs_hip import lib
    for name, nargs in (("svs_tsdf_integrate", 17), ("svs_tsdf_face_keep", 9), ("svs_tsdf_vertex_colors", 9)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
    assert lib.ABI_VERSION == 101


def test_argument_errors_name_the_entry():
    """the checks come before any device work: no GPU needed"""
    import ctypes
    from svs_hip import lib
    L = lib.load()
    d = ctypes.c_void_p(64)                                                     # never dereferenced
    o = (ctypes.c_double * 3)(0, 0, 0)
    ptrs = (ctypes.c_void_p * 17)(*([64] * 17))
    assert L.svs_tsdf_integrate(d, d, None, 4, 4, 4, o, 1.0, 3.0, ptrs, None, None, d, 17, 8, 8, None) < 0
    assert b"svs_tsdf_integrate" in L.svs_last_error_string() and b"16" in L.svs_last_error_string()
    assert L.svs_tsdf_integrate(d, d, None, 4, 4, 4, o, 1.0, 3.0, ptrs, None, None, d, 1, 0, 8, None) < 0
    assert b"svs_tsdf_integrate" in L.svs_last_error_string()
    for voxel, trunc in ((0.0, 3.0), (1.0, 0.0), (-1.0, 3.0), (1.0, -3.0)):
        assert L.svs_tsdf_integrate(d, d, None, 4, 4, 4, o, voxel, trunc, ptrs, None, None, d, 1, 8, 8, None) < 0
        assert b"svs_tsdf_integrate" in L.svs_last_error_string()
    assert L.svs_tsdf_integrate(None, d, None, 4, 4, 4, o, 1.0, 3.0, ptrs, None, None, d, 1, 8, 8, None) < 0
    assert L.svs_tsdf_face_keep(None, 4, 4, 4, d, 5, 1.0, d, None) < 0 and b"svs_tsdf_face_keep" in L.svs_last_error_string()
    assert L.svs_tsdf_face_keep(d, 1, 4, 4, d, 5, 1.0, d, None) < 0
    assert L.svs_tsdf_vertex_colors(d, d, 4, 4, 4, None, 5, d, None) < 0
    assert b"svs_tsdf_vertex_colors" in L.svs_last_error_string()
    assert L.svs_tsdf_face_keep(None, 4, 4, 4, None, 0, 1.0, None, None) == 0   # an empty mesh is not an error
