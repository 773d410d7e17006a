"""svs_hip.meshview without a GPU: the float64 oracle (tests/meshview_oracle.py) against the analytic sphere, a hand-built exact
case, its order independence, the cull rule on host arrays, the ctypes table, the build list and the command line."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import meshview_oracle as mv
import tsdf_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 64


def test_oracle_depth_of_a_sphere_mesh_is_the_analytic_depth_within_two_sagittas():
    """A latitude-longitude mesh is inscribed in its sphere.  A triangle of it is half of a planar isosceles trapezoid, whose
    circumcircle it shares; near the equator, where the faces are largest, the trapezoid is almost a rectangle and the
    circumradius is half its diagonal, the mesh's longest edge.  So the plane of a face is at most the sagitta
    r - sqrt(r^2 - (edge / 2)^2) inside the sphere, and a ray that meets the surface at |n.d| >= 0.5 travels at most twice
    that between the two."""
    verts, faces = mv.uv_sphere(24, 48, mv.BIG_RADIUS, mv.BIG_CENTRE)
    verts = verts.astype(np.float32)
    tri = verts[faces].astype(np.float64)
    edge = max(np.linalg.norm(tri[:, a] - tri[:, b], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    sagitta = mv.BIG_RADIUS - np.sqrt(mv.BIG_RADIUS ** 2 - (edge / 2) ** 2)
    views = mv.cameras(3)
    zbuf, fragile = mv.raster(verts, faces, views, H, W)
    depth = mv.resolve(zbuf, verts, faces, views)[0]
    assert int(fragile.sum()) == 0
    for v, view in enumerate(views):
        K, E = view["K"], view["E"]
        want = to.sphere_depth(K, E, H, W, mv.BIG_CENTRE, mv.BIG_RADIUS).astype(np.float64)
        xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T
        hit = rays * want[..., None]
        normal = (hit - (E[:3, :3] @ mv.BIG_CENTRE + E[:3, 3])) / mv.BIG_RADIUS
        ndotd = np.abs((normal * rays).sum(-1) / np.linalg.norm(rays, axis=-1))
        at = (want > 0) & (ndotd >= 0.5)
        assert at.sum() > 300 and (depth[v][at] > 0).all()
        err = np.abs(depth[v].astype(np.float64) - want)[at].max()
        print(f"view {v}: {int(at.sum())} pixels, longest edge {edge:.4f}, sagitta {sagitta:.2e}, worst error {err / (2 * sagitta):.3f} of the bound")
        assert err <= 2 * sagitta
        assert (depth[v][want == 0] == 0).all()              # the inscribed mesh stays inside the sphere's outline


def test_oracle_exact_case_shared_edge():
    view = dict(K=mv.EXACT_K, E=np.eye(4))
    want_d, want_f = mv.exact_case_expectation()
    for faces, base in ((mv.EXACT_FACES, 5), (mv.EXACT_FACES[:, [0, 2, 1]], 5)):           # both orientations are drawn
        zbuf, fragile = mv.raster(mv.EXACT_VERTS, faces, [view], 9, 9, face_base=base)
        depth, face, normal, shade = mv.resolve(zbuf, mv.EXACT_VERTS, faces, [view], face_base=base)
        np.testing.assert_array_equal(depth[0], want_d)
        np.testing.assert_array_equal(face[0], want_f)
        diag = np.eye(9, dtype=bool) & (want_d > 0)
        assert fragile[0][diag].all()                        # on the shared edge: both faces cover these centres
        np.testing.assert_array_equal(normal[0][want_d > 0], np.broadcast_to([0.0, 0.0, -1.0], (25, 3)))
        assert (shade[0][want_d > 0] == 255).all() and (shade[0][want_d == 0] == 255).all()
    # the second face alone takes the diagonal too: the test is inclusive
    zbuf, _ = mv.raster(mv.EXACT_VERTS, mv.EXACT_FACES[1:], [view], 9, 9, face_base=6)
    face = mv.resolve(zbuf, mv.EXACT_VERTS, mv.EXACT_FACES[1:], [view], face_base=6)[1]
    assert (face[0][np.eye(9, dtype=bool) & (want_d > 0)] == 6).all()
    # a vertex colour per corner: at the square's centre the two ends of the diagonal mix half and half
    colors = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]], np.uint8)
    zbuf, _ = mv.raster(mv.EXACT_VERTS, mv.EXACT_FACES, [view], 9, 9)
    shade = mv.resolve(zbuf, mv.EXACT_VERTS, mv.EXACT_FACES, [view], colors=colors)[3]
    np.testing.assert_array_equal(shade[0, 4, 4], [128, 0, 128])
    np.testing.assert_array_equal(shade[0, 2, 2], [255, 0, 0])


def test_oracle_is_order_independent():
    verts, faces = mv.scene(12, 24)
    views = mv.cameras(3)
    whole, _ = mv.raster(verts, faces, views, H, W)
    cuts = [0, 200, 450, len(faces)]
    zbuf = None
    for k in (2, 0, 1):                                      # the blocks in another order, their ids carried by face_base
        zbuf, _ = mv.raster(verts, faces[cuts[k]:cuts[k + 1]], views, H, W, face_base=cuts[k], zbuf=zbuf)
    np.testing.assert_array_equal(zbuf, whole)
    rev = faces[::-1]                                        # and every face reversed in place: the winner's DEPTH is the same
    other, _ = mv.raster(verts, rev, views, H, W)
    np.testing.assert_array_equal(other >> np.uint64(32), whole >> np.uint64(32))


def test_cull_rule_on_host_arrays():
    from svs_hip import meshview
    verts = np.arange(18, dtype=np.float32).reshape(6, 3)
    faces = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5]], np.int32)
    colors = (np.arange(18).reshape(6, 3) * 10).astype(np.uint8)
    seen = np.array([2, 2, 2, 1, 0, 3], np.int32)
    off = np.array([0, 1, 0, 2, 0, 0], np.int32)
    cases = [(dict(), [0, 1]), (dict(mode="any"), [0, 1, 2, 3]), (dict(min_views=2), [0]), (dict(min_views=2, mode="any"), [0, 1, 2, 3]),
             (dict(max_off_mask=1), [0]), (dict(max_off_mask=0, mode="any"), [0, 1, 2, 3]), (dict(min_views=3, mode="any"), [3]), (dict(min_views=4, mode="any"), [])]
    for kw, want in cases:
        keep = mv.cull(verts, faces, seen, off, **kw)[-1]
        assert list(np.nonzero(keep)[0]) == want, kw
        ov, of, oc, _ = mv.cull(verts, faces, seen, off, colors=colors, **kw)
        gv, gf, gc = meshview.cull(torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(seen), torch.from_numpy(off),
                                   colors=torch.from_numpy(colors), **kw)
        np.testing.assert_array_equal(gv.numpy(), ov)
        np.testing.assert_array_equal(gf.numpy(), of)
        np.testing.assert_array_equal(gc.numpy(), oc)        # colours follow their vertices
        assert len(gf) == len(want) and (len(want) == 0 or int(gf.max()) == len(gv) - 1)
    assert len(meshview.cull(torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(seen))) == 2
    with pytest.raises(ValueError):
        meshview.cull(torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(seen), mode="most")
    with pytest.raises(ValueError):
        meshview.cull(torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(seen), max_off_mask=1)


def test_symbols_unit_and_command_line():
    from svs_hip import lib, meshview
    for name, nargs in (("svs_mesh_raster", 15), ("svs_mesh_raster_resolve", 16), ("svs_mesh_vertex_visibility", 14),
                        ("svs_mesh_raster_small_box", 0)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
    assert lib.ABI_VERSION == 101
    spec = importlib.util.spec_from_file_location("svs_build", os.path.join(ROOT, "s-volsdf_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.UNITS["svs_meshview.hip"] == ["-ffp-contract=off"]
    a = meshview.parse_args(["--ply", "m.ply", "--scan-folder", "s", "--out-folder", "o", "--views", "25", "22", "28"])
    assert a.views == [25, 22, 28] and a.size is None and not a.cull and a.min_views == 1 and a.max_off_mask is None
    assert a.rel == 0.01 and a.abs_tol == 0.0 and not a.any and a.ply_out is None and a.dataset is None
    a = meshview.parse_args(["--ply", "m.ply", "--scan-folder", "s", "--out-folder", "o", "--views", "1", "--size", "48", "64", "--cull",
                             "--min-views", "2", "--max-off-mask", "0", "--any", "--rel", "0.02", "--abs-tol", "0.5", "--ply-out",
                             "p.ply", "--data-dir-root", "d", "--dataset", "DTU"])
    assert a.size == [48, 64] and a.cull and a.min_views == 2 and a.max_off_mask == 0 and a.any and a.rel == 0.02
    assert a.abs_tol == 0.5 and a.ply_out == "p.ply" and a.data_dir_root == "d" and a.dataset == "DTU"
    with pytest.raises(SystemExit):
        meshview.parse_args(["--ply", "m.ply", "--scan-folder", "s", "--out-folder", "o", "--views", "1", "--dataset", "DTU"])


def test_runner_carries_the_switch():
    from svs_hip import run
    args = run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", "+tsdf_views=true"])
    assert args["tsdf_views"] is True
    assert "tsdf_views" not in run.default_args()            # without the key nothing new runs
    with pytest.raises(KeyError):
        run.apply_overrides(run.default_args(), ["tsdf_views=true"])


def test_argument_errors_name_the_entry():
    """the checks come before any device work: no GPU needed"""
    from svs_hip import lib
    L = lib.load()
    d = ctypes.c_void_p(64)                                  # never dereferenced
    ESHAPE, EINVAL = -2, -1
    raster = lambda n_views=1, H=8, W=8, near=1e-6, n_faces=5: L.svs_mesh_raster(d, 4, d, n_faces, d, n_views, H, W, near, 0, d, d,
                                                                                  4 + 16 * 5, 0, None)
    assert raster(n_views=17) == ESHAPE and b"svs_mesh_raster" in L.svs_last_error_string() and b"16" in L.svs_last_error_string()
    assert raster(H=0) == ESHAPE and raster(W=0) == ESHAPE
    for near in (0.0, -1.0, float("nan")):
        assert raster(near=near) == EINVAL and b"svs_mesh_raster: near" in L.svs_last_error_string()
    assert L.svs_mesh_raster(d, 4, d, 5, d, 2, 8, 8, 1e-6, 0, d, d, 4 + 9, 0, None) == ESHAPE          # work too small
    assert raster(n_faces=0) == 0                            # an empty mesh is not an error
    assert L.svs_mesh_raster(None, 0, None, 0, d, 3, 8, 8, 1e-6, 0, d, d, 4, 0, None) == 0
    resolve = lambda n_views=1, H=8: L.svs_mesh_raster_resolve(d, d, 4, d, 5, d, n_views, H, 8, 0, None, d, d, None, None, None)
    assert resolve(n_views=17) == ESHAPE and b"svs_mesh_raster_resolve" in L.svs_last_error_string()
    assert resolve(H=0) == ESHAPE
    assert L.svs_mesh_raster_resolve(None, d, 4, d, 5, d, 1, 8, 8, 0, None, d, d, None, None, None) == EINVAL
    vis = lambda n_views=1, H=8, near=1e-6, rel=0.01, tol=0.0, n=5: L.svs_mesh_vertex_visibility(d, n, d, n_views, H, 8, near, d, None,
                                                                                                 rel, tol, d, d, None)
    assert vis(n_views=17) == ESHAPE and b"svs_mesh_vertex_visibility" in L.svs_last_error_string()
    assert vis(H=0) == ESHAPE
    for kw in (dict(near=0.0), dict(rel=-0.01), dict(tol=-1.0)):
        assert vis(**kw) == EINVAL and b"svs_mesh_vertex_visibility" in L.svs_last_error_string()
    assert vis(n=0) == 0
    assert L.svs_mesh_raster_small_box() == 64
