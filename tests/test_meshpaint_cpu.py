"""svs_hip.meshpaint without a GPU: the float64 oracle (tests/meshpaint_oracle.py) against the analytic sphere, hand-built exact
cases, the hole filling on small meshes, the ctypes table, the build list, the command line and the argument checks."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import meshpaint_oracle as mp
import meshview_oracle as mv
import tsdf_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 64


def _codes(img):
    return np.clip(np.floor(np.asarray(img, np.float64) * 255.0 + 0.5), 0, 255).astype(np.uint8)


def test_oracle_colours_of_a_sphere_mesh_are_the_analytic_colours_within_the_footprint():
    """The photographs of tsdf_oracle.sphere_scene show colour = 0.5 + 0.8 (world - centre) at the point where a pixel centre's
    ray meets the sphere: linear in position, 0.8 per unit per channel, inside [0.1, 0.9] (nothing is clipped).  The vertices of
    the inscribed latitude-longitude mesh lie on the sphere.  A bilinear blend of linear colours is the colour of the same
    blend of the four hit points, so a view's colour at a vertex V is off by at most 0.8 D, D = the largest distance from V
    to the point where a ray through a tap meets the sphere.
    Footprint: a tap lies within one pixel of V's projection in x and in y, so its ray passes V within
    delta = sqrt(2) (z + 0.2) / f (f = the smaller focal length; rays off the axis are closer together; z = the distance from
    the eye to the sphere's centre, which no vertex on the side of the sphere that faces the eye exceeds; 0.2: more than the D
    below, for the rays' divergence between V and the hit).
    Angle: a point of the sphere at arc angle phi from V is, across the ray, at least r (c sin(phi) - sqrt(1 - c^2) (1 -
    cos(phi))) away from it, c = |normal . ray|: the step along the tangent plane seen at the cosine c, less what the sphere
    falls away.  The smallest phi at which that reaches delta bounds the hit, and D = 2 r sin(phi / 2) is its chord.
    Sagitta: a view counts when the MESH normal has c >= cos_min = 0.5.  A face's normal is the sphere's normal at the
    centre of its circumcircle, which the face's corners see at an angle theta with sin(theta) = (edge / 2) / r (the
    circumradius is half the longest edge, as test_meshview_cpu.py derives; the sagitta is r (1 - cos(theta))); the
    area-weighted mean of normals inside that cone stays inside it, so the true c >= cos(acos(0.5) + theta).
    Codes: 255 * 0.8 * D, plus 0.5 for the photographs' rounding to codes (a blend of taps each off by at most 0.5) and 0.5
    for the result's."""
    sc = to.sphere_scene()
    r, centre = sc["radius"], sc["centre"]
    verts, faces = mv.uv_sphere(48, 96, r, centre)
    verts = verts.astype(np.float32)
    views = sc["views"]
    images = [_codes(v["img"]) for v in views]
    zbuf, _ = mv.raster(verts, faces, views, H, W)
    depth = mv.resolve(zbuf, verts, faces, views)[0]
    normals, _, degenerate = mp.vertex_normals(verts, faces)
    assert not degenerate.any()
    true_n = (verts.astype(np.float64) - centre) / r
    tri = verts[faces].astype(np.float64)
    edge = max(np.linalg.norm(tri[:, a] - tri[:, b], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    theta = np.arcsin(edge / 2 / r)
    sagitta = r * (1 - np.cos(theta))
    assert np.degrees(np.arccos(np.clip((normals * true_n).sum(1), -1, 1))).max() <= np.degrees(theta)
    c0 = np.cos(np.arccos(0.5) + theta)
    z_max = max(np.linalg.norm(np.asarray(e) - centre) for e in to.SPHERE_EYES)
    delta = np.sqrt(2) * (z_max + 0.2) / min(views[0]["K"][0, 0], views[0]["K"][1, 1])
    phi = np.linspace(0, np.pi / 2, 200001)
    across = r * (c0 * np.sin(phi) - np.sqrt(1 - c0 ** 2) * (1 - np.cos(phi)))
    reach = np.nonzero(across >= delta)[0]
    assert len(reach) and (np.diff(across[:reach[0] + 1]) > 0).all()       # monotone up to there: the first hit
    D = 2 * r * np.sin(phi[reach[0]] / 2)
    assert D < 0.2
    bound = 255 * 0.8 * D + 1.0
    acc, fragile = mp.paint(verts, normals.astype(np.float32), views, depth, images, cos_min=0.5)
    rgb, painted = mp.finish(acc)
    want = 255.0 * (0.5 + 0.8 * (verts.astype(np.float64) - centre))
    err = np.abs(rgb.astype(np.float64) - want)[painted > 0].max()
    print(f"{int(painted.sum())} of {len(verts)} vertices painted at c >= 0.5, longest edge {edge:.4f}, sagitta {sagitta:.2e}, theta "
          f"{np.degrees(theta):.2f} deg, D {D:.4f}, bound {bound:.2f} codes, worst error {err:.2f} codes = {err / bound:.3f} of the bound, "
          f"{int(fragile.sum())} fragile")
    assert painted.sum() > 0.25 * len(verts) and err <= bound              # three caps of c >= 0.5 hold a quarter of the sphere each
    assert want.min() >= 0.1 * 255 - 1e-3 and want.max() <= 0.9 * 255 + 1e-3       # float32 vertices; far from any clipping
    # one view, both sides of the normal allowed: the far side is hidden behind the near one by the depth test alone
    acc0, _ = mp.paint(verts, normals.astype(np.float32), views[:1], depth[:1], images[:1])
    rgb0, painted0 = mp.finish(acc0)
    E = views[0]["E"]
    to_eye = -E[:3, :3].T @ E[:3, 3] - verts.astype(np.float64)
    far = (true_n * to_eye).sum(1) / np.linalg.norm(to_eye, axis=1) < -0.3
    assert far.sum() > 200 and not painted0[far].any() and (rgb0[far] == 128).all() and painted0.sum() > 200
    # the hole filling then reaches every vertex of the connected sphere
    _, filled, rounds = mp.spread(faces, len(verts), rgb0, painted0)
    assert rounds > 3 and (filled > 0).all() and filled.max() == rounds + 1


EXACT_K = np.array([[8.0, 0, 16.0], [0, 8.0, 16.0], [0, 0, 1]])


def exact_views():
    """cameras A at the origin, B at (2,0,0), C at (-2,0,0), all looking along +z; the vertex (0,0,2) with normal (0,0,-1)
    projects to pixel (16,16), (8,16), (24,16), with cosine 1 and twice the bitwise same 2 / sqrt(8)"""
    out = []
    for eye in ((0.0, 0, 0), (2.0, 0, 0), (-2.0, 0, 0)):
        E = np.eye(4)
        E[:3, 3] = -np.asarray(eye)
        out.append(dict(K=EXACT_K, E=E))
    return out


def exact_images(n=3, h=33, w=33, seed=2):
    return [np.random.default_rng(seed + i).integers(0, 256, (h, w, 3)).astype(np.uint8) for i in range(n)]


def pixel_vertex(x, y, z=2.0, K=EXACT_K):
    return [(x - K[0, 2]) * z / K[0, 0], (y - K[1, 2]) * z / K[1, 1], z]


def test_oracle_exact_cases():
    A, B, C = exact_views()
    img = exact_images()
    zero = np.zeros((3, 33, 33), np.float32)                  # nothing drawn: every view sees every vertex
    verts = np.array([pixel_vertex(3, 5), pixel_vertex(3.5, 5.5), pixel_vertex(32, 0), pixel_vertex(32.25, 5), pixel_vertex(-0.25, 5)],
                     np.float32)
    acc, _ = mp.paint(verts, None, [A], zero[:1], img[:1])
    rgb, painted = mp.finish(acc)
    np.testing.assert_array_equal(painted, [1, 1, 1, 0, 0])                      # a footprint that leaves the image is skipped
    np.testing.assert_array_equal(acc[0], list(img[0][5, 3]) + [1.0])            # a pixel centre: that pixel's code
    np.testing.assert_array_equal(rgb[0], img[0][5, 3])
    four = img[0][5:7, 3:5].astype(np.int64).sum((0, 1))
    np.testing.assert_array_equal(rgb[1], (2 * four + 4) // 8)                   # a half pixel: the rounded mean of four
    np.testing.assert_array_equal(rgb[2], img[0][0, 32])                         # the last column: x1 = min(x0 + 1, W - 1)
    np.testing.assert_array_equal(rgb[3:], [[128] * 3] * 2)
    # W = 1, H = 1 and a column of three
    K0 = np.array([[8.0, 0, 0], [0, 8.0, 0], [0, 0, 1]])
    one = dict(K=K0, E=np.eye(4))
    for shape, v, want in (((1, 1), [0, 0, 2.0], lambda im: im[0, 0]), ((3, 1), pixel_vertex(0, 1.5, K=K0), lambda im: (im[1, 0].astype(int) + im[2, 0] + 1) // 2),
                           ((1, 3), pixel_vertex(2, 0, K=K0), lambda im: im[0, 2])):
        im = np.random.default_rng(7).integers(0, 256, shape + (3,)).astype(np.uint8)
        acc, _ = mp.paint(np.array([v], np.float32), None, [one], np.zeros((1,) + shape, np.float32), [im])
        rgb, painted = mp.finish(acc)
        assert painted[0] == 1
        np.testing.assert_array_equal(rgb[0], want(im))
    # best: the steeper view, whatever its place; the earlier one on an exact tie
    v = np.array([[0, 0, 2.0]], np.float32)
    n = np.array([[0, 0, -1.0]], np.float32)
    for order, winner, pix in (((0, 1), 0, (16, 16)), ((1, 0), 0, (16, 16)), ((1, 2), 1, (16, 8)), ((2, 1), 2, (16, 24)), ((2, 1, 0), 0, (16, 16))):
        views, ims = [(A, B, C)[i] for i in order], [img[i] for i in order]
        acc, fragile = mp.paint(v, n, views, zero[:len(order)], ims, mode="best")
        np.testing.assert_array_equal(mp.finish(acc, "best")[0][0], img[winner][pix])
        assert acc[0, 3] == (1.0 if winner == 0 else (2.0 / np.sqrt(8.0)) ** 2)
        assert bool(fragile[0]) == (set(order) == {1, 2})                         # the tie of computed cosines is flagged
    # blend: weights cos^2 = 1 and 1/2 (to rounding); power 0 and no normals weigh every view 1
    acc, _ = mp.paint(v, n, [A, B], zero[:2], img[:2])
    w = (2.0 / np.sqrt(8.0)) ** 2
    np.testing.assert_array_equal(acc[0], list(img[0][16, 16] + w * img[1][16, 8]) + [1.0 + w])
    for kw in (dict(normals=None), dict(normals=n, power=0)):
        acc, _ = mp.paint(v, kw.pop("normals"), [A, B], zero[:2], img[:2], **kw)
        np.testing.assert_array_equal(acc[0], list(img[0][16, 16].astype(float) + img[1][16, 8]) + [2.0])
    # one-sided: a normal that points away counts with |c| only by default; cos_min cuts B and C; masks and depth cut views
    back = -n
    assert mp.paint(v, back, [A], zero[:1], img[:1])[0][0, 3] == 1.0
    assert mp.paint(v, back, [A], zero[:1], img[:1], one_sided=True)[0][0, 3] == 0.0
    assert mp.paint(v, n, [A, B, C], zero, img, cos_min=0.8)[0][0, 3] == 1.0
    mask = np.ones((33, 33), np.uint8)
    mask[16, 16] = 0
    assert mp.paint(v, n, [A, B], zero[:2], img[:2], masks=[mask, None])[0][0, 3] == w
    near_surface = np.full((1, 33, 33), 1.9, np.float32)
    assert mp.paint(v, n, [A], near_surface, img[:1])[0][0, 3] == 0.0            # z = 2 > 1.9 * 1.01
    assert mp.paint(v, n, [A], near_surface, img[:1], rel=0.06)[0][0, 3] == 1.0
    assert mp.paint(v, n, [A], near_surface, img[:1], rel=0.0, abs_tol=0.2)[0][0, 3] == 1.0
    # a zero or NaN normal: skipped in every view
    for bad in ([0, 0, 0], [np.nan, 0, 1]):
        assert mp.paint(v, np.array([bad], np.float32), [A, B], zero[:2], img[:2])[0][0, 3] == 0.0


def test_oracle_stays_inside_the_fragile_cap_for_the_gpu_tests_cameras():
    """test_gpu_meshpaint.py allows 0.1 % fragile vertices; on the 403-vertex scene that is none.  The oracle alone, on its own
    depth maps and normals, for the cameras and rules that file uses."""
    verts, faces = mv.scene(12, 24)
    colors = mv.vertex_colors(len(verts))
    normals = mp.vertex_normals(verts, faces)[0].astype(np.float32)
    for views in (mv.cameras(3), mv.cameras(17, seed=3)):
        zbuf, _ = mv.raster(verts, faces, views, H, W)
        depth, _, _, shade = mv.resolve(zbuf, verts, faces, views, colors=colors)
        for rules in (dict(), dict(mode="best"), dict(one_sided=True, mode="best", power=1), dict(cos_min=0.5, power=8), dict(cos_min=0.0, power=3)):
            acc, fragile = mp.paint(verts, normals, views, depth, list(shade), **rules)
            assert fragile.sum() <= 0.001 * len(verts) and (acc[:, 3] > 0).sum() > 100, rules
        acc, fragile = mp.paint(verts, None, views, depth, list(shade), mode="best")
        assert not fragile.any()                              # ties of weights that are 1 by construction are exact, not fragile


def strip(n_quads):
    """two rows of n_quads + 1 vertices: vertex 2 i and 2 i + 1 are ring i; quad i = faces (2i, 2i+1, 2i+2), (2i+1, 2i+3, 2i+2)"""
    f = []
    for i in range(n_quads):
        f += [[2 * i, 2 * i + 1, 2 * i + 2], [2 * i + 1, 2 * i + 3, 2 * i + 2]]
    return np.array(f, np.int32)


def test_oracle_spread():
    faces = strip(4)
    n = 10
    fill = (128, 128, 128)
    rgb = np.tile(np.uint8(fill), (n, 1))
    painted = np.zeros(n, np.int32)
    c0, c1 = np.array([10, 200, 31]), np.array([51, 100, 250])
    rgb[0], rgb[1] = c0, c1
    painted[:2] = 1
    # round 1: vertex 2 hears vertex 0 once (face 0) and vertex 1 twice (the edge (1,2) lies in faces 0 and 1); vertex 3
    # hears vertex 1 once
    r1, p1, changed = mp.spread_round(faces, n, 1, rgb, painted)
    assert changed
    np.testing.assert_array_equal(p1, [1, 1, 2, 2, 0, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(r1[2], (2 * (c0 + 2 * c1) + 3) // 6)
    np.testing.assert_array_equal(r1[3], c1)
    np.testing.assert_array_equal(r1[4:], rgb[4:])
    # round 2: ring 2 from ring 1 by the same counts
    r2, p2, _ = mp.spread_round(faces, n, 2, r1, p1)
    np.testing.assert_array_equal(p2, [1, 1, 2, 2, 3, 3, 0, 0, 0, 0])
    np.testing.assert_array_equal(r2[4], (2 * (r1[2].astype(int) + 2 * r1[3].astype(int)) + 3) // 6)
    np.testing.assert_array_equal(r2[5], r1[3])
    # a vertex filled in round r is not a source in round r: Jacobi
    stale, ps, _ = mp.spread_round(faces, n, 1, r1, p1)
    np.testing.assert_array_equal(ps, p1)
    # to the end: one ring per round, then a round that changes nothing
    out, p, rounds = mp.spread(faces, n, rgb, painted)
    assert rounds == 4
    np.testing.assert_array_equal(p, [1, 1, 2, 2, 3, 3, 4, 4, 5, 5])
    np.testing.assert_array_equal(out[:6], r2[:6])
    assert mp.spread(faces, n, rgb, painted, rounds=2)[2] == 2
    np.testing.assert_array_equal(mp.spread(faces, n, rgb, painted, rounds=2)[1], p2)
    np.testing.assert_array_equal(mp.spread(faces, n, rgb, painted, rounds=0)[0], rgb)
    # a component without a seed keeps `fill`; faces with bad indices are skipped
    both = np.concatenate([faces, strip(2) + 10, [[0, 1, 99], [-1, 0, 1]]]).astype(np.int32)
    rgb2 = np.tile(np.uint8(fill), (16, 1))
    rgb2[:2] = rgb[:2]
    painted2 = np.zeros(16, np.int32)
    painted2[:2] = 1
    out2, p2, rounds2 = mp.spread(both, 16, rgb2, painted2)
    assert rounds2 == 4 and (p2[10:] == 0).all() and (out2[10:] == 128).all()
    np.testing.assert_array_equal(out2[:10], out)
    # the two-triangle square: the diagonal (0,2) lies in both faces and counts twice
    square = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    rgb3 = np.tile(np.uint8(fill), (4, 1))
    rgb3[0], rgb3[1] = c0, c1
    out3, p3, _ = mp.spread_round(square, 4, 1, rgb3, np.array([1, 1, 0, 0], np.int32))
    np.testing.assert_array_equal(out3[2], (2 * (2 * c0 + c1) + 3) // 6)
    np.testing.assert_array_equal(out3[3], c0)
    np.testing.assert_array_equal(p3, [1, 1, 2, 2])


def test_oracle_normals_and_score():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 2], [np.nan, 0, 0], [5, 5, 5]], np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 1, 4], [0, 1, 9]], np.int32)
    normals, accum, fragile = mp.vertex_normals(verts, faces)
    np.testing.assert_array_equal(accum[0], [0, 2, 1])          # (0,0,1) of area 1/2 and (0,2,0) of area 1, unnormalised
    np.testing.assert_array_equal(accum[2], [0, 0, 1])
    np.testing.assert_array_equal(normals[2], [0, 0, 1])
    np.testing.assert_allclose(normals[0], np.array([0, 2, 1]) / np.sqrt(5.0), rtol=0, atol=1e-16)
    assert (normals[4:] == 0).all() and not fragile.any()
    flat = mp.vertex_normals(verts[:3], np.array([[0, 1, 2], [0, 2, 1]], np.int32))
    assert (flat[0] == 0).all() and flat[2].all()               # two faces that cancel: zero, and flagged
    acc = np.array([[20.0, 40, 60, 2], [0, 0, 0, 0], [7, 7, 7, 1]])
    s = mp.consistency(np.array([[10, 20, 33], [1, 2, 3], [7, 7, 4]], np.uint8), acc)
    assert s["n"] == 2 and s["mad"] == 1.0 and s["psnr"] == pytest.approx(10 * np.log10(255.0 ** 2 / 3.0), rel=1e-15)
    assert mp.consistency(np.zeros((2, 3), np.uint8), np.zeros((2, 4)))["n"] == 0


def test_symbols_unit_and_command_line():
    from svs_hip import lib, meshpaint
    for name, nargs in (("svs_mesh_vertex_normals", 7), ("svs_mesh_paint", 18), ("svs_mesh_paint_finish", 6), ("svs_mesh_paint_spread", 9)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
    assert lib.ABI_VERSION == 101 and (lib.PAINT_BEST, lib.PAINT_ONE_SIDED) == (1, 2)
    assert lib.SIGNATURES["svs_mesh_paint"][1][9] is lib.SIGNATURES["svs_mesh_paint"][1][10] is ctypes.POINTER(ctypes.c_void_p)
    spec = importlib.util.spec_from_file_location("svs_build", os.path.join(ROOT, "s-volsdf_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.UNITS["svs_meshpaint.hip"] == ["-ffp-contract=off"]
    assert set(meshpaint.ENTRY_CALLS) == {"normals", "paint", "finish", "spread"}
    base = ["--ply", "m.ply", "--scan-folder", "s", "--views", "25", "22", "28", "--ply-out", "p.ply"]
    a = meshpaint.parse_args(base)
    assert a.views == [25, 22, 28] and a.holdout == [] and a.mode == "blend" and a.cos_min == 0.1 and a.power == 2
    assert not a.one_sided and not a.no_normals and a.rel == 0.01 and a.abs_tol == 0.0 and a.spread_rounds is None
    assert a.fill == [128, 128, 128] and a.dataset is None and a.data_dir_root is None
    a = meshpaint.parse_args(base + ["--holdout", "23", "24", "--mode", "best", "--cos-min", "0.3", "--power", "0", "--one-sided",
                                     "--no-normals", "--rel", "0.02", "--abs-tol", "0.5", "--spread-rounds", "0", "--fill", "1", "2", "3",
                                     "--data-dir-root", "d", "--dataset", "DTU"])
    assert a.holdout == [23, 24] and a.mode == "best" and a.cos_min == 0.3 and a.power == 0 and a.one_sided and a.no_normals
    assert a.rel == 0.02 and a.abs_tol == 0.5 and a.spread_rounds == 0 and a.fill == [1, 2, 3] and a.dataset == "DTU"
    for bad in (["--dataset", "DTU"], ["--data-dir-root", "d"], ["--power", "9"], ["--cos-min", "1.5"], ["--rel", "-1"], ["--mode", "mean"],
                ["--holdout", "25"], ["--fill", "1", "2", "300"], ["--spread-rounds", "-1"]):
        with pytest.raises(SystemExit):
            meshpaint.parse_args(base + bad)
    with pytest.raises(SystemExit):
        meshpaint.parse_args(base[:-2])                        # --ply-out is required
    with pytest.raises(ValueError, match="svs_mesh_paint"):
        meshpaint.flags_of("mean")
    assert meshpaint.flags_of("best", True) == 3 and meshpaint.flags_of() == 0


def test_one_rules_record_serves_the_painter_the_atlas_and_both_command_lines(capsys):
    """`meshpaint.check_rules` is the one place that knows the rules: `flags_of`, `_check_rules` and `meshtexture._rules` are
    calls of it, with the messages they always had; both parsers take their shared options and range checks from meshpaint,
    and give the namespaces recorded below before they did."""
    from svs_hip import meshpaint, meshtexture
    r, flags = meshpaint.check_rules(dict(mode="best", one_sided=True))
    assert flags == 3 == meshpaint.flags_of("best", True) and r == dict(meshpaint.RULES, one_sided=True) and "mode" not in r
    assert meshpaint.check_rules({}) == (meshpaint.RULES, 0) and meshtexture._rules(dict(power=0, near=0.5))[0]["near"] == 0.5
    for call in (meshpaint.check_rules, meshtexture._rules):
        with pytest.raises(ValueError, match=r"svs_mesh_paint: cos_min in \[0,1\] and power an integer in \[0,8\], got 0.1 and 9"):
            call(dict(power=9))
        with pytest.raises(ValueError, match="svs_mesh_paint: mode 'blend' or 'best', got 'mean'"):
            call(dict(mode="mean"))
        with pytest.raises(ValueError, match="svs_mesh_paint: near must be positive, rel and abs_tol not negative, got 0.0, 0.01, 0.0"):
            call(dict(near=0.0))
    with pytest.raises(TypeError, match=r"svs_mesh_paint: unknown rules \['spread_rounds'\] \(known: \['abs_tol', 'cos_min', 'mode', 'near'"):
        meshpaint.check_rules(dict(spread_rounds=3))
    with pytest.raises(TypeError, match=r"svs_mesh_atlas_bake: unknown rules \['spread_rounds'\]"):
        meshtexture._rules(dict(spread_rounds=3, power=9))     # the unknown name is refused first
    with pytest.raises(ValueError, match="mode"):
        meshpaint.check_rules(dict(mode="mean", power=9))      # then the mode, then the ranges
    with pytest.raises(ValueError, match="svs_mesh_paint: cos_min"):
        meshpaint._check_rules(0.1, 2.5, 0.01, 0.0, 1e-6)
    shared = ["--views", "25", "22", "28", "--holdout", "23", "24", "--mode", "best", "--cos-min", "0.3", "--power", "3", "--one-sided",
              "--no-normals", "--rel", "0.02", "--abs-tol", "0.5", "--fill", "1", "2", "3"]
    want = dict(abs_tol=0.5, cos_min=0.3, data_dir_root=None, dataset=None, fill=[1, 2, 3], holdout=[23, 24], mode="best", no_normals=True,
                one_sided=True, ply="m.ply", power=3, rel=0.02, scan_folder="s", views=[25, 22, 28])
    a = meshpaint.parse_args(["--ply", "m.ply", "--scan-folder", "s", "--ply-out", "p.ply", "--spread-rounds", "4"] + shared)
    assert vars(a) == dict(want, ply_out="p.ply", spread_rounds=4)
    b = meshtexture.parse_args(["--ply", "m.ply", "--scan-folder", "s", "--obj-out", "o.obj", "--size", "512", "--cell", "9"] + shared)
    assert vars(b) == dict(want, obj_out="o.obj", size=512, cell=9)
    rules = dict(mode="best", cos_min=0.3, power=3, one_sided=True, use_normals=False, rel=0.02, abs_tol=0.5)
    assert meshpaint.painter_rules(a) == meshpaint.painter_rules(b) == rules and meshtexture._rules(rules)[1] == 3
    paint_base = ["--ply", "m.ply", "--scan-folder", "s", "--views", "25", "--ply-out", "p.ply"]
    bake_base = ["--ply", "m.ply", "--scan-folder", "s", "--views", "25", "--obj-out", "o.obj"]
    for parse, base, second in ((meshpaint.parse_args, paint_base, "--rel, --abs-tol and --spread-rounds are not negative, --fill holds codes in [0,255]"),
                                (meshtexture.parse_args, bake_base, "--rel and --abs-tol are not negative, --fill holds codes in [0,255]")):
        for bad, text in ((["--power", "9"], "--cos-min lies in [0,1] and --power in [0,8]"), (["--cos-min", "-0.1"], "--cos-min lies in [0,1] and --power in [0,8]"),
                          (["--abs-tol", "-1"], second), (["--fill", "0", "-1", "0"], second), (["--power", "9", "--rel", "-1"], "--cos-min lies"),
                          (["--dataset", "DTU", "--power", "9"], "--data-dir-root and --dataset come together")):
            with pytest.raises(SystemExit):
                parse(base + bad)
            assert text in capsys.readouterr().err, (bad, text)


def test_argument_errors_name_the_entry():
    """the checks come before any device work: no GPU needed"""
    from svs_hip import lib
    L = lib.load()
    d = ctypes.c_void_p(64)                                  # never dereferenced
    ESHAPE, EINVAL = -2, -1
    images = (ctypes.c_void_p * 16)(*([64] * 16))            # a host table of device addresses that are never read

    def paint(n_views=1, H=8, W=8, near=1e-6, rel=0.01, tol=0.0, cos_min=0.1, power=2, flags=0, n=5, images=images, acc=d):
        return L.svs_mesh_paint(d, n, d, d, n_views, H, W, near, d, images, None, rel, tol, cos_min, power, flags, acc, None)
    assert paint(n_views=17) == ESHAPE and b"svs_mesh_paint" in L.svs_last_error_string() and b"16" in L.svs_last_error_string()
    assert paint(H=0) == ESHAPE and paint(W=0) == ESHAPE and paint(n=-1) == ESHAPE
    for kw in (dict(power=9), dict(power=-1), dict(cos_min=1.5), dict(cos_min=-0.1), dict(cos_min=float("nan")), dict(near=0.0),
               dict(near=-1.0), dict(rel=-0.01), dict(tol=-1.0), dict(flags=4), dict(images=None), dict(acc=None)):
        assert paint(**kw) == EINVAL, kw
        assert L.svs_last_error_string().startswith(b"svs_mesh_paint: "), kw
    holes = (ctypes.c_void_p * 16)(*([64] * 16))
    holes[1] = None
    assert paint(n_views=2, images=holes) == EINVAL and b"svs_mesh_paint: view 1" in L.svs_last_error_string()
    assert paint(n=0) == 0 and paint(n_views=0) == 0          # an empty mesh is not an error
    normals = lambda n=5, f=4, verts=d, accum=d: L.svs_mesh_vertex_normals(verts, n, d, f, accum, d, None)
    assert normals(n=-1) == ESHAPE and normals(f=-1) == ESHAPE
    for kw in (dict(verts=None), dict(accum=None)):
        assert normals(**kw) == EINVAL and b"svs_mesh_vertex_normals" in L.svs_last_error_string()
    assert normals(n=0) == 0
    finish = lambda n=5, flags=0, rgb=d: L.svs_mesh_paint_finish(d, n, flags, rgb, d, None)
    assert finish(n=-1) == ESHAPE and finish(flags=8) == EINVAL and finish(rgb=None) == EINVAL
    assert b"svs_mesh_paint_finish" in L.svs_last_error_string() and finish(n=0) == 0
    spread = lambda n=5, f=4, round=1, work=d, changed=d: L.svs_mesh_paint_spread(d, f, n, round, d, d, work, changed, None)
    assert spread(n=-1) == ESHAPE and spread(f=-1) == ESHAPE
    for kw in (dict(round=0), dict(work=None), dict(changed=None)):
        assert spread(**kw) == EINVAL and b"svs_mesh_paint_spread" in L.svs_last_error_string()
    assert spread(n=0) == 0 and spread(f=0) == 0
