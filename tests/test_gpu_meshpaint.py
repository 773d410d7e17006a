"""svs_hip.meshpaint on the GPU against the float64 oracle (tests/meshpaint_oracle.py): view counts, masks, both modes, the
normal rules, image sizes, tolerances, bad input, repeatability, the normals, the hole filling, the round trip with the TSDF,
the folder path, the command and the error paths.

Comparison rule.  The oracle is given what the device was given: the depth maps the GPU rasterised (the rasteriser has its
own tests) and the float32 normals the GPU computed (their last bits depend on the order of the atomic adds).  At most 0.1 %
of the vertices may be `fragile` (a decision within 1e-9 of flipping); outside them `acc` agrees to 1e-12 relative (every
term is non-negative, a term costs about 30 float64 operations and there are at most 17 views, so the float64 bound is near
1e-13; the margin absorbs a differently rounded divide or square root), `rgb` codes and `painted` are exactly the oracle's.
Normals are within 2**-23 per component of the float64 ones (the rule for `normal` in test_gpu_meshview.py), outside the
vertices whose sum cancellation decides.  The hole filling is exact on every vertex when fed the oracle's inputs."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import meshpaint_oracle as mp
import meshview_oracle as mv
import tsdf_oracle as to
from svs_hip import lib, meshpaint, meshview, tsdf
from svs_hip import views as svs_views
from svs_hip.lib import SvsError
from test_gpu_meshview import VIEW_IDS, scan_folder  # noqa: F401  -- the scan folder fixture and its view ids

pytestmark = pytest.mark.gpu
TOL = 2.0 ** -23
ACC_TOL = 1e-12
DEV = "cuda"
H, W = 48, 64
_CACHE = {}


def _scene(n_lat, n_lon):
    key = (n_lat, n_lon)
    if key not in _CACHE:
        verts, faces = mv.scene(n_lat, n_lon)
        _CACHE[key] = dict(verts=verts, faces=faces, colors=mv.vertex_colors(len(verts)))
    return _CACHE[key]


def _rendered(s, views, h, w):
    """photographs of the scene in its vertex colours, drawn by the meshview oracle, computed once per set of cameras"""
    key = ("photos", len(s["verts"]), np.stack([np.concatenate([v["K"].ravel(), v["E"].ravel()]) for v in views]).tobytes(), h, w)
    if key not in _CACHE:
        zbuf, _ = mv.raster(s["verts"], s["faces"], views, h, w)
        _CACHE[key] = list(mv.resolve(zbuf, s["verts"], s["faces"], views, colors=s["colors"])[3])
    return _CACHE[key]


def _noise(n, h, w, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)]


def _np(t):
    return None if t is None else t.cpu().numpy()


def _check_acc(got, want, fragile, what):
    cap = 0.001 * len(fragile)
    n_frag = int(fragile.sum())
    assert n_frag <= cap, f"{what}: {n_frag} fragile vertices of {len(fragile)}"
    ok = ~fragile
    g, w = got[ok], want[ok]
    assert np.array_equal(g == 0, w == 0), f"{what}: the accumulators are not empty in the same places"
    with np.errstate(all="ignore"):
        ratio = np.where(w != 0, np.abs(g - w) / (ACC_TOL * np.abs(w)), 0.0)
    worst = float(ratio.max(initial=0.0))
    print(f"{what}: {len(fragile)} vertices, {n_frag} fragile, {int((want[:, 3] > 0).sum())} painted, acc error {worst:.4f} of the bound")
    assert worst <= 1.0
    return ok


def _run(s, views, images, masks=None, what="", h=H, w=W, **rules):
    """paint on the GPU and by the oracle on the same depth maps and normals, compared by the rule -> dict of both sides"""
    mode = rules.get("mode", "blend")
    stats = {}
    depth = meshview.rasterize(s["verts"], s["faces"], views, h, w)["depth"]
    colors, painted = meshpaint.paint(s["verts"], s["faces"], views, images, masks, depth=depth, spread_rounds=0, stats=stats, **rules)
    assert colors.dtype == torch.uint8 and tuple(colors.shape) == (len(s["verts"]), 3) and colors.is_cuda
    assert painted.dtype == torch.int32 and tuple(painted.shape) == (len(s["verts"]),)
    acc, normals = _np(stats["acc"]), _np(stats["normals"])
    assert (normals is None) == (not rules.get("use_normals", True))
    kw = {k: v for k, v in rules.items() if k != "use_normals"}
    want, fragile = mp.paint(s["verts"], normals, views, _np(depth), images, masks, **kw)
    ok = _check_acc(acc, want, fragile, what)
    rgb, flag = mp.finish(want, mode)
    assert np.array_equal(_np(colors)[ok], rgb[ok]) and np.array_equal(_np(painted)[ok], flag[ok]), f"{what}: codes differ"
    return dict(acc=acc, want=want, fragile=fragile, colors=_np(colors), painted=_np(painted), normals=normals, depth=depth)


# ---- paint -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_views", [1, 3, 16, 17])
def test_view_counts(n_views):
    s = _scene(12, 24)
    views = mv.cameras(n_views, seed=3)
    calls = dict(meshpaint.ENTRY_CALLS)
    res = _run(s, views, _rendered(s, views, H, W), what=f"{n_views} views")
    assert meshpaint.ENTRY_CALLS["paint"] - calls["paint"] == (n_views + 15) // 16          # 17 views: accumulated in two launches
    assert meshpaint.ENTRY_CALLS["finish"] - calls["finish"] == 1 and meshpaint.ENTRY_CALLS["spread"] == calls["spread"]
    assert 0 < res["painted"].sum() < len(res["painted"])


RULES = [dict(), dict(mode="best"), dict(use_normals=False), dict(use_normals=False, mode="best"), dict(one_sided=True),
         dict(one_sided=True, mode="best", power=1), dict(power=0), dict(power=0, mode="best"), dict(cos_min=0.5, power=8),
         dict(cos_min=0.0, power=3), dict(cos_min=1.0)]


@pytest.mark.parametrize("rules", RULES, ids=lambda r: "-".join(f"{k}={v}" for k, v in r.items()) or "defaults")
def test_rules_with_and_without_masks(rules):
    s = _scene(12, 24)
    views = mv.cameras(3)
    rng = np.random.default_rng(11)
    masks = [None if v == 1 else (rng.random((H, W)) > 0.3).astype(np.uint8) for v in range(3)]
    plain = _run(s, views, _rendered(s, views, H, W), what=f"{rules}", **rules)
    masked = _run(s, views, _rendered(s, views, H, W), masks, what=f"{rules} masked", **rules)
    if rules.get("cos_min") == 1.0:
        assert plain["painted"].sum() == 0                       # no generic vertex faces a camera exactly
    elif rules.get("mode") != "best":                            # a mask only takes views away
        assert (masked["want"][:, 3] <= plain["want"][:, 3]).all() and masked["want"][:, 3].sum() < plain["want"][:, 3].sum()
    if rules.get("one_sided"):
        assert plain["painted"].sum() <= _run(s, views, _rendered(s, views, H, W), what="two-sided", **dict(rules, one_sided=False))["painted"].sum()


def test_large_scene_noise_photographs():
    """20 000 vertices in 80 workgroups, photographs of seeded noise (every tap differs from its neighbours), both modes"""
    s = _scene(100, 200)
    views = mv.cameras(3)
    images = _noise(3, H, W)
    blend = _run(s, views, images, what="100 x 200 blend")
    best = _run(s, views, images, what="100 x 200 best", mode="best")
    assert np.array_equal(blend["painted"], best["painted"]) and blend["painted"].sum() > 5000
    assert (best["acc"][:, 3] <= blend["acc"][:, 3]).all()


@pytest.mark.parametrize("size", [(1, 1), (5, 7), (48, 64)])
def test_image_sizes(size):
    s = _scene(12, 24)
    views = mv.cameras(3)
    if size != (48, 64):                                       # the principal point moved so that the small image sees the scene
        for v in views:
            v["K"][0, 2], v["K"][1, 2] = size[1] / 2 - 0.2, size[0] / 2 - 0.1
    res = _run(s, views, _noise(3, *size, seed=9), what=f"{size}", h=size[0], w=size[1])
    if size == (1, 1):
        assert res["painted"].sum() == 0                       # 0 <= x <= W - 1 = 0: only a vertex exactly on the pixel centre
    else:
        assert res["painted"].sum() > 0


def test_tolerances_let_more_views_through():
    s = _scene(100, 200)
    views = mv.cameras(3, seed=5)
    images = _noise(3, H, W, seed=6)
    base = _run(s, views, images, what="rel 0.01", power=0)
    for kw in (dict(rel=0.5), dict(rel=0.0, abs_tol=0.2)):
        other = _run(s, views, images, what=f"{kw}", power=0, **kw)
        assert (other["acc"][:, 3] >= base["acc"][:, 3]).all() and other["acc"][:, 3].sum() > base["acc"][:, 3].sum()


def _bad_scene():
    """test_bad_faces_are_skipped's recipe: indices out of range, NaN, infinite and overflowing vertices, faces far off-screen"""
    from test_gpu_meshview import _off_screen
    s = _scene(12, 24)
    views = mv.cameras(3)
    n = len(s["verts"])
    extra_v = [[[np.nan, 0.1, 0.2], [np.inf, 0.0, 0.0], [3e38, 3e38, 3e38]]]
    for view in views:
        extra_v.append(_off_screen(view, [(1e6, 20.0), (1e6 + 30, 25.0), (1e6 + 10, 60.0)], 3.0))
        extra_v.append(_off_screen(view, [(-1e30, 2e29), (3e29, -1e30), (1e30, 1e30)], 0.01))
    verts = np.concatenate([s["verts"]] + extra_v).astype(np.float32)
    extra_f = [[0, 1, len(verts)], [-1, 0, 1], [2 ** 31 - 1, 3, 4], [0, 1, n], [5, n + 1, 6], [n + 2, 0, 1], [n, n + 1, n + 2]]
    extra_f += [[n + 3 + 3 * k, n + 4 + 3 * k, n + 5 + 3 * k] for k in range(6)]
    faces = np.concatenate([s["faces"], np.array(extra_f, np.int32)])
    return s, dict(verts=verts, faces=faces), views, n


def test_bad_vertices_and_faces_are_skipped():
    s, bad, views, n = _bad_scene()
    images = _rendered(s, views, H, W)
    for rules in (dict(), dict(use_normals=False, mode="best")):
        clean = _run(s, views, images, what=f"clean {rules}", **rules)
        res = _run(bad, views, images, what=f"bad input {rules}", **rules)
        assert not res["painted"][n:n + 3].any() and (res["colors"][n:n + 3] == 128).all()       # NaN, infinite, overflowing: unpainted
        assert np.array_equal(res["painted"][:n], clean["painted"]) and np.array_equal(res["colors"][:n], clean["colors"])
    res = _run(bad, views, images, what="bad input, normals")
    assert not np.isnan(res["normals"]).any() and (res["normals"][n:n + 2] == 0).all()      # the NaN and the infinite vertex
    # the hole filling walks the faces with valid indices only, and agrees with the oracle on this mesh too
    colors, painted = meshpaint.paint(bad["verts"], bad["faces"], views, images, depth=res["depth"])
    rgb, flag = mp.finish(res["acc"])
    rgb, flag, rounds = mp.spread(bad["faces"], len(bad["verts"]), rgb, flag)
    assert np.array_equal(_np(colors), rgb) and np.array_equal(_np(painted), flag) and rounds >= 1
    assert (flag[n:n + 3] > 1).all()                           # [5, n + 1, 6] has valid indices: an edge is an edge


def test_two_runs_are_bit_identical():
    s = _scene(100, 200)
    views = mv.cameras(17, seed=3)
    images = _noise(17, H, W, seed=8)
    verts, faces = svs_views.mesh_args(s["verts"], s["faces"])[:2]
    normals = meshpaint.vertex_normals(verts, faces)
    depth = meshview.rasterize(verts, faces, views, H, W)["depth"]
    out = []
    for mode in ("blend", "best"):
        runs = []
        for _ in range(2):
            acc = meshpaint.accumulate(verts, faces, views, images, normals=normals, depth=depth, flags=meshpaint.flags_of(mode))
            runs.append((acc,) + meshpaint.finish(acc, meshpaint.flags_of(mode)))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64))       # the bits, not only the values
        out.append(runs[0])
    assert int(out[0][2].sum()) > 5000 and torch.equal(out[0][2], out[1][2])
    # the normals go through atomic adds: a second run is within the tolerance of the first, not bound to its bits
    again = meshpaint.vertex_normals(verts, faces)
    assert float((again - normals).abs().max()) <= TOL


# ---- normals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lat,n_lon", [(12, 24), (100, 200)])
def test_normals_against_the_oracle(n_lat, n_lon):
    s = _scene(n_lat, n_lon)
    want, accum, fragile = mp.vertex_normals(s["verts"], s["faces"])
    calls = meshpaint.ENTRY_CALLS["normals"]
    acc = torch.zeros((len(s["verts"]), 3), dtype=torch.float64, device=DEV)
    got = meshpaint.vertex_normals(s["verts"], s["faces"], accum=acc)
    assert meshpaint.ENTRY_CALLS["normals"] - calls == 1 and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert not fragile.any()
    err = float(np.abs(_np(got).astype(np.float64) - want).max())
    scale = np.abs(accum).max(1, keepdims=True) + 1e-300
    print(f"{len(want)} vertices: normal error {err / TOL:.3f} of the bound, sums within {np.abs(_np(acc) - accum).max() / scale.max():.2e}")
    assert err <= TOL and np.allclose(_np(acc), accum, rtol=0, atol=1e-13 * float(scale.max()))
    # unit length, outward on the spheres
    n_big = (n_lat + 1) * n_lon
    out = (s["verts"][:n_big].astype(np.float64) - mv.BIG_CENTRE) / mv.BIG_RADIUS
    assert ((_np(got)[:n_big] * out).sum(1) > 0.9).all()
    # the faces in chunks compose: three calls, the last one normalises
    chunked = meshpaint.vertex_normals(s["verts"], s["faces"], chunk=len(s["faces"]) // 3 + 1)
    assert meshpaint.ENTRY_CALLS["normals"] - calls == 4
    assert float((chunked - got).abs().max()) <= TOL and np.abs(_np(chunked).astype(np.float64) - want).max() <= TOL


def test_normals_of_degenerate_input():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 2], [np.nan, 0, 0], [5, 5, 5]], np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 1, 4], [0, 1, 9], [-1, 0, 1]], np.int32)
    got = _np(meshpaint.vertex_normals(verts, faces))
    want = mp.vertex_normals(verts, faces)[0]
    assert np.abs(got - want).max() <= TOL and (got[4:] == 0).all() and np.array_equal(got[2], [0, 0, 1])
    assert tuple(meshpaint.vertex_normals(verts, faces[:0]).shape) == (6, 3)            # no faces: zeros
    assert tuple(meshpaint.vertex_normals(verts[:0], faces[:0]).shape) == (0, 3)        # an empty mesh is not an error


# ---- exact cases ---------------------------------------------------------------------------------------------------------
def test_exact_cases():
    from test_meshpaint_cpu import exact_images, exact_views, pixel_vertex
    A, B, C = exact_views()
    img = exact_images()
    zero = torch.zeros((3, 33, 33), dtype=torch.float32, device=DEV)
    tri = np.array([[0, 1, 2]], np.int32)
    verts = np.array([pixel_vertex(3, 5), pixel_vertex(3.5, 5.5), pixel_vertex(32, 0), pixel_vertex(32.25, 5), pixel_vertex(-0.25, 5)],
                     np.float32)
    rgb, painted = (_np(t) for t in meshpaint.paint(verts, tri, [A], img[:1], depth=zero[:1], use_normals=False, spread_rounds=0))
    four = img[0][5:7, 3:5].astype(np.int64).sum((0, 1))
    assert np.array_equal(painted, [1, 1, 1, 0, 0]) and np.array_equal(rgb[0], img[0][5, 3]) and np.array_equal(rgb[1], (2 * four + 4) // 8)
    assert np.array_equal(rgb[2], img[0][0, 32]) and (rgb[3:] == 128).all()
    # best on an exact tie: a triangle in the plane z = 2 whose normal is (0,0,-1) at every corner
    flat = np.array([[0, 0, 2.0], [0, 1, 2.0], [1, 0, 2.0]], np.float32)
    assert np.array_equal(_np(meshpaint.vertex_normals(flat, tri)), [[0, 0, -1.0]] * 3)
    for order, winner, pix in (((0, 1), 0, (16, 16)), ((1, 0), 0, (16, 16)), ((1, 2), 1, (16, 8)), ((2, 1), 2, (16, 24)), ((2, 1, 0), 0, (16, 16))):
        views, ims = [(A, B, C)[i] for i in order], [img[i] for i in order]
        rgb = _np(meshpaint.paint(flat, tri, views, ims, depth=zero[:len(order)], mode="best", spread_rounds=0)[0])
        assert np.array_equal(rgb[0], img[winner][pix]), order
        want = mp.finish(mp.paint(flat, np.float32([[0, 0, -1]] * 3), views, np.zeros((len(order), 33, 33), np.float32), ims, mode="best")[0], "best")[0]
        assert np.array_equal(rgb, want)


# ---- spread ------------------------------------------------------------------------------------------------------------
def test_spread_is_exact_on_the_oracles_inputs():
    s = _scene(100, 200)
    views = mv.cameras(1)
    res = _run(s, views, _noise(1, H, W, seed=12), what="one view, for the hole filling")
    rgb, flag = mp.finish(res["want"])                          # the oracle's inputs, fragile vertices and all
    faces = torch.from_numpy(s["faces"]).to(DEV)
    for rounds in (1, 3, None):
        colors, painted = torch.from_numpy(rgb).to(DEV), torch.from_numpy(flag).to(DEV)
        calls = meshpaint.ENTRY_CALLS["spread"]
        done = meshpaint.spread(faces, colors, painted, rounds)
        want_rgb, want_flag, want_done = mp.spread(s["faces"], len(rgb), rgb, flag, rounds)
        assert done == want_done and meshpaint.ENTRY_CALLS["spread"] - calls == want_done + (rounds is None)
        assert np.array_equal(_np(colors), want_rgb) and np.array_equal(_np(painted), want_flag)
    print(f"hole filling: {int((flag > 0).sum())} of {len(flag)} painted by the view, {want_done} rounds until nothing changes, "
          f"{int((want_flag == 0).sum())} never reached")
    # the spheres and the floor are components of their own: the view reaches into each, the triangle behind the cameras stays
    assert want_done > 10 and (want_flag[:-3] > 0).all() and (want_flag[-3:] == 0).all() and (want_rgb[-3:] == 128).all()
    # the strip and the square of test_meshpaint_cpu.py
    from test_meshpaint_cpu import strip
    colors = torch.full((16, 3), 128, dtype=torch.uint8, device=DEV)
    colors[0], colors[1] = torch.tensor([10, 200, 31], dtype=torch.uint8), torch.tensor([51, 100, 250], dtype=torch.uint8)
    painted = torch.zeros(16, dtype=torch.int32, device=DEV)
    painted[:2] = 1
    both = np.concatenate([strip(4), strip(2) + 10, [[0, 1, 99], [-1, 0, 1]]]).astype(np.int32)
    want = mp.spread(both, 16, _np(colors), _np(painted))
    assert meshpaint.spread(torch.from_numpy(both).to(DEV), colors, painted) == want[2] == 4
    assert np.array_equal(_np(colors), want[0]) and np.array_equal(_np(painted), want[1]) and (_np(painted)[10:] == 0).all()


# ---- round trip with the TSDF, the folder, the command ---------------------------------------------------------------------
def _codes(img):
    return np.clip(np.floor(np.asarray(img, np.float64) * 255.0 + 0.5), 0, 255).astype(np.uint8)


def test_round_trip_with_the_tsdf():
    """The sphere mesh of test_gpu_tsdf.py painted from its three views agrees with a fourth camera's photograph better than
    the same mesh in one colour (its own mean) does: a relative condition, no fixed figure."""
    shape, voxel = (33, 35, 67), 0.05
    sc = to.sphere_scene(shape, voxel)
    vol = tsdf.Volume(sc["origin"], shape, voxel, sc["trunc"])
    vol.integrate(sc["views"])
    verts, faces, _ = vol.mesh()
    images = [_codes(v["img"]) for v in sc["views"]]
    colors, painted = meshpaint.paint(verts, faces, sc["views"], images)
    assert int((painted == 1).sum()) > 0.5 * len(verts)
    E = to.look_at((1.1, 1.7, 0.9))
    depth4 = to.sphere_depth(to.SPHERE_K, E, H, W)
    fourth = [dict(K=to.SPHERE_K, E=E)]
    photo = [_codes(to.sphere_image(to.SPHERE_K, E, depth4))]
    score = meshpaint.consistency(verts, faces, colors, fourth, photo)
    mean = colors[painted > 0].double().mean(0).round().to(torch.uint8)
    flat = meshpaint.consistency(verts, faces, mean.repeat(len(verts), 1), fourth, photo)
    print(f"tsdf round trip: {len(verts)} vertices, {score['n']} seen by the fourth camera: PSNR {score['psnr']:.2f} dB, mean |difference| "
          f"{score['mad']:.2f} codes; in one colour {flat['psnr']:.2f} dB, {flat['mad']:.2f} codes")
    assert score["n"] == flat["n"] > 300 and score["psnr"] > flat["psnr"] and score["mad"] < flat["mad"]
    # the score is the oracle's on the same accumulators
    v, f = _np(verts), _np(faces)
    depth = meshview.rasterize(verts, faces, fourth, H, W)["depth"]
    acc = mp.paint(v, _np(meshpaint.vertex_normals(verts, faces)), fourth, _np(depth), photo)[0]
    want = mp.consistency(_np(colors), acc)
    assert want["n"] == score["n"] and abs(want["psnr"] - score["psnr"]) < 1e-6 and abs(want["mad"] - score["mad"]) < 1e-6


def test_paint_folder_and_command(scan_folder):
    from svs_hip import ply
    folder = str(scan_folder["folder"])
    out = str(scan_folder["root"] / "painted" / "sphere.ply")
    calls = dict(meshpaint.ENTRY_CALLS)
    colors, painted, stats = meshpaint.paint_folder(scan_folder["ply"], folder, VIEW_IDS, out)
    views = meshview.folder_cameras(folder, VIEW_IDS)
    images = meshpaint.folder_images(folder, VIEW_IDS)
    assert images[0].shape == (H, W, 3) and images[0].dtype == np.uint8
    direct = meshpaint.paint(scan_folder["verts"], scan_folder["faces"], views, images)
    assert torch.equal(colors, direct[0]) and torch.equal(painted, direct[1])
    rv, rf = ply.read_mesh(out)
    assert np.array_equal(rv, scan_folder["verts"].astype(np.float64)) and np.array_equal(rf, scan_folder["faces"])
    assert np.array_equal(ply.read_points(out)[1], _np(colors))
    assert stats["n_verts"] == len(rv) and stats["n_faces"] == len(rf) and stats["files"] == dict(ply=out) and stats["holdout"] is None
    assert sum(stats["painted"]) + stats["unpainted"] == len(rv) and stats["painted"][0] == int((painted == 1).sum()) > 100
    assert sum(stats["views"]) == len(rv) and len(stats["views"]) == 4
    assert stats["launches"]["paint"] == 1 and stats["launches"]["normals"] == 1 and stats["launches"]["finish"] == 1
    assert stats["launches"]["spread"] == len(stats["painted"])  # every round that filled, and the one that found nothing
    assert list(stats["seconds"]) == ["read", "upload", "normals", "raster", "paint", "spread", "download", "write"]
    assert all(x >= 0 for x in stats["seconds"].values()) and stats["seconds"]["paint"] > 0
    # the command: two views painted, the third held out
    cmd_out = str(scan_folder["root"] / "painted" / "cmd" / "two.ply")
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        c2, p2, st2 = meshpaint.main(["--ply", scan_folder["ply"], "--scan-folder", folder, "--views", str(VIEW_IDS[0]), str(VIEW_IDS[1]),
                                      "--holdout", str(VIEW_IDS[2]), "--ply-out", cmd_out, "--mode", "best", "--spread-rounds", "0",
                                      "--fill", "1", "2", "3"])
    assert "seconds: read" in text.getvalue() and cmd_out in text.getvalue() and "held-out views 28" in text.getvalue()
    direct = meshpaint.paint(scan_folder["verts"], scan_folder["faces"], views[:2], images[:2], mode="best", spread_rounds=0, fill=(1, 2, 3))
    assert torch.equal(c2, direct[0]) and np.array_equal(ply.read_points(cmd_out)[1], _np(c2))
    assert st2["unpainted"] > 0 and (_np(c2)[_np(p2) == 0] == [1, 2, 3]).all() and st2["launches"]["spread"] == 0
    want = meshpaint.consistency(scan_folder["verts"], scan_folder["faces"], c2, views[2:], images[2:])
    assert st2["holdout"]["n"] == want["n"] > 100 and np.isfinite(want["psnr"])
    assert abs(st2["holdout"]["psnr"] - want["psnr"]) < 1e-9 and abs(st2["holdout"]["mad"] - want["mad"]) < 1e-9
    # the painted file renders in colour where the unpainted one rendered its own
    res, _ = meshview.view_folder(out, folder, str(scan_folder["root"] / "painted" / "views"), VIEW_IDS)
    shade, depth = _np(res["shade"]), _np(res["depth"])
    drawn = shade[depth > 0].astype(int)
    assert (shade[depth == 0] == 255).all() and len(drawn) > 1000 and (np.abs(drawn[:, 0] - drawn[:, 2]) > 8).mean() > 0.5
    assert meshpaint.ENTRY_CALLS["paint"] - calls["paint"] == 6


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors(scan_folder, tmp_path):
    s = _scene(12, 24)
    verts, faces = torch.from_numpy(s["verts"]).to(DEV), torch.from_numpy(s["faces"]).to(DEV)
    views = mv.cameras(17)
    images = [torch.from_numpy(im).to(DEV) for im in _noise(17, H, W)]
    mats = svs_views.mats(views, DEV)
    depth = torch.zeros((17, H, W), device=DEV)
    acc = torch.zeros((len(verts), 4), dtype=torch.float64, device=DEV)
    rc = meshpaint.paint_raw(verts, None, mats, 17, H, W, depth, images, None, acc)
    with pytest.raises(SvsError, match="svs_mesh_paint.*16"):
        lib.check(rc, "svs_mesh_paint")
    for kw in (dict(power=9), dict(cos_min=1.5), dict(near=0.0), dict(rel=-0.1), dict(abs_tol=-1.0), dict(flags=4)):
        rc = meshpaint.paint_raw(verts, None, mats, 3, H, W, depth, images[:3], None, acc, **kw)
        with pytest.raises(SvsError, match="svs_mesh_paint: "):
            lib.check(rc, "svs_mesh_paint")
    rc = meshpaint.paint_raw(verts, None, mats, 3, H, W, depth, images[:2] + [None], None, acc)
    with pytest.raises(SvsError, match="svs_mesh_paint: view 2"):
        lib.check(rc, "svs_mesh_paint")
    torch.cuda.synchronize()
    assert float(acc.abs().sum()) == 0                          # nothing ran
    calls = dict(meshpaint.ENTRY_CALLS)
    host = [_np(im) for im in images[:3]]
    for kw, named in ((dict(power=9), "svs_mesh_paint"), (dict(cos_min=-0.5), "svs_mesh_paint"), (dict(mode="mean"), "svs_mesh_paint"),
                      (dict(rel=-1.0), "svs_mesh_paint"), (dict(near=0.0), "svs_mesh_paint"), (dict(masks=[None]), "svs_mesh_paint.*masks"),
                      (dict(masks=[np.ones((3, 3))] * 3), "svs_mesh_paint.*mask"), (dict(depth=depth[:2]), "svs_mesh_paint.*depth")):
        with pytest.raises(ValueError, match=named):
            meshpaint.paint(verts, faces, views[:3], host, use_normals=False, **kw)
    with pytest.raises(ValueError, match="svs_mesh_paint.*images"):
        meshpaint.paint(verts, faces, views[:3], host[:2], use_normals=False)
    with pytest.raises(ValueError, match="svs_mesh_paint.*one size"):
        meshpaint.paint(verts, faces, views[:3], host[:2] + [host[2][:40]], use_normals=False)
    with pytest.raises(ValueError, match="svs_mesh_paint: no views"):
        meshpaint.paint(verts, faces, [], [], use_normals=False)
    assert meshpaint.ENTRY_CALLS == calls                       # refused before anything was launched
    # views of different sizes in a folder
    import shutil
    from PIL import Image
    folder = tmp_path / "scan106"
    shutil.copytree(scan_folder["folder"], folder)
    Image.fromarray(np.zeros((40, 64, 3), np.uint8)).save(folder / "images" / f"{VIEW_IDS[1]:08}.jpg")
    with pytest.raises(ValueError, match="svs_mesh_paint.*different sizes"):
        meshpaint.paint_folder(scan_folder["ply"], str(folder), VIEW_IDS, str(tmp_path / "out.ply"))
    assert not os.path.exists(tmp_path / "out.ply") and meshpaint.ENTRY_CALLS == calls
    # an empty mesh is not an error
    colors, painted = meshpaint.paint(verts[:0], faces[:0], views[:2], host[:2])
    assert tuple(colors.shape) == (0, 3) and tuple(painted.shape) == (0,)
    colors, painted = meshpaint.paint(verts, faces[:0], views[:2], host[:2], use_normals=False, depth=depth[:2])
    assert int(painted.sum()) > 0 and meshpaint.ENTRY_CALLS["spread"] == calls["spread"]          # no faces: no edges to fill over
