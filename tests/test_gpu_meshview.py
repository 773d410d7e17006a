"""svs_hip.meshview on the GPU against the float64 oracle (tests/meshview_oracle.py): the rasteriser on both of its paths and
at their threshold, bad input, view counts and image sizes, order independence, the resolve step, the vertex visibility,
the round trip with the TSDF, the cull rule, the folder path, the command, the runner switch and the error paths.

Comparison rule: outside the oracle's `fragile` pixels and vertices (a decision within 1e-9 of flipping, or two covering
depths within 2**-21; at most 0.1 % of a view's pixels and of the vertices) `face` and the float32 `depth` are exactly the
oracle's, `normal` is within 2**-23 per component (one float32 rounding of a component of magnitude <= 1, plus float64
noise that may move that rounding by one unit), `shade` codes are within 1, `seen` and `off_mask` are exact."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import mesh_oracle as mo
import meshview_oracle as mv
import tsdf_oracle as to
from svs_hip import lib, meshview, tsdf
from svs_hip import views as svs_views
from svs_hip.lib import SvsError

pytestmark = pytest.mark.gpu
TOL = 2.0 ** -23
DEV = "cuda"
H, W = 48, 64
_CACHE = {}


def _scene(n_lat, n_lon):
    """the two-sphere scene with colours and its oracle result in the three cameras at 48x64, computed once"""
    key = (n_lat, n_lon)
    if key not in _CACHE:
        verts, faces = mv.scene(n_lat, n_lon)
        colors = mv.vertex_colors(len(verts))
        views = mv.cameras(3)
        zbuf, fragile = mv.raster(verts, faces, views, H, W)
        _CACHE[key] = dict(verts=verts, faces=faces, colors=colors, views=views, zbuf=zbuf, fragile=fragile,
                           plain=mv.resolve(zbuf, verts, faces, views), coloured=mv.resolve(zbuf, verts, faces, views, colors=colors))
    return _CACHE[key]


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _check(got, want, fragile, what=""):
    """the comparison rule; want = (depth, face, normal, shade) of the oracle -> covered pixels"""
    depth, face, normal, shade = want
    n_views = fragile.shape[0]
    cap = 0.001 * fragile[0].size
    worst_n, worst_s = 0.0, 0
    for v in range(n_views):
        n_frag = int(fragile[v].sum())
        assert n_frag <= cap, f"{what}view {v}: {n_frag} fragile pixels of {fragile[v].size}"
        ok = ~fragile[v]
        assert np.array_equal(got["face"][v][ok], face[v][ok]), f"{what}view {v}: face ids differ"
        assert np.array_equal(got["depth"][v][ok].view(np.uint32), depth[v][ok].view(np.uint32)), f"{what}view {v}: depths differ"
        if "normal" in got:
            worst_n = max(worst_n, float(np.abs(got["normal"][v].astype(np.float64) - normal[v])[ok].max(initial=0.0)))
        if "shade" in got:
            worst_s = max(worst_s, int(np.abs(got["shade"][v].astype(np.int64) - shade[v].astype(np.int64))[ok].max(initial=0)))
    covered = int((face >= 0).sum())
    print(f"{what}{n_views} views of {fragile.shape[1]} x {fragile.shape[2]}: {covered} pixels covered, {int(fragile.sum())} fragile, "
          f"normal error {worst_n / TOL:.3f} of the bound, shade codes within {worst_s}")
    assert worst_n <= TOL and worst_s <= 1
    empty = (face < 0) & ~fragile
    assert (got["depth"][empty] == 0).all() and (got["face"][empty] == -1).all()
    if "normal" in got:
        assert (got["normal"][empty] == 0).all()
    if "shade" in got:
        assert (got["shade"][empty] == 255).all()
    return covered


def _large_pairs(verts, faces, views, h, w):
    box = np.stack([mv.box_pixels(verts, faces, v["K"], v["E"], h, w) for v in views])
    return int((box > meshview.small_box()).sum()), int(((box > 0) & (box <= meshview.small_box())).sum())


# ---- the rasteriser ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lat,n_lon", [(12, 24), (100, 200)])
@pytest.mark.parametrize("coloured", [True, False])
def test_scene_against_the_oracle(n_lat, n_lon, coloured):
    s = _scene(n_lat, n_lon)
    stats = {}
    got = _host(meshview.rasterize(s["verts"], s["faces"], s["views"], H, W, colors=s["colors"] if coloured else None, normals=True,
                                   shade=True, stats=stats))
    assert got["depth"].dtype == np.float32 and got["face"].dtype == np.int32 and got["shade"].dtype == np.uint8
    covered = _check(got, s["coloured" if coloured else "plain"], s["fragile"], f"{len(s['faces'])} faces: ")
    face = s["plain"][1]
    n_faces = len(s["faces"])
    floor = int(np.isin(face, [n_faces - 3, n_faces - 2]).sum())
    assert covered > 0.6 * face.size and floor > 2000          # about two thirds covered, the floor seen beside the spheres
    assert not (got["face"] == n_faces - 1).any()              # the face that reaches behind the cameras is not drawn
    # both paths were taken, by exactly the pairs the oracle's boxes name
    large, small = _large_pairs(s["verts"], s["faces"], s["views"], H, W)
    print(f"  {large} (view, face) pairs on the large path, {small} on the small one, {len(np.unique(face)) - 1} faces win a pixel")
    assert stats["large"] == large > 0 and small > 0
    if n_lat == 100:
        assert len(np.unique(face)) - 1 < 0.1 * n_faces         # most faces win no pixel


def test_most_faces_on_the_large_path():
    """the 12 x 24 scene four times as large (192 x 256): the spheres' faces hold a few hundred pixels each"""
    s = _scene(12, 24)
    views = mv.cameras(3, zoom=4.0)
    zbuf, fragile = mv.raster(s["verts"], s["faces"], views, 192, 256)
    stats = {}
    got = _host(meshview.rasterize(s["verts"], s["faces"], views, 192, 256, colors=s["colors"], normals=True, shade=True, stats=stats))
    _check(got, mv.resolve(zbuf, s["verts"], s["faces"], views, colors=s["colors"]), fragile, "zoom 4: ")
    large, small = _large_pairs(s["verts"], s["faces"], views, 192, 256)
    print(f"  {large} pairs on the large path, {small} on the small one")
    assert stats["large"] == large and large > small > 0


def _pixel_triangle(corners, z):
    """vertices whose projections under mv.EXACT_K are the given pixel positions at the given depths"""
    K = mv.EXACT_K
    return np.array([[(x - K[0, 2]) * d / K[0, 0], (y - K[1, 2]) * d / K[1, 1], d] for (x, y), d in zip(corners, z)], np.float32)


def test_boxes_at_the_small_threshold():
    """a box of exactly kSmallBox = 64 pixels (8 x 8) is walked by its lane, one of 65 (5 x 13) goes through the list"""
    assert meshview.small_box() == 64
    view = dict(K=mv.EXACT_K, E=np.eye(4))
    tri64 = _pixel_triangle([(0.3, 0.4), (8.2, 0.7), (0.6, 8.3)], (2.0, 2.1, 2.3))
    tri65 = _pixel_triangle([(0.3, 0.3), (5.4, 0.6), (0.7, 13.6)], (1.7, 1.9, 1.8))
    faces = np.array([[0, 1, 2]], np.int32)
    for verts, box, on_list in ((tri64, 64, 0), (tri65, 65, 1)):
        assert mv.box_pixels(verts, faces, view["K"], view["E"], 16, 16)[0] == box
        mats = svs_views.mats([view], DEV)
        zbuf = meshview.new_zbuf(1, 16, 16)
        stats = {}
        v_d, f_d = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
        meshview.raster_into(zbuf, v_d, f_d, mats, flags=meshview.FLAG_COUNT, stats=stats)
        got = _host(meshview.resolve(zbuf, v_d, f_d, mats, normals=True, shade=True))
        want_z, fragile = mv.raster(verts, faces, [view], 16, 16)
        covered = _check(got, mv.resolve(want_z, verts, faces, [view]), fragile, f"box of {box}: ")
        assert stats["large"] == on_list and stats["small"] == 1 - on_list
        assert stats["atomics"] == covered > 20               # one face, empty buffer: every covered pixel issues its atomic


def _off_screen(view, pixels, z):
    """world positions that `view` projects to the given pixel positions at depth z"""
    K, E = view["K"], view["E"]
    cam = np.array([[(x - K[0, 2]) * z / K[0, 0], (y - K[1, 2]) * z / K[1, 1], z] for x, y in pixels])
    return (cam - E[:3, 3]) @ E[:3, :3]


def test_bad_faces_are_skipped():
    """indices out of range, NaN, infinite and overflowing vertices, per view a face a million pixels off-screen and one
    with pixel coordinates of 1e30 change nothing; nothing faults"""
    s = _scene(12, 24)
    n = len(s["verts"])
    extra_v = [[[np.nan, 0.1, 0.2], [np.inf, 0.0, 0.0], [3e38, 3e38, 3e38]]]
    for view in s["views"]:
        extra_v.append(_off_screen(view, [(1e6, 20.0), (1e6 + 30, 25.0), (1e6 + 10, 60.0)], 3.0))
        extra_v.append(_off_screen(view, [(-1e30, 2e29), (3e29, -1e30), (1e30, 1e30)], 0.01))
    verts = np.concatenate([s["verts"]] + extra_v).astype(np.float32)
    extra_f = [[0, 1, len(verts)], [-1, 0, 1], [2 ** 31 - 1, 3, 4], [0, 1, n], [5, n + 1, 6], [n + 2, 0, 1], [n, n + 1, n + 2]]
    extra_f += [[n + 3 + 3 * k, n + 4 + 3 * k, n + 5 + 3 * k] for k in range(6)]
    faces = np.concatenate([s["faces"], np.array(extra_f, np.int32)])
    box = np.stack([mv.box_pixels(verts, faces, v["K"], v["E"], H, W) for v in s["views"]])
    assert (box[:, len(s["faces"]):] == 0).all()               # a condition on the input: none of them reaches a pixel
    want_z, fragile = mv.raster(verts, faces, s["views"], H, W)
    assert np.array_equal(want_z, s["zbuf"])
    got = _host(meshview.rasterize(verts, faces, s["views"], H, W, normals=True, shade=True))
    clean = _host(meshview.rasterize(s["verts"], s["faces"], s["views"], H, W, normals=True, shade=True))
    for k in clean:
        assert np.array_equal(got[k], clean[k]), k              # the rest of the image is unchanged
    _check(got, s["plain"], fragile, "bad faces: ")
    seen, off = meshview.visibility(verts, s["views"], clean["depth"])
    want_seen, want_off, frag = mv.visibility(verts, s["views"], clean["depth"], fragile_pixels=fragile)
    assert np.array_equal(seen.cpu().numpy()[~frag], want_seen[~frag]) and int(frag.sum()) == 0
    assert int(seen[n:n + 3].sum()) == 0                        # NaN, infinite and overflowing vertices are seen by no view


@pytest.mark.parametrize("n_views", [1, 3, 16, 17])
def test_view_counts(n_views):
    s = _scene(12, 24)
    views = mv.cameras(n_views, seed=3)
    calls = dict(meshview.ENTRY_CALLS)
    got = _host(meshview.rasterize(s["verts"], s["faces"], views, H, W, colors=s["colors"], normals=True, shade=True))
    launches = (n_views + 15) // 16
    assert meshview.ENTRY_CALLS["raster"] - calls["raster"] == launches == meshview.ENTRY_CALLS["resolve"] - calls["resolve"]
    zbuf, fragile = mv.raster(s["verts"], s["faces"], views, H, W)
    assert got["depth"].shape == (n_views, H, W) and got["normal"].shape == (n_views, H, W, 3)
    _check(got, mv.resolve(zbuf, s["verts"], s["faces"], views, colors=s["colors"]), fragile, f"{n_views} views: ")


@pytest.mark.parametrize("size", [(1, 1), (5, 7), (48, 64)])
def test_image_sizes(size):
    s = _scene(12, 24)
    views = mv.cameras(3)
    if size != (48, 64):                                       # the principal point moved so that the small image sees the scene
        for v in views:
            v["K"][0, 2], v["K"][1, 2] = size[1] / 2 - 0.2, size[0] / 2 - 0.1
    got = _host(meshview.rasterize(s["verts"], s["faces"], views, *size, colors=s["colors"], normals=True, shade=True))
    zbuf, fragile = mv.raster(s["verts"], s["faces"], views, *size)
    covered = _check(got, mv.resolve(zbuf, s["verts"], s["faces"], views, colors=s["colors"]), fragile, f"{size}: ")
    assert covered > 0


def test_order_independence_and_repeatability():
    s = _scene(100, 200)
    verts, faces = torch.from_numpy(s["verts"]).to(DEV), torch.from_numpy(s["faces"]).to(DEV)
    mats = svs_views.mats(s["views"], DEV)
    one = meshview.raster_into(meshview.new_zbuf(3, H, W), verts, faces, mats)
    again = meshview.raster_into(meshview.new_zbuf(3, H, W), verts, faces, mats)
    assert torch.equal(one, again)                              # two runs of the same call are bit-identical
    # the faces in blocks, the blocks in another order and reversed inside, their ids carried by face_base: two calls (and
    # then five) into one buffer give the same buffer everywhere, fragile pixels included
    n = len(s["faces"])
    for cuts in ([0, n // 3, n], [0, 777, 20001, 20002, 41000, n]):
        zbuf = meshview.new_zbuf(3, H, W)
        for k in reversed(range(len(cuts) - 1)):
            meshview.raster_into(zbuf, verts, faces[cuts[k]:cuts[k + 1]].contiguous(), mats, face_base=cuts[k])
        assert torch.equal(zbuf, one)
    got = _host(meshview.resolve(one, verts, faces, mats))
    _check(got, s["plain"], s["fragile"], "one call: ")


def test_exact_shared_edge():
    view = dict(K=mv.EXACT_K, E=np.eye(4))
    want_d, want_f = mv.exact_case_expectation()
    mats = svs_views.mats([view], DEV)
    verts = torch.from_numpy(mv.EXACT_VERTS).to(DEV)
    for faces in (mv.EXACT_FACES, mv.EXACT_FACES[:, [0, 2, 1]]):
        zbuf = meshview.new_zbuf(1, 9, 9)
        f_d = torch.from_numpy(np.ascontiguousarray(faces)).to(DEV)
        meshview.raster_into(zbuf, verts, f_d, mats, face_base=5)
        got = _host(meshview.resolve(zbuf, verts, f_d, mats, face_base=5, normals=True, shade=True))
        assert np.array_equal(got["depth"][0], want_d) and np.array_equal(got["face"][0], want_f)
        assert np.array_equal(got["normal"][0][want_d > 0], np.broadcast_to(np.float32([0, 0, -1]), (25, 3)))
        assert (got["shade"] == 255).all()
    # the second face first, in a call of its own: the smaller id still wins the diagonal
    zbuf = meshview.new_zbuf(1, 9, 9)
    for k in (1, 0):
        meshview.raster_into(zbuf, verts, torch.from_numpy(mv.EXACT_FACES[k:k + 1].copy()).to(DEV), mats, face_base=5 + k)
    assert np.array_equal(_host(meshview.resolve(zbuf, verts, torch.from_numpy(mv.EXACT_FACES).to(DEV), mats, face_base=5))["face"][0],
                          want_f)
    colors = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]], np.uint8)
    shade = _host(meshview.rasterize(mv.EXACT_VERTS, mv.EXACT_FACES, [view], 9, 9, colors=colors, shade=True))["shade"]
    assert np.array_equal(shade[0, 4, 4], [128, 0, 128]) and np.array_equal(shade[0, 2, 2], [255, 0, 0])


# ---- resolve -----------------------------------------------------------------------------------------------------------
def test_resolve_leaves_the_ids_of_another_calls_mesh():
    s = _scene(12, 24)
    n_big = 2 * 12 * 24                                        # the large sphere's faces: mesh A; the rest: mesh B
    verts = torch.from_numpy(s["verts"]).to(DEV)
    fa, fb = (torch.from_numpy(np.ascontiguousarray(f)).to(DEV) for f in (s["faces"][:n_big], s["faces"][n_big:]))
    mats = svs_views.mats(s["views"], DEV)
    zbuf = meshview.new_zbuf(3, H, W)
    meshview.raster_into(zbuf, verts, fb, mats, face_base=n_big)
    meshview.raster_into(zbuf, verts, fa, mats)
    colors = torch.from_numpy(s["colors"]).to(DEV)
    out = dict(normal=torch.full((3, H, W, 3), 7.0, device=DEV), shade=torch.full((3, H, W, 3), 9, dtype=torch.uint8, device=DEV))
    first = _host(meshview.resolve(zbuf, verts, fa, mats, colors=colors, normals=True, shade=True, out=out))
    want = s["coloured"]
    others = want[1] >= n_big
    assert others.sum() > 1000 and (want[1][~others] >= -1).all()
    assert (first["normal"][others] == 7).all() and (first["shade"][others] == 9).all()       # B's pixels: untouched
    assert np.array_equal(first["face"], want[1]) or s["fragile"].any()
    empty = want[1] < 0
    assert (first["normal"][empty & ~s["fragile"]] == 0).all() and (first["shade"][empty & ~s["fragile"]] == 255).all()
    second = _host(meshview.resolve(zbuf, verts, fb, mats, face_base=n_big, colors=colors, normals=True, shade=True, out=out))
    _check(second, want, s["fragile"], "two meshes: ")


# ---- visibility --------------------------------------------------------------------------------------------------------
def _far_side(verts, views, n_big):
    """vertices of the large sphere that face away from every camera by a clear margin"""
    v = verts[:n_big].astype(np.float64)
    normal = (v - mv.BIG_CENTRE) / mv.BIG_RADIUS
    far = np.ones(len(v), bool)
    for view in views:
        eye = -view["E"][:3, :3].T @ view["E"][:3, 3]
        to_eye = eye - v
        far &= (normal * to_eye).sum(1) / np.linalg.norm(to_eye, axis=1) < -0.3
    return np.nonzero(far)[0]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n_views", [3, 17])
def test_visibility(masked, n_views):
    s = _scene(12, 24) if n_views == 17 else _scene(100, 200)
    views = mv.cameras(n_views, seed=5)
    zbuf, frag_px = mv.raster(s["verts"], s["faces"], views, H, W)
    res = meshview.rasterize(s["verts"], s["faces"], views, H, W)
    depth = res["depth"].cpu().numpy()
    masks = None
    if masked:
        rng = np.random.default_rng(11)
        masks = [None if v == 1 else (rng.random((H, W)) > 0.3).astype(np.uint8) for v in range(n_views)]
    calls = meshview.ENTRY_CALLS["visibility"]
    seen, off = meshview.visibility(s["verts"], views, res["depth"], masks)
    assert meshview.ENTRY_CALLS["visibility"] - calls == (n_views + 15) // 16          # 17 views: accumulated in two launches
    seen, off = seen.cpu().numpy(), off.cpu().numpy()
    want_seen, want_off, fragile = mv.visibility(s["verts"], views, depth, masks, fragile_pixels=frag_px)
    n_frag = int(fragile.sum())
    assert n_frag <= 0.001 * len(fragile), f"{n_frag} fragile vertices of {len(fragile)}"
    ok = ~fragile
    assert seen.dtype == np.int32 and np.array_equal(seen[ok], want_seen[ok]) and np.array_equal(off[ok], want_off[ok])
    print(f"{len(seen)} vertices, {n_views} views{', masks' if masked else ''}: {n_frag} fragile, visible from at least one view "
          f"{(seen > 0).mean():.3f}, histogram {np.bincount(seen).tolist()}, off a mask {int((off > 0).sum())}")
    assert (off > 0).any() == masked and (seen > 0).any() and (seen == 0).any()
    if n_views == 3 and not masked:
        n_big = (100 + 1) * 200
        far = _far_side(s["verts"], views, n_big)
        assert len(far) > 100 and (seen[far] == 0).all()        # the far hemisphere is hidden behind the near one
    # a larger tolerance lets more through; abs_tol alone decides too
    for kw in (dict(rel=0.5), dict(rel=0.0, abs_tol=0.2)):
        other = meshview.visibility(s["verts"], views, res["depth"], masks, **kw)[0].cpu().numpy()
        want_other, _, frag = mv.visibility(s["verts"], views, depth, masks, fragile_pixels=frag_px, **kw)
        assert frag.sum() <= 0.001 * len(frag) and np.array_equal(other[~frag], want_other[~frag])
        assert (other >= seen).all() and other.sum() > seen.sum()


# ---- round trip with the TSDF --------------------------------------------------------------------------------------------
def test_round_trip_with_the_tsdf():
    """The sphere scene of test_gpu_tsdf.py meshed by tsdf.Volume(...).mesh() and rendered into its own three cameras.  The
    TSDF test puts the vertices within 1 voxel of the sphere, a chord of length `edge` adds its sagitta edge^2 / (8 radius), and a
    ray at |n.d| >= 0.5 at most doubles the sum: |depth - analytic| <= 2 (voxel + edge^2 / (8 radius)).  Compared where the
    views observed the surface: the pixels whose analytic hit lies in a cell all of whose nodes, and those of the cells
    around it, were observed (weight >= 1) -- there the TSDF's face rule keeps the surface; next to never-observed space it
    drops faces and a ray would see the cap of another view through the gap."""
    shape, voxel = (33, 35, 67), 0.05
    sc = to.sphere_scene(shape, voxel)
    vol = tsdf.Volume(sc["origin"], shape, voxel, sc["trunc"])
    vol.integrate(sc["views"])
    verts, faces, rgb = vol.mesh()
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    tri = v[f].astype(np.float64)
    edge = max(np.linalg.norm(tri[:, a] - tri[:, b], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    bound = 2 * (voxel + edge ** 2 / (8 * sc["radius"]))
    got = _host(meshview.rasterize(verts, faces, sc["views"], H, W, colors=rgb, normals=True, shade=True))
    zbuf, fragile = mv.raster(v, f, sc["views"], H, W)
    _check(got, mv.resolve(zbuf, v, f, sc["views"], colors=rgb.cpu().numpy()), fragile, "tsdf mesh: ")
    observed = vol.weight.cpu().numpy() >= 1
    worst = 0.0
    for i, view in enumerate(sc["views"]):
        K, E = view["K"], view["E"]
        want = to.sphere_depth(K, E, H, W).astype(np.float64)
        xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T
        hit = rays * want[..., None]
        normal = (hit - (E[:3, :3] @ sc["centre"] + E[:3, 3])) / sc["radius"]
        ndotd = np.abs((normal * rays).sum(-1) / np.linalg.norm(rays, axis=-1))
        cell = np.floor(((hit - E[:3, 3]) @ E[:3, :3] - sc["origin"]) / voxel).astype(int)
        at = (want > 0) & (ndotd >= 0.5)
        for y, x in zip(*np.nonzero(at)):
            a, b, c = cell[y, x]
            block = observed[max(a - 1, 0):a + 3, max(b - 1, 0):b + 3, max(c - 1, 0):c + 3]
            at[y, x] = block.size == 64 and bool(block.all())
        assert at.sum() > 200 and (got["depth"][i][at] > 0).all()
        worst = max(worst, float(np.abs(got["depth"][i] - want)[at].max()))
    print(f"tsdf round trip: {len(f)} faces, longest edge {edge / voxel:.2f} voxels, worst depth error {worst / bound:.3f} of the bound")
    assert worst <= bound


# ---- cull --------------------------------------------------------------------------------------------------------------
def test_cull_against_the_oracle():
    s = _scene(12, 24)
    res = meshview.rasterize(s["verts"], s["faces"], s["views"], H, W)
    seen, off = meshview.visibility(s["verts"], s["views"], res["depth"])
    want_seen, _, fragile = mv.visibility(s["verts"], s["views"], res["depth"].cpu().numpy(), fragile_pixels=s["fragile"])
    assert not fragile.any() and np.array_equal(seen.cpu().numpy(), want_seen)
    verts, faces, colors = (torch.from_numpy(s[k]).to(DEV) for k in ("verts", "faces", "colors"))
    v, f, c = (t.cpu().numpy() for t in meshview.cull(verts, faces, seen, min_views=1, colors=colors))
    ov, of, oc, keep = mv.cull(s["verts"], s["faces"], want_seen, colors=s["colors"])
    assert np.array_equal(v, ov) and np.array_equal(f, of) and np.array_equal(c, oc)     # face for face; colours follow
    assert 0 < len(f) == int(keep.sum()) < len(s["faces"])
    assert (want_seen[s["faces"][keep]] >= 1).all()             # every surviving face has all of its vertices seen
    assert f.dtype == np.int32 and f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)
    assert len(mo.vertex_labels(len(v), f)) == len(v) and (mo.face_areas(v, f) >= 0).all()
    v2, f2 = meshview.cull(verts, faces, seen, off, min_views=2, max_off_mask=0, mode="any")
    assert np.array_equal(f2.cpu().numpy(), mv.cull(s["verts"], s["faces"], want_seen, off.cpu().numpy(), 2, 0, "any")[1])
    print(f"cull: {len(s['faces'])} -> {len(f)} faces at min_views 1, {len(f2)} at min_views 2 / any")


# ---- folder, command, runner ---------------------------------------------------------------------------------------------
VIEW_IDS = (25, 22, 28)
NEAR_EYES = ((2.03, 0.31, 0.42), (1.9, 0.62, 0.5), (1.95, 0.0, 0.28))
FOLDER_VOXEL = 0.05


@pytest.fixture(scope="module")
def scan_folder(tmp_path_factory):
    """{root}/scan106 as test_gpu_tsdf.py writes it (cams, JPEGs, depth and confidence PFMs), and a coloured mesh file"""
    from datasets.data_io import save_pfm
    from helpers.utils import write_cam
    from PIL import Image
    from svs_hip import ply
    root = tmp_path_factory.mktemp("meshview")
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
    verts, faces = mv.uv_sphere(16, 32, sc["radius"], sc["centre"])
    colors = mv.vertex_colors(len(verts), seed=4)
    mesh_file = str(root / "sphere.ply")
    ply.write(mesh_file, verts.astype(np.float32), colors, faces.astype(np.int32))
    return dict(root=root, folder=folder, scene=sc, ply=mesh_file, verts=verts.astype(np.float32), faces=faces.astype(np.int32),
                colors=colors)


def _read_outputs(out_folder):
    from datasets.data_io import read_pfm
    from svs_hip.images import read_png
    depth = np.stack([np.ascontiguousarray(read_pfm(os.path.join(out_folder, "mesh_depth", f"{v:08}.pfm"))[0]) for v in VIEW_IDS])
    shade = np.stack([read_png(os.path.join(out_folder, "mesh_shade", f"{v:08}.png")) for v in VIEW_IDS])
    return depth, shade


def test_view_folder(scan_folder):
    folder, out = str(scan_folder["folder"]), str(scan_folder["root"] / "views")
    res, stats = meshview.view_folder(scan_folder["ply"], folder, out, VIEW_IDS)
    views = meshview.folder_cameras(folder, VIEW_IDS)
    direct = _host(meshview.rasterize(scan_folder["verts"], scan_folder["faces"], views, H, W, colors=scan_folder["colors"], shade=True))
    depth, shade = _read_outputs(out)
    assert np.array_equal(depth, direct["depth"]) and np.array_equal(shade, direct["shade"])
    assert sorted(os.listdir(out)) == ["mesh_depth", "mesh_shade"]
    assert sorted(os.listdir(os.path.join(out, "mesh_depth"))) == [f"{v:08}.pfm" for v in sorted(VIEW_IDS)]
    assert stats["n_faces"] == len(scan_folder["faces"]) and stats["faces_kept"] is None
    assert stats["covered"] == [int((d > 0).sum()) for d in direct["depth"]] and min(stats["covered"]) > 300
    assert stats["launches"] == dict(raster=1, resolve=1, visibility=0)
    assert list(stats["seconds"]) == ["read", "upload", "raster", "visibility", "download", "write"]
    assert all(x >= 0 for x in stats["seconds"].values()) and stats["seconds"]["raster"] > 0
    # the file's cameras are float32: the oracle on the same cameras
    zbuf, fragile = mv.raster(scan_folder["verts"], scan_folder["faces"], views, H, W)
    _check(direct, mv.resolve(zbuf, scan_folder["verts"], scan_folder["faces"], views, colors=scan_folder["colors"]), fragile, "folder: ")
    # size given: another pixel grid for the same cameras
    res2, _ = meshview.view_folder(scan_folder["ply"], folder, str(scan_folder["root"] / "small"), VIEW_IDS, size=(30, 40))
    assert tuple(res2["depth"].shape) == (3, 30, 40)
    assert np.array_equal(res2["depth"].cpu().numpy(), direct["depth"][:, :30, :40])


def test_command_cull(scan_folder):
    from svs_hip.ply import read_mesh, read_points
    folder, out = str(scan_folder["folder"]), str(scan_folder["root"] / "cmd")
    ply_out = str(scan_folder["root"] / "cmd" / "sub" / "culled.ply")
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res, stats = meshview.main(["--ply", scan_folder["ply"], "--scan-folder", folder, "--out-folder", out, "--views",
                                    *map(str, VIEW_IDS), "--cull", "--min-views", "2", "--ply-out", ply_out])
    assert "seconds: read" in text.getvalue() and ply_out in text.getvalue()
    views = meshview.folder_cameras(folder, VIEW_IDS)
    seen, _ = meshview.visibility(scan_folder["verts"], views, res["depth"])
    ov, of, oc, keep = mv.cull(scan_folder["verts"], scan_folder["faces"], seen.cpu().numpy(), min_views=2, colors=scan_folder["colors"])
    rv, rf = read_mesh(ply_out)
    assert np.array_equal(rv, ov.astype(np.float64)) and np.array_equal(rf, of) and np.array_equal(read_points(ply_out)[1], oc)
    assert stats["faces_kept"] == len(rf) == int(keep.sum()) and 0 < len(rf) < len(scan_folder["faces"])
    assert stats["launches"]["visibility"] == 1 and stats["files"]["ply"] == ply_out
    depth, _ = _read_outputs(out)
    assert np.array_equal(depth, res["depth"].cpu().numpy())


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)


def test_runner_switch(scan_folder, tmp_path):
    import shutil
    from svs_hip import run
    root = tmp_path / "fused"
    shutil.copytree(scan_folder["folder"], root / "scan106")
    base = [f"outdir={root}", "filter_only=true", "eval_mask=false", "testlist=scan106", f"+tsdf_voxel={FOLDER_VOXEL}"]
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base)
    plain = _tree(root)
    assert "mesh_views" not in res and "tsdf views seconds" not in text.getvalue()
    assert sorted(os.listdir(root / "tsdf")) == ["mvsnet106_l3.ply"]           # what a run without the switch writes today
    assert sorted(os.listdir(root / "scan106")) == ["cams", "confidence", "depth_est", "images", "mask"]
    mesh_bytes = open(root / "tsdf" / "mvsnet106_l3.ply", "rb").read()
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base + ["+tsdf_views=true"])
    new = sorted(set(_tree(root)) - set(plain))
    assert new == sorted(os.path.join("tsdf", "scan106", sub, f"{v:08}{ext}") for sub, ext in (("mesh_depth", ".pfm"), ("mesh_shade", ".png"))
                         for v in VIEW_IDS)
    assert open(root / "tsdf" / "mvsnet106_l3.ply", "rb").read() == mesh_bytes
    assert text.getvalue().count("scan106 tsdf views seconds: read ") == 1
    stats = res["mesh_views"]["scan106"]
    assert stats["n_faces"] == res["meshes"]["scan106"]["n_faces"] and min(stats["covered"]) > 100
    depth, shade = _read_outputs(str(root / "tsdf" / "scan106"))
    assert depth.shape == (3, H, W) and shade.shape == (3, H, W, 3) and (shade[depth == 0] == 255).all()
    # the rendered TSDF mesh lies on the depth maps it was fused from, where both exist
    both = (depth > 0) & (np.stack([v["depth"] for v in scan_folder["scene"]["views"]]) > 0)
    ref = np.stack([v["depth"] for v in scan_folder["scene"]["views"]])
    assert both.sum() > 500 and np.median(np.abs(depth - ref)[both]) < FOLDER_VOXEL


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors(scan_folder, tmp_path):
    s = _scene(12, 24)
    verts, faces = torch.from_numpy(s["verts"]).to(DEV), torch.from_numpy(s["faces"]).to(DEV)
    views = mv.cameras(17)
    mats = svs_views.mats(views, DEV)
    zbuf = meshview.new_zbuf(17, H, W)
    work = torch.zeros(4 + 17 * len(faces), dtype=torch.int32, device=DEV)
    rc, _ = meshview.raster_raw(zbuf, verts, faces, mats, 17, H, W, work=work)
    assert rc < 0
    with pytest.raises(SvsError, match="svs_mesh_raster.*16"):
        lib.check(rc, "svs_mesh_raster")
    torch.cuda.synchronize()
    assert bool((zbuf == -1).all())                             # nothing ran
    rc, _ = meshview.raster_raw(zbuf[:1], verts, faces, mats, 1, H, W, near=0.0)
    with pytest.raises(SvsError, match="svs_mesh_raster: near"):
        lib.check(rc, "svs_mesh_raster")
    with pytest.raises(ValueError, match="svs_mesh_raster"):
        meshview.rasterize(verts, faces, views[:1], H, W, near=-1.0)
    depth = torch.zeros((17, H, W), device=DEV)
    seen = torch.zeros(len(verts), dtype=torch.int32, device=DEV)
    rc = meshview.visibility_raw(verts, mats, 17, H, W, depth, None, 0.01, 0.0, seen, seen.clone())
    with pytest.raises(SvsError, match="svs_mesh_vertex_visibility.*16"):
        lib.check(rc, "svs_mesh_vertex_visibility")
    for kw in (dict(rel=-0.01), dict(abs_tol=-1.0)):
        with pytest.raises(ValueError, match="svs_mesh_vertex_visibility"):
            meshview.visibility(verts, views[:3], depth[:3], **kw)
        rc = meshview.visibility_raw(verts, mats, 3, H, W, depth, None, kw.get("rel", 0.01), kw.get("abs_tol", 0.0), seen, seen.clone())
        with pytest.raises(SvsError, match="svs_mesh_vertex_visibility"):
            lib.check(rc, "svs_mesh_vertex_visibility")
    assert int(seen.sum()) == 0
    with pytest.raises(ValueError, match="svs_mesh_raster_resolve.*colours"):
        meshview.rasterize(verts, faces, views[:1], H, W, colors=s["colors"][:-1], shade=True)
    with pytest.raises(ValueError, match="masks"):
        meshview.visibility(verts, views[:3], depth[:3], masks=[None])
    # views of different sizes
    import shutil
    from PIL import Image
    folder = tmp_path / "scan106"
    shutil.copytree(scan_folder["folder"], folder)
    Image.fromarray(np.zeros((40, 64, 3), np.uint8)).save(folder / "images" / f"{VIEW_IDS[1]:08}.jpg")
    with pytest.raises(ValueError, match="svs_mesh_raster.*different sizes"):
        meshview.view_folder(scan_folder["ply"], str(folder), str(tmp_path / "out"), VIEW_IDS)
    # an empty mesh is not an error
    res = meshview.rasterize(verts, faces[:0], views[:2], H, W, normals=True, shade=True)
    assert bool((res["face"] == -1).all()) and bool((res["depth"] == 0).all()) and bool((res["shade"] == 255).all())
