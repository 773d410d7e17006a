"""svs_hip.tsdf on the GPU against the float64 oracle (tests/tsdf_oracle.py): the integration at the kernel's dispatch edges
and pixel cases, the face rule, the vertex colours, the sphere scene end to end, the folder path, the command, the runner
switch and the error paths.

Comparison rule: outside the oracle's `fragile` voxels (a decision within 1e-9 of flipping; at most 0.1 % of a volume)
the weight is exactly the oracle's and tsdf / every colour channel is within 2**-23: one float32 rounding of a value of
magnitude <= 1, plus float64 noise that may move that rounding by one unit."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import mesh_oracle as mo
import tsdf_oracle as to
from svs_hip import lib, mesh, tsdf
from svs_hip.lib import SvsError

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                                              # unit roundoff of float32
TOL = 2.0 ** -23
DEV = "cuda"
SPHERE = ((33, 35, 67), 0.05)


def _views(n_views, H=48, W=64, seed=0, wall=None):
    """the scene's three cameras, then perturbed copies of them.  wall: the depth of the pixels that miss the sphere (a plane
    in front of every camera, through the volume's middle), so that a thin volume is observed along its whole length"""
    rng = np.random.default_rng(seed)
    eyes = [to.SPHERE_EYES[i % 3] for i in range(n_views)]
    eyes = [tuple(np.asarray(e) + (0.0 if i < 3 else 1.0) * rng.uniform(-0.15, 0.15, 3)) for i, e in enumerate(eyes)]
    views = to.sphere_scene(SPHERE[0], SPHERE[1], H, W, eyes=eyes)["views"]
    if wall is not None:
        for v in views:
            v["depth"] = np.where(v["depth"] > 0, v["depth"], np.float32(wall)).astype(np.float32)
    return views


def _origin(shape, voxel):
    return -voxel * (np.asarray(shape, np.float64) - 1) / 2 + np.array([0.003, -0.002, 0.001])


def _gpu_volume(shape, origin, voxel, trunc, launches, colors=True):
    vol = tsdf.Volume(origin, shape, voxel, trunc, colors=colors)
    for views in launches:
        vol.integrate(views)
    return vol


def _compare(vol, launches, colors=True, what=""):
    want_t, want_w, want_c, fragile = to.integrate_f32(vol.shape, vol.origin, vol.voxel, vol.trunc, launches, colors=colors)
    got_t, got_w = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
    ok = ~fragile
    n_frag = int(fragile.sum())
    assert n_frag <= 0.001 * fragile.size, f"{n_frag} fragile voxels of {fragile.size}"
    seen = int((want_w > 0).sum())
    err_t = float(np.abs(got_t.astype(np.float64) - want_t)[ok].max())
    err_c = 0.0
    if colors:
        got_c = vol.rgb.cpu().numpy()
        err_c = float(np.abs(got_c.astype(np.float64) - want_c)[:, ok].max())
    print(f"{what}{vol.shape}: {seen} of {fragile.size} voxels observed, {n_frag} fragile, "
          f"tsdf error {err_t / TOL:.3f} of the bound, colour error {err_c / TOL:.3f}")
    assert np.array_equal(got_w[ok], want_w[ok])
    assert err_t <= TOL and err_c <= TOL
    unseen = (got_w == 0) & ok
    assert (got_t[unseen] == 1).all()                       # unobserved voxels still hold (1, 0)
    if colors:
        assert (got_c[:, unseen] == 0).all()
    return seen


# ---- integrate ---------------------------------------------------------------------------------------------------------
# the last axis around multiples of 4 and 64, voxel counts off 256; a column through the sphere along z
@pytest.mark.parametrize("shape,voxel", [((5, 7, 63), 0.05), ((3, 5, 64), 0.05), ((3, 4, 65), 0.05), ((2, 3, 257), 0.0125),
                                         ((33, 35, 67), 0.05)])
@pytest.mark.parametrize("colors", [True, False])
def test_integrate_shapes(shape, voxel, colors):
    views = _views(3, wall=2.1)
    vol = _gpu_volume(shape, _origin(shape, voxel), voxel, 3 * voxel, [views], colors)
    _compare(vol, [views], colors)
    assert vol.launches == 1
    # the input reaches every store path: groups of four consecutive voxels fully, partly and not observed, and a last group
    # of fewer than four where the voxel count is no multiple of 4
    w = vol.weight.cpu().numpy().reshape(-1)
    full = (w[:len(w) // 4 * 4].reshape(-1, 4) > 0).sum(1)
    assert (full == 4).any() and ((full > 0) & (full < 4)).any() and (full == 0).any()


@pytest.mark.parametrize("shape", [(3, 3, 7), (1, 2, 3), (1, 1, 5), (1, 1, 2)])
def test_integrate_last_group_of_fewer_than_four(shape):
    """small volumes on the sphere's surface towards the first camera: every voxel is observed, the last 3, 2 or 1 of
    them (or the only 2) by the scalar group behind the 16-byte ones"""
    views = _views(3)
    voxel = 0.05
    origin = np.array([0.556, 0.047, 0.187]) - voxel * (np.asarray(shape, np.float64) - 1) / 2
    vol = _gpu_volume(shape, origin, voxel, 3 * voxel, [views])
    assert _compare(vol, [views], what="last group ") == vol.tsdf.numel() and vol.tsdf.numel() % 4 != 0


@pytest.mark.parametrize("n_views", [1, 3, 16])
@pytest.mark.parametrize("size", [(48, 64), (37, 53)])
def test_integrate_view_counts_and_image_sizes(n_views, size):
    views = _views(n_views, *size, wall=2.1)
    shape, voxel = (9, 10, 67), 0.05
    vol = _gpu_volume(shape, _origin(shape, voxel), voxel, 3 * voxel, [views])
    assert _compare(vol, [views], what=f"{n_views} views {size} ") > 0
    assert vol.launches == 1


def _spoiled(views, seed=3):
    """masks on two of three views, and patches of 0, -1, inf and NaN in the depth maps"""
    rng = np.random.default_rng(seed)
    out = []
    for i, v in enumerate(views):
        d = v["depth"].copy()
        H, W = d.shape
        for k, bad in enumerate((0.0, -1.0, np.inf, np.nan)):
            y, x = H // 4 + 6 * k, W // 3 + 3 * i
            d[y:y + 4, x:x + 12] = bad
        v = dict(v, depth=d)
        if i != 1:
            v["mask"] = (rng.random((H, W)) > 0.3).astype(np.uint8)
        out.append(v)
    return out


@pytest.mark.parametrize("colors", [True, False])
def test_integrate_masks_and_bad_depth_pixels(colors):
    views = _spoiled(_views(3))
    shape, voxel = SPHERE
    vol = _gpu_volume(shape, _origin(shape, voxel), voxel, 3 * voxel, [views], colors)
    seen = _compare(vol, [views], colors, what="masks + bad pixels ")
    clean = to.integrate_f32(shape, _origin(shape, voxel), voxel, 3 * voxel, [_views(3)], colors=False)[1]
    assert 0 < seen < int((clean > 0).sum())                # the masks and the bad pixels did remove observations


def test_integrate_camera_inside_the_volume():
    shape, voxel = SPHERE
    eye = (0.1, 0.05, 1.2)                                  # inside the volume (|z| <= 1.65), outside the sphere
    views = to.sphere_scene(shape, voxel, eyes=(eye,) + to.SPHERE_EYES[:1])["views"]
    origin = _origin(shape, voxel)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    z = (origin + idx * voxel) @ views[0]["E"][2, :3] + views[0]["E"][2, 3]
    assert (z <= 0).sum() > 1000 and (z > 0).sum() > 1000   # voxels behind the first camera and in front of it
    vol = _gpu_volume(shape, origin, voxel, 3 * voxel, [views])
    _compare(vol, [views], what="camera inside ")


def test_two_launches_equal_the_oracle_launch_by_launch():
    views = _views(5, seed=4)
    shape, voxel = SPHERE
    launches = [views[:3], _spoiled(views[2:], seed=5)]
    vol = _gpu_volume(shape, _origin(shape, voxel), voxel, 2.5 * voxel, launches)
    _compare(vol, launches, what="two launches ")
    assert vol.launches == 2 and float(vol.weight.max()) >= 3


def test_more_than_sixteen_views_are_chunked():
    views = _views(19, seed=6, wall=2.1)
    shape, voxel = (3, 4, 65), 0.05
    vol = _gpu_volume(shape, _origin(shape, voxel), voxel, 3 * voxel, [views])
    assert vol.launches == 2
    _compare(vol, [views[:16], views[16:]], what="19 views ")


# ---- the sphere: one GPU volume and one oracle pipeline for the tests below ----------------------------------------------
_CACHE = {}


def _sphere():
    if not _CACHE:
        shape, voxel = SPHERE
        sc = to.sphere_scene(shape, voxel)
        vol = _gpu_volume(shape, sc["origin"], voxel, sc["trunc"], [sc["views"]])
        o_t, o_w, o_c, _ = to.integrate_f32(shape, sc["origin"], voxel, sc["trunc"], [sc["views"]])
        _CACHE.update(scene=sc, vol=vol, o_tsdf=o_t, o_weight=o_w, o_rgb=o_c)
    return _CACHE


def test_face_keep_is_the_oracles_rule():
    s = _sphere()
    vol = s["vol"]
    verts, faces, cells = mesh.marching_cubes(vol.tsdf, 0.0, (1.0, 1.0, 1.0), return_cells=True)
    v2, f2 = mesh.marching_cubes(vol.tsdf, 0.0, (1.0, 1.0, 1.0))
    assert torch.equal(verts, v2) and torch.equal(faces, f2)                    # the default path returns what it returned
    assert cells.dtype == torch.int32 and cells.shape == (faces.shape[0],)
    got_t, got_w = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
    assert np.array_equal(cells.cpu().numpy(), to.mc_cells(got_t, 0.0))
    counts = {}
    for min_weight in (1, 2):
        keep = tsdf.face_keep(vol.weight, cells, min_weight).cpu().numpy()
        want = to.face_keep(got_w, cells.cpu().numpy(), min_weight)
        assert np.array_equal(keep.astype(bool), want)
        counts[min_weight] = int(keep.sum())
    print(f"faces {faces.shape[0]}, kept at min_weight 1 / 2: {counts[1]} / {counts[2]}")
    assert 0 < counts[2] < counts[1] < faces.shape[0]
    assert bool(tsdf.face_keep(vol.weight, cells, 0).all())


def test_vertex_colors_match_the_oracle():
    s = _sphere()
    vol = s["vol"]
    n = np.asarray(vol.shape)
    verts = mesh.marching_cubes(vol.tsdf, 0.0, (1.0, 1.0, 1.0))[0]
    rng = np.random.default_rng(9)
    extra = rng.uniform(0, 1, (400, 3)) * (n - 1)
    extra[:120, 0] = n[0] - 1                                # on the volume's upper faces, edges and corner
    extra[60:180, 1] = n[1] - 1
    extra[150:240, 2] = n[2] - 1
    extra[240:260] = np.floor(extra[240:260])                # on nodes
    extra[260] = n - 1
    extra[261] = 0
    pts = torch.cat([verts, torch.from_numpy(extra.astype(np.float32)).to(DEV)])
    got = tsdf.vertex_colors(vol.rgb, vol.weight, pts).cpu().numpy()
    want = to.vertex_colors(vol.rgb.cpu().numpy(), vol.weight.cpu().numpy(), pts.cpu().numpy())
    err = float(np.abs(got - want).max())
    print(f"{len(pts)} vertices: colour error {err / TOL:.3f} of the bound; {int((want.sum(1) == 0).sum())} without an observed node")
    assert got.shape == (len(pts), 3) and err <= TOL
    assert (want.sum(1) == 0).any() and (want.sum(1) > 0).any()


def _canon(faces):
    """faces as a sorted list of triples, each rotated to start at its smallest entry (orientation kept)"""
    f = np.asarray(faces, np.int64)
    r = np.argmin(f, 1)
    rows = np.arange(len(f))
    return sorted(zip(f[rows, r].tolist(), f[rows, (r + 1) % 3].tolist(), f[rows, (r + 2) % 3].tolist()))


def _position_bound(shape, sp, origin):
    """|gpu - float64| per axis.  Marching cubes, as tests/test_gpu_mesh.py derives it: t = fl(fl(level - v0) / fl(v1 - v0)),
    three roundings without cancellation, |dt| < 4u; the coordinate fl(fl(i s) + fl(t s)) is off by u (2 P + 5 s) with
    P = (n - 1) s, one more u s for the float64 side: u (2 P + 6 s).  The shift fl(p + origin) adds one rounding of a
    coordinate of magnitude <= |origin| + P."""
    return np.array([U * (2 * (n - 1) * s + 6 * s) + U * (abs(o) + (n - 1) * s) for n, s, o in zip(shape, sp, origin)])


def _oracle_pipeline(s, min_weight=1):
    sc = s["scene"]
    voxel = sc["voxel"]
    verts, faces, _ = mo.marching_cubes(s["o_tsdf"].astype(np.float64), 0.0, (voxel,) * 3)
    keep = to.face_keep(s["o_weight"], to.mc_cells(s["o_tsdf"], 0.0), min_weight)
    verts, faces, _ = to.compact(verts, faces[keep])
    col = to.colors_u8(to.vertex_colors(s["o_rgb"], s["o_weight"], verts / voxel))
    return verts + sc["origin"], faces, col


def test_sphere_end_to_end():
    s = _sphere()
    sc, vol = s["scene"], s["vol"]
    want_v, want_f, want_c = _oracle_pipeline(s)
    v, f, c = vol.mesh()
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and c.dtype == torch.uint8
    v, f, c = v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy()
    assert v.shape == want_v.shape and c.shape == want_c.shape
    assert _canon(f) == _canon(want_f)                       # same vertex order (grid edge order), so equal triples are equal faces
    ratio = float((np.abs(v.astype(np.float64) - want_v) / _position_bound(vol.shape, (vol.voxel,) * 3, vol.origin)).max())
    dc = int(np.abs(c.astype(np.int64) - want_c.astype(np.int64)).max())
    dist = np.abs(np.linalg.norm(v - sc["centre"], axis=1) - sc["radius"]).max() / vol.voxel
    print(f"sphere: {len(v)} vertices, {len(f)} faces, worst position error / bound {ratio:.3f}, colour codes within {dc}, "
          f"within {dist:.2f} voxel of the sphere")
    assert ratio <= 1.0 and dc <= 1 and dist <= 1.0
    # largest=True: one of the three caps, the one with the largest area
    v1, f1, c1 = vol.mesh(largest=True)
    assert 0 < f1.shape[0] < len(f) and c1.shape[0] == v1.shape[0]
    assert len(np.unique(mo.vertex_labels(len(v1), f1.cpu().numpy()))) == 1
    # without colours
    plain = _gpu_volume(vol.shape, vol.origin, vol.voxel, vol.trunc, [[dict(x, img=None) for x in sc["views"]]], colors=False)
    v2, f2, c2 = plain.mesh()
    assert c2 is None and np.array_equal(v2.cpu().numpy(), v) and np.array_equal(f2.cpu().numpy(), f)


# ---- folder, command, runner ---------------------------------------------------------------------------------------------
VIEW_IDS = (25, 22, 28)                                      # the runner's training views of a DTU scan
NEAR_EYES = ((2.03, 0.31, 0.42), (1.9, 0.62, 0.5), (1.95, 0.0, 0.28))         # neighbours, as a scan's training views are
FOLDER_VOXEL = 0.05


@pytest.fixture(scope="module")
def scan_folder(tmp_path_factory):
    """{root}/scan106 with cams/, images/, depth_est/, confidence/ written by the project's own writers"""
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


def _check_mesh_file(ply, v, f, c, sc, voxel):
    from svs_hip import clouds
    from svs_hip.ply import read_mesh, read_points
    rv, rf = read_mesh(ply)
    assert np.array_equal(rv, v.astype(np.float64)) and np.array_equal(rf, f)
    assert np.array_equal(read_points(ply)[1], c)
    assert len(f) > 0 and f.min() >= 0 and f.max() < len(v)
    pts = clouds.sample_mesh(rv, rf, voxel / 2)
    assert pts.shape[0] > len(v) and pts.shape[1] == 3 and bool(torch.isfinite(pts).all())
    # the averaged depth of a surviving pixel is within filter_diff = 1 % of the view's own, which is exact: the surface moves
    # by at most 0.01 * depth along the ray, on top of the one voxel of the grid (tests/test_tsdf_cpu.py)
    far = max(float(x["depth"].max()) for x in sc["views"])
    dist = float(np.abs(np.linalg.norm(v - sc["centre"], axis=1) - sc["radius"]).max())
    print(f"{ply}: {len(v)} vertices, {len(f)} faces, within {dist / voxel:.2f} voxel of the sphere")
    assert dist <= voxel + 0.01 * far
    return pts


def test_fuse_folder(scan_folder):
    folder, sc = str(scan_folder["folder"]), scan_folder["scene"]
    v, f, c, stats = tsdf.fuse_folder(folder, folder, VIEW_IDS, FOLDER_VOXEL)
    assert stats["file"] == os.path.join(folder, "tsdf.ply") and stats["launches"] == 1
    assert stats["n_verts"] == len(v) and stats["n_faces"] == len(f) and c.dtype == np.uint8
    assert list(stats["seconds"]) == ["read", "filter", "bounds", "integrate", "scan", "classify", "emit", "keep", "colors",
                                      "download", "write"]
    assert all(x >= 0 for x in stats["seconds"].values()) and stats["seconds"]["integrate"] > 0
    # default bounds: the fused points padded by trunc + voxel
    lo, hi = stats["origin"], stats["origin"] + (np.asarray(stats["shape"]) - 1) * FOLDER_VOXEL
    assert (v.min(0) >= lo).all() and (v.max(0) <= hi).all()
    _check_mesh_file(stats["file"], v, f, c, sc, FOLDER_VOXEL)
    assert c.astype(int).sum(1).min() > 0                    # every vertex took a colour from a view
    with pytest.raises(ValueError, match="voxels"):
        tsdf.fuse_folder(folder, folder, VIEW_IDS, FOLDER_VOXEL, max_voxels=1000)
    with pytest.raises(ValueError, match="depth"):
        tsdf.fuse_folder(folder, folder, VIEW_IDS, FOLDER_VOXEL, depth="median")


def test_command_raw_bounds_largest(scan_folder):
    folder, sc = str(scan_folder["folder"]), scan_folder["scene"]
    ply = str(scan_folder["root"] / "cmd" / "raw.ply")
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        v, f, c, stats = tsdf.main(["--scan-folder", folder, "--out-folder", folder, "--views", *map(str, VIEW_IDS), "--voxel",
                                    "0.0625", "--trunc", "0.15", "--bounds", "-0.75", "-0.875", "-0.625", "0.75", "0.625", "0.875",
                                    "--raw", "--largest", "--ply", ply])
    assert stats["file"] == ply and "seconds: read" in text.getvalue() and ply in text.getvalue()
    assert np.array_equal(stats["origin"], [-0.75, -0.875, -0.625]) and stats["shape"] == (25, 25, 25)      # exact in binary
    _check_mesh_file(ply, v, f, c, sc, 0.0625)
    assert len(np.unique(mo.vertex_labels(len(v), f))) == 1


def test_runner_switch(scan_folder):
    from svs_hip import clouds, run
    from svs_hip.ply import read_mesh
    root = scan_folder["root"]
    base = [f"outdir={root}", "filter_only=true", "eval_mask=false", "testlist=scan106"]
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base)
    assert "meshes" not in res and not os.path.exists(root / "tsdf") and "tsdf seconds" not in text.getvalue()
    cloud = open(root / "mvsnet106_l3.ply", "rb").read()
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base + [f"+tsdf_voxel={FOLDER_VOXEL}", "+tsdf_trunc=0.12"])
    ply = root / "tsdf" / "mvsnet106_l3.ply"
    assert os.path.exists(ply) and open(root / "mvsnet106_l3.ply", "rb").read() == cloud
    assert text.getvalue().count("scan106 tsdf seconds: read ") == 1
    stats = res["meshes"]["scan106"]
    rv, rf = read_mesh(str(ply))
    assert len(rv) == stats["n_verts"] > 0 and len(rf) == stats["n_faces"] > 0
    assert clouds.sample_mesh(rv, rf, 0.025).shape[0] > len(rv)


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors():
    shape, voxel = (3, 4, 65), 0.05
    views = _views(17, seed=7)
    vol = tsdf.Volume(_origin(shape, voxel), shape, voxel)
    assert vol.trunc == 3 * voxel
    depths = [torch.from_numpy(v["depth"]).to(DEV) for v in views]
    images = [torch.from_numpy(v["img"]).to(DEV) for v in views]
    mats = torch.from_numpy(np.stack([tsdf.view_matrices(v["K"], v["E"]) for v in views])).to(DEV)
    rc = tsdf.integrate_raw(vol.tsdf, vol.weight, vol.rgb, vol.origin, voxel, vol.trunc, depths, None, images, mats, 48, 64)
    assert rc < 0
    with pytest.raises(SvsError, match="16"):
        lib.check(rc, "svs_tsdf_integrate")
    torch.cuda.synchronize()
    assert float(vol.weight.sum()) == 0 and bool((vol.tsdf == 1).all())          # nothing ran
    small = dict(views[1], depth=views[1]["depth"][:-1], img=views[1]["img"][:-1])
    with pytest.raises(AssertionError):
        vol.integrate([views[0], small])
    with pytest.raises(AssertionError):
        vol.integrate([dict(views[0], img=views[0]["img"][:, :-1])])
    with pytest.raises(AssertionError):
        vol.integrate([dict(views[0], mask=np.ones((5, 5), np.uint8))])
    with pytest.raises(ValueError):
        vol.mesh()                                           # nothing integrated: no crossing
    s = _sphere()
    with pytest.raises(ValueError, match="kept"):
        s["vol"].mesh(min_weight=100)
    with pytest.raises(ValueError):
        tsdf.Volume((0, 0, 0), (4, 4, 4), 0.0)
