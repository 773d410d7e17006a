"""svs_hip.mesh on the GPU against the float64 oracle (tests/mesh_oracle.py): marching cubes on analytic volumes and at the
classify tile's edges, components, the half-space clip, the chunked grid SDF and one end-to-end surface."""
import numpy as np
import pytest
import torch

import mesh_oracle as mo
from svs_hip import mesh
from svs_hip.lib import SvsError

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                                              # unit roundoff of float32
DEV = "cuda"


def _coords(shape, spacing):
    return np.meshgrid(*[np.arange(n) * s for n, s in zip(shape, spacing)], indexing="ij")


def _sphere(shape, spacing, centre, radius):
    x, y, z = _coords(shape, spacing)
    return np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius


def _volumes():
    out = {}
    sp = (0.5, 0.25, 0.375)
    out["sphere"] = (_sphere((24, 20, 28), sp, (5.3, 2.4, 5.1), 2.0), 0.0, sp, 2)
    x, y, z = _coords((24, 24, 16), (1, 1, 1))
    q = np.sqrt((x - 11.5) ** 2 + (y - 11.5) ** 2) - 7.0
    out["torus"] = (np.sqrt(q ** 2 + (z - 7.5) ** 2) - 2.6, 0.0625, (1.0, 1.0, 1.0), 0)
    one = (1.0, 1.0, 1.0)
    three = np.minimum(np.minimum(_sphere((28, 20, 20), one, (6, 9, 9), 4.2), _sphere((28, 20, 20), one, (19, 10, 10), 4.5)),
                       _sphere((28, 20, 20), one, (12.5, 3, 3), 1.3))
    out["three"] = (three, 0.0, one, 6)
    x, y, z = _coords((12, 11, 9), one)
    out["plane"] = (x + y - 10.0, 0.0, (0.5, 2.0, 1.0), None)          # values equal the level at grid nodes
    return {k: (np.ascontiguousarray(v[0], np.float32),) + v[1:] for k, v in out.items()}


VOLUMES = _volumes()
_CACHE = {}


def _oracle(name):
    if name not in _CACHE:
        vol, level, sp, _ = VOLUMES[name]
        _CACHE[name] = mo.marching_cubes(vol.astype(np.float64), level, sp)
    return _CACHE[name]


def _gpu(vol, level, sp):
    v, f = mesh.marching_cubes(torch.from_numpy(vol).to(DEV), level, sp)
    return v, f


def _canon(faces):
    """faces as a sorted list of triples, each rotated to start at its smallest entry (orientation kept)"""
    f = np.asarray(faces, np.int64)
    r = np.argmin(f, 1)
    rows = np.arange(len(f))
    return sorted(zip(f[rows, r].tolist(), f[rows, (r + 1) % 3].tolist(), f[rows, (r + 2) % 3].tolist()))


def _position_bound(shape, sp):
    """|gpu - float64| per axis.  t = fl(fl(level - v0) / fl(v1 - v0)): three roundings, no cancellation (the ends differ in
    sign), |dt| <= 3u(1 + u)^2 t < 4u.  The coordinate fl(fl(i s) + fl(t s)): u |i s| for the first product,
    (4u + u) s for the second, u |p| for the sum, with |i s|, |p| <= P = (n - 1) s:  u (2 P + 5 s); one more u s covers
    the float64 side and the second-order terms."""
    return np.array([U * (2 * (n - 1) * s + 6 * s) for n, s in zip(shape, sp)])


def _check_against_oracle(vol, level, sp, oracle=None):
    ov, of, keys = oracle if oracle is not None else mo.marching_cubes(vol.astype(np.float64), level, sp)
    v, f = _gpu(vol, level, sp)
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    assert v.shape[0] == len(ov) and f.shape[0] == len(of)
    # vertices come in the order of their grid edge (node index, then axis), which is the oracle's key order: vertex i of
    # both sits on grid edge keys[i], so equal index triples are equal grid-edge triples; the positions confirm it
    gf = f.cpu().numpy()
    assert _canon(keys[gf]) == _canon(keys[of])
    err = np.abs(v.cpu().numpy().astype(np.float64) - ov)
    ratio = float((err / _position_bound(vol.shape, sp)).max()) if len(ov) else 0.0
    print(f"marching cubes {vol.shape}: {len(ov)} vertices, {len(of)} faces, worst position error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    return v, f


@pytest.mark.parametrize("name", list(VOLUMES))
def test_analytic_volume_matches_the_oracle(name):
    vol, level, sp, euler = VOLUMES[name]
    v, f = _check_against_oracle(vol, level, sp, _oracle(name))
    if euler is not None:
        gf = f.cpu().numpy()
        assert mo.is_closed_oriented_manifold(gf)
        assert mo.euler_characteristic(gf) == euler
        assert mo.signed_volume(v.cpu().numpy(), gf) > 0
    v2, f2 = _gpu(vol, level, sp)
    assert torch.equal(v.view(torch.int32), v2.view(torch.int32)) and torch.equal(f, f2)


def _smooth(shape, seed):
    rng = np.random.default_rng(seed)
    x, y, z = _coords(shape, (1, 1, 1))
    a = rng.uniform(0.3, 1.1, 3)
    p = rng.uniform(0, 6, 3)
    return (np.sin(a[0] * x + p[0]) + np.sin(a[1] * y + p[1]) + np.sin(a[2] * z + p[2]) + 0.1).astype(np.float32)


def test_dispatch_edges():
    ti, tj, tk = mesh.classify_tile()
    shapes = [(2, 2, 2), (ti - 1, tj - 1, tk - 1), (ti + 1, tj + 1, tk + 1), (2, tj + 1, tk + 1), (ti + 1, 2, tk - 1),
              (ti - 1, tj + 1, 2), (2 * ti + 1, 2, 2)]
    for n, shape in enumerate(shapes):
        vol = _smooth(shape, n)
        if shape == (2, 2, 2):
            vol = np.array([[[-1, 1], [1, -1]], [[1, 1], [-1, 1]]], np.float32)
        _check_against_oracle(vol, 0.0, (1.0, 0.5, 0.25))


def test_transposed_view_is_taken_as_it_is():
    vol = _smooth((9, 7, 11), 5)
    t = torch.from_numpy(vol).to(DEV)
    v0, f0 = mesh.marching_cubes(t.permute(1, 0, 2), 0.0, (1, 1, 1))
    v1, f1 = mesh.marching_cubes(t.permute(1, 0, 2).contiguous(), 0.0, (1, 1, 1))
    assert torch.equal(v0, v1) and torch.equal(f0, f1) and f0.shape[0] > 0


def test_no_crossing_raises():
    vol = torch.ones(5, 6, 7, device=DEV)
    with pytest.raises(ValueError):
        mesh.marching_cubes(vol, 0.0)
    with pytest.raises(ValueError):
        mesh.marching_cubes(-vol, 0.0)


def test_level_touched_but_never_crossed_raises():
    """the range holds the level, no value lies below it: no grid edge changes sign, so there is no surface"""
    vol = torch.ones(5, 6, 7, device=DEV)
    vol[2, 3, 4] = 0.0
    with pytest.raises(ValueError):
        mesh.marching_cubes(vol, 0.0)
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.zeros(4, 4, 4, device=DEV), 0.0)


def test_every_cell_active():
    i, j, k = np.meshgrid(np.arange(7), np.arange(6), np.arange(9), indexing="ij")
    vol = np.where((i + j + k) % 2 == 0, -1.0, 1.0).astype(np.float32)
    _, f = _check_against_oracle(vol, 0.0, (1.0, 1.0, 1.0))
    assert f.shape[0] >= 6 * 5 * 8                           # no cell without a triangle


# ---- components ------------------------------------------------------------------------------------------------------
def test_components_match_the_oracle_partition():
    ov, of, _ = _oracle("three")
    faces = torch.from_numpy(of.astype(np.int32)).to(DEV)
    verts = torch.from_numpy(ov.astype(np.float32)).to(DEV)
    labels = mesh.vertex_labels(faces, len(ov)).cpu().numpy()
    assert np.array_equal(labels, mo.vertex_labels(len(ov), of))
    assert len(np.unique(labels)) == 3
    v, f = mesh.largest_component(verts, faces)
    keep = mo.largest_component_faces(ov.astype(np.float32), of)
    assert f.shape[0] == len(keep)
    got = v.cpu().numpy()[f.cpu().numpy()]
    want = ov.astype(np.float32)[of[keep]]
    assert np.array_equal(got, want)                         # the same triangles in the same order, vertices re-indexed
    area = mesh.face_areas(verts, faces).cpu().numpy()
    assert np.allclose(area, mo.face_areas(ov.astype(np.float32), of), rtol=1e-12, atol=0)


def test_long_thin_helix_converges_within_the_bound():
    """a strip of 6000 triangles wound into a helix, vertex ids shuffled: the minimum label has to travel the whole strip"""
    n = 3001
    t = np.linspace(0, 60 * np.pi, n)
    a = np.stack([np.cos(t), np.sin(t), 0.01 * t], 1)
    verts = np.concatenate([a, a + [0, 0, 0.05]]).astype(np.float32)
    i = np.arange(n - 1)
    faces = np.concatenate([np.stack([i, i + 1, i + n], 1), np.stack([i + 1, i + n + 1, i + n], 1)])
    perm = np.random.default_rng(11).permutation(2 * n)
    faces = perm[faces].astype(np.int32)
    ft = torch.from_numpy(faces).to(DEV)
    labels, rounds = mesh.vertex_labels(ft, 2 * n, return_rounds=True)
    print(f"helix: {rounds} rounds")
    assert rounds > 1 and bool((labels == 0).all())
    assert np.array_equal(labels.cpu().numpy(), mo.vertex_labels(2 * n, faces))
    with pytest.raises(SvsError):
        mesh.vertex_labels(ft, 2 * n, max_rounds=1)          # the bound: an error code, not a spin


# ---- clip ------------------------------------------------------------------------------------------------------------
def test_clip_sphere_by_a_box_through_it():
    ov, of, _ = _oracle("sphere")
    v32 = ov.astype(np.float32)
    lo, hi = np.array([3.7, 1.0, 3.3]), np.array([7.1, 3.9, 8.0])
    verts, faces = torch.from_numpy(v32).to(DEV), torch.from_numpy(of.astype(np.int32)).to(DEV)
    cv, cf = mesh.clip_to_box(verts, faces, lo, hi)
    cv, cf = cv.cpu().numpy(), cf.cpu().numpy()
    wv, wf = mo.clip_to_box(v32.astype(np.float64), of, lo, hi)
    assert len(cf) == len(wf) and len(cv) == len(wv)
    # triangles wholly inside: bit-identical coordinates
    inside = ((v32 >= lo) & (v32 <= hi)).all(1)
    whole = of[inside[of].all(1)]
    got = {tuple(r) for r in cv[cf].reshape(-1, 9).view(np.uint32).tolist()}
    assert len(whole) > 100 and all(tuple(r) in got for r in v32[whole].reshape(-1, 9).view(np.uint32).tolist())
    # every vertex inside the box, within 4 float32 ulps of the plane coordinate
    tol = 4 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(np.float32)).astype(np.float64)
    assert (cv >= lo - tol).all() and (cv <= hi + tol).all()
    # every boundary edge lies on a box plane: the weld left no seam inside
    edges = mo.boundary_edges(cf)
    assert len(edges) > 20
    for a, b in edges:
        on = [abs(cv[a, d] - p[d]) <= tol[d] and abs(cv[b, d] - p[d]) <= tol[d] for d in range(3) for p in (lo, hi)]
        assert any(on), (cv[a], cv[b])
    # area against the float64 clip.  A vertex is rounded to float32 when it is made and again by each later cut that
    # moves it: at most 3 roundings of coordinates below P = 14, each u P, and the cut parameter of a later plane sees
    # ends perturbed by as much: delta = 8 u P per vertex.  A triangle's area moves by at most its perimeter times delta.
    P = 14.0
    tri = wv[wf]
    perimeter = sum(np.linalg.norm(tri[:, i] - tri[:, (i + 1) % 3], axis=1) for i in range(3)).sum()
    got_area, want_area = mo.face_areas(cv, cf).sum(), mo.face_areas(wv, wf).sum()
    print(f"clip: {len(cf)} faces, area {got_area:.6f} vs {want_area:.6f}, error / bound = "
          f"{abs(got_area - want_area) / (8 * U * P * perimeter):.4f}")
    assert abs(got_area - want_area) <= 8 * U * P * perimeter


def test_clip_that_keeps_nothing_or_everything():
    ov, of, _ = _oracle("sphere")
    verts, faces = torch.from_numpy(ov.astype(np.float32)).to(DEV), torch.from_numpy(of.astype(np.int32)).to(DEV)
    v, f = mesh.clip_halfspace(verts, faces, [100.0, 0, 0], [1.0, 0, 0])         # the whole mesh lies outside
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and f.dtype == torch.int32
    v, f = mesh.clip_halfspace(v, f, [0.0, 0, 0], [1.0, 0, 0])                   # and an empty mesh stays empty
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    v, f = mesh.clip_halfspace(verts, faces, [-100.0, 0, 0], [1.0, 0, 0])        # the whole mesh lies inside
    assert torch.equal(v, verts) and torch.equal(f, faces)


# ---- grid SDF ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def network():
    from volsdf.model.network import VolSDFNetwork
    from volsdf.utils.conf import dtu_model_conf
    torch.manual_seed(0)
    return VolSDFNetwork(dtu_model_conf()).to(DEV).eval().implicit_network


def _grid_9_7_11():
    return {"xyz": [np.linspace(-0.9, 0.9, 9), np.linspace(-0.7, 0.8, 7), np.linspace(-1.0, 1.0, 11)]}


def _reference_points(grid):
    xx, yy, zz = np.meshgrid(*grid["xyz"])                                              # plots.py:294-295
    return torch.tensor(np.vstack([xx.ravel(), yy.ravel(), zz.ravel()]).T, dtype=torch.float)


def test_grid_sdf_is_the_one_call_result(network):
    grid = _grid_9_7_11()
    with torch.no_grad():
        vol = mesh.grid_sdf(network, grid, split=100)                                   # 693 points: 6 chunks of 100 and 93
        pts = _reference_points(grid).to(DEV)
        assert torch.equal(mesh.grid_points(grid, 0, 693), pts)
        want = network.get_sdf_vals(pts)
    assert tuple(vol.shape) == (7, 9, 11)
    assert torch.equal(vol.reshape(-1).view(torch.int32), want.reshape(-1).view(torch.int32))


def test_grid_sdf_with_rotation_and_offset(network):
    grid = _grid_9_7_11()
    q = np.linalg.qr(np.random.default_rng(2).standard_normal((3, 3)))[0]
    vecs = torch.tensor(q, dtype=torch.float32)
    s_mean = torch.tensor([0.05, -0.1, 0.02])
    pnts = _reference_points(grid)
    want = torch.bmm(vecs.unsqueeze(0).repeat(pnts.shape[0], 1, 1).transpose(1, 2), pnts.unsqueeze(-1)).squeeze() + s_mean
    got = torch.cat([mesh.grid_points(grid, s, min(100, 693 - s), vecs, s_mean) for s in range(0, 693, 100)]).cpu()
    # three products and three additions per coordinate on either side, each within u of its exact value:
    # |error| <= 4 u (sum_j |vecs[j][i] p_j| + |s_i|) per side
    bound = 8 * U * (pnts.abs().double() @ vecs.abs().double() + s_mean.abs().double())
    ratio = float(((got.double() - want.double()).abs() / bound).max())
    print(f"rotated grid points: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    with torch.no_grad():
        vol = mesh.grid_sdf(network, grid, rotation=vecs, offset=s_mean, split=100)
        one = network.get_sdf_vals(got.to(DEV))
    assert torch.equal(vol.reshape(-1), one.reshape(-1))


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_surface_high_res_end_to_end(network, tmp_path):
    from svs_hip import clouds
    from svs_hip.ply import read_mesh
    with torch.no_grad():
        out = mesh.surface_high_res(network, resolution=32, grid_boundary=(-1.5, 1.5), coarse_resolution=32, n_samples=2000)
    assert out is not None
    verts, faces = out
    f = faces.cpu().numpy()
    assert mo.is_closed_oriented_manifold(f) and mo.euler_characteristic(f) == 2
    assert len(np.unique(mo.vertex_labels(verts.shape[0], f))) == 1
    assert mo.signed_volume(verts.cpu().numpy(), f) > 0
    radius = verts.norm(dim=1)
    assert float(radius.min()) > 0.3 and float(radius.max()) < 1.2           # the geometric initialisation's sphere
    fn = str(tmp_path / "mesh_0" / "scan1.ply")
    scale = np.diag([2.0, 2.0, 2.0, 1.0])
    scale[:3, 3] = [1.0, -2.0, 0.5]
    v, ff = mesh.finish_mesh(verts, faces, scale, fn)
    rv, rf = read_mesh(fn)
    assert np.array_equal(rv, v.astype(np.float64)) and np.array_equal(rf, ff.astype(np.int64))
    cloud = clouds.sample_mesh(rv, rf, 0.2)
    assert cloud.shape[0] >= len(rv) and cloud.shape[1] == 3


# ---- checkpoint -> file ------------------------------------------------------------------------------------------------
def _scan_folder(root, dataset, scan, scale):
    import os
    os.makedirs(os.path.join(root, dataset, f"scan{scan}", "image"))
    np.savez(os.path.join(root, dataset, f"scan{scan}", "cameras.npz"), scale_mat_0=scale, world_mat_0=np.eye(4))


def _checkpoint(root, model, epoch):
    import os
    os.makedirs(os.path.join(root, "checkpoints", "ModelParameters"))
    torch.save({"model_state_dict": model.state_dict(), "epoch": epoch},
               os.path.join(root, "checkpoints", "ModelParameters", "latest.pth"))
    return os.path.join(root, "checkpoints")


@pytest.mark.parametrize("dataset", ["DTU", "BlendedMVS"])
def test_extract_from_a_checkpoint(dataset, tmp_path):
    """extract() and the command line's arguments on a synthetic checkpoint of the geometric initialisation: the file of
    eval_vsdf.py:148-150, scale_mat applied, one component; DTU cut by its box (scan 82 reads 83's)."""
    import os
    from svs_hip.evalviews import build_model
    from svs_hip.ply import read_mesh
    root, scan = str(tmp_path), 82 if dataset == "DTU" else 1
    torch.manual_seed(0)
    ckpt = _checkpoint(root, build_model(dataset), 7)
    scale = np.diag([2.0, 2.0, 2.0, 1.0])
    scale[:3, 3] = [1.0, -2.0, 0.5]
    _scan_folder(root, dataset, scan, scale)
    if dataset == "DTU":
        np.savez(os.path.join(root, "DTU", "bbs.npz"), **{"83": np.array([[-0.6, -0.6, -0.6], [0.9, 0.9, 0.3]])})
    a = mesh.parse_args(["--ckpt", ckpt, "--data-dir-root", root, "--dataset", dataset, "--scan", str(scan), "--resolution", "32",
                         "--evals-folder", os.path.join(root, "evals"), "--expname", "t", "--grid-boundary", "-1.2", "1.2"])
    lines = []
    res = mesh.extract(a.ckpt, a.data_dir_root, a.dataset, a.scan, resolution=a.resolution, evals_folder=a.evals_folder,
                       expname=a.expname, checkpoint=a.checkpoint, level=a.level, grid_boundary=tuple(a.grid_boundary),
                       seed=a.seed, log=lines.append)
    assert res["file"] == os.path.join(root, "evals", f"t_{scan}", "mesh_7", f"scan{scan}.ply") and res["epoch"] == 7
    assert any(line.startswith("seconds: ") and "sdf" in line and "write" in line for line in lines)
    v, f = read_mesh(res["file"])
    assert len(v) == res["n_verts"] > 100 and len(f) == res["n_faces"] > 100
    assert len(np.unique(mo.vertex_labels(len(v), f))) == 1
    local = (v - scale[:3, 3]) / 2.0                                        # back to the model's frame
    r = np.linalg.norm(local, axis=1)
    assert 0.3 < r.min() and r.max() < 1.2                                  # the initial sphere, radius about 0.6
    if dataset == "DTU":
        assert local[:, 2].max() <= 0.3 + 1e-6 and len(mo.boundary_edges(f)) > 10       # cut open by the box at z = 0.3
        assert local[:, 2].min() < -0.4
    else:
        assert mo.is_closed_oriented_manifold(f) and mo.euler_characteristic(f) == 2
