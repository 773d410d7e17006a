"""svs_hip.poisson on the GPU against the float64 oracle (tests/poisson_oracle.py): the splat's counts and planes, divergence
and the operator at the stencil's dispatch edges on aligned and misaligned volumes, conjugate gradients against the oracle's
recurrence and a direct solve, sample / level / trim, the closed and the open surface end to end, files and the runner."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import mesh_oracle as mo
import poisson_oracle as po
import tsdf_oracle as to
from svs_hip import poisson as ps

pytestmark = pytest.mark.gpu
WORST = dict(splat=0.0, divergence=0.0, apply=0.0)


def _steps(got, want64):
    """|got - float32(want)| in float32 steps of float32(want)"""
    want = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _misaligned(a):
    """the same float32 values in a contiguous view that starts one element into its buffer: no 16-byte alignment"""
    buf = torch.empty(a.size + 5, dtype=torch.float32, device="cuda")
    view = buf[1:1 + a.size].view(a.shape)
    view.copy_(_dev(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


# ---- 1: splat ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(po.SPLAT_GRIDS) + ["segment"])
def test_splat_parity(name):
    pts, nrm, dims, origin, h = po.segment_case() if name == "segment" else po.splat_case(name)
    want, counted, skipped = po.splat(pts, nrm, dims, origin, h)
    field, c, s = ps.splat(pts, nrm, dims, origin, h)
    got = field.cpu().numpy()
    assert (c, s) == (counted, skipped) and got.shape == want.shape
    dev = _steps(got, want)
    WORST["splat"] = max(WORST["splat"], float(dev.max()))
    print(f"splat {name}: {len(pts)} points, {counted} counted, {skipped} skipped; worst deviation {dev.max():.3f} float32 steps "
          f"(so far {WORST['splat']:.3f}); equal bytes: {np.array_equal(got, want.astype(np.float32))}")
    assert np.isfinite(got).all() and (dev <= 1.0).all()
    again = ps.splat(pts, nrm, dims, origin, h)[0]
    assert torch.equal(field, again)                                             # the same bytes every run
    if name == "segment":
        assert (got[0] == 0).all() and got[3].sum() == 128.0


def test_splat_refuses_empty_and_all_skipped_clouds():
    with pytest.raises(ValueError, match="empty cloud"):
        ps.splat(np.zeros((0, 3)), np.zeros((0, 3), np.float32), (4, 4, 4), np.zeros(3), 1.0)
    far = np.array([[9.0, 1, 1], [np.nan, 1, 1], [1, 1, 3.0]])
    with pytest.raises(ValueError, match="all 3 points were skipped"):
        ps.splat(far, np.ones((3, 3), np.float32), (4, 4, 4), np.zeros(3), 1.0)
    with pytest.raises(ValueError, match="voxel"):
        ps.splat(far, np.ones((3, 3), np.float32), (4, 4, 4), np.zeros(3), 0.0)


# ---- 2: divergence and the operator -------------------------------------------------------------------------------------------------
def _shapes():
    return po.VOLUME_SHAPES + po.tile_shapes(ps.stencil_tile())


def test_divergence_parity():
    for n, shape in enumerate(_shapes()):
        field, h = po.random_volume(shape, 10 + n, planes=4), 0.5 + 0.25 * (n % 3)
        want = po.divergence(field, h)
        for how, put in (("aligned", _dev), ("misaligned", _misaligned)):
            got = ps.divergence(put(field), h).cpu().numpy()
            dev = _steps(got, want)
            WORST["divergence"] = max(WORST["divergence"], float(dev.max()))
            assert got.shape == tuple(shape) and (dev <= 1.0).all(), (shape, how, dev.max())
    print(f"divergence: {len(_shapes())} shapes, worst deviation {WORST['divergence']:.3f} float32 steps")


def test_apply_parity():
    assert ps.stencil_tile()[2] % 4 == 0
    for n, shape in enumerate(_shapes()):
        x, h = po.random_volume(shape, 40 + n), 0.5 + 0.25 * (n % 3)
        want = po.apply(x, h)
        for how, put in (("aligned", _dev), ("misaligned", _misaligned)):
            src = put(x)
            out = put(np.full(shape, np.nan, np.float32))
            got = ps.apply(src, h, out=out)
            assert got.data_ptr() == out.data_ptr() and src.data_ptr() % 16 == (0 if how == "aligned" else 4)
            dev = _steps(got.cpu().numpy(), want)
            WORST["apply"] = max(WORST["apply"], float(dev.max()))
            assert (dev <= 1.0).all(), (shape, how, dev.max())
        # what lies around a misaligned volume is left alone
        buf = torch.full((x.size + 5,), 7.0, dtype=torch.float32, device="cuda")
        ps.apply(_dev(x), h, out=buf[1:1 + x.size].view(shape))
        assert buf[0] == 7.0 and (buf[1 + x.size:] == 7.0).all()
    print(f"apply: {len(_shapes())} shapes, worst deviation {WORST['apply']:.3f} float32 steps")


# ---- 3: conjugate gradients ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", po.CG_GRIDS)
def test_cg_against_the_oracle_and_the_direct_solve(dims):
    s = po.sphere_solution(dims=dims)
    rhs64, tol = s["rhs"].astype(np.float64), 1e-4
    rhs = _dev(s["rhs"])
    x, info = ps.solve(rhs, 1.0, tol=tol, check_every=1)
    got = x.cpu().numpy().astype(np.float64)
    _, info64 = po.cg(rhs64, 1.0, tol=tol)
    direct = po.direct_solve(rhs64, 1.0)
    err = lambda v: float(np.linalg.norm(v - direct) / np.linalg.norm(direct))
    true = po.true_residual(got, rhs64, 1.0)
    e_gpu, e_emulated = err(got), err(s["x"].astype(np.float64))
    print(f"cg {dims}: {info['iterations']} iterations (oracle float64 {info64['iterations']}, float32 storage {s['info']['iterations']}), "
          f"recursive residual {info['residual']:.6e}, true {true:.6e} = {true / tol:.4f} tol; error against the direct solve "
          f"{e_gpu:.6e}, the oracle's float32-emulated CG {e_emulated:.6e}")
    assert info["converged"] and abs(info["iterations"] - info64["iterations"]) <= 2
    assert true <= 1.1 * tol
    assert e_gpu <= 2.0 * e_emulated
    again = ps.solve(rhs, 1.0, tol=tol, check_every=1)[0]
    assert torch.equal(x, again)                                                 # the same bytes every run
    # a right-hand side and a solution at an odd offset: the scalar path of the flat kernels, the same values
    odd = ps.solve(_misaligned(s["rhs"]), 1.0, tol=tol, check_every=1, out=_misaligned(np.zeros(dims, np.float32)))[0]
    assert torch.equal(odd, x)


@pytest.mark.parametrize("dims", po.CG_GRIDS)
def test_cg_stopping_rules(dims):
    s = po.sphere_solution(dims=dims)
    rhs = _dev(s["rhs"])
    # tol = 1e-9: ends at max_iter, unconverged, finite (po.STALL_ITERATIONS: why this max_iter)
    x, info = ps.solve(rhs, 1.0, tol=1e-9, max_iter=po.STALL_ITERATIONS, check_every=1)
    assert info["iterations"] == po.STALL_ITERATIONS and not info["converged"] and torch.isfinite(x).all()
    assert 0 < info["residual"] < 1e-2
    x, info = ps.solve(rhs, 1.0, tol=1e-4, check_every=32)
    max_iter = 4 * max(dims)
    assert info["converged"] and (info["iterations"] % 32 == 0 or info["iterations"] == max_iter)
    assert info["iterations"] == (56 if dims == (12, 13, 14) else 64)           # 33 and 51 are needed (test_poisson_cpu.py)
    assert po.true_residual(x.cpu().numpy(), s["rhs"], 1.0) <= 1.1e-4
    x, info = ps.solve(rhs, 1.0, tol=1e-4, max_iter=7, check_every=32)
    assert info["iterations"] == 7 and not info["converged"] and torch.isfinite(x).all()


def test_cg_default_max_iter_ends_a_tolerance_out_of_reach():
    s = po.sphere_solution(dims=(12, 13, 14))
    x, info = ps.solve(_dev(s["rhs"]), 1.0, tol=1e-9)
    assert info["iterations"] == 56 and not info["converged"] and torch.isfinite(x).all()
    true = po.true_residual(x.cpu().numpy(), s["rhs"], 1.0)
    print(f"cg (12, 13, 14) at tol 1e-9: recursive residual {info['residual']:.3e}, true {true:.3e} after {info['iterations']} iterations")
    assert true < 1e-5


def test_cg_refuses_a_zero_right_hand_side():
    with pytest.raises(ValueError, match="no normal field"):
        ps.solve(torch.zeros((4, 5, 6), device="cuda"), 1.0)
    with pytest.raises(ValueError, match="tol"):
        ps.solve(torch.ones((4, 5, 6), device="cuda"), 1.0, tol=2.0)


# ---- 4: sample, level, trim ---------------------------------------------------------------------------------------------------------
def test_sample_and_level():
    pts, nrm, dims, origin, h = po.splat_case("9x10x11")
    x = po.random_volume(dims, 3)
    want, level, counted = po.sample(x, pts, dims, origin, h)
    vals, got_level, got_counted = ps.sample(_dev(x), pts, origin, h)
    got = vals.cpu().numpy()
    assert got_counted == counted and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isnan(want), ~po.locate(pts, dims, origin, h)[0])
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok])).all()
    assert abs(got_level - level) <= 1e-12 * abs(level)
    print(f"sample: {counted} of {len(pts)} counted, equal bytes {np.array_equal(got[ok], want[ok])}, level {got_level!r} / {level!r}")
    s = po.sphere_solution()
    _, lvl, cnt = ps.sample(_dev(s["x"]), s["pts"], np.zeros(3), 1.0)
    assert cnt == 3000 and abs(lvl - s["level"]) <= 1e-12 * abs(s["level"])


def test_face_keep_is_the_oracles_mask():
    W, cells, dens = po.dyadic_keep_case()
    assert ps.face_keep(_dev(W), _dev(cells, torch.int32), dens).cpu().numpy().tolist() == po.face_keep(W, cells, dens).tolist() \
        == [1, 0, 1, 0, 0, 0, 0, 1]                                             # cell (1,1,1) sums to exactly 2.0: >=, not >
    s = po.sphere_solution(upper=True)
    W = s["field"][3]
    rng = np.random.default_rng(5)
    cells = rng.integers(-3, W.size + 3, 5000).astype(np.int32)
    for dens in (0.5, 2.0, 3.75):
        want = po.face_keep(W, cells, dens)
        assert 0 < want.sum() < len(want)
        assert np.array_equal(ps.face_keep(_dev(W), _dev(cells, torch.int32), dens).cpu().numpy(), want)
    assert ps.face_keep(_dev(W), torch.zeros(0, dtype=torch.int32, device="cuda"), 2.0).numel() == 0


# ---- 5, 6: end to end -----------------------------------------------------------------------------------------------------------------
def _stages(pts, nrm, dims=po.DIMS):
    field, counted, skipped = ps.splat(pts, nrm, dims, np.zeros(3), 1.0)
    rhs = ps.divergence(field, 1.0)
    x, info = ps.solve(rhs, 1.0, tol=1e-4)
    level = ps.sample(x, pts, np.zeros(3), 1.0)[1]
    return field, x, level, info


BOUNDS = (0, 0, 0, 23, 23, 23)                                                  # `tsdf.bounds_from_points`: the 24^3 grid at the origin


def test_closed_surface_end_to_end():
    pts, nrm = po.sphere_cloud()
    field, x, level, info = _stages(pts, nrm)
    out = ps.reconstruct(pts, nrm, voxel=1.0, bounds=BOUNDS, min_density=None)          # --raw
    st = out["stats"]
    assert st["grid"] == po.DIMS and (st["counted"], st["skipped"]) == (3000, 0) and st["converged"] and st["level"] == level
    assert st["faces_before"] == st["faces_after"] == len(out["faces"]) and out["rgb"] is None
    fig = po.check_closed_surface(x.cpu().numpy(), level, out["verts"], out["faces"])
    assert mo.is_closed_oriented_manifold(out["faces"])
    oracle = po.sphere_solution()
    print(f"sphere: {st['iterations']} iterations (oracle {oracle['info']['iterations']}), level {level:.9f} (oracle {oracle['level']:.9f}), {fig}")
    assert abs(level - oracle["level"]) <= 1e-3 * abs(oracle["level"])
    assert np.abs(x.cpu().numpy() - oracle["x"]).max() <= 1e-3 * np.abs(oracle["x"]).max()


def test_open_surface_end_to_end():
    from svs_hip import mesh
    pts, nrm = po.sphere_cloud(upper=True)
    field, x, level, info = _stages(pts, nrm)
    verts, faces, cells = mesh.marching_cubes(x, level, (1.0, 1.0, 1.0), return_cells=True)
    keep = ps.face_keep(field[3], cells, 2.0)
    assert np.array_equal(keep.cpu().numpy(), po.face_keep(field[3].cpu().numpy(), cells.cpu().numpy(), 2.0))
    kept = cells[keep.bool()].cpu().numpy()
    fig = po.check_open_surface(x.cpu().numpy(), level, field[3].cpu().numpy(), kept)
    print(f"hemisphere: {len(pts)} points, {info['iterations']} iterations, faces {len(faces)} -> {int(keep.sum())}, {fig}")
    rgb = np.random.default_rng(1).integers(0, 256, (len(pts), 3)).astype(np.uint8)
    out = ps.reconstruct(pts, nrm, rgb, voxel=1.0, bounds=BOUNDS, min_density=2.0)
    st = out["stats"]
    assert (st["faces_before"], st["faces_after"]) == (len(faces), int(keep.sum())) and len(out["faces"]) == st["faces_after"]
    assert out["faces"].max() == len(out["verts"]) - 1 and out["rgb"].shape == out["verts"].shape and out["rgb"].dtype == np.uint8
    # a vertex has the colour of the cloud point nearest to it
    d = np.linalg.norm(out["verts"][:50, None].astype(np.float64) - pts[None], axis=2)
    near = d.argmin(1)
    unique = np.sort(d, 1)[:, 1] - np.sort(d, 1)[:, 0] > 1e-6
    assert unique.sum() > 40 and np.array_equal(out["rgb"][:50][unique], rgb[near][unique])
    big = ps.reconstruct(pts, nrm, voxel=1.0, bounds=BOUNDS, min_density=2.0, largest=True)
    assert 0.9 * len(out["faces"]) <= len(big["faces"]) <= len(out["faces"])
    assert len(np.unique(mo.vertex_labels(len(big["verts"]), big["faces"]))) == 1


# ---- 7: files and the runner --------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path):
    from svs_hip import ply
    pts, nrm = po.sphere_cloud(upper=True)
    rgb = np.random.default_rng(2).integers(0, 256, (len(pts), 3)).astype(np.uint8)
    src, dst = str(tmp_path / "cloud.ply"), str(tmp_path / "out" / "mesh.ply")
    ply.write(src, pts, rgb, coords="double", normals=nrm)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        out = ps.main(["--ply", src, "--ply-out", dst, "--voxel", "1.0", "--bounds"] + [str(b) for b in BOUNDS])
    verts, faces = ply.read_mesh(dst)
    colors = ply.read_points(dst)[1]
    assert np.array_equal(verts, out["verts"].astype(np.float64)) and np.array_equal(faces, out["faces"])
    assert colors is not None and np.array_equal(colors, out["rgb"]) and len(faces) == out["stats"]["faces_after"] > 500
    said = text.getvalue()
    assert f"{len(pts)} points counted, 0 skipped, grid 24 x 24 x 24" in said and "seconds: read" in said and "solve" in said
    assert out["stats"]["launches"] == dict(splat=1, divergence=1, apply=0, cg=1, sample=1, keep=1)
    with contextlib.redirect_stdout(io.StringIO()):
        raw = ps.main(["--ply", src, "--ply-out", dst, "--voxel", "1.0", "--raw", "--bounds"] + [str(b) for b in BOUNDS])
    assert raw["stats"]["faces_after"] == raw["stats"]["faces_before"] == out["stats"]["faces_before"] > len(faces)
    bare = str(tmp_path / "bare.ply")
    ply.write(bare, pts, rgb)
    with pytest.raises(ValueError, match="nx ny nz"):
        ps.main(["--ply", bare, "--ply-out", dst, "--voxel", "1.0"])


VIEW_IDS = (25, 22, 28)
NEAR_EYES = ((2.03, 0.31, 0.42), (1.9, 0.62, 0.5), (1.95, 0.0, 0.28))


def test_runner_switch(tmp_path):
    from datasets.data_io import save_pfm
    from helpers.utils import write_cam
    from PIL import Image
    from svs_hip import ply, run
    folder = tmp_path / "scan106"
    for sub in ("cams", "images", "depth_est", "confidence"):
        os.makedirs(folder / sub)
    sc = to.sphere_scene(eyes=NEAR_EYES)
    for vid, view in zip(VIEW_IDS, sc["views"]):
        cam = np.zeros((2, 4, 4))
        cam[0] = view["E"]
        cam[1, :3, :3] = view["K"]
        write_cam(str(folder / "cams" / f"{vid:08}_cam.txt"), cam, (1.0, 0.01, 192, 3.0))
        save_pfm(str(folder / "depth_est" / f"{vid:08}.pfm"), view["depth"])
        save_pfm(str(folder / "confidence" / f"{vid:08}.pfm"), (view["depth"] > 0).astype(np.float32))
        Image.fromarray(np.clip(view["img"] * 255, 0, 255).astype(np.uint8)).save(folder / "images" / f"{vid:08}.jpg", quality=95)
    base = [f"outdir={tmp_path}", "filter_only=true", "eval_mask=false", "testlist=scan106"]
    with pytest.raises(ValueError, match="cloud_poisson"):
        run.main(base + ["+cloud_poisson=0.05"])
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base + ["+cloud_clean=true"])
    assert "poisson" not in res and not os.path.exists(tmp_path / "poisson") and "cloud poisson" not in text.getvalue()
    clean = open(tmp_path / "clean" / "mvsnet106_l3.ply", "rb").read()
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base + ["+cloud_clean=true", "+cloud_poisson=0.05"])
    assert os.listdir(tmp_path / "poisson") == ["mvsnet106_l3.ply"] and open(tmp_path / "clean" / "mvsnet106_l3.ply", "rb").read() == clean
    assert text.getvalue().count("scan106 cloud poisson seconds: read ") == 1
    stats = res["poisson"]["scan106"]
    verts, faces = ply.read_mesh(str(tmp_path / "poisson" / "mvsnet106_l3.ply"))
    assert stats["counted"] == res["clean"]["scan106"]["points_kept"] and stats["skipped"] == 0 and stats["converged"]
    assert len(faces) == stats["faces_after"] > 100 and faces.min() == 0 and faces.max() == len(verts) - 1
    assert ply.read_points(str(tmp_path / "poisson" / "mvsnet106_l3.ply"))[1] is not None
    # the mesh lies on the scene's sphere: every vertex within two voxels of it
    off = np.abs(np.linalg.norm(verts - np.asarray(sc["centre"], np.float64), axis=1) - float(sc["radius"]))
    assert off.max() <= 2 * 0.05
