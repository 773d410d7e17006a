"""Screened svs_hip.poisson on the GPU against the float64 oracle (tests/poisson_screen_oracle.py): the screened operator at
the stencil's dispatch edges with x, W and out aligned and not, the preconditioned solve against the oracle's recurrence and
a direct solve of the screened system, its stopping rules, what screening buys on a cloud of uneven density, and the
`screen` switch of reconstruct, the command line and the runner."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import poisson_oracle as po
import poisson_screen_oracle as so
import tsdf_oracle as to
from svs_hip import poisson as ps

pytestmark = pytest.mark.gpu
TOL = 1e-4
WEIGHTS = (0.0, 0.37, 50.0)
BOUNDS = (0, 0, 0, 23, 23, 23)                                                  # `tsdf.bounds_from_points`: the 24^3 grid at the origin


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


def _weights_plane(shape, seed):
    """random, not negative: half the nodes exactly 0, the others log-uniform in [1e-3, 1e3]"""
    rng = np.random.default_rng(seed)
    W = (10.0 ** rng.uniform(-3, 3, shape)) * (rng.random(shape) < 0.5)
    W.reshape(-1)[:2] = (0.0, 1e3)                                              # both ends whatever the draw
    return W.astype(np.float32)


# ---- the operator ----------------------------------------------------------------------------------------------------------------
# which of x, W, out sit one element off a 16-byte boundary: only all three aligned (and n2 % 4 == 0) takes the 16-byte path
ALIGNMENTS = {"aligned": (False, False, False), "all off": (True, True, True), "W off": (False, True, False), "x off": (True, False, False)}


def test_screened_apply_parity():
    shapes = po.VOLUME_SHAPES + po.tile_shapes(ps.stencil_tile())
    worst = 0.0
    for n, shape in enumerate(shapes):
        x, W, h = po.random_volume(shape, 70 + n), _weights_plane(shape, 90 + n), 0.5 + 0.25 * (n % 3)
        assert (W >= 0).all() and W.max() == 1e3 and (W.size <= 8 or 0.3 < (W == 0).mean() < 0.7)
        nan = np.full(shape, np.nan, np.float32)
        for weight in WEIGHTS:
            want = so.apply(x, W, h, weight)
            for how, (x_off, w_off, out_off) in ALIGNMENTS.items():
                src, plane, out = (_misaligned if x_off else _dev)(x), (_misaligned if w_off else _dev)(W), (_misaligned if out_off else _dev)(nan)
                got = ps.apply_screened(src, plane, weight, h, out=out)
                assert got.data_ptr() == out.data_ptr() and plane.data_ptr() % 16 == (4 if w_off else 0)
                dev = _steps(got.cpu().numpy(), want)
                worst = max(worst, float(dev.max()))
                assert (dev <= 1.0).all(), (shape, weight, how, dev.max())
        # weight 0: the bytes of the unscreened entry
        assert torch.equal(ps.apply_screened(_dev(x), _dev(W), 0.0, h).view(torch.int32), ps.apply(_dev(x), h).view(torch.int32))
        # what lies around a misaligned volume is left alone
        buf = torch.full((x.size + 5,), 7.0, dtype=torch.float32, device="cuda")
        ps.apply_screened(_dev(x), _dev(W), 0.37, h, out=buf[1:1 + x.size].view(shape))
        assert buf[0] == 7.0 and (buf[1 + x.size:] == 7.0).all() and torch.isfinite(buf).all()
    print(f"screened apply: {len(shapes)} shapes x {len(WEIGHTS)} weights x {len(ALIGNMENTS)} alignments, worst deviation {worst:.3f} float32 steps")


def test_screened_apply_refuses_bad_arguments():
    x = torch.ones((4, 5, 6), device="cuda")
    for weight in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight"):
            ps.apply_screened(x, x.clone(), weight, 1.0)
    with pytest.raises(ValueError, match="shape"):
        ps.apply_screened(x, torch.ones((4, 5, 7), device="cuda"), 1.0, 1.0)
    with pytest.raises(TypeError):
        ps.apply_screened(x, x.double(), 1.0, 1.0)


# ---- the preconditioned solve ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", po.CG_GRIDS)
def test_pcg_against_the_oracle_and_the_direct_solve(dims):
    s = so.uneven_system(dims)
    weight = so.screen_weight(s["W"], s["counted"], 4.0, 1.0)[0]
    rhs64 = s["rhs"].astype(np.float64)
    field, rhs = _dev(s["field"]), _dev(s["rhs"])
    W = field[3]                                                                # the plane where the splat leaves it: no copy
    assert W.data_ptr() == field.data_ptr() + 3 * 4 * rhs.numel()
    x, info = ps.solve_screened(rhs, W, weight, 1.0, tol=TOL, check_every=1)
    got = x.cpu().numpy().astype(np.float64)
    e32, e64 = so.uneven_solution(dims, 4.0, "float32"), so.uneven_solution(dims, 4.0, "float64")
    direct = so.direct_solve(rhs64, s["W"], 1.0, weight)
    err = lambda v: float(np.linalg.norm(v - direct) / np.linalg.norm(direct))
    true = so.true_residual(got, rhs64, s["W"], 1.0, weight)
    e_gpu, e_emulated = err(got), err(e32["x"])
    print(f"pcg {dims} screen 4 (weight {weight:.4f}): {info['iterations']} iterations (oracle float64 {e64['info']['iterations']}, float32 "
          f"storage {e32['info']['iterations']}), recursive residual {info['residual']:.6e}, true {true:.6e} = {true / TOL:.4f} tol; error "
          f"against the direct solve {e_gpu:.6e}, the oracle's float32-emulated PCG {e_emulated:.6e}")
    assert info["converged"] and abs(info["iterations"] - e64["info"]["iterations"]) <= 2
    assert true <= 1.1 * TOL
    assert e_gpu <= 2.0 * e_emulated
    again = ps.solve_screened(rhs, W, weight, 1.0, tol=TOL, check_every=1)[0]
    assert torch.equal(x, again)                                                # the same bytes every run
    # a right-hand side and a solution at an odd offset, then W as well: the scalar paths, the same values
    odd = ps.solve_screened(_misaligned(s["rhs"]), W, weight, 1.0, tol=TOL, check_every=1, out=_misaligned(np.zeros(dims, np.float32)))[0]
    assert torch.equal(odd, x)
    odd = ps.solve_screened(_misaligned(s["rhs"]), _misaligned(s["W"]), weight, 1.0, tol=TOL, check_every=1,
                            out=_misaligned(np.zeros(dims, np.float32)))[0]
    assert torch.equal(odd, x)


@pytest.mark.parametrize("dims", po.CG_GRIDS)
def test_pcg_stopping_rules(dims):
    s = so.uneven_system(dims)
    weight = so.screen_weight(s["W"], s["counted"], 4.0, 1.0)[0]
    rhs, W = _dev(s["rhs"]), _dev(s["W"])
    x, info = ps.solve_screened(rhs, W, weight, 1.0, tol=TOL, max_iter=7, check_every=32)
    assert info["iterations"] == 7 and not info["converged"] and torch.isfinite(x).all() and 0 < info["residual"] < 1
    x, info = ps.solve_screened(rhs, W, weight, 1.0, tol=TOL, check_every=32)
    max_iter = 4 * max(dims)
    assert info["converged"] and (info["iterations"] % 32 == 0 or info["iterations"] == max_iter)
    assert info["iterations"] == (32 if dims == (12, 13, 14) else 64)           # 22 and 38 are needed (test_poisson_screen_cpu.py)
    assert so.true_residual(x.cpu().numpy(), s["rhs"], s["W"], 1.0, weight) <= 1.1 * TOL


def test_pcg_refuses_a_zero_right_hand_side_and_a_negative_weight():
    zero, one = torch.zeros((4, 5, 6), device="cuda"), torch.ones((4, 5, 6), device="cuda")
    with pytest.raises(ValueError, match="no normal field"):
        ps.solve_screened(zero, one, 1.0, 1.0)
    with pytest.raises(ValueError, match="weight"):
        ps.solve_screened(one, one, -1.0, 1.0)
    with pytest.raises(ValueError, match="tol"):
        ps.solve_screened(one, one, 1.0, 1.0, tol=2.0)


# ---- what screening buys, on the GPU stages ----------------------------------------------------------------------------------------
def test_screening_keeps_the_level_set_on_an_uneven_cloud():
    pts, nrm = so.uneven_cloud()
    origin = np.zeros(3)
    field, counted, skipped = ps.splat(pts, nrm, po.DIMS, origin, 1.0)
    rhs = ps.divergence(field, 1.0)
    weight, density = ps.screen_weight(field[3], counted, 4.0, 1.0)
    want = so.screen_weight(so.uneven_system()["W"], counted, 4.0, 1.0)
    assert (counted, skipped) == (1699, 0) and (weight, density) == want
    x_off, info_off = ps.solve(rhs, 1.0, tol=TOL)
    x_on, info_on = ps.solve_screened(rhs, field[3], weight, 1.0, tol=TOL)
    fig = {}
    for name, x in (("off", x_off), ("on", x_on)):
        level = ps.sample(x, pts, origin, 1.0)[1]
        host = x.cpu().numpy()
        fig[name] = dict(level=level, worst=po.worst_misclassified(host, level), **so.radial_error(host, level))
    print(f"uneven sphere on the GPU stages: unscreened {info_off['iterations']} iterations {fig['off']}; screen 4 (weight {weight:.4f}) "
          f"{info_on['iterations']} iterations {fig['on']}")
    assert info_off["converged"] and info_on["converged"]
    assert fig["off"]["worst"] > 1.0 and fig["on"]["worst"] < 0.5
    assert fig["on"]["rms"] < 0.5 * fig["off"]["rms"]


# ---- the switch: reconstruct, the command line, the runner -------------------------------------------------------------------------
def test_reconstruct_with_and_without_screen():
    pts, nrm = so.uneven_cloud()
    calls, screened = dict(ps.ENTRY_CALLS), dict(ps.SCREENED_CALLS)
    out = ps.reconstruct(pts, nrm, voxel=1.0, bounds=BOUNDS, min_density=None, screen=4.0)
    st = out["stats"]
    assert st["screen"] == 4.0 and (st["screen_weight"], st["density"]) == so.screen_weight(so.uneven_system()["W"], 1699, 4.0, 1.0)
    assert st["converged"] and len(out["faces"]) == st["faces_after"] > 500 and out["faces"].max() == len(out["verts"]) - 1
    assert ps.SCREENED_CALLS["pcg"] == screened["pcg"] + 1 and ps.ENTRY_CALLS["cg"] == calls["cg"]
    off = np.abs(np.linalg.norm(out["verts"].astype(np.float64) - po.CENTRE, axis=1) - po.RADIUS)
    calls, screened = dict(ps.ENTRY_CALLS), dict(ps.SCREENED_CALLS)
    plain = ps.reconstruct(pts, nrm, voxel=1.0, bounds=BOUNDS, min_density=None)
    assert plain["stats"]["screen"] is None and ps.ENTRY_CALLS["cg"] == calls["cg"] + 1 and ps.SCREENED_CALLS == screened
    zero = ps.reconstruct(pts, nrm, voxel=1.0, bounds=BOUNDS, min_density=None, screen=0)
    assert ps.SCREENED_CALLS == screened and np.array_equal(zero["verts"], plain["verts"]) and np.array_equal(zero["faces"], plain["faces"])
    off_plain = np.abs(np.linalg.norm(plain["verts"].astype(np.float64) - po.CENTRE, axis=1) - po.RADIUS)
    print(f"uneven sphere meshed: farthest vertex {off.max():.3f} voxel from the sphere at screen 4, {off_plain.max():.3f} unscreened")
    # a vertex lies on an edge of length 1 one end of which is a node at most 0.5 voxel on the wrong side (the property above);
    # unscreened the level set itself is more than a voxel off (a node 2.18 voxels inside the sphere is classified outside)
    assert off.max() <= 1.5 and off_plain.max() > 1.0
    with pytest.raises(ValueError, match="screen"):
        ps.reconstruct(pts, nrm, voxel=1.0, bounds=BOUNDS, screen=-1)


def test_command_line(tmp_path):
    from svs_hip import ply
    pts, nrm = so.uneven_cloud()
    src, dst = str(tmp_path / "cloud.ply"), str(tmp_path / "out" / "mesh.ply")
    ply.write(src, pts, None, coords="double", normals=nrm)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        out = ps.main(["--ply", src, "--ply-out", dst, "--voxel", "1.0", "--screen", "4", "--bounds"] + [str(b) for b in BOUNDS])
    verts, faces = ply.read_mesh(dst)
    assert np.array_equal(verts, out["verts"].astype(np.float64)) and np.array_equal(faces, out["faces"]) and len(faces) > 500
    st = out["stats"]
    assert st["screen"] == 4.0 and st["launches"] == dict(splat=1, divergence=1, apply=0, cg=0, sample=1, keep=1)
    assert st["screened_launches"] == dict(apply=0, pcg=1)
    assert "screen 4 (weight " in text.getvalue() and "1699 points counted" in text.getvalue()
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        plain = ps.main(["--ply", src, "--ply-out", dst, "--voxel", "1.0", "--bounds"] + [str(b) for b in BOUNDS])
    assert "screened_launches" not in plain["stats"] and plain["stats"]["launches"]["cg"] == 1 and "screen" not in text.getvalue()


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
    base = [f"outdir={tmp_path}", "filter_only=true", "eval_mask=false", "testlist=scan106", "+cloud_clean=true"]
    with pytest.raises(ValueError, match="cloud_poisson_screen"):
        run.main(base + ["+cloud_poisson_screen=4"])
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base + ["+cloud_poisson=0.05", "+cloud_poisson_screen=4"])
    stats = res["poisson"]["scan106"]
    assert stats["screen"] == 4.0 and stats["screened_launches"] == dict(apply=0, pcg=1) and stats["launches"]["cg"] == 0
    assert stats["converged"] and stats["counted"] == res["clean"]["scan106"]["points_kept"] and ", screen 4)" in text.getvalue()
    verts, faces = ply.read_mesh(str(tmp_path / "poisson" / "mvsnet106_l3.ply"))
    assert len(faces) == stats["faces_after"] > 100 and faces.min() == 0 and faces.max() == len(verts) - 1
    # the mesh lies on the scene's sphere: every vertex within two voxels of it, the bound the unscreened mesh is held to
    off = np.abs(np.linalg.norm(verts - np.asarray(sc["centre"], np.float64), axis=1) - float(sc["radius"]))
    print(f"runner, screen 4: {len(faces)} faces, farthest vertex {off.max() / 0.05:.3f} voxels from the sphere")
    assert off.max() <= 2 * 0.05
