"""svs_hip.meshsimplify on the GPU against the float64 oracle (tests/meshsimplify_oracle.py): integers element for element,
coordinates to one float32 step in the cells where the two eigen solvers cannot disagree, the derived closeness bound,
topology, duplicates, colours, bad input, determinism, the search, the command line and the runner."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import meshsimplify_oracle as so
import tsdf_oracle as to
from svs_hip import meshsimplify as ms

pytestmark = pytest.mark.gpu
WORST = dict(coord=0.0, err=0.0)


def _gpu(v, f, h, origin, colors=None, tol=1e-3):
    out = ms.cluster(v, f, h, origin=origin, colors=colors, tol=tol, return_info=True)
    info = out[-1]
    return dict(verts=out[0].cpu().numpy(), faces=out[1].cpu().numpy(), colors=out[2].cpu().numpy() if colors is not None else None,
                vert_cell=info["vert_cell"].cpu().numpy(), info=info["info"].cpu().numpy(), err=info["err"].cpu().numpy())


def _integers(got, want):
    assert np.array_equal(got["vert_cell"], want["vert_cell"]) and len(got["verts"]) == want["n_cells"]
    assert got["faces"].shape == want["faces"].shape and np.array_equal(got["faces"], want["faces"])


def _parity(v, f, h, origin, what, colors=None):
    """the whole comparison of the issue's check 1 -> the GPU's result"""
    want = so.cluster(v, f, h, origin, colors)
    got = _gpu(v, f, h, origin, colors)
    _integers(got, want)
    assert np.array_equal(got["info"], want["info"])
    clear = want["clear"]
    assert clear.mean() >= 0.95 if len(clear) else True
    wv = want["verts"].astype(np.float64)
    step = 2.0 ** -23 * np.maximum(np.abs(wv), h)
    dev = np.abs(got["verts"].astype(np.float64) - wv) / step
    off = np.abs(got["verts"].astype(np.float64) - want["centre"]).max(1) if len(clear) else np.zeros(0)
    err_dev = np.abs(got["err"] - want["err"]) / (1e-9 * h * h * want["trace"]) if len(clear) else np.zeros(0)
    worst = (float(dev[clear].max()) if clear.any() else 0.0, float(err_dev.max()) if len(clear) else 0.0)
    WORST["coord"], WORST["err"] = max(WORST["coord"], worst[0]), max(WORST["err"], worst[1])
    print(f"{what}: {len(clear)} cells, {int(clear.sum())} clear, {len(got['faces'])} faces; worst coordinate deviation {worst[0]:.3f} float32 "
          f"steps, worst err deviation {worst[1]:.3e} of its bound (so far {WORST['coord']:.3f} and {WORST['err']:.3e})")
    assert (dev[clear] <= 1.0).all()
    assert (off <= h * (1 + 1e-6)).all()
    assert (err_dev <= 1.0).all()
    if colors is not None:
        assert np.array_equal(got["colors"], want["colors"])
    return got


# ---- 1, 2: parity and run lengths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere_0.5", "sphere_0.3", "cube_0.5", "plane_0.45", "wedge_2.5", "wedge_1.0"])
def test_parity(name):
    v, f, h, o = so.case(name)
    got = _parity(v, f, h, o, name)
    if name == "wedge_2.5":
        assert got["info"].tolist() == [6] and len(got["faces"]) == 0
    if name == "cube_0.5":
        assert set((got["info"] & 3).tolist()) == {1, 2, 3}


@pytest.mark.parametrize("n", [63, 64, 65, 4097])
def test_run_lengths_fan(n):
    v, f, h, o = so.case(f"fan_{n}")
    got = _parity(v, f, h, o, f"fan_{n}")
    hub = got["vert_cell"][0]
    assert (got["vert_cell"] == hub).sum() == 1                 # the hub alone in its cell: a run of n pairs


def test_run_lengths_whole_sphere_in_one_cell():
    v, f, h, o = so.case("sphere_one_cell")
    assert 3 * len(f) == 6624
    got = _parity(v, f, h, o, "sphere_one_cell")
    assert len(got["verts"]) == 1 and got["faces"].shape == (0, 3)


def test_threshold_is_strict():
    """an eigenvalue that equals tol * the largest exactly (a diagonal quadric of dyadic numbers) is not kept"""
    v, f, h, o, tol = so.threshold_case()
    got, want = _gpu(v, f, h, o, tol=tol), so.cluster(v, f, h, o, tol=tol)
    assert got["info"].tolist() == want["info"].tolist() and (got["info"][0] & 3) == 1
    assert (_gpu(v, f, h, o, tol=0.2499)["info"][0] & 3) == 2
    assert np.array_equal(got["verts"], want["verts"]) and got["err"][0] == want["err"][0]


# ---- 3: closeness, derived ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere_0.3", "torus_0.4", "cube_0.5", "wedge_2.5"])
def test_closeness(name):
    """a used vertex is within half a cell of its cell's centre and the output within one cell of it (the clamp), per axis"""
    v, f, h, o = so.case(name)
    got = _gpu(v, f, h, o)
    used = got["vert_cell"] >= 0
    assert used.any()
    d = np.abs(got["verts"][got["vert_cell"][used]].astype(np.float64) - v[used].astype(np.float64)).max()
    print(f"{name}: farthest output vertex {d / h:.3f} cells from an input vertex of its cell")
    assert d <= 1.5 * h * (1 + 1e-6)


# ---- 4: topology ---------------------------------------------------------------------------------------------------------------
def test_topology_and_order():
    for name, chi in (("sphere_0.5", 2), ("sphere_0.3", 2), ("torus_0.4", 0)):
        v, f, h, o = so.case(name)
        want = so.cluster(v, f, h, o)
        got = _gpu(v, f, h, o)
        _integers(got, want)
        assert so.closed_oriented_manifold(got["faces"]) and so.euler(len(got["verts"]), got["faces"]) == chi
        # input order and corner order: face m is the remapped input face source[m]
        src = want["source"]
        assert (np.diff(src) > 0).all() and np.array_equal(got["faces"], got["vert_cell"][f[src]])


# ---- 5: duplicates -------------------------------------------------------------------------------------------------------------
def test_duplicates():
    (v, f), n1 = so.slab(0.5)
    o = np.zeros(3)
    got = _gpu(v, f, 0.5, o)
    first = _gpu(v[:len(v) // 2], f[:n1], 0.5, o)
    _integers(got, so.cluster(v, f, 0.5, o))
    assert len(got["faces"]) > 0 and np.array_equal(got["faces"], first["faces"])
    v, f, h, o = so.case("sphere_0.3")
    single = _gpu(v, f, h, o)
    twice = _gpu(v, np.concatenate([f, f[:, ::-1]]), h, o)
    assert np.array_equal(twice["faces"], single["faces"]) and np.array_equal(twice["vert_cell"], single["vert_cell"])
    rev_first = _gpu(v, np.concatenate([f[:, ::-1], f]), h, o)
    assert np.array_equal(rev_first["faces"], single["faces"][:, ::-1])           # the first listing wins, whatever its orientation


# ---- 6: colours ----------------------------------------------------------------------------------------------------------------
def test_colours():
    v, f, h, o = so.case("cube_0.5")
    col = np.random.default_rng(5).integers(0, 256, (len(v), 3)).astype(np.uint8)
    got = _parity(v, f, h, o, "cube_0.5 with colours", colors=col)
    assert got["colors"].dtype == np.uint8 and got["colors"].shape == (len(got["verts"]), 3)
    edge = np.concatenate([np.zeros((len(v) // 2, 3)), np.full((len(v) - len(v) // 2, 3), 255)]).astype(np.uint8)
    _parity(v, f, h, o, "cube_0.5 with codes 0 and 255", colors=edge)


# ---- 7: bad input ----------------------------------------------------------------------------------------------------------------
def test_bad_input():
    v, f, h, o = so.case("sphere_0.5")
    n = len(v)
    bad_v = np.concatenate([v, [[np.nan, 0, 0], [np.inf, 0, 0], [0.5, 0.5, 0.5], [0, -np.inf, np.nan]]]).astype(np.float32)
    bad_f = np.concatenate([[[0, 1, n]], f[:100], [[0, n + 1, 2], [0, 1, n + 4], [-1, 0, 1], [5, 5, 9], [0, 0, 0], [2 ** 31 - 1, 0, 1],
                                                   [-2 ** 31, 0, 1], [n + 3, 1, 2]], f[100:], [[3, 4, n + 9]]]).astype(np.int32)
    got = _parity(bad_v, bad_f, h, o, "sphere_0.5 with bad faces")
    clean = _gpu(v, f, h, o)
    assert np.array_equal(got["faces"], clean["faces"]) and np.array_equal(got["verts"], clean["verts"])
    assert np.array_equal(got["err"], clean["err"]) and (got["vert_cell"][n:] == -1).all()
    # the default origin ignores the vertices that are not finite
    auto = ms.cluster(bad_v, bad_f, h, return_info=True)
    assert np.array_equal(auto[-1]["origin"], so.default_origin(v)) and len(auto[1]) > 0
    for ev, ef in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), (v, np.zeros((0, 3), np.int32)),
                   (v, np.array([[0, 0, 1], [0, 1, n], [2, 2, 2]], np.int32)), (np.zeros((0, 3), np.float32), np.array([[0, 1, 2]], np.int32))):
        out = ms.cluster(ev, ef, h, colors=np.zeros((len(ev), 3), np.uint8), return_info=True)
        assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[2].shape == (0, 3)
        assert out[3]["vert_cell"].shape == (len(ev),) and bool((out[3]["vert_cell"] == -1).all()) and out[3]["err"].shape == (0,)
    with pytest.raises(ValueError, match="cell"):
        ms.cluster(v, f, 0.0)
    with pytest.raises(ValueError, match="tol"):
        ms.cluster(v, f, h, tol=1.0)
    with pytest.raises(ValueError, match="2\\^21"):
        ms.cluster(v, f, 1e-7)
    with pytest.raises(ValueError, match="2\\^21"):
        ms.cluster(v, f, h, origin=(-2.0 ** 21 * h, 0, 0))


# ---- 8: the same bits twice --------------------------------------------------------------------------------------------------
def test_same_bits_twice():
    v, f, h, o = so.case("fan_4097")
    tv, tf = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    col = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (len(v), 3)).astype(np.uint8)).cuda()
    a = ms.cluster(tv, tf, h, origin=o, colors=col, return_info=True)
    b = ms.cluster(tv, tf, h, origin=o, colors=col, return_info=True)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert all(torch.equal(a[3][k], b[3][k]) for k in ("vert_cell", "info", "err"))


# ---- 9: the search -----------------------------------------------------------------------------------------------------------
def test_simplify_target_and_ratio():
    v, f = so.torus()
    target = 300
    out = ms.simplify(v, f, target_faces=target, return_info=True)
    info = out[-1]
    assert 0 < out[1].shape[0] <= target and len(info["tried"]) == 16
    lo, hi = info["bracket"]
    tri = v.astype(np.float64)[f]
    edge = np.mean([np.linalg.norm(tri[:, a] - tri[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))])
    assert lo == pytest.approx(edge, rel=1e-12) and hi == pytest.approx(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)), rel=1e-12)
    best, tried = so.bisect(lambda h: so.count_faces(v, f, h), lo, hi, target, tries=16)
    assert tried == info["tried"] and best == info["cell"]
    assert np.array_equal(out[1].cpu().numpy(), so.cluster(v, f, best)["faces"])
    assert info["cell"] == min(h for h, n in tried if n <= target)
    by_ratio = ms.simplify(v, f, ratio=target / len(f), return_info=True)
    assert int(target / len(f) * len(f)) == target and by_ratio[-1]["cell"] == info["cell"] and torch.equal(by_ratio[1], out[1])
    fixed = ms.simplify(v, f, cell=info["cell"])
    assert torch.equal(fixed[0], out[0]) and torch.equal(fixed[1], out[1])
    # a target the tries do not reach: the box diagonal itself is the last resort (a mesh inside one cell has no faces left)
    none = ms.simplify(*so.uv_sphere(), target_faces=0, tries=2, return_info=True)
    assert none[1].shape == (0, 3) and len(none[-1]["tried"]) == 3 and none[-1]["cell"] == none[-1]["bracket"][1]
    with pytest.raises(ValueError, match="target_faces"):
        ms.simplify(v, f, target_faces=-1)


# ---- 10: end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coloured", [False, True])
def test_command_line(tmp_path, coloured):
    from svs_hip import ply
    v, f, h, _ = so.case("sphere_0.3")
    col = np.random.default_rng(2).integers(0, 256, (len(v), 3)).astype(np.uint8) if coloured else None
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    ply.write(src, v, col, f)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        rv, rf, rc, stats = ms.main(["--ply", src, "--ply-out", dst, "--cell", str(h), "--report"])
    want = ms.cluster(v, f, h, colors=col)
    fv, ff = ply.read_mesh(dst)
    assert np.array_equal(fv, want[0].cpu().numpy().astype(np.float64)) and np.array_equal(ff, want[1].cpu().numpy())
    file_col = ply.read_points(dst)[1]
    assert (file_col is None and rc is None) if not coloured else np.array_equal(file_col, want[2].cpu().numpy())
    said = text.getvalue()
    assert f"faces {len(f)} -> {len(ff)}" in said and "cells by rank" in said and "seconds: read" in said and "distance in -> out mean" in said
    assert stats["faces_out"] == len(ff) and sum(stats["ranks"]) == len(fv) and stats["fallbacks"] == 0 and stats["launches"]["solve"] == 1
    # the simplified sphere stays within the derived 1.5 cells (plus the sampling step) of the input surface
    assert 0 < stats["distance"]["max"] <= 1.5 * h * 3 ** 0.5 + 0.5 * h
    with contextlib.redirect_stdout(io.StringIO()):
        stats = ms.main(["--ply", src, "--ply-out", dst, "--ratio", "0.1"])[3]
    assert 0 < stats["faces_out"] <= 0.1 * len(f) and len(stats["tried"]) == 16 and stats["distance"] is None


VIEW_IDS = (25, 22, 28)
NEAR_EYES = ((2.03, 0.31, 0.42), (1.9, 0.62, 0.5), (1.95, 0.0, 0.28))


def test_runner_switch(tmp_path):
    from datasets.data_io import save_pfm
    from evals import eval_dtu
    from helpers.utils import write_cam
    from PIL import Image
    from svs_hip import run
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
    base = [f"outdir={tmp_path}", "filter_only=true", "eval_mask=false", "testlist=scan106", "+tsdf_voxel=0.05", "+tsdf_trunc=0.12"]
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base)
    assert "simple_meshes" not in res and not os.path.exists(tmp_path / "tsdf_simple") and "tsdf simplify" not in text.getvalue()
    full = open(tmp_path / "tsdf" / "mvsnet106_l3.ply", "rb").read()
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base + ["+tsdf_simplify=0.25"])
    small = tmp_path / "tsdf_simple" / "mvsnet106_l3.ply"
    assert os.path.exists(small) and open(tmp_path / "tsdf" / "mvsnet106_l3.ply", "rb").read() == full
    assert text.getvalue().count("scan106 tsdf simplify seconds: read ") == 1
    stats = res["simple_meshes"]["scan106"]
    fv, ff = eval_dtu.ply.read_mesh(str(tmp_path / "tsdf" / "mvsnet106_l3.ply"))
    sv, sf = eval_dtu.ply.read_mesh(str(small))
    assert stats["faces_in"] == len(ff) and stats["faces_out"] == len(sf) and 0 < len(sf) <= 0.25 * len(ff) and len(sv) < len(fv)
    assert sf.min() >= 0 and sf.max() < len(sv) and eval_dtu.ply.read_points(str(small))[1] is not None    # the TSDF mesh's colours are kept
    with pytest.raises(ValueError, match="tsdf_simplify"):
        run.main([f"outdir={tmp_path}", "filter_only=true", "testlist=scan106", "+tsdf_simplify=0.25"])
