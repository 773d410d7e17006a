"""svs_hip.meshsmooth on the GPU against the float64 oracle (tests/meshsmooth_oracle.py): the connectivity element for element,
the float32 outputs of every pass to at most one float32 step (0 is expected: the worst deviation is printed), both parities
of the buffer swap, the boundary modes, long lists, bad input, determinism, the command line and the runner."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest
import torch

import meshsmooth_oracle as mo
import tsdf_oracle as to
from svs_hip import meshsmooth as sm

pytestmark = pytest.mark.gpu
WORST = dict(steps=0.0)
LAM, MU = 0.5, -0.53


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (verts float32, faces int32, the oracle's adjacency): computed once, shared, never written to"""
    if name == "sphere":
        v, f = mo.icosphere(3)
        v = mo.noisy(v, f, 0.1, seed=1)
    elif name == "sphere_shuffled":
        v, f, _ = case("sphere")
        f = f[np.random.default_rng(7).permutation(len(f))]
    elif name == "cube":
        v, f = mo.cube(8)
        v = mo.noisy(v, f, 0.1 * 0.25 / mo.mean_edge(v, f), seed=2)
    elif name == "patch":
        v, f = mo.patch(8)
        v = mo.noisy(v, f, 0.1, seed=3, axes=(2,))
    elif name.startswith("bipyramid_"):
        v, f = mo.bipyramid(int(name[10:]))
        v = (v + np.random.default_rng(4).normal(0, 1e-4, v.shape)).astype(np.float32)
    elif name == "fin":
        v, f = mo.fin()
    elif name == "bad":
        v, f, _ = mo.bad_input()
        v = v.copy()
        v[:162] = mo.noisy(*mo.icosphere(2), 0.1, seed=5)
    elif name == "empty":
        v, f = mo.EMPTY
    else:
        v, f = mo.small(name)
    for a in (v, f):
        a.setflags(write=False)
    return v, f, mo.adjacency(v, f)


def _steps(got, want, what):
    """the worst deviation of two float32 arrays in float32 steps of the wanted value (equal bits, NaN included: 0)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    same = got.view(np.uint32) == want.view(np.uint32)
    with np.errstate(all="ignore"):
        dev = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    dev = np.where(same, 0.0, np.where(np.isfinite(dev), dev, np.inf))
    worst = float(dev.max()) if dev.size else 0.0
    WORST["steps"] = max(WORST["steps"], worst)
    print(f"{what}: worst deviation {worst:.3f} float32 steps (so far {WORST['steps']:.3f})")
    return worst


def _adjacency_equal(got, want, what):
    c = got["counts"]
    assert [c["edges"], c["boundary_edges"], c["nonmanifold_edges"], c["valid_faces"]] == want["counts"], what
    for k in ("nbr_start", "nbr", "nbr_boundary", "face_start", "vert_face", "face_valid", "flags"):
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape and np.array_equal(g, want[k]), (what, k)


# ---- adjacency -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["empty", "triangle", "two_triangles", "tetrahedron", "three_on_an_edge", "face_twice", "unused_vertex",
                                  "bad_faces", "no_valid_face", "fin", "cube", "sphere", "patch", "sphere_shuffled", "bad", "bipyramid_63",
                                  "bipyramid_64", "bipyramid_65", "bipyramid_4097"])
def test_adjacency(name):
    v, f, want = case(name)
    got = sm.adjacency(v, f)
    _adjacency_equal(got, want, name)
    if name.startswith("bipyramid_"):
        n = int(name[10:])
        assert want["counts"] == [3 * n, 0, 0, 2 * n] and np.diff(want["nbr_start"])[-2:].tolist() == [n, n]
    if len(f) and want["counts"][3]:
        assert got["mean_edge"] == pytest.approx(mo.mean_edge(v, f), rel=1e-12)
    if name == "sphere_shuffled":
        plain = case("sphere")[2]
        assert all(np.array_equal(want[k], plain[k]) for k in ("nbr_start", "nbr", "nbr_boundary", "flags"))


def test_adjacency_of_a_mesh_without_faces_or_vertices():
    v = case("sphere")[0]
    for ev, ef in ((v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.array([[0, 1, 2]], np.int32))):
        _adjacency_equal(sm.adjacency(ev, ef), mo.adjacency(ev, ef), "no faces or no vertices")
        assert sm.taubin(ev, ef)[0].shape == ev.shape and sm.denoise(ev, ef)[0].shape == ev.shape


# ---- Taubin --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", ["fixed", "curve", "free"])
@pytest.mark.parametrize("name", ["sphere", "patch", "bipyramid_65", "bipyramid_4097", "bad"])
def test_taubin(name, boundary):
    v, f, adj = case(name)
    tv, tf = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    gadj = sm.adjacency(tv, tf)
    used = (adj["flags"] & mo.USED) != 0
    worst = 0.0
    for mu in (0.0, MU):
        x = v.astype(np.float64)
        for iters in range(4):
            if iters:
                x = mo.taubin_pass(x, adj, LAM, mo.MODES[boundary])
                x = mo.taubin_pass(x, adj, mu, mo.MODES[boundary]) if mu != 0 else x
            want = x.astype(np.float32)
            got, faces_out = sm.taubin(tv, tf, iters=iters, lam=LAM, mu=mu, boundary=boundary, adj=gadj)
            assert faces_out.data_ptr() == tf.data_ptr() and got.dtype == torch.float32 and got.data_ptr() != tv.data_ptr()
            got = got.cpu().numpy()
            worst = max(worst, _steps(got, want, f"taubin {name} {boundary} mu {mu} iters {iters}"))
            assert np.array_equal(got[~used].view(np.uint32), v[~used].view(np.uint32))
            if iters == 0:
                assert np.array_equal(got.view(np.uint32), v.view(np.uint32))
            elif boundary == "fixed" and name == "patch":
                edge = (adj["flags"] & mo.BOUNDARY) != 0
                assert np.array_equal(got[edge], v[edge]) and not np.array_equal(got[~edge], v[~edge])
    assert worst <= 1.0
    assert np.array_equal(tv.cpu().numpy().view(np.uint32), v.view(np.uint32))      # the input is not written to


def test_taubin_curve_differs_from_free_and_fixed_on_the_boundary():
    v, f, adj = case("patch")
    edge = (adj["flags"] & mo.BOUNDARY) != 0
    out = {b: sm.taubin(v, f, iters=3, mu=0.0, boundary=b)[0].cpu().numpy() for b in ("fixed", "curve", "free")}
    assert np.array_equal(out["curve"][edge][:, 2] != out["free"][edge][:, 2], np.ones(edge.sum(), bool))
    assert not np.array_equal(out["curve"][edge], out["fixed"][edge])
    for b in out:
        assert _steps(out[b], mo.taubin(v, f, iters=3, mu=0.0, boundary=b), f"patch {b}") <= 1.0


# ---- denoising -----------------------------------------------------------------------------------------------------------------
RS = {"cube": 0.5, "fin": 1.5, "bipyramid_65": 0.3}


@pytest.mark.parametrize("boundary", ["fixed", "free"])
@pytest.mark.parametrize("name", ["cube", "fin", "bipyramid_65"])
def test_denoise_passes(name, boundary):
    v, f, adj = case(name)
    tv, tf = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    gadj = sm.adjacency(tv, tf)
    x64 = v.astype(np.float64)
    want = mo.face_frames(x64, f, adj)
    x, tmp = sm._working(tv)
    frames = sm.face_frames_raw(x, tf, gadj)
    worst = max(_steps(g.cpu().numpy(), w, f"face_frames {name} {what}") for g, w, what in zip(frames, want, ("normals", "areas", "centroids")))
    exact = all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(frames, want))
    print(f"face_frames {name}: float64 outputs equal to the bit: {exact}")
    rs, rn = RS[name], 0.6
    filtered = {}
    for passes in (1, 3):
        n = sm.normal_filter_raw(frames[0].clone(), frames[1], frames[2], tf, len(v), gadj, passes, rs, rn)
        filtered[passes] = n
        wn = mo.normal_filter(want[0], want[1], want[2], f, adj, passes, rs, rn)
        worst = max(worst, _steps(n.cpu().numpy(), wn, f"normal_filter {name} passes {passes}"))
        assert not np.array_equal(wn, want[0])                      # the filter did something
    wn = mo.normal_filter(want[0], want[1], want[2], f, adj, 3, rs, rn)
    movable = ((adj["flags"] & mo.USED) != 0) & ~(((adj["flags"] & mo.BOUNDARY) != 0) & (boundary == "fixed"))
    for passes in (1, 2, 3):
        x, tmp = sm._working(tv)
        sm.vertex_update_raw(x, tmp, filtered[3], tf, gadj, passes, mo.MODES[boundary])
        wx = mo.vertex_update(x64, wn, f, adj, passes, mo.MODES[boundary])
        worst = max(worst, _steps(x.cpu().numpy(), wx, f"vertex_update {name} {boundary} passes {passes}"))
        assert np.array_equal(wx, x64) != bool(movable.any())
    assert worst <= 1.0
    # the whole of it through the public function
    got = sm.denoise(tv, tf, 3, 3, rn=rn, rs=rs, boundary=boundary, adj=gadj)[0].cpu().numpy()
    assert _steps(got, mo.denoise(v, f, 3, 3, rn=rn, rs=rs, boundary=boundary), f"denoise {name} {boundary}") <= 1.0


def test_denoise_with_a_support_that_sees_no_neighbour():
    """every neighbour skipped: the normals are renormalised own normals, and a vertex lies in the planes of its own faces"""
    v, f, adj = case("cube")
    tv, tf = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    out, _, info = sm.denoise(tv, tf, 3, 3, rs=1e-6, boundary="free", return_info=True)
    x, _ = sm._working(tv)
    own = sm.face_frames_raw(x, tf, info["adj"])[0]
    assert _steps(info["normals"].cpu().numpy(), own.cpu().numpy(), "normals, no neighbour seen") <= 1.0
    assert _steps(out.cpu().numpy(), v, "positions, no neighbour seen") <= 1.0
    assert _steps(out.cpu().numpy(), mo.denoise(v, f, 3, 3, rs=1e-6, boundary="free"), "against the oracle") <= 1.0


# ---- robustness and plumbing -----------------------------------------------------------------------------------------------------
def test_same_bytes_twice_and_from_an_unaligned_tensor():
    v, f, _ = case("bipyramid_4097")
    tv, tf = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    store = torch.zeros(v.size + 8, dtype=torch.float32, device="cuda")
    assert store.data_ptr() % 16 == 0
    off = store[1:1 + v.size].view(-1, 3)
    off.copy_(tv)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    for fn in (lambda t: sm.taubin(t, tf, iters=3), lambda t: sm.denoise(t, tf, 2, 3, rs=0.3, boundary="free")):
        a, b, c = fn(tv)[0], fn(tv)[0], fn(off)[0]
        assert torch.equal(a, b) and torch.equal(a, c) and not torch.equal(a, tv)
    a, b = sm.adjacency(tv, tf), sm.adjacency(off, tf)
    assert all(torch.equal(a[k], b[k]) for k in ("nbr_start", "nbr", "nbr_boundary", "face_start", "vert_face", "face_valid", "flags"))


def test_bad_input_and_pass_through():
    v, f, adj = case("bad")
    n = 162
    clean_f = mo.icosphere(2)[1]
    tf = torch.from_numpy(f).cuda()
    for fn, ofn in ((lambda vv, ff: sm.taubin(vv, ff, iters=3), lambda vv, ff: mo.taubin(vv, ff, iters=3)),
                    (lambda vv, ff: sm.denoise(vv, ff, 2, 3, rs=0.5), lambda vv, ff: mo.denoise(vv, ff, 2, 3, rs=0.5))):
        got, faces_out = fn(v, tf)
        got = got.cpu().numpy()
        assert faces_out.data_ptr() == tf.data_ptr() and torch.equal(tf.cpu(), torch.from_numpy(f))    # faces pass through, the bad ones too
        assert np.array_equal(got[n:].view(np.uint32), v[n:].view(np.uint32))                 # NaN, inf and unused: their input bits
        assert np.array_equal(got[:n], fn(v[:n], clean_f)[0].cpu().numpy())                   # bad faces contribute nothing
        assert _steps(got, ofn(v, f), "bad input") <= 1.0 and not np.array_equal(got[:n], v[:n])
    assert adj["face_valid"].sum() == 320 and (adj["flags"][n:] == 0).all()
    for bad in (dict(iters=-1), dict(iters=1.5), dict(lam=0.0), dict(lam=1.1), dict(mu=0.1), dict(mu=-2.1), dict(boundary="loose")):
        with pytest.raises(ValueError, match="svs_mesh_taubin"):
            sm.taubin(v, f, **bad)
    for bad, entry in ((dict(normal_iters=-1), "svs_mesh_normal_filter"), (dict(vertex_iters=-1), "svs_mesh_vertex_update"),
                       (dict(rn=0.0), "svs_mesh_normal_filter"), (dict(rn=2.5), "svs_mesh_normal_filter"), (dict(rs=0.0), "svs_mesh_normal_filter"),
                       (dict(boundary="curve"), "svs_mesh_vertex_update")):
        with pytest.raises(ValueError, match=entry):
            sm.denoise(v, f, **bad)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_what_the_smoothers_are_for():
    """the inequalities of tests/test_meshsmooth_cpu.py, on the device's output"""
    clean, f = mo.icosphere(3)
    v = case("sphere")[0]
    err = lambda p: float(np.abs(np.linalg.norm(p.astype(np.float64), axis=1) - 1.0).mean())
    out = sm.taubin(v, f, iters=10)[0].cpu().numpy()
    assert err(out) < 0.5 * err(v) and abs(mo.volume(out, f) / mo.volume(clean, f) - 1.0) < 0.02
    assert mo.volume(sm.taubin(v, f, iters=10, mu=0.0)[0].cpu().numpy(), f) / mo.volume(clean, f) < 0.9
    clean, f = mo.cube(8)
    v = case("cube")[0]
    out = sm.denoise(v, f, 5, 10, rn=0.6)[0].cpu().numpy()
    before, after = mo.mean_angle(v, f, clean), mo.mean_angle(out, f, clean)
    print(f"cube: mean normal angle {before:.2f} -> {after:.2f} degrees")
    assert after < 0.25 * before and abs(mo.volume(out, f) / mo.volume(v, f) - 1.0) < 0.01
    for k in (5, 10):
        assert mo.mean_angle(sm.taubin(v, f, iters=k)[0].cpu().numpy(), f, clean) > 0.5 * before
    rep = sm.report(v, out, f)
    assert rep["volume_in"] == pytest.approx(mo.volume(v, f), rel=1e-12) and rep["volume_out"] == pytest.approx(mo.volume(out, f), rel=1e-12)
    assert 0 < rep["displacement_mean"] < rep["displacement_max"] < 1.0 and 0 < rep["distance"]["mean"] < rep["mean_edge"]


@pytest.mark.parametrize("coloured", [False, True])
def test_command_line(tmp_path, coloured):
    from svs_hip import ply
    v, f, adj = case("cube")
    col = np.random.default_rng(2).integers(0, 256, (len(v), 3)).astype(np.uint8) if coloured else None
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    ply.write(src, v, col, f)
    how = ["--method", "denoise", "--normal-iters", "2", "--vertex-iters", "3", "--rs", "0.5"] if coloured else ["--iters", "3", "--boundary", "free"]
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        rv, rf, rc, stats = sm.main(["--ply", src, "--ply-out", dst, "--report"] + how)
    want = mo.denoise(v, f, 2, 3, rs=0.5) if coloured else mo.taubin(v, f, iters=3, boundary="free")
    fv, ff = ply.read_mesh(dst)
    assert _steps(fv.astype(np.float32), want, "command line") <= 1.0 and np.array_equal(rv, fv.astype(np.float32))
    assert np.array_equal(ff, f) and np.array_equal(rf, f)
    file_col = ply.read_points(dst)[1]
    assert (file_col is None and rc is None) if not coloured else (np.array_equal(file_col, col) and np.array_equal(rc, col))
    said = text.getvalue()
    assert f"{len(v)} vertices, {len(f)} faces ({len(f)} valid), 1152 edges (0 boundary, 0 non-manifold)" in said
    assert "vertices by flags 0..7: 0 386 0 0 0 0 0 0" in said and "seconds: read" in said and "displacement mean" in said
    rep = stats["report"]
    assert all(np.isfinite(rep[k]) for k in ("displacement_mean", "displacement_max", "volume_in", "volume_out", "mean_edge"))
    assert all(np.isfinite(x) for x in rep["distance"].values()) and rep["displacement_max"] > 0
    assert stats["counts"]["edges"] == 1152 and stats["flags"][1] == 386 and stats["launches"]["adjacency"] == 1
    assert stats["launches"]["taubin"] == (0 if coloured else 1) and stats["launches"]["vertex_update"] == (1 if coloured else 0)
    with contextlib.redirect_stdout(io.StringIO()):
        assert sm.main(["--ply", src, "--ply-out", dst, "--iters", "0"])[3]["report"] is None
    assert np.array_equal(ply.read_mesh(dst)[0].astype(np.float32), v)


VIEW_IDS = (25, 22, 28)
NEAR_EYES = ((2.03, 0.31, 0.42), (1.9, 0.62, 0.5), (1.95, 0.0, 0.28))


def test_runner_switch(tmp_path):
    """the toy scan of test_gpu_meshsimplify.py::test_runner_switch"""
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
    base = [f"outdir={tmp_path}", "filter_only=true", "eval_mask=false", "testlist=scan106", "+tsdf_voxel=0.05", "+tsdf_trunc=0.12"]
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base + ["+tsdf_smooth=3", "+tsdf_smooth_method=denoise", "+tsdf_simplify=0.25"])
    smooth = tmp_path / "tsdf_smooth" / "mvsnet106_l3.ply"
    assert os.path.exists(smooth) and text.getvalue().count("scan106 tsdf smooth seconds: read ") == 1
    fv, ff = ply.read_mesh(str(tmp_path / "tsdf" / "mvsnet106_l3.ply"))
    sv, sf = ply.read_mesh(str(smooth))
    stats = res["smooth_meshes"]["scan106"]
    assert np.array_equal(sf, ff) and sv.shape == fv.shape and not np.array_equal(sv, fv) and stats["faces"] == len(ff) > 0
    assert stats["method"] == "denoise" and stats["launches"] == dict(adjacency=1, taubin=0, face_frames=1, normal_filter=1, vertex_update=1)
    assert stats["counts"]["boundary_edges"] > 0                                 # an open surface: its boundary is held
    assert ply.read_points(str(smooth))[1] is not None                         # the TSDF mesh's colours are kept
    gadj = sm.adjacency(fv, ff)
    want = mo.denoise(fv, ff, 1, 3, rs=2.0 * gadj["mean_edge"], boundary="fixed")      # max(1, 3 // 2) normal passes
    assert _steps(sv.astype(np.float32), want, "runner: denoise of the TSDF mesh") <= 1.0
    edge = (gadj["flags"].cpu().numpy() & mo.BOUNDARY) != 0
    assert edge.any() and np.array_equal(sv[edge], fv[edge])
    # the simplifier read the smoothed mesh
    simple = res["simple_meshes"]["scan106"]
    assert simple["faces_in"] == len(ff) and 0 < simple["faces_out"] <= 0.25 * len(ff)
    from svs_hip import meshsimplify
    again = meshsimplify.simplify_ply(str(smooth), str(tmp_path / "again.ply"), ratio=0.25)
    assert open(tmp_path / "again.ply", "rb").read() == open(tmp_path / "tsdf_simple" / "mvsnet106_l3.ply", "rb").read() and again[3]["faces_in"] == len(ff)
    with pytest.raises(ValueError, match="tsdf_smooth"):
        run.main([f"outdir={tmp_path}", "filter_only=true", "testlist=scan106", "+tsdf_smooth=3"])
