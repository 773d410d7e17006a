"""`svs_cloud_normals` (normals_kernel of csrc/svs_cloudknn.hip, the Jacobi of csrc/svs_jacobi3.h) on the GPU, held to the
criterion of tests/normals_cases.py on EVERY point with at least three points in its set: the eigen-equation against a
covariance summed on the host with math.fsum, the length, the curvature, the angle where the spectrum is clear; exact axes
and signs on the exact cases.  tests/test_normals_cases_cpu.py shows that the float64 oracle alone meets the same bounds on
the same cases and that the cases reach the branches they name.  Each test prints its worst figures before it asserts.

After the criterion every case is also held to the kernel restated in numpy in its operation order (nc.kernel_normals), bit
for bit: the unit is compiled with -ffp-contract=off and holds only IEEE float64 operations, and equality is what lets the
mutants that tests/test_normals_cases_cpu.py runs on the restatement speak for the kernel itself."""
import numpy as np
import pytest
import torch

import cloudclean_oracle as co
import normals_cases as nc

pytestmark = pytest.mark.gpu


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def H(t):
    return t.cpu().numpy()


def run(c):
    from svs_hip import clouds
    n, curv = clouds.normals_from_neighbors(G(c["pts"]), G(c["idx"]), c["include_self"], c["view_index"], c["centres"])
    n, curv = H(n), H(curv)
    assert n.dtype == np.float32 and curv.dtype == np.float32 and n.shape == (len(c["pts"]), 3) and curv.shape == (len(c["pts"]),)
    return n, curv


def judge(c):
    """run the case, print its figures, assert everything it asks -> the outputs"""
    n, curv = run(c)
    f, bad = nc.all_failures(c, n, curv)
    rn, rc = nc.kernel_normals(c["pts"], c["idx"], c["include_self"], c["view_index"], c["centres"])
    differ = int(((n.view(np.uint32) != rn.view(np.uint32)).any(1) | (curv.view(np.uint32) != rc.view(np.uint32))).sum())
    print(f"{c['name']}: {nc.summary(f)}; {differ} rows differ from the restated kernel")
    assert not bad, (c["name"], bad, nc.summary(f))
    assert differ == 0, (c["name"], differ)
    return n, curv


@pytest.mark.parametrize("name", nc.NAMES["scan"])
def test_scan_scale(name):
    """the unit clouds at the coordinates of a DTU scan, of a small scene and a million units from the origin: the criterion,
    the unit cloud's normals and curvatures, and the whole function (its own neighbour search) bit for bit"""
    from svs_hip import clouds
    c = nc.case(name)
    base = nc.case(c["base"])
    n, curv = judge(c)
    clear = (base["lam"][:, 1] - base["lam"][:, 0]) >= nc.CLEAR * base["lam"][:, 2]
    ang = co.angle(n, base["oracle"][0])
    off = np.abs(curv - base["oracle"][1])
    print(f"{name}: against the unit cloud's oracle: angle {ang[clear].max():.3e} rad on {int(clear.sum())} clear points, "
          f"curvature off by {off.max():.3e}")
    assert clear.mean() >= 0.95 and (ang[clear] <= nc.ANGLE).all() and (off <= nc.CURVATURE).all()
    pts = G(c["pts"])
    _, idx = clouds.knn(pts, pts, c["k"], c["radius"], exclude_same_index=True)
    assert np.array_equal(H(idx), c["idx"])
    n2, curv2 = clouds.estimate_normals(pts, c["k"], c["radius"], view_index=c["view_index"], centres=c["centres"])
    assert np.array_equal(H(n2).view(np.uint32), n.view(np.uint32)) and np.array_equal(H(curv2).view(np.uint32), curv.view(np.uint32))


@pytest.mark.parametrize("name", nc.NAMES["ladder"])
def test_anisotropy_ladder(name):
    """planes, a graded needle, a near-tie at the bottom of the spectrum, a near-isotropic ball: 8 fixed sweeps must do"""
    judge(nc.case(name))


def test_anisotropy_ladder_twice_gives_equal_bits():
    for name in nc.NAMES["ladder"]:
        (a, ca), (b, cb) = run(nc.case(name)), run(nc.case(name))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ca.view(np.uint32), cb.view(np.uint32)), name


@pytest.mark.parametrize("name", nc.NAMES["exact"])
def test_exact_degeneracies(name):
    """integer sets whose covariance is diagonal with equal entries (the tie rule, no rotation), exactly coplanar (the
    clamp), all coincident (zero trace): the stated axis with the stated sign, a curvature that is never below +0"""
    c = nc.case(name)
    n, curv = judge(c)
    print(f"{name}: normal {n[0].tolist()}, curvature {float(curv[0])!r}")
    assert np.isfinite(n).all() and not np.signbit(curv).any()


@pytest.mark.parametrize("name", nc.NAMES["slots"])
def test_slots(name):
    """k = 2, 3, 32; with and without the point itself; -1 and indices >= n between the valid slots; valid slots only at
    the end; exactly three points in the set, and exactly two (zeros)"""
    c = nc.case(name)
    n, curv = judge(c)
    dead = c["m"] < 3
    assert not n[dead].any() and not curv[dead].any() and (np.abs(np.linalg.norm(n[~dead].astype(np.float64), axis=1) - 1) <= nc.LENGTH).all()


@pytest.mark.parametrize("name", nc.NAMES["facing"])
def test_facing(name):
    """view indices outside [0, n_views) are clamped; a centre in the tangent plane (dot == 0) does not flip; of two centres
    at the same distance the first one decides"""
    c = nc.case(name)
    n, _ = judge(c)
    if name == "facing-view_clamp":
        from svs_hip import clouds
        n2, _ = clouds.normals_from_neighbors(G(c["pts"]), G(c["idx"]), True, c["clamped"], c["centres"])
        assert np.array_equal(H(n2).view(np.uint32), n.view(np.uint32))


@pytest.mark.parametrize("n_points", nc.COUNTS)
def test_point_counts(n_points):
    """one point, one short of a block, a block, one more, two blocks and one"""
    judge(nc.case(f"count-{n_points}"))


def test_c_entry_without_curvature():
    """curvature = NULL through the C entry: the same normals, and nothing written behind them"""
    from svs_hip import clouds, lib
    from svs_hip.ops import _ptr, _stream
    c = nc.case("count-257")
    n = len(c["pts"])
    pts, idx = G(c["pts"]), G(c["idx"])
    want, want_curv = clouds.normals_from_neighbors(pts, idx)
    guard = 1024
    buf = torch.full((3 * n + guard,), -12345.0, dtype=torch.float32, device=pts.device)
    L = lib.load()
    lib.check(L.svs_cloud_normals(_ptr(pts), n, _ptr(idx), idx.shape[1], 1, None, None, 0, _ptr(buf), None, _stream()),
              "svs_cloud_normals")
    torch.cuda.synchronize()
    got = H(buf)
    assert np.array_equal(got[:3 * n].view(np.uint32), H(want).reshape(-1).view(np.uint32))
    assert (got[3 * n:] == np.float32(-12345.0)).all()
    f, bad = nc.all_failures(c, got[:3 * n].reshape(n, 3), H(want_curv))
    print(f"curvature = NULL, n = {n}: {nc.summary(f)}; {guard} guard words untouched")
    assert not bad
