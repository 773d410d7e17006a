"""Screened svs_hip.poisson without a GPU: the float64 oracle (tests/poisson_screen_oracle.py) against a direct solve of the
screened system, what screening buys on a cloud of uneven density (on the oracle alone), the density rule, the runner key, the
command line, and the argument checks of the svs_screened_* entries (which come before any device work)."""
import ctypes

import numpy as np
import pytest

import poisson_oracle as po
import poisson_screen_oracle as so

TOL = 1e-4
# iterations to tol 1e-4 at screen 0, 1, 4, 16 on the uneven cloud, float32 and float64 storage alike
ITERATIONS = {(12, 13, 14): (33, 25, 22, 20), (24, 24, 24): (55, 44, 38, 34)}


# ---- the oracle against a direct solve -----------------------------------------------------------------------------------------
def test_uneven_cloud_is_the_one_the_figures_were_taken_on():
    pts, nrm = so.uneven_cloud()
    assert len(pts) == 1699 and nrm.dtype == np.float32
    s = so.uneven_system()
    assert s["counted"] == 1699 and s["W"].min() >= 0 and abs(float(s["W"].astype(np.float64).sum()) - 1699) <= 1e-3


@pytest.mark.parametrize("dims", po.CG_GRIDS)
def test_pcg_agrees_with_the_direct_solve(dims):
    s = so.uneven_system(dims)
    rhs = s["rhs"].astype(np.float64)
    for screen, want in zip(so.SCREENS, ITERATIONS[dims]):
        weight = so.screen_weight(s["W"], s["counted"], screen, 1.0)[0]
        direct = so.direct_solve(rhs, s["W"], 1.0, weight)
        assert so.true_residual(direct, rhs, s["W"], 1.0, weight) <= 1e-12
        e32, e64 = so.uneven_solution(dims, screen, "float32"), so.uneven_solution(dims, screen, "float64")
        err = lambda v: float(np.linalg.norm(v - direct) / np.linalg.norm(direct))
        true = so.true_residual(e32["x"], rhs, s["W"], 1.0, weight)
        print(f"{dims} screen {screen:g} (weight {weight:.4f}): {e32['info']['iterations']} / {e64['info']['iterations']} iterations "
              f"(float32 / float64 storage), true residual {true / TOL:.3f} tol, error against the direct solve {err(e32['x']):.3e} / "
              f"{err(e64['x']):.3e}")
        assert e32["info"]["converged"] and e64["info"]["converged"]
        assert e32["info"]["iterations"] == e64["info"]["iterations"] == want
        assert 0.7 * TOL <= true <= 0.95 * TOL
        assert 4e-5 <= err(e32["x"]) <= 3.5e-4 and abs(err(e32["x"]) - err(e64["x"])) <= 1e-3 * err(e64["x"])


@pytest.mark.parametrize("dims", po.CG_GRIDS)
def test_weight_zero_is_plain_conjugate_gradients(dims):
    """d is then the constant 6 / h^2: the same iterates as `po.cg` up to rounding, the same count"""
    s = so.uneven_system(dims)
    x, info = so.pcg(s["rhs"], s["W"], 1.0, 0.0, tol=TOL)
    x0, info0 = po.cg(s["rhs"], 1.0, tol=TOL)
    assert info["iterations"] == info0["iterations"] == ITERATIONS[dims][0]
    assert np.abs(x - x0).max() <= 1e-9 * np.abs(x0).max()
    assert np.array_equal(so.apply(x0, s["W"], 1.0, 0.0), po.apply(x0, 1.0))
    with pytest.raises(ValueError, match="no normal field"):
        so.pcg(np.zeros((4, 4, 4)), np.ones((4, 4, 4)), 1.0, 1.0)


def test_stopping_rules_on_the_oracle():
    s = so.uneven_system()
    w = so.screen_weight(s["W"], s["counted"], 4.0, 1.0)[0]
    x, info = so.pcg(s["rhs"], s["W"], 1.0, w, tol=TOL, max_iter=7, check_every=32, storage=np.float32)
    assert info["iterations"] == 7 and not info["converged"] and np.isfinite(x).all()
    _, info = so.pcg(s["rhs"], s["W"], 1.0, w, tol=TOL, check_every=32, storage=np.float32)     # 38 are needed: seen at 64
    assert info["iterations"] == 64 and info["converged"]


# ---- what screening buys -----------------------------------------------------------------------------------------------------------
def test_screening_keeps_the_level_set_on_an_uneven_cloud():
    off, on = so.uneven_solution(screen=0.0), so.uneven_solution(screen=4.0)
    worst_off, worst_on = po.worst_misclassified(off["x"], off["level"]), po.worst_misclassified(on["x"], on["level"])
    r_off, r_on = so.radial_error(off["x"], off["level"]), so.radial_error(on["x"], on["level"])
    print(f"uneven sphere: unscreened level {off['level']:.4f}, worst wrongly classified node {worst_off:.3f} voxel, radial error "
          f"{r_off}; screen 4 level {on['level']:.4f}, worst {worst_on:.3f}, radial {r_on}")
    assert worst_off > 1.0 and worst_on < 0.5
    assert r_on["rms"] < 0.5 * r_off["rms"]
    even = so.uneven_solution(screen=4.0, even=True)
    worst_even = po.worst_misclassified(even["x"], even["level"])
    print(f"even sphere at screen 4: worst wrongly classified node {worst_even:.3f} voxel, radial {so.radial_error(even['x'], even['level'])}")
    assert worst_even < 0.5


def test_radial_error_of_an_exact_distance_field():
    d = po.node_distance()
    fig = so.radial_error(d, 0.0)
    # trilinear interpolation of a field of curvature 1 / RADIUS is off by at most h^2 / (8 RADIUS) per axis: 3 / 64 voxel
    assert fig["rms"] <= fig["max"] <= 3.0 / (8.0 * po.RADIUS)
    assert abs(so.radial_error(d, 1.0)["rms"] - 1.0) <= 0.05


# ---- the density rule -----------------------------------------------------------------------------------------------------------------
def test_screen_weight():
    import torch
    from svs_hip import poisson
    W = np.zeros((3, 4, 5), np.float32)
    W[1, 1, 1:4] = (0.5, 2.0, 1.5)
    W[2, 3, 4] = 1e-30                                                          # touched, however lightly
    for fn in (so.screen_weight, poisson.screen_weight):
        assert fn(W, 8, 4.0, 1.0) == (2.0, 2.0)
        assert fn(W, 8, 4.0, 0.5) == (8.0, 2.0)                                 # a grid of half the spacing in the same unit
        assert fn(W, 2, 16.0, 2.0) == (8.0, 0.5)
        assert fn(W, 8, 0.0, 1.0) == (0.0, 2.0)
    assert poisson.screen_weight(torch.from_numpy(W), 8, 4.0, 1.0) == (2.0, 2.0)
    s = so.uneven_system()
    assert poisson.screen_weight(s["W"], s["counted"], 4.0, 1.0) == so.screen_weight(s["W"], s["counted"], 4.0, 1.0)
    with pytest.raises(ValueError, match="no density"):
        poisson.screen_weight(np.zeros((2, 2, 2), np.float32), 5, 4.0, 1.0)
    with pytest.raises(ValueError, match="voxel"):
        poisson.screen_weight(W, 8, 4.0, 0.0)


# ---- runner, command line, C entries ---------------------------------------------------------------------------------------------
def test_runner_key_is_validated():
    from svs_hip import run
    both = ["+cloud_clean=true", "+cloud_poisson=1.5"]
    args = run.apply_overrides(run.default_args(), both + ["+cloud_poisson_screen=4"])
    assert run.check_cloud_poisson_screen(args) == 4.0 and run.check_cloud_poisson(args) == 1.5
    assert "cloud_poisson_screen" not in run.default_args() and run.check_cloud_poisson_screen(run.default_args()) is None
    assert run.check_cloud_poisson_screen(run.apply_overrides(run.default_args(), both)) is None
    with pytest.raises(ValueError, match="cloud_poisson_screen"):
        run.check_cloud_poisson_screen(run.apply_overrides(run.default_args(), ["+cloud_clean=true", "+cloud_poisson_screen=4"]))
    for bad in ("0", "-1", "true", "abc", ".inf", ".nan"):
        with pytest.raises(ValueError, match="cloud_poisson_screen"):
            run.check_cloud_poisson_screen(run.apply_overrides(run.default_args(), both + [f"+cloud_poisson_screen={bad}"]))
    with pytest.raises(ValueError, match="cloud_poisson_screen"):
        run.run_help(run.apply_overrides(run.default_args(), ["+cloud_poisson_screen=4"]), select_device=False)
    assert "+cloud_poisson_screen=S" in run.__doc__ and "no default value" in run.__doc__


def test_command_line():
    from svs_hip import poisson
    base = ["--ply", "i", "--ply-out", "o", "--voxel", "1.5"]
    assert poisson.parse_args(base).screen is None
    assert poisson.parse_args(base + ["--screen", "4"]).screen == 4.0
    assert poisson.parse_args(base + ["--screen", "0"]).screen == 0.0
    for bad in ("-1", "nan", "inf", "x"):
        with pytest.raises(SystemExit):
            poisson.parse_args(base + ["--screen", bad])
    for doc in (poisson.__doc__, poisson.reconstruct.__doc__, poisson.reconstruct_ply.__doc__):
        assert "no default value" in doc and "real scan" in doc
    assert "nobody has tried them on a real scan" in poisson.reconstruct.__doc__
    assert set(poisson.ENTRY_CALLS) == {"splat", "divergence", "apply", "cg", "sample", "keep"} and set(poisson.SCREENED_CALLS) == {"apply", "pcg"}


def test_reconstruct_refuses_a_bad_screen(tmp_path):
    """before anything else is looked at: no GPU, no file"""
    from svs_hip import poisson
    pts, nrm = po.sphere_cloud(100)
    for bad in (-1, -1.0, float("nan"), float("inf"), "4", True):
        with pytest.raises(ValueError, match="screen"):
            poisson.reconstruct(pts, nrm, voxel=1.0, screen=bad)
        with pytest.raises(ValueError, match="screen"):
            poisson.reconstruct_ply(str(tmp_path / "none.ply"), str(tmp_path / "out.ply"), 1.0, screen=bad)
    assert poisson.check_screen(None) is None and poisson.check_screen(0) is None and poisson.check_screen(0.0) is None
    assert poisson.check_screen(4) == 4.0


def test_symbols_are_in_the_ctypes_table():
    from svs_hip import lib
    want = {"svs_screened_apply": 9, "svs_screened_pcg_workspace_bytes": 3, "svs_screened_pcg": 16}
    assert {k: len(lib.SIGNATURES[k][1]) for k in lib.SIGNATURES if k.startswith("svs_screened")} == want
    assert lib.SIGNATURES["svs_screened_pcg"][1][12:15] == [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double),
                                                            ctypes.POINTER(ctypes.c_int)]
    assert lib.SIGNATURES["svs_screened_pcg"][1][5:8] == [ctypes.c_double] * 3 and lib.SIGNATURES["svs_screened_apply"][1][5:7] == [ctypes.c_double] * 2
    assert lib.SIGNATURES["svs_screened_pcg_workspace_bytes"][0] is ctypes.c_size_t
    assert lib.ABI_VERSION == 101
    L = lib.load()
    assert L.svs_version() == 101 and all(hasattr(L, k) for k in want)


def test_argument_errors_name_the_entry():
    """the checks come before any device work: no GPU needed"""
    from svs_hip import lib
    L = lib.load()
    d, e = 4096, 8192                                                           # never dereferenced
    it, res, conv = ctypes.byref(ctypes.c_int(0)), ctypes.byref(ctypes.c_double(0)), ctypes.byref(ctypes.c_int(0))
    calls = {
        "svs_screened_apply": lambda g=(4, 4, 4), h=1.0, w=1.0, x=d, W=d, y=e: L.svs_screened_apply(x, W, *g, h, w, y, None),
        "svs_screened_pcg": lambda g=(4, 4, 4), h=1.0, w=1.0, x=d, W=d, y=e, tol=1e-4, mi=10, ce=1, ws=d:
            L.svs_screened_pcg(x, W, *g, h, w, tol, mi, ce, ws, y, it, res, conv, None),
    }
    for name, call in calls.items():
        for g in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (2048, 2048, 2048)):
            assert call(g=g) == lib.ESHAPE and L.svs_last_error_string().startswith(name.encode()), (name, g)
        for null in ("x", "W", "y"):
            assert call(**{null: None}) == lib.EINVAL and L.svs_last_error_string().startswith(name.encode() + b": bad argument"), (name, null)
        for h in (0.0, -1.0, float("nan"), float("inf")):
            assert call(h=h) == lib.EINVAL and b"spacing" in L.svs_last_error_string() and L.svs_last_error_string().startswith(name.encode())
        for w in (-1e-300, -1.0, float("nan"), float("inf"), float("-inf")):
            assert call(w=w) == lib.EINVAL and b"weight" in L.svs_last_error_string() and L.svs_last_error_string().startswith(name.encode())
    assert calls["svs_screened_apply"](y=d) == lib.EINVAL and b"same array" in L.svs_last_error_string()
    pcg = calls["svs_screened_pcg"]
    for tol, mi, ce in ((0.0, 10, 1), (1.0, 10, 1), (1e-4, 0, 1), (1e-4, 10, 0)):
        assert pcg(tol=tol, mi=mi, ce=ce) == lib.EINVAL and L.svs_last_error_string().startswith(b"svs_screened_pcg")
    assert pcg(ws=None) == lib.EINVAL
    assert L.svs_screened_pcg(d, d, 4, 4, 4, 1.0, 1.0, 1e-4, 10, 1, d, e, None, res, conv, None) == lib.EINVAL
    # one more row of partial sums than the unscreened solve, nothing else
    assert L.svs_poisson_cg_workspace_bytes(24, 24, 24) < L.svs_screened_pcg_workspace_bytes(24, 24, 24) <= \
        L.svs_poisson_cg_workspace_bytes(24, 24, 24) + 8 * 2048 + 256
    assert L.svs_screened_pcg_workspace_bytes(1, 4, 4) == 0
