"""CPU checks of image-based rendering (simple_ibr.py:116-235): the numpy oracle against the reference-generated fixture
ibr_blend.npz (tests/golden/make_ibr_fixture.py), the OpenCV restatements on their own properties and against their
definitions (tests/ibr_cases.py), the conditions of the cases that tests/test_gpu_ibr_edges.py runs, and the C-ABI
declarations of the svs_ibr_* entries -- no GPU work here."""
import importlib.util
import os
import re

import numpy as np
import pytest

import ibr_cases as ic
import ibr_oracle as io_
from make_ibr_fixture import digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
IBR_ENTRIES = ("svs_ibr_workspace_bytes", "svs_ibr_weights", "svs_ibr_laplacian_blend")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ibr_blend.npz")))


def test_oracle_reproduces_reference_ibr(golden, tmp_path):
    """ibr_oracle.blend_view == the reference's image_based_render (captured arrays, bit for bit; PNG pixels exactly)."""
    _, _, views = io_.fixture_views(golden, tmp_path)
    step = int(golden["row_step"])
    for vid, (ref, srcs, pred) in views.items():
        got = io_.blend_view(ref, srcs, pred)
        assert np.array_equal(got["geo"], golden[f"geo_{vid}"])
        assert digest(got["fill"]) == str(golden[f"sha_fill_{vid}"]), "fill images differ from the reference's"
        assert digest(got["masks"]) == str(golden[f"sha_masks_{vid}"]), "masks differ from the reference's"
        np.testing.assert_allclose(got["blend"][::step], golden[f"blend_rows_{vid}"], rtol=0, atol=1e-12)
        assert digest(got["blend"]) == str(golden[f"sha_blend_{vid}"])
        np.testing.assert_array_equal(got["png"], golden[f"png_{vid}"])
        assert 0.2 < got["geo"].mean() < 0.8 and (got["masks"][:-1] > 0).any()


def test_pyramid_constant_image():
    for shape in ((16, 24), (8, 8, 3), (2, 2), (1, 4)):
        c = np.full(shape, 0.375)
        np.testing.assert_array_equal(io_.pyr_down(c), np.full(((shape[0] + 1) // 2, (shape[1] + 1) // 2) + shape[2:], 0.375))
        np.testing.assert_array_equal(io_.pyr_up(c), np.full((2 * shape[0], 2 * shape[1]) + shape[2:], 0.375))


def test_pyr_up_borders():
    """pyrUp on the source grid: reflection at the top / left, (src[-2] + 7 src[-1]) / 8 then src[-1] at the bottom /
    right, the interior the [1 6 1] / [4 4] phases."""
    rng = np.random.default_rng(3)
    s = rng.uniform(0, 1, (5, 7))
    up = io_.pyr_up(s)
    # separable: a constant-in-y image isolates the column rule
    row = np.tile(s[:1], (5, 1))
    u = io_.pyr_up(row)[4]
    w = s.shape[1]
    np.testing.assert_allclose(u[0], (6 * s[0, 0] + 2 * s[0, 1]) / 8, rtol=1e-15)
    np.testing.assert_allclose(u[1], (s[0, 0] + s[0, 1]) / 2, rtol=1e-15)
    np.testing.assert_allclose(u[4], (s[0, 1] + 6 * s[0, 2] + s[0, 3]) / 8, rtol=1e-15)
    np.testing.assert_allclose(u[2 * w - 2], (s[0, w - 2] + 7 * s[0, w - 1]) / 8, rtol=1e-15)
    np.testing.assert_allclose(u[2 * w - 1], s[0, w - 1], rtol=1e-15)
    colimg = np.tile(s[:, :1], (1, 4))
    v = io_.pyr_up(colimg)[:, 3]
    h = s.shape[0]
    np.testing.assert_allclose(v[0], (6 * s[0, 0] + 2 * s[1, 0]) / 8, rtol=1e-15)
    np.testing.assert_allclose(v[2 * h - 2], (s[h - 2, 0] + 7 * s[h - 1, 0]) / 8, rtol=1e-15)
    np.testing.assert_allclose(v[2 * h - 1], s[h - 1, 0], rtol=1e-15)
    # a single column / row: 8 c for both phases
    np.testing.assert_allclose(io_.pyr_up(s[:, :1])[:, 1], io_.pyr_up(s[:, :1])[:, 0], rtol=0)
    assert up.shape == (10, 14)


def test_remap_cubic_properties():
    rng = np.random.default_rng(0)
    img = rng.uniform(0, 1, (9, 11, 3)).astype(F32)
    y, x = np.meshgrid(np.arange(9, dtype=F32), np.arange(11, dtype=F32), indexing="ij")
    # integer map points return the image (the weights at fraction 0 are 0, 1, 0, 0), borders included
    np.testing.assert_array_equal(io_.remap_cubic(img, x, y), img)
    np.testing.assert_array_equal(io_.remap_cubic(img[..., 0], x, y), img[..., 0])
    # wholly outside and NaN give 0; the window straddling the edge reads 0 outside
    far = np.array([[-5.0, 20.0, np.nan]], F32)
    np.testing.assert_array_equal(io_.remap_cubic(img, far, np.zeros_like(far)), 0)
    edge = io_.remap_cubic(np.ones((9, 11), F32), np.array([[-0.5]], F32), np.array([[4.0]], F32))
    assert 0 < edge[0, 0] < 1
    # interior: a constant image stays constant up to the table's rounding (A = -0.75 does not reproduce linear ramps)
    const = io_.remap_cubic(np.ones((9, 11), F32), x[2:6, 2:7] + F32(0.3), y[2:6, 2:7] + F32(0.55))
    np.testing.assert_allclose(const, 1, atol=1e-6)
    # a half-pixel step in x only: the four taps of row iy with the weights of fraction 16/32
    got = io_.remap_cubic(img[..., 1], np.array([[4.5]], F32), np.array([[3.0]], F32))[0, 0]
    want = img[3, 3:7, 1].astype(np.float64) @ io_.CUBIC_TAB[16].astype(np.float64)
    np.testing.assert_allclose(got, want, rtol=1e-6)


def test_cubic_weights_sum_to_one():
    tab = io_.CUBIC_TAB
    assert tab.shape == (32, 4) and tab.dtype == F32
    np.testing.assert_array_equal(tab[0], [0, 1, 0, 0])
    np.testing.assert_allclose(tab.astype(np.float64).sum(1), 1.0, atol=1e-7)
    np.testing.assert_allclose(tab[16], [-0.09375, 0.59375, 0.59375, -0.09375], atol=1e-7)


def test_erode_ignores_outside():
    m = np.ones((6, 7))
    np.testing.assert_array_equal(io_.erode(m, np.ones((5, 5))), m)
    m[3, 3] = 0
    e = io_.erode(m, np.ones((5, 5)))
    assert e[1:6, 1:6].sum() == 0 and e[0].sum() == 7 and e[:, 6].sum() == 6


def _header():
    src = open(os.path.join(ROOT, "include", "svolsdf_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_and_library_export_ibr_entries():
    import importlib.util
    src = _header()
    for name in IBR_ENTRIES:
        assert re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(", src), f"{name} is not declared"
    spec = importlib.util.spec_from_file_location("svs_build", os.path.join(ROOT, "s-volsdf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "svs_ibr.hip" in mod.UNITS and "-ffp-contract=off" in mod.UNITS["svs_ibr.hip"]
    mod.build(verbose=False)
    from svs_hip import lib
    L = lib.load()
    for name in IBR_ENTRIES:
        assert name in lib.SIGNATURES and hasattr(L, name), name
    # the size query is host-only
    ws = L.svs_ibr_workspace_bytes(3, 576, 768)
    assert ws >= 4 * 576 * 768 * 4 + 3 * 576 * 768
    assert L.svs_ibr_workspace_bytes(0, 576, 768) == 0 and L.svs_ibr_workspace_bytes(17, 8, 8) == 0
    assert L.svs_version() == 101


# ---- the closed forms against the definition, and the cases of tests/test_gpu_ibr_edges.py -------------------------------
def test_pyramid_closed_forms_match_definition():
    """ibr_oracle.pyr_up / pyr_down (closed-form edge rules) == zero injection, BORDER_REFLECT_101 and a dense 25-tap sum,
    to 1e-14 (measured: 3.3e-16) at every size down to 1x1."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for h in range(1, 6):
        for w in range(1, 7):
            for shape in ((h, w), (h, w, 3)):
                a = rng.uniform(0, 1, shape)
                got, want = io_.pyr_up(a), ic.pyr_up_def(a)
                assert got.shape == want.shape == (2 * h, 2 * w) + shape[2:]
                worst = max(worst, float(np.abs(got - want).max()))
    for shape in [(h, w) for h in (2, 4, 6) for w in (2, 4, 6)] + [(4, 6, 3), (5, 7), (3, 1, 3), (1, 1), (1, 2)]:
        a = rng.uniform(0, 1, shape)
        got, want = io_.pyr_down(a), ic.pyr_down_def(a)
        assert got.shape == want.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2) + shape[2:]
        worst = max(worst, float(np.abs(got - want).max()))
    assert worst <= 1e-14, worst


@pytest.mark.parametrize("case", ic.BLEND_CASES, ids=ic.case_id)
def test_oracle_blend_matches_definition(case):
    """ibr_oracle.laplacian_blending == ibr_cases.blend_def to 1e-14 on every blend case; the float32-storage yardstick
    sits where the GPU bound expects it (1e-8 .. 2e-7, so 10 x stays far below a wrong border rule's 1e-2)."""
    H, W, n_src, kind = case
    fill, masks = ic.blend_case(*case)
    assert fill.shape == (n_src + 1, H, W, 3) and masks.shape == (n_src + 1, H, W) and fill.dtype == masks.dtype == F32
    np.testing.assert_allclose(masks.astype(np.float64).sum(0), 1.0, atol=1e-6)
    want = ic.blend_def(fill, masks)
    got = io_.laplacian_blending(fill, masks[..., None].repeat(3, -1))
    assert np.abs(got - want).max() <= 1e-14
    bound, yard = ic.blend_bound(fill, masks, want)
    assert 1e-8 < yard < 2e-7 and bound < 2.1e-6, (yard, bound)
    if kind == "constant":
        assert np.abs(want - ic.CONSTANT).max() < 1e-7
    if kind == "clip":
        assert ((want == 0.0) | (want == 1.0)).mean() > 0.10
    if kind == "onehot":
        assert set(np.unique(masks)) == {0.0, 1.0}


def test_blend_cases_cover_the_listed_sizes():
    sizes = {c[:2] for c in ic.BLEND_CASES}
    assert sizes == {(8, 8), (8, 16), (16, 8), (8, 24), (24, 8), (16, 16), (24, 40), (40, 24), (8, 264)}
    for hw in sizes:
        ns = {c[2] for c in ic.BLEND_CASES if c[:2] == hw}
        assert len(ns) >= 2 and ns <= {1, 2, 16}, (hw, ns)
    assert (8, 8, 16) in {c[:3] for c in ic.BLEND_CASES} and (8, 264, 16) in {c[:3] for c in ic.BLEND_CASES}
    assert {c[3] for c in ic.BLEND_CASES} == {"random", "onehot", "constant", "clip"}


def test_laplacian_pyramid_reconstructs():
    """One entry with mask 1: the blend is the clipped image itself (what test_blend_levels_alone asks of the kernels)."""
    for H, W in ((8, 8), (8, 24), (24, 8), (8, 264)):
        img = np.random.default_rng(H + W).uniform(0, 1, (H, W, 3)).astype(F32)
        fill = np.stack([img, np.zeros_like(img)])
        masks = np.stack([np.ones((H, W), F32), np.zeros((H, W), F32)])
        assert np.abs(ic.blend_def(fill, masks) - img).max() <= 1e-14


def _erode_brute(b):
    """minimum over the in-image part of the 5x5 window, pixel by pixel"""
    H, W = b.shape
    out = np.zeros_like(b)
    for y in range(H):
        for x in range(W):
            out[y, x] = b[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3].min()
    return out


@pytest.mark.parametrize("hwn", ic.WEIGHTS_CASES, ids=ic.case_id)
def test_weights_case_conditions(hwn):
    """Every weights case satisfies its own conditions (the builder asserts the threshold ones on the oracle's result)."""
    H, W, n = hwn
    c = ic.weights_case(H, W, n)
    on = list(c["on"])
    assert ic.near_threshold(c["weights"]).sum() == 0
    # at most four sources on; the others 0 everywhere; the high-index variant exists
    assert c["geo"].sum(0).max() == min(n, 4) and not c["geo"][[s for s in range(n) if s not in on]].any()
    assert (min(on) >= 4) == (hwn == ic.HIGH_SOURCES_ON)
    # every cubic_tap mode occurs, on crafted pixels and (mode 1, 2) on identity pixels
    assert set(np.unique(c["mode"][c["crafted"]])) == {0, 1, 2}
    assert set(np.unique(c["mode"][~c["crafted"]])) == {1, 2}
    names = set(c["crafted_names"])
    for axis, size in (("x", W), ("y", H)):
        assert {axis + "=" + nm for nm, _ in ic.limit_values(size)} <= names
    assert {"corner00", "cornerHW", "tie", "tie'", "2+1/64"} <= names
    assert ({"phase%d" % k for k in range(32)} <= names) == (H * W > 64)
    assert c["crafted"][0].any() and c["crafted"][n - 1].any() and c["crafted"].sum() == len(names) * len({0, n - 1})
    # hole positions: corners, edge middles, both sides of every seam, distance 2 and 3 from a seam and from the edge
    at = {(y, x) for _, _, y, x in c["holes"]}
    assert all(c["geo"][s, y, x] == 0 for _, s, y, x in c["holes"])
    want = {(0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1),
            (2, W - 1), (3, W - 1)}
    if H * W > 64:
        want |= {(0, 0), (0, 2), (0, 3)}
    assert want <= at
    for s in range(ic.SEAM, W, ic.SEAM):
        assert {s + d for d in (-3, -2, -1, 0, 1, 2, 3) if s + d < W} <= {x for _, x in at}
    for s in range(ic.SEAM, H, ic.SEAM):
        assert {s + d for d in (-3, -2, -1, 0, 1, 2, 3) if s + d < H} <= {y for y, _ in at}
    # the thresholds are the geometric pattern away from the crafted maps and the planted direction windows
    thr = c["weights"][:-1] > 0.2
    free = ~c["crafted"] & ~c["planted"]
    assert np.array_equal(thr[free], c["geo"].astype(bool)[free])
    # the planted windows do what they are planted for
    assert c["n_anti"] > 0 and (c["n_nan"] > 0 or H * W <= 64)
    # erosion: neither empty nor full, and the oracle's separable form equals a per-pixel minimum
    alive = c["masks"][on] > 0
    assert 0 < alive.sum() < alive.size
    if H * W > 64:
        assert 0.2 < alive.mean() < 0.9
    for s in on:
        np.testing.assert_array_equal(io_.erode(thr[s] * 1.0, np.ones((5, 5), np.uint8)), _erode_brute(thr[s] * 1.0))
    if H * W <= 64:
        assert alive[0, 0, 0], "pixel (0, 0) survives only because outside pixels take no part"
    assert not c["masks"][[s for s in range(n) if s not in on]].any()
    np.testing.assert_allclose(c["masks"].astype(np.float64).sum(0), 1.0, atol=1e-6)


def _bicubic64(img, mx, my):
    """A plain float64 bicubic: A = -0.75, coordinates quantised to 1/32 with round-half-even, zero outside the image."""
    H, W = img.shape[:2]
    out = np.zeros(mx.shape + img.shape[2:])

    def coeffs(t, A=-0.75):
        d = np.array([1 + t, t, 1 - t, 2 - t])
        return np.where(d <= 1, ((A + 2) * d - (A + 3)) * d * d + 1, ((A * d - 5 * A) * d + 8 * A) * d - 4 * A)

    for idx in np.ndindex(mx.shape):
        fx, fy = np.float32(mx[idx]) * np.float32(32), np.float32(my[idx]) * np.float32(32)
        if not (abs(fx) < 2.1e9 and abs(fy) < 2.1e9):
            continue
        qx, qy = int(np.rint(fx)), int(np.rint(fy))                  # numpy rounds half to even
        ix, iy = max(min(qx // 32, 32767), -32768), max(min(qy // 32, 32767), -32768)
        wx, wy = coeffs((qx % 32) / 32.0), coeffs((qy % 32) / 32.0)
        for i in range(4):
            for j in range(4):
                y, x = iy - 1 + i, ix - 1 + j
                if 0 <= y < H and 0 <= x < W:
                    out[idx] += wy[i] * wx[j] * img[y, x]
    return out


@pytest.mark.parametrize("hwn", ic.WEIGHTS_CASES, ids=ic.case_id)
def test_remap_cubic_on_crafted_maps(hwn):
    """ibr_oracle.remap_cubic on the crafted maps == a float64 bicubic written out above, to 1e-6, and exactly at integer
    coordinates (the weights there are 0, 1, 0, 0)."""
    H, W, n = hwn
    c = ic.weights_case(H, W, n)
    for s in sorted({0, n - 1}):
        img = c["imgs"][s]
        got = io_.remap_cubic(img, c["x2d"][s], c["y2d"][s])
        want = _bicubic64(img.astype(np.float64), c["x2d"][s], c["y2d"][s])
        assert np.abs(got - want).max() <= 1e-6
        with np.errstate(invalid="ignore"):
            whole = (np.rint(c["x2d"][s]) == c["x2d"][s]) & (np.rint(c["y2d"][s]) == c["y2d"][s]) & \
                    (np.abs(c["x2d"][s]) < 3e4) & (np.abs(c["y2d"][s]) < 3e4)
        assert whole.sum() > (~c["crafted"][s]).sum()               # the identity pixels and the whole-number limits
        np.testing.assert_array_equal(got[whole], want[whole].astype(F32))
    # the ties: x * 32 = k + 0.5 exactly, rounded to the even neighbour
    for k, want_k in ((ic.TIE_EVEN, ic.TIE_EVEN), (ic.TIE_ODD, ic.TIE_ODD + 1)):
        v = np.float32(2 + (k + 0.5) / 32)
        assert float(v) * 32 == 64 + k + 0.5 and int(np.rint(v * np.float32(32))) == 64 + want_k


def test_workspace_query_rejects_what_the_entries_reject():
    """svs_ibr_workspace_bytes (host only): 0 for every size svs_ibr_weights / svs_ibr_laplacian_blend reject, and at
    least the planes of the layout comment for the sizes they accept."""
    spec = importlib.util.spec_from_file_location("svs_build", os.path.join(ROOT, "s-volsdf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from svs_hip import lib
    L = lib.load()
    for n, h, w in ((1, 8, 12), (1, 12, 8), (1, 0, 8), (1, 8, 0), (1, 4, 8), (1, 8, 4), (1, 4, 4), (17, 8, 8), (0, 8, 8),
                    (-1, 8, 8), (3, -8, 8), (3, 20, 24), (1, 8192, 8200)):
        assert L.svs_ibr_workspace_bytes(n, h, w) == 0, (n, h, w)
    for n, h, w in ((1, 8, 8), (16, 8, 8), (2, 24, 40), (16, 8, 264), (3, 576, 768), (1, 8192, 8192)):
        got = L.svs_ibr_workspace_bytes(n, h, w)
        planes = ic.workspace_planes(n, h, w)
        assert planes <= got <= planes + 10 * ic.ALIGN, (n, h, w, got, planes)
        assert ic.thr_offset(n, h, w) + n * h * w <= got
