"""CPU checks of image-based rendering (simple_ibr.py:116-235): the numpy oracle against the reference-generated fixture
ibr_blend.npz (tests/golden/make_ibr_fixture.py), the OpenCV restatements on their own properties, and the C-ABI
declarations of the svs_ibr_* entries -- no GPU work here."""
import os
import re

import numpy as np
import pytest

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
