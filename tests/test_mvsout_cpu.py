"""svs_hip.mvsout without a GPU: the oracle (tests/mvsout_oracle.py) against second opinions, the evaluation-mask file
rule, and the C-ABI of the new entry points (declared, bound with matching argument counts, exported; their argument
checks, which launch nothing)."""
import ctypes
import os
import re

import numpy as np
import pytest

import mvsout_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"svs_mask_dilate_workspace_bytes": 3, "svs_mask_dilate_disk": 8, "svs_mask_resize_any": 12,
           "svs_mvs_confidence": 25}
EINVAL, ESHAPE = -1, -2


# ---- the oracle against second opinions ----
def test_disk_is_the_documented_footprint():
    d = mo.disk(12)
    assert d.shape == (25, 25) and int(d.sum()) == 441
    assert mo.half_widths(12) == [12, 11, 11, 11, 11, 10, 10, 9, 8, 7, 6, 4, 0]
    assert [int(r.sum()) for r in d[12:]] == [2 * w + 1 for w in mo.half_widths(12)]
    assert np.array_equal(d, d.T) and mo.disk(0).tolist() == [[True]]


@pytest.mark.parametrize("hw,r,density", [((1, 1), 1, 1.0), ((7, 5), 2, 0.1), ((13, 17), 3, 0.03), ((20, 9), 12, 0.01),
                                          ((9, 30), 5, 0.02), ((6, 6), 0, 0.3)])
def test_dilate_is_some_set_pixel_within_the_footprint(hw, r, density):
    m = mo.blobs(np.random.default_rng(hw[0] * 31 + r), hw, density)
    assert np.array_equal(mo.dilate(m, r), mo.dilate_brute(m, r))
    assert np.array_equal(mo.dilate(m, r), mo.dilate_spans(m, r))


def test_dilate_is_the_25_span_formulation_at_full_size():
    m = mo.blobs(np.random.default_rng(5), (1200, 1600), 3e-4)
    m[0, 0] = m[1199, 1599] = m[0, 800] = m[600, 0] = 1
    want = mo.dilate(m, 12)
    assert np.array_equal(want, mo.dilate_spans(m, 12)) and 0.05 < want.mean() < 0.5


@pytest.mark.parametrize("src,dst", [((1200, 1600), (1152, 1536)), ((57, 70), (131, 167)), ((40, 52), (40, 52)),
                                     ((1, 37), (3, 20)), ((29, 1), (50, 4)), ((75, 100), (72, 96))])
def test_resize_any_is_float64_bilinear_above_zero(src, dst):
    m = mo.blobs(np.random.default_rng(src[0] + dst[1]), src, 0.05)
    got = mo.resize_any(m, *dst)
    assert got.shape == dst and got.dtype == np.uint8
    assert np.array_equal(got, mo.resize_any_float64(m, *dst))
    assert 0 < got.mean() < 1


def _cascade(rng, sizes):
    maps = [rng.random(s).astype(np.float32) for s in sizes]
    maps[0][::3, ::2] = 0.0
    maps[1][1::2, ::5] = 1.0
    return maps


@pytest.mark.parametrize("sizes,hw", [([(72, 96), (144, 192), (288, 384)], (288, 384)),
                                      ([(288, 384), (576, 768), (1152, 1536)], (1152, 1536)),
                                      ([(31, 45), (50, 77), (101, 67)], (97, 131)),
                                      ([(40, 60)] * 3, (40, 60))])
def test_float32_confidence_is_within_the_derived_bound_of_float64(sizes, hw):
    c = _cascade(np.random.default_rng(hw[0]), sizes)
    f32, f64 = mo.final_confidence(*c, *hw), mo.final_confidence64(*c, *hw)
    assert f32.dtype == np.float32 and f32.shape == hw
    err = float(np.abs(f32.astype(np.float64) - f64).max())
    print(f"{sizes} -> {hw}: max |float32 - float64| {err:.3g} (bound {mo.CONF_BOUND:.3g})")
    assert err <= mo.CONF_BOUND
    if all(s == hw for s in sizes):
        assert np.array_equal(f32, (c[0] * c[1]) * c[2])


# ---- the evaluation-mask file rule ----
def test_eval_mask_path_layouts(tmp_path):
    from svs_hip import mvsout
    root = str(tmp_path)
    for rel in ("BlendedMVS/eval_mask/scan3/mask/00000007.png", "DTU/eval_mask/scan24/mask/025.png",
                "DTU/eval_mask/scan37/022.png"):
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_bytes(b"")
    assert mvsout.eval_mask_path(root, "BlendedMVS", "scan3", 7) == str(tmp_path / "BlendedMVS/eval_mask/scan3/mask/00000007.png")
    assert mvsout.eval_mask_path(root, "DTU", "scan24", 25) == str(tmp_path / "DTU/eval_mask/scan24/mask/025.png")
    assert mvsout.eval_mask_path(root, "DTU", "scan37", 22) == str(tmp_path / "DTU/eval_mask/scan37/022.png")
    with pytest.raises(FileNotFoundError, match="023.png"):
        mvsout.eval_mask_path(root, "DTU", "scan37", 23)
    with pytest.raises(FileNotFoundError, match="00000008.png"):
        mvsout.eval_mask_path(root, "BlendedMVS", "scan3", 8)
    with pytest.raises(NotImplementedError):
        mvsout.eval_mask_path(root, "ETH3D", "scan1", 0)


# ---- the C-ABI ----
def test_new_entries_are_declared_bound_and_exported():
    from svs_hip import lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svolsdf_hip.h")).read(), flags=re.S)
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/svolsdf_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        assert name in lib.SIGNATURES, f"{name} is not in svs_hip/lib.py"
        assert len(lib.SIGNATURES[name][1]) == nargs, name
    if os.path.exists(lib.LIB_PATH):
        L = ctypes.CDLL(lib.LIB_PATH)
        for name in ENTRIES:
            assert hasattr(L, name), f"{name} is not exported by {lib.LIB_PATH}"


def test_entry_points_check_their_arguments():
    from svs_hip import lib
    L = lib.load()
    d = ctypes.c_void_p(64)                      # never dereferenced

    def dilate(mask=d, V=2, Hs=40, Ws=50, r=12, ws=d, out=d):
        return L.svs_mask_dilate_disk(mask, V, Hs, Ws, r, ws, out, None)

    def resize(mask=d, V=2, Hs=40, Ws=50, H=20, W=30, tabs=(d, d, d, d), out=d):
        return L.svs_mask_resize_any(mask, V, Hs, Ws, H, W, *tabs, out, None)

    def conf(c=(d, d, d), sizes=((5, 6), (10, 12), (20, 24)), tabs=(d, d, d, d), H=20, W=24, out=d):
        args = []
        for ck, (h, w) in zip(c, sizes):
            args += [ck, h, w, *tabs]
        return L.svs_mvs_confidence(*args, H, W, out, None)
    for fn, name, bad in ((dilate, b"svs_mask_dilate_disk",
                           [(dict(mask=None), EINVAL), (dict(ws=None), EINVAL), (dict(out=None), EINVAL),
                            (dict(ws=ctypes.c_void_p(68)), EINVAL), (dict(r=33), EINVAL), (dict(r=-1), EINVAL),
                            (dict(V=0), EINVAL), (dict(Hs=0), ESHAPE), (dict(Ws=0), ESHAPE), (dict(Hs=-3), ESHAPE)]),
                          (resize, b"svs_mask_resize_any",
                           [(dict(mask=None), EINVAL), (dict(out=None), EINVAL), (dict(tabs=(d, None, d, d)), EINVAL),
                            (dict(V=0), EINVAL), (dict(Hs=0), ESHAPE), (dict(W=0), ESHAPE), (dict(H=0, W=0), ESHAPE)]),
                          (conf, b"svs_mvs_confidence",
                           [(dict(c=(d, None, d)), EINVAL), (dict(out=None), EINVAL), (dict(tabs=(d, d, d, None)), EINVAL),
                            (dict(H=0), ESHAPE), (dict(sizes=((5, 6), (0, 12), (20, 24))), ESHAPE)])):
        for kw, code in bad:
            assert fn(**kw) == code, (name, kw)
            assert name in L.svs_last_error_string(), (name, kw)
    assert L.svs_mask_dilate_workspace_bytes(3, 1200, 1600) == 2 * 3 * 1200 * 25 * 8
    assert L.svs_mask_dilate_workspace_bytes(1, 1, 1) == 16 and L.svs_mask_dilate_workspace_bytes(0, 5, 5) == 0
