"""CPU checks of the novel-view scores (eval_vsdf.py:186-212): the numpy oracle against the reference-generated fixture
nvs_scores.npz (tests/golden/make_nvs_fixture.py), svs_hip.nvs's ground-truth and mask loader against the arrays the
reference's SceneDataset built, the SSIM restatement on closed forms, and the C-ABI declarations -- no GPU work here."""
import os
import re

import numpy as np
import pytest

import nvs_oracle as no

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NVS_ENTRIES = ("svs_nvs_workspace_bytes", "svs_nvs_score")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "nvs_scores.npz")))


@pytest.fixture(scope="module")
def tree(golden, tmp_path_factory):
    return no.fixture_tree(golden, tmp_path_factory.mktemp("nvs"))


def _pred(case, rf, v):
    name = f"eval_blend_{v:03d}.png" if rf == "blend" else f"eval_{v:03d}.png"
    return no.read_png(os.path.join(case["rendering_dir"], name))


def test_fixture_covers_the_rules(golden):
    """Both datasets, both DTU mask layouts, an unmasked DTU scan, masks that are neither all 0 nor all 1."""
    cases = [str(c) for c in golden["cases"]]
    assert {str(golden[f"{c}/dataset"]) for c in cases} == {"DTU", "BlendedMVS"}
    for c in cases:
        m = golden[f"{c}/mask"]
        if int(golden[f"{c}/scan"]) in (1, 4, 11, 13, 48):
            assert (m == 1).all()
        else:
            assert 0.1 < m.mean() < 0.95, c
            assert (m[..., 0] != m[..., 1]).any() or str(golden[f"{c}/dataset"]) == "BlendedMVS"
        assert golden[f"{c}/gt"].dtype == np.float32 and m.dtype == np.float32


def test_oracle_reproduces_reference_scores(golden, tree):
    """nvs_oracle.score_view on the fixture's files and the reference's arrays == the reference's psnrs / ssims (PSNR to
    1e-4 dB: the reference's mean is float32; SSIM exactly: the fixture's SSIM is the restatement)."""
    for name, case in tree.items():
        for rf in (str(r) for r in golden["result_from"]):
            for i, v in enumerate(case["views"]):
                psnr, ssim = no.score_view(_pred(case, rf, v), golden[f"{name}/gt"][i], golden[f"{name}/mask"][i])
                assert abs(psnr - golden[f"{name}/{rf}/psnr"][i]) <= 1e-4, (name, rf, v)
                assert ssim == golden[f"{name}/{rf}/ssim"][i], (name, rf, v)


def test_load_gt_matches_reference_dataset(golden, tree):
    """svs_hip.nvs.load_gt == the ground truth and masks of the reference's SceneDataset, exactly, for every case (DTU
    mask/ and flat layouts, an unmasked DTU scan, BlendedMVS RGBA masks)."""
    from svs_hip import nvs
    for name, case in tree.items():
        gt, mask = nvs.load_gt(case["data_dir_root"], case["dataset"], case["scan"], case["views"], img_res=case["img_res"])
        assert gt.dtype == np.uint8 and mask.dtype == np.uint8
        np.testing.assert_array_equal(gt.astype(np.float32) / np.float32(255.0), golden[f"{name}/gt"], err_msg=name)
        np.testing.assert_array_equal(mask.astype(np.float32), golden[f"{name}/mask"], err_msg=name)


def test_load_gt_rejects_what_it_does_not_port(tree, tmp_path):
    from PIL import Image
    from svs_hip import nvs
    case = tree["dtu106"]
    with pytest.raises(NotImplementedError, match="cv2.resize"):
        nvs.load_gt(case["data_dir_root"], "DTU", case["scan"], case["views"][:1], img_res=(576, 768))
    with pytest.raises(NotImplementedError):
        nvs.load_gt(case["data_dir_root"], "Tanks", case["scan"], case["views"][:1])
    img = tmp_path / "data" / "DTU" / "scan9" / "image"
    img.mkdir(parents=True)
    Image.fromarray(np.zeros((8, 8), np.uint16)).save(img / "000000.png")
    with pytest.raises(ValueError, match="8-bit"):
        nvs.load_gt(str(tmp_path / "data"), "DTU", 9, [0], img_res=(8, 8), mask=False)


def near_rounding_edge(x, tol=1e-5):
    """x within tol of a point where "%.4f" changes: a float32-vs-float64 difference of ~1e-6 may flip the last digit"""
    return abs(x * 1e4 - np.floor(x * 1e4) - 0.5) < tol * 1e4


def assert_scan_lines(got, want, ref_means):
    """got == want line by line; a number may differ by one unit in the fourth decimal only where the reference's
    unrounded value (ref_means: psnr mean, psnr std, ssim mean, ssim std) sits at a rounding edge."""
    assert len(got) == len(want) == 3 and got[0] == want[0]
    num = re.compile(r"-?\d+\.\d{4}|nan|inf")
    for k, (g, w) in enumerate(zip(got[1:], want[1:])):
        assert num.sub("#", g) == num.sub("#", w), (g, w)
        for j, (a, b) in enumerate(zip(num.findall(g), num.findall(w))):
            if a != b:
                assert near_rounding_edge(ref_means[2 * k + j]) and abs(float(a) - float(b)) <= 1.5e-4, (g, w)


def test_cli_prints_reference_scan_lines(golden, tree, capsys, monkeypatch):
    """python -m svs_hip.nvs prints the reference's SCAN block to four decimals (scores from the oracle: no GPU here)."""
    from svs_hip import nvs
    monkeypatch.setattr(nvs, "score_views", no.score_views)
    for name, case in tree.items():
        for rf in (str(r) for r in golden["result_from"]):
            nvs.main(["--data-dir-root", case["data_dir_root"], "--dataset", case["dataset"], "--scan", str(case["scan"]),
                      "--rendering-dir", case["rendering_dir"], "--views", *map(str, case["views"]), "--result-from", rf,
                      "--img-res", *map(str, case["img_res"])])
            got = capsys.readouterr().out.splitlines()
            p, s = golden[f"{name}/{rf}/psnr"], golden[f"{name}/{rf}/ssim"]
            assert_scan_lines(got, [str(x) for x in golden[f"{name}/{rf}/lines"]], [p.mean(), p.std(), s.mean(), s.std()])
    # the scan this repository documents prints the reference's lines exactly
    case = tree["dtu106"]
    nvs.main(["--data-dir-root", case["data_dir_root"], "--dataset", "DTU", "--scan", "106", "--rendering-dir",
              case["rendering_dir"], "--views", *map(str, case["views"]), "--img-res", *map(str, case["img_res"])])
    assert capsys.readouterr().out.splitlines() == [str(x) for x in golden["dtu106/blend/lines"]]


def test_ssim_constant_images_closed_form():
    """Constant images a, b: S = (2ab + C1) / (a^2 + b^2 + C1) everywhere, C1 = (0.01 * 2)^2 = 4e-4 (data_range 2)."""
    for a, b in ((0.25, 0.75), (1.0, 1.0), (0.0, 1.0), (0.5, 0.49)):
        x = np.full((9, 11, 3), a, np.float32)
        y = np.full((9, 11, 3), b, np.float32)
        a64, b64 = float(np.float32(a)), float(np.float32(b))
        want = (2 * a64 * b64 + 4e-4) / (a64 * a64 + b64 * b64 + 4e-4)
        np.testing.assert_allclose(no.structural_similarity(x, y, multichannel=True), want, rtol=1e-12)
    with pytest.raises(ValueError):
        no.structural_similarity(np.zeros((6, 9), np.float32), np.zeros((6, 9), np.float32))


def test_psnr_edges():
    g = np.full((7, 7, 3), 0.5, np.float32)
    m = np.ones((7, 7, 3), np.float32)
    assert no.psnr_masked(g, g, m) == np.inf
    assert np.isnan(no.psnr_masked(g, g, 0 * m))


def test_header_and_library_export_nvs_entries():
    import importlib.util
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svolsdf_hip.h")).read(), flags=re.S)
    for name in NVS_ENTRIES:
        assert re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(", src), f"{name} is not declared"
    spec = importlib.util.spec_from_file_location("svs_build", os.path.join(ROOT, "s-volsdf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "svs_nvs.hip" in mod.UNITS
    mod.build(verbose=False)
    from svs_hip import lib
    L = lib.load()
    for name in NVS_ENTRIES:
        assert name in lib.SIGNATURES and hasattr(L, name), name
    assert L.svs_nvs_workspace_bytes(25, 576, 768) == 25 * 12 * 36 * 40
    assert L.svs_nvs_workspace_bytes(0, 576, 768) == 0 and L.svs_nvs_workspace_bytes(1, 6, 768) == 0
    assert L.svs_version() == 101
