"""GPU parity of the novel-view scores (eval_vsdf.py:186-212, csrc/svs_nvs.hip) through the C-ABI and svs_hip.nvs, against
the reference-generated fixture nvs_scores.npz and the numpy oracle (which reproduces the fixture: tests/test_nvs_cpu.py).
The kernel's window moments are exact integers and only S is float64, so SSIM agrees with the float64 oracle to ~1e-10;
PSNR differs from the reference's float32 value by its float32 rounding (1e-4 dB bound)."""
import os

import numpy as np
import pytest
import torch

import nvs_oracle as no

pytestmark = pytest.mark.gpu
SVS_EINVAL, SVS_ESHAPE = -1, -2
PSNR_TOL, SSIM_TOL = 1e-4, 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "nvs_scores.npz")))


@pytest.fixture(scope="module")
def tree(golden, tmp_path_factory):
    return no.fixture_tree(golden, tmp_path_factory.mktemp("nvs"))


def random_views(seed, V, H, W, p_mask=0.8):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (40 + 150 * yy / H + 50 * np.sin(xx / 5.0))[None, ..., None]
    gt = np.clip(np.rint(base + rng.normal(0, 15, (V, H, W, 3))), 0, 255).astype(np.uint8)
    noise = np.rint(rng.normal(0, 6, gt.shape)).astype(int)
    noise[rng.random(gt.shape) < 0.3] = 0
    pred = np.clip(gt.astype(int) + noise, 0, 255).astype(np.uint8)
    mask = (rng.random(gt.shape) < p_mask).astype(np.uint8)
    return pred, gt, mask


def check_vs_oracle(pred, gt, mask):
    from svs_hip import nvs
    psnr, ssim = nvs.score_views(pred, gt, mask)
    want_p, want_s = no.score_views(pred, gt, mask)
    assert np.abs(psnr - want_p).max() <= PSNR_TOL, float(np.abs(psnr - want_p).max())
    assert np.abs(ssim - want_s).max() <= SSIM_TOL, float(np.abs(ssim - want_s).max())
    return psnr, ssim


def test_fixture_views_match_reference(dev, golden, tree):
    """score_views on the fixture's PNG codes and the reference's ground truth and masks: the reference's psnrs and
    ssims, every case and result_from."""
    from svs_hip import nvs
    worst_p = worst_s = 0.0
    for name, case in tree.items():
        gt = np.rint(golden[f"{name}/gt"] * 255).astype(np.uint8)
        mask = golden[f"{name}/mask"].astype(np.uint8)
        for rf in (str(r) for r in golden["result_from"]):
            pred = np.stack([no.read_png(nvs.prediction_path(case["rendering_dir"], v, rf)) for v in case["views"]])
            psnr, ssim = nvs.score_views(pred, gt, mask)
            worst_p = max(worst_p, float(np.abs(psnr - golden[f"{name}/{rf}/psnr"]).max()))
            worst_s = max(worst_s, float(np.abs(ssim - golden[f"{name}/{rf}/ssim"]).max()))
    print(f"fixture: max |dPSNR| {worst_p:.3g} dB, max |dSSIM| {worst_s:.3g}")
    assert worst_p <= PSNR_TOL and worst_s <= SSIM_TOL


def test_full_size_25_views(dev):
    """25 random 576x768 views (one DTU scan) against the float64 oracle."""
    pred, gt, mask = random_views(3, 25, 576, 768)
    psnr, ssim = check_vs_oracle(pred, gt, mask)
    assert np.isfinite(psnr).all() and (ssim < 1).all()


@pytest.mark.parametrize("hw", [(7, 7), (13, 70), (577, 769), (16, 64), (17, 65)])
def test_sizes_off_the_tile_grid(dev, hw):
    pred, gt, mask = random_views(11 + hw[0], 2, *hw)
    check_vs_oracle(pred, gt, mask)


def test_edges_perfect_match_and_empty_mask(dev):
    from svs_hip import nvs
    _, gt, mask = random_views(5, 3, 40, 90)
    mask[1] = 0
    pred = gt.copy()
    pred[2, 10, 10, 1] ^= 1                                     # one code off, inside or outside the mask
    mask[2, 10, 10, 1] = 1
    psnr, ssim = nvs.score_views(pred, gt, mask)
    assert psnr[0] == np.inf and ssim[0] == pytest.approx(1.0, abs=1e-12)
    assert np.isnan(psnr[1]) and ssim[1] == pytest.approx(1.0, abs=1e-12)  # all-white composites
    assert np.isfinite(psnr[2]) and ssim[2] < 1
    want_p, want_s = no.score_views(pred, gt, mask)
    assert want_p[0] == np.inf and np.isnan(want_p[1])
    assert abs(psnr[2] - want_p[2]) <= PSNR_TOL and np.abs(ssim - want_s).max() <= SSIM_TOL
    # an empty mask with different images: SSIM still scores the all-white composite
    m0 = np.zeros_like(mask[:1])
    p1, s1 = nvs.score_views(np.zeros_like(gt[:1]), gt[:1], m0)
    assert np.isnan(p1[0]) and s1[0] == pytest.approx(1.0, abs=1e-12)


def test_bit_identical_repeats(dev):
    from svs_hip import lib
    from svs_hip.ops import _ptr, _stream
    L = lib.load()
    pred, gt, mask = (torch.from_numpy(a).to(dev) for a in random_views(7, 5, 300, 400))
    ws = torch.empty(int(L.svs_nvs_workspace_bytes(5, 300, 400)), dtype=torch.uint8, device=dev)
    outs = []
    for _ in range(2):
        out = torch.full((5, 3), -1.0, dtype=torch.float64, device=dev)
        assert L.svs_nvs_score(_ptr(pred), _ptr(gt), _ptr(mask), 5, 300, 400, _ptr(ws), _ptr(out), _stream()) == 0
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()


def test_rejected_calls_write_nothing(dev):
    from svs_hip import lib
    from svs_hip.ops import _ptr, _stream
    L = lib.load()
    V, H, W = 2, 16, 20
    pred, gt, mask = (torch.from_numpy(a).to(dev) for a in random_views(9, V, H, W))
    ws = torch.full((int(L.svs_nvs_workspace_bytes(V, H, W)),), 7, dtype=torch.uint8, device=dev)
    out = torch.full((V, 3), 7.0, dtype=torch.float64, device=dev)

    def call(v, h, w, **over):
        p = dict(pred=_ptr(pred), gt=_ptr(gt), mask=_ptr(mask), ws=_ptr(ws), out=_ptr(out))
        p.update(over)
        return L.svs_nvs_score(p["pred"], p["gt"], p["mask"], v, h, w, p["ws"], p["out"], _stream())

    for k in ("pred", "gt", "mask", "ws", "out"):
        assert call(V, H, W, **{k: None}) == SVS_EINVAL, k
        assert b"svs_nvs_score" in L.svs_last_error_string()
    for v in (0, -3):
        assert call(v, H, W) == SVS_EINVAL
    for h, w in ((6, W), (H, 6), (0, 0), (-7, W)):
        assert call(V, h, w) == SVS_ESHAPE, (h, w)
        assert b"svs_nvs_score" in L.svs_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 7).all())
    assert call(V, H, W) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


def test_score_scan_end_to_end(dev, golden, tree):
    """score_scan on the fixture tree (files -> load_gt -> kernel) gives the reference's per-view numbers."""
    from svs_hip import nvs
    for name, case in tree.items():
        for rf in (str(r) for r in golden["result_from"]):
            r = nvs.score_scan(case["rendering_dir"], case["data_dir_root"], case["dataset"], case["scan"], case["views"],
                               result_from=rf, img_res=case["img_res"])
            assert list(r["views"]) == case["views"]
            assert np.abs(r["psnr"] - golden[f"{name}/{rf}/psnr"]).max() <= PSNR_TOL, (name, rf)
            assert np.abs(r["ssim"] - golden[f"{name}/{rf}/ssim"]).max() <= SSIM_TOL, (name, rf)


def test_device_tensors_and_type_errors(dev):
    from svs_hip import nvs
    pred, gt, mask = random_views(13, 2, 20, 30)
    a = nvs.score_views(pred, gt, mask)
    b = nvs.score_views(*(torch.from_numpy(x).to(dev) for x in (pred, gt, mask)))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(TypeError):
        nvs.score_views(pred.astype(np.float32), gt, mask)
    with pytest.raises(ValueError):
        nvs.score_views(pred[:, :6], gt[:, :6], mask[:, :6])
