"""CPU checks of LPIPS (svs_hip.lpips, csrc/svs_lpips.hip): the float64 oracle on closed forms, the weight reader on the
three key styles, the printed block with and without the fourth line, and the argument checks of the new entry points,
which answer with codes before anything is launched -- no GPU work here.

The float32 comparator at the end-to-end test's largest case (V = 2 at 64x96, weights make_weights(0), views
make_views(3, 2, 64, 96)): d64 = 3.28e-3 and 1.60e-3, |d32 - d64| = 1.1e-10 and 3.2e-11, far inside the 5e-5 that half a unit of the fourth
printed decimal allows."""
import numpy as np
import pytest
import torch

import lpips_oracle as lo


@pytest.fixture(scope="module")
def weights():
    return lo.make_weights(0)


def test_identical_images_score_exactly_zero(weights):
    pred, gt, mask = lo.make_views(5, 1, 16, 24)
    assert lo.lpips(gt, gt, mask, weights)[0] == 0.0
    # outside the mask both are white: a prediction that differs only there scores 0 too
    pred2 = np.where(mask != 0, gt, pred)
    assert lo.lpips(pred2, gt, mask, weights)[0] == 0.0


def test_head_two_taps_by_hand():
    """Tap A (2 channels, 2x2): one pixel holds f0 = (3,4), f1 = (4,3): unit vectors (0.6,0.8), (0.8,0.6), squared
    differences (0.04,0.04), weights (0.25,0.75): d = 0.04; the other three pixels agree: mean 0.01.  Tap B: f0 = (1,0) and
    f1 = (0,1) everywhere, weights (0.5,0.5): d = 1.  Sum 1.01 (the 1e-10 moves it by less than 1e-10)."""
    f0 = torch.ones(2, 2, 2, dtype=torch.float64)
    f1 = torch.ones(2, 2, 2, dtype=torch.float64)
    f0[:, 0, 1] = torch.tensor([3.0, 4.0], dtype=torch.float64)
    f1[:, 0, 1] = torch.tensor([4.0, 3.0], dtype=torch.float64)
    a = lo.head(f0, f1, torch.tensor([0.25, 0.75], dtype=torch.float64))
    g0 = torch.zeros(2, 2, 2, dtype=torch.float64)
    g1 = torch.zeros(2, 2, 2, dtype=torch.float64)
    g0[0], g1[1] = 1.0, 1.0
    b = lo.head(g0, g1, torch.tensor([0.5, 0.5], dtype=torch.float64))
    assert abs(float(a) - 0.01) < 1e-10 and abs(float(b) - 1.0) < 1e-9
    assert abs(float(a + b) - 1.01) < 1e-9
    # a pixel without features: finite, and 0
    z = torch.zeros(2, 2, 2, dtype=torch.float64)
    assert float(lo.head(z, z, torch.tensor([0.5, 0.5], dtype=torch.float64))) == 0.0


def test_pooling_is_floor_mode(weights):
    x = torch.zeros(1, 3, 35, 50, dtype=torch.float64)
    shapes = [tuple(t.shape[1:]) for t in lo.features(x, weights, torch.float64)]
    assert shapes == [(64, 35, 50), (128, 17, 25), (256, 8, 12), (512, 4, 6), (512, 2, 3)]
    # the odd last row and column are dropped, not padded
    a = torch.arange(35 * 50, dtype=torch.float64).view(1, 1, 35, 50)
    p = torch.nn.functional.max_pool2d(a, 2, 2)
    assert tuple(p.shape) == (1, 1, 17, 25) and float(p.max()) == 33 * 50 + 49


def _save(sd, path):
    if str(path).endswith(".npz"):
        np.savez(path, **sd)
    else:
        torch.save({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, path)


@pytest.mark.parametrize("style,ext", [("torchvision", ".pth"), ("lpips", ".pth"), ("lins", ".npz")])
def test_load_weights_key_styles(weights, tmp_path, style, ext):
    from svs_hip import lpips
    sd = lo.state_dict(weights, style)
    conv = {k: v for k, v in sd.items() if ".model.1." not in k}
    lin = {k: v for k, v in sd.items() if ".model.1." in k}
    vgg, linf, both = tmp_path / ("vgg" + ext), tmp_path / ("lin" + ext), tmp_path / ("both" + ext)
    _save(conv, vgg); _save(lin, linf); _save(sd, both)
    for got in (lpips.load_weights(vgg, linf), lpips.load_weights(both)):
        assert len(got["conv"]) == 13 and len(got["lin"]) == 5
        for (w, b), (w0, b0) in zip(got["conv"], weights["conv"]):
            assert w.dtype == np.float32 and np.array_equal(w, w0) and np.array_equal(b, b0)
        for w, w0 in zip(got["lin"], weights["lin"]):
            assert w.shape == w0.shape and np.array_equal(w, w0)


def test_load_weights_names_what_is_wrong(weights, tmp_path):
    from svs_hip import lpips
    sd = lo.state_dict(weights)
    missing = {k: v for k, v in sd.items() if k != "features.17.bias"}
    _save(missing, tmp_path / "a.npz")
    with pytest.raises(KeyError, match=r"features\.17 .*bias"):
        lpips.load_weights(tmp_path / "a.npz")
    conv_only = {k: v for k, v in sd.items() if ".model.1." not in k}
    _save(conv_only, tmp_path / "b.pth")
    with pytest.raises(KeyError, match=r"lin layer 0"):
        lpips.load_weights(tmp_path / "b.pth")
    bad = dict(sd)
    bad["features.5.weight"] = bad["features.5.weight"][:, :32]
    _save(bad, tmp_path / "c.npz")
    with pytest.raises(ValueError, match=r"features\.5\.weight has shape \(128, 32, 3, 3\)"):
        lpips.load_weights(tmp_path / "c.npz")


def test_scan_lines_three_or_four():
    from svs_hip import nvs
    psnr, ssim, lp = [20.0, 22.0], [0.5, 0.7], [0.1234, 0.2346]
    three = ["SCAN 106:", "    psnr mean = 21.0000, std 1.0000", "    ssim mean = 0.6000, std 0.1000"]
    assert nvs.scan_lines(106, psnr, ssim) == three
    assert nvs.scan_lines(106, psnr, ssim, None) == three
    assert nvs.scan_lines(106, psnr, ssim, lp) == three + ["    lpips mean = 0.1790, std 0.0556"]
    # the reference's format (eval_vsdf.py:277)
    want = "    lpips mean = {0}, std {1}".format("%.4f" % np.mean(lp), "%.4f" % np.std(lp))
    assert nvs.scan_lines(106, psnr, ssim, lp)[3] == want


def test_clis_take_the_weight_files():
    import argparse
    from svs_hip import evalviews, nvs
    p = argparse.ArgumentParser()
    nvs.add_lpips_arguments(p)
    a = p.parse_args([])
    assert a.lpips_vgg is None and a.lpips_lin is None and nvs.lpips_from_arguments(a) is None
    a = evalviews.parse_args(["--ckpt", "c", "--data-dir-root", "d", "--dataset", "DTU", "--scan", "1", "--score",
                              "--lpips-vgg", "v.pth", "--lpips-lin", "l.pth"])
    assert (a.lpips_vgg, a.lpips_lin) == ("v.pth", "l.pth")
    with pytest.raises(SystemExit):
        nvs.lpips_from_arguments(p.parse_args(["--lpips-lin", "l.pth"]))


def test_argument_errors_are_codes_before_any_launch():
    """NULL pointers, H < 16, an unsupported (Cin, Cout): negative codes and a message, on a machine without a GPU."""
    from svs_hip import lib
    L = lib.load()
    EINVAL, ESHAPE = -1, -2
    p = 4096                                                       # never dereferenced: the checks come first
    assert L.svs_conv3x3_mfma_supported(3, 64) == 1 and L.svs_conv3x3_mfma_supported(512, 512) == 1
    assert L.svs_conv3x3_mfma_supported(32, 64) == 0 and L.svs_conv3x3_mfma_supported(64, 32) == 0
    assert L.svs_conv3x3_mfma_wfrag_bytes(32, 64) == 0
    # fragments: Cout/64 blocks x Cin/32 slices x 9 k-steps x 4 M tiles x 2 pieces x 1 KiB, + Cout inverse scales
    assert L.svs_conv3x3_mfma_wfrag_bytes(64, 128) == 2 * 2 * 9 * 4 * 2 * 1024 + 128 * 4
    assert L.svs_conv3x3_mfma_wfrag_bytes(3, 64) == 3 * 4 * 2 * 1024 + 64 * 4
    assert L.svs_conv3x3_mfma_pack(None, 64, 64, p, None) == EINVAL
    assert L.svs_conv3x3_mfma_pack(p, 64, 48, p, None) == ESHAPE
    assert L.svs_conv3x3_mfma(None, p, None, p, 64, 64, 8, 8, 1, None) == EINVAL
    assert L.svs_conv3x3_mfma(p, p, None, p, 32, 64, 8, 8, 1, None) == ESHAPE
    assert b"unsupported" in L.svs_last_error_string()
    assert L.svs_conv3x3_mfma(p, p, None, p, 64, 64, 0, 8, 1, None) == ESHAPE
    assert L.svs_maxpool2(None, p, 4, 8, 8, None) == EINVAL
    assert L.svs_maxpool2(p, p, 4, 1, 8, None) == ESHAPE
    assert L.svs_lpips_head(p, None, p, 64, 2, 2, p, None) == EINVAL
    assert L.svs_lpips_head(p, p, p, 96, 2, 2, p, None) == ESHAPE
    assert L.svs_lpips_workspace_bytes(1, 15, 64) == 0 and L.svs_lpips_workspace_bytes(0, 64, 64) == 0
    assert L.svs_lpips_workspace_bytes(1, 16, 16) > 2 * 2 * 64 * 16 * 16 * 4
    assert L.svs_lpips_score(p, p, p, 1, 64, 64, p, None, p, None) == EINVAL
    assert L.svs_lpips_score(p, p, p, 0, 64, 64, p, p, p, None) == EINVAL
    assert L.svs_lpips_score(p, p, p, 1, 15, 64, p, p, p, None) == ESHAPE
    assert b">= 16" in L.svs_last_error_string()
    assert L.svs_lpips_net_offset(0, 13) == 2 ** 64 - 1 and L.svs_lpips_net_offset(0, 0) == 0
    assert L.svs_lpips_net_offset(2, 4) + 512 * 4 <= L.svs_lpips_net_bytes()
    assert L.svs_version() == 101


def test_float32_comparator_inside_the_printed_decimal(weights):
    """The independent condition of the end-to-end test, for the comparator: |d32 - d64| <= 5e-5 at 64x96."""
    pred, gt, mask = lo.make_views(3, 2, 64, 96)
    d64 = lo.lpips(pred, gt, mask, weights)
    d32 = lo.Float32Comparator(weights)(pred, gt, mask)
    print("d64", d64, "|d32 - d64|", np.abs(d32 - d64))
    assert (d64 > 1e-3).all() and np.abs(d32 - d64).max() <= 5e-5
