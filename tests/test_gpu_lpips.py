"""GPU checks of LPIPS (svs_hip.lpips, csrc/svs_lpips.hip) against the float64 oracle of tests/lpips_oracle.py.

Tolerances are measured, not chosen: every bound is a multiple of the error the float32 comparator (the same definition
through torch's float32 conv2d on the CPU) makes against float64 on the very inputs of the case, computed in the test.
  one layer   max |y - y64| / sum |w||x| over the outputs; the HIP path gets 4x the comparator's figure (the fp16x2 split
              drops the mid * mid term: 2^-22 per product against float32's 2^-24).
  the score   |d - d64| per view; the HIP path gets 8x the comparator's largest figure over the case's views (thirteen
              layers compound), and at 64x96 additionally |d_hip - d64| <= 5e-5 whatever the comparator does.
Figures measured for the cases below (seed-fixed, so they repeat): profiles/lpips_bench.txt holds the table.
  layers, comparator: 3.1e-08 (512 -> 512, inputs times 2^8) to 2.6e-07 (3 -> 64 at 33x40); bounds 1.2e-07 to 1.0e-06
  score, comparator: 16x16 |d32 - d64| = 1.2e-10, 5.1e-10 (bound 4.1e-09); 35x50 5.3e-11, 2.3e-10 (bound 1.8e-09);
         64x96 1.1e-10, 3.2e-11 on d64 = 3.28e-3, 1.60e-3 (bound 8.6e-10)
Every test prints its case's comparator figure, bound and HIP figure before it asserts (pytest -s).
HIP figures: with one accumulation chain per output the 256 -> 512 layer at 9x21 (ReLU on) gave 1.72e-07 against its
bound of 1.43e-07, while the 3 -> 64, 64 -> 64 and 64 -> 128 cases passed; the kernel now restarts the hi * hi chain every
32-channel slice (csrc/svs_lpips.hip).  The figures of that kernel are not recorded here yet: a run of this file with -s
prints them.
"""
import functools
import os

import numpy as np
import pytest
import torch

import lpips_oracle as lo

pytestmark = pytest.mark.gpu

LAYERS = [(3, 64), (64, 64), (64, 128), (256, 512), (512, 512)]
SIZES = [(9, 21), (33, 40)]            # tile remainders in x and y; 9x21 is smaller than two workgroup windows across


@functools.lru_cache(maxsize=None)
def layer_case(cin, cout, H, W, w_exp, x_exp):
    """seeded x, w, b and what float64 and the float32 comparator make of them (before the ReLU)"""
    rng = np.random.default_rng(1000 * cin + cout + H + 7 * w_exp + 11 * x_exp)
    w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin)) * 2.0 ** w_exp).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.05 * 2.0 ** (w_exp + x_exp)).astype(np.float32)
    x = (rng.standard_normal((cin, H, W)) * 2.0 ** x_exp).astype(np.float32)
    y64, mag = lo.conv64(x, w, b, False)
    y32 = lo.Float32Comparator(None).conv(x, w, b, False)
    return x, w, b, y64, y32, mag


def check_layer(cin, cout, H, W, relu, w_exp=0, x_exp=0):
    from svs_hip import lpips
    x, w, b, y64, y32, mag = layer_case(cin, cout, H, W, w_exp, x_exp)
    if relu:
        y64, y32 = np.maximum(y64, 0.0), np.maximum(y32, 0.0)
    got = lpips.conv3x3(x, torch.from_numpy(w), b, relu=relu).cpu().numpy()
    assert got.shape == y64.shape and np.isfinite(got).all()
    e32 = float((np.abs(y32 - y64) / mag).max())
    e = float((np.abs(got - y64) / mag).max())
    print(f"layer {cin}->{cout} {H}x{W} relu={relu} w*2^{w_exp} x*2^{x_exp}: comparator {e32:.3e} bound {4 * e32:.3e} hip {e:.3e}")
    assert e <= 4 * e32


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("cin,cout", LAYERS)
def test_one_layer(cin, cout, H, W, relu):
    check_layer(cin, cout, H, W, relu)


@pytest.mark.parametrize("w_exp,x_exp", [(-10, 0), (0, 8)])
@pytest.mark.parametrize("cin,cout", LAYERS)
def test_one_layer_operand_ranges(cin, cout, w_exp, x_exp):
    """weights times 2^-10 (their unscaled mid pieces would be fp16 subnormals), inputs times 2^8"""
    check_layer(cin, cout, 33, 40, True, w_exp, x_exp)


def test_overflowing_input_is_a_code():
    from svs_hip import lib, lpips
    x, w, b, *_ = layer_case(64, 64, 9, 21, 0, 0)
    x = x.copy()
    x[5, 3, 7] = 1e6
    with pytest.raises(lib.SvsError, match=r"code -4"):
        lpips.conv3x3(x, torch.from_numpy(w), b)
    # and the next call is clean again
    assert np.isfinite(lpips.conv3x3(layer_case(64, 64, 9, 21, 0, 0)[0], torch.from_numpy(w), b).cpu().numpy()).all()


@pytest.mark.parametrize("H,W", [(9, 21), (16, 16)])
def test_pool(H, W):
    from svs_hip import lpips
    x = torch.from_numpy(np.random.default_rng(H).standard_normal((70, H, W)).astype(np.float32))
    got = lpips.maxpool2(x).cpu()
    assert torch.equal(got, torch.nn.functional.max_pool2d(x[None], 2, 2)[0])


@pytest.mark.parametrize("C", [64, 512])
def test_head(C):
    """5x7 pixels; one of them without any feature in both images, one without in one image: the 1e-10 keeps both finite"""
    from svs_hip import lpips
    rng = np.random.default_rng(C)
    f0 = np.maximum(rng.standard_normal((C, 5, 7)), 0).astype(np.float32)
    f1 = np.maximum(f0 + 0.3 * rng.standard_normal((C, 5, 7)), 0).astype(np.float32)
    f0[:, 2, 3] = 0
    f1[:, 2, 3] = 0
    f1[:, 4, 6] = 0
    w = rng.random(C)
    w = (w / w.sum()).astype(np.float32)
    want = float(lo.head(torch.from_numpy(f0).double(), torch.from_numpy(f1).double(), torch.from_numpy(w).double()))
    got = lpips.head(f0, f1, w)
    print(f"head C={C}: oracle {want:.17g} hip {got:.17g}")
    assert np.isfinite(got) and abs(got - want) <= 1e-13 * abs(want)          # float64 both: only the order of the sums differs


@pytest.fixture(scope="module")
def weights():
    return lo.make_weights(0)


@pytest.fixture(scope="module")
def net(weights):
    from svs_hip import lpips
    return lpips.LpipsNet(weights)


@functools.lru_cache(maxsize=None)
def score_case(H, W):
    weights = lo.make_weights(0)
    pred, gt, mask = lo.make_views(3, 2, H, W)
    return pred, gt, mask, lo.lpips(pred, gt, mask, weights), lo.Float32Comparator(weights)(pred, gt, mask)


@pytest.mark.parametrize("H,W", [(16, 16), (35, 50), (64, 96)])
def test_end_to_end(net, H, W):
    pred, gt, mask, d64, d32 = score_case(H, W)
    assert (mask[..., 0] != mask[..., 1]).any()
    got = net.score_views(pred, gt, mask)
    again = net.score_views(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(mask).cuda())
    e32, e = np.abs(d32 - d64), np.abs(got - d64)
    print(f"score {H}x{W}: d64 {d64} comparator |d32-d64| {e32} bound {8 * e32.max():.3e} hip |d-d64| {e}")
    assert got.dtype == np.float64 and got.shape == (2,)
    assert np.array_equal(got, again)                              # bit-identical run to run
    if (H, W) == (64, 96):
        assert e.max() <= 5e-5
    assert e.max() <= 8 * e32.max()


def test_printed_value(net, golden_dir, tmp_path):
    """score_scan on a folder of PNGs: the fourth line is formatted from the values score_views returns"""
    import nvs_oracle as no
    from svs_hip import nvs
    case = no.fixture_tree(dict(np.load(os.path.join(golden_dir, "nvs_scores.npz"))), tmp_path)["dtu24"]
    views = case["views"][:3]
    args = (case["rendering_dir"], case["data_dir_root"], case["dataset"], case["scan"], views)
    plain = nvs.score_scan(*args, img_res=case["img_res"])
    r = nvs.score_scan(*args, img_res=case["img_res"], lpips=net)
    assert "lpips" not in plain and np.array_equal(plain["psnr"], r["psnr"]) and np.array_equal(plain["ssim"], r["ssim"])
    preds = np.stack([no.read_png(nvs.prediction_path(case["rendering_dir"], v)) for v in views])
    gt, m = nvs.load_gt(case["data_dir_root"], case["dataset"], case["scan"], views, img_res=case["img_res"])
    want = lo.lpips(preds, gt, m, lo.make_weights(0))
    assert r["lpips"].shape == (3,) and np.abs(r["lpips"] - want).max() <= 5e-5
    lines = nvs.scan_lines(case["scan"], r["psnr"], r["ssim"], r["lpips"])
    assert lines[:3] == nvs.scan_lines(case["scan"], plain["psnr"], plain["ssim"]) and len(lines) == 4
    assert lines[3] == "    lpips mean = {0}, std {1}".format("%.4f" % r["lpips"].mean(), "%.4f" % r["lpips"].std())
