"""GPU parity of UCSNet (s-volsdf_amd/models/ucsnet.py on csrc/svs_ucsnet.hip and the tail of csrc/svs_costvol.hip): the
transposed convolutions against float64, the feature extractor and the three stages against what the reference wrote into
tests/golden/ucsnet_3stage.npz, the per-pixel uncertainty against float64 and against the old tail, the uncertainty-aware
hypotheses against the restatement of tests/ucsnet_oracle.py.  The CPU-side checks of that restatement and of the fixture
(near-tie cap included) are tests/test_ucsnet_cpu.py."""
import os

import numpy as np
import pytest
import torch

import costvol_tail_cases as cases
import costvol_tail_ref as tref
import ucsnet_oracle as uo

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
TIE_CAP = 0.002            # tests/test_gpu_costvol_tail.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ucsnet_3stage.npz")))


def G(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _model(dev, g):
    from models.ucsnet import UCSNetHip as UCSNet          # the mirror, whether or not a checkout is on the path
    m = UCSNet(lamb=float(g["lamb"]), stage_configs=[int(x) for x in g["ndepths"]], grad_method="detach", base_chs=[8, 8, 8],
               feat_ext_ch=8)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in uo.ucsnet_state_dict(int(g["seed"])).items()}, strict=True)
    return m.to(dev).eval()


# ---------------------------------------------------------------------------------------------------------------------
# transposed convolution
# ---------------------------------------------------------------------------------------------------------------------
def _deconv64(x, w, b, relu):
    ref = torch.nn.functional.conv_transpose2d(torch.from_numpy(x).double()[None], torch.from_numpy(w).double(),
                                               None if b is None else torch.from_numpy(b).double(), stride=2, padding=1,
                                               output_padding=1)[0]
    return (ref.clamp(min=0) if relu else ref).numpy()


@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (8, 16), (17, 33), (20, 130)])
@pytest.mark.parametrize("Cin,Cout", [(32, 16), (16, 8)])
def test_deconv2d_vs_float64(dev, Cin, Cout, hw):
    """svs_deconv2d_mfma and svs_deconv2d against a float64 conv_transpose2d: one pixel (every class is border), odd sizes (the
    +1 row and column of output_padding), a width that is no multiple of the 32-wide window, several windows per row; with and
    without bias and ReLU; 3e-6 of the output scale, the bound of test_conv2d_mfma_single_layer for the same operand scheme.
    Then into the first half of a buffer whose other half is NaN and stays NaN."""
    from svs_hip import costvol
    H, W = hw
    rs = np.random.default_rng(1000 * Cin + 10 * H + W)
    x = rs.standard_normal((Cin, H, W)).astype(F32)
    w = (rs.standard_normal((Cin, Cout, 3, 3)) / np.sqrt(Cin * 9 / 4)).astype(F32)
    b = rs.standard_normal(Cout).astype(F32)
    assert costvol.deconv2d_mfma_supported(Cin, Cout)
    for bias, relu in ((b, True), (b, False), (None, False), (None, True)):
        ref = _deconv64(x, w, bias, relu)
        np.testing.assert_allclose(ref, np.maximum(uo.deconv2d_taps(x, w, bias), 0) if relu else uo.deconv2d_taps(x, w, bias), atol=1e-12)
        for mfma in (True, False):
            got = costvol.deconv2d(G(x, dev), G(w, dev), None if bias is None else G(bias, dev), relu=relu, mfma=mfma).cpu().numpy()
            assert got.shape == ref.shape == (Cout, 2 * H, 2 * W)
            err = np.abs(got - ref).max() / np.abs(ref).max()
            print(f"deconv2d {Cin}->{Cout} {hw} mfma={mfma} bias={bias is not None} relu={relu}: {err:.2e} of the output scale")
            np.testing.assert_allclose(got, ref, atol=3e-6 * np.abs(ref).max())
    ref = _deconv64(x, w, b, True)
    for mfma in (True, False):
        buf = torch.full((2 * Cout, 2 * H, 2 * W), float("nan"), device=dev)
        out = costvol.deconv2d(G(x, dev), G(w, dev), G(b, dev), relu=True, out=buf, mfma=mfma)
        assert out is buf
        np.testing.assert_allclose(buf[:Cout].cpu().numpy(), ref, atol=3e-6 * np.abs(ref).max())
        assert torch.isnan(buf[Cout:]).all()


@pytest.mark.parametrize("Cin,Cout", [(32, 16), (16, 8)])
def test_deconv2d_small_weights_large_activations(dev, Cin, Cout):
    """Weights of about 1e-2 (BatchNorm-folded size: their fp16 mid piece is subnormal, 3e-8 absolute) against activations of
    about 1e3: the unscaled split's weak spot (include/svolsdf_hip.h states the range).  Same bound, 3e-6 of the output scale."""
    from svs_hip import costvol
    rs = np.random.default_rng(Cin)
    x = (1e3 * rs.standard_normal((Cin, 17, 33))).astype(F32)
    w = (1e-2 * rs.standard_normal((Cin, Cout, 3, 3))).astype(F32)
    ref = _deconv64(x, w, None, False)
    for mfma in (True, False):
        got = costvol.deconv2d(G(x, dev), G(w, dev), None, mfma=mfma).cpu().numpy()
        print(f"deconv2d {Cin}->{Cout} weights 1e-2, activations 1e3, mfma={mfma}: {np.abs(got - ref).max() / np.abs(ref).max():.2e}")
        np.testing.assert_allclose(got, ref, atol=3e-6 * np.abs(ref).max())


def test_deconv2d_arguments(dev):
    from svs_hip import costvol, lib
    assert not costvol.deconv2d_mfma_supported(8, 8) and not costvol.deconv2d_mfma_supported(32, 17)
    x, w = torch.zeros(8, 4, 4, device=dev), torch.zeros(8, 5, 3, 3, device=dev)
    with pytest.raises(ValueError):
        costvol.deconv2d(x, w, mfma=True)
    assert costvol.deconv2d(x, w).shape == (5, 8, 8)                  # any shape on the float32 kernel
    with pytest.raises(ValueError):
        costvol.deconv2d(x, w, out=torch.zeros(5, 8, 9, device=dev))
    L = lib.load()
    assert L.svs_deconv2d(x.data_ptr(), w.data_ptr(), None, torch.zeros(5, 8, 8, device=dev).data_ptr(), 63, 8, 5, 4, 4, 0, None) != 0


# ---------------------------------------------------------------------------------------------------------------------
# feature extractor
# ---------------------------------------------------------------------------------------------------------------------
def test_feature_extractor_golden_and_in_place_concatenation(dev, g):
    """FeatExtNet from one call against the reference's three maps (1e-5, the bound test_feature_net_hip holds the FPN to), and
    bit for bit against the same layers launched one by one with a real torch.cat -- which proves the concatenation that
    svs_featurenet_unet forms in place; the transposed layers' raw outputs against the reference's on both paths."""
    from svs_hip import costvol
    m = _model(dev, g)
    fe = m.feature_extraction
    img = G(uo.fixture_image(int(g["seed"])), dev)
    with torch.no_grad():
        out = fe(torch.stack([img, img.flip(-1)]))
    for k in ("stage1", "stage2", "stage3"):
        got, want = uo.pinned(g, "feat_" + k, out[k][0].cpu().numpy())
        np.testing.assert_allclose(got, want, atol=1e-5, err_msg=k)
    layers = fe.layers()
    frags = fe._unet.tables(layers)[6]
    # (the defaults: deconv1.deconv on the matrix cores, deconv2.deconv on the float32 kernel -- FeatureNetUnet.tables)
    assert frags[9] is not None and frags[12] is None and frags[10] is not None and frags[13] is not None and frags[0] is None

    def conv(i, x, stride=1, relu=True):
        w, b = layers[i]
        return (costvol.conv2d_mfma if frags[i] is not None else costvol.conv2d)(x, w, b, stride=stride, relu=relu)

    def deconv(i, x):
        w, b = layers[i]
        return costvol.deconv2d(x, w, b, relu=True, mfma=frags[i] is not None)

    d1_of, c0_of = {}, {}
    for image, key in ((img, 0), (img.flip(-1).contiguous(), 1)):
        c0 = conv(1, conv(0, image))
        c1 = conv(4, conv(3, conv(2, c0, stride=2)))
        c2 = conv(7, conv(6, conv(5, c1, stride=2)))
        s1 = conv(8, c2, relu=False)
        d1 = conv(10, torch.cat((deconv(9, c2), c1), 0))
        s2 = conv(11, d1, relu=False)
        d1_of[key], c0_of[key] = d1, c0
        d2 = conv(13, torch.cat((deconv(12, d1), c0), 0))
        s3 = conv(14, d2, relu=False)
        for k, t in (("stage1", s1), ("stage2", s2), ("stage3", s3)):
            assert torch.equal(out[k][key], t), k
        if key == 0:
            for name, x, wkey in (("deconv1_raw", c2, "deconv1"), ("deconv2_raw", d1, "deconv2")):
                wraw = fe.state_dict()[f"{wkey}.deconv.conv.weight"]
                for mfma in (True, False):
                    got, want = uo.pinned(g, "feat_" + name, costvol.deconv2d(x, wraw, None, mfma=mfma).cpu().numpy())
                    np.testing.assert_allclose(got, want, atol=1e-5, err_msg=name)
    both = costvol.FeatureNetUnet(8, deconv_mfma=True)                  # both transposed layers on the matrix cores
    assert all(f is not None for f in (both.tables(layers)[6][9], both.tables(layers)[6][12]))
    s3 = both(img, layers)[2]
    d2 = conv(13, torch.cat((costvol.deconv2d(d1_of[0], *layers[12], relu=True, mfma=True), c0_of[0]), 0))
    assert torch.equal(s3, conv(14, d2, relu=False))
    with pytest.raises(Exception):
        fe(torch.zeros(1, 3, 30, 40, device=dev))                      # H, W multiples of 4
    costvol.clear_caches()
    assert fe._unet._tables.value is None and fe._unet._ws is None
    with torch.no_grad():
        assert torch.equal(fe(img[None])["stage3"][0], out["stage3"][0])


# ---------------------------------------------------------------------------------------------------------------------
# tail with the per-pixel uncertainty
# ---------------------------------------------------------------------------------------------------------------------
VAR_HW = ((7, 9), (37, 53))
LAMB = 1.5


def _var_err(v, v64, dv):
    """error of a variance map relative to the variance plus the floor a rounded depth leaves of a zero variance"""
    return np.abs(np.asarray(v, F64) - v64) / (v64 + uo.variance_floor(dv, LAMB))


@pytest.fixture(scope="module")
def var_bound():
    """4 x the largest error of the float32 numpy restatement (ucsnet_oracle.variance32) against float64 over the cases of
    test_tail_var: the kernel sums up to 257 terms in another order (interleaved slices, then across slices).
    Measured: the restatement's largest error is 9.17e-7, so the kernel is allowed 3.67e-6; its own largest is 1.04e-6
    (D = 15 at 37 x 53), 2e-7 to 4e-7 at most sizes."""
    worst = 0.0
    for D in cases.TAIL_D:
        for (H, W) in VAR_HW:
            reg, dv = cases.tail_case(D, H, W, 0)[:2]
            worst = max(worst, _var_err(uo.variance32(reg, dv, LAMB), uo.variance64(reg, dv, LAMB), dv).max())
    print(f"variance32 against float64 over TAIL_D x {VAR_HW}: {worst:.3e}; the kernel is allowed {4 * worst:.3e}")
    return 4.0 * worst


@pytest.mark.parametrize("D", cases.TAIL_D)
def test_tail_var(dev, D, var_bound):
    """svs_prob_depth_conf_var over every D at which the tail changes its path (register-cached up to 192, looped beyond; the
    three block shapes) x two image sizes: prob, depth, conf and index bit-equal to svs_prob_depth_conf on the same input;
    variance against float64 within 4 x the float32 numpy restatement's own error (measured by `var_bound` on the same cases:
    see its printed figure; relative to variance + the floor of ucsnet_oracle.variance_floor)."""
    from svs_hip import costvol
    for (H, W) in VAR_HW:
        reg, dv = cases.tail_case(D, H, W, 0)[:2]
        old = costvol.prob_depth_conf(G(reg, dev), G(dv, dev))
        new = costvol.prob_depth_conf_var(G(reg, dev), G(dv, dev), LAMB)
        for a, b, name in zip(old, new[:4], ("prob", "depth", "conf", "index")):
            assert torch.equal(a, b), (name, D, H, W)
        var = new[4].cpu().numpy()
        v64 = uo.variance64(reg, dv, LAMB)
        err = _var_err(var, v64, dv).max()
        print(f"variance D={D} {H}x{W}: {err:.3e} (bound {var_bound:.3e})")
        assert np.isfinite(var).all() and (var >= 0).all()
        assert err <= var_bound, (D, H, W, err)


@pytest.mark.parametrize("D", (2, 8, 64, 192, 257))
def test_tail_var_closed_forms(dev, D, var_bound):
    """Flat logits: the probability is 1/D and the variance lamb * std(z) of the pixel's hypotheses (population form).  One-hot
    logits (one plane 800 above the rest: every other exponential is 0 in float32 and in float64): the depth is that plane's
    hypothesis and the variance 0 up to the depth's rounding (ucsnet_oracle.variance_floor)."""
    from svs_hip import costvol
    H, W = 5, 13
    rs = np.random.default_rng(D)
    dv = np.sort(rs.uniform(425, 935, (D, H, W)), 0).astype(F32)
    flat = np.broadcast_to(rs.normal(0, 5, (1, H, W)), (D, H, W)).astype(F32).copy()
    var = costvol.prob_depth_conf_var(G(flat, dev), G(dv, dev), LAMB)[4].cpu().numpy()
    want = LAMB * dv.astype(F64).std(0)
    np.testing.assert_allclose(uo.variance64(flat, dv, LAMB), want, rtol=1e-12)
    assert _var_err(var, want, dv).max() <= var_bound
    hot = rs.normal(0, 1, (D, H, W)).astype(F32)
    k = rs.integers(0, D, (H, W))
    np.put_along_axis(hot, k[None], 800.0, 0)
    _, depth, _, idx, var = costvol.prob_depth_conf_var(G(hot, dev), G(dv, dev), LAMB)
    assert np.array_equal(depth.cpu().numpy(), np.take_along_axis(dv, k[None], 0)[0])
    assert np.array_equal(idx.cpu().numpy(), k)
    assert (var.cpu().numpy() <= uo.variance_floor(dv, LAMB)).all()


# ---------------------------------------------------------------------------------------------------------------------
# hypotheses
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (2, 8, 192))
def test_stage1_planes_bit_equal(dev, D):
    """Stage 1 (models/ucsnet.py:47-57, restated with torch float32 on the CPU by ucsnet_oracle.stage1_planes): the planes of
    svs_depth_hypotheses(prev = NULL), which the mirror calls, are the reference's bit for bit -- linear and inverse."""
    from svs_hip import costvol
    for dmin, dmax in ((425.0, 935.0), (0.5, 6.0)):
        for inverse in (False, True):
            got = costvol.uncertainty_hypotheses(None, None, (6, 10), D, dmin, dmax, inverse, dev).cpu().numpy()
            want = uo.stage1_planes(dmin, dmax, D, inverse)
            assert got.shape == (D, 6, 10)
            assert np.array_equal(got, np.broadcast_to(want.reshape(-1, 1, 1), got.shape)), (D, dmin, inverse)


def _hypo_inputs(hp, wp, seed):
    """previous depth 500 .. 800 with an uncertainty of 2 .. 30 % of it; rows 0-2: depth 1, uncertainty 3 (var >= cur: the
    samples start at 0); the last three columns: uncertainty 0 (all samples equal)"""
    cur = cases.prev_depth_field((hp, wp), seed)
    rs = np.random.default_rng([seed, hp])
    var = (cur * rs.uniform(0.02, 0.3, (hp, wp))).astype(F32)
    cur[:3], var[:3] = 1.0, 3.0
    var[3:, -3:] = 0.0
    return cur, var


@pytest.mark.parametrize("D", (2, 8, 32))
@pytest.mark.parametrize("prev,hw", [((16, 24), (32, 48)), ((32, 48), (64, 96)), ((64, 96), (64, 96)), ((10, 13), (20, 26))])
def test_uncertainty_hypotheses(dev, prev, hw, D):
    """svs_uncertainty_hypotheses against the float32 restatement bit for bit and against float64 to 5e-6 (the bound
    test_three_stage_forward_golden holds hypotheses to)."""
    from svs_hip import costvol
    cur, var = _hypo_inputs(prev[0], prev[1], D)
    got = costvol.uncertainty_hypotheses(G(cur, dev), G(var, dev), hw, D).cpu().numpy()
    want32 = uo.uncertainty_samples32(cur, var, hw, D)
    assert got.shape == want32.shape == (D,) + hw
    assert np.array_equal(got, want32), f"{int((got != want32).sum())} of {got.size} differ, max {np.abs(got - want32).max()}"
    np.testing.assert_allclose(got, uo.uncertainty_samples64(cur, var, hw, D), rtol=5e-6)
    sy, sx = hw[0] // prev[0], hw[1] // prev[1]
    assert (got[0, :2 * sy] == F32(1e-12)).all()                         # var >= cur: the first sample is exactly eps
    np.testing.assert_allclose(got[-1, :2 * sy], 4.0, rtol=2e-7)
    tail = got[:, 4 * sy:, hw[1] - 2 * sx:]
    assert (tail == tail[0]).all() and (tail[0] > 400).all()             # var = 0: all D samples equal


def test_uncertainty_hypotheses_arguments(dev):
    from svs_hip import costvol, lib
    L = lib.load()
    cur, var = torch.ones(4, 6, device=dev), torch.ones(4, 6, device=dev)
    out = torch.full((8, 8, 12), float("nan"), device=dev)
    args = lambda d, v, D: (d.data_ptr(), d.shape[0], d.shape[1], v.data_ptr(), v.shape[0], v.shape[1], 8, 12, D, out.data_ptr(), None)
    assert L.svs_uncertainty_hypotheses(*args(cur, var, 1)) != 0
    assert L.svs_uncertainty_hypotheses(*args(cur, torch.ones(4, 5, device=dev), 8)) != 0
    assert L.svs_uncertainty_hypotheses(*args(cur, torch.ones(6, 4, device=dev), 8)) != 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                       # nothing was launched
    with pytest.raises(lib.SvsError):
        costvol.uncertainty_hypotheses(cur, var, (8, 12), 1)
    assert L.svs_uncertainty_hypotheses(*args(cur, var, 8)) == 0 and not torch.isnan(out).any()


# ---------------------------------------------------------------------------------------------------------------------
# three stages
# ---------------------------------------------------------------------------------------------------------------------
def _sample(dev, seed):
    feats, proj, depth_values = uo.fixture_sample(seed)
    H, W = uo.FIXTURE_HW
    sample = dict(imgs=torch.zeros(1, 3, 3, H, W, device=dev), depth_values=G(depth_values, dev)[None],
                  proj_matrices={k: G(v, dev)[None] for k, v in proj.items()})
    return sample, [{k: G(v, dev)[None] for k, v in f.items()} for f in feats]


def test_three_stage_forward_golden(dev, g):
    """UCSNet.forward x 3 stages through the reference's call surface with the structure and tolerances of
    tests/test_gpu_costvol.py::test_three_stage_forward_golden.  Every stage starts from the reference's previous depth (stage
    1's overridden as in runner.py:240-243) and uncertainty, so that its hypotheses can be held to 5e-6: fed with its own
    previous uncertainty, a stage's samples would carry that map's distance from the reference's, which is bounded by the
    regulariser's 2e-3 and not by 5e-6.  The chain on its own outputs is test_stage_loop_with_the_mirror.
    variance: logits within eps = 2e-3 move every probability by at most exp(2 eps) - 1, hence sum p (z - depth)^2 by that
    share and its root by half of it (the depth's own change enters to second order); the hypotheses' 5e-6 moves z - depth by
    at most 1e-5 of the largest hypothesis.  The tight check of the variance is the tail on the fixture's own logits, at every
    stage.  Sampled cost-volume voxels: 2e-4 as in that test, although the features here are three times as large
    (measured: 1.7e-5, 3.8e-5, 4.2e-5 at stages 1 to 3, values up to 9)."""
    from svs_hip import costvol, ops
    m = _model(dev, g)
    lamb = float(g["lamb"])
    sample, features = _sample(dev, int(g["seed"]))
    outputs, extra = None, None
    stage_out = []
    for st in range(3):
        cr = m.cost_regularization[st]
        cap = {}
        orig = cr.forward
        cr.forward = lambda x, _o=orig, _c=cap: _c.setdefault("reg", _o(_c.setdefault("var", x)))
        outputs, extra_out = m(st, sample, features=features, extra=extra, outputs=outputs, int_r=None)
        cr.forward = orig
        o = outputs[f"stage{st + 1}"]
        assert extra_out is o["variance"] and set(o) == {"depth", "photometric_confidence", "prob_volume", "variance", "depth_values"}
        hyp = o["depth_values"][0].cpu().numpy()
        np.testing.assert_allclose(*uo.pinned(g, f"s{st}_depth_values", hyp), rtol=5e-6, err_msg=f"hypotheses stage {st + 1}")
        vol = cap["var"]            # conv0's input travels as a SplitVolume (fp16 hi + mid pieces)
        vol = (vol.float() if hasattr(vol, "buf") else vol[0]).cpu().numpy().reshape(-1)
        e_vol = np.abs(vol[g[f"s{st}_volume_idx"]] - g[f"s{st}_volume_val"]).max()
        print(f"stage {st + 1}: sampled cost-volume voxels off by at most {e_vol:.2e} (values up to {np.abs(g[f's{st}_volume_val']).max():.1f})")
        np.testing.assert_allclose(vol[g[f"s{st}_volume_idx"]], g[f"s{st}_volume_val"], atol=2e-4)
        reg = cap["reg"][0, 0].cpu().numpy()
        np.testing.assert_allclose(reg, g[f"s{st}_reg"], atol=2e-3, err_msg=f"reg stage {st + 1}")
        assert np.abs(reg - g[f"s{st}_reg"]).mean() < 5e-5
        np.testing.assert_allclose(o["depth"][0].cpu().numpy(), g[f"s{st}_depth"], rtol=2e-5)
        dconf = np.abs(o["photometric_confidence"][0].cpu().numpy() - g[f"s{st}_conf"])
        assert (dconf > 1e-4).mean() < 0.01
        np.testing.assert_allclose(*uo.pinned(g, f"s{st}_prob", o["prob_volume"][0].cpu().numpy()), atol=2e-5, err_msg=f"prob stage {st + 1}")
        want_v = g[f"s{st}_variance"].astype(F64)
        tol_v = (np.expm1(2 * 2e-3) / 2) * want_v + lamb * 1e-5 * np.abs(hyp).max(0) + uo.variance_floor(hyp, lamb)
        dv_ = np.abs(o["variance"][0].cpu().numpy() - want_v)
        print(f"stage {st + 1}: variance off by at most {(dv_ / want_v).max():.2e} of itself, {(dv_ / tol_v).max():.2f} of its bound")
        assert (dv_ <= tol_v).all(), f"variance stage {st + 1}"
        # ---- the tail alone on the reference's logits and hypotheses: index exact outside near-ties, variance to 2e-5
        dvs = g[f"s{st}_depth_values"]
        prob, depth, conf, idx, var = costvol.prob_depth_conf_var(G(g[f"s{st}_reg"], dev), G(dvs, dev), lamb)
        r_prob, r_depth, r_conf, r_idx, r_idxf = tref.tail64(g[f"s{st}_reg"], dvs)
        tie = tref.near_tie(r_idxf, r_prob, dvs.shape[0])
        assert tie.mean() <= TIE_CAP
        assert np.array_equal(idx.cpu().numpy()[~tie], r_idx[~tie])
        same = idx.cpu().numpy() == r_idx
        np.testing.assert_allclose(conf.cpu().numpy()[same], g[f"s{st}_conf"][same], atol=1e-6)
        v64 = uo.variance64(g[f"s{st}_reg"], dvs, lamb)
        assert (np.abs(var.cpu().numpy() - v64) <= 2e-5 * v64 + uo.variance_floor(dvs, lamb)).all()
        np.testing.assert_allclose(var.cpu().numpy(), g[f"s{st}_variance"], rtol=4e-5, atol=float(uo.variance_floor(dvs, lamb).max()))
        stage_out.append(dict(prob_volume=o["prob_volume"], depth_values=o["depth_values"]))
        # ---- the next stage starts from the reference's maps
        nxt = G(g["stage1_depth_override"] if st == 0 else g[f"s{st}_depth"], dev)[None]
        outputs[f"stage{st + 1}"]["depth"] = nxt
        outputs["depth"] = nxt
        extra = G(g[f"s{st}_variance"], dev)[None]
    # ---- VolOpt-style consumption: each stage's probability volume and hypotheses go through the prior look-up as three views
    # of different (D,h,w), the way get_mvs_input hands them over.  (No float64 comparison here: hypotheses 0.2 apart at a depth
    # of 900 leave float32 three digits of the normalised depth; tests/test_gpu_costvol_tail.py holds the look-up to float64.)
    H, W = uo.FIXTURE_HW
    K = np.eye(4, dtype=F32); K[0, 0] = K[1, 1] = 120.0; K[0, 2], K[1, 2] = (W - 1) / 2, (H - 1) / 2
    views = [dict(K=torch.from_numpy(K), c2w=torch.eye(4), cost=o["prob_volume"][0], z_mvs=o["depth_values"][0]) for o in stage_out]
    rs = np.random.default_rng(5)
    z = rs.uniform(440, 920, (32, 24))
    xy = rs.uniform(-0.9, 0.9, (32, 1, 2)) * np.array([(W - 1) / 2, (H - 1) / 2]) / 120.0
    xyz = np.concatenate([xy * z[..., None], z[..., None]], -1).astype(F32)
    pj, pi, valid = ops.cost_lookup(views, 2, (H, W), xyz=G(xyz, dev))
    assert pj.shape == pi.shape == valid.shape == (32, 24)
    assert valid.all()                                                  # stage 1's planes span every sampled depth
    assert torch.isfinite(pj).all() and torch.isfinite(pi).all() and (pj >= 0).all() and (pj <= 2.0 + 1e-5).all() and (pj > 0).any()
    costvol.clear_caches()


def test_stage_loop_with_the_mirror(dev, g):
    """runner.py:178-243 through StageLoop with the real mirror: three reference views x three stages extract the features of
    three images once each (model.feature_extraction: UCSNet has no `feature`), int_r stays None, and the uncertainty each
    view's stage returns comes back as its `extra` at the next stage -- whose hypotheses are then the float32 restatement's on
    that view's own previous depth (handed off as runner.py:240-243 does) and uncertainty, bit for bit."""
    from svs_hip.stage_loop import StageLoop
    m = _model(dev, g)
    H, W = uo.FIXTURE_HW
    rng = np.random.default_rng(3)
    images = [torch.from_numpy(rng.uniform(0, 1, (1, 3, H, W)).astype(F32)).to(dev) for _ in range(3)]
    _, proj, depth_values = uo.fixture_sample(11)
    samples = []
    for r in range(3):
        order = [r] + [v for v in range(3) if v != r]
        samples.append(dict(imgs=torch.stack([images[v].clone() for v in order], 1), depth_values=G(depth_values, dev)[None],
                            proj_matrices={k: G(v[order], dev)[None] for k, v in proj.items()}))
    loop = StageLoop(m)
    outs, extras = [None] * 3, None
    for st in range(3):
        prev = [(None, None) if st == 0 else (o["depth"][0].cpu().numpy(), e[0].cpu().numpy()) for o, e in zip(outs, extras or [None] * 3)]
        outs, extras = loop.cost_volumes(st, samples, outs, view_extra_samples=extras)
        for i, (o, e) in enumerate(zip(outs, extras)):
            assert e is o[f"stage{st + 1}"]["variance"] and torch.isfinite(e).all() and torch.isfinite(o["depth"]).all()
            if st:
                sc = (4, 2, 1)[st]
                want = uo.uncertainty_samples32(prev[i][0], prev[i][1], (H // sc, W // sc), m.stage_configs[st])
                assert np.array_equal(o["depth_values"][0].cpu().numpy(), want), (st, i)
        depths = [o[f"stage{st + 1}"]["depth"] * 1.01 for o in outs]          # stands in for the rendered depths
        outs = StageLoop.hand_off_depth(outs, st, depths)
    assert loop.feature_calls == 3
    assert len({float(e.sum()) for e in extras}) == 3                        # three different views
    loop.clear()
