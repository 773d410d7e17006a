"""UCSNet without a GPU: the restatement of tests/ucsnet_oracle.py reproduces what the reference wrote into
tests/golden/ucsnet_3stage.npz (so that the GPU tests may lean on it at other sizes), the mirror's state dict is the
reference's, and StageLoop takes UCSNet's route for a model without `feature` / `depth_interals_ratio`."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import costvol_tail_ref as tref
import ucsnet_oracle as uo

F32, F64 = np.float32, np.float64
TIE_CAP = 0.002            # the share of near-tie pixels tests/test_costvol_tail_cpu.py allows an input


@pytest.fixture(scope="module")
def g(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ucsnet_3stage.npz")))


def test_mirror_state_dict_is_the_reference_s(g):
    """models.ucsnet.UCSNet has the reference's 258 state-dict entries, names, order and shapes, and loads them strictly."""
    from models.ucsnet import UCSNetHip as UCSNet          # the mirror, whether or not a checkout is on the path
    from svs_hip import refpath
    m = UCSNet(lamb=1.5, stage_configs=[16, 8, 8], grad_method="detach", base_chs=[8, 8, 8], feat_ext_ch=8)
    assert refpath.in_this_tree(UCSNet)
    if refpath.reference_root() is None:            # no checkout on the path: the reference's name gives the mirror
        import models.ucsnet
        assert models.ucsnet.UCSNet is UCSNet
    sd = m.state_dict()
    assert len(g["state_dict_keys"]) == 258
    assert list(sd.keys()) == [str(k) for k in g["state_dict_keys"]]
    assert [",".join(str(n) for n in v.shape) for v in sd.values()] == [str(s) for s in g["state_dict_shapes"]]
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in uo.ucsnet_state_dict().items()}, strict=True)
    m.train()
    with pytest.raises(NotImplementedError):
        m(0, dict(imgs=None, proj_matrices=None, depth_values=None), features=[], extra=None, outputs=None, int_r=None)
    # CasMVSNet keeps its own names
    from models.CasMVSNet import CostRegNet
    assert [k for k in CostRegNet(8, 8).state_dict() if k.startswith(("conv7.", "conv9.", "conv11."))]


@pytest.mark.parametrize("cin,cout,hw", [(32, 16, (1, 1)), (16, 8, (3, 5)), (5, 3, (4, 7))])
def test_tap_rule_is_conv_transpose2d(cin, cout, hw):
    rs = np.random.default_rng(cin + hw[1])
    x, w, b = rs.standard_normal((cin,) + hw), rs.standard_normal((cin, cout, 3, 3)), rs.standard_normal(cout)
    ref = Fn.conv_transpose2d(torch.from_numpy(x)[None], torch.from_numpy(w), torch.from_numpy(b), stride=2, padding=1,
                              output_padding=1)[0].numpy()
    got = uo.deconv2d_taps(x, w, b)
    assert got.shape == (cout, 2 * hw[0], 2 * hw[1])
    np.testing.assert_allclose(got, ref, atol=1e-12 * np.abs(ref).max())


def test_feature_extractor_restatement_vs_fixture(g):
    """float64 restatement against the reference's float32 outputs: the 1e-5 tests/test_gpu_costvol.py holds the FPN to."""
    out = uo.feat_ext_net(uo.make_featext_params(int(g["seed"])), uo.fixture_image(int(g["seed"])))
    for k in ("stage1", "stage2", "stage3", "deconv1_raw", "deconv2_raw"):
        got, want = uo.pinned(g, "feat_" + k, out[k])
        np.testing.assert_allclose(got, want, atol=1e-5, err_msg=k)
        assert np.abs(want).max() > 0.1


def test_bilinear_restatement_is_interpolate():
    rs = np.random.default_rng(3)
    for (hp, wp), hw in (((16, 24), (32, 48)), ((10, 13), (20, 26)), ((64, 96), (64, 96)), ((7, 9), (20, 31))):
        a = rs.uniform(1, 2, (hp, wp))
        ref = Fn.interpolate(torch.from_numpy(a)[None, None], list(hw), mode="bilinear")[0, 0].numpy()
        np.testing.assert_allclose(uo.resize_bilinear64(a, hw), ref, rtol=1e-14)
        ref32 = Fn.interpolate(torch.from_numpy(a.astype(F32))[None, None], list(hw), mode="bilinear")[0, 0].numpy()
        np.testing.assert_allclose(uo.resize_bilinear32(a.astype(F32), hw), ref32, rtol=3e-7)


def test_hypotheses_restatement_vs_fixture(g):
    """Stages 2 and 3 from the fixture's previous depth (stage 1: the override) and uncertainty: the float32 restatement within
    1e-6 of the reference's hypotheses (8 ulp: torch's vectorised resize associates its four products differently, each map is
    then good to 2 ulp and the sample adds three more roundings; two thirds of the values are equal bit for bit, the largest
    difference is 3.5e-7), the float64 one within the 5e-6 the GPU test holds the kernel to; stage 1's planes bit for bit."""
    H, W = uo.FIXTURE_HW
    _, _, dv = uo.fixture_sample(int(g["seed"]))
    want0 = uo.pinned(g, "s0_depth_values", np.broadcast_to(uo.stage1_planes(dv[0], dv[-1], 16, False).reshape(-1, 1, 1), (16, H // 4, W // 4)))
    assert np.array_equal(*want0)
    prev = {1: g["stage1_depth_override"], 2: g["s1_depth"]}
    for st, sc in ((1, 2), (2, 1)):
        hw = (H // sc, W // sc)
        got32, want = uo.pinned(g, f"s{st}_depth_values", uo.uncertainty_samples32(prev[st], g[f"s{st - 1}_variance"], hw, 8))
        np.testing.assert_allclose(got32, want, rtol=1e-6, err_msg=f"stage {st + 1}")
        got64, want = uo.pinned(g, f"s{st}_depth_values", uo.uncertainty_samples64(prev[st], g[f"s{st - 1}_variance"], hw, 8))
        np.testing.assert_allclose(got64, want, rtol=5e-6, err_msg=f"stage {st + 1}")


def test_clamp_at_zero_depth():
    """var >= cur: the first hypothesis is exactly eps (the reference gives 1e-12, 1.3333, 2.6667, 4.0 at cur 1, var 3)"""
    h = uo.uncertainty_samples32(np.full((2, 2), 1.0, F32), np.full((2, 2), 3.0, F32), (2, 2), 4)[:, 0, 0]
    assert h[0] == F32(1e-12)
    np.testing.assert_allclose(h[1:], [4.0 / 3, 8.0 / 3, 4.0], rtol=2e-7)
    z = uo.uncertainty_samples32(np.full((2, 2), 5.0, F32), np.zeros((2, 2), F32), (4, 4), 8)
    assert np.all(z == z[0]) and np.all(z == F32(5.0))


def test_variance_restatement_vs_fixture(g):
    """variance64 on the fixture's own logits and hypotheses against the reference's float32 variance: 2e-5 relative (the
    float32 softmax, 1e-5, and a few roundings of the sum; the depth's own error enters only to second order, since
    d/d(depth) sum p (z - depth)^2 = 0 at depth = sum p z) above the floor a rounded depth leaves of a zero variance; and the
    fixture's logits stay within the near-tie cap the GPU test's index comparison relies on."""
    for st in range(3):
        reg = g[f"s{st}_reg"]
        dv = g[f"s{st}_depth_values"]
        want = uo.variance64(reg, dv, float(g["lamb"]))
        np.testing.assert_array_less(np.abs(g[f"s{st}_variance"] - want), 2e-5 * want + uo.variance_floor(dv, float(g["lamb"])))
        prob, depth, conf, idx, idx_f = tref.tail64(reg, dv)
        np.testing.assert_allclose(g[f"s{st}_depth"], depth, rtol=3e-6)
        assert tref.near_tie(idx_f, prob, reg.shape[0]).mean() <= TIE_CAP, f"stage {st + 1}"
    v = g["s0_variance"]
    assert v.max() >= 3 * v.min()


class _StubUcs:
    """what StageLoop sees of UCSNet: `feature_extraction`, no `feature`, no `depth_interals_ratio`"""

    def __init__(self):
        self.calls = []

    def feature_extraction(self, img):
        return {"stage1": img.sum()}

    def __call__(self, stage_idx, sample, features, extra, outputs, int_r, prevent_oom=False, inverse_depth=False):
        self.calls.append((stage_idx, extra, int_r, len(features)))
        return {"depth": stage_idx}, ("var", stage_idx, sample["id"])


class _StubCas:
    depth_interals_ratio = [4, 2, 1]

    def __init__(self):
        self.calls = []

    def feature(self, img):
        return {"stage1": img.sum()}

    def feature_extraction(self, img):
        raise AssertionError("CasMVSNet's extractor is `feature`")

    def __call__(self, stage_idx, sample, features, extra, outputs, int_r, prevent_oom=False, inverse_depth=False):
        self.calls.append((stage_idx, extra, int_r, len(features)))
        return {"depth": stage_idx}, None


def test_stage_loop_routes():
    from svs_hip.stage_loop import StageLoop
    rs = np.random.default_rng(0)
    imgs = [torch.from_numpy(rs.uniform(0, 1, (1, 3, 8, 12)).astype(F32)) for _ in range(3)]
    samples = [dict(id=r, imgs=torch.stack([imgs[v] for v in [r] + [v for v in range(3) if v != r]], 1)) for r in range(3)]
    for stub, want_r in ((_StubUcs(), [None, None, None]), (_StubCas(), [4, 2, 1])):
        loop = StageLoop(stub)
        outs, extras = [None] * 3, None
        for st in range(3):
            outs, extras = loop.cost_volumes(st, samples, outs, view_extra_samples=extras)
        assert loop.feature_calls == 3
        assert [c[2] for c in stub.calls[::3]] == want_r
        assert all(c[3] == 3 for c in stub.calls)
        if isinstance(stub, _StubUcs):
            # the previous stage's second return value of the same view comes back as `extra`
            assert [c[1] for c in stub.calls[:3]] == [None] * 3
            assert [c[1] for c in stub.calls[3:6]] == [("var", 0, r) for r in range(3)]
            assert [c[1] for c in stub.calls[6:]] == [("var", 1, r) for r in range(3)]
        else:
            assert all(c[1] is None for c in stub.calls)
