"""CPU-side checks of TransMVSNet's test infrastructure and of what runs without a device: the restatements of
tests/transmvs_oracle.py against what the reference wrote into tests/golden/transmvs_3stage.npz, the deformable convolution's
restatement three independent ways, the mirror's state dict, the orchestration of models/transmvs.py's transformer (with
float64 stand-ins for the kernels), StageLoop's call of it, and the fixture's near-tie share.

Tolerances: the reference is a float32 computation of the formulas the oracle restates, so it may be as far from the float64
restatement as the oracle's own float32 restatement is, times transmvs_oracle.ALLOW_FACTOR -- computed here, per piece."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import transmvs_oracle as to

F32, F64 = np.float32, np.float64
T32, T64 = to.T32, to.T64


@pytest.fixture(scope="module")
def g(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "transmvs_3stage.npz")))


@pytest.fixture(scope="module")
def sd(g):
    return to.transmvs_state_dict(int(g["seed"]))


@pytest.fixture(scope="module")
def matched(sd):
    """fmt_with_pathway on the fixture's features in float64 and float32"""
    feats = to.fixture_sample()[0]
    p = to.sub(sd, "FMT_with_pathway")
    return {td: to.fmt_with_pathway(p, feats, td) for td in (T64, T32)}


def _close(g, name, a64, a32, what=None):
    tol = to.allowance(a32, a64)
    got, want = to.pinned(g, name, a64)
    err = np.abs(got - want).max()
    print(f"{what or name}: reference off the float64 restatement by {err:.2e}, allowed {tol:.2e}")
    assert err <= tol, (name, err, tol)
    return tol


# ---------------------------------------------------------------------------------------------------------------------
# the deformable convolution's restatement, three ways
# ---------------------------------------------------------------------------------------------------------------------
def _dcn_inputs(seed, H=9, W=11, Cout=8):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (32, H, W)), rng.normal(0, 0.1, (Cout, 32, 3, 3)), rng.normal(0, 0.1, Cout),
            rng.uniform(0.1, 0.9, (9, H, W)))


def test_dcn_zero_offsets_is_a_masked_convolution():
    x, w, b, mask = _dcn_inputs(0)
    got = to.deform_conv2d_tv(to.T(x)[None], torch.zeros(1, 18, 9, 11, dtype=T64), to.T(w), to.T(b), mask=to.T(mask)[None])[0]
    # mask * conv, tap by tap
    want = sum(Fn.conv2d(to.T(x)[None], to.T(w * (np.arange(9).reshape(3, 3) == k)), padding=1) * to.T(mask)[None, k:k + 1]
               for k in range(9))[0] + to.T(b).view(-1, 1, 1)
    assert np.abs((got - want).numpy()).max() < 1e-12
    ones = to.deform_conv2d_tv(to.T(x)[None], torch.zeros(1, 18, 9, 11, dtype=T64), to.T(w), to.T(b), mask=torch.ones(1, 9, 9, 11, dtype=T64))
    assert np.abs((ones - Fn.conv2d(to.T(x)[None], to.T(w), to.T(b), padding=1)).numpy()).max() < 1e-12


def test_dcn_integer_offsets_are_a_shifted_convolution():
    x, w, b, mask = _dcn_inputs(1)
    H, W = x.shape[1:]
    shifts = [(2, -1), (0, 3), (-4, 0), (1, 1), (-1, -2), (5, 5), (0, 0), (-3, 2), (2, 2)]
    off = np.zeros((18, H, W))
    want = np.zeros((8, H, W))
    pad = np.zeros((32, H + 20, W + 20))
    pad[:, 10:10 + H, 10:10 + W] = x
    for k, (dy, dx) in enumerate(shifts):
        off[2 * k], off[2 * k + 1] = dy, dx
        ky, kx = divmod(k, 3)
        shifted = pad[:, 10 + ky - 1 + dy:10 + ky - 1 + dy + H, 10 + kx - 1 + dx:10 + kx - 1 + dx + W]
        want += np.einsum("oc,chw->ohw", w[:, :, ky, kx], shifted * mask[k][None])
    got = to.deform_conv2d_tv(to.T(x)[None], to.T(off)[None], to.T(w), None, mask=to.T(mask)[None])[0].numpy()
    assert np.abs(got - want).max() < 1e-12
    assert np.abs(to.deform_conv2d_gather(x, off, w, None, mask) - want).max() < 1e-12


def test_dcn_gather_form_at_fractional_offsets_and_borders():
    x, w, b, mask = _dcn_inputs(2)
    H, W = x.shape[1:]
    rng = np.random.default_rng(3)
    off = rng.uniform(-4, 4, (18, H, W))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    # sampling points at exactly -1, H-1 and H (rows) / -1, W-1 and W (columns), by tap
    for k, (ty, tx) in enumerate([(-1.0, 2.5), (H - 1.0, 0.25), (float(H), 1.0), (3.5, -1.0), (0.75, W - 1.0), (2.0, float(W)),
                                  (-1.0, -1.0), (H - 1.0, W - 1.0), (-0.5, W - 0.5)]):
        ky, kx = divmod(k, 3)
        off[2 * k, :, ::2] = (ty - (yy + ky - 1))[:, ::2]
        off[2 * k + 1, :, ::2] = (tx - (xx + kx - 1))[:, ::2]
    got = to.deform_conv2d_tv(to.T(x)[None], to.T(off)[None], to.T(w), to.T(b), mask=to.T(mask)[None])[0].numpy()
    want = to.deform_conv2d_gather(x, off, w, b, mask)
    # (the grid_sample form passes the point through normalised coordinates: 1e-15 of a pixel at these sizes)
    assert np.abs(got - want).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the restatements reproduce the fixture
# ---------------------------------------------------------------------------------------------------------------------
def test_extractor_restatement(g, sd):
    p = to.sub(sd, "feature")
    f64, f32 = to.feature_net(p, to.fixture_image(), T64), to.feature_net(p, to.fixture_image(), T32)
    for k in ("stage1", "stage2", "stage3"):
        _close(g, "feat_" + k, f64[k], f32[k])


def test_transformer_and_pathway_restatement(g, matched):
    (out64, ref64), (out32, ref32) = matched[T64], matched[T32]
    for i in range(4):
        _close(g, f"fmt_ref{i}", ref64[i], ref32[i])
    for v in (0, 1):
        for k in ("stage1", "stage2", "stage3"):
            _close(g, f"fmt_v{v}_{k}", out64[v][k], out32[v][k])


@pytest.fixture(scope="module")
def stages(g, sd, matched):
    """per stage, in float64 and float32: similarity, view weights, logits -- each stage from the reference's previous depth
    and view weights"""
    _, proj, depth_values = to.fixture_sample()
    out = []
    for st in range(3):
        hyp = to.hypotheses(None if st == 0 else g[f"s{st - 1}_depth"], st, depth_values, int(g["ratios"][st]))
        prev_w = None if st == 0 else to.upsample_nearest2(g["s0_view_weights"], st - 1)
        res = {"hyp": hyp}
        for td in (T64, T32):
            feats = [f[f"stage{st + 1}"] for f in matched[td][0]]
            sim, w = to.similarity_volume(feats, proj[f"stage{st + 1}"], hyp, prev_w, to.sub(sd, "DepthNet.pixel_wise_net"), td)
            res[td] = dict(sim=sim, w=w, reg=to.cost_reg(to.sub(sd, f"cost_regularization.{st}"), sim[None], td))
        out.append(res)
    return out


def test_three_stage_restatement_and_near_tie_cap(g, stages):
    for st, res in enumerate(stages):
        r64, r32 = res[T64], res[T32]
        np.testing.assert_allclose(*to.pinned(g, f"s{st}_depth_values", res["hyp"]), rtol=5e-6)
        _close(g, f"s{st}_similarity", r64["sim"], r32["sim"])
        if st == 0:
            _close(g, "s0_view_weights", r64["w"], r32["w"])
        tol = _close(g, f"s{st}_reg", r64["reg"], r32["reg"])
        # the cap on what the winner-take-all comparison may leave out: a condition on the fixture, with this allowance
        gap = to.top_two_gap(g[f"s{st}_reg"])
        share = (gap <= 2 * tol).mean()
        print(f"stage {st + 1}: logit allowance {tol:.2e}, {100 * share:.2f} % of the pixels have a top-two gap within twice that")
        assert 2 * tol <= 1e-3 and share <= to.TIE_CAP
        prob, idx, depth, conf = to.tail_wta(g[f"s{st}_reg"], res["hyp"])
        np.testing.assert_allclose(*to.pinned(g, f"s{st}_prob", prob), rtol=2e-5, atol=1e-9)
        np.testing.assert_allclose(g[f"s{st}_depth"], depth, rtol=5e-6)
        np.testing.assert_allclose(g[f"s{st}_conf"], conf, rtol=2e-5)
        # and from the restated logits, where the reference's winner is clear
        clear = gap > 2 * tol
        assert np.array_equal(np.argmax(r64["reg"], 0)[clear], idx[clear])


# ---------------------------------------------------------------------------------------------------------------------
# the mirror
# ---------------------------------------------------------------------------------------------------------------------
def _mirror(g, sd):
    from models.transmvs import TransMVSNet, TransMVSNetHip
    assert TransMVSNet is TransMVSNetHip
    m = TransMVSNetHip(refine=False, ndepths=[int(x) for x in g["ndepths"]], depth_interals_ratio=[int(x) for x in g["ratios"]],
                       share_cr=False, grad_method="detach", arch_mode="fpn", cr_base_chs=[8, 8, 8])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval()


def test_mirror_state_dict_is_the_reference_s(g, sd):
    m = _mirror(g, sd)
    state = m.state_dict()
    assert len(state) == 465
    assert list(state.keys()) == list(g["state_dict_keys"])
    assert [",".join(str(n) for n in v.shape) for v in state.values()] == list(g["state_dict_shapes"])
    assert not any("pos_encoding" in k for k in state)
    for attr in ("feature", "FMT_with_pathway", "cost_regularization", "DepthNet", "depth_interals_ratio", "ndepths"):
        assert hasattr(m, attr)
    assert hasattr(m.DepthNet, "pixel_wise_net")
    from models.transmvs import TransMVSNetHip
    for kw in (dict(refine=True), dict(share_cr=True), dict(ndepths=[8, 8], depth_interals_ratio=[2, 1])):
        with pytest.raises(NotImplementedError):
            TransMVSNetHip(**kw)
    with pytest.raises(NotImplementedError):
        m.train()(0, None, None, None, None, None)
    import models
    assert not hasattr(models, "TransMVSNetHip") and hasattr(models, "CascadeMVSNet")


def test_transformer_orchestration_leaves_its_input_unchanged(g, sd, matched, monkeypatch):
    """FMT_with_pathway of models/transmvs.py with float64 stand-ins for its six kernels: which layer reads which source, the
    order of reduction, up-sampling and smoothing -- against the fixture -- and its input dicts afterwards."""
    from svs_hip import costvol

    def fmt_kv(source, k_w, k_b, v_w, v_b):
        K = Fn.elu((source @ k_w.double().t() + k_b.double()).view(-1, 8, 4)) + 1
        V = (source @ v_w.double().t() + v_b.double()).view(-1, 8, 4)
        return torch.cat([torch.einsum("shd,shm->hmd", K, V).reshape(-1), K.sum(0).reshape(-1)])

    def fmt_layer(x, kv, ws):
        qw, qb, ow, ob, w1, b1, w2, b2, g1, c1, g2, c2 = [w.detach().double() for w in ws]
        Q = Fn.elu((x @ qw.t() + qb).view(-1, 8, 4)) + 1
        Z = 1 / (torch.einsum("lhd,hd->lh", Q, kv[128:].view(8, 4)) + 1e-6)
        x = x + torch.einsum("lhd,hmd,lh->lhm", Q, kv[:128].view(8, 4, 4), Z).reshape(-1, 32) @ ow.t() + ob
        x = Fn.layer_norm(x, (32,), g1, c1, 1e-5)
        return Fn.layer_norm(x + Fn.relu(x @ w1.t() + b1) @ w2.t() + b2, (32,), g2, c2, 1e-5)

    monkeypatch.setattr(costvol, "fmt_tokens_in", lambda f: to.tokens(f.numpy(), T64, pe=True))
    monkeypatch.setattr(costvol, "fmt_tokens_out", lambda t, hw: t.t().reshape(32, *hw))
    monkeypatch.setattr(costvol, "fmt_kv", fmt_kv)
    monkeypatch.setattr(costvol, "fmt_layer", fmt_layer)
    monkeypatch.setattr(costvol, "pathway_step", lambda x, w, y: torch.from_numpy(to.pathway_step(x.numpy(), w.detach().numpy(), y.numpy())))
    monkeypatch.setattr(costvol, "conv2d", lambda x, w: Fn.conv2d(x.double()[None], w.double(), padding=1)[0])
    m = _mirror(g, sd)
    feats = to.fixture_sample()[0]
    features = [{k: torch.from_numpy(v)[None] for k, v in f.items()} for f in feats]
    keep = [{k: (v, v.clone()) for k, v in f.items()} for f in features]
    out = m.FMT_with_pathway(features)
    for f, k in zip(features, keep):
        assert set(f) == set(k)
        for name, (same, copy) in k.items():
            assert f[name] is same and torch.equal(same, copy)
    out64, out32 = matched[T64][0], matched[T32][0]
    for v in (0, 1):
        for k in ("stage1", "stage2", "stage3"):
            assert out[v][k].shape[0] == 1 and out[v][k] is not features[v][k]
            got, want = to.pinned(g, f"fmt_v{v}_{k}", out[v][k][0].numpy())
            assert np.abs(got - want).max() <= to.allowance(out32[v][k], out64[v][k])


def test_stage_loop_calls_the_transformer_once_per_sample():
    from svs_hip.stage_loop import StageLoop
    calls = []

    class WithFMT:
        depth_interals_ratio = [4, 2, 1]

        def feature(self, img):
            calls.append("feature")
            return {"stage1": img * 2}

        def FMT_with_pathway(self, features):
            calls.append(("fmt", len(features)))
            return [{"stage1": f["stage1"] + 1} for f in features]

        def __call__(self, stage_idx, sample, features, extra, outputs, int_r, prevent_oom, inverse_depth):
            calls.append(("model", stage_idx, int_r, [float(f["stage1"].sum()) for f in features]))
            return {"depth": None}, "weights"

    class Plain(WithFMT):
        FMT_with_pathway = property()          # no such attribute: hasattr is False

    imgs = [torch.full((1, 3, 4, 4), float(v + 1)) for v in range(3)]
    samples = [dict(imgs=torch.stack([imgs[v] for v in order], 1)) for order in ((0, 1, 2), (1, 0, 2))]
    loop = StageLoop(WithFMT())
    loop.clear = lambda: None
    outs, extras = [None, None], None
    for st in range(3):
        outs, extras = loop.cost_volumes(st, samples, outs, view_extra_samples=extras)
        assert extras == ["weights", "weights"]
    # three images extracted once each, the transformer once per sample (it depends on the order of the views), both before
    # the first model call that uses them; 6 model calls on the transformer's output (+1), the cache untouched
    assert loop.feature_calls == 3 and loop.fmt_calls == 2
    assert [c for c in calls if c == "feature" or c[0] == "fmt"] == ["feature"] * 3 + [("fmt", 3), ("fmt", 3)]
    assert calls.index(("fmt", 3)) < [i for i, c in enumerate(calls) if c[0] == "model"][0]
    models = [c for c in calls if c[0] == "model"]
    assert len(models) == 6 and models[0][3] == [2 * 48 + 48.0, 4 * 48 + 48.0, 6 * 48 + 48.0] and models[1][3][0] == 4 * 48 + 48.0
    assert [c[2] for c in models] == [4, 4, 2, 2, 1, 1]
    assert all(float(f["stage1"].sum()) in (96.0, 192.0, 288.0) for f in loop._features.values())
    calls.clear()
    plain = StageLoop(Plain())
    assert not hasattr(plain.model, "FMT_with_pathway")
    plain.cost_volumes(0, samples, [None, None])
    assert plain.fmt_calls == 0 and not any(c[0] == "fmt" for c in calls if c != "feature")
    assert [c for c in calls if c != "feature"][0][3] == [96.0, 192.0, 288.0]
