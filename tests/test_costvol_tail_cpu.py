"""The float64 references of tests/costvol_tail_ref.py are right before any GPU sees them, and the exclusion caps of
tests/test_gpu_costvol_tail.py hold on every input that file uses -- both shown here with the float32 oracles alone.

  * Each reference agrees with its float32 oracle (casmvs_oracle.depthnet_tail / depth_hypotheses, svs_oracle.cost_mapping)
    to float32 rounding, and with the reference-generated fixtures at the tolerances the GPU tests apply to them.
  * A float32 evaluation can legitimately land on the other side of a discrete decision.  A pixel is a near-tie when its
    float64 sum p*k lies within D * 2^-20 of an integer (costvol_tail_ref.near_tie); a point is near-threshold when one of its
    validity margins is below 1e-5 in the compared unit.  The GPU tests exclude only those; here: at most 0.2 % of the pixels
    of every tail input and 0.05 % of the points of every look-up input are excluded, outside them the float32 oracle's
    index / `valid` equals the reference's, and the deliberate edge cases (window clipping, border points, points on the
    first / last plane, ...) exclude nothing."""
import os

import numpy as np
import pytest

import casmvs_oracle as corc
import costvol_tail_cases as cases
import costvol_tail_ref as ref
import svs_oracle as orc
import synth

F32 = np.float32
F64 = np.float64
TIE_CAP = 0.002
THRESHOLD_CAP = 0.0005


def load(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name + ".npz")))


def hypo_cpu(prev, img_hw, D, scale, dmin, dmax, pix, inverse):
    return ref.hypotheses64(prev, img_hw, D, scale, dmin, dmax, pix, inverse).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# tail
# ---------------------------------------------------------------------------------------------------------------------
def test_tail64_fixture_d192(golden_dir):
    g = load(golden_dir, "depthnet_tail_d192")
    prob, depth, conf, idx, idx_f = ref.tail64(g["reg"], g["depth_values"])
    np.testing.assert_allclose(prob, g["prob"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(depth, g["depth"], rtol=3e-6)
    tie = ref.near_tie(idx_f, prob, 192)
    assert tie.mean() <= TIE_CAP
    assert np.array_equal(idx[~tie], g["idx"][~tie])
    same = idx == g["idx"]
    np.testing.assert_allclose(conf[same], g["conf"][same], atol=1e-6)


def test_tail64_fixture_three_stages(golden_dir):
    g = load(golden_dir, "casmvs_3stage")
    for st in range(3):
        prob, depth, conf, idx, idx_f = ref.tail64(g[f"s{st}_reg"], g[f"s{st}_depth_values"])
        np.testing.assert_allclose(prob, g[f"s{st}_prob"], rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(depth, g[f"s{st}_depth"], rtol=3e-6)
        tie = ref.near_tie(idx_f, prob, prob.shape[0])
        assert tie.mean() <= TIE_CAP
        np.testing.assert_allclose(conf[~tie], g[f"s{st}_conf"][~tie], atol=1e-6)


@pytest.mark.parametrize("D", cases.TAIL_D)
def test_tail_inputs_caps_and_oracle(D):
    """Every input of the GPU tail test: the near-tie share, the float32 oracle against the reference outside it, and the
    constructed families sitting where they were put."""
    for (H, W, shift) in cases.tail_shapes():
        reg, dv, offset, fam, target = cases.tail_case(D, H, W, shift)
        prob, depth, conf, idx, idx_f = ref.tail64(reg, dv)
        tie = ref.near_tie(idx_f, prob, D)
        tag = f"D={D} {H}x{W} shift {shift}"
        assert tie.mean() <= TIE_CAP, f"{tag}: {int(tie.sum())} near-ties"
        # only the random families may hold a near-tie: the constructed ones sit clearly on one side
        built = np.isin(fam, [cases.FAMILIES.index(n) for n in ("flat", "peak200", "window")])
        assert not (tie & built).any(), tag
        frac = np.abs(idx_f - np.rint(idx_f))
        one_hot = prob.max(0) == 1.0
        decided = (frac > 0.05) | one_hot | (np.rint(idx_f) == 0)
        assert decided[built].all(), tag
        w = fam == cases.FAMILIES.index("window")
        assert np.array_equal(idx[w], target[w]), tag
        # the float32 oracle
        o_prob, o_depth, o_conf, o_idx = corc.depthnet_tail(reg, dv)
        assert np.array_equal(o_idx[~tie], idx[~tie]), tag
        # (the oracle subtracts the maximum in float32 before its float64 exponential: the bound's |x - max| term)
        assert np.all(np.abs(o_prob - prob) <= 1e-37 + 0.5 * ref.prob_rtol(reg) * prob), tag
        assert np.all(np.abs(o_depth - depth) <= 3e-6 * np.abs(dv).max(0)), tag
        same = o_idx == idx
        np.testing.assert_allclose(o_conf[same], conf[same], atol=1e-6, err_msg=tag)
        # the offset launch: float32(reg + offset) is exact, so its softmax is that of reg
        shifted = (reg + offset[None]).astype(F32)
        assert np.array_equal(shifted.astype(F64) - offset[None].astype(F64), reg.astype(F64)), tag
        if H * W > 1:
            q = fam == cases.FAMILIES.index("q10")
            assert (offset[q] > 0).any() and (offset[q] < 0).any(), tag


def test_tail_window_terms():
    """The window family clips the confidence window as announced: 3 terms at index 0 and D-2, 4 at index 1 (D >= 4), 2 at
    D-1, every present term well above the confidence tolerance except the underflowed ones of the one-hot pixels."""
    D = 17
    reg, dv, _, fam, target = cases.tail_case(D, 15, 17, 0)
    prob, _, conf, idx, _ = ref.tail64(reg, dv)
    w = fam == cases.FAMILIES.index("window")
    for t, terms in ((0, 3), (1, 4), (D - 2, 3), (D - 1, 2)):
        px = w & (target == t)
        assert px.any()
        lo, hi = max(t - 1, 0), min(t + 2, D - 1)
        assert hi - lo + 1 == terms
        np.testing.assert_allclose(conf[px], prob[lo:hi + 1][:, px].sum(0), rtol=1e-14)
        if t != D - 1:
            assert prob[lo:hi + 1][:, px].min() > 1e-2 and (conf[px] < 0.99).all()     # and mass outside the window


# ---------------------------------------------------------------------------------------------------------------------
# hypotheses
# ---------------------------------------------------------------------------------------------------------------------
def test_hypotheses64_fixture_three_stages(golden_dir):
    g = load(golden_dir, "casmvs_3stage")
    _, _, depth_values = synth.make_mvs_sample(int(g["seed"]), img_hw=(64, 96))
    ndepths = [int(x) for x in g["ndepths"]]
    dmin, dmax = float(depth_values[0]), float(depth_values[-1])
    interval = (dmax - dmin) / depth_values.shape[0]
    prev = None
    for st in range(3):
        got = ref.hypotheses64(prev, (64, 96), ndepths[st], (4, 2, 1)[st], dmin, dmax, (1.0, 0.5, 0.5)[st] * interval, False)
        np.testing.assert_allclose(got, g[f"s{st}_depth_values"], rtol=5e-6, err_msg=f"stage {st + 1}")
        prev = g["stage1_depth_override"] if st == 0 else g[f"s{st}_depth"]


@pytest.mark.parametrize("D,inverse,rng_", cases.HYPO_STAGE1)
def test_hypotheses64_stage1_vs_oracle(D, inverse, rng_):
    got = ref.hypotheses64(None, (40, 52), D, 4, rng_[0], rng_[1], 0.0, inverse)
    dv1d = np.linspace(rng_[0], rng_[1], 192).astype(F32)
    want = corc.depth_hypotheses(0, dv1d, (40, 52), D, 4, 1.0, inverse_depth=inverse)
    assert got.shape == want.shape == (D, 10, 13)
    np.testing.assert_allclose(got, want, rtol=1e-6)
    assert got[0, 0, 0] == pytest.approx(rng_[0], rel=1e-12) and got[-1, 0, 0] == pytest.approx(rng_[1], rel=1e-12)
    if inverse:                                                 # planes d and D-1-d mirror each other in 1/depth
        inv = 1.0 / got[:, 0, 0]
        np.testing.assert_allclose(inv + inv[::-1], 1.0 / rng_[0] + 1.0 / rng_[1], rtol=1e-13)


@pytest.mark.parametrize("img_hw,scale,prev_hw,D", [c for c in cases.hypo_later_cases() if c[0] != (576, 768)])
def test_hypotheses64_later_vs_oracle(img_hw, scale, prev_hw, D):
    prev = cases.prev_depth_field(prev_hw, 3)
    interval = (935.0 - 425.0) / 192
    got = ref.hypotheses64(prev, img_hw, D, scale, 425.0, 935.0, 0.5 * interval, False)
    dv1d = np.linspace(425.0, 935.0, 192).astype(F32)
    # the oracle forms the interval from (dmax - dmin) / 192 of the float32 range itself
    want = corc.depth_hypotheses(1, dv1d, img_hw, D, scale, 0.5, prev_depth=prev)
    np.testing.assert_allclose(got, want, rtol=2e-6)
    # "identity along D, linear in space" is what the trilinear resize amounts to at integer scales: plane d of the resized
    # volume only mixes plane d of the full one
    assert np.all(np.diff(got, axis=0) > 0)


# ---------------------------------------------------------------------------------------------------------------------
# look-up
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cost_mapping_inv0_v0", "cost_mapping_inv0_v2", "cost_mapping_inv1_v0",
                                  "cost_mapping_inv1_v2"])
def test_cost_mapping64_fixture(golden_dir, name):
    g = load(golden_dir, name)
    views = synth.make_mvs_views(int(g["seed"]))
    pj, pi, valid, margins, _ = ref.cost_mapping64(g["xyz"], int(g["view_index"]), views, (576, 768), bool(g["inverse_depth"]))
    near = ref.near_threshold(margins)
    assert near.mean() <= THRESHOLD_CAP
    assert np.array_equal(valid[~near], g["valid"][~near])
    # Where a view samples its depth range with partial weight, the reference's own float32 arithmetic is ill-conditioned
    # (costvol_tail_cases.past_last_texel); in these fixtures that is also the edge of view 2's band of zero hypotheses (rows
    # 0-3 of 36).  A handful of points (4 of the 9408 of the four fixtures lie above 3e-6, the worst at 9.5e-6): held to 2e-5
    # there, to the GPU test's 3e-6 everywhere else.
    x, y, z = cases.project64(views, g["xyz"])
    iy2 = (y[2] + 1) / 2 * 35
    ill = cases.past_last_texel(views, g["xyz"]) | ((iy2 > 3) & (iy2 < 4) & (np.abs(x[2]) <= 1.001) & (z[2] > 0))
    assert ill.mean() < 0.03
    # (the reference's float32 arithmetic against float64 measured 3.35e-6 at one point of each inverse-depth fixture, just
    # behind the first plane, where 1 - near / z cancels: pj, which adds two views, and the inverse-depth pi get twice 3e-6)
    ok = (valid == g["valid"]) & ~ill
    np.testing.assert_allclose(pj[ok], g["pj"][ok], atol=2 * 3e-6)
    np.testing.assert_allclose(pi[ok], g["pi"][ok], atol=2 * 3e-6 if bool(g["inverse_depth"]) else 3e-6)
    ok = (valid == g["valid"]) & ill
    np.testing.assert_allclose(pj[ok], g["pj"][ok], atol=2e-5)
    np.testing.assert_allclose(pi[ok], g["pi"][ok], atol=2e-5)


def _oracle_views(views):
    return [dict(K=v["K"], c2w=v["c2w"], cost=v["cost"], z_mvs=np.stack([v["z_near"], v["z_far"]])) for v in views]


def lookup_atol(D):
    return 5e-5 if D > 48 else 3e-6          # (D = 48: the fixtures' volumes, held to 3e-6 by the existing GPU test)


def _check_lookup_against_oracle(tag, xyz, vi, views, inverse, cap=THRESHOLD_CAP):
    pj, pi, valid, margins, _ = ref.cost_mapping64(xyz, vi, views, cases.IMG_RES, inverse)
    near = ref.near_threshold(margins)
    assert near.mean() <= cap, f"{tag}: {int(near.sum())} of {near.size} points near a threshold"
    o_pj, o_pi, o_valid = orc.cost_mapping(xyz, vi, _oracle_views(views), cases.IMG_RES, inverse)
    ok = ~near
    assert np.array_equal(o_valid[ok], valid[ok]), tag
    Ds = [v["cost"].shape[0] for v in views]
    others = [d for k, d in enumerate(Ds) if k != vi]
    np.testing.assert_allclose(o_pi[ok], pi[ok], atol=lookup_atol(Ds[vi]), err_msg=tag)
    if others:
        np.testing.assert_allclose(o_pj[ok], pj[ok], atol=lookup_atol(max(others)), err_msg=tag)
    return valid, near


@pytest.mark.parametrize("case", cases.lookup_cases(), ids=lambda c: c[0])
def test_lookup_inputs_caps_and_oracle(case):
    name, dims, (R, S), vi, inverse, seed = case
    views = cases.make_views(seed, dims, hypo_cpu)
    cam, dirs, z, xyz = cases.random_rays(views, vi, R, S, seed)
    valid, _ = _check_lookup_against_oracle(name, xyz, vi, views, inverse)
    # ray mode looks the same rays up at cam + z * dir, which the reference forms in float64
    xyz_ray = cam.astype(F64)[None, None] + z.astype(F64)[:, :, None] * dirs.astype(F64)[:, None, :]
    _, _, _, margins, _ = ref.cost_mapping64(xyz_ray, vi, views, cases.IMG_RES, inverse)
    assert ref.near_threshold(margins).mean() <= THRESHOLD_CAP
    if len(dims) == 1:
        assert not valid.any()
    elif R * S >= 1000:
        assert 0.02 < valid.mean() < 0.98, "the input must mix valid and invalid points"


@pytest.mark.parametrize("inverse", [False, True])
def test_lookup_edge_points_sit_clearly(inverse):
    """The edge-case points, un-projected from view 0: none within 1e-5 of any threshold in any view (nothing is excluded),
    each on the announced side in view 0, and the border / partial-weight / last-plane points really sample the volume."""
    views = cases.make_views(70, cases.MIXED_DIMS[:3], hypo_cpu)
    xyz, expected, labels = cases.edge_points(views, 0, inverse)
    for vi in range(3):
        _check_lookup_against_oracle(f"edge vi={vi}", xyz, vi, views, inverse, cap=0.0)
    _, _, _, margins, inval = ref.cost_mapping64(xyz, 1, views, cases.IMG_RES, inverse)
    assert margins.min() > 2e-4                                    # the closest: 1.0005 and 1.002 against 1.001
    got = ~inval[0, 0]
    assert np.array_equal(got, expected), [l for l, a, b in zip(labels, got, expected) if a != b]
    # two copies of view 0 alone: what the look-up returns for the valid ones is that view's sample, not 0
    pj, _, _, _, _ = ref.cost_mapping64(xyz, 1, [views[0], views[0]], cases.IMG_RES, inverse)
    assert (pj[0][expected] > 1e-5).all() and (pj[0][~expected] == 0).all()
    # and only view 0 sees its own partial-weight points that way
    other = cases.past_last_texel(views[1:], xyz)
    assert not other.any()


def test_lookup_lonely_point():
    views = cases.make_views(70, cases.MIXED_DIMS[:3], hypo_cpu)
    xyz = cases.lonely_point(views)
    for vi in range(3):
        valid, near = _check_lookup_against_oracle(f"lonely vi={vi}", xyz, vi, views, False, cap=0.0)
        assert bool(valid[0, 0]) == (vi != 0)
    _, _, _, _, inval = ref.cost_mapping64(xyz, 0, views, cases.IMG_RES, False)
    assert list(inval[:, 0, 0]) == [False, True, True]


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
def test_chain_inputs_caps_and_oracle():
    """The inputs of the GPU chain test, run through the float64 chain: near-ties under 0.2 % of the pixels of every stage,
    points within 1e-5 of a threshold under 0.05 %, and at most CHAIN_CARRIED_CAP points whose margin the carried tolerance
    of the planes could use up; outside them the float32 oracles -- fed with the reference's planes and volumes rounded to
    float32 -- give the reference's index and `valid`, and their depth, confidence, pi and pj lie within the bounds the GPU
    test applies."""
    regs, cams, xyz = cases.chain_inputs()
    assert [r.shape for r in regs] == [(16, 16, 24), (8, 32, 48), (8, 64, 96)]
    stages = ref.chain64(regs, cases.CHAIN_IMG, cases.CHAIN_SCALE, *cases.CHAIN_RANGE, cases.CHAIN_PIX)
    for k, (reg, r) in enumerate(zip(regs, stages)):
        tie = ref.near_tie(r["idx_f"], r["prob"], reg.shape[0])
        assert tie.mean() <= TIE_CAP, f"stage {k + 1}: {int(tie.sum())} near-ties"
        o_prob, o_depth, o_conf, o_idx = corc.depthnet_tail(reg, r["h"].astype(F32))
        assert np.array_equal(o_idx[~tie], r["idx"][~tie])
        assert np.all(np.abs(o_prob - r["prob"]) <= r["t_p"])
        assert np.all(np.abs(o_depth - r["depth"]) <= r["t_d"])
        same = o_idx == r["idx"]
        np.testing.assert_allclose(o_conf[same], r["conf"][same], atol=1e-6)
    o_views = [dict(K=c["K"], c2w=c["c2w"], cost=r["prob"].astype(F32), z_mvs=np.stack([r["h"][0], r["h"][-1]]).astype(F32))
               for c, r in zip(cams, stages)]
    for vi in range(3):
        want, carried_pj, carried_pi, carried_m = ref.chain_lookup64(xyz, vi, cams, stages, cases.IMG_RES)
        assert ref.near_threshold(want[3]).mean() <= THRESHOLD_CAP
        near = want[3].min(-1).min(0) < 1e-5 + carried_m
        assert near.sum() <= cases.CHAIN_CARRIED_CAP, f"vi={vi}: {int(near.sum())} points within the carried margin"
        o_pj, o_pi, o_valid = orc.cost_mapping(xyz, vi, o_views, cases.IMG_RES, False)
        ok = ~near
        assert np.array_equal(o_valid[ok], want[2][ok])
        assert 0.05 < want[2].mean() < 0.95
        assert np.all(np.abs(o_pi - want[1])[ok] <= 3e-6 + carried_pi[ok])
        assert np.all(np.abs(o_pj - want[0])[ok] <= 3e-6 + carried_pj[ok])


def test_partial_weight_points_sit_clearly():
    """The partial-weight points on the depth-constant volume: nothing near a threshold, all valid, the reference's sample is
    the border texels' bilinear value times the weight left inside the image, and the float32 oracle is within 3e-6 of it."""
    view, xyz, weight = cases.partial_weight_case()
    pj, pi, valid, margins, _ = ref.cost_mapping64(xyz, 1, [view, view], cases.IMG_RES, False)
    assert not ref.near_threshold(margins).any() and margins.min() > 2e-4
    assert valid.all()
    assert ((weight > 0.97) & (weight < 0.995)).all()
    assert np.all(pj > 0.9 * 0.05) and np.all(pj < 0.125) and np.array_equal(pj, pi)
    whole, _, _, _, _ = ref.cost_mapping64(cases.partial_weight_case(inside=True)[1], 1, [view, view], cases.IMG_RES, False)
    # (the points moved onto the last texel, times the weight; the points are float32, good to 2e-7 in x: 5e-6 of the weight)
    np.testing.assert_allclose(pj, weight * whole, rtol=1e-5)
    o_pj, o_pi, o_valid = orc.cost_mapping(xyz, 1, _oracle_views([view, view]), cases.IMG_RES, False)
    assert o_valid.all()
    np.testing.assert_allclose(o_pj, pj, atol=3e-6)
    np.testing.assert_allclose(o_pi, pi, atol=3e-6)
