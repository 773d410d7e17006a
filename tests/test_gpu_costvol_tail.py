"""The three kernels between the regularised cost volume and the MVS prior of the loss -- svs_prob_depth_conf,
svs_depth_hypotheses (csrc/svs_costvol.hip) and svs_cost_lookup (csrc/svs_render.hip) -- against the float64 references of
tests/costvol_tail_ref.py at the shapes where their dispatch changes: every template instance of the softmax, its register-cached
path on both sides of its limit, last blocks that are not full, images smaller than a block, the clipped confidence window;
linear / inverse planes and previous depths at every ratio to the image; 1..4 views of different sizes, point counts around the
64-point block, ray and explicit-point mode, the device-side view index, points on every edge of the frustum.

The inputs come from tests/costvol_tail_cases.py; tests/test_costvol_tail_cpu.py shows on the same arrays, without a GPU, that
the references are right and that the only items excluded here -- near-ties of the truncated index, points within 1e-5 of a
validity threshold -- stay below 0.2 % of the pixels / 0.05 % of the points of every input.  Every test prints the figures it
asserts on (pytest -s)."""
import numpy as np
import pytest
import torch

import costvol_tail_cases as cases
import costvol_tail_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
TIE_CAP = 0.002
THRESHOLD_CAP = 0.0005


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def G(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def take(*tensors):
    """Host copies of kernel outputs; the device buffers are then filled with NaN, so that a later launch which is handed the
    same memory by the allocator cannot pass on what an earlier one left there."""
    out = [t.cpu().numpy() for t in tensors]
    for t in tensors:
        if t.is_floating_point():
            t.fill_(float("nan"))
        else:
            t.fill_(-1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# softmax over D, depth regression, confidence
# ---------------------------------------------------------------------------------------------------------------------
def _tail_no_index(reg, dv):
    """svs_prob_depth_conf with index = NULL, outputs preset to NaN."""
    from svs_hip import lib
    from svs_hip.ops import _ptr, _stream
    L = lib.load()
    D, H, W = reg.shape
    prob = torch.full((D, H, W), float("nan"), device=reg.device)
    depth = torch.full((H, W), float("nan"), device=reg.device)
    conf = torch.full((H, W), float("nan"), device=reg.device)
    lib.check(L.svs_prob_depth_conf(_ptr(reg), _ptr(dv), D, H, W, _ptr(prob), _ptr(depth), _ptr(conf), None, _stream()),
              "svs_prob_depth_conf")
    return prob, depth, conf


def _check_tail(tag, got, want, reg, dv, stats):
    """The assertions of one launch against tail64's outputs.
    prob:  |got - ref| <= 1e-9 + (16 + 2 |reg_d - max|) 2^-24 ref  (costvol_tail_ref.prob_rtol).  Derivation: the kernel forms
           exp2((x - max) * log2 e); the float32 subtraction and the product round once each, |x - max| 2^-24 of the exponent
           apiece, which the exponential turns into that relative error; the rounded constant log2 e adds a quarter as much;
           the exponential instruction is good to 2^-23; the float32 sum over D and the division cost a few units, for which
           the 16 stands.  At the spread of the d192 fixture (|x - max| < 70, probabilities above 1e-9 only for |x - max| < 21)
           this is the existing rtol = 1e-5.
    sum of prob = 1 to 1e-5; depth to 3e-6 of the pixel's largest hypothesis; conf to 1e-6 where the index agrees: the bounds
    of test_tail_d192_golden and test_config3_sizes_run.  idx: exact outside the near-tie set."""
    prob, depth, conf, idx = got
    r_prob, r_depth, r_conf, r_idx, r_idxf = want
    D = reg.shape[0]
    assert np.isfinite(prob).all() and np.isfinite(depth).all() and np.isfinite(conf).all(), tag
    tie = ref.near_tie(r_idxf, r_prob, D)
    assert tie.mean() <= TIE_CAP, tag
    assert np.array_equal(idx[~tie], r_idx[~tie]), f"{tag}: index differs at {int((idx != r_idx)[~tie].sum())} pixels"
    assert (np.abs(idx - r_idx)[tie] <= 1).all(), tag
    e_prob = np.abs(prob - r_prob) / (1e-9 + ref.prob_rtol(reg) * r_prob)
    e_sum = np.abs(prob.astype(F64).sum(0) - 1.0)
    e_depth = np.abs(depth - r_depth) / (3e-6 * np.abs(dv).max(0))
    same = idx == r_idx
    e_conf = np.abs(conf - r_conf)[same]
    stats["prob"] = max(stats.get("prob", 0.0), float(e_prob.max()))
    stats["sum"] = max(stats.get("sum", 0.0), float(e_sum.max()))
    stats["depth"] = max(stats.get("depth", 0.0), float(e_depth.max()))
    stats["conf"] = max(stats.get("conf", 0.0), float(e_conf.max()) if e_conf.size else 0.0)
    stats["ties"] = stats.get("ties", 0) + int(tie.sum())
    far = np.abs(reg.astype(F64) - reg.astype(F64).max(0, keepdims=True)) > 30
    if far.any():
        stats["prob_far"] = max(stats.get("prob_far", 0.0), float(e_prob[far].max()))
    assert e_prob.max() <= 1.0, f"{tag}: prob at {e_prob.max():.3f} of its bound"
    assert e_sum.max() <= 1e-5, f"{tag}: sum of prob off by {e_sum.max():.2e}"
    assert e_depth.max() <= 1.0, f"{tag}: depth at {e_depth.max():.3f} of its bound"
    assert e_conf.size == 0 or e_conf.max() <= 1e-6, f"{tag}: conf off by {e_conf.max():.2e}"


@pytest.mark.parametrize("D", cases.TAIL_D)
def test_tail_vs_float64(dev, D):
    """Every D of the dispatch edges (DS = 1 / 4 / 8 at 16 and 64; the register-cached path up to 24 * DS = 192 and the
    re-reading one beyond) x 1, 31, 33, 63, 65, 255, 257, 37 x 53 and 128 x 160 pixels, the seven logit families of
    costvol_tail_cases.tail_case side by side in every image, per-pixel hypotheses.  A second launch adds +-1e4 to the
    quantised spread-10 pixels (exactly representable, so the softmax must not move); a third passes index = NULL and
    must give the other outputs bit for bit."""
    from svs_hip import costvol
    stats = {}
    for (H, W, shift) in cases.tail_shapes():
        reg, dv, offset, fam, target = cases.tail_case(D, H, W, shift)
        tag = f"D={D} {H}x{W} shift {shift}"
        want = ref.tail64(reg, dv)
        d_reg, d_dv = G(reg, dev), G(dv, dev)
        out = costvol.prob_depth_conf(d_reg, d_dv)
        assert out[0].shape == (D, H, W) and out[3].dtype == torch.int32
        if H * W in (1, 257, 37 * 53):
            bare = _tail_no_index(d_reg, d_dv)
            for a, b in zip(bare, out[:3]):
                assert torch.equal(a, b), f"{tag}: index = NULL changes an output"
        got = take(*out)
        _check_tail(tag, got, want, reg, dv, stats)
        w = fam == cases.FAMILIES.index("window")
        assert np.array_equal(got[3][w], target[w]), tag
        if offset.any():
            shifted = (reg + offset[None]).astype(F32)
            got2 = take(*costvol.prob_depth_conf(G(shifted, dev), d_dv))
            _check_tail(tag + " offset", got2, want, reg, dv, stats)            # the reference of the plain logits
            moved = np.abs(got2[0] - got[0]) / (1e-9 + ref.prob_rtol(reg) * want[0])
            stats["offset"] = max(stats.get("offset", 0.0), float(moved.max()))
            assert moved.max() <= 1.0, f"{tag}: a common offset moves prob by {moved.max():.3f} of the bound"
    print(f"\ntail D={D}: worst error / bound: prob {stats['prob']:.3f} (|x-max| > 30: {stats.get('prob_far', 0.0):.3f}), "
          f"depth {stats['depth']:.3f}; |sum-1| {stats['sum']:.2e}, conf {stats['conf']:.2e}, offset move "
          f"{stats.get('offset', 0.0):.3f}, near-ties excluded {stats['ties']}")


# ---------------------------------------------------------------------------------------------------------------------
# depth hypotheses
# ---------------------------------------------------------------------------------------------------------------------
HYPO_RTOL = 5e-6              # the bound of test_three_stage_forward_golden


@pytest.mark.parametrize("D,inverse,rng_", cases.HYPO_STAGE1)
def test_hypotheses_stage1(dev, D, inverse, rng_):
    """Linear and inverse planes; 10 x 13 and 9 x 30 pixels per plane (neither a multiple of 256)."""
    from svs_hip import costvol
    worst, mirror = 0.0, 0.0
    for img_hw, scale in (((40, 52), 4), ((18, 60), 2)):
        got, = take(costvol.depth_hypotheses(None, img_hw, D, scale, rng_[0], rng_[1], 0.0, inverse, dev))
        want = ref.hypotheses64(None, img_hw, D, scale, rng_[0], rng_[1], 0.0, inverse)
        assert got.shape == want.shape == (D, img_hw[0] // scale, img_hw[1] // scale)
        worst = max(worst, float((np.abs(got - want) / np.abs(want)).max()))
        np.testing.assert_allclose(got, want, rtol=HYPO_RTOL)
        assert (got == got[:, :1, :1]).all(), "a stage-1 plane is constant over the image"
        if inverse:
            # Planes d and D-1-d mirror each other in 1/depth: 1/z[d] + 1/z[D-1-d] = 1/dmin + 1/dmax, to 8 * 2^-24 of that sum.
            # With u = 2^-24, a = 1/dmin, b = 1/dmax and the plane's fraction t, each float32 plane 1 / (a (1-t) + b t)
            # carries: a, 1-t and their product one rounding each (3 u of that term), b and b t 2 u, the sum 1 u, the final
            # reciprocal up to 2.5 u (a division that need not be correctly rounded) -- at most 6.5 u of 1/z, every term
            # being positive; the two fractions of a mirrored pair add up to 1 within half an ulp of 1, u/2 of |a - b|.
            inv = 1.0 / got[:, 0, 0].astype(F64)
            total = 1.0 / float(F32(rng_[0])) + 1.0 / float(F32(rng_[1]))
            mirror = max(mirror, float(np.abs(inv + inv[::-1] - total).max() / total))
            assert np.all(np.abs(inv + inv[::-1] - total) <= 8 * 2.0 ** -24 * total), f"mirror off by {mirror:.2e} of the sum"
    print(f"\nhypotheses stage 1 D={D} inverse={inverse} {rng_}: worst relative error {worst:.2e} (bound {HYPO_RTOL:.0e}), "
          f"mirror sum off by {mirror:.2e} of it (bound {8 * 2.0 ** -24:.1e})")


@pytest.mark.parametrize("img_hw,scale,prev_hw,D", cases.hypo_later_cases())
def test_hypotheses_later_stages(dev, img_hw, scale, prev_hw, D):
    """Previous depth at 1/4, 1/2 and 1/1 of the image (the last is what StageLoop.hand_off_depth passes) and at a ratio that
    is no integer, against the reference's two real resizes: bilinear to the image, then TRILINEAR to (D, H/s, W/s) -- which
    the kernel replaces by "identity along D, 2 x 2 average in space".  Depths in 500..800 with the interval of the d192
    configuration, and in 2.0..3.0 (scene units) with +-0.4."""
    from svs_hip import costvol
    worst = 0.0
    for lo, hi, pix in ((500.0, 800.0, float(F32(0.5 * 510.0 / 192))), (2.0, 3.0, float(F32(0.8 / D)))):
        if img_hw == (576, 768) and lo < 100:
            continue
        prev = cases.prev_depth_field(prev_hw, 7, lo, hi)
        got, = take(costvol.depth_hypotheses(G(prev, dev), img_hw, D, scale, lo, hi, pix, False, dev))
        want = ref.hypotheses64(prev, img_hw, D, scale, lo, hi, pix, False)
        assert got.shape == want.shape
        worst = max(worst, float((np.abs(got - want) / np.abs(want)).max()))
        np.testing.assert_allclose(got, want, rtol=HYPO_RTOL)
    print(f"\nhypotheses {img_hw} /{scale} prev {prev_hw} D={D}: worst relative error {worst:.2e} (bound {HYPO_RTOL:.0e})")


@pytest.mark.parametrize("bad", [dict(D=1), dict(D=0), dict(H=66), dict(W=98), dict(scale=0), dict(scale=-2)])
def test_hypotheses_rejects(dev, bad):
    """D < 2, an image that the scale does not divide, scale < 1: a non-zero return code and a message, no launch."""
    from svs_hip import lib
    from svs_hip.ops import _ptr, _stream
    L = lib.load()
    a = dict(D=8, H=64, W=96, scale=4)
    a.update(bad)
    out = torch.full((8, 16, 24), 7.0, device=dev)
    rc = L.svs_depth_hypotheses(None, 0, 0, a["H"], a["W"], a["D"], a["scale"], 1.0, 2.0, 0.0, 0, _ptr(out), _stream())
    assert rc != 0
    assert b"svs_depth_hypotheses" in L.svs_last_error_string()
    assert bool((out == 7.0).all())
    with pytest.raises(lib.SvsError, match="svs_depth_hypotheses"):
        lib.check(rc, "svs_depth_hypotheses")


# ---------------------------------------------------------------------------------------------------------------------
# MVS prior look-up
# ---------------------------------------------------------------------------------------------------------------------
def lookup_atol(D):
    """3e-6 up to the fixtures' D = 48, 5e-5 at D = 192 (test_cost_lookup_golden, test_cost_lookup_ray_mode_full_size).  The
    bound grows with D because the trilinear weight along depth is (zn + 1) / 2 * (D - 1): one float32 ulp of the normalised
    depth zn moves it by about D * 2^-24, and neighbouring planes of a softmax volume differ by a sizeable part of 1 / D * e."""
    return 5e-5 if D > 48 else 3e-6


def _hypo_gpu(dev):
    from svs_hip import costvol

    def f(prev, img_hw, D, scale, dmin, dmax, pix, inverse):
        p = G(prev, dev) if prev is not None else None
        return costvol.depth_hypotheses(p, img_hw, D, scale, dmin, dmax, pix, inverse, dev).cpu().numpy()
    return f


def _device_views(views, dev):
    return [dict(K=v["K"], c2w=v["c2w"], cost=G(v["cost"], dev), z_near=G(v["z_near"], dev), z_far=G(v["z_far"], dev))
            for v in views]


def _check_lookup(tag, got, want, views, vi, stats, cap=THRESHOLD_CAP):
    pj, pi, valid = got
    r_pj, r_pi, r_valid, margins, _ = want
    near = ref.near_threshold(margins)
    assert near.mean() <= cap, f"{tag}: {int(near.sum())} points near a threshold"
    ok = ~near
    assert np.array_equal(valid[ok], r_valid[ok]), f"{tag}: valid differs at {int((valid != r_valid)[ok].sum())} points"
    assert np.isfinite(pj).all() and np.isfinite(pi).all(), tag
    ok = ok & (valid == r_valid)
    Ds = [v["cost"].shape[0] for v in views]
    others = [d for k, d in enumerate(Ds) if k != vi]
    e_pi, e_pj = np.abs(pi - r_pi)[ok], np.abs(pj - r_pj)[ok]
    a_pi, a_pj = lookup_atol(Ds[vi]), lookup_atol(max(others)) if others else 0.0
    for k, e, a in (("pi", e_pi, a_pi), ("pj", e_pj, a_pj)):
        stats[k] = max(stats.get(k, 0.0), float(e.max()) if e.size else 0.0)
        assert e.size == 0 or e.max() <= a, f"{tag}: {k} off by {e.max():.2e} (bound {a:.0e})"
        if e.size >= 500:                        # (a mean over a handful of points is no mean)
            stats[k + "_mean"] = float(e.mean())
            assert e.mean() < 1e-7, f"{tag}: mean {k} error {e.mean():.2e}"
    stats["near"] = stats.get("near", 0) + int(near.sum())
    return ok


@pytest.mark.parametrize("case", cases.lookup_cases(), ids=lambda c: c[0])
def test_lookup_vs_float64(dev, case):
    """1..4 views, equal or different in (D,H,W) -- (192,36,48), (32,72,96), (8,144,192), (48,36,48), the depth ranges of the
    72 x 96 and 144 x 192 ones produced by costvol.depth_hypotheses from a previous depth, so they vary per pixel -- and
    1, 63, 64, 65, 1000 points, in explicit-point and in ray mode, with and without inverse depth.  The two modes look the same
    rays up, but the kernel forms cam + z * dir itself (the compiler may contract it to fused multiply-adds), so each is held
    to its own float64 reference and the two to one another within the tolerance, not bit for bit.  `same_view_dev` holding
    each view index in turn (with a DIFFERENT by-value index next to it) equals the by-value call bit for bit."""
    from svs_hip import ops
    name, dims, (R, S), vi, inverse, seed = case
    V = len(dims)
    views = cases.make_views(seed, dims, _hypo_gpu(dev))
    dviews = _device_views(views, dev)
    cam, dirs, z, xyz = cases.random_rays(views, vi, R, S, seed)
    stats = {}
    exp_out = ops.cost_lookup(dviews, vi, cases.IMG_RES, xyz=G(xyz, dev), inverse_depth=inverse)
    assert exp_out[2].dtype == torch.bool and exp_out[0].shape == (R, S)
    for k in range(V):
        by_value = ops.cost_lookup(dviews, k, cases.IMG_RES, xyz=G(xyz, dev), inverse_depth=inverse)
        by_dev = ops.cost_lookup(dviews, (k + 1) % max(V, 2), cases.IMG_RES, xyz=G(xyz, dev), inverse_depth=inverse,
                                 same_view_dev=torch.tensor([k], dtype=torch.int32, device=dev))
        for a, b in zip(by_value, by_dev):
            assert torch.equal(a, b), f"{name}: same_view_dev = {k} differs from the by-value index"
    got = take(*exp_out)
    want = ref.cost_mapping64(xyz, vi, views, cases.IMG_RES, inverse)
    ok = _check_lookup(name + " explicit", got, want, views, vi, stats)
    got_r = take(*ops.cost_lookup(dviews, vi, cases.IMG_RES, cam=G(cam, dev), dirs=G(dirs, dev), z=G(z, dev),
                                  inverse_depth=inverse))
    xyz_ray = cam.astype(F64)[None, None] + z.astype(F64)[:, :, None] * dirs.astype(F64)[:, None, :]
    want_r = ref.cost_mapping64(xyz_ray, vi, views, cases.IMG_RES, inverse)
    ok_r = _check_lookup(name + " ray", got_r, want_r, views, vi, stats)
    both = ok & ok_r
    Ds = [d[0] for d in dims]
    assert np.array_equal(got[2][both], got_r[2][both])
    assert np.all(np.abs(got[1] - got_r[1])[both] <= lookup_atol(Ds[vi]))
    if V > 1:
        assert np.all(np.abs(got[0] - got_r[0])[both] <= lookup_atol(max(d for k, d in enumerate(Ds) if k != vi)))
    if V == 1:
        for o in (got, got_r):
            assert not o[0].any() and not o[1].any() and not o[2].any(), "one view: pj = 0, pi = 0, valid = 0"
    elif R * S >= 1000:
        assert 0.02 < got[2].mean() < 0.98
    if R * S >= 1000:
        assert "pi_mean" in stats and "pj_mean" in stats, "the 1000-point inputs must reach the mean-error assertion"
    print(f"\nlookup {name}: max |pi| error {stats['pi']:.2e}, |pj| {stats['pj']:.2e}, means {stats.get('pi_mean', float('nan')):.1e}"
          f" / {stats.get('pj_mean', float('nan')):.1e}, valid {got[2].mean():.2f}, excluded {stats['near']}")


def test_lookup_five_views_rejected(dev):
    from svs_hip import lib, ops
    views = cases.make_views(3, cases.EQUAL_DIMS, _hypo_gpu(dev))
    dviews = _device_views(views + views[:1], dev)
    xyz = G(np.zeros((2, 3, 3), F32), dev)
    with pytest.raises(lib.SvsError, match="views"):
        ops.cost_lookup(dviews, 0, cases.IMG_RES, xyz=xyz)


@pytest.mark.parametrize("inverse", [False, True])
def test_lookup_edge_points(dev, inverse):
    """Points un-projected from view 0 of the mixed set (D = 192 at 36 x 48), so that their place in that view is known: the
    four image corners and border mid-points, x or y at +-1.0005 (inside the 1.001 bound but past the last texel: the weights
    are partial) and at +-1.002 (invalid), behind the camera, on the first and on the last plane, normalised depth +-1.005
    (beyond the last plane, inside the 1.01 bound) and +-1.04 (invalid); and a point that view 0 alone sees.  None of them
    lies within 1e-5 of a threshold (test_costvol_tail_cpu.py), so nothing is excluded and `valid` is exact."""
    from svs_hip import ops
    views = cases.make_views(70, cases.MIXED_DIMS[:3], _hypo_gpu(dev))
    dviews = _device_views(views, dev)
    xyz, expected, labels = cases.edge_points(views, 0, inverse)
    stats = {}
    for vi in range(3):
        got = take(*ops.cost_lookup(dviews, vi, cases.IMG_RES, xyz=G(xyz, dev), inverse_depth=inverse))
        want = ref.cost_mapping64(xyz, vi, views, cases.IMG_RES, inverse)
        _check_lookup(f"edge vi={vi}", got, want, views, vi, stats, cap=0.0)
    # view 0 on its own (twice, so that one copy is the "other" view): the valid points sample it, the others return 0
    two = [dviews[0], dviews[0]]
    pj, pi, valid = take(*ops.cost_lookup(two, 1, cases.IMG_RES, xyz=G(xyz, dev), inverse_depth=inverse))
    assert np.array_equal(valid[0], expected), [l for l, a, b in zip(labels, valid[0], expected) if a != b]
    want = ref.cost_mapping64(xyz, 1, [views[0], views[0]], cases.IMG_RES, inverse)
    _check_lookup("edge view 0 alone", (pj, pi, valid), want, [views[0], views[0]], 1, stats, cap=0.0)
    assert (pj[0][expected] > 1e-5).all() and (pj[0][~expected] == 0).all()
    if not inverse:
        lone = cases.lonely_point(views)
        for vi in range(3):
            pj, pi, valid = take(*ops.cost_lookup(dviews, vi, cases.IMG_RES, xyz=G(lone, dev)))
            want = ref.cost_mapping64(lone, vi, views, cases.IMG_RES, False)
            _check_lookup(f"lonely vi={vi}", (pj, pi, valid), want, views, vi, stats, cap=0.0)
            assert bool(valid[0, 0]) == (vi != 0)
            if vi == 0:
                assert pi[0, 0] == 0 and pj[0, 0] == 0          # seen by the rendered view only: masked out
    print(f"\nlookup edge points inverse={inverse}: max |pi| error {stats['pi']:.2e}, |pj| {stats['pj']:.2e}")


def test_lookup_partial_weights_tight(dev):
    """x, y or both at +-1.0005 on a volume that is the same on every plane (costvol_tail_cases.partial_weight_case): the
    normalised depth, which makes these points ill-conditioned in a probability volume, drops out, and the partial weight of
    the last texel is held to 3e-6 -- a dropped or a fully weighted last texel would be off by 6e-4 or more.  Nothing is
    excluded (test_costvol_tail_cpu.py::test_partial_weight_points_sit_clearly)."""
    from svs_hip import ops
    view, xyz, weight = cases.partial_weight_case()
    dviews = _device_views([view, view], dev)
    stats = {}
    got = take(*ops.cost_lookup(dviews, 1, cases.IMG_RES, xyz=G(xyz, dev)))
    want = ref.cost_mapping64(xyz, 1, [view, view], cases.IMG_RES, False)
    _check_lookup("partial weights", got, want, [view, view], 1, stats, cap=0.0)
    assert got[2].all()
    print(f"\nlookup partial weights: max |pi| error {stats['pi']:.2e}, |pj| {stats['pj']:.2e} (bound 3e-06), weights "
          f"{weight.min():.4f} .. {weight.max():.4f}")


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
def test_chain_tail_hypotheses_tail_lookup(dev):
    """64 x 96 image, D = (16, 8, 8) at scales (4, 2, 1), random logits: hypotheses -> tail three times over, then the look-up
    over one view per stage, on the GPU, each stage fed with the GPU's previous output, against the same chain in float64 fed
    with its own (costvol_tail_ref.chain64 / chain_lookup64; inputs: costvol_tail_cases.chain_inputs).  Hypotheses, prob and
    depth are held to their bounds above plus the error their input carries, measured on the reference: its input is moved by
    the previous stage's tolerance and the change of its output is added.  The index and the confidence depend on the logits
    alone, which both sides share, so they carry nothing: the index is exact outside the near-ties, the confidence good to
    1e-6.  In the look-up, `valid` is exact outside the points whose margin the carried tolerance of the planes could use up;
    test_costvol_tail_cpu.py::test_chain_inputs_caps_and_oracle holds those to CHAIN_CARRIED_CAP points, the near-ties to
    0.2 % and the points within 1e-5 of a threshold to 0.05 %, as here."""
    from svs_hip import costvol, ops
    regs, cams, xyz = cases.chain_inputs()
    (dmin, dmax), img = cases.CHAIN_RANGE, cases.CHAIN_IMG
    stages = ref.chain64(regs, img, cases.CHAIN_SCALE, dmin, dmax, cases.CHAIN_PIX, hypo_rtol=HYPO_RTOL, depth_rtol=3e-6)
    g_prev, dviews, lines = None, [], []
    for k, (reg, r) in enumerate(zip(regs, stages)):
        D, tag = reg.shape[0], f"chain stage {k + 1}"
        g_h = costvol.depth_hypotheses(g_prev, img, D, cases.CHAIN_SCALE[k], dmin, dmax, cases.CHAIN_PIX[k], False, dev)
        g_p, g_d, g_c, g_i = costvol.prob_depth_conf(G(reg, dev), g_h)
        h, p, d, c, i = (t.cpu().numpy() for t in (g_h, g_p, g_d, g_c, g_i))
        e_h, e_p, e_d = np.abs(h - r["h"]) / r["t_h"], np.abs(p - r["prob"]) / r["t_p"], np.abs(d - r["depth"]) / r["t_d"]
        tie = ref.near_tie(r["idx_f"], r["prob"], D)
        same = i == r["idx"]
        e_c = np.abs(c - r["conf"])[same]
        lines.append(f"stage {k + 1}: error / bound: hypotheses {e_h.max():.3f}, prob {e_p.max():.3f}, depth {e_d.max():.3f}; "
                     f"conf {e_c.max():.2e}, near-ties {int(tie.sum())}")
        assert e_h.max() <= 1.0, f"{tag}: hypotheses at {e_h.max():.3f} of their bound"
        assert e_p.max() <= 1.0, f"{tag}: prob at {e_p.max():.3f} of its bound"
        assert e_d.max() <= 1.0, f"{tag}: depth at {e_d.max():.3f} of its bound"
        assert tie.mean() <= TIE_CAP, tag
        assert np.array_equal(i[~tie], r["idx"][~tie]), tag
        assert e_c.max() <= 1e-6, f"{tag}: conf off by {e_c.max():.2e}"
        dviews.append(dict(K=cams[k]["K"], c2w=cams[k]["c2w"], cost=g_p, z_near=g_h[0].contiguous(),
                           z_far=g_h[-1].contiguous()))
        g_prev = g_d
    # look-up: view k holds stage k's volume and its first and last plane
    for vi in range(3):
        got = take(*ops.cost_lookup(dviews, vi, cases.IMG_RES, xyz=G(xyz, dev)))
        want, carried_pj, carried_pi, carried_m = ref.chain_lookup64(xyz, vi, cams, stages, cases.IMG_RES)
        assert ref.near_threshold(want[3]).mean() <= THRESHOLD_CAP
        near = want[3].min(-1).min(0) < 1e-5 + carried_m
        assert near.sum() <= cases.CHAIN_CARRIED_CAP
        ok = ~near
        assert np.array_equal(got[2][ok], want[2][ok]), f"chain look-up vi={vi}: valid differs"
        assert 0.05 < got[2].mean() < 0.95
        ok = ok & (got[2] == want[2])
        e_pi, e_pj = np.abs(got[1] - want[1])[ok], np.abs(got[0] - want[0])[ok]
        lines.append(f"look-up vi={vi}: pi {e_pi.max():.2e} (carried up to {carried_pi.max():.2e}), pj {e_pj.max():.2e} "
                     f"(carried up to {carried_pj.max():.2e}), excluded {int(near.sum())}")
        assert np.all(e_pi <= 3e-6 + carried_pi[ok]), f"chain look-up vi={vi}: pi"
        assert np.all(e_pj <= 3e-6 + carried_pj[ok]), f"chain look-up vi={vi}: pj"
    print("\nchain: " + "\n       ".join(lines))
