"""Without a GPU: the float64 reference of tests/warp_cases.py is torch's grid_sample, its case table reaches every kernel
instance, corner state, depth transition and tail that tests/test_gpu_warp_edges.py is there for (counted from the float64
sample positions), the float32 comparator meets the GPU test's bound on every voxel of every case, and every mutant of the
reference misses that bound by a factor of 100 or more."""
import collections

import numpy as np
import pytest
import torch

import warp_cases as wc

F32 = np.float32
F64 = np.float64
NAMES = [k.name for k in wc.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_grid_sample(name):
    """warp64 == torch.nn.functional.grid_sample (float64, bilinear, zeros, align_corners=False) fed the grid the reference
    normalises with the (W-1)/2 formula, on every voxel with finite coordinates, to float64 rounding; voxels without finite
    coordinates are zero in the reference.  (Coordinates beyond 2^31 px are finite and stay in: both give 0 there.)"""
    k = wc.BY_NAME[name]
    feats, rts, dv = wc.features(k), wc.rot_trans(k), wc.depths(k)
    for v, (rot, trans) in enumerate(rts):
        got, pos, n_in, n_pos = wc.warp64(feats[v + 1], rot, trans, dv)
        with np.errstate(all="ignore"):
            px, py = pos["qx"] / pos["qz"], pos["qy"] / pos["qz"]
            gx, gy = px / ((k.W - 1) / 2.0) - 1.0, py / ((k.H - 1) / 2.0) - 1.0
        fin = np.isfinite(gx) & np.isfinite(gy)
        assert fin.sum() >= 0.9 * fin.size or k.D * k.H * k.W < 64
        grid = np.stack([np.where(fin, gx, -9.0), np.where(fin, gy, -9.0)], -1)            # (D,H,W,2)
        x = torch.from_numpy(feats[v + 1].astype(F64))[None].expand(k.D, -1, -1, -1)
        ref = torch.nn.functional.grid_sample(x, torch.from_numpy(grid), mode="bilinear", padding_mode="zeros", align_corners=False)
        ref = ref.permute(1, 0, 2, 3).numpy()                                               # (C,D,H,W)
        sel = np.broadcast_to(fin[None], got.shape)
        assert np.abs(got - ref)[sel].max() <= 1e-12
        assert (got[~sel] == 0).all() and (n_in[~fin] == 0).all()
        # strictly positive features: a positive value exactly where a corner of positive weight is inside
        assert np.array_equal(got > 0, np.broadcast_to((n_pos > 0)[None], got.shape))
        assert float(feats[v + 1].min()) >= 0.5


def test_launch_arguments_are_the_librarys():
    """The float32 rot / trans the reference takes are bit for bit what the comparator (corc.relative_proj) and the library
    (costvol.relative_projection, rounded to float as _rot_trans does) form from the same projection matrices, and they are the
    roundings of source_camera's."""
    from svs_hip import costvol
    for k in wc.CASES:
        P = wc.case_projs(k)
        for v, (rot, trans) in enumerate(wc.rot_trans(k)):
            assert rot.dtype == F32 and trans.dtype == F32
            lib12 = np.array(costvol.relative_projection(P[v + 1], P[0]), F64).astype(F32)
            assert np.array_equal(lib12[:9].reshape(3, 3), rot) and np.array_equal(lib12[9:], trans)
            r64, t64 = wc.source_camera(k.kinds[v], v, k.H, k.W)
            assert np.array_equal(r64.astype(F32), rot) and np.array_equal(t64.astype(F32), trans)


def test_split_dispatch():
    """costvol.split_fits holds for every case (restated from csrc/svs_split_volume.h, and asked of the library): the split call
    reaches warp_variance_reuse2_kernel, not the float32 kernel's split epilogue."""
    from svs_hip import costvol
    for k in wc.CASES:
        nbytes = wc.split_volume_bytes(k.C, k.D, k.H, k.W)
        assert nbytes < (1 << 32) and k.H * k.W * k.C * 4 < (1 << 31)
        assert costvol.split_fits(k.C, k.D, k.H, k.W)
        from svs_hip import lib
        assert lib.load().svs_split_volume_dims(k.C, k.D, k.H, k.W, None) == nbytes


def test_instances_and_tails():
    """All 12 (C, NS) instances (each case runs both kernels and, with source 0, the raw warp: every C), and per C every tail:
    D % 4 = 0..3 and D = 1, 2, 3 across the table; per C a D >= 64 with D % 4 != 0 (four planes per workgroup of the float32
    kernel), two x tiles of EACH kernel, a last tile with a full, a partly filled and an empty wave in one pass for each kernel,
    widths that are and are not multiples of 4; one case with H = W = 2.  Shapes stay small."""
    assert {(k.C, k.NS) for k in wc.CASES} == {(C, NS) for C in (8, 16, 32) for NS in (1, 2, 3, 4)}
    every = set().union(*(wc.tails(k) for k in wc.CASES))
    assert {f"D%4={r}" for r in range(4)} | {"D=1", "D=2", "D=3", "H=W=2"} <= every
    for C in (8, 16, 32):
        t = set().union(*(wc.tails(k) for k in wc.CASES if k.C == C))
        assert {"D>=64,D%4!=0", "two_f32_tiles", "two_split_tiles", "full_part_empty_f32", "full_part_empty_split", "W%4==0",
                "W%4!=0"} <= t, (C, t)
    for k in wc.CASES:
        assert k.H <= 12 and k.C * k.D * k.H * k.W * 4 <= 1 << 20 and len(k.kinds) == k.NS
    # the tiles of the two kernels (csrc/svs_costvol.hip: kWarpPasses = 5; WarpCfg<C, 4>)
    assert wc.F32_TILE == {C: 5 * 256 // (C // 4) for C in (8, 16, 32)}
    assert wc.SPLIT_TILE == {32: 5 * 32, 16: 2 * 64, 8: 1 * 128}


# what the table must reach, and how often at least: (across the table, per C).  Per C = per kernel instance family: every
# case runs both kernels on the same inputs.
MINIMUM = {
    "all_in": (10000, 1000), "x0_is_-1": (100, 20), "x1_is_W": (100, 20), "y0_is_-1": (1000, 100), "y1_is_H": (1000, 100),
    "two_sided": (100, 20), "outside_near": (1000, 100), "outside_2^31": (12, 4), "qz_neg_inside": (1000, 100),
    "qz_zero": (100, 20), "qz_sign_rows": (100, 20), "div_small_qz": (12, 4), "div_big_q": (12, 4), "div_big_q_inside": (12, 4),
    "hyp_zero": (12, 4), "hyp_neg": (12, 4), "hyp_inf": (12, 4), "hyp_nan": (12, 4),
    # inside one four-plane run of the split producer
    "step_0": (1000, 100), "step_1": (1000, 100), "step_more": (1000, 100), "in_to_out": (100, 20), "out_to_in": (100, 20),
    "enter_at_00": (30, 4), "wave_none_moves": (100, 20), "wave_some_move": (100, 20),
}


def test_categories_are_reached():
    """Counted from the float64 sample positions, summed over sources: corner states (all inside, each one-sided border, two-sided,
    outside by at most 8 px, outside beyond 2^31 px), q.z < 0 landing inside, q.z = 0, rows along which q.z changes sign, operands
    of the division fall-back (|q.z| < 2^-40; |q.x| or |q.y| >= 2^40, also landing inside), the isolated hypotheses 0, negative,
    +inf, NaN; and between two planes of one four-plane run: corners unchanged / moved by one pixel / by more, inside -> outside,
    outside -> inside, outside -> the cell (-1,-1) whose one corner inside is pixel (0,0) (offset 0 = the `outside' offset), waves
    (of the split producer: 8 / 16 / 32 consecutive voxels) in which no voxel's offsets change and in which some but not all do."""
    per_c = {C: collections.Counter() for C in (8, 16, 32)}
    for k in wc.CASES:
        n = wc.categories(k)
        print(k.name, dict(n))
        per_c[k.C] += n
    total = sum(per_c.values(), collections.Counter())
    for key, (table, each) in MINIMUM.items():
        assert total[key] >= table, (key, total[key])
        for C in (8, 16, 32):
            assert per_c[C][key] >= each, (key, C, per_c[C][key])
    # q.z exactly 0 and sign changes come from a `skew' source too, not only from the isolated hypotheses
    for C in (8, 16, 32):
        assert any("skew" in k.kinds and wc.categories(k)["qz_zero"] >= 10 for k in wc.CASES if k.C == C)


@pytest.mark.parametrize("name", NAMES)
def test_corners_are_decidable_in_float32(name):
    """No finite sample within MARGIN_PX of a line where a corner enters the image (warp_cases.undecided), and the float32
    positions (the comparator's arithmetic) lie within MARGIN_PX / 4 of the float64 ones wherever the sample is within reach of
    the image: float32 and float64 agree on which corners are inside, so no voxel has to be left out of the raw test's pattern --
    the comparator's raw warp is > 0 exactly where the reference says a corner of positive weight is inside."""
    k = wc.BY_NAME[name]
    dv, rts = wc.depths(k), wc.rot_trans(k)
    assert not wc.undecided(k, dv, rts).any()
    y, x = np.meshgrid(np.arange(k.H, dtype=F32), np.arange(k.W, dtype=F32), indexing="ij")
    for rot, trans in rts:
        p = wc.project64(rot, trans, dv)
        with np.errstate(all="ignore"):
            q = [((rot[i, 0] * x + rot[i, 1] * y) + rot[i, 2]) * dv + trans[i] for i in range(3)]
            assert all(a.dtype == F32 for a in q)
            ix = ((((q[0] / q[2]) / F32((k.W - 1) / 2) - F32(1)) + F32(1)) * F32(k.W) - F32(1)) / F32(2)
            iy = ((((q[1] / q[2]) / F32((k.H - 1) / 2) - F32(1)) + F32(1)) * F32(k.H) - F32(1)) / F32(2)
            near = (p["ix"] > -2) & (p["ix"] < k.W + 1) & (p["iy"] > -2) & (p["iy"] < k.H + 1)
            err = np.maximum(np.abs(ix - p["ix"]), np.abs(iy - p["iy"]))[near]
        assert err.size and err.max() <= wc.MARGIN_PX / 4, err.max()
    _, raw64, info = wc.reference(k)
    _, raw32 = wc.comparator(k)
    want = np.broadcast_to((info[0]["n_pos"] > 0)[None], raw32.shape)
    assert np.array_equal(raw32 > 0, want) and np.array_equal(raw32 == 0, ~want)
    assert np.array_equal(raw64 > 0, want)


def test_comparator_meets_the_bound():
    """max |comparator - ref64| / max |ref64| over EVERY voxel of every case, variance and raw warp; the GPU bound of a C is 4 x
    the largest figure among its cases, so the comparator meets it with that margin by construction -- what is asserted here is
    that nothing had to be masked for that (all outputs finite, every voxel in), that the figures stay in the range the bound
    was designed for (below 2e-4: a few float32 ulp of sample position times the features' slope), and that the output scale
    is O(1) in every case."""
    for C in (8, 16, 32):
        figs = wc.comparator_figures(C)
        for name, (fv, fr) in figs.items():
            k = wc.BY_NAME[name]
            var, raw = wc.comparator(k)
            rv, rr, _ = wc.reference(k)
            assert np.isfinite(var).all() and np.isfinite(raw).all() and np.isfinite(rv).all() and np.isfinite(rr).all()
            assert var.shape == rv.shape == (k.C, k.D, k.H, k.W)
            assert 0.3 <= np.abs(rv).max() <= 3.0 and 0.3 <= np.abs(rr).max() <= 3.0
            print(f"{name}: comparator {fv:.2e} (variance) {fr:.2e} (raw) of the output scale; bounds {wc.bound(C):.2e} / "
                  f"{wc.bound(C, True):.2e}")
            assert fv <= wc.bound(C) and fr <= wc.bound(C, True)
            assert 0 < fv <= 2e-4 and 0 < fr <= 2e-4
        assert wc.bound(C) == wc.BOUND_FACTOR * max(f[0] for f in figs.values())


def touches(k, mutant):
    n = wc.categories(k)
    if mutant == "z_guard":
        return n["qz_neg_inside"] >= 1
    if mutant == "clamp":
        return n["x0_is_-1"] + n["x1_is_W"] + n["y0_is_-1"] + n["y1_is_H"] + n["two_sided"] + n["outside_near"] >= 1
    return True


@pytest.mark.parametrize("mutant", wc.MUTANTS)
def test_mutants_miss_the_bound(mutant):
    """Each mutant of the reference -- align_corners=True un-normalisation, W/2 instead of (W-1)/2, border clamping, a z guard,
    two corners' weights exchanged, the variance divided by NS -- is at least 100 bounds away from the reference on every case
    whose categories it touches (all cases, but the z guard only where q.z < 0 lands inside)."""
    touched = 0
    for k in wc.CASES:
        if not touches(k, mutant):
            continue
        touched += 1
        rv, rr, _ = wc.reference(k)
        mv, mr, _ = wc.reference(k, mutant)
        fv = wc.figure(mv, rv) / wc.bound(k.C)
        print(f"{k.name} {mutant}: variance at {fv:.0f} bounds", end="")
        assert fv >= wc.MUTANT_FACTOR, (k.name, mutant, fv)
        if mutant != "div_ns" and (mutant != "z_guard" or (_qz_neg_inside_source0(k))):
            fr = wc.figure(mr, rr) / wc.bound(k.C, True)
            print(f", raw warp at {fr:.0f} bounds", end="")
            assert fr >= wc.MUTANT_FACTOR, (k.name, mutant, fr)
        print()
    assert touched >= (10 if mutant == "z_guard" else len(wc.CASES))


def _qz_neg_inside_source0(k):
    info = wc.reference(k)[2][0]
    return int(((info["qz"] < 0) & (info["n_in"] > 0)).sum()) >= 1
