"""The depth-fusion case table (tests/fusion_cases.py) is sound and sharp -- no GPU work here.

Sound: the ordered oracle (the kernel's operation order, no BLAS) equals the float64 oracle (oracle/fusion_oracle.py, numpy
matmul) in every element of every general-camera case, and no (pixel, source) entry of any case sits in the threshold band
(dist within 2 float64 ulp of filter_dist, rel within 1 float32 ulp of filter_diff) except in the manufactured ties -- the
condition under which tests/test_gpu_fusion_exact.py may demand equality from the GPU.
Sharp: every branch of the sampler and of the filter is reached (counted below), and each mutant of the ordered oracle
changes at least one output element of the table."""
import numpy as np
import pytest

import fusion_cases as fc
import fusion_oracle as forc

F32 = np.float32
GENERAL = [c["name"] for c in fc.table() if c["group"] == "general"]
REMAP = [c["name"] for c in fc.table() if c["group"] == "remap"]


@pytest.mark.parametrize("name", GENERAL)
def test_ordered_oracle_equals_float64_oracle(name):
    c = fc.case(name)
    want, kw = c["want"], c["kw"]
    fd, fr = kw.get("filter_dist", 1), kw.get("filter_diff", 0.01)
    assert not fc.threshold_band(want, fd, fr).any()                     # hence: agreement in EVERY element
    ref = c["ref"]
    for v, s in enumerate(c["srcs"]):
        m, d, x, y = forc.check_geometric_consistency(ref["depth"], ref["K"], ref["E"], s["depth"], s["K"], s["E"], fd, fr)
        assert fc.same(m.astype(np.uint8), want["src_mask"][v]), (name, v)
        assert fc.same(d, want["src_depth_reproj"][v]), (name, v)
        assert fc.same(x, want["src_x"][v]) and fc.same(y, want["src_y"][v]), (name, v)
    f = forc.fuse_view(ref, c["srcs"], **kw)
    assert fc.same(f["depth_avg"], want["depth_avg"])
    for k in ("photo_mask", "geo_mask", "final_mask"):
        assert fc.same(f[k].astype(np.uint8), want[k]), k
    assert fc.same(f["xyz"], want["xyz"]) and fc.same(f["rgb"], want["rgb"])


def test_ordered_oracle_equals_the_reference_fixture(golden_dir):
    """fusion_geo.npz (the reference's own check_geometric_consistency, see tests/test_fusion_cpu.py): no entry in the band,
    every element equal -- so the GPU drop-in is held to equality on it (tests/test_gpu_fusion.py)."""
    import os
    import synth
    g = dict(np.load(os.path.join(golden_dir, "fusion_geo.npz")))
    views = synth.make_fusion_views(int(g["seed"]), hw=tuple(int(v) for v in g["hw"]), n_views=3)
    tags = [key[:-5] for key in g if key.endswith("/mask")]
    assert len(tags) == 8
    for tag in tags:
        ref, src = int(tag[1]), int(tag[3])
        fd, fr = (float(v) for v in tag.split("_")[1:])
        w = fc.ordered_fuse_view(dict(views[ref]), [views[src]], filter_dist=fd, filter_diff=fr)
        assert not fc.threshold_band(w, fd, fr).any(), tag
        assert fc.same(w["src_mask"][0] != 0, g[tag + "/mask"].astype(bool)) and fc.same(w["src_depth_reproj"][0], g[tag + "/depth"])
        assert fc.same(w["src_x"][0], g[tag + "/x"]) and fc.same(w["src_y"][0], g[tag + "/y"]), tag


def test_threshold_band_is_empty_except_in_the_ties():
    for c in fc.table():
        n = int(fc.threshold_band(c["want"], c["raw"]["filter_dist"], c["raw"]["filter_diff"]).sum())
        if c["group"] == "tie":
            assert n == (0 if c["name"] == "rel-tie-accepted" else 2 if c["name"] == "zero-ref" else 15), (c["name"], n)
        else:
            assert n == 0, (c["name"], n)


def test_ties_fall_on_the_side_the_strict_comparison_puts_them():
    t = {c["name"]: c["want"] for c in fc.table() if c["group"] == "tie"}
    assert (t["dist-tie-rejected"]["dist"] == 1.0).all() and (t["dist-tie-accepted"]["dist"] == 1.0).all()
    assert not t["dist-tie-rejected"]["src_mask"].any() and t["dist-tie-accepted"]["src_mask"].all()
    assert (t["rel-tie-rejected"]["rel"] == F32(0.25)).all() and not t["rel-tie-rejected"]["src_mask"].any()
    assert (t["rel-tie-accepted"]["rel"] == F32(0.25) - F32(2.0 ** -23)).all() and t["rel-tie-accepted"]["src_mask"].all()
    assert (t["dist-tie-accepted"]["xyz"].shape, t["dist-tie-rejected"]["xyz"].shape) == ((15, 3), (0, 3))


def test_pair_matrices_equal_the_oracles_bit_for_bit():
    from svs_hip import fusion
    n = 0
    for c in fc.table():
        if "ref" not in c:
            continue
        for v, s in enumerate(c["srcs"]):
            got = fusion.pair_matrices(c["ref"]["K"], c["ref"]["E"], s["K"], s["E"])
            assert got.dtype == np.float64 and got.tobytes() == c["raw"]["mats"][v].tobytes(), (c["name"], v)
            n += 1
    assert n > 300


def test_remap_probes_hand_the_sampler_exact_coordinates():
    """In the probes inv(K_src) is exact in float32, src_x = x + sx and src_y = y + sy exactly, and the reprojected depth is
    the sample itself bit for bit wherever the sample is finite and nonzero (a zero, inf or NaN sample is rejected: 0)."""
    n_kept = 0
    for name in REMAP:
        c = fc.case(name)
        want = c["want"]
        H, W = c["raw"]["ref_depth"].shape
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        for v, (sx, sy) in enumerate(c["shifts"]):
            if np.isnan(sx):
                assert np.isnan(want["src_x"][v]).all() and not want["src_mask"][v].any()
                continue
            assert np.array_equal(c["raw"]["mats"][v][34:43].reshape(3, 3), [[1, 0, -sx], [0, 1, -sy], [0, 0, 1]])
            assert np.array_equal(want["src_x"][v], (xx + np.float64(sx)).astype(F32))
            assert np.array_equal(want["src_y"][v], (yy + np.float64(sy)).astype(F32))
            ds = forc.remap_linear(c["srcs"][v]["depth"], want["src_x"][v], want["src_y"][v])
            assert fc.same(ds, want["ds"][v])
            live = np.isfinite(ds) & (ds != 0)
            assert np.array_equal(want["src_mask"][v] != 0, live)
            assert np.array_equal(want["src_depth_reproj"][v], np.where(live, ds, F32(0)))
            n_kept += int(live.sum())
    assert n_kept > 30000


def _all_samples():
    for c in fc.table():
        for v, src in enumerate(c["raw"]["src_depths"]):
            yield c, v, src, c["want"]["src_x"][v], c["want"]["src_y"][v]


def test_remap_variant_without_mutants_is_the_oracles_sampler():
    for c, v, src, x, y in _all_samples():
        assert fc.same(fc.remap_variant(src, x, y), forc.remap_linear(src, x, y)), (c["name"], v)


def test_every_branch_is_reached():
    """Counted over the samples the table hands to the sampler, and over the filter's inputs."""
    n = dict(bad=0, saturated=0, neg_fixed=0, tie_up_x=0, tie_down_x=0, tie_up_y=0, tie_down_y=0, neg_tie_up=0, neg_tie_down=0)
    only_inside, outside_weighted = [0] * 4, [0] * 4
    for c, v, src, x, y in _all_samples():
        H, W = src.shape
        p = fc.remap_parts(H, W, x, y)
        good = ~p["bad"]
        n["bad"] += int(p["bad"].sum())
        n["saturated"] += int((good & ((p["ix"] != p["cx"]) | (p["iy"] != p["cy"]))).sum())
        n["neg_fixed"] += int((good & (((p["sx"] < 0) & (p["sx"] & 31 != 0)) | ((p["sy"] < 0) & (p["sy"] & 31 != 0)))).sum())
        with np.errstate(all="ignore"):
            for ax, m, s in (("x", x, p["sx"]), ("y", y, p["sy"])):
                f = (np.asarray(m, F32) * F32(32)).astype(np.float64)
                tie = good & (np.abs(f - np.floor(f) - 0.5) == 0)
                n["tie_up_" + ax] += int((tie & (s > f)).sum())
                n["tie_down_" + ax] += int((tie & (s < f)).sum())
                n["neg_tie_up"] += int((tie & (f < 0) & (s > f)).sum())
                n["neg_tie_down"] += int((tie & (f < 0) & (s < f)).sum())
        ins = p["inside"] & good
        wpos = [np.ones(x.shape, bool), p["sx"] & 31 != 0, p["sy"] & 31 != 0, (p["sx"] & 31 != 0) & (p["sy"] & 31 != 0)]
        for t in range(4):
            others = np.any([ins[u] for u in range(4) if u != t], axis=0)
            only_inside[t] += int((ins[t] & ~others & wpos[t]).sum())               # this tap alone carries the sample
            outside_weighted[t] += int((good & ~ins[t] & others & wpos[t]).sum())   # this tap reads the border, others the image
    assert all(k > 0 for k in n.values()), n
    # (a tap cannot be the ONLY one outside: the inside taps of a 2x2 footprint form a product of column and row sets)
    assert all(k > 0 for k in only_inside) and all(k > 0 for k in outside_weighted), (only_inside, outside_weighted)

    general = [c for c in fc.table() if c["group"] == "general"]
    assert sum(int((c["want"]["kz"] <= 0).sum()) for c in general) > 100                     # behind a source camera
    zero_over_zero = sum(int(((c["want"]["drep_raw"] == 0) & (c["raw"]["ref_depth"] == 0)[None]).sum()) for c in fc.table())
    assert zero_over_zero >= 2
    for special in (lambda d: d == 0, lambda d: d < 0, np.isinf, np.isnan):
        assert any(special(c["raw"]["ref_depth"]).any() for c in general)
        assert any(special(s).any() for c in fc.table() if c["group"] == "remap" for s in c["raw"]["src_depths"])
    assert any(((s != 0) & (np.abs(s) < np.finfo(F32).tiny)).any() for c in fc.table() for s in c["raw"]["src_depths"])
    for slot in range(16):                                                                  # every source slot accepts somewhere
        assert any(len(c["raw"]["src_depths"]) == 16 and c["want"]["src_mask"][slot].any() for c in fc.table()), slot
    assert {len(c["raw"]["src_depths"]) for c in general} >= {0, 1, 16}
    assert {c["raw"]["thres_view"] for c in general if len(c["raw"]["src_depths"]) == 2} >= {0, 1, 2, 3}
    tie = [c for c in general if (c["raw"]["confidence"] == F32(c["raw"]["conf"])).any()]
    assert tie and any(c["raw"]["extra_mask"] is not None for c in general)
    # three or more sources accepted at one pixel (the float32 sum's order shows), and the scan's block edges
    assert max(int(c["want"]["src_mask"].sum(0).max()) for c in general if len(c["raw"]["src_depths"])) >= 8
    pts = [c for c in fc.table() if c["group"] == "points"]
    assert {c["raw"]["ref_depth"].size for c in pts} == {1, 255, 256, 257, 4097}
    counts = {(c["raw"]["ref_depth"].size, len(c["want"]["xyz"])) for c in pts}
    assert {(4097, 0), (4097, 4097), (4097, 1), (1, 0), (1, 1), (256, 256), (257, 257), (255, 255)} <= counts
    big = fc.case("points-17x241-all")
    v255 = big["raw"]["img"].astype(np.float64).reshape(-1) * 255
    exact = np.abs(v255 - np.rint(v255)) < 1e-4
    assert set(np.rint(v255[exact]).astype(int)) == set(range(256))                          # every code k / 255 ...
    assert np.array_equal(big["want"]["rgb"].reshape(-1)[exact], np.rint(v255[exact]))       # ... comes back as k
    assert np.array_equal(big["want"]["rgb"].reshape(-1), np.floor(v255 + 1e-4))             # the rest truncate
    assert int((np.rint(v255) > np.floor(v255 + 1e-4)).sum()) > 4000                         # where rounding would go up
    assert big["raw"]["img"].min() >= 0 and big["raw"]["img"].max() <= 1


@pytest.mark.parametrize("mut", fc.MUTANTS)
def test_each_mutant_changes_an_output_of_the_table(mut):
    hit = []
    for c in fc.table():
        got = fc.ordered_fuse_mats(mut={mut}, **c["raw"])
        if any(k in c["want"] and not fc.same(got[k], c["want"][k]) for k in fc.OUTPUTS):
            hit.append(c["name"])
    print(f"{mut}: {len(hit)} cases change, e.g. {hit[:4]}")
    assert hit, mut
