"""The case table of the cloud normals (tests/normals_cases.py) is sound and sharp -- no GPU work here.

Sound: the float64 oracle (cloudclean_oracle.normals, np.linalg.eigh) alone meets every bound of the criterion on every case,
every point with m >= 3 included, and so does the kernel restated in its operation order.  Each case is what it claims: the
rungs' spectra, the exact spectra and ties, the numbers of points per set, the zero dot product, the equal distances.
Sharp: every mutant of the restated kernel misses a bound on some case."""
import fractions

import numpy as np
import pytest

import cloudclean_oracle as co
import normals_cases as nc


def restated(c, **kw):
    return nc.kernel_normals(c["pts"], c["idx"], c["include_self"], c["view_index"], c["centres"], **kw)


@pytest.mark.parametrize("name", nc.ALL)
def test_oracle_and_restated_kernel_meet_the_criterion(name):
    c = nc.case(name)
    want_n, want_c = c["oracle"][:2]
    f, bad = nc.all_failures(c, want_n, want_c)
    assert not bad, (bad, nc.summary(f))
    assert np.array_equal(f["live"], c["m"] >= 3)                        # no escape: every such point is in the figures
    assert not want_n[~f["live"]].any() and not want_c[~f["live"]].any()
    f, bad = nc.all_failures(c, *restated(c))
    assert not bad, (bad, nc.summary(f))


def test_every_family_has_points_to_judge():
    for family, names in nc.NAMES.items():
        live = {name: int((nc.case(name)["m"] >= 3).sum()) for name in names}
        none = {"slots-k2_noself", "count-1"}                              # by construction: m < 3 everywhere
        assert all((live[name] == 0) == (name in none) for name in names), live
    assert set(nc.SCALES) == {"unit", "dtu", "small", "far"} and nc.COUNTS == (1, 255, 256, 257, 513)
    assert nc.SCALES["dtu"] == (100.0, (-250.0, 410.0, 630.0)) and nc.SCALES["small"] == (2.0 ** -10, (0.37, -0.12, 0.05))
    assert nc.SCALES["far"] == (1.0, (1e6, -1e6, 1e6))


# ---- scan scale ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.NAMES["scan"])
def test_scan_cases_are_the_unit_cloud_moved(name):
    c, base = nc.case(name), nc.case(nc.case(name)["base"])
    assert np.array_equal(c["idx"], base["idx"]) and (c["m"] == nc.K + 1).all()       # the same neighbours in the same order
    s = c["s"]
    spacing = np.linalg.norm(c["pts"][c["idx"][:, 0]] - c["pts"], axis=1)
    offset = np.linalg.norm(c["pts"].mean(0))
    print(f"{name}: |centre| {offset:.3g}, nearest neighbour {np.median(spacing):.3g}")
    if name.endswith("dtu"):
        assert offset > 500 and np.median(spacing) < 10
    if name.endswith("small"):
        assert np.median(spacing) < 1e-4
    if name.endswith("far"):
        assert offset > 1e6 and np.median(spacing) < 0.1
    # the oracle on the moved cloud gives the unit cloud's normals and curvatures
    clear = (base["lam"][:, 1] - base["lam"][:, 0]) >= nc.CLEAR * base["lam"][:, 2]
    assert clear.mean() >= 0.95
    assert (co.angle(c["oracle"][0], base["oracle"][0], signed=True)[clear] <= nc.ANGLE).all()
    assert (np.abs(c["oracle"][1] - base["oracle"][1]) <= nc.CURVATURE).all()
    assert np.allclose(c["lam"], s * s * base["lam"], rtol=1e-6, atol=1e-9 * s * s * base["lam"][:, 2].max())


# ---- anisotropy ladder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.NAMES["ladder"])
def test_ladder_rungs_have_the_requested_spectra(name):
    c = nc.case(name)
    r1, r0 = c["ratios"]
    lam = c["lam"]
    assert len(c["pts"]) == 64 * 17 and (c["m"] == 17).all()
    lo, hi = min(r1, r0), max(r1, r0)
    assert ((lam[:, 0] / lam[:, 2] > lo / 2) & (lam[:, 0] / lam[:, 2] < lo * 2)).all()
    assert ((lam[:, 1] / lam[:, 2] > hi / 2) & (lam[:, 1] / lam[:, 2] < hi * 2)).all()
    # the gaps the rung is about, each within a factor 2 as well: the near-ties are resolved, not rounded away
    for a, b, want in ((0, 1, hi - lo), (1, 2, 1.0 - hi)):
        if want > 0:
            gap = (lam[:, b] - lam[:, a]) / lam[:, 2]
            assert ((gap > want / 2) & (gap < want * 2)).all(), (name, a, b, want, gap.min(), gap.max())
    # 64 rotations of their own: the smallest eigenvector points everywhere
    first = c["oracle"][0][::17]
    assert (np.abs(first @ first.T) < 0.99).sum() >= 64 * 60 and (np.abs(first).max(1) < 0.9999).all()
    # every point of a block sees the same 17 points in another order
    sets = nc.neighbour_sets(c["pts"], c["idx"], True)
    assert all(sorted(sets[i]) == list(range(i - i % 17, i - i % 17 + 17)) and sets[i][0] == i for i in range(len(sets)))


def test_ladder_reaches_the_unclear_spectra():
    clear = {name: float(((nc.case(name)["lam"][:, 1] - nc.case(name)["lam"][:, 0]) >= nc.CLEAR * nc.case(name)["lam"][:, 2]).mean())
             for name in nc.NAMES["ladder"]}
    assert clear == {"ladder-plane": 1.0, "ladder-sharp_plane": 1.0, "ladder-needle": 0.0, "ladder-needle_tie": 0.0,
                     "ladder-ball": 0.0}


# ---- exact degeneracies ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.NAMES["exact"])
def test_exact_cases_have_exactly_the_stated_spectrum(name):
    c = nc.case(name)
    assert (c["m"] == len(c["pts"])).all() and (c["pts"] == np.round(c["pts"] * 8) / 8).all()      # small dyadic coordinates
    if c["spectrum"] is None:
        # the tilted lattice: coplanar in exact arithmetic (rational determinant 0, rank 2), not diagonal, and the kernel's
        # arithmetic leaves its smallest eigenvalue BELOW zero: the clamp is reached
        F = [[fractions.Fraction(v) for v in p] for p in c["pts"].tolist()]
        mean = [sum(p[a] for p in F) / len(F) for a in range(3)]
        cov = [[sum((p[a] - mean[a]) * (p[b] - mean[b]) for p in F) / len(F) for b in range(3)] for a in range(3)]
        det = (cov[0][0] * (cov[1][1] * cov[2][2] - cov[1][2] * cov[2][1]) - cov[0][1] * (cov[1][0] * cov[2][2] - cov[1][2] * cov[2][0])
               + cov[0][2] * (cov[1][0] * cov[2][1] - cov[1][1] * cov[2][0]))
        assert det == 0 and cov[0][0] * cov[1][1] - cov[0][1] ** 2 != 0 and all(cov[a][b] != 0 for a in range(3) for b in range(3))
        raw = restated(c, raw=True)[2]
        assert (raw["lmin"] < 0).any() and (raw["trace"] > 0).all()
        assert (np.abs(co.angle(c["oracle"][0], np.tile([1.0, 2.0, -1.0], (len(F), 1)))) < 1e-12).all()
        return
    for C in c["C"]:
        assert not (C - np.diag(np.diag(C))).any()                       # diagonal as summed: no rotation runs
        assert np.array_equal(np.sort(np.diag(C)), np.array(c["spectrum"]))                  # ties exact in float64
    assert np.array_equal(c["lam"], np.tile(c["spectrum"], (len(c["pts"]), 1)))
    # the stated normal is the lowest axis of the smallest diagonal entry, positive
    d = np.diag(c["C"][0])
    assert np.array_equal(c["expect"][0], np.eye(3)[int(np.argmin(d))]) and np.array_equal(c["oracle"][0], c["expect"])
    ties = {"exact-collinear_x": (1, 2), "exact-collinear_z": (0, 1), "exact-star111": (0, 1, 2), "exact-star211": (1, 2),
            "exact-star112": (0, 1), "exact-star121": (0, 2), "exact-coincident": (0, 1, 2), "exact-lattice331": (2,)}[name]
    assert tuple(np.flatnonzero(d == d.min())) == ties
    if name == "exact-coincident":
        raw = restated(c, raw=True)[2]
        assert not c["C"].any() and not raw["trace"].any()               # trace == 0: the curvature's other branch


# ---- slots ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.NAMES["slots"])
def test_slot_cases_hold_what_they_claim(name):
    c = nc.case(name)
    n, idx = len(c["pts"]), c["idx"]
    assert set(c["m"].tolist()) == c["m_values"]
    assert idx.shape[1] == {"k2": 2, "k3": 3, "k32": 32}[name.split("-")[1].split("_")[0]]
    assert c["include_self"] == name.endswith("_self")
    valid = (idx >= 0) & (idx < n)
    assert np.array_equal(c["m"], valid.sum(1) + int(c["include_self"]))
    if name != "slots-k2_noself":
        assert (idx >= n).any() and (idx < 0).any()                      # both kinds of slot the kernel skips
    if name.startswith("slots-k32"):
        assert (idx == 2 ** 31 - 1).any()
        late = valid.any(1) & ~valid[:, :28].any(1)
        between = (valid[:, 0:-2] & ~valid[:, 1:-1] & valid[:, 2:]).any(1) | (valid[:, 0:-3] & ~valid[:, 1:-2] & ~valid[:, 2:-1] & valid[:, 3:]).any(1)
        assert late.sum() >= 8 and between.sum() >= 8 and (valid.sum(1) == 32).sum() >= 8 and (valid.sum(1) == 0).sum() >= 8
    # m == 3 exactly, reached with and without the point itself
    assert ((c["m"] == 3).sum() >= 8) == (name in ("slots-k2_self", "slots-k3_noself", "slots-k32_self"))


# ---- facing --------------------------------------------------------------------------------------------------------------------
def test_facing_cases_hold_what_they_claim():
    c = nc.case("facing-view_clamp")
    assert (c["view_index"] < 0).sum() > 30 and (c["view_index"] >= len(c["centres"])).sum() > 30
    moved = dict(c, view_index=c["clamped"])
    assert np.array_equal(co.normals(c["pts"], c["idx"], True, c["clamped"], c["centres"])[0], c["oracle"][0])
    assert np.array_equal(restated(moved)[0], restated(c)[0])
    plain = co.normals(c["pts"], c["idx"], True)[0]
    assert 0.1 < ((plain * c["oracle"][0]).sum(1) < 0).mean() < 0.9      # the rule flips some normals and leaves others
    for name in ("facing-tangent", "facing-tangent_by_view"):
        t = nc.case(name)
        assert not restated(t, raw=True)[2]["dot"].any() and not t["oracle"][3].any()       # dot == 0 exactly, every row
    for name, sign in (("facing-below", -1), ("facing-above", 1)):
        t = nc.case(name)
        assert (np.sign(restated(t, raw=True)[2]["dot"]) == sign).all()
    for name in ("facing-nearest_tie_down", "facing-nearest_tie_up"):
        t = nc.case(name)
        d2 = ((t["pts"][:, None] - t["centres"][None]) ** 2).sum(-1)
        assert (d2[:, 0] == d2[:, 1]).all() and t["view_index"] is None
        assert (np.sign(t["expect"][:, 2]) == np.sign(t["centres"][0, 2])).all()                # the first centre wins


def test_counts_straddle_the_block():
    for n in nc.COUNTS:
        c = nc.case(f"count-{n}")
        assert len(c["pts"]) == n and np.linalg.norm(c["pts"].mean(0)) > 500 * (n > 1)
    assert [n % 256 for n in nc.COUNTS] == [1, 255, 0, 1, 1] and [-(-n // 256) for n in nc.COUNTS] == [1, 1, 1, 2, 3]


# ---- sharp ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def caught():
    """mutant -> {case: what it misses there}"""
    table = {}
    for mut in nc.MUTANTS:
        table[mut] = {}
        for name in nc.ALL:
            c = nc.case(name)
            bad = nc.all_failures(c, *restated(c, mut={mut}))[1]
            if bad:
                table[mut][name] = bad
    return table


@pytest.mark.parametrize("mut", nc.MUTANTS)
def test_every_mutant_misses_a_bound(caught, mut):
    print(mut, {name: bad for name, bad in caught[mut].items()})
    assert caught[mut]
    families = {name.split("-")[0] for name in caught[mut]}
    want = {"sweeps2": {"scan", "count", "slots", "exact", "facing"}, "pick_lt": {"exact"}, "no_clamp": {"exact", "slots"},
            "first_centroid": {"scan", "ladder", "exact", "slots", "count", "facing"}, "dot_le": {"facing"},
            "nearest_le": {"facing"}}[mut]
    assert families == want
    if mut == "pick_lt":                                     # l1 == l2 < l0: the mutant takes column 0, the LARGEST eigenvalue
        assert set(caught[mut]) == {"exact-collinear_x", "exact-star211"}
    if mut == "no_clamp":                                    # seen only through the sign of the curvature
        assert all(bad == ["negative curvature"] for bad in caught[mut].values())
    if mut in ("dot_le", "nearest_le"):
        assert all("expected normal" in bad for bad in caught[mut].values())


# ---- the oracle's own rules ------------------------------------------------------------------------------------------------------
def test_oracle_skips_and_clamps_as_the_header_states():
    pts = co.random_cloud(12, 4)
    idx = np.array([[(i + 1) % 12, (i + 5) % 12, (i + 7) % 12] for i in range(12)])
    wide = np.concatenate([idx[:, :1], np.full((12, 1), 12), idx[:, 1:2], np.full((12, 1), -1), idx[:, 2:], np.full((12, 1), 2 ** 31 - 1)], 1)
    a, b = co.normals(pts, idx, True), co.normals(pts, wide, True)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    view = np.array([-1, 0, 1, 2, 5, -9, 1, 1, 0, 2, 2, 100])
    a = co.normals(pts, idx, True, view, nc.CENTRES)
    b = co.normals(pts, idx, True, np.clip(view, 0, 2), nc.CENTRES)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
