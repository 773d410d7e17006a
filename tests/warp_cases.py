"""TEST INFRASTRUCTURE ONLY -- the float64 reference, the inputs and the case table of tests/test_gpu_warp_edges.py, built here
(numpy on the host, no GPU import) so that tests/test_warp_cases_cpu.py can show without a GPU that the reference is right, that
the table reaches every kernel instance, corner state and tail of the two cost-volume builders, and that the bound of the GPU
test is one that a float32 evaluation of exactly these inputs meets while every mutant of the reference misses it.

Operation: DepthNet.forward step 2 (models/CasMVSNet.py:611-642) and homo_warping alone (:280-315) as csrc/svs_warp_taps.h
defines them (kHalfPixel, no z guard): q = (rot @ [x,y,1]) * depth + trans, p = q.xy / q.z, normalised with the (W-1)/2
formula, sampled bilinearly with align_corners=False and zeros padding.  A negative q.z projects mirrored and IS sampled; a
corner outside, or a coordinate that is not finite, contributes nothing.  rot / trans are the float32 launch arguments;
everything behind them is float64 here.

FEATURES.  Strictly positive and band-limited: 1.5 + a sum of three products of sines of total amplitude <= 1 per channel and
view, so a raw warped value is > 0 exactly where a corner of positive weight is inside.  The angular frequencies lie in
[OMEGA_MIN, OMEGA_MAX] rad/px.  How OMEGA_MAX was chosen: the float32 comparator (oracle/casmvs_oracle.py) differs from this
reference by (a) a sample-position error of a few float32 ulp of the coordinate -- up to ~1e-4 px at |coordinate| ~ 700 px --
times the features' slope, ~ OMEGA * amplitude per px, and (b) ~1e-7 of plain float32 rounding of O(1) values.  Every mutant
that moves a sample (by 0.5 px and more) or exchanges two weights changes the output in proportion to the same slope, so its
distance from the bound does not depend on OMEGA once (a) dominates (b); the mutants that drop or add whole corners (border
clamping, z guard, the divisor) do not depend on it at all.  0.6 rad/px (a period of ~10 px) puts (a) two orders above (b) at
the wide cases, keeps the narrow cases (W < 50, coordinate error ~1e-5 px) at a comparator figure of ~1e-6, and measured here
(tests/test_warp_cases_cpu.py prints it) the comparator stays within 9e-8 ... 9.4e-5 of the output scale over the table
(the largest at W = 677, where a float32 ulp of the coordinate is 6e-5 px)."""
import collections
import functools

import numpy as np

import casmvs_oracle as corc

F32 = np.float32
F64 = np.float64
OMEGA_MIN, OMEGA_MAX = 0.15, 0.6
MARGIN_PX = 2e-3                   # no sample lies this close to a line where a corner enters or leaves the image (see depths)
BOUND_FACTOR = 4.0                 # GPU bound = 4 x the largest comparator figure of the same C (tests/test_gpu_lpips.py's margin)
MUTANT_FACTOR = 100.0              # every mutant misses that bound by this factor at least
KWARP_DZ = 4                       # csrc/svs_costvol.hip: kWarpDz, planes per workgroup of the split producer
F32_TILE = {32: 160, 16: 320, 8: 640}       # warp_variance_kernel: kWarpPasses * 256 / (C / 4) voxels in x
SPLIT_TILE = {32: 160, 16: 128, 8: 128}     # warp_variance_reuse2_kernel<C, NS, 4>: WarpCfg<C, 4>::P * 256 / (C / 4)
PASS_VOXELS = {32: 32, 16: 64, 8: 128}      # voxels per pass over x (both kernels: 256 threads, C / 4 lanes per voxel)
WAVE_VOXELS = {32: 8, 16: 16, 8: 32}        # voxels per wave
MUTANTS = ("align_corners", "norm_w2", "clamp", "z_guard", "swap_weights", "div_ns")

Case = collections.namedtuple("Case", "name C NS D H W kinds jitter")
Case.__doc__ = """kinds: one source-camera recipe per source view (source_camera); jitter: relative per-voxel spread of the
hypotheses around the inverse-depth sweep."""


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def project64(rot, trans, dv, mutant=None):
    """rot (3,3), trans (3,) float32 launch arguments, dv (D,H,W) -> dict of float64 (D,H,W) arrays: q = (qx,qy,qz), the sample
    position (ix, iy) in source pixels (svs_warp_taps.h, kHalfPixel) and `dead` (z guard mutant only)."""
    D, H, W = dv.shape
    R, t, d = np.asarray(rot, F32).astype(F64), np.asarray(trans, F32).astype(F64), np.asarray(dv, F32).astype(F64)
    y, x = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    with np.errstate(all="ignore"):
        qx = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2]) * d + t[0]
        qy = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2]) * d + t[1]
        qz = ((R[2, 0] * x + R[2, 1] * y) + R[2, 2]) * d + t[2]
        px, py = qx / qz, qy / qz
        if mutant == "norm_w2":
            gx, gy = px / (W / 2.0) - 1.0, py / (H / 2.0) - 1.0
        else:
            gx, gy = px / ((W - 1) / 2.0) - 1.0, py / ((H - 1) / 2.0) - 1.0
        if mutant == "align_corners":
            ix, iy = ((gx + 1.0) / 2.0) * (W - 1), ((gy + 1.0) / 2.0) * (H - 1)
        else:
            ix, iy = ((gx + 1.0) * W - 1.0) / 2.0, ((gy + 1.0) * H - 1.0) / 2.0
    dead = ~(qz >= 1e-6) if mutant == "z_guard" else np.zeros(dv.shape, bool)
    return dict(qx=qx, qy=qy, qz=qz, ix=ix, iy=iy, dead=dead)


def corners64(pos, H, W, mutant=None):
    """-> x0, y0 (floor of the position), per corner k = 2 dy + dx: weight w[k], inside[k], integer column / row xi[k], yi[k]
    (0 where outside), all (D,H,W)."""
    ix, iy = pos["ix"], pos["iy"]
    with np.errstate(all="ignore"):
        x0, y0 = np.floor(ix), np.floor(iy)
        tx, ty = ix - x0, iy - y0
    w, inside, xi, yi = [], [], [], []
    for k in range(4):
        dx, dy = k & 1, k >> 1
        with np.errstate(all="ignore"):
            xx, yy = x0 + dx, y0 + dy
            wk = (tx if dx else 1.0 - tx) * (ty if dy else 1.0 - ty)
        if mutant == "clamp":
            ok = np.isfinite(xx) & np.isfinite(yy)
            xx, yy = np.clip(xx, 0, W - 1), np.clip(yy, 0, H - 1)
        else:
            ok = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)          # NaN compares false
        ok &= ~pos["dead"]
        w.append(np.where(ok, wk, 0.0))
        inside.append(ok)
        xi.append(np.where(ok, xx, 0).astype(np.int64))
        yi.append(np.where(ok, yy, 0).astype(np.int64))
    if mutant == "swap_weights":
        w[0], w[1] = w[1], w[0]
        w[0], w[1] = np.where(inside[0], w[0], 0.0), np.where(inside[1], w[1], 0.0)
    return x0, y0, w, inside, xi, yi


def warp64(fea, rot, trans, dv, mutant=None):
    """homo_warping of one source: fea (C,H,W) -> warped (C,D,H,W) float64, the positions (project64), the number of corners
    inside per voxel and the number of those with a positive weight."""
    C, H, W = fea.shape
    f = np.asarray(fea, F32).astype(F64)
    pos = project64(rot, trans, dv, mutant)
    _, _, w, inside, xi, yi = corners64(pos, H, W, mutant)
    out = np.zeros((C,) + dv.shape, F64)
    for k in range(4):
        out += np.where(inside[k][None], w[k][None] * f[:, yi[k], xi[k]], 0.0)
    n_in = sum(m.astype(np.int64) for m in inside)
    n_pos = sum((m & (wk > 0)).astype(np.int64) for m, wk in zip(inside, w))
    return out, pos, n_in, n_pos


def variance64(ref, warped, mutant=None):
    """DepthNet.forward :611-642: ref (C,H,W), warped: list of (C,D,H,W) -> E[v^2] - E[v]^2 over the NS + 1 views."""
    D = warped[0].shape[1]
    s = np.repeat(np.asarray(ref, F32).astype(F64)[:, None], D, 1)
    sq = s * s
    for wv in warped:
        s = s + wv
        sq = sq + wv * wv
    n = float(len(warped)) if mutant == "div_ns" else float(len(warped) + 1)
    return sq / n - (s / n) ** 2


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def source_camera(kind, v, H, W):
    """-> (rot (3,3), trans (3,)) of a source view in float64, before their rounding to float32.  The reference camera is the
    identity pose with focal length 64 and principal point (floor(W/2), floor(H/2)); a source has the same focal length, its
    principal point shifted by +-9 px (a quarter of the side where that is less) and a baseline of 0.5 (v + 1), alternating in sign:
       base  a translation                      turn  a half-turn about y in front of it: q.z < 0 everywhere, samples inside
       skew  q.z = (1 - (x - cx) / 16) depth: exactly 0 in column cx + 16, negative beyond it
       diag  a small translation towards (-1,-1): voxel (0,0) samples around the image's first pixel
       tiny  base with a baseline that keeps a 2 x 2 image in sight"""
    f = 64.0
    crx, cry = float(W // 2), float(H // 2)
    sx, sy = min(9.0, W / 4.0), min(9.0, H / 4.0)
    sgn = -1.0 if v % 2 else 1.0
    Kr = np.array([[f, 0, crx], [0, f, cry], [0, 0, 1]], F64)
    Ks = np.array([[f, 0, crx + sgn * sx], [0, f, cry - sgn * sy], [0, 0, 1]], F64)
    A, b = np.eye(3), np.array([sgn * 0.5 * (v + 1), 0.125 * (v + 1), 0.0])
    if kind == "turn":
        A = np.diag([-1.0, 1.0, -1.0])
    elif kind == "skew":
        A = np.array([[1.0, 0, 0], [0, 1.0, 0], [-4.0, 0, 1.0]])
    elif kind == "diag":
        Ks = Kr
        b = np.array([-1.0 / 32, -(1.0 / 32) * ((H - 1) / H) / ((W - 1) / W), 0.0])
    elif kind == "tiny":
        Ks = np.array([[f, 0, crx + 0.25], [0, f, cry - 0.25], [0, 0, 1]], F64)
        b = np.array([sgn / 64, 1.0 / 128, 0.0])
    else:
        assert kind == "base", kind
    return Ks @ A @ np.linalg.inv(Kr), Ks @ b


def case_projs(k):
    """(NS + 1, 2, 4, 4) float32 projection matrices [extrinsic, intrinsic] whose relative projections are EXACTLY the float32
    roundings of source_camera's: reference = identity, source = [rot | trans] with identity intrinsics, so that the library's
    host arithmetic (costvol.relative_projection, float64) and the comparator's (corc.combine_proj / relative_proj, float32
    products) hand the same twelve floats to the kernels and to this reference."""
    P = np.zeros((k.NS + 1, 2, 4, 4), F32)
    P[:, 0], P[:, 1] = np.eye(4, dtype=F32), np.eye(4, dtype=F32)
    for v, kind in enumerate(k.kinds):
        rot, trans = source_camera(kind, v, k.H, k.W)
        P[v + 1, 0, :3, :3], P[v + 1, 0, :3, 3] = rot.astype(F32), trans.astype(F32)
    return P


def rot_trans(k):
    """the float32 launch arguments, as the comparator forms them: [(rot (3,3), trans (3,))] per source"""
    P = case_projs(k)
    ref = corc.combine_proj(P[0])
    return [corc.relative_proj(corc.combine_proj(P[v + 1]), ref) for v in range(k.NS)]


def features(k):
    """NS + 1 float32 (C,H,W) maps, reference first: 1.5 + sum of three sine products, amplitudes summing to at most 1."""
    rng = np.random.default_rng(1000 + 7 * k.C + k.NS + 31 * k.D)
    y, x = np.meshgrid(np.arange(k.H, dtype=F64), np.arange(k.W, dtype=F64), indexing="ij")
    out = []
    for _ in range(k.NS + 1):
        f = np.full((k.C, k.H, k.W), 1.5)
        amp = rng.uniform(0.2, 1.0, (k.C, 3))
        amp /= np.maximum(amp.sum(1, keepdims=True), 1.0)
        for c in range(k.C):
            for j in range(3):
                wx, wy = rng.uniform(OMEGA_MIN, OMEGA_MAX, 2)
                px, py = rng.uniform(0, 2 * np.pi, 2)
                f[c] += amp[c, j] * np.sin(wx * x + px) * np.sin(wy * y + py)
        out.append(f.astype(F32))
    return out


SPECIALS = (0.0, -5.0, float("inf"), float("nan"), 1e-13, 1e13)       # isolated hypotheses; 1e-13: |q.z| < 2^-40 and a
#                                                                     coordinate beyond 2^31; 1e13: |q.x| >= 2^40, lands inside


def undecided(k, dv, rts):
    """voxels whose sample, for some source, lies within MARGIN_PX of a line ix = -1, ix = W, iy = -1 or iy = H while the other
    coordinate is within reach of the image: there float32 and float64 may disagree on whether a corner is inside"""
    bad = np.zeros(dv.shape, bool)
    for rot, trans in rts:
        p = project64(rot, trans, dv)
        ix, iy = p["ix"], p["iy"]
        with np.errstate(all="ignore"):
            nx = np.minimum(np.abs(ix + 1.0), np.abs(ix - k.W)) < MARGIN_PX
            ny = np.minimum(np.abs(iy + 1.0), np.abs(iy - k.H)) < MARGIN_PX
            bad |= (nx & (iy > -2.0) & (iy < k.H + 1.0)) | (ny & (ix > -2.0) & (ix < k.W + 1.0))
    return bad


@functools.lru_cache(maxsize=None)
def _depths(k):
    rng = np.random.default_rng(77 + 13 * k.C + 5 * k.NS + k.D + k.W)
    rts = rot_trans(k)
    inv = np.linspace(1.0 / 4, 1.0 / 40, k.D) if k.D > 1 else np.array([1.0 / 8])
    dv = (1.0 / (inv[:, None, None] * (1.0 + k.jitter * rng.uniform(-1, 1, (k.D, k.H, k.W))))).astype(F32)
    fixed = np.zeros(dv.shape, bool)
    if "diag" in k.kinds:
        # voxel (0,0), first two planes of every four-plane run: outside (3 px up and left), then cell (-1,-1): only corner 3 is
        # inside, at pixel (0,0), whose byte offset is the `outside' offset 0
        t0 = float(rts[k.kinds.index("diag")][1][0])
        for d in range(0, k.D - 1, KWARP_DZ):
            dv[d, 0, 0], dv[d + 1, 0, 0] = t0 / -3.0, t0 / (-0.2 * (k.W - 1) / k.W)
            fixed[d:d + 2, 0, 0] = True
    n = k.D * k.H * k.W
    if n >= 64:
        free = np.flatnonzero(~fixed.reshape(-1))
        take = rng.choice(free, 2 * len(SPECIALS) if n >= 256 else len(SPECIALS), replace=False)
        dv.reshape(-1)[take] = np.resize(np.array(SPECIALS, F32), take.size)
        fixed.reshape(-1)[take] = True
    for _ in range(40):
        bad = undecided(k, dv, rts) & np.isfinite(dv)
        if not bad.any():
            break
        assert not (bad & fixed).any(), f"{k.name}: a constructed hypothesis is undecided"
        dv[bad] *= F32(1.0 + 0.004 * rng.uniform(1, 2))
    dv.setflags(write=False)
    return dv


def depths(k):
    """(D,H,W) float32 hypotheses: an inverse-depth sweep from 4 to 40 with +-jitter per voxel; the constructed transitions of
    voxel (0,0) where the case has a `diag' source; isolated 0, negative, +inf, NaN, 1e-13 and 1e13; and every ordinary voxel
    whose sample would fall within MARGIN_PX of a line where a corner enters the image moved off it (scaled by < 1 % until
    none is left), so that which corners are inside is decided alike in float32 and float64."""
    return _depths(k)


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
def _c(C, NS, D, H, W, kinds, jitter=0.1):
    assert len(kinds) == NS
    return Case(f"c{C}_ns{NS}_{D}x{H}x{W}", C, NS, D, H, W, tuple(kinds), jitter)


CASES = [
    # C = 32: float32 tile 160, split tile 160, 8 voxels per wave.  170 = 160 + a full wave + 2 voxels of the next
    _c(32, 1, 1, 2, 2, ["tiny"]),
    _c(32, 2, 5, 5, 170, ["base", "skew"]),
    _c(32, 3, 66, 3, 37, ["diag", "base", "turn"], 0.004),
    _c(32, 4, 7, 12, 44, ["base", "turn", "skew", "diag"]),
    # C = 16: float32 tile 320, split tile 128, 16 voxels per wave.  341 = 320 + a full wave + 5
    _c(16, 1, 3, 4, 341, ["skew"]),
    _c(16, 2, 65, 3, 40, ["base", "diag"], 0.004),
    _c(16, 3, 2, 6, 37, ["turn", "diag", "base"]),
    _c(16, 4, 8, 7, 70, ["diag", "skew", "base", "turn"]),
    # C = 8: float32 tile 640, split tile 128, 32 voxels per wave.  677 = 640 + a full wave + 5
    _c(8, 1, 6, 3, 677, ["base"]),
    _c(8, 2, 4, 5, 132, ["diag", "turn"]),
    _c(8, 3, 67, 2, 39, ["base", "skew", "diag"], 0.004),
    _c(8, 4, 9, 6, 131, ["skew", "base", "diag", "turn"]),
]
BY_NAME = {k.name: k for k in CASES}
assert len(BY_NAME) == len(CASES)


def split_volume_bytes(C, D, H, W):
    """svs_split_volume_dims (csrc/svs_split_volume.h): padded (D+2, 4 ceil(H/4) + 2, 2 pieces, C/8, 32 ceil(W/32) + 4) 16-byte units"""
    return (D + 2) * (4 * ((H + 3) // 4) + 2) * 2 * (C // 8) * (32 * ((W + 31) // 32) + 4) * 16


@functools.lru_cache(maxsize=None)
def _reference(k, mutant):
    feats, rts, dv = features(k), rot_trans(k), depths(k)
    warped, info = [], []
    for v, (rot, trans) in enumerate(rts):
        w, pos, n_in, n_pos = warp64(feats[v + 1], rot, trans, dv, mutant)
        warped.append(w)
        info.append(dict(pos, n_in=n_in, n_pos=n_pos))
    var = variance64(feats[0], warped, mutant)
    for a in (var, warped[0]):
        a.setflags(write=False)
    return var, warped[0], info


def reference(k, mutant=None):
    """-> variance (C,D,H,W) float64, the raw warp of source 0 (C,D,H,W) float64, and per source a dict with the float64 q,
    sample position, corners inside (n_in) and corners inside with positive weight (n_pos).  Computed once per case."""
    return _reference(k, mutant)


@functools.lru_cache(maxsize=None)
def _comparator(k):
    feats, P, dv = features(k), case_projs(k), depths(k)
    with np.errstate(all="ignore"):                      # the isolated hypotheses: inf - inf, 0 * inf
        var = corc.variance_volume(feats, list(P), np.asarray(dv))
        raw = corc.homo_warp(feats[1], corc.combine_proj(P[1]), corc.combine_proj(P[0]), np.asarray(dv))
    return var, raw


def comparator(k):
    """the oracle's float32 numpy evaluation of the same inputs -> variance, raw warp of source 0"""
    return _comparator(k)


def figure(got, ref):
    """max |got - ref| / max |ref| over every voxel"""
    return float(np.abs(np.asarray(got, F64) - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def comparator_figures(C):
    """{case name: (variance figure, raw figure)} of the cases with C channels"""
    out = {}
    for k in CASES:
        if k.C == C:
            var, raw = comparator(k)
            rv, rr, _ = reference(k)
            out[k.name] = (figure(var, rv), figure(raw, rr))
    return out


def bound(C, raw=False):
    """the GPU bound of the cases with C channels, relative to each case's output scale: BOUND_FACTOR x the largest comparator
    figure among them (the kernels contract and pair their multiplies differently from numpy: each gets a few ulp of sample
    position)"""
    return BOUND_FACTOR * max(f[1 if raw else 0] for f in comparator_figures(C).values())


# ---------------------------------------------------------------------------------------------------------------------
# categories, counted from the float64 positions
# ---------------------------------------------------------------------------------------------------------------------
def offsets(k, info):
    """the corner offsets the kernels keep per (voxel, source), in pixels (y * W + x, 0 where outside): (4,D,H,W)"""
    _, _, _, inside, xi, yi = corners64(info, k.H, k.W)
    return np.stack([np.where(m, y * k.W + x, 0) for m, x, y in zip(inside, xi, yi)])


def categories(k):
    """-> Counter of what the case reaches, summed over its sources (see tests/test_warp_cases_cpu.py for the list)"""
    _, _, infos = reference(k)
    dv = depths(k)
    H, W, D = k.H, k.W, k.D
    n = collections.Counter()
    n["hyp_zero"], n["hyp_neg"] = int((dv == 0).sum()), int((dv < 0).sum())
    n["hyp_inf"], n["hyp_nan"] = int(np.isposinf(dv).sum()), int(np.isnan(dv).sum())
    vw = WAVE_VOXELS[k.C]
    for info in infos:
        ix, iy, qz, n_in = info["ix"], info["iy"], info["qz"], info["n_in"]
        with np.errstate(all="ignore"):
            x0, y0 = np.floor(ix), np.floor(iy)
            fin = np.isfinite(ix) & np.isfinite(iy)
            xin, yin = (x0 >= 0) & (x0 <= W - 2), (y0 >= 0) & (y0 <= H - 2)
            n["all_in"] += int((n_in == 4).sum())
            n["x0_is_-1"] += int(((x0 == -1) & yin).sum())
            n["x1_is_W"] += int(((x0 == W - 1) & yin).sum())
            n["y0_is_-1"] += int(((y0 == -1) & xin).sum())
            n["y1_is_H"] += int(((y0 == H - 1) & xin).sum())
            n["two_sided"] += int((((x0 == -1) | (x0 == W - 1)) & ((y0 == -1) | (y0 == H - 1))).sum())
            dist = np.maximum(np.maximum(-1 - ix, ix - W), np.maximum(-1 - iy, iy - H))
            n["outside_near"] += int((fin & (n_in == 0) & (dist <= 8)).sum())
            n["outside_2^31"] += int((fin & ((np.abs(ix) > 2.0 ** 31) | (np.abs(iy) > 2.0 ** 31))).sum())
            n["qz_neg_inside"] += int(((qz < 0) & (n_in > 0)).sum())
            n["qz_zero"] += int((qz == 0).sum())
            n["qz_sign_rows"] += int(((qz < 0).any(2) & (qz > 0).any(2)).sum())
            n["div_small_qz"] += int(((np.abs(qz) < 2.0 ** -40) & (qz != 0)).sum())
            big = (np.abs(info["qx"]) >= 2.0 ** 40) | (np.abs(info["qy"]) >= 2.0 ** 40)
            n["div_big_q"] += int((big & np.isfinite(info["qx"]) & np.isfinite(qz)).sum())
            n["div_big_q_inside"] += int((big & (n_in > 0)).sum())
        off = offsets(k, info)
        for d in range(D - 1):
            if d % KWARP_DZ == KWARP_DZ - 1:
                continue                                  # the next plane starts a new run: everything is fetched anyway
            a_in, b_in = n_in[d] > 0, n_in[d + 1] > 0
            with np.errstate(all="ignore"):
                step = np.maximum(np.abs(x0[d + 1] - x0[d]), np.abs(y0[d + 1] - y0[d]))
            both = a_in & b_in
            n["step_0"] += int((both & (step == 0)).sum())
            n["step_1"] += int((both & (step == 1)).sum())
            n["step_more"] += int((both & (step > 1)).sum())
            n["in_to_out"] += int((a_in & ~b_in).sum())
            n["out_to_in"] += int((~a_in & b_in).sum())
            n["enter_at_00"] += int((~a_in & (x0[d + 1] == -1) & (y0[d + 1] == -1)).sum())
            moved = (off[:, d] != off[:, d + 1]).any(0)                      # (H,W)
            pad = (-W) % vw
            mv = np.pad(moved, ((0, 0), (0, pad))).reshape(H, -1, vw)        # lanes beyond W never move
            some, every = mv.any(2), np.pad(moved, ((0, 0), (0, pad)), constant_values=True).reshape(H, -1, vw).all(2)
            n["wave_none_moves"] += int((~some).sum())
            n["wave_some_move"] += int((some & ~every).sum())
    return n


def tails(k):
    """what the case's shape reaches in the launch geometry of the two kernels"""
    vw, vp = WAVE_VOXELS[k.C], PASS_VOXELS[k.C]
    t = set()
    t.add(f"D%4={k.D % 4}")
    if k.D <= 3:
        t.add(f"D={k.D}")
    if k.D >= 64 and k.D % 4:
        t.add("D>=64,D%4!=0")
    if k.W > F32_TILE[k.C]:
        t.add("two_f32_tiles")
    if k.W > SPLIT_TILE[k.C]:
        t.add("two_split_tiles")
    for tile, tag in ((F32_TILE[k.C], "f32"), (SPLIT_TILE[k.C], "split")):
        xt = (k.W - 1) // tile * tile                                           # the last tile
        for p0 in range(xt, xt + tile, vp):                                     # its passes
            fill = [min(max(k.W - x, 0), vw) for x in range(p0, p0 + vp, vw)]   # voxels inside, per wave
            if vw in fill and 0 in fill and any(0 < f < vw for f in fill):
                t.add(f"full_part_empty_{tag}")
    t.add("W%4==0" if k.W % 4 == 0 else "W%4!=0")
    if k.H == 2 and k.W == 2:
        t.add("H=W=2")
    return t
