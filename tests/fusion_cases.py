"""TEST INFRASTRUCTURE ONLY -- the ordered oracle of the depth-fusion unit (csrc/svs_fusion.hip) and its case table.

`ordered_fuse_view` / `ordered_fuse_mats` restate `fuse_view_kernel` and `fuse_points_kernel` in numpy IN THE KERNEL'S
OPERATION ORDER: the six matrices per source formed in float32 and widened, every dot product written out term by term
and summed left to right (no BLAS), `fusion_oracle.remap_linear` for the sample, the reprojected depths summed in float32
in view order and divided in float64.  The unit is compiled with -ffp-contract=off and holds only IEEE float64 / float32
operations, so the GPU must give these numbers bit for bit (tests/test_gpu_fusion_exact.py); tests/test_fusion_cases_cpu.py
shows that the restatement equals the float64 oracle (oracle/fusion_oracle.py, numpy matmul) on every general-camera case,
that no case of the table has a quantity within rounding of a threshold (the *threshold band*; the manufactured ties
excepted), that the table reaches every branch, and that every mutant below changes an output of the table.

Mutants (argument `mut`, a set of names; the empty set is the kernel):
  round_away     cvRound as half-away-from-zero instead of half-to-even
  trunc_shift    sx / 32 truncated toward zero instead of the arithmetic shift sx >> 5
  replicate      taps outside the image read the nearest pixel instead of 0
  dist_le        dist <= filter_dist          rel_le     rel <= filter_diff
  conf_ge        confidence >= conf           geo_gt     geo_sum > thres_view
  dsum_f64       the running sum of the reprojected depths kept in float64
  reverse_views  the reprojected depths summed from the last view to the first
  round_colour   colours rounded to nearest instead of truncated
Short saturation (ix, iy clamped to [-32768, 32767]) has NO mutant: a clamped coordinate and the unclamped one are both
outside any image narrower than 32768 pixels, so no case of a quick suite can observe it.  The table still runs shifts
beyond +-40000 so that the branch executes.

Every case is in *raw* form: what `svs_fuse_view` / `svs_fuse_points` take (depth maps, 68 float64 per source, 25 for the
points); cases built from cameras also keep the view dicts (`ref`, `srcs`, `kw`) for `svs_hip.fusion.fuse_view` and the
float64 oracle.
"""
import functools

import numpy as np

import fusion_oracle as forc
import synth

F32 = np.float32
F64 = np.float64
MUTANTS = ("round_away", "trunc_shift", "replicate", "dist_le", "rel_le", "conf_ge", "dsum_f64", "reverse_views",
           "round_colour", "geo_gt")
PER_SOURCE = ("src_mask", "src_depth_reproj", "src_x", "src_y")
OUTPUTS = PER_SOURCE + ("depth_avg", "photo_mask", "geo_mask", "final_mask", "xyz", "rgb")


# ---- matrices ----------------------------------------------------------------------------------------------------------
def oracle_matrices(K_ref, E_ref, K_src, E_src):
    """The six matrices of oracle/fusion_oracle.py::reproject_with_depth, as it writes them, widened: (68,) float64."""
    mats = (np.linalg.inv(K_ref), np.matmul(E_src, np.linalg.inv(E_ref)), K_src, np.linalg.inv(K_src),
            np.matmul(E_ref, np.linalg.inv(E_src)), K_ref)
    return np.concatenate([np.asarray(m, F64).reshape(-1) for m in mats])


def point_matrices(K_ref, E_ref):
    """inv(K_ref) (9), inv(E_ref) (16) of fusion_oracle.fuse_view's back-projection, widened: (25,) float64."""
    return np.concatenate([np.asarray(np.linalg.inv(np.asarray(K_ref)), F64).reshape(-1),
                           np.asarray(np.linalg.inv(np.asarray(E_ref)), F64).reshape(-1)])


def _mat3(M, a, b, c):
    return (M[0] * a + M[1] * b + M[2] * c, M[3] * a + M[4] * b + M[5] * c, M[6] * a + M[7] * b + M[8] * c)


def _mat4(M, a, b, c):
    return (M[0] * a + M[1] * b + M[2] * c + M[3], M[4] * a + M[5] * b + M[6] * c + M[7],
            M[8] * a + M[9] * b + M[10] * c + M[11])


# ---- the sampler, with its branches exposed ---------------------------------------------------------------------------------
def remap_parts(H, W, mapx, mapy, mut=frozenset()):
    """The integer side of cv2.remap(INTER_LINEAR): -> dict(bad, sx, sy (5-bit fixed point), ix, iy (before saturation),
    inside (4, ...): tap (0,0), (0,1), (1,0), (1,1) lies in the image)."""
    fx = (np.asarray(mapx, F32) * F32(32.0)).astype(F32)
    fy = (np.asarray(mapy, F32) * F32(32.0)).astype(F32)
    bad = ~((fx > -2.1e9) & (fx < 2.1e9) & (fy > -2.1e9) & (fy < 2.1e9))
    fx, fy = np.where(bad, 0, fx), np.where(bad, 0, fy)
    if "round_away" in mut:
        sx = (np.sign(fx) * np.floor(np.abs(fx.astype(F64)) + 0.5)).astype(np.int64)
        sy = (np.sign(fy) * np.floor(np.abs(fy.astype(F64)) + 0.5)).astype(np.int64)
    else:
        sx, sy = np.rint(fx).astype(np.int64), np.rint(fy).astype(np.int64)
    if "trunc_shift" in mut:
        ix, iy = np.fix(sx / 32.0).astype(np.int64), np.fix(sy / 32.0).astype(np.int64)
    else:
        ix, iy = sx >> 5, sy >> 5
    cx, cy = np.clip(ix, -32768, 32767), np.clip(iy, -32768, 32767)
    inside = np.stack([(cx + dx >= 0) & (cx + dx < W) & (cy + dy >= 0) & (cy + dy < H)
                       for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))])
    return dict(bad=bad, sx=sx, sy=sy, ix=ix, iy=iy, cx=cx, cy=cy, inside=inside)


def remap_variant(img, mapx, mapy, mut=frozenset()):
    """`fusion_oracle.remap_linear` with the sampler's mutants; with none of them it equals that function bit for bit
    (asserted on every sample of the table by tests/test_fusion_cases_cpu.py)."""
    img = np.asarray(img, F32)
    H, W = img.shape
    p = remap_parts(H, W, mapx, mapy, mut)
    ax = ((p["sx"] & 31).astype(F32) * F32(1.0 / 32.0)).astype(F32)
    ay = ((p["sy"] & 31).astype(F32) * F32(1.0 / 32.0)).astype(F32)
    one = F32(1.0)
    w = [(one - ay) * (one - ax), (one - ay) * ax, ay * (one - ax), ay * ax]
    out = None
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        pix = img[np.clip(p["cy"] + dy, 0, H - 1), np.clip(p["cx"] + dx, 0, W - 1)]
        s = pix if "replicate" in mut else np.where(p["inside"][k], pix, F32(0.0)).astype(F32)
        t = (s * w[k]).astype(F32)
        out = t if out is None else (out + t).astype(F32)
    return np.where(p["bad"], F32(0.0), out).astype(F32)


# ---- the ordered oracle ----------------------------------------------------------------------------------------------------
def ordered_fuse_mats(ref_depth, confidence, src_depths, mats, pmats=None, img=None, conf=0.0, filter_dist=1, filter_diff=0.01,
                      thres_view=1, extra_mask=None, mut=frozenset()):
    """`svs_fuse_view` then `svs_fuse_points` on raw arguments, in the kernels' operation order.
    ref_depth, confidence (H,W) float32; src_depths: n_src (H,W) float32 maps; mats (n_src,68) float64; pmats (25,) float64
    or None (no points); img (H,W,3) float32 or None; extra_mask (H,W), nonzero = keep, or None.
    -> every array the kernels write (OUTPUTS; masks uint8 0/1) plus, per (source, pixel), the float64 `dist`, the float32
    `rel`, the sampled source depth `ds` and the reprojected depth before rejection `drep_raw`, and `kz` (the source-camera
    z of the reference pixel)."""
    mut = frozenset(mut)
    assert mut <= set(MUTANTS), mut - set(MUTANTS)
    dref = np.ascontiguousarray(ref_depth, F32)
    H, W = dref.shape
    n_src = len(src_depths)
    mats = np.asarray(mats, F64).reshape(n_src, 68)
    fdist, fdiff, fconf = F64(filter_dist), F32(filter_diff), F32(conf)
    yi, xi = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xd, yd, dd = xi.astype(F64), yi.astype(F64), dref.astype(F64)
    out = {k: np.zeros((n_src, H, W), F32) for k in ("src_depth_reproj", "src_x", "src_y", "rel", "ds", "drep_raw")}
    out["src_mask"] = np.zeros((n_src, H, W), np.uint8)
    out["dist"], out["kz"] = np.zeros((n_src, H, W), F64), np.zeros((n_src, H, W), F64)
    geo_sum = np.zeros((H, W), np.int32)
    with np.errstate(all="ignore"):
        for v in range(n_src):
            M = mats[v]
            p = _mat3(M, xd * dd, yd * dd, 1.0 * dd)
            q = _mat4(M[9:], *p)
            k = _mat3(M[25:], *q)
            xs, ys = k[0] / k[2], k[1] / k[2]
            xsf, ysf = xs.astype(F32), ys.astype(F32)
            src = np.asarray(src_depths[v], F32)
            assert src.shape == (H, W)
            ds = remap_variant(src, xsf, ysf, mut) if mut & {"round_away", "trunc_shift", "replicate"} else forc.remap_linear(src, xsf, ysf)
            dsd = ds.astype(F64)
            p = _mat3(M[34:], xs * dsd, ys * dsd, 1.0 * dsd)
            q = _mat4(M[43:], *p)
            drep = q[2].astype(F32)
            k2 = _mat3(M[59:], *q)
            xr, yr = (k2[0] / k2[2]).astype(F32), (k2[1] / k2[2]).astype(F32)
            ex, ey = xr.astype(F64) - xd, yr.astype(F64) - yd
            dist = np.sqrt(ex * ex + ey * ey)
            rel = (np.abs((drep - dref).astype(F32)) / dref).astype(F32)
            ok = (dist <= fdist if "dist_le" in mut else dist < fdist) & (rel <= fdiff if "rel_le" in mut else rel < fdiff)
            out["drep_raw"][v], out["ds"][v], out["dist"][v], out["rel"][v], out["kz"][v] = drep, ds, dist, rel, k[2]
            out["src_mask"][v], out["src_depth_reproj"][v] = ok, np.where(ok, drep, F32(0.0))
            out["src_x"][v], out["src_y"][v] = xsf, ysf
            geo_sum += ok
        reps = out["src_depth_reproj"]
        order = range(n_src - 1, -1, -1) if "reverse_views" in mut else range(n_src)
        if n_src == 0:
            tot = dref.astype(F64)
        elif "dsum_f64" in mut:
            tot = functools.reduce(lambda a, b: a + b, [reps[v].astype(F64) for v in order]) + dd
        else:
            tot = (functools.reduce(lambda a, b: (a + b).astype(F32), [reps[v] for v in order]) + dref).astype(F32).astype(F64)
        out["depth_avg"] = tot / (geo_sum + 1).astype(F64)
    c = np.asarray(confidence, F32)
    photo = c >= fconf if "conf_ge" in mut else c > fconf
    geo = geo_sum > thres_view if "geo_gt" in mut else geo_sum >= thres_view
    fin = photo & geo
    if extra_mask is not None:
        fin = fin & (np.asarray(extra_mask) != 0)
    out["photo_mask"], out["geo_mask"], out["final_mask"] = (m.astype(np.uint8) for m in (photo, geo, fin))
    if pmats is not None:
        pm = np.asarray(pmats, F64).reshape(25)
        x, y, d = xd[fin], yd[fin], out["depth_avg"][fin]                      # row-major order of the surviving pixels
        with np.errstate(all="ignore"):
            p = _mat3(pm, x * d, y * d, 1.0 * d)
            q = _mat4(pm[9:], *p)
        out["xyz"] = np.stack(q, 1).astype(F32).reshape(-1, 3)
        if img is not None:
            c255 = (np.asarray(img, F32)[fin] * F32(255.0)).astype(F32)
            out["rgb"] = (np.rint(c255) if "round_colour" in mut else c255).astype(np.int32).astype(np.uint8).reshape(-1, 3)
    return out


def raw_from_views(ref, srcs, conf=0.0, filter_dist=1, filter_diff=0.01, thres_view=1, extra_mask=None):
    """The raw arguments of one `fuse_view(ref, srcs, ...)` call, matrices formed as the float64 oracle forms them."""
    mats = np.zeros((len(srcs), 68), F64)
    for v, s in enumerate(srcs):
        mats[v] = oracle_matrices(ref["K"], ref["E"], s["K"], s["E"])
    return dict(ref_depth=np.ascontiguousarray(ref["depth"], F32), confidence=np.ascontiguousarray(ref["confidence"], F32),
                src_depths=[np.ascontiguousarray(s["depth"], F32) for s in srcs], mats=mats,
                pmats=point_matrices(ref["K"], ref["E"]), img=ref.get("img"), conf=conf, filter_dist=filter_dist,
                filter_diff=filter_diff, thres_view=thres_view,
                extra_mask=None if extra_mask is None else (np.asarray(extra_mask) > 0).astype(np.uint8))


def ordered_fuse_view(ref, srcs, conf=0.0, filter_dist=1, filter_diff=0.01, thres_view=1, extra_mask=None, mut=frozenset()):
    """`svs_hip.fusion.fuse_view(ref, srcs, ..., per_source=True)` in the kernels' operation order (see ordered_fuse_mats)."""
    return ordered_fuse_mats(mut=mut, **raw_from_views(ref, srcs, conf, filter_dist, filter_diff, thres_view, extra_mask))


def threshold_band(out, filter_dist, filter_diff):
    """(n_src,H,W) bool: `dist` within 2 float64 ulp of filter_dist, or `rel` within 1 float32 ulp of filter_diff -- the only
    entries where a differently ordered float64 evaluation may decide a threshold the other way."""
    fd, fr = F64(filter_dist), F32(filter_diff)
    band = np.zeros(out["dist"].shape, bool)
    with np.errstate(all="ignore"):
        if np.isfinite(fd):
            band |= np.abs(out["dist"] - fd) <= 2 * np.spacing(fd)
        if np.isfinite(fr):
            band |= np.abs(out["rel"].astype(F64) - F64(fr)) <= F64(np.spacing(fr))
    return band


def same(a, b):
    """np.array_equal with NaN equal to NaN on float arrays; dtype and shape must match too."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def n_unequal(a, b):
    """number of unequal elements (NaN equal to NaN); -1 for a shape or dtype mismatch"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return -1
    ne = a != b
    if a.dtype.kind == "f":
        ne &= ~(np.isnan(a) & np.isnan(b))
    return int(ne.sum())


# ---- the case table ----------------------------------------------------------------------------------------------------------
T64 = 1.0 / 64.0
# (sx, sy) per source slot: set A = integers, multiples of 1/32, ties (odd multiples of 1/64) of both signs on each axis
SHIFTS_A = [(0, 0), (1, 0), (0, -1), (-2, 3),
            (0.25, 0), (0, 0.75), (5 / 32, -7 / 32), (-1 / 32, 31 / 32),
            (T64, 0), (3 * T64, 0), (-T64, 0), (-3 * T64, 0),
            (0, T64), (0, 3 * T64), (0, -T64), (7 * T64, -5 * T64)]
# set B = half-inside footprints on each side and corner, wholly outside, short saturation, the out-of-int branch, NaN
SHIFTS_B = [(-0.5, 0), (0.5, 0), (0, -0.5), (0, 0.5),
            (-0.5, -0.5), (0.5, 0.5), (-0.5, 0.5), (0.5, -0.5),
            (-300, 0), (0, 300), (40000, 0), (0, -40000),
            (-65536, 40000), (1e8, 0), (0, -1e8), (float("nan"), 0)]
REMAP_SIZES = [(1, 1), (1, 9), (7, 1), (5, 9), (3, 257)]
SPECIALS_FINITE = [0.0, -1.5, 1e-42]                    # zero, a negative, a float32 subnormal
SPECIALS_POISON = [float("inf"), float("nan")]


def _probe_image(rng, H, W, slot, poison):
    """a source depth map of dyadic values (k / 8) holding 0, a negative and a subnormal, and with poison=True inf and NaN"""
    img = (rng.integers(1, 64, (H, W)) / 8.0).astype(F32)
    flat = img.reshape(-1)
    specials = SPECIALS_FINITE + (SPECIALS_POISON if poison else [])
    if flat.size >= 9:
        for j, s in enumerate(specials):
            flat[(5 * slot + 2 * j + 1) % flat.size] = F32(s)
    elif slot % 2:                                                        # too small to hold them all: one per slot
        flat[slot % flat.size] = F32(specials[(slot // 2) % len(specials)])
    return img


def remap_probe_cases():
    """Identity geometry: K_ref = I, E = I, reference depth 1, K_src a pure dyadic shift, both thresholds inf.  Then
    src_x = x + sx exactly and src_depth_reproj is remap(src_depth, x + sx, y + sy) wherever that sample is finite and
    nonzero (a zero, inf or NaN sample fails the test and writes 0).  All 16 source slots in every call."""
    cases = []
    eye3, eye4 = np.eye(3, dtype=F32), np.eye(4, dtype=F32)
    for H, W in REMAP_SIZES:
        for tag, shifts in (("A", SHIFTS_A), ("B", SHIFTS_B)):
            for poison in (False, True):
                rng = np.random.default_rng(1000 * H + W + (7 if poison else 0))
                ref = dict(K=eye3, E=eye4, depth=np.ones((H, W), F32), confidence=np.ones((H, W), F32),
                           img=(rng.integers(0, 256, (H, W, 3)).astype(F32) / F32(255.)))
                srcs = []
                for slot, (sx, sy) in enumerate(shifts):
                    K = np.array([[1, 0, sx], [0, 1, sy], [0, 0, 1]], F32)
                    srcs.append(dict(K=K, E=eye4, depth=_probe_image(rng, H, W, slot, poison)))
                kw = dict(conf=0.0, filter_dist=float("inf"), filter_diff=float("inf"), thres_view=3)
                cases.append(dict(name=f"remap{tag}-{H}x{W}-{'poison' if poison else 'finite'}", group="remap", ref=ref,
                                  srcs=srcs, kw=kw, shifts=shifts))
    return cases


def _turn_y(E, ang):
    R = np.eye(4)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
    return (R @ np.asarray(E, F64)).astype(F32)


def general_cases():
    cases = []

    def add(name, views, ref, src_ids, **kw):
        cases.append(dict(name=name, group="general", ref=views[ref], srcs=[views[s] for s in src_ids], kw=kw))

    # the three view sets of test_gpu_fusion.py::test_fuse_view_vs_oracle, every reference view
    for hw, n_views, thres, conf in (((48, 64), 3, 1, 0.3), ((37, 53), 4, 2, 0.0), ((25, 31), 2, 1, 0.9)):
        views = synth.make_fusion_views(5 + n_views, hw=hw, n_views=n_views)
        extra = (np.random.default_rng(1).uniform(0, 1, hw) > 0.2).astype(F32) if n_views == 4 else None
        for ref in range(n_views):
            add(f"set{hw[0]}x{hw[1]}-ref{ref}", views, ref, [s for s in range(n_views) if s != ref], conf=conf, filter_dist=1,
                filter_diff=0.01, thres_view=thres, extra_mask=extra)
    # thres_view from 0 to n_src + 1; conf equal to a confidence that occurs (strict >); with and without extra_mask
    views = synth.make_fusion_views(31, hw=(20, 23), n_views=3)
    tie_conf = float(views[0]["confidence"][7, 11])
    extra = (np.random.default_rng(2).uniform(0, 1, (20, 23)) > 0.3).astype(F32)
    for thres in range(0, 4):
        add(f"thres{thres}", views, 0, [1, 2], conf=tie_conf, filter_dist=1, filter_diff=0.01, thres_view=thres,
            extra_mask=extra if thres % 2 else None)
    # a source turned so far that part of the reference projects behind it (k[2] <= 0)
    views = synth.make_fusion_views(32, hw=(25, 31), n_views=3)
    views[1] = dict(views[1], E=_turn_y(views[1]["E"], 1.45))
    add("turned", views, 0, [1, 2], conf=0.1, filter_dist=1, filter_diff=0.01, thres_view=1)
    # reference depths of 0, negative, inf and NaN; the same in a source
    views = synth.make_fusion_views(33, hw=(19, 27), n_views=3)
    for v, step in ((0, 7), (2, 11)):
        d = views[v]["depth"].copy().reshape(-1)
        for j, s in enumerate((0.0, -2.5, float("inf"), float("nan"), -0.0)):
            d[(3 + j)::5 * step] = F32(s)
        views[v] = dict(views[v], depth=d.reshape(19, 27))
    add("special-depths", views, 0, [1, 2], conf=0.0, filter_dist=1, filter_diff=0.01, thres_view=1)
    # n_src = 0 (thres_view 0 keeps everything, 1 nothing), 1 and 16
    views = synth.make_fusion_views(34, hw=(9, 14), n_views=2)
    add("nsrc0-thres0", views, 0, [], conf=0.5, thres_view=0)
    add("nsrc0-thres1", views, 0, [], conf=0.5, thres_view=1)
    add("nsrc1", views, 1, [0], conf=0.5, filter_dist=1, filter_diff=0.01, thres_view=1)
    views = synth.make_fusion_views(35, hw=(17, 257), n_views=17, noise=5e-4)       # an arc of 4 rad: some look from behind
    add("nsrc16-17x257", views, 8, [s for s in range(17) if s != 8], conf=0.2, filter_dist=1, filter_diff=0.01, thres_view=1)
    # the same upright: the views' height offsets stay inside the image, so most pixels are kept by several sources
    views = synth.make_fusion_views(35, hw=(257, 17), n_views=17, noise=5e-4)
    add("nsrc16-257x17", views, 8, [s for s in range(17) if s != 8], conf=0.2, filter_dist=1, filter_diff=0.01, thres_view=3)
    # the smallest and the thinnest images
    for hw in ((1, 1), (1, 300), (300, 1)):
        views = _thin_views(36 + hw[0] % 7, hw)
        add(f"size{hw[0]}x{hw[1]}", views, 0, [1, 2], conf=0.3, filter_dist=1, filter_diff=0.01, thres_view=1)
    return cases


def _thin_views(seed, hw):
    """Three views of ONE pose for images one pixel high or wide, where the parallax of make_fusion_views' arc would carry
    every sample off the image: the sources differ from the reference in focal length (3 % and 6 %) and principal point, so a
    reference pixel lands at a fractional position ALONG the image and, up to float32 rounding, on its row across it.  A
    source's depth map is the reference's at the nearest corresponding pixel, with noise."""
    H, W = hw
    base = synth.make_fusion_views(seed, hw=hw, n_views=1)[0]
    rng = np.random.default_rng(seed + 100)
    K = base["K"].astype(F64)
    # no skew and a zero principal point across the image: the coordinate across it is then 0 from exact zeros, not the
    # remainder of a cancellation (which would make its last bits a matter of summation order, BLAS against the kernel)
    K[0, 1] = 0.0
    if W == 1:
        K[0, 2] = 0.0
    if H == 1:
        K[1, 2] = 0.0
    views = {0: dict(base, K=K.astype(F32))}
    for j in (1, 2):
        s = 1.0 + 0.03 * j
        Kj = K.copy()
        Kj[0, 0], Kj[0, 1], Kj[1, 1] = s * K[0, 0], s * K[0, 1], s * K[1, 1]
        Kj[0, 2] = s * K[0, 2] + (1.7 * j if W > 1 else 0.0)
        Kj[1, 2] = s * K[1, 2] + (1.7 * j if W == 1 and H > 1 else 0.0)
        vs, us = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
        vr = (vs - Kj[1, 2]) / s + K[1, 2]
        ur = (us - Kj[0, 2] - Kj[0, 1] * (vr - K[1, 2]) / K[1, 1]) / s + K[0, 2] + K[0, 1] * (vr - K[1, 2]) / K[1, 1]
        d = base["depth"][np.clip(np.rint(vr).astype(int), 0, H - 1), np.clip(np.rint(ur).astype(int), 0, W - 1)]
        d = d * (1.0 + 2e-3 * rng.normal(0, 1, (H, W)))
        views[j] = dict(K=Kj.astype(F32), E=base["E"], depth=d.astype(F32), confidence=rng.uniform(0, 1, (H, W)).astype(F32),
                        img=base["img"])
    return views


def _identity_mats():
    return np.concatenate([np.eye(3).reshape(-1), np.eye(4).reshape(-1), np.eye(3).reshape(-1), np.eye(3).reshape(-1),
                           np.eye(4).reshape(-1), np.eye(3).reshape(-1)])


def tie_cases():
    """Hand-made matrices (raw form only).  dist tie: every matrix the identity except the final K_ref, whose cx is 1, so
    that every pixel's dist is exactly 1.0: rejected at filter_dist = 1, accepted at nextafter(1, 2).  rel tie: identity
    matrices, reference depth 1, source depth 1.25 (rel = 0.25 exactly: rejected at filter_diff = 0.25) or the float32 just
    below 1.25 (accepted).  zero-ref: a source one unit along z with a zero where the zero reference depths land, so that
    rel is 0 / 0 there."""
    H, W = 3, 5
    cases = []
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (H, W, 3)).astype(F32) / F32(255.)
    pm = np.concatenate([np.eye(3).reshape(-1), np.eye(4).reshape(-1)])
    ones = np.ones((H, W), F32)

    def add(name, mats, src, ref_depth=ones, **kw):
        raw = dict(ref_depth=ref_depth, confidence=ones, src_depths=[src], mats=mats.reshape(1, 68), pmats=pm, img=img, conf=0.0,
                   thres_view=1, extra_mask=None)
        raw.update(kw)
        cases.append(dict(name=name, group="tie", raw=raw))

    m = _identity_mats()
    m[59 + 2] = 1.0                                                      # final K_ref: cx = 1
    add("dist-tie-rejected", m, ones, filter_dist=1.0, filter_diff=0.01)
    add("dist-tie-accepted", m, ones, filter_dist=float(np.nextafter(1.0, 2.0)), filter_diff=0.01)
    m = _identity_mats()
    add("rel-tie-rejected", m, np.full((H, W), 1.25, F32), filter_dist=1.0, filter_diff=0.25)
    add("rel-tie-accepted", m, np.full((H, W), np.nextafter(F32(1.25), F32(0.0)), F32), filter_dist=1.0, filter_diff=0.25)
    m = _identity_mats()
    m[9 + 11] = 1.0                                                      # E_src @ inv(E_ref): one unit along z
    ref_depth = ones.copy()
    ref_depth[0, 1] = ref_depth[2, 3] = 0.0
    src = np.full((H, W), 2.0, F32)
    src[0, 0] = 0.0                                                      # the zero reference depths project to (0, 0)
    add("zero-ref", m, src, ref_depth=ref_depth, filter_dist=1.0, filter_diff=0.01)
    return cases


POINT_SIZES = [(1, 1), (3, 85), (16, 16), (1, 257), (17, 241)]             # H * W = 1, 255, 256, 257, 4097


def point_cases():
    """`fuse_points_kernel` and the scan of svs_scan.h through n_src = 0, thres_view = 0: the final mask is `confidence >
    0.5`, depth_avg the reference depth.  Masks with no survivor, with all, and ragged ones; H * W across the scan's block
    edges.  Image values: float32(k / 255) for all 256 codes -- float32(float32(k / 255) * 255) is k itself for every k (two
    roundings of at most half an ulp each cannot leave k's half-ulp neighbourhood), so these alone cannot tell truncation
    from rounding -- and, on three runs of five pixels out of four, (k + 1/4, 1/2, 3/4) / 255, which can."""
    cases = []
    for H, W in POINT_SIZES:
        view = synth.make_fusion_views(40 + H, hw=(H, W), n_views=1)[0]
        codes = (np.arange(H * W * 3) * 37 + H) % 256                      # 37 is coprime to 256: every code occurs
        frac = np.repeat((np.arange(H * W) // 5) % 4, 3) * 0.25
        frac[codes == 255] = 0.0                                           # values stay inside [0, 1]
        view = dict(view, img=((codes + frac).astype(F32) / F32(255.)).reshape(H, W, 3))
        rng = np.random.default_rng(H * W)
        masks = dict(none=np.zeros((H, W), F32), all=np.ones((H, W), F32), ragged=(rng.uniform(0, 1, (H, W)) < 0.4).astype(F32),
                     last=np.zeros((H, W), F32))
        masks["last"].reshape(-1)[-1] = 1.0
        for tag, m in masks.items():
            cases.append(dict(name=f"points-{H}x{W}-{tag}", group="points", ref=dict(view, confidence=m), srcs=[],
                              kw=dict(conf=0.5, thres_view=0)))
    return cases


@functools.lru_cache(maxsize=None)
def table():
    """every case, in raw form (`raw`), with the ordered oracle's result (`want`) computed once and shared"""
    cases = remap_probe_cases() + general_cases() + tie_cases() + point_cases()
    for c in cases:
        if "raw" not in c:
            c["raw"] = raw_from_views(c["ref"], c["srcs"], **c["kw"])
        c["want"] = ordered_fuse_mats(**c["raw"])
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def case_names():
    return [c["name"] for c in table()]


def case(name):
    return next(c for c in table() if c["name"] == name)
