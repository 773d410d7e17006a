"""TEST INFRASTRUCTURE ONLY -- the seeded inputs of tests/test_gpu_costvol_tail.py, built here so that
tests/test_costvol_tail_cpu.py can examine exactly the same arrays without a GPU (exclusion caps, deliberate edge cases sitting
clearly on one side of their decision).  numpy only (and the oracle's linear resize)."""
import numpy as np

import casmvs_oracle
import synth

F32 = np.float32
F64 = np.float64

# ---------------------------------------------------------------------------------------------------------------------
# softmax / depth / confidence
# ---------------------------------------------------------------------------------------------------------------------
TAIL_D = (1, 2, 3, 8, 15, 16, 17, 32, 63, 64, 65, 191, 192, 193, 200, 257)
# pixels per launch: 1, one less / one more than 32, 64 and 256 (a block's pixels in each of the three dispatch classes, so
# every D meets both sides of its own block size and of the other two), a prime-sided image, the stage-1 size of config 3
TAIL_HW = ((1, 1), (1, 31), (3, 11), (7, 9), (5, 13), (15, 17), (1, 257), (37, 53), (128, 160))
FAMILIES = ("n1", "n10", "n80", "flat", "peak200", "q10", "window")
NF = len(FAMILIES)


def tail_shapes():
    """(H, W, shift): pixel p holds family (p + shift) % NF; the one-pixel image is repeated with every shift."""
    out = []
    for (H, W) in TAIL_HW:
        for shift in (range(NF) if H * W == 1 else (0,)):
            out.append((H, W, shift))
    return out


def _paired(rng, D, n, spread):
    """Normal logits of which adjacent planes share one draw, pairs counted from the last plane (plane 0 stays alone when D
    is odd).  At spread >= 10 a softmax of independent draws is close to one-hot at most pixels, which puts sum p*k within
    rounding of an integer -- a tie that float32 and float64 may truncate differently at MOST pixels.  With pairs the dominant
    mass straddles two planes: sum p*k sits near k + 0.5 (or just above 0, where truncation has no decision to make)."""
    draws = rng.normal(0, spread, ((D + 1) // 2, n))
    idx = (np.arange(D) + (D % 2)) // 2
    return draws[idx]


# inputs whose first seed put a pixel within D * 2^-20 of a tie in an image too small to afford one under the 0.2 % cap
TAIL_SEEDS = {(16, 15, 17, 0): 1}


def tail_case(D, H, W, shift):
    """-> reg (D,H,W) float32, depth_values (D,H,W) float32, offset (H,W) float32, family (H,W) int, target (H,W) int.
    Families, one per pixel:
      n1       normal logits, spread 1
      n10,n80  normal logits, spread 10 / 80, adjacent planes paired (see _paired)
      flat     all logits equal (a per-pixel constant).  Odd D >= 3: equal logits make sum p*k = (D-1)/2 an exact integer, a
               true tie; plane 0 is lowered by ln 2 there, which moves the sum to D(D-1)/(2D-1), about (D-1)/2 + 0.25
      peak200  one logit 200 above spread-1 logits (every other exponential underflows in float32) and, so that the index does
               not sit on an integer, a neighbour of the peak ln 3 below it: sum p*k = peak +- 0.25
      q10      n10 quantised to multiples of 2^-8: adding the common offset +-1e4 (ulp 2^-10) is then exact, so the softmax
               of the offset logits is mathematically that of the plain ones
      window   mass placed so that the index lands on 0, 1, D-2 or D-1 (`target`, cycling over the pixels): planes t, t+1 with
               weight 1, t-2, t-1, t+2, t+3 with weight 0.1 where they exist, the rest 14 + spread-1 noise below; the
               confidence window then has 3, 4, 3 terms.  Target D-1 is only reachable by an exact one-hot (sum p*k < D-1
               otherwise): plane D-1 sits 800 above spread-1 logits, which underflows in float64 too -- 2 terms.
    `offset` is +1e4 / -1e4 / 0 on the q10 pixels in turn and 0 elsewhere (the second launch of the offset test)."""
    rng = np.random.default_rng([TAIL_SEEDS.get((D, H, W, shift), 0), D, H, W, shift])
    n = H * W
    fam = (np.arange(n) + shift) % NF
    reg = rng.normal(0, 1, (D, n))
    target = np.full(n, -1)
    for f, name in enumerate(FAMILIES):
        px = np.nonzero(fam == f)[0]
        m = px.size
        if m == 0:
            continue
        if name == "n10":
            reg[:, px] = _paired(rng, D, m, 10.0)
        elif name == "n80":
            reg[:, px] = _paired(rng, D, m, 80.0)
        elif name == "flat":
            reg[:, px] = rng.normal(0, 5, (1, m))
            if D >= 3 and D % 2 == 1:
                reg[0, px] -= np.log(2.0)
        elif name == "peak200":
            peak = rng.integers(0, D, m)
            nb = np.where(peak + 1 < D, peak + 1, peak - 1)
            top = reg[:, px].max(0) + 200.0
            reg[peak, px] = top
            if D >= 2:
                reg[nb, px] = top - np.log(3.0)
        elif name == "q10":
            reg[:, px] = np.round(_paired(rng, D, m, 10.0) * 256.0) / 256.0
        elif name == "window":
            t = np.array([0, 1, D - 2, D - 1])[(px // NF) % 4]
            t = np.clip(t, 0, D - 1)
            target[px] = t
            for j, pj in enumerate(px):
                col = rng.normal(0, 1, D) - 14.0
                if t[j] == D - 1 and D >= 2:
                    col = rng.normal(0, 1, D)
                    col[D - 1] = col.max() + 800.0
                else:
                    for off, wgt in ((-2, 0.1), (-1, 0.1), (0, 1.0), (1, 1.0), (2, 0.1), (3, 0.1)):
                        if 0 <= t[j] + off < D:
                            col[t[j] + off] = np.log(wgt)
                reg[:, pj] = col + rng.normal(0, 3)
    reg = reg.astype(F32)
    offset = np.zeros(n, F32)
    q = np.nonzero(fam == FAMILIES.index("q10"))[0]
    offset[q] = np.array([1e4, -1e4, 0.0], F32)[np.arange(q.size) % 3]
    # hypotheses that vary per pixel: a per-pixel scale on the planes and a per-voxel jitter below the plane spacing
    planes = np.linspace(425.0, 935.0, D) if D > 1 else np.array([680.0])
    dv = planes[:, None] * (1.0 + 0.05 * rng.uniform(-1, 1, (1, n))) + rng.uniform(0, 0.4 * 510.0 / max(D - 1, 1), (D, n))
    return (reg.reshape(D, H, W), dv.astype(F32).reshape(D, H, W), offset.reshape(H, W), fam.reshape(H, W),
            target.reshape(H, W))


# ---------------------------------------------------------------------------------------------------------------------
# depth hypotheses
# ---------------------------------------------------------------------------------------------------------------------
HYPO_STAGE1 = [(D, inv, rng_) for D in (2, 3, 8, 32, 33, 192) for inv in (False, True) for rng_ in ((425.0, 935.0), (0.5, 6.0))]
HYPO_IMG = ((64, 96), (40, 52), (576, 768))


def hypo_later_cases():
    """(img_hw, scale, prev_hw, D): every image size x scale x previous depth at 1/4, 1/2, 1/1 of the image and at one ratio
    that is no integer (37 x 53 -> 64 x 96, and the same ratio at the other sizes), D = 8 and 32."""
    out = []
    for (H, W) in HYPO_IMG:
        prevs = ((H // 4, W // 4), (H // 2, W // 2), (H, W), ((37 * H) // 64, (53 * W) // 96))
        for scale in (1, 2, 4):
            for prev in prevs:
                for D in (8, 32):
                    out.append(((H, W), scale, prev, D))
    return out


def prev_depth_field(hw, seed, lo=500.0, hi=800.0, noise=0.01):
    """A smooth field between lo and hi plus white noise of `noise` times the range."""
    h, w = hw
    rng = np.random.default_rng([seed, h, w])
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    s = 0.5 + 0.25 * np.sin(2 * np.pi * (1.3 * xx + 0.4)) * np.cos(2 * np.pi * 0.9 * yy) + 0.2 * (xx - yy)
    s = np.clip(s, 0.0, 1.0)
    return (lo + (hi - lo) * s + noise * (hi - lo) * rng.normal(0, 1, (h, w))).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# MVS prior look-up
# ---------------------------------------------------------------------------------------------------------------------
IMG_RES = (576, 768)
CAMS = ((0.0, 0.0, 0.0), (0.3, 0.02, 0.4), (-0.3, 0.04, 0.8), (0.15, -0.03, 0.2))      # x offset, y offset, skew
MIXED_DIMS = ((192, 36, 48), (32, 72, 96), (8, 144, 192), (48, 36, 48))
EQUAL_DIMS = ((48, 36, 48),) * 4


def _softmax_volume(rng, D, h, w):
    """softmax over D of N(0,1) logits drawn at 36 x 48; finer volumes resize them linearly in space and add 0.1 of white
    noise.  White noise at 144 x 192 would differ by 0.2 between neighbouring texels, and the float32 rounding of the image
    position (2e-7 of 96 texels) would then move the sample by 4e-6 -- measured between the float32 oracle and the float64
    reference -- which says nothing about who evaluates it.  A probability volume is as smooth as its image."""
    logits = rng.normal(0, 1, (D, 36, 48))
    if (h, w) != (36, 48):
        logits = casmvs_oracle.resize_linear(logits.astype(F32), (h, w)).astype(F64) + 0.1 * rng.normal(0, 1, (D, h, w))
    e = np.exp(logits - logits.max(0, keepdims=True))
    return (e / e.sum(0, keepdims=True)).astype(F32)


def make_views(seed, dims, hypo):
    """len(dims) <= 4 views looking at the origin from z = -2.5 (synth.make_camera), probability volumes softmax(N(0,1)).
    hypo(prev_depth, img_hw, D, scale, dmin, dmax, pix_interval, inverse) -> (D,h,w) float32 supplies the depth planes: the
    GPU test passes the kernel, the CPU test the float64 reference rounded to float32.
      * 36 x 48 volumes: stage-1 planes 1.5 .. 3.5 (a view with D = 48: linear in 1/depth);
      * 72 x 96 (stage 2): 32 planes, +-0.48 around a 36 x 48 depth field;  144 x 192 (stage 3): 8 planes, +-0.8 around a
        72 x 96 field.  Both vary per pixel.  The intervals are wider than a trained cascade's on purpose: the normalised
        depth divides by far - near, so a narrow range amplifies the float32 rounding of the camera-space depth (3e-7 here)
        into the trilinear weight -- at D = 8, where neighbouring planes differ by 0.3, a range of 0.48 measured 3.4e-6
        between the float32 oracle and the float64 reference, above the look-up's 3e-6; at these widths it stays below."""
    rng = np.random.default_rng([seed, len(dims)])
    views = []
    for j, (D, h, w) in enumerate(dims):
        dx, dy, sk = CAMS[j]
        K, pose = synth.make_camera(center=(dx, dy, -2.5), tilt=-0.12 * dx / 0.3, skew=sk)
        if (h, w) == (36, 48):
            z = hypo(None, (144, 192), D, 4, 1.5, 3.5, 0.0, D == 48)
        elif (h, w) == (72, 96):
            z = hypo(prev_depth_field((36, 48), seed + j, 2.3, 2.9, 0.02), (144, 192), D, 2, 1.5, 3.5, 0.03, False)
        else:
            z = hypo(prev_depth_field((72, 96), seed + j, 2.2, 2.8, 0.02), (144, 192), D, 1, 1.5, 3.5, 0.2, False)
        z = np.asarray(z, F32)
        assert z.shape == (D, h, w)
        views.append(dict(K=K, c2w=pose, cost=_softmax_volume(rng, D, h, w), z_near=z[0].copy(), z_far=z[-1].copy()))
    return views


def project64(views, xyz):
    """Normalised image position and camera-space depth of world points in every view, float64 (vsdf.py:405-415):
    -> x, y, z, each (V,) + xyz.shape[:-1]."""
    H, W = IMG_RES
    xs, ys, zs = [], [], []
    for v in views:
        K, c2w = np.asarray(v["K"], F64), np.asarray(v["c2w"], F64)
        p = (np.asarray(xyz, F64) - c2w[:3, 3]) @ c2w[:3, :3]
        with np.errstate(all="ignore"):
            y = p[..., 1] / p[..., 2] * K[1, 1] + K[1, 2]
            x = p[..., 0] / p[..., 2] * K[0, 0] + K[0, 2] + (y - K[1, 2]) * K[0, 1] / K[1, 1]
        xs.append(x / ((W - 1) / 2) - 1); ys.append(y / ((H - 1) / 2) - 1); zs.append(p[..., 2])
    return np.stack(xs), np.stack(ys), np.stack(zs)


def past_last_texel(views, xyz):
    """Points that some view sees between the last texel and the frustum bound (1 < |x| or |y| <= 1.001, in front of it).
    There the zero padding scales the sampled near and far planes by the weight t of the last texel, and the normalised depth
    2 (z - t near) / (t (far - near)) - 1 moves by 2 z / (far - near) per unit of t, while t itself moves by (W-1)/2 per unit of
    x: the float32 rounding of x (2e-7) reaches the trilinear weight multiplied by 1e3 or more in a fine, narrow-range
    volume.  That is a property of the formula in float32, whoever evaluates it; the typical-point inputs leave such points
    out, and the edge-case set places them on purpose in the one view whose bound has room for them (D = 192 at 36 x 48)."""
    x, y, z = project64(views, xyz)
    band = lambda a: (np.abs(a) > 1.0 - 1e-6) & (np.abs(a) <= 1.0011)
    return (((band(x) & (np.abs(y) <= 1.0011)) | (band(y) & (np.abs(x) <= 1.0011))) & (z > 0)).any(0)


def random_rays(views, vi, R, S, seed):
    """R rays through continuous pixels of views[vi] (some up to 3 % outside the image), S sorted depths 0.2 .. 5.5 each, drawn
    again where a point falls past the last texel of some view (past_last_texel).
    -> cam (3,), dirs (R,3), z (R,S), xyz (R,S,3) = float32(cam + z * dir)."""
    rng = np.random.default_rng([seed, R, S])
    H, W = IMG_RES
    u = rng.uniform(-0.03, 1.03, (R, 2))
    u = np.where(((u > -0.001) & (u < 0)) | ((u > 1) & (u < 1.001)), 0.5, u) * np.array([W - 1, H - 1])   # (a whole ray there)
    K, c2w = np.asarray(views[vi]["K"], F64), np.asarray(views[vi]["c2w"], F64)
    yl = (u[:, 1] - K[1, 2]) / K[1, 1]
    xl = (u[:, 0] - K[0, 2] - yl * K[0, 1]) / K[0, 0]
    d = np.stack([xl, yl, np.ones(R)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    dirs = (d @ c2w[:3, :3].T).astype(F32)
    cam = c2w[:3, 3].astype(F32)
    z = rng.uniform(0.2, 5.5, (R, S)).astype(F32)
    for _ in range(20):
        xyz = (cam[None, None] + z[:, :, None] * dirs[:, None, :]).astype(F32)
        bad = past_last_texel(views, xyz)
        if not bad.any():
            break
        z[bad] = rng.uniform(0.2, 5.5, int(bad.sum())).astype(F32)
    assert not bad.any()
    z = np.sort(z, -1)
    xyz = (cam[None, None] + z[:, :, None] * dirs[:, None, :]).astype(F32)
    return cam, dirs, z, xyz


def _bilinear64(img, xn, yn):
    """align_corners=True sample of (h,w) at normalised (xn, yn) inside the image, float64."""
    h, w = img.shape
    ix, iy = (xn + 1) / 2 * (w - 1), (yn + 1) / 2 * (h - 1)
    x0, y0 = int(min(max(np.floor(ix), 0), w - 2)), int(min(max(np.floor(iy), 0), h - 2))
    tx, ty = ix - x0, iy - y0
    a = np.asarray(img, F64)
    return ((1 - tx) * (1 - ty) * a[y0, x0] + tx * (1 - ty) * a[y0, x0 + 1] + (1 - tx) * ty * a[y0 + 1, x0]
            + tx * ty * a[y0 + 1, x0 + 1])


def unproject(view, xn, yn, z):
    """World point (float64) that `view` sees at normalised image position (xn, yn) and camera-space depth z."""
    H, W = IMG_RES
    K, c2w = np.asarray(view["K"], F64), np.asarray(view["c2w"], F64)
    xp, yp = (xn + 1) * (W - 1) / 2, (yn + 1) * (H - 1) / 2
    yl = (yp - K[1, 2]) / K[1, 1]
    xl = (xp - K[0, 2] - (yp - K[1, 2]) * K[0, 1] / K[1, 1]) / K[0, 0]
    return c2w[:3, :3] @ np.array([xl * z, yl * z, z]) + c2w[:3, 3]


def depth_at(view, xn, yn, zn, inverse):
    """Camera-space depth whose normalised depth in `view` at (xn, yn) is zn (vsdf.py:428 / :432 solved for z)."""
    near = _bilinear64(view["z_near"], np.clip(xn, -1, 1), np.clip(yn, -1, 1))
    far = _bilinear64(view["z_far"], np.clip(xn, -1, 1), np.clip(yn, -1, 1))
    if inverse:
        return near / (1.0 - (zn + 1) / 2 * (1.0 - near / far))
    return near + (zn + 1) / 2 * (far - near)


# (label, xn, yn, zn or None, z or None, expected validity IN THE VIEW the point is built from)
def edge_specs():
    s = []
    for xn, yn in ((-1, -1), (1, -1), (-1, 1), (1, 1), (-1, 0), (1, 0), (0, -1), (0, 1)):
        s.append((f"border({xn},{yn})", float(xn), float(yn), 0.1, None, True))
    for sg in (-1.0, 1.0):
        s.append((f"x={sg * 1.0005}", sg * 1.0005, 0.3, -0.2, None, True))       # past the last texel, inside the bound
        s.append((f"y={sg * 1.0005}", -0.2, sg * 1.0005, 0.3, None, True))
        s.append((f"x={sg * 1.002}", sg * 1.002, 0.3, -0.2, None, False))
        s.append((f"y={sg * 1.002}", 0.45, sg * 1.002, 0.3, None, False))
        s.append((f"zn={sg}", 0.3, -0.4, sg, None, True))                         # on the first / last plane
        s.append((f"zn={sg * 1.005}", -0.5, 0.2, sg * 1.005, None, True))         # 0.25 % of the range outside: valid
        s.append((f"zn={sg * 1.04}", 0.6, 0.5, sg * 1.04, None, False))           # 2 % of the range outside: invalid
    s.append(("behind -2.0", 0.0, 0.0, None, -2.0, False))
    s.append(("behind -0.1", 0.4, -0.3, None, -0.1, False))
    s.append(("corner on last plane", 1.0, 1.0, 1.0, None, True))
    s.append(("corner on first plane", -1.0, -1.0, -1.0, None, True))
    return s


def edge_points(views, e, inverse):  # e = 0 in the tests: see past_last_texel
    """-> xyz (1,N,3) float32, expected (N,) bool (validity in view e), labels: the points of edge_specs() un-projected
    from view e, so that their position in that view is known."""
    pts, exp, labels = [], [], []
    for label, xn, yn, zn, z, ok in edge_specs():
        zz = depth_at(views[e], xn, yn, zn, inverse) if z is None else z
        pts.append(unproject(views[e], xn, yn, zz))
        exp.append(ok)
        labels.append(label)
    return np.asarray(pts, F64).astype(F32)[None], np.asarray(exp), labels


def lonely_point(views):
    """A point in front of view 0 (depth 1.55 of its 1.5 .. 3.5, near its right border) that no other view of the three-view
    mixed set sees: view 1's range starts above 1.7, and it lies to the right of view 2's frustum."""
    return unproject(views[0], 0.98, 0.1, 1.55).astype(F32).reshape(1, 1, 3)


# (name, dims, n_views, (R,S), view_index, inverse, seed)
def lookup_cases():
    c = []
    for V in (1, 2, 3, 4):
        c.append((f"equal_v{V}", EQUAL_DIMS[:V], (10, 100), V - 1, False, 20 + V))
    # inverse depth goes with stage-1 planes only (the reference raises for later stages, vsdf.py:429; with a narrow range
    # 1 - near / far is small and the expression cancels): the equal-size set, whose planes are linear in 1 / depth
    for k, (R, S) in enumerate(((1, 1), (7, 9), (8, 8), (5, 13), (10, 100))):
        c.append((f"mixed3_n{R * S}", MIXED_DIMS[:3], (R, S), k % 3, False, 40 + 2 * k))
        c.append((f"equal3_n{R * S}_inv", EQUAL_DIMS[:3], (R, S), k % 3, True, 41 + 2 * k))
    c.append(("mixed4_n1000", MIXED_DIMS, (10, 100), 3, False, 60))
    c.append(("mixed2_n1000", MIXED_DIMS[1:3], (10, 100), 0, False, 61))
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_IMG = (64, 96)
CHAIN_D = (16, 8, 8)
CHAIN_SCALE = (4, 2, 1)
CHAIN_RANGE = (1.5, 3.5)
CHAIN_PIX = (0.0, float(F32(0.12)), float(F32(0.1)))          # stage 2: +-0.48 around stage 1's depth, stage 3: +-0.4
CHAIN_POINTS = (16, 40)
# Points whose validity the carried tolerance of the planes could turn (a margin below 1e-5 + the carried change): held to
# an absolute count, since the carried change is a property of the chain and not of a float32 rounding.  2 of 640.
CHAIN_CARRIED_CAP = 2


def chain_inputs():
    """-> regs: one random (D, H/s, W/s) volume of logits (spread 1.5) per stage;  cams: K and c2w of three views;
    xyz (16,40,3): points along rays of view 1, not past the last texel of any view (random_rays)."""
    rng = np.random.default_rng(11)
    H, W = CHAIN_IMG
    regs = [rng.normal(0, 1.5, (D, H // s, W // s)).astype(F32) for D, s in zip(CHAIN_D, CHAIN_SCALE)]
    cams = [dict(K=v["K"], c2w=v["c2w"])
            for v in make_views(5, EQUAL_DIMS[:3], lambda *a: np.zeros((48, 36, 48), F32))]
    _, _, _, xyz = random_rays(cams, 1, CHAIN_POINTS[0], CHAIN_POINTS[1], 13)
    return regs, cams, xyz


# ---------------------------------------------------------------------------------------------------------------------
# partial weights past the last texel, at the tight bound
# ---------------------------------------------------------------------------------------------------------------------
def partial_weight_case(inside=False):
    """-> view, xyz (1,N,3) float32, weight (1,N).  Between the last texel and the 1.001 bound the zero padding leaves the
    sample a partial weight.  In a probability volume that is ill-conditioned through the normalised depth (past_last_texel),
    so the edge-case set can only hold such points to the D = 192 bound.  This view takes the depth out of it: (8, 36, 48)
    with the SAME map, values 0.05 .. 0.125, on every plane, stage-1 planes 1.5 .. 3.5.  Anywhere between the first and the
    last plane the sample is then the map's bilinear value times the weight inside the image, 1 - 0.0005 * (n - 1) / 2 per
    axis that is past its last texel -- and the float32 rounding of the image position (3e-7) moves it by 0.125 * 24 * 3e-7,
    a third of the 3e-6 bound, while a dropped or fully weighted last texel moves it by 6e-4 or more.
    Points: x or y or both at +-1.0005, normalised depth -0.2 and 0.3 (before the padding scales the planes; -0.17 .. 0.37
    after it).  inside=True: the same points moved onto the last texel (+-1), whose sample the weight multiplies."""
    rng = np.random.default_rng(91)
    K, pose = synth.make_camera(center=CAMS[0][:2] + (-2.5,), tilt=0.0, skew=CAMS[0][2])
    D, h, w = 8, 36, 48
    planes = np.linspace(1.5, 3.5, D).astype(F32)
    cost = np.broadcast_to(rng.uniform(0.05, 0.125, (1, h, w)), (D, h, w)).astype(F32).copy()
    view = dict(K=K, c2w=pose, cost=cost, z_near=np.full((h, w), planes[0], F32), z_far=np.full((h, w), planes[-1], F32))
    e = 1.0 if inside else 1.0005
    pts, weight = [], []
    for zn in (-0.2, 0.3):
        for xn, yn in ((e, 0.3), (-e, -0.55), (0.2, e), (-0.7, -e), (e, e), (-e, e), (e, -e), (-e, -e)):
            pts.append(unproject(view, xn, yn, 1.5 + (zn + 1) / 2 * 2.0))
            wx = 1.0 - (abs(xn) - 1.0) * (w - 1) / 2 if abs(xn) > 1 else 1.0
            wy = 1.0 - (abs(yn) - 1.0) * (h - 1) / 2 if abs(yn) > 1 else 1.0
            weight.append(wx * wy)
    return view, np.asarray(pts, F64).astype(F32)[None], np.asarray(weight)[None]
