"""TEST INFRASTRUCTURE ONLY -- float64 references of the three operations between the regularised cost volume and the
MVS prior of the loss, written from the reference project's formulas (not from the kernels, not from oracle/):

  * tail64           DepthNet.forward, models/CasMVSNet.py:653-661: softmax over D, depth regression, the truncated
                     regression index, the zero-padded 4-tap confidence.
  * hypotheses64     CascadeMVSNet.forward :712-751 with get_depth_range_samples (:579-595), its inverse form (:538-547) and
                     get_cur_depth_range_samples (:519-536).  The two resizes are torch.nn.functional.interpolate in float64
                     (bilinear for the previous depth, trilinear for the hypothesis volume, align_corners=False): the REAL
                     trilinear resize, which is what tests the kernel's "identity along D, 2x2 in space" evaluation.
  * cost_mapping64   VolOpt.cost_mapping, volsdf/vsdf.py:382-452, with torch.nn.functional.grid_sample in float64 (bilinear,
                     zero padding, align_corners=True); views may differ in (D,H,W).  Also returns, per view and point, the
                     distance of every quantity of the two `invalid` chains from its threshold.

Inputs are the float32 values the kernels receive, widened to float64; nothing is rounded on the way.
Only tests/ may import this module.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

F64 = np.float64


# ---------------------------------------------------------------------------------------------------------------------
# softmax / depth / confidence
# ---------------------------------------------------------------------------------------------------------------------
def tail64(reg, depth_values):
    """reg (D,H,W), depth_values (D,H,W) -> prob (D,H,W), depth (H,W), conf (H,W), idx (H,W int64), idx_f (H,W):
    idx_f is the float64 sum p*k whose truncation is idx, so that a caller can see how close to an integer it is."""
    reg = np.asarray(reg, F64)
    dv = np.asarray(depth_values, F64)
    D = reg.shape[0]
    e = np.exp(reg - reg.max(0, keepdims=True))
    prob = e / e.sum(0, keepdims=True)
    depth = (prob * dv).sum(0)
    k = np.arange(D, dtype=F64).reshape(-1, 1, 1)
    idx_f = (prob * k).sum(0)
    idx = np.clip(np.trunc(idx_f).astype(np.int64), 0, D - 1)
    # 4 * avg_pool3d(pad(prob, (1 before, 2 after)), (4,1,1)): the sum of p[k-1 .. k+2], zero padded
    z = np.zeros((1,) + prob.shape[1:], F64)
    padded = np.concatenate([z, prob, z, z], 0)
    sum4 = padded[0:D] + padded[1:D + 1] + padded[2:D + 2] + padded[3:D + 3]
    conf = np.take_along_axis(sum4, idx[None], 0)[0]
    return prob, depth, conf, idx, idx_f


def prob_rtol(reg):
    """Relative bound of a float32 softmax evaluated as exp2((x - max) * log2(e)), elementwise (D,H,W):
    (16 + 2 * |x - max|) * 2^-24.  The float32 subtraction x - max and the product with log2(e) round once each, which moves
    the exponent by up to |x - max| * 2^-24 each, i.e. the exponential by that relative amount; the rounded constant adds a
    quarter of that; the exponential instruction is good to 2^-23; the float32 sum over D and the division add a few units
    more (16 covers them).  At |x - max| <= 8 this is the rtol = 1e-5 * (a fifth) the fixtures are held to."""
    reg = np.asarray(reg, F64)
    return (16.0 + 2.0 * np.abs(reg - reg.max(0, keepdims=True))) * 2.0 ** -24


def near_tie(idx_f, prob, D):
    """Pixels whose index a float32 evaluation may legitimately truncate to the neighbouring plane: the float64 sum p*k
    lies within D * 2^-20 of an integer n in 1 .. D-1.  Two refinements of "within D * 2^-20 of an integer", both of
    which only shrink the set:
      * n = 0 is no decision point: truncation sends all of (-1, 1) to 0, and the sum is never negative;
      * a softmax that is exactly one-hot already in float64 (every other exponential underflows to 0.0, a gap above 745)
        is exactly one-hot in float32 as well, and the sum is then the exact integer in both: nothing is rounded."""
    n = np.rint(idx_f)
    close = (np.abs(idx_f - n) < D * 2.0 ** -20) & (n >= 1) & (n <= D - 1)
    return close & ~(prob.max(0) == 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# depth hypotheses
# ---------------------------------------------------------------------------------------------------------------------
def hypotheses64(prev_depth, img_hw, ndepth, scale, dmin, dmax, pix_interval, inverse):
    """The arguments of svs_hip.costvol.depth_hypotheses -> (D, H/scale, W/scale) float64.
    prev_depth None: stage 1, D planes between dmin and dmax (linear, or linear in 1/depth), the same for every pixel.
    prev_depth (Hp,Wp): resized to the image (bilinear), +-(D/2)*pix_interval around it in D planes (the reference does this
    in both the linear and the `inverse` call, :554), then the volume resized to (D, H/scale, W/scale) (trilinear)."""
    H, W = img_hw
    D = int(ndepth)
    k = torch.arange(D, dtype=torch.float64)
    if prev_depth is None:
        lo, hi = float(np.float32(dmin)), float(np.float32(dmax))
        if inverse:
            t = torch.linspace(0, 1, D, dtype=torch.float64)
            planes = 1.0 / (1.0 / lo * (1.0 - t) + 1.0 / hi * t)
        else:
            planes = lo + k * ((hi - lo) / (D - 1))
        vol = planes.view(D, 1, 1).repeat(1, H, W)
    else:
        prev = torch.from_numpy(np.ascontiguousarray(np.asarray(prev_depth, F64)))
        cur = Fn.interpolate(prev[None, None], [H, W], mode="bilinear", align_corners=False)[0, 0]
        pix = float(np.float32(pix_interval))
        cmin = cur - D / 2 * pix
        cmax = cur + D / 2 * pix
        new_interval = (cmax - cmin) / (D - 1)
        vol = cmin[None] + k.view(D, 1, 1) * new_interval[None]
    out = Fn.interpolate(vol[None, None], [D, H // int(scale), W // int(scale)], mode="trilinear", align_corners=False)
    return out[0, 0].numpy()


# ---------------------------------------------------------------------------------------------------------------------
# MVS prior look-up
# ---------------------------------------------------------------------------------------------------------------------
MARGIN_NAMES = ("z>1e-5", "x<1.001", "x>-1.001", "y<1.001", "y>-1.001", "near>1e-5", "far>1e-5", "zn<1.01", "zn>-1.01")


def _near_far(v):
    if "z_mvs" in v:
        return np.asarray(v["z_mvs"][0], F64), np.asarray(v["z_mvs"][-1], F64)
    return np.asarray(v["z_near"], F64), np.asarray(v["z_far"], F64)


def cost_mapping64(xyz, view_index, views, img_res, inverse_depth=False):
    """xyz (R,S,3); views: dicts of K (4,4), c2w (4,4), cost (D,h,w) and z_mvs (D,h,w) or z_near / z_far (h,w), sizes free per
    view; img_res (H,W) of the scene's images.
    -> pj (R,S), pi (R,S), valid (R,S) bool, margins (V,R,S,9), inval (V,R,S) bool.
    margins[v,r,s,c] = |quantity - threshold| of comparison c (MARGIN_NAMES) in view v, in the unit of that comparison.  The
    four comparisons made after the depth range is sampled are only decisions where the first five passed: elsewhere (the
    point is already invalid and its coordinates are -99) their margin is +inf.  A NaN quantity (0/0 where near = far = 0)
    compares false whatever its rounding: +inf as well."""
    xyz = torch.from_numpy(np.ascontiguousarray(np.asarray(xyz, F64)))
    R, S, _ = xyz.shape
    _h, _w = img_res
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, F64)))
    pj = torch.zeros(R, S, dtype=torch.float64)
    pi = torch.zeros(R, S, dtype=torch.float64)
    valid = torch.zeros(R, S, dtype=torch.bool)
    margins, invals = [], []
    gs = lambda vol, grid: Fn.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    for i, v in enumerate(views):
        K, c2w = T(v["K"]), T(v["c2w"])[:3]
        fx, fy, cx, cy, sk = K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]
        p = (xyz - c2w[:, 3].view(1, 1, 3)) @ c2w[:, :3]
        z = p[..., 2].clone()
        y = p[..., 1] / z * fy + cy
        x = p[..., 0] / z * fx + cx + (y - cy) * sk / fy
        x = x / ((_w - 1) / 2) - 1
        y = y / ((_h - 1) / 2) - 1
        m = torch.full((R, S, 9), float("inf"), dtype=torch.float64)
        m[..., 0] = (z - 1e-5).abs()
        m[..., 1], m[..., 2] = (x - 1.001).abs(), (x + 1.001).abs()
        m[..., 3], m[..., 4] = (y - 1.001).abs(), (y + 1.001).abs()
        inval = (z < 1e-5) | (x > 1.001) | (x < -1.001) | (y > 1.001) | (y < -1.001)
        first = inval.clone()
        x, y, z = x.masked_fill(inval, -99.0), y.masked_fill(inval, -99.0), z.masked_fill(inval, -99.0)
        near_map, far_map = _near_far(v)
        grid2 = torch.stack([x, y], -1)[None]
        near = gs(T(near_map)[None, None], grid2)[0, 0]
        far = gs(T(far_map)[None, None], grid2)[0, 0]
        if inverse_depth:
            far = torch.where(inval, torch.full_like(far, 1e-8), far)
            zn = 2 * (1.0 - near / z) / (1.0 - near / far) - 1
        else:
            zn = 2 * (z - near) / (far - near) - 1
        second = torch.stack([(near - 1e-5).abs(), (far - 1e-5).abs(), (zn - 1.01).abs(), (zn + 1.01).abs()], -1)
        second = torch.where(torch.isnan(second) | first[..., None], torch.full_like(second, float("inf")), second)
        m[..., 5:] = second
        inval = (near < 1e-5) | (far < 1e-5) | (zn > 1.01) | (zn < -1.01) | inval
        x, y, zn = x.masked_fill(inval, -99.0), y.masked_fill(inval, -99.0), zn.masked_fill(inval, -99.0)
        grid3 = torch.stack([x, y, zn], -1).view(1, R, S, 1, 3).permute(0, 2, 1, 3, 4)
        cost = gs(T(v["cost"])[None, None], grid3)[0, 0, :, :, 0].permute(1, 0)
        if i == view_index:
            pi = cost
        else:
            pj = pj + cost
            valid = valid | ~inval
        margins.append(m)
        invals.append(inval)
    pi = torch.where(valid, pi, torch.zeros_like(pi))
    return pj.numpy(), pi.numpy(), valid.numpy(), torch.stack(margins).numpy(), torch.stack(invals).numpy()


def near_threshold(margins, tol=1e-5):
    """(V,R,S,9) margins -> (R,S) bool: some comparison of some view sits within `tol` of its threshold."""
    return (margins < tol).any(-1).any(0)


# ---------------------------------------------------------------------------------------------------------------------
# the chain: hypotheses -> tail -> hypotheses -> tail -> ... -> look-up, with the tolerance each stage hands on
# ---------------------------------------------------------------------------------------------------------------------
def chain64(regs, img_hw, scales, dmin, dmax, pixes, hypo_rtol=5e-6, depth_rtol=3e-6):
    """The cascade in float64, every stage fed with its own previous depth -> one dict per stage: h (hypotheses), prob, depth,
    conf, idx, idx_f, and the tolerances t_h, t_p, t_d of h, prob and depth for an evaluation that is fed with ITS OWN previous
    output: the stage's own bound (hypo_rtol of the plane, prob_rtol, depth_rtol of the pixel's largest plane) plus the error
    its input carries, measured here by moving the input by the previous tolerance and taking the change of the output.  Both
    maps are linear in that input with weights >= 0, so moving every element up by its tolerance gives the largest change.
    The index and the confidence depend on the logits alone, which both sides share: they carry nothing."""
    stages, prev, t_prev = [], None, None
    for reg, scale, pix in zip(regs, scales, pixes):
        D = reg.shape[0]
        h = hypotheses64(prev, img_hw, D, scale, dmin, dmax, pix, False)
        t_h = hypo_rtol * np.abs(h)
        if prev is not None:
            t_h = t_h + np.abs(hypotheses64(prev + t_prev, img_hw, D, scale, dmin, dmax, pix, False) - h)
        prob, depth, conf, idx, idx_f = tail64(reg, h)
        t_p = 1e-9 + prob_rtol(reg) * prob
        t_d = depth_rtol * np.abs(h).max(0) + np.abs(tail64(reg, h + t_h)[1] - depth)
        stages.append(dict(h=h, prob=prob, depth=depth, conf=conf, idx=idx, idx_f=idx_f, t_h=t_h, t_p=t_p, t_d=t_d))
        prev, t_prev = depth, t_d
    return stages


def chain_lookup64(xyz, view_index, cams, stages, img_res):
    """The look-up over one view per stage (its probability volume, its first and last plane) -> the outputs of
    cost_mapping64 and what the stages' tolerances can move: carried_pj, carried_pi (R,S) and carried_margin (R,S), the largest
    change of any validity margin of any view.  The planes are moved by +-t_h, near and far together and apart (four runs);
    the volumes by +t_p (one run: the sample is a sum with weights >= 0); the two changes add."""
    mk = lambda c, cost, near, far: dict(K=c["K"], c2w=c["c2w"], cost=cost, z_near=near, z_far=far)
    want = cost_mapping64(xyz, view_index, [mk(c, s["prob"], s["h"][0], s["h"][-1]) for c, s in zip(cams, stages)], img_res)
    up = cost_mapping64(xyz, view_index, [mk(c, s["prob"] + s["t_p"], s["h"][0], s["h"][-1]) for c, s in zip(cams, stages)],
                        img_res)
    by_prob_pj, by_prob_pi = np.abs(up[0] - want[0]), np.abs(up[1] - want[1])
    c_pj, c_pi, c_m = 0.0, 0.0, 0.0
    for s_near, s_far in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        moved = cost_mapping64(xyz, view_index, [mk(c, s["prob"], s["h"][0] + s_near * s["t_h"][0],
                                                    s["h"][-1] + s_far * s["t_h"][-1]) for c, s in zip(cams, stages)], img_res)
        c_pj = np.maximum(c_pj, np.abs(moved[0] - want[0]))
        c_pi = np.maximum(c_pi, np.abs(moved[1] - want[1]))
        with np.errstate(invalid="ignore"):
            dm = np.abs(moved[3] - want[3])
        c_m = np.maximum(c_m, np.where(np.isfinite(dm), dm, 0.0).max(-1).max(0))
    return want, c_pj + by_prob_pj, c_pi + by_prob_pi, c_m
