"""TEST INFRASTRUCTURE ONLY -- a plain numpy / torch restatement of the parts of UCSNet (models/ucsnet.py of the reference)
that CasMVSNet has no counterpart for, written from the reference's formulas and not from the kernels:

  * deconv2d_taps              ConvTranspose2d(k3, s2, p1, output_padding 1) by its tap rule (:135, 225)
  * feat_ext_net               FeatExtNet (:237-302) with torch functional convolutions and deconv2d_taps
  * resize_bilinear32 / 64     F.interpolate(mode='bilinear', align_corners=False) (:450-452)
  * uncertainty_samples32 / 64 uncertainty_aware_samples at stages 2 and 3 (:59-70), float32 in the reference's operation order
  * stage1_planes              the same function at stage 1 (:47-57), torch float32 on the CPU
  * variance64                 exp_variance (:393-394) in float64 on costvol_tail_ref.tail64
  * variance32                 the same in float32 numpy (the yardstick for the float32 error of that formula)

and the seeded parameters / inputs that tests/golden/make_ucsnet_fixture.py and the tests share.
"""
import numpy as np

import costvol_tail_ref as tref
import synth

F32 = np.float32
F64 = np.float64
EPS = 1e-12

FIXTURE_SEED = 21
FIXTURE_HW = (64, 96)
FIXTURE_NDEPTHS = (16, 8, 8)
FIXTURE_LAMB = 1.5
PIN = 6000                 # arrays with more than PIN_ABOVE elements are pinned at PIN sampled positions
PIN_ABOVE = 16384


# ---------------------------------------------------------------------------------------------------------------------
# seeded parameters
# ---------------------------------------------------------------------------------------------------------------------
def make_featext_params(seed, base=8):
    """State-dict-named float32 arrays of FeatExtNet (models/ucsnet.py:237-302), BatchNorm in eval form with non-trivial
    running statistics."""
    rng = np.random.default_rng(seed)
    p = {}

    def bn(name, c):
        p[f"{name}.bn.weight"] = rng.uniform(0.6, 1.4, c).astype(F32)
        p[f"{name}.bn.bias"] = rng.normal(0, 0.1, c).astype(F32)
        p[f"{name}.bn.running_mean"] = rng.normal(0, 0.1, c).astype(F32)
        p[f"{name}.bn.running_var"] = rng.uniform(0.5, 1.5, c).astype(F32)
        p[f"{name}.bn.num_batches_tracked"] = np.asarray(1, np.int64)

    def block(name, cin, cout, k):
        p[f"{name}.conv.weight"] = rng.normal(0, np.sqrt(2.0 / (k * k * cin)), (cout, cin, k, k)).astype(F32)
        bn(name, cout)

    def up(name, cin, cout):
        # a transposed layer's output sums 9 / 4 taps per input channel on average
        p[f"{name}.deconv.conv.weight"] = rng.normal(0, np.sqrt(2.0 / (9 * cin / 4)), (cin, cout, 3, 3)).astype(F32)
        bn(f"{name}.deconv", cout)
        block(f"{name}.conv", 2 * cout, cout, 3)

    b = base
    for name, cin, cout, k in (("conv0.0", 3, b, 3), ("conv0.1", b, b, 3), ("conv1.0", b, 2 * b, 5), ("conv1.1", 2 * b, 2 * b, 3),
                               ("conv1.2", 2 * b, 2 * b, 3), ("conv2.0", 2 * b, 4 * b, 5), ("conv2.1", 4 * b, 4 * b, 3),
                               ("conv2.2", 4 * b, 4 * b, 3)):
        block(name, cin, cout, k)
    p["out1.weight"] = rng.normal(0, np.sqrt(1.0 / (4 * b)), (4 * b, 4 * b, 1, 1)).astype(F32)
    up("deconv1", 4 * b, 2 * b)
    up("deconv2", 2 * b, b)
    p["out2.weight"] = rng.normal(0, np.sqrt(1.0 / (2 * b)), (2 * b, 2 * b, 1, 1)).astype(F32)
    p["out3.weight"] = rng.normal(0, np.sqrt(1.0 / b), (b, b, 1, 1)).astype(F32)
    return p


def make_ucs_costreg_params(seed, in_channels, base=8):
    """synth.make_costreg_params under UCSNet's attribute names (conv7 / 9 / 11 -> deconv7 / 8 / 9)."""
    ren = {"conv7": "deconv7", "conv9": "deconv8", "conv11": "deconv9"}
    return {".".join([ren.get(k.split(".")[0], k.split(".")[0])] + k.split(".")[1:]): v
            for k, v in synth.make_costreg_params(seed, in_channels, base).items()}


def ucsnet_state_dict(seed=FIXTURE_SEED):
    """The whole model's seeded state dict (258 entries)."""
    sd = {f"feature_extraction.{k}": v for k, v in make_featext_params(seed).items()}
    for st, cin in enumerate((32, 16, 8)):
        sd.update({f"cost_regularization.{st}.{k}": v for k, v in make_ucs_costreg_params(seed + 100 + st, cin).items()})
    return sd


def fixture_image(seed=FIXTURE_SEED, hw=FIXTURE_HW):
    return np.random.default_rng([seed, 7]).uniform(0, 1, (3,) + tuple(hw)).astype(F32)


def fixture_sample(seed=FIXTURE_SEED):
    """synth.make_mvs_sample with the features three times as large -> feats, proj, depth_values.  The variance volume then
    is nine times as large and the seeded regulariser's probability has a peak at most pixels: stage 1's uncertainty spans
    16 .. 377 over the image.  The cameras and the depth range cannot do that with these weights: at the plain amplitude the
    logits are so small that the probability is nearly flat whatever is warped -- baselines of 30 .. 600, ranges 425 .. 935,
    150 .. 935 and 60 .. 400 and view angles up to 0.3 rad all leave max / min of stage 1's uncertainty between 1.3 and 1.5."""
    feats, proj, depth_values = synth.make_mvs_sample(seed, img_hw=FIXTURE_HW)
    return [{k: (3.0 * v).astype(F32) for k, v in f.items()} for f in feats], proj, depth_values


def pin_positions(name, n):
    """PIN sampled flat positions of an array of n elements (stored in the fixture beside the values)."""
    seed = int(np.frombuffer(name.encode().ljust(8, b"_")[:8], np.uint32).sum())
    return np.sort(np.random.default_rng([seed, n]).choice(n, PIN, replace=False)).astype(np.int32)


def pinned(g, name, got):
    """(got, want) of fixture entry `name`: the whole array, or its pinned positions."""
    got = np.asarray(got)
    if name in g:
        assert got.shape == g[name].shape, (name, got.shape, g[name].shape)
        return got, g[name]
    assert tuple(g[name + "_shape"]) == got.shape, (name, got.shape)
    return got.reshape(-1)[g[name + "_idx"]], g[name + "_val"]


# ---------------------------------------------------------------------------------------------------------------------
# transposed convolution and the feature extractor
# ---------------------------------------------------------------------------------------------------------------------
def deconv2d_taps(x, w, bias=None, relu=False, dtype=F64):
    """out[co,oy,ox] = sum_ci sum_(ky,kx) x[ci,(oy+1-ky)/2,(ox+1-kx)/2] * w[ci,co,ky,kx] over the taps for which oy+1-ky and
    ox+1-kx are even and in range.  x (Cin,H,W), w (Cin,Cout,3,3) -> (Cout,2H,2W) in `dtype`."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    Cin, H, W = x.shape
    Cout = w.shape[1]
    out = np.zeros((Cout, 2 * H, 2 * W), dtype)
    for ky in range(3):
        for kx in range(3):
            # oy = 2 iy - 1 + ky for every input row iy with 0 <= oy < 2H
            iy = np.arange(H); oy = 2 * iy - 1 + ky
            ix = np.arange(W); ox = 2 * ix - 1 + kx
            iy, oy = iy[(oy >= 0) & (oy < 2 * H)], oy[(oy >= 0) & (oy < 2 * H)]
            ix, ox = ix[(ox >= 0) & (ox < 2 * W)], ox[(ox >= 0) & (ox < 2 * W)]
            out[np.ix_(np.arange(Cout), oy, ox)] += np.einsum("ic,iyx->cyx", w[:, :, ky, kx], x[np.ix_(np.arange(Cin), iy, ix)])
    if bias is not None:
        out += np.asarray(bias, dtype).reshape(-1, 1, 1)
    return np.maximum(out, 0) if relu else out


def fold_bn(p, name, transposed=False):
    """(weight, bias) of block `name` with its BatchNorm (eval, eps 1e-5) folded in, float64"""
    scale = np.asarray(p[f"{name}.bn.weight"], F64) / np.sqrt(np.asarray(p[f"{name}.bn.running_var"], F64) + 1e-5)
    shift = np.asarray(p[f"{name}.bn.bias"], F64) - np.asarray(p[f"{name}.bn.running_mean"], F64) * scale
    w = np.asarray(p[f"{name}.conv.weight"], F64)
    return w * (scale.reshape(1, -1, 1, 1) if transposed else scale.reshape(-1, 1, 1, 1)), shift


def feat_ext_net(params, img, dtype=F64):
    """FeatExtNet.forward (models/ucsnet.py:279-302): img (3,H,W) -> dict of stage1, stage2, stage3 and the two transposed
    layers' raw outputs (before BatchNorm) deconv1_raw, deconv2_raw."""
    import torch
    import torch.nn.functional as Fn
    td = torch.float64 if dtype == F64 else torch.float32
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype)))

    def block(name, x, stride, pad):
        w, b = fold_bn(params, name)
        return Fn.relu(Fn.conv2d(x, T(w), T(b), stride=stride, padding=pad))

    x = T(img)[None].to(td)
    c0 = block("conv0.1", block("conv0.0", x, 1, 1), 1, 1)
    c1 = block("conv1.2", block("conv1.1", block("conv1.0", c0, 2, 2), 1, 1), 1, 1)
    c2 = block("conv2.2", block("conv2.1", block("conv2.0", c1, 2, 2), 1, 1), 1, 1)
    out = {"stage1": Fn.conv2d(c2, T(params["out1.weight"]))[0].numpy()}

    def up(name, x_pre, x):
        raw = deconv2d_taps(x[0].numpy(), params[f"{name}.deconv.conv.weight"], dtype=dtype)
        w, b = fold_bn(params, f"{name}.deconv", transposed=True)
        y = T(deconv2d_taps(x[0].numpy(), w, b, relu=True, dtype=dtype))[None]
        return raw, block(f"{name}.conv", torch.cat((y, x_pre), 1), 1, 1)

    out["deconv1_raw"], f = up("deconv1", c1, c2)
    out["stage2"] = Fn.conv2d(f, T(params["out2.weight"]))[0].numpy()
    out["deconv2_raw"], f = up("deconv2", c0, f)
    out["stage3"] = Fn.conv2d(f, T(params["out3.weight"]))[0].numpy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# hypotheses
# ---------------------------------------------------------------------------------------------------------------------
def _lin_src(n_in, n_out, dtype):
    """PyTorch's align_corners=False source index, clamped at 0 -> i0, i1, t"""
    scale = dtype(n_in) / dtype(n_out)
    src = (np.arange(n_out, dtype=dtype) + dtype(0.5)) * scale - dtype(0.5)
    src = np.maximum(src, dtype(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (src - i0.astype(dtype)).astype(dtype)


def _resize_bilinear(a, hw, dtype):
    a = np.asarray(a, dtype)
    y0, y1, ty = _lin_src(a.shape[0], hw[0], dtype)
    x0, x1, tx = _lin_src(a.shape[1], hw[1], dtype)
    one = dtype(1)
    tx, ty = tx[None, :], ty[:, None]
    top = (one - tx) * a[y0][:, x0] + tx * a[y0][:, x1]
    bot = (one - tx) * a[y1][:, x0] + tx * a[y1][:, x1]
    return ((one - ty) * top + ty * bot).astype(dtype)


def resize_bilinear32(a, hw):
    return _resize_bilinear(a, hw, F32)


def resize_bilinear64(a, hw):
    """float64, cross-checked against torch.nn.functional.interpolate by tests/test_ucsnet_cpu.py"""
    return _resize_bilinear(a, hw, F64)


def _samples(cur, var, D, dtype):
    low = -np.minimum(cur, var)
    step = ((var - low) / dtype(float(D) - 1)).astype(dtype)
    base = (cur + low).astype(dtype)
    return np.stack([((base + step * dtype(i)).astype(dtype) + dtype(EPS)).astype(dtype) for i in range(D)], 0)


def uncertainty_samples32(prev_depth, prev_var, hw, D):
    """(Hp,Wp) maps -> (D,) + hw float32: cur + low + step * i + eps evaluated left to right in float32"""
    assert D > 1
    return _samples(resize_bilinear32(prev_depth, hw), resize_bilinear32(prev_var, hw), D, F32)


def uncertainty_samples64(prev_depth, prev_var, hw, D):
    assert D > 1
    return _samples(resize_bilinear64(prev_depth, hw), resize_bilinear64(prev_var, hw), D, F64)


def stage1_planes(dmin, dmax, D, inverse):
    """models/ucsnet.py:49-56 with torch float32 on the CPU -> (D,) float32"""
    import torch
    lo, hi = torch.tensor([float(dmin)], dtype=torch.float32), torch.tensor([float(dmax)], dtype=torch.float32)
    if inverse:
        z = torch.linspace(0, 1, D)[None, :]
        return (1 / (1 / lo[:, None] * (1 - z) + 1 / hi[:, None] * z))[0].numpy()
    interval = (hi - lo) / (D - 1)
    return (lo.unsqueeze(1) + torch.arange(0, D, dtype=torch.float32).reshape(1, -1) * interval.unsqueeze(1))[0].numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the per-pixel uncertainty
# ---------------------------------------------------------------------------------------------------------------------
def variance64(reg, depth_values, lamb):
    """lamb * sqrt(sum_d p_d (z_d - depth)^2) in float64 on tail64's probabilities and depth -> (H,W)"""
    prob, depth = tref.tail64(reg, depth_values)[:2]
    return float(lamb) * np.sqrt((prob * (np.asarray(depth_values, F64) - depth[None]) ** 2).sum(0))


def variance32(reg, depth_values, lamb):
    """the same formula with every operation in float32 numpy (softmax by exp of the difference to the maximum)"""
    reg, dv = np.asarray(reg, F32), np.asarray(depth_values, F32)
    e = np.exp(reg - reg.max(0, keepdims=True), dtype=F32)
    prob = (e / e.sum(0, keepdims=True, dtype=F32)).astype(F32)
    depth = (prob * dv).sum(0, dtype=F32)
    return (F32(lamb) * np.sqrt(((dv - depth[None]) ** 2 * prob).sum(0, dtype=F32), dtype=F32)).astype(F32)


def variance_floor(depth_values, lamb):
    """What the rounding of the depth alone can leave of a variance that is mathematically zero (a one-hot pixel): the depth
    is a float32 sum good to 3e-6 of the largest hypothesis (the bound tests/test_gpu_costvol.py holds it to) -> (H,W)"""
    return float(lamb) * 3e-6 * np.abs(np.asarray(depth_values, F64)).max(0)
