"""TEST INFRASTRUCTURE ONLY -- plain torch / numpy restatements, on the CPU, of what TransMVSNet does beyond CasMVSNet, written
from the reference's formulas (models/dcn.py, models/FMT.py, models/position_encoding.py, models/TransMVSNet.py,
models/module.py) and not from the kernels.  Every function takes the torch dtype to work in: float64 is the yardstick,
float32 the measure of what float32 arithmetic alone costs (the GPU tests allow a kernel ALLOW_FACTOR times that).

  * deform_conv2d_tv       torchvision.ops.deform_conv2d as models/dcn.py:71-80 calls it: one grid_sample(align_corners=True,
                           zeros padding) per tap in pixel coordinates, then an einsum.  Keeps its input's dtype, so it also
                           stands in for torchvision when tests/golden/make_transmvs_fixture.py runs the reference.
  * deform_conv2d_gather   the same by torchvision's own rule: floor, four weights, a corner outside contributes nothing
  * dcn / feature_net      DCN.forward and FeatureNet.forward (models/module.py:345-423)
  * encoder_layer, fmt_ref, fmt_src, pathway_step, fmt_with_pathway     models/FMT.py
  * similarity_views, pixel_wise_logit, similarity_volume               models/TransMVSNet.py:52-91 on models/module.py:285-324
  * cost_reg               CostRegNet (models/module.py:426-457), BatchNorm in eval form
  * tail_wta               models/TransMVSNet.py:100-109, 225-227

and the seeded parameters / inputs that tests/golden/make_transmvs_fixture.py and the tests share.
"""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

import costvol_tail_ref as tref
import synth

F32 = np.float32
F64 = np.float64
T32, T64 = torch.float32, torch.float64

FIXTURE_SEED = 31
FIXTURE_HW = (64, 96)
FIXTURE_NDEPTHS = (16, 8, 8)
FIXTURE_RATIOS = (4, 2, 1)
PIN = 4000                 # arrays with more than PIN_ABOVE elements are pinned at PIN positions
PIN_ABOVE = 8192
ALLOW_FACTOR = 4.0         # a kernel may be this many times as far from float64 as the float32 restatement is
TIE_CAP = 0.01             # share of pixels whose winner-take-all depth may be left unchecked at any stage


def T(a, td=T64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(td)


def allowance(a32, a64):
    """ALLOW_FACTOR x the largest distance of the float32 restatement from the float64 one"""
    return ALLOW_FACTOR * float(np.abs(np.asarray(a32, F64) - np.asarray(a64, F64)).max())


# ---------------------------------------------------------------------------------------------------------------------
# pinned positions: a fixed multiplicative walk, no random generator (the fixture stores values and shape only)
# ---------------------------------------------------------------------------------------------------------------------
def pin_positions(name, n):
    start = sum(name.encode()) * 7919
    return np.unique((start + np.arange(PIN, dtype=np.int64) * 2654435761) % n)


def put(arr, name, a):
    """store `a` whole, or its pinned values and its shape"""
    a = np.ascontiguousarray(a)
    if a.size > PIN_ABOVE:
        arr[name + "_val"], arr[name + "_shape"] = a.reshape(-1)[pin_positions(name, a.size)], np.asarray(a.shape)
    else:
        arr[name] = a


def pinned(g, name, got):
    """(got, want) of fixture entry `name`: the whole array, or its pinned positions"""
    got = np.asarray(got)
    if name in g:
        assert got.shape == g[name].shape, (name, got.shape, g[name].shape)
        return got, g[name]
    assert tuple(g[name + "_shape"]) == got.shape, (name, got.shape)
    return got.reshape(-1)[pin_positions(name, got.size)], g[name + "_val"]


# ---------------------------------------------------------------------------------------------------------------------
# seeded parameters
# ---------------------------------------------------------------------------------------------------------------------
def _bn(p, rng, name, c):
    p[f"{name}.weight"] = rng.uniform(0.6, 1.4, c).astype(F32)
    p[f"{name}.bias"] = rng.normal(0, 0.1, c).astype(F32)
    p[f"{name}.running_mean"] = rng.normal(0, 0.1, c).astype(F32)
    p[f"{name}.running_var"] = rng.uniform(0.5, 1.5, c).astype(F32)
    p[f"{name}.num_batches_tracked"] = np.asarray(1, np.int64)


def make_featurenet_params(seed):
    """FeatureNet of models/module.py:345-423: the FPN's first eight layers and laterals from synth.make_featurenet_params, the
    three output branches He-scaled.  conv_offset_mask (zero in the reference's initialisation) produces offsets of a few
    pixels and masks spread over (0, 1)."""
    p = {k: v for k, v in synth.make_featurenet_params(seed).items() if k.split(".")[0] not in ("out1", "out2", "out3")}
    rng = np.random.default_rng([seed, 11])
    for name, k, cout in (("out1", 1, 32), ("out2", 3, 16), ("out3", 3, 8)):
        p[f"{name}.0.conv.weight"] = rng.normal(0, np.sqrt(2.0 / (k * k * 32)), (32, 32, k, k)).astype(F32)
        _bn(p, rng, f"{name}.0.bn", 32)
        for i, co in ((1, 32), (4, 32), (7, cout)):
            # He-scaled, times 1.5: the masks average a half
            p[f"{name}.{i}.weight"] = rng.normal(0, 1.5 * np.sqrt(2.0 / (9 * 32)), (co, 32, 3, 3)).astype(F32)
            p[f"{name}.{i}.bias"] = rng.normal(0, 0.1, co).astype(F32)
            w = rng.normal(0, 1.0, (27, 32, 3, 3))
            w[:18] *= 0.12                               # offsets: about 2 px on O(1) features
            w[18:] *= 0.06
            p[f"{name}.{i}.conv_offset_mask.weight"] = w.astype(F32)
            p[f"{name}.{i}.conv_offset_mask.bias"] = np.concatenate([rng.normal(0, 0.5, 18), rng.normal(0, 0.5, 9)]).astype(F32)
            if i != 7:
                _bn(p, rng, f"{name}.{i + 1}", 32)
    return p


def make_fmt_params(seed):
    """FMT_with_pathway of models/FMT.py: LayerNorm gains and biases away from 1 and 0, the pathway's convolutions with a gain
    that keeps every stage's features O(1)."""
    rng = np.random.default_rng([seed, 12])
    p = {}
    for i in range(8):
        pre = f"FMT.layers.{i}"
        for name, cin, cout in (("attention.query_projection", 32, 32), ("attention.key_projection", 32, 32),
                                ("attention.value_projection", 32, 32), ("attention.out_projection", 32, 32),
                                ("linear1", 32, 64), ("linear2", 64, 32)):
            p[f"{pre}.{name}.weight"] = rng.normal(0, np.sqrt(1.0 / cin), (cout, cin)).astype(F32)
            p[f"{pre}.{name}.bias"] = rng.normal(0, 0.1, cout).astype(F32)
        for name in ("norm1", "norm2"):
            p[f"{pre}.{name}.weight"] = rng.uniform(0.6, 1.4, 32).astype(F32)
            p[f"{pre}.{name}.bias"] = rng.normal(0, 0.2, 32).astype(F32)
    p["dim_reduction_1.weight"] = rng.normal(0, np.sqrt(1.0 / 32), (16, 32, 1, 1)).astype(F32)
    p["dim_reduction_2.weight"] = rng.normal(0, np.sqrt(1.0 / 16), (8, 16, 1, 1)).astype(F32)
    p["smooth_1.weight"] = rng.normal(0, np.sqrt(1.0 / (9 * 16)), (16, 16, 3, 3)).astype(F32)
    p["smooth_2.weight"] = rng.normal(0, np.sqrt(1.0 / (9 * 8)), (8, 8, 3, 3)).astype(F32)
    return p


def make_pixelwise_params(seed):
    """PixelwiseNet: default-sized weights times 6, 2 and 6 (the plain ones give every pixel a weight of 0.41)"""
    rng = np.random.default_rng([seed, 13])
    p = {"conv0.conv.weight": (6.0 * rng.uniform(-1, 1, (16, 1, 1, 1, 1))).astype(F32),
         "conv1.conv.weight": (2.0 * rng.uniform(-0.25, 0.25, (8, 16, 1, 1, 1))).astype(F32),
         "conv2.weight": (6.0 * rng.uniform(-0.354, 0.354, (1, 8, 1, 1, 1))).astype(F32),
         "conv2.bias": rng.uniform(-0.354, 0.354, 1).astype(F32)}
    _bn(p, rng, "conv0.bn", 16)
    _bn(p, rng, "conv1.bn", 8)
    return p


def transmvs_state_dict(seed=FIXTURE_SEED):
    """The whole model's seeded state dict (465 entries) under the reference's names."""
    sd = {f"feature.{k}": v for k, v in make_featurenet_params(seed).items()}
    sd.update({f"FMT_with_pathway.{k}": v for k, v in make_fmt_params(seed).items()})
    for st in range(3):
        sd.update({f"cost_regularization.{st}.{k}": v for k, v in synth.make_costreg_params(seed + 100 + st, 1, 8).items()})
    sd.update({f"DepthNet.pixel_wise_net.{k}": v for k, v in make_pixelwise_params(seed).items()})
    return sd


def sub(sd, prefix):
    """the entries below `prefix.` with the prefix removed"""
    return {k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")}


def fixture_image(seed=FIXTURE_SEED, hw=FIXTURE_HW):
    return np.random.default_rng([seed, 7]).uniform(0, 1, (3,) + tuple(hw)).astype(F32)


def fixture_sample(seed=FIXTURE_SEED):
    """synth.make_mvs_sample -> feats (what `feature` would give, per view and stage), proj, depth_values"""
    return synth.make_mvs_sample(seed, img_hw=FIXTURE_HW)


def upsample_nearest2(w, times=1):
    """F.interpolate(scale_factor=2, mode='nearest') of (V,H,W), `times` times (models/TransMVSNet.py:208)"""
    w = np.asarray(w)
    for _ in range(times):
        w = w.repeat(2, axis=-2).repeat(2, axis=-1)
    return w


# ---------------------------------------------------------------------------------------------------------------------
# DCNv2
# ---------------------------------------------------------------------------------------------------------------------
def deform_conv2d_tv(input, offset, weight, bias=None, stride=(1, 1), padding=(1, 1), dilation=(1, 1), mask=None):
    """torchvision.ops.deform_conv2d for 3x3, stride 1, padding 1, dilation 1, one offset group: input (B,C,H,W), offset
    (B,18,H,W) with channels 2k, 2k+1 = dy, dx of tap k = 3 ky + kx, mask (B,9,H,W), in the input's dtype."""
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    assert pair(stride) == (1, 1) and pair(padding) == (1, 1) and pair(dilation) == (1, 1) and tuple(weight.shape[2:]) == (3, 3)
    B, C, H, W = input.shape
    td = input.dtype
    ys = torch.arange(H, dtype=td, device=input.device).view(1, H, 1)
    xs = torch.arange(W, dtype=td, device=input.device).view(1, 1, W)
    cols = []
    for k in range(9):
        ky, kx = divmod(k, 3)
        py = ys + (ky - 1) + offset[:, 2 * k]
        px = xs + (kx - 1) + offset[:, 2 * k + 1]
        grid = torch.stack((2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1), -1)
        s = Fn.grid_sample(input, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        cols.append(s if mask is None else s * mask[:, k:k + 1])
    col = torch.stack(cols, 2)                                        # (B,C,9,H,W)
    out = torch.einsum("ock,bckhw->bohw", weight.reshape(weight.shape[0], C, 9), col)
    return out if bias is None else out + bias.view(1, -1, 1, 1)


def deform_conv2d_gather(x, offset, weight, bias=None, mask=None):
    """The same operation by torchvision's bilinear rule, in float64 numpy: 0 when y <= -1, y >= H, x <= -1 or x >= W; else
    floor, the four corner weights, a corner outside the image contributing 0.  x (C,H,W), offset (18,H,W), mask (9,H,W)."""
    x, offset, weight = np.asarray(x, F64), np.asarray(offset, F64), np.asarray(weight, F64)
    C, H, W = x.shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.zeros((weight.shape[0], H, W))
    for k in range(9):
        ky, kx = divmod(k, 3)
        h = yy + (ky - 1) + offset[2 * k]
        w = xx + (kx - 1) + offset[2 * k + 1]
        inside = (h > -1) & (h < H) & (w > -1) & (w < W)
        h0, w0 = np.floor(h).astype(np.int64), np.floor(w).astype(np.int64)
        lh, lw = h - h0, w - w0
        val = np.zeros((C, H, W))
        for dh, dw, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
            hi, wi = h0 + dh, w0 + dw
            ok = inside & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
            val += np.where(ok, wt, 0.0)[None] * x[:, np.clip(hi, 0, H - 1), np.clip(wi, 0, W - 1)]
        if mask is not None:
            val = val * np.asarray(mask, F64)[k][None]
        out += np.einsum("oc,chw->ohw", weight[:, :, ky, kx], val)
    return out if bias is None else out + np.asarray(bias, F64).reshape(-1, 1, 1)


def dcn_from_raw(x, om, weight, bias=None, scale=None, shift=None, relu=False, td=T64):
    """what svs_deform_conv2d computes: x (32,H,W), om (27,H,W) the raw conv_offset_mask output -> (Cout,H,W) numpy"""
    om = T(om, td)[None]
    out = deform_conv2d_tv(T(x, td)[None], om[:, :18], T(weight, td), None if bias is None else T(bias, td),
                           mask=torch.sigmoid(om[:, 18:]))[0]
    if scale is not None:
        out = out * T(scale, td).view(-1, 1, 1) + T(shift, td).view(-1, 1, 1)
    return (out.clamp(min=0) if relu else out).numpy()


def _fold(p, name, td, eps=1e-5):
    scale = T(p[f"{name}.weight"], T64) / torch.sqrt(T(p[f"{name}.running_var"], T64) + eps)
    return scale.to(td), (T(p[f"{name}.bias"], T64) - T(p[f"{name}.running_mean"], T64) * scale).to(td)


def _block2d(p, name, x, stride, pad, td):
    scale, shift = _fold(p, f"{name}.bn", td)
    y = Fn.conv2d(x, T(p[f"{name}.conv.weight"], td), stride=stride, padding=pad)
    return Fn.relu(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))


def dcn(p, name, x, td):
    """DCN.forward (models/dcn.py:66-80): x (1,32,H,W) torch"""
    om = Fn.conv2d(x, T(p[f"{name}.conv_offset_mask.weight"], td), T(p[f"{name}.conv_offset_mask.bias"], td), padding=1)
    o1, o2, m = torch.chunk(om, 3, dim=1)
    return deform_conv2d_tv(x, torch.cat((o1, o2), 1), T(p[f"{name}.weight"], td), T(p[f"{name}.bias"], td), mask=torch.sigmoid(m))


def feature_net(p, img, td=T64):
    """FeatureNet.forward: img (3,H,W) -> {'stage1','stage2','stage3'} numpy"""
    x = T(img, td)[None]
    c0 = _block2d(p, "conv0.1", _block2d(p, "conv0.0", x, 1, 1, td), 1, 1, td)
    c1 = _block2d(p, "conv1.2", _block2d(p, "conv1.1", _block2d(p, "conv1.0", c0, 2, 2, td), 1, 1, td), 1, 1, td)
    c2 = _block2d(p, "conv2.2", _block2d(p, "conv2.1", _block2d(p, "conv2.0", c1, 2, 2, td), 1, 1, td), 1, 1, td)

    def branch(name, x, k):
        x = _block2d(p, f"{name}.0", x, 1, k // 2, td)
        for i in (1, 4):
            scale, shift = _fold(p, f"{name}.{i + 1}", td)
            x = Fn.relu(dcn(p, f"{name}.{i}", x, td) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
        return dcn(p, f"{name}.7", x, td)

    out = {"stage1": branch("out1", c2, 1)}
    f = Fn.interpolate(c2, scale_factor=2, mode="nearest") + Fn.conv2d(c1, T(p["inner1.weight"], td), T(p["inner1.bias"], td))
    out["stage2"] = branch("out2", f, 3)
    f = Fn.interpolate(f, scale_factor=2, mode="nearest") + Fn.conv2d(c0, T(p["inner2.weight"], td), T(p["inner2.bias"], td))
    out["stage3"] = branch("out3", f, 3)
    return {k: v[0].numpy() for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# Feature Matching Transformer
# ---------------------------------------------------------------------------------------------------------------------
def pos_encoding(H, W, td=T64):
    """PositionEncodingSine(32, temp_bug_fix=True)[:, :H, :W]: positions count from 1 -> (32,H,W) torch"""
    pe = torch.zeros(32, H, W, dtype=td)
    y = torch.ones(H, W, dtype=td).cumsum(0)[None]
    x = torch.ones(H, W, dtype=td).cumsum(1)[None]
    div = torch.exp(torch.arange(0, 16, 2, dtype=td) * (-math.log(10000.0) / 16))[:, None, None]
    pe[0::4], pe[1::4], pe[2::4], pe[3::4] = torch.sin(x * div), torch.cos(x * div), torch.sin(y * div), torch.cos(y * div)
    return pe


def tokens(chw, td=T64, pe=False):
    """(32,H,W) numpy -> (H*W,32) torch, with the position encoding added when asked"""
    x = T(chw, td)
    if pe:
        x = x + pos_encoding(x.shape[1], x.shape[2], td)
    return x.reshape(32, -1).t().contiguous()


def kv_sums(source, p, td=T64):
    """LinearAttention's sums over the source tokens (S,32): KV (8,4,4) [h][m][d] and Ksum (8,4) [h][d]"""
    lin = lambda n: source @ T(p[f"attention.{n}.weight"], td).t() + T(p[f"attention.{n}.bias"], td)
    K = Fn.elu(lin("key_projection").view(-1, 8, 4)) + 1
    V = lin("value_projection").view(-1, 8, 4)
    return torch.einsum("shd,shm->hmd", K, V), K.sum(0)


def encoder_layer(x, source, p, td=T64):
    """EncoderLayer.forward (models/FMT.py:96-111) with LinearAttention (:22-37): x (L,32), source (S,32) torch -> (L,32)"""
    W = lambda n: T(p[n], td)
    KV, Ksum = kv_sums(source, p, td)
    Q = Fn.elu((x @ W("attention.query_projection.weight").t() + W("attention.query_projection.bias")).view(-1, 8, 4)) + 1
    Z = 1 / (torch.einsum("lhd,hd->lh", Q, Ksum) + 1e-6)
    att = torch.einsum("lhd,hmd,lh->lhm", Q, KV, Z).reshape(-1, 32)
    x = x + att @ W("attention.out_projection.weight").t() + W("attention.out_projection.bias")
    x = Fn.layer_norm(x, (32,), W("norm1.weight"), W("norm1.bias"), 1e-5)
    y = Fn.relu(x @ W("linear1.weight").t() + W("linear1.bias")) @ W("linear2.weight").t() + W("linear2.bias")
    return Fn.layer_norm(x + y, (32,), W("norm2.weight"), W("norm2.bias"), 1e-5)


def fmt_ref(p, feature, td=T64):
    """FMT.forward(feat='ref'): (32,H,W) -> the four self layers' outputs as (L,32) torch tokens"""
    x = tokens(feature, td, pe=True)
    outs = []
    for i in (0, 2, 4, 6):
        x = encoder_layer(x, x, sub(p, f"FMT.layers.{i}"), td)
        outs.append(x)
    return outs


def fmt_src(p, ref_tokens, feature, td=T64):
    """FMT.forward(feat='src'): all eight layers, layer 2i+1 reads the reference's i-th output -> (L,32) torch tokens"""
    x = tokens(feature, td, pe=True)
    for i in range(8):
        x = encoder_layer(x, x if i % 2 == 0 else ref_tokens[i // 2], sub(p, f"FMT.layers.{i}"), td)
    return x


def untokens(t, hw):
    return t.t().reshape(32, *hw).numpy()


def pathway_step(x, weight, y, td=T64):
    """_upsample_add(dim_reduction(x), y): x (Cin,h,w), weight (Cin/2,Cin,1,1), y (Cin/2,2h,2w) -> numpy"""
    r = Fn.conv2d(T(x, td)[None], T(weight, td))
    return (Fn.interpolate(r, size=tuple(np.shape(y)[-2:]), mode="bilinear") + T(y, td)[None])[0].numpy()


def fmt_with_pathway(p, feats, td=T64):
    """FMT_with_pathway.forward on per-view dicts of (C,H,W) arrays -> (new per-view dicts, the reference view's four outputs
    as (32,H,W) arrays)"""
    out, ref_tokens = [], None
    for v, f in enumerate(feats):
        hw = f["stage1"].shape[-2:]
        if v == 0:
            ref_tokens = fmt_ref(p, f["stage1"], td)
            s1 = untokens(ref_tokens[-1], hw)
        else:
            s1 = untokens(fmt_src(p, ref_tokens, f["stage1"], td), hw)
        smooth = lambda x, n: Fn.conv2d(T(x, td)[None], T(p[n], td), padding=1)[0].numpy()
        s2 = smooth(pathway_step(s1, p["dim_reduction_1.weight"], f["stage2"], td), "smooth_1.weight")
        s3 = smooth(pathway_step(s2, p["dim_reduction_2.weight"], f["stage3"], td), "smooth_2.weight")
        out.append({"stage1": s1, "stage2": s2, "stage3": s3})
    return out, [untokens(t, feats[0]["stage1"].shape[-2:]) for t in ref_tokens]


# ---------------------------------------------------------------------------------------------------------------------
# similarity cost volume
# ---------------------------------------------------------------------------------------------------------------------
def relative(src_proj, ref_proj):
    """(2,4,4) projection pairs -> rot (3,3), trans (3,) of src @ inv(ref), K @ [R|t] formed first (float64)"""
    def comb(P):
        P = np.asarray(P, F64)
        out = P[0].copy()
        out[:3, :4] = P[1][:3, :3] @ P[0][:3, :4]
        return out
    rel = comb(src_proj) @ np.linalg.inv(comb(ref_proj))
    return rel[:3, :3], rel[:3, 3]


def homo_warp(src, rot, trans, depth_values, td=T64):
    """models/module.py:285-324: src (C,H,W), depth_values (D,H,W) -> (C,D,H,W) torch.  align_corners=True; a hypothesis whose
    projected z is below 1e-6 gets both grid coordinates set to -99 and samples 0."""
    src, dv = T(src, td), T(depth_values, td)
    C, H, W = src.shape
    D = dv.shape[0]
    rot, trans = T(rot, td), T(trans, td)
    y, x = torch.meshgrid(torch.arange(H, dtype=td), torch.arange(W, dtype=td), indexing="ij")
    xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(H * W, dtype=td)))
    proj = (rot @ xyz)[:, None, :] * dv.view(1, D, -1) + trans.view(3, 1, 1)
    invalid = proj[2] < 1e-6
    xy = proj[:2] / proj[2:3]
    gx = xy[0] / ((W - 1) / 2) - 1
    gy = xy[1] / ((H - 1) / 2) - 1
    gx[invalid] = -99.0
    gy[invalid] = -99.0
    grid = torch.stack((gx, gy), -1).view(1, D * H, W, 2)
    return Fn.grid_sample(src[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(C, D, H, W)


def similarity_views(feats, proj, depth_values, td=T64):
    """per source view, mean over the channels of warped * ref: feats list of (C,H,W), proj (V,2,4,4) -> list of (D,H,W) torch"""
    ref = T(feats[0], td)
    out = []
    for v in range(1, len(feats)):
        rot, trans = relative(proj[v], proj[0])
        out.append((homo_warp(feats[v], rot, trans, depth_values, td) * ref[:, None]).mean(0))
    return out


def pixel_wise_logit(p, sim, td=T64):
    """PixelwiseNet before its sigmoid, on a (D,H,W) torch similarity"""
    x = sim[None, None]
    for name in ("conv0", "conv1"):
        scale, shift = _fold(p, f"{name}.bn", td)
        x = Fn.relu(Fn.conv3d(x, T(p[f"{name}.conv.weight"], td)) * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1))
    return Fn.conv3d(x, T(p["conv2.weight"], td), T(p["conv2.bias"], td))[0, 0]


def similarity_volume(feats, proj, depth_values, prev_weights, pw_params, td=T64):
    """DepthNet.forward steps 1-2: -> similarity (D,H,W), view weights (V-1,H,W) at this stage's size (numpy).  prev_weights
    None: the weights are max_d sigmoid(net(sim_v)); else (V-1,H/2,W/2), up-sampled nearest x2."""
    sims = similarity_views(feats, proj, depth_values, td)
    if prev_weights is None:
        weights = [torch.sigmoid(pixel_wise_logit(pw_params, s, td)).max(0)[0] for s in sims]
    else:
        weights = [w for w in T(upsample_nearest2(prev_weights), td)]
    num, den = 0, 1e-5
    for s, w in zip(sims, weights):
        num = num + s * w[None]
        den = den + w
    return (num / den[None]).numpy(), torch.stack(weights).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# regularisation and tail
# ---------------------------------------------------------------------------------------------------------------------
def cost_reg(p, x, td=T64):
    """CostRegNet.forward (models/module.py:448-457): x (Cin,D,H,W) -> logits (D,H,W) numpy"""
    def block(name, x, stride=1, transposed=False):
        scale, shift = _fold(p, f"{name}.bn", td)
        w = T(p[f"{name}.conv.weight"], td)
        y = (Fn.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1) if transposed
             else Fn.conv3d(x, w, stride=stride, padding=1))
        return Fn.relu(y * scale.view(1, -1, 1, 1, 1) + shift.view(1, -1, 1, 1, 1))
    x = T(x, td)[None]
    c0 = block("conv0", x)
    c2 = block("conv2", block("conv1", c0, 2))
    c4 = block("conv4", block("conv3", c2, 2))
    y = block("conv6", block("conv5", c4, 2))
    y = c4 + block("conv7", y, transposed=True)
    y = c2 + block("conv9", y, transposed=True)
    y = c0 + block("conv11", y, transposed=True)
    return Fn.conv3d(y, T(p["prob.weight"], td), padding=1)[0, 0].numpy()


def tail_wta(reg, depth_values):
    """float64: prob (D,H,W), index = the first argmax of the logits (H,W), depth = depth_values[index], conf = prob[index]"""
    prob = tref.tail64(reg, depth_values)[0]
    idx = np.argmax(np.asarray(reg, F64), 0)
    take = lambda a: np.take_along_axis(np.asarray(a, F64), idx[None], 0)[0]
    return prob, idx, take(depth_values), take(prob)


def top_two_gap(reg):
    """the distance between the two largest logits of every pixel (H,W), float64"""
    s = np.sort(np.asarray(reg, F64), 0)
    return s[-1] - s[-2]


def hypotheses(prev_depth, st, depth_values, int_r):
    """the stage's hypotheses (D,h,w) in float64: tref.hypotheses64 with the arguments TransMVSNet.forward:171-223 forms"""
    dv = np.asarray(depth_values, F64)
    H, W = FIXTURE_HW
    interval = (dv[-1] - dv[0]) / dv.size
    return tref.hypotheses64(prev_depth, (H, W), FIXTURE_NDEPTHS[st], (4, 2, 1)[st], dv[0], dv[-1],
                             0.0 if prev_depth is None else int_r * interval, False)
