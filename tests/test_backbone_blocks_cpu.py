"""models/blocks.py without a GPU: every BatchNorm fold against eval-mode BatchNorm in float64, the fold cache's invalidation,
every `.folded()` of the three seeded checkpoints against the formulas the backbones carried before they shared one, and the
bound below which costvol.warp_variance chooses the split form.

The fold's tolerance is derived, not tuned.  With u = 2^-24 (float32 unit round-off): scale = g / sqrt(var + eps) carries the
roundings of the sum (u), the root (u / 2) and the quotient (u), and the folded weight w * scale one more: 3.5 u, taken as 4 u.
A folded bias fl(fl(b * scale) + fl(beta - fl(mean * scale))) is off by at most 4 u (|mean scale| + |b scale|) for the products,
u |shift| for the difference and u |bias| for the sum.  A layer's output then differs from float64 BatchNorm by at most
4 u conv(|x|, |w scale|) plus the bias term."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn

import synth
import transmvs_oracle as to
import ucsnet_oracle as uo

U = 2.0 ** -24


def _randomise(module, seed):
    """non-trivial parameters and BatchNorm statistics"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm3d)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) * 1.5 + 0.25)
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen))
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=gen) * 2 + 0.05)
            elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d, nn.Conv3d, nn.ConvTranspose3d)):
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen))
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=gen))
    return module.eval()


def _bn64(bn):
    """(scale, shift, mean) of eval-mode BatchNorm in float64"""
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return scale.detach(), (bn.bias.double() - bn.running_mean.double() * scale).detach(), bn.running_mean.double()


def _bias_bound(bn, conv_bias=None):
    scale, shift, mean = _bn64(bn)
    b = torch.zeros_like(scale) if conv_bias is None else conv_bias.detach().double()
    return 4 * U * ((mean * scale).abs() + (b * scale).abs()) + U * shift.abs() + U * (b * scale + shift).abs()


def _blocks():
    """name -> (module, op(x, w, b) in float64, weight (Cout first or the op's layout) from folded(), channel axis of Cout, x)"""
    from models.blocks import Conv2d
    from models.CasMVSNet import Conv3d, Deconv3d
    from models.ucsnet import Deconv2dUnit
    gen = torch.Generator().manual_seed(5)
    x2, x3 = torch.randn(1, 3, 7, 9, generator=gen).double(), torch.randn(1, 3, 4, 5, 6, generator=gen).double()
    from_rows = lambda w: w.reshape(w.shape[0], 3, 3, 3, w.shape[2])          # [Cin][27][Cout] -> (Cin,3,3,3,Cout)
    return {
        "conv2d": (Conv2d(3, 5, 3, 1, padding=1), lambda x, w, b: Fn.conv2d(x, w, b, padding=1), lambda w: w, 0, x2),
        "conv2d_s2_k5": (Conv2d(3, 4, 5, stride=2, padding=2), lambda x, w, b: Fn.conv2d(x, w, b, stride=2, padding=2),
                         lambda w: w, 0, x2),
        "conv2d_bias_no_bn": (Conv2d(3, 5, 3, 1, bn=False, padding=1), lambda x, w, b: Fn.conv2d(x, w, b, padding=1),
                              lambda w: w, 0, x2),
        "deconv2d": (Deconv2dUnit(3, 5), lambda x, w, b: Fn.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1),
                     lambda w: w, 1, x2),
        "conv3d": (Conv3d(3, 5), lambda x, w, b: Fn.conv3d(x, w, b, padding=1), lambda w: from_rows(w).permute(4, 0, 1, 2, 3), 0, x3),
        "conv3d_s2": (Conv3d(3, 4, stride=2), lambda x, w, b: Fn.conv3d(x, w, b, stride=2, padding=1),
                      lambda w: from_rows(w).permute(4, 0, 1, 2, 3), 0, x3),
        "deconv3d": (Deconv3d(3, 5), lambda x, w, b: Fn.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1),
                     lambda w: from_rows(w).permute(0, 4, 1, 2, 3), 1, x3),
    }


@pytest.mark.parametrize("name", ["conv2d", "conv2d_s2_k5", "conv2d_bias_no_bn", "deconv2d", "conv3d", "conv3d_s2", "deconv3d"])
def test_fold_is_eval_batchnorm_in_float64(name):
    block, op, to_op_layout, cout_axis, x = _blocks()[name]
    _randomise(block, 11)
    w, b = block.folded()
    assert w.dtype == torch.float32 and w.is_contiguous() and (b is None or b.dtype == torch.float32)
    got = op(x, to_op_layout(w).double(), None if b is None else b.double())
    ref64 = copy.deepcopy(block).double()
    want = op(x, ref64.conv.weight, ref64.conv.bias)
    if block.bn is not None:
        want = ref64.bn(want)
        scale, _, _ = _bn64(block.bn)
        shape = [1] * block.conv.weight.dim()
        shape[cout_axis] = -1
        w_exact = block.conv.weight.detach().double() * scale.view(shape)
        bound = 4 * U * op(x.abs(), w_exact.abs(), None) + _bias_bound(block.bn, block.conv.bias).view([1, -1] + [1] * (x.dim() - 2))
    else:
        bound = torch.zeros_like(want)                   # no BatchNorm: the fold is the layer's own float32 parameters
    err = (got - want.detach()).abs()
    print(f"{name}: max err {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


def test_fold_bn_is_eval_batchnorm_in_float64():
    from models.blocks import fold_bn
    bn = _randomise(nn.BatchNorm2d(16), 3)
    scale, shift = fold_bn(bn)
    s64, t64, mean = _bn64(bn)
    assert scale.dtype == shift.dtype == torch.float32
    assert bool(((scale.double() - s64).abs() <= 2.5 * U * s64.abs()).all())
    assert bool(((shift.double() - t64).abs() <= 3.5 * U * (mean * s64).abs() + U * t64.abs()).all())


def _pixelwise64(net, s):
    """models/TransMVSNet.py:17-28 before the sigmoid, through the modules in float64"""
    m = copy.deepcopy(net).double().eval()
    x = s.view(1, 1, 1, 1, -1)
    x = torch.relu(m.conv0.bn(m.conv0.conv(x)))
    x = torch.relu(m.conv1.bn(m.conv1.conv(x)))
    return m.conv2(x).reshape(-1)


def test_pixelwise_fold_is_the_net_in_float64():
    from models.transmvs import PixelwiseNet
    net = _randomise(PixelwiseNet(), 17)
    f = net.folded()
    assert f.dtype == torch.float32 and f.shape == (177,) and f.is_contiguous()
    f = f.double()
    w0, t0, w1, t1, w2, b2 = f[:16], f[16:32], f[32:160].view(8, 16), f[160:168], f[168:176], f[176]
    s = torch.linspace(-3, 3, 41, dtype=torch.float64)
    a0 = torch.relu(w0[:, None] * s + t0[:, None])
    a1 = torch.relu(w1 @ a0 + t1[:, None])
    got = w2 @ a1 + b2
    want = _pixelwise64(net, s).detach()
    # the bound, layer by layer (relu does not enlarge an error; conv2 is not folded: exact)
    s0, _, _ = _bn64(net.conv0.bn)
    s1, _, _ = _bn64(net.conv1.bn)
    e0 = 4 * U * (net.conv0.conv.weight.double().reshape(16) * s0).abs()[:, None] * s.abs() + _bias_bound(net.conv0.bn)[:, None]
    w1x = net.conv1.conv.weight.double().reshape(8, 16) * s1[:, None]
    e1 = w1.abs() @ e0 + 4 * U * (w1x.abs() @ a0.abs()) + _bias_bound(net.conv1.bn)[:, None]
    bound = (w2.abs() @ e1).detach()
    err = (got - want).abs()
    print(f"pixelwise: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------------------------------------------------------------
# cache invalidation
def _flat(v):
    return [t for t in (v if isinstance(v, tuple) else (v,)) if t is not None]


@pytest.mark.parametrize("name", ["conv2d", "conv2d_bias_no_bn", "deconv2d", "conv3d", "deconv3d", "pixelwise"])
def test_cached_fold_invalidation(name):
    if name == "pixelwise":
        from models.transmvs import PixelwiseNet
        block = PixelwiseNet()
        written = block.conv1.bn.running_var
    else:
        block = _blocks()[name][0]
        written = block.conv.weight if block.bn is None else block.bn.running_mean
    _randomise(block, 2)
    first = block.folded()
    assert block.folded() is first                                      # by identity on a second call
    before = [t.clone() for t in _flat(first)]                          # (without BatchNorm the fold aliases the parameters)
    with torch.no_grad():
        written.add_(0.5)                                               # an in-place parameter update
    second = block.folded()
    assert second is not first
    assert any(not torch.equal(a, b) for a, b in zip(before, _flat(second)))
    assert block.folded() is second
    other = _randomise(copy.deepcopy(block), 9)
    block.load_state_dict(other.state_dict(), strict=True)
    third = block.folded()
    assert third is not second
    for a, b in zip(_flat(third), _flat(other.folded())):
        assert torch.equal(a, b)


def test_cached_fold_sees_a_replaced_tensor():
    from models.blocks import CachedFold
    fold, calls = CachedFold(), []
    make = lambda: calls.append(1) or len(calls)
    t = torch.zeros(3)
    assert fold([t], make) == 1 and fold([t], make) == 1
    assert fold([torch.zeros(3)], make) == 2                            # another tensor (another address)
    assert fold([t, t], make) == 3                                      # another dependency list


# ---------------------------------------------------------------------------------------------------------------------
# the seeded checkpoints: every .folded() against the formulas the backbones carried before models/blocks.py
def _parent_folded(m):
    from models.blocks import Conv2d
    from models.CasMVSNet import _Block3d
    from models.transmvs import PixelwiseNet
    from models.ucsnet import Deconv2dUnit
    if isinstance(m, Conv2d):                                           # CasMVSNet.Conv2d.folded
        w = m.conv.weight.detach().float()
        b = m.conv.bias.detach().float() if m.conv.bias is not None else None
        if m.bn is not None:
            scale = (m.bn.weight / torch.sqrt(m.bn.running_var + m.bn.eps)).detach().float()
            shift = (m.bn.bias - m.bn.running_mean * scale).detach().float()
            w = w * scale.view(-1, 1, 1, 1)
            b = shift if b is None else b * scale + shift
        return w.contiguous(), b.contiguous() if b is not None else None
    if isinstance(m, _Block3d):                                         # CasMVSNet._Block3d.folded
        scale = m.bn.weight / torch.sqrt(m.bn.running_var + m.bn.eps)
        shift = m.bn.bias - m.bn.running_mean * scale
        w = m.conv.weight.detach()
        if m.transposed:
            w = w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], 27, w.shape[1])
        else:
            w = w.permute(1, 2, 3, 4, 0).reshape(w.shape[1], 27, w.shape[0])
        return (w * scale.view(1, 1, -1)).contiguous().float(), shift.detach().contiguous().float()
    if isinstance(m, Deconv2dUnit):                                     # ucsnet.Deconv2dUnit.folded
        scale = (m.bn.weight / torch.sqrt(m.bn.running_var + m.bn.eps)).detach().float()
        shift = (m.bn.bias - m.bn.running_mean * scale).detach().float()
        return (m.conv.weight.detach().float() * scale.view(1, -1, 1, 1)).contiguous(), shift.contiguous()
    if isinstance(m, PixelwiseNet):                                     # transmvs.PixelwiseNet.folded with transmvs._fold_bn
        def fold(bn):
            scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().float()
            return scale.contiguous(), (bn.bias - bn.running_mean * scale).detach().float().contiguous()
        s0, t0 = fold(m.conv0.bn)
        s1, t1 = fold(m.conv1.bn)
        w0 = m.conv0.conv.weight.detach().float().reshape(16) * s0
        w1 = m.conv1.conv.weight.detach().float().reshape(8, 16) * s1[:, None]
        return torch.cat([w0, t0, w1.reshape(-1), t1, m.conv2.weight.detach().float().reshape(8),
                          m.conv2.bias.detach().float().reshape(1)]).contiguous()
    return None


def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _casmvs(golden_dir):
    from models.CasMVSNet import CascadeMVSNet
    import os
    g = dict(np.load(os.path.join(golden_dir, "casmvs_3stage.npz")))
    m = CascadeMVSNet(refine=False, ndepths=[int(x) for x in g["ndepths"]], depth_interals_ratio=[1.0, 0.5, 0.5], share_cr=False,
                      cr_base_chs=[8, 8, 8], grad_method="detach")
    m.feature.load_state_dict(_tensors(synth.make_featurenet_params(int(g["seed"]))), strict=True)
    for st, cin in enumerate((32, 16, 8)):
        m.cost_regularization[st].load_state_dict(_tensors(synth.make_costreg_params(100 + st, cin)), strict=True)
    return m


def _ucsnet(golden_dir):
    from models.ucsnet import UCSNetHip
    import os
    g = dict(np.load(os.path.join(golden_dir, "ucsnet_3stage.npz")))
    m = UCSNetHip(lamb=float(g["lamb"]), stage_configs=[int(x) for x in g["ndepths"]], grad_method="detach", base_chs=[8, 8, 8],
                  feat_ext_ch=8)
    m.load_state_dict(_tensors(uo.ucsnet_state_dict(int(g["seed"]))), strict=True)
    return m


def _transmvs(golden_dir):
    from models.transmvs import TransMVSNetHip
    import os
    g = dict(np.load(os.path.join(golden_dir, "transmvs_3stage.npz")))
    m = TransMVSNetHip(refine=False, ndepths=[int(x) for x in g["ndepths"]], depth_interals_ratio=[int(x) for x in g["ratios"]],
                       share_cr=False, grad_method="detach", arch_mode="fpn", cr_base_chs=[8, 8, 8])
    m.load_state_dict(_tensors(to.transmvs_state_dict(int(g["seed"]))), strict=True)
    return m


@pytest.mark.parametrize("make,count", [(_casmvs, 8 + 3 * 10), (_ucsnet, 8 + 4 + 3 * 10), (_transmvs, 8 + 3 + 3 * 10 + 1)])
def test_checkpoint_folds_are_the_parents(golden_dir, make, count):
    model = make(golden_dir).eval()
    n = 0
    for name, m in model.named_modules():
        if not hasattr(m, "folded"):
            continue
        want = _parent_folded(m)
        assert want is not None, f"{name}: a .folded() this test has no formula for"
        got = m.folded()
        for a, b in zip(_flat(got), _flat(want)):
            assert a.dtype == b.dtype and torch.equal(a, b), name
        assert len(_flat(got)) == len(_flat(want)), name
        n += 1
    assert n == count
    from models.blocks import fold_bn
    from models import transmvs
    assert transmvs._fold_bn is fold_bn


# ---------------------------------------------------------------------------------------------------------------------
# the split form's bound (size functions only: nothing is allocated)
def test_split_form_bound():
    from svs_hip import costvol, lib
    L = lib.load()
    big, small = (32, 200, 1200, 1600), (32, 48, 144, 192)
    assert L.svs_split_volume_dims(*big, None) >= 1 << 32              # 6.3 GB as fp16 hi / mid pieces
    assert not costvol.split_fits(*big)
    assert 0 < L.svs_split_volume_dims(*small, None) < 1 << 32
    assert costvol.split_fits(*small)
