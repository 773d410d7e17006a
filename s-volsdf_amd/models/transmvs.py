"""TransMVSNet with the reference's constructor, parameter names and forward() contract (models/TransMVSNet.py:118-232), on the
HIP kernels: the FPN's first eight layers (svs_conv2d), the nine modulated deformable convolutions of the three output
branches (svs_deform_conv2d, csrc/svs_transmvs.hip), the Feature Matching Transformer (svs_fmt_kv / svs_fmt_layer) with its
pathway (svs_pathway_step), the similarity cost volume with learned per-pixel view weights (svs_warp_similarity), CasMVSNet's
regularisation network on one input channel and the winner-take-all tail (svs_prob_wta).  A checkpoint of the reference loads
with strict=True (465 entries for refine=False, share_cr=False).  Inference only, batch 1, three stages, like models/ucsnet.py.

The module has a name of its own: the reference's file is models/TransMVSNet.py, and the drop-in boundary
(tests/test_dropin_imports.py) keeps that name for the reference's class.  `models.transmvs.TransMVSNet` is
always the mirror: the reference's file needs torchvision and relative imports and cannot be loaded beside this package.
"""
import torch
import torch.nn as nn

from svs_hip import costvol
from models.blocks import (CachedFold, Conv2d, bn_tensors, encoder_trunk, fold_bn, range_hypotheses, stack_stages,
                           stage_inputs)
from models.CasMVSNet import CostRegNet

Align_Corners_Range = False
_fold_bn = fold_bn


# ---------------------------------------------------------------------------------------------------------------------
# FeatureNet (models/module.py:345-423) with the DCN of models/dcn.py
# ---------------------------------------------------------------------------------------------------------------------
class DCN(nn.Module):
    """models/dcn.py:15-80 for the one configuration the network uses (3x3, stride 1, padding 1, one deformable group):
    `weight`, `bias`, `conv_offset_mask.{weight,bias}`.  forward(x, bn, relu) folds the BatchNorm and ReLU that follow six of
    the nine layers into the kernel's epilogue."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, deformable_groups=1):
        super().__init__()
        if (kernel_size, stride, padding, dilation, deformable_groups) != (3, 1, 1, 1, 1) or in_channels != 32:
            raise NotImplementedError("the DCN kernel is declared for 32 input channels, 3x3, stride 1, padding 1, one group")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.conv_offset_mask = nn.Conv2d(in_channels, 27, 3, stride=1, padding=1, bias=True)
        bound = 1.0 / (in_channels * 9) ** 0.5
        nn.init.uniform_(self.weight, -bound, bound)
        nn.init.zeros_(self.conv_offset_mask.weight)
        nn.init.zeros_(self.conv_offset_mask.bias)
        self._bn_fold = CachedFold()

    def forward(self, x, bn=None, relu=False):
        """x (32,H,W) on the device -> (Cout,H,W)"""
        om = costvol.conv2d(x, self.conv_offset_mask.weight.detach(), self.conv_offset_mask.bias.detach())
        scale, shift = self._bn_fold(bn_tensors(bn), lambda: fold_bn(bn)) if bn is not None else (None, None)
        return costvol.deform_conv2d(x, om, self.weight.detach(), self.bias.detach(), scale, shift, relu=relu)


def _out_branch(k, cout):
    """out1 / out2 / out3: Conv-BN-ReLU, then DCN-BN-ReLU twice, then a DCN (models/module.py:364-397)"""
    return nn.Sequential(Conv2d(32, 32, k, 1, padding=k // 2), DCN(32, 32), nn.BatchNorm2d(32), nn.ReLU(inplace=True),
                         DCN(32, 32), nn.BatchNorm2d(32), nn.ReLU(inplace=True), DCN(32, cout))


class FeatureNet(nn.Module):
    def __init__(self, base_channels):
        super().__init__()
        if base_channels != 8:
            raise NotImplementedError("base_channels 8 (the DCN kernel takes 32 input channels)")
        b = base_channels
        self.base_channels = b
        self.conv0, self.conv1, self.conv2 = encoder_trunk(b)
        self.out1 = _out_branch(1, 4 * b)
        self.inner1 = nn.Conv2d(2 * b, 4 * b, 1, bias=True)
        self.inner2 = nn.Conv2d(b, 4 * b, 1, bias=True)
        self.out2 = _out_branch(3, 2 * b)
        self.out3 = _out_branch(3, b)
        self.out_channels = [4 * b, 2 * b, b]

    @staticmethod
    def _branch(seq, x):
        x = seq[0](x[None])[0]
        x = seq[1](x, bn=seq[2], relu=True)
        x = seq[4](x, bn=seq[5], relu=True)
        return seq[7](x)

    def forward(self, x):
        if self.training:
            raise NotImplementedError("TransMVSNet is inference-only in S-VolSDF (runner.py:153); call .eval()")
        if not x.is_cuda:
            raise NotImplementedError("the feature extractor runs on the HIP kernels: device tensors only")
        if x.shape[-2] % 4 or x.shape[-1] % 4:
            raise ValueError("image height and width must be multiples of 4")
        per_image = []
        for xi in x:
            c0 = self.conv0(xi[None])
            c1 = self.conv1(c0)
            c2 = self.conv2(c1)
            s1 = self._branch(self.out1, c2[0])
            # the FPN's top-down path: nearest x2 plus the lateral 1x1 convolution, in one launch
            f = costvol.conv2d(c1[0], self.inner1.weight.detach(), self.inner1.bias.detach(), add=c2[0], add_upsample2=True)
            s2 = self._branch(self.out2, f)
            f = costvol.conv2d(c0[0], self.inner2.weight.detach(), self.inner2.bias.detach(), add=f, add_upsample2=True)
            s3 = self._branch(self.out3, f)
            per_image.append((s1, s2, s3))
        return stack_stages(per_image)


# ---------------------------------------------------------------------------------------------------------------------
# Feature Matching Transformer with its pathway (models/FMT.py)
# ---------------------------------------------------------------------------------------------------------------------
class AttentionLayer(nn.Module):
    def __init__(self, d_model, n_heads):
        super().__init__()
        self.query_projection = nn.Linear(d_model, d_model)
        self.key_projection = nn.Linear(d_model, d_model)
        self.value_projection = nn.Linear(d_model, d_model)
        self.out_projection = nn.Linear(d_model, d_model)
        self.n_heads = n_heads


class EncoderLayer(nn.Module):
    def __init__(self, d_model, n_heads):
        super().__init__()
        self.attention = AttentionLayer(d_model, n_heads)
        self.linear1 = nn.Linear(d_model, 2 * d_model)
        self.linear2 = nn.Linear(2 * d_model, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)

    def forward(self, x, source):
        """x (L,32), source (S,32) tokens -> (L,32) (models/FMT.py:96-111)"""
        at = self.attention
        kv = costvol.fmt_kv(source, at.key_projection.weight, at.key_projection.bias, at.value_projection.weight,
                            at.value_projection.bias)
        return costvol.fmt_layer(x, kv, [at.query_projection.weight, at.query_projection.bias, at.out_projection.weight,
                                         at.out_projection.bias, self.linear1.weight, self.linear1.bias, self.linear2.weight,
                                         self.linear2.bias, self.norm1.weight, self.norm1.bias, self.norm2.weight, self.norm2.bias])


class FMT(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.d_model, self.nhead, self.layer_names = config["d_model"], config["nhead"], config["layer_names"]
        if (self.d_model, self.nhead) != (32, 8) or list(self.layer_names) != ["self", "cross"] * 4:
            raise NotImplementedError("d_model 32, 8 heads, ['self', 'cross'] * 4")
        self.layers = nn.ModuleList([EncoderLayer(self.d_model, self.nhead) for _ in self.layer_names])
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, ref_feature=None, src_feature=None, feat="ref"):
        """feat 'ref': ref_feature (1,32,H,W) -> the four self layers' outputs as (H*W,32) TOKENS (the cross layers of the
        source views read them in that form).  feat 'src': ref_feature = that list, src_feature (1,32,H,W) -> (1,32,H,W)."""
        if feat == "ref":
            x = costvol.fmt_tokens_in(ref_feature[0])
            outs = []
            for layer, name in zip(self.layers, self.layer_names):
                if name == "self":
                    x = layer(x, x)
                    outs.append(x)
            return outs
        if feat == "src":
            hw = tuple(src_feature.shape[-2:])
            x = costvol.fmt_tokens_in(src_feature[0])
            for i, (layer, name) in enumerate(zip(self.layers, self.layer_names)):
                x = layer(x, x if name == "self" else ref_feature[i // 2])
            return costvol.fmt_tokens_out(x, hw)[None]
        raise ValueError("Wrong feature name")


class FMT_with_pathway(nn.Module):
    def __init__(self, base_channels=8, FMT_config={"d_model": 32, "nhead": 8, "layer_names": ["self", "cross"] * 4}):
        super().__init__()
        b = base_channels
        self.FMT = FMT(FMT_config)
        self.dim_reduction_1 = nn.Conv2d(b * 4, b * 2, 1, bias=False)
        self.dim_reduction_2 = nn.Conv2d(b * 2, b * 1, 1, bias=False)
        self.smooth_1 = nn.Conv2d(b * 2, b * 2, 3, padding=1, bias=False)
        self.smooth_2 = nn.Conv2d(b * 1, b * 1, 3, padding=1, bias=False)

    def _pathway(self, s1, f):
        s2 = costvol.conv2d(costvol.pathway_step(s1[0], self.dim_reduction_1.weight, f["stage2"][0]), self.smooth_1.weight.detach())
        s3 = costvol.conv2d(costvol.pathway_step(s2, self.dim_reduction_2.weight, f["stage3"][0]), self.smooth_2.weight.detach())
        return {"stage1": s1, "stage2": s2[None], "stage3": s3[None]}

    @torch.no_grad()
    def forward(self, features):
        """features: per view {'stage1','stage2','stage3'} of (1,C,H,W), the reference view first -> NEW dicts; the input is
        left as it is (the reference overwrites it in place, models/FMT.py:213-223; StageLoop caches it per image)."""
        if self.training:
            raise NotImplementedError("TransMVSNet is inference-only in S-VolSDF (runner.py:153); call .eval()")
        out, ref_tokens = [], None
        for v, f in enumerate(features):
            if f["stage1"].shape[0] != 1:
                raise NotImplementedError("batch size 1 (runner.py:122)")
            if v == 0:
                ref_tokens = self.FMT(f["stage1"], feat="ref")
                s1 = costvol.fmt_tokens_out(ref_tokens[-1], tuple(f["stage1"].shape[-2:]))[None]
            else:
                s1 = self.FMT(ref_tokens, f["stage1"], feat="src")
            out.append(self._pathway(s1, f))
        return out


# ---------------------------------------------------------------------------------------------------------------------
# cost volume
# ---------------------------------------------------------------------------------------------------------------------
class ConvBnReLU3D(nn.Module):
    """parameter container of models/module.py:215-222 (1x1x1 here)"""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Conv3d(in_channels, out_channels, 1, stride=1, padding=0, bias=False)
        self.bn = nn.BatchNorm3d(out_channels)


class PixelwiseNet(nn.Module):
    """models/TransMVSNet.py:12-32: a scalar function of one scalar, 1 -> 16 -> 8 -> 1, evaluated inside svs_warp_similarity."""

    def __init__(self):
        super().__init__()
        self.conv0 = ConvBnReLU3D(1, 16)
        self.conv1 = ConvBnReLU3D(16, 8)
        self.conv2 = nn.Conv3d(8, 1, 1, stride=1, padding=0)
        self._fold = CachedFold()

    def folded(self):
        """the 177 floats svs_warp_similarity reads: scale0[16] shift0[16] W1[8][16] shift1[8] w2[8] b2, BatchNorm folded"""
        def make():
            s0, t0 = fold_bn(self.conv0.bn)
            s1, t1 = fold_bn(self.conv1.bn)
            w0 = self.conv0.conv.weight.detach().float().reshape(16) * s0
            w1 = self.conv1.conv.weight.detach().float().reshape(8, 16) * s1[:, None]
            return torch.cat([w0, t0, w1.reshape(-1), t1, self.conv2.weight.detach().float().reshape(8),
                              self.conv2.bias.detach().float().reshape(1)]).contiguous()
        ts = [self.conv0.conv.weight, self.conv1.conv.weight, self.conv2.weight, self.conv2.bias]
        return self._fold(ts + bn_tensors(self.conv0.bn) + bn_tensors(self.conv1.bn), make)


class DepthNet(nn.Module):
    """models/TransMVSNet.py:35-115."""

    def __init__(self):
        super().__init__()
        self.pixel_wise_net = PixelwiseNet()

    def forward(self, features, proj_matrices, depth_values, num_depth, cost_regularization, prob_volume_init=None,
                view_weights=None):
        """view_weights: None at stage 1 (they are produced), else the previous stage's (1,V-1,H/2,W/2).  Returns the stage's
        outputs and the weights at this stage's size (the reference up-samples them before the call, :208)."""
        assert len(features) == proj_matrices.shape[1], "Different number of images and projection matrices"
        assert depth_values.shape[1] == num_depth
        if prob_volume_init is not None:
            raise NotImplementedError("prob_volume_init is always None on this path")
        net = self.pixel_wise_net.folded() if view_weights is None else None
        similarity, weights = costvol.warp_similarity(features, proj_matrices, depth_values, view_weights, net)
        reg = cost_regularization(similarity)[0, 0]
        prob, depth, conf, _ = costvol.prob_wta(reg, depth_values[0])
        return {"depth": depth[None], "photometric_confidence": conf[None], "prob_volume": prob[None],
                "depth_values": depth_values}, weights


class TransMVSNet(nn.Module):
    def __init__(self, refine=False, ndepths=[48, 32, 8], depth_interals_ratio=[4, 2, 1], share_cr=False,
                 grad_method="detach", arch_mode="fpn", cr_base_chs=[8, 8, 8]):
        super().__init__()
        if refine:
            raise NotImplementedError("refine=False everywhere in S-VolSDF (runner.py:131)")
        if share_cr:
            raise NotImplementedError("share_cr=False (one regularisation network per stage)")
        self.refine, self.share_cr, self.ndepths = refine, share_cr, ndepths
        self.depth_interals_ratio, self.grad_method, self.arch_mode = depth_interals_ratio, grad_method, arch_mode
        self.cr_base_chs, self.num_stage = cr_base_chs, len(ndepths)
        assert len(ndepths) == len(depth_interals_ratio)
        if self.num_stage != 3:
            raise NotImplementedError("three stages (config/base.yaml)")
        self.stage_infos = {"stage1": {"scale": 4.0}, "stage2": {"scale": 2.0}, "stage3": {"scale": 1.0}}
        self.feature = FeatureNet(base_channels=8)
        self.FMT_with_pathway = FMT_with_pathway()
        self.cost_regularization = nn.ModuleList([CostRegNet(in_channels=1, base_channels=cr_base_chs[i])
                                                  for i in range(self.num_stage)])
        self.DepthNet = DepthNet()

    @torch.no_grad()
    def forward(self, stage_idx, sample_cuda, features, extra, outputs, int_r, depth=None, inverse_depth=False,
                prevent_oom=False):
        if self.training:
            raise NotImplementedError("TransMVSNet is inference-only in S-VolSDF (runner.py:153); call .eval()")
        view_weights = extra
        imgs, proj_matrices = sample_cuda["imgs"], sample_cuda["proj_matrices"]
        if imgs.shape[0] != 1:
            raise NotImplementedError("batch size 1 (runner.py:122)")
        key, features_stage, depth, outputs = stage_inputs(stage_idx, features, outputs, depth)
        scale, nd = int(self.stage_infos[key]["scale"]), self.ndepths[stage_idx]
        hyp = range_hypotheses(sample_cuda, depth, nd, scale, int_r, inverse_depth, features_stage[0].device)
        if (view_weights is None) != (stage_idx == 0):
            raise ValueError("view weights are produced at stage 1 and passed on to stages 2 and 3")
        outputs_stage, view_weights = self.DepthNet(features_stage, proj_matrices[key], depth_values=hyp[None], num_depth=nd,
                                                    cost_regularization=self.cost_regularization[stage_idx],
                                                    view_weights=view_weights)
        outputs[key] = outputs_stage
        outputs.update(outputs_stage)
        return outputs, view_weights


TransMVSNetHip = TransMVSNet
