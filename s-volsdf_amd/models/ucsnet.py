"""UCSNet with the reference's constructor, parameter names and forward() contract (models/ucsnet.py:398-477), on the HIP
kernels: the "unet" feature extractor from one library call (csrc/svs_ucsnet.hip: svs_featurenet_unet, transposed
convolutions on the matrix cores), the cost volume of CasMVSNet (fused homography warp + variance, the 3-D U-Net with folded
BatchNorm -- the same eleven layers under other attribute names), the tail with the per-pixel uncertainty
(svs_prob_depth_conf_var) and the uncertainty-aware hypotheses (svs_uncertainty_hypotheses).  A checkpoint of the reference
loads with strict=True (`feature_extraction.*`, `cost_regularization.{0,1,2}.*`).  Inference only, like the reference
(`@torch.no_grad()` forward).

Which class the name `UCSNet` gives: the drop-in boundary (tests/test_dropin_imports.py) lists UCSNet among
the names that resolve to the reference whenever a checkout of it is on the path, so there `models.ucsnet.UCSNet` stays the
reference's class and the mirror is `models.ucsnet.UCSNetHip`; without a checkout (a box that only runs the hot path, where
`mvs_model_name=ucsnet` had no class at all) `UCSNet` is the mirror.  `UCSNetHip` is the mirror in both cases.
"""
import torch
import torch.nn as nn

from svs_hip import costvol
from svs_hip.refpath import reference_module
from models.blocks import CachedFold, Conv2d, bn_tensors, encoder_trunk, fold_bn, stack_stages, stage_inputs
from models.CasMVSNet import Conv3d, CostRegNet as _CasCostRegNet

eps = 1e-12


class Deconv2dUnit(nn.Module):
    """ConvTranspose2d(k3, s2, p1, output_padding 1) + BatchNorm2d + ReLU with the reference's parameter names (`conv.weight`,
    `bn.*`; models/ucsnet.py:114-149)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.ConvTranspose2d(cin, cout, 3, stride=2, padding=1, output_padding=1, bias=False)
        self.bn = nn.BatchNorm2d(cout)
        self._fold = CachedFold()

    def folded(self):
        """(weight (Cin,Cout,3,3), bias) with the BatchNorm (eval) folded in"""
        def make():
            scale, shift = fold_bn(self.bn)
            return (self.conv.weight.detach().float() * scale.view(1, -1, 1, 1)).contiguous(), shift
        return self._fold([self.conv.weight] + bn_tensors(self.bn), make)


class Deconv2dBlock(nn.Module):
    """models/ucsnet.py:220-235: `deconv` (transposed, x2), cat with the encoder level, `conv` (3x3)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.deconv = Deconv2dUnit(cin, cout)
        self.conv = Conv2d(2 * cout, cout, 3, 1, padding=1)


class FeatExtNet(nn.Module):
    """models/ucsnet.py:237-302, num_stage 3."""

    def __init__(self, base_channels, num_stage=3):
        super().__init__()
        if num_stage != 3:
            raise NotImplementedError("only the 3-stage feature extractor is declared")
        b = base_channels
        self.base_channels, self.num_stage = b, num_stage
        self.conv0, self.conv1, self.conv2 = encoder_trunk(b)
        self.out1 = nn.Conv2d(4 * b, 4 * b, 1, bias=False)
        self.deconv1 = Deconv2dBlock(4 * b, 2 * b)
        self.deconv2 = Deconv2dBlock(2 * b, b)
        self.out2 = nn.Conv2d(2 * b, 2 * b, 1, bias=False)
        self.out3 = nn.Conv2d(b, b, 1, bias=False)
        self.out_channels = [4 * b, 2 * b, b]
        self._unet = None

    def layers(self):
        """(weight, bias) of the 15 layers in svs_featurenet_unet's order, BatchNorm folded."""
        plain = lambda c: (c.weight.detach(), None)
        enc = [blk.folded() for blk in list(self.conv0) + list(self.conv1) + list(self.conv2)]
        return enc + [plain(self.out1), self.deconv1.deconv.folded(), self.deconv1.conv.folded(), plain(self.out2),
                      self.deconv2.deconv.folded(), self.deconv2.conv.folded(), plain(self.out3)]

    def forward(self, x):
        if self.training:
            raise NotImplementedError("UCSNet is inference-only in S-VolSDF (runner.py:153); call .eval()")
        if not x.is_cuda:
            raise NotImplementedError("the feature extractor runs on the HIP kernels: device tensors only")
        if self._unet is None:
            self._unet = costvol.FeatureNetUnet(self.base_channels)
        layers = self.layers()
        return stack_stages([self._unet(xi, layers) for xi in x])


class CostRegNet(_CasCostRegNet):
    """models/ucsnet.py:304-335: CasMVSNet's regularisation network with the transposed layers named deconv7 / 8 / 9."""
    DECONV_NAMES = ("deconv7", "deconv8", "deconv9")


def compute_depth(feats, proj_mats, depth_samps, cost_reg, lamb, is_training=False):
    """models/ucsnet.py:338-396.  feats: list of (1,C,H,W) (reference first), proj_mats (1,V,2,4,4), depth_samps (1,D,H,W)."""
    if is_training:
        raise NotImplementedError("UCSNet is inference-only in S-VolSDF (runner.py:153); call .eval()")
    assert len(feats) == proj_mats.shape[1], "Different number of images and projection matrices"
    conv0 = getattr(cost_reg, "conv0", None)
    split = (isinstance(conv0, Conv3d) and not conv0.training and feats[0].is_cuda
             and costvol.pair_supported(feats[0].shape[1], conv0.conv.out_channels))
    variance = costvol.warp_variance(feats, proj_mats, depth_samps, split=split)
    reg = cost_reg(variance)[0, 0]
    prob, depth, conf, _, var = costvol.prob_depth_conf_var(reg, depth_samps[0], lamb)
    return {"depth": depth[None], "photometric_confidence": conf[None], "prob_volume": prob[None], "variance": var[None],
            "depth_values": depth_samps}


class UCSNet(nn.Module):
    def __init__(self, lamb=1.5, stage_configs=[64, 32, 8], grad_method="detach", base_chs=[8, 8, 8], feat_ext_ch=8):
        super().__init__()
        self.stage_configs, self.grad_method, self.base_chs, self.lamb = stage_configs, grad_method, base_chs, lamb
        self.num_stage = len(stage_configs)
        if self.num_stage != 3:
            raise NotImplementedError("three stages (config/base.yaml)")
        self.ds_ratio = {"stage1": 4.0, "stage2": 2.0, "stage3": 1.0}
        self.feature_extraction = FeatExtNet(base_channels=feat_ext_ch, num_stage=self.num_stage)
        self.cost_regularization = nn.ModuleList(
            [CostRegNet(in_channels=self.feature_extraction.out_channels[i], base_channels=self.base_chs[i])
             for i in range(self.num_stage)])

    @torch.no_grad()
    def forward(self, stage_idx, sample_cuda, features, extra, outputs, int_r, depth=None, prevent_oom=False,
                inverse_depth=False):
        if self.training:
            raise NotImplementedError("UCSNet is inference-only in S-VolSDF (runner.py:153); call .eval()")
        exp_var = extra
        imgs, proj_matrices, depth_values = sample_cuda["imgs"], sample_cuda["proj_matrices"], sample_cuda["depth_values"]
        key, features_stage, depth, outputs = stage_inputs(stage_idx, features, outputs, depth)
        scale, nd = int(self.ds_ratio[key]), self.stage_configs[stage_idx]
        cur_h, cur_w = imgs.shape[-2] // scale, imgs.shape[-1] // scale
        dev = features_stage[0].device
        if depth is not None:
            # the previous depth (possibly the rendered one, runner.py:240-243) and uncertainty, resized inside the kernel
            hyp = costvol.uncertainty_hypotheses(depth[0], exp_var[0], (cur_h, cur_w), nd)
        else:
            dv = costvol.host_copy(depth_values)[0]
            hyp = costvol.uncertainty_hypotheses(None, None, (cur_h, cur_w), nd, float(dv[0]), float(dv[-1]), inverse_depth, dev)
        outputs_stage = compute_depth(features_stage, proj_matrices[key], depth_samps=hyp[None],
                                      cost_reg=self.cost_regularization[stage_idx], lamb=self.lamb, is_training=self.training)
        exp_var = outputs_stage["variance"]
        outputs[key] = outputs_stage
        outputs.update(outputs_stage)
        return outputs, exp_var


UCSNetHip = UCSNet
_reference = reference_module("models.ucsnet")
if _reference is not None:
    UCSNet = _reference.UCSNet
