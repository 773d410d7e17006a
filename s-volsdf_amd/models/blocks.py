"""What the three MVS backbones (models/CasMVSNet.py, models/ucsnet.py, models/transmvs.py) share: eval-mode BatchNorm folding
with its cache, the Conv-BN-ReLU block and the eight-layer encoder of the feature extractors, and the per-stage bookkeeping of
the cascade's forward()."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from svs_hip import costvol
from svs_hip.tensor_cache import Derived as CachedFold   # folded weights, remade when a tensor they were folded from changes


def fold_bn(bn):
    """eval-mode BatchNorm as (scale, shift), float32: y = x * scale + shift"""
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().float()
    return scale.contiguous(), (bn.bias - bn.running_mean * scale).detach().float().contiguous()


def bn_tensors(bn):
    """the tensors fold_bn reads"""
    return [bn.weight, bn.bias, bn.running_mean, bn.running_var]


def _conv_batch(x, w, b, add=None, add_upsample2=False, stride=1, relu=False):
    """(B,Cin,H,W) -> (B,Cout,Ho,Wo): one launch per image, written straight into the batch tensor."""
    k = w.shape[-1]
    Ho, Wo = (x.shape[2] + 2 * (k // 2) - k) // stride + 1, (x.shape[3] + 2 * (k // 2) - k) // stride + 1
    out = torch.empty(x.shape[0], w.shape[0], Ho, Wo, device=x.device)
    for i in range(x.shape[0]):
        costvol.conv2d(x[i], w, b, add=None if add is None else add[i], add_upsample2=add_upsample2, stride=stride, relu=relu,
                       out=out[i])
    return out


class Conv2d(nn.Module):
    """conv + BatchNorm2d + ReLU with the reference's parameter names (`conv.weight`, `bn.*`).  On the device, in eval
    mode, the block is ONE launch of svs_conv2d with the BatchNorm folded into the weights."""

    def __init__(self, cin, cout, k, stride=1, relu=True, bn=True, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, bias=not bn, **kw)
        self.bn = nn.BatchNorm2d(cout) if bn else None
        self.relu, self.stride = relu, stride
        self._fold = CachedFold()

    def folded(self):
        """(weight (Cout,Cin,k,k), bias or None), float32, the BatchNorm (eval) folded in"""
        def make():
            w = self.conv.weight.detach().float()
            b = self.conv.bias.detach().float() if self.conv.bias is not None else None
            if self.bn is not None:
                scale, shift = fold_bn(self.bn)
                w = w * scale.view(-1, 1, 1, 1)
                b = shift if b is None else b * scale + shift
            return w.contiguous(), b.contiguous() if b is not None else None
        ts = [self.conv.weight] + ([self.conv.bias] if self.conv.bias is not None else [])
        return self._fold(ts + (bn_tensors(self.bn) if self.bn is not None else []), make)

    def forward(self, x):
        if x.is_cuda and not self.training:
            w, b = self.folded()
            return _conv_batch(x, w, b, stride=self.stride, relu=self.relu)
        x = self.conv(x)
        if self.bn is not None:
            x = self.bn(x)
        return F.relu(x) if self.relu else x


def encoder_trunk(b):
    """conv0, conv1, conv2 of the three feature extractors (models/CasMVSNet.py:343-361, models/ucsnet.py:244-259,
    models/module.py:349-362): 3 -> b at full resolution, -> 2b at half, -> 4b at quarter resolution, eight Conv-BN-ReLU blocks"""
    return (nn.Sequential(Conv2d(3, b, 3, 1, padding=1), Conv2d(b, b, 3, 1, padding=1)),
            nn.Sequential(Conv2d(b, 2 * b, 5, stride=2, padding=2), Conv2d(2 * b, 2 * b, 3, 1, padding=1),
                          Conv2d(2 * b, 2 * b, 3, 1, padding=1)),
            nn.Sequential(Conv2d(2 * b, 4 * b, 5, stride=2, padding=2), Conv2d(4 * b, 4 * b, 3, 1, padding=1),
                          Conv2d(4 * b, 4 * b, 3, 1, padding=1)))


def stack_stages(per_image):
    """[(stage1, stage2, stage3) per image] -> {'stage1': (B,...), 'stage2': ..., 'stage3': ...}"""
    return {f"stage{j + 1}": torch.stack([o[j] for o in per_image]) if len(per_image) > 1 else per_image[0][j][None]
            for j in range(3)}


def stage_inputs(stage_idx, features, outputs, depth):
    """The head of every backbone's forward(stage_idx, ...): the previous depth defaults to the previous stage's output.
    -> key 'stageN', that stage's feature list, depth, outputs"""
    if depth is None:
        depth = outputs['depth'] if stage_idx > 0 else None
    key = "stage{}".format(stage_idx + 1)
    return key, [feat[key] for feat in features], depth, {} if outputs is None else outputs


def range_hypotheses(sample_cuda, depth, nd, scale, int_r, inverse_depth, device):
    """CasMVSNet's depth hypotheses (models/CasMVSNet.py:733-751; TransMVSNet's :185-223 is the same text): stage 1 spans the
    scan's depth range, later stages a window of nd * int_r depth intervals round the previous depth (stages 2, 3 of the
    inverse variant use the same window, models/CasMVSNet.py:548-554) -> (nd, H/scale, W/scale)"""
    imgs, depth_values = sample_cuda["imgs"], sample_cuda["depth_values"]
    dv = costvol.host_copy(depth_values)[0]
    depth_min, depth_max = float(dv[0]), float(dv[-1])
    depth_interval = (depth_max - depth_min) / depth_values.size(1)
    hw = (imgs.shape[-2], imgs.shape[-1])
    if depth is not None:
        return costvol.depth_hypotheses(depth[0], hw, nd, scale, depth_min, depth_max, int_r * depth_interval, False, device)
    return costvol.depth_hypotheses(None, hw, nd, scale, depth_min, depth_max, 0.0, inverse_depth, device)
