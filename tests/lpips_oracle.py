"""LPIPS v0.1 (net-lin, vgg) restated in plain torch on the CPU: the float64 oracle of svs_hip.lpips and the same definition
in float32 (the comparator whose own error sets the tolerances of tests/test_gpu_lpips.py).  The definition is the one in
svs_hip/lpips.py's docstring; the weights are seeded, never the real ones.

    inputs    x = code / 255 (float32), x * mask + (1 - mask) (float32: what SSIM sees), then in `dtype`: x * 2 - 1,
              (x - shift[c]) / scale[c]
    features  13 3x3 convolutions (padding 1, bias, ReLU), 2x2 max-pool (floor) before every group but the first
    distance  per tap: mean over the pixels of sum_c w[c] (n(f0)_c - n(f1)_c)^2, n(f) = f / (sqrt(sum_c f_c^2) + 1e-10)
"""
import numpy as np
import torch
import torch.nn.functional as F

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_SHAPE = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512),
              (512, 512), (512, 512), (512, 512), (512, 512))
CONV_GROUP = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)


def make_weights(seed=0, conv_factor=1.0):
    """Seeded weights: convolutions N(0, 2 / (9 Cin)) times conv_factor with biases N(0, 0.05^2), lin weights >= 0 that
    sum to 1 per tap.  -> dict(conv=[(weight, bias)], lin=[w]) of float32 arrays (svs_hip.lpips.load_weights's layout)"""
    rng = np.random.default_rng(seed)
    conv = []
    for cin, cout in CONV_SHAPE:
        w = rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin)) * conv_factor
        b = rng.standard_normal(cout) * 0.05
        conv.append((w.astype(np.float32), b.astype(np.float32)))
    lin = []
    for c in TAP_CHANNELS:
        w = rng.random(c)
        lin.append((w / w.sum()).astype(np.float32))
    return dict(conv=conv, lin=lin)


def state_dict(weights, style="torchvision"):
    """the weights under the key names of `style`: 'torchvision' (features.{i}, lin{k}.model.1), 'lpips' (net.slice{s}.{i},
    lin{k}.model.1) or 'lins' (features.{i}, lins.{k}.model.1) -> {name: float32 array}"""
    ends = (4, 9, 16, 23, 30)
    sd = {}
    for i, (w, b) in zip(CONV_INDEX, weights["conv"]):
        s = next(k + 1 for k, e in enumerate(ends) if i < e)
        stem = f"net.slice{s}.{i}" if style == "lpips" else f"features.{i}"
        sd[stem + ".weight"], sd[stem + ".bias"] = w, b
    for k, w in enumerate(weights["lin"]):
        sd[(f"lins.{k}" if style == "lins" else f"lin{k}") + ".model.1.weight"] = w.reshape(1, -1, 1, 1)
    return sd


def composite(codes, mask):
    """(...,H,W,3) uint8 codes and mask (nonzero: inside) -> the float32 image eval_vsdf.py:199-204 hands to SSIM and LPIPS"""
    x = np.asarray(codes, np.float32) / np.float32(255.0)
    m = (np.asarray(mask) != 0).astype(np.float32)
    return x * m + (np.float32(1.0) - m)


def network_input(img, dtype):
    """float32 (N,H,W,3) in [0,1] -> (N,3,H,W) in dtype: x * 2 - 1, then the scaling layer"""
    x = torch.from_numpy(np.ascontiguousarray(img)).to(dtype).permute(0, 3, 1, 2)
    x = x * 2 - 1
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    return (x - shift) / scale


def features(x, weights, dtype):
    """(N,3,H,W) -> the five taps [(N,C,h,w)]"""
    taps = []
    for i, (w, b) in enumerate(weights["conv"]):
        if i > 0 and CONV_GROUP[i] != CONV_GROUP[i - 1]:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype), padding=1))
        if i + 1 == len(CONV_GROUP) or CONV_GROUP[i + 1] != CONV_GROUP[i]:
            taps.append(x)
    return taps


def head(f0, f1, w):
    """(C,h,w) features and (C,) lin weights, tensors of one dtype -> the tap's distance (0-d tensor)"""
    n0 = f0 / (torch.sqrt((f0 * f0).sum(0, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 * f1).sum(0, keepdim=True)) + 1e-10)
    d = (w.view(-1, 1, 1) * (n0 - n1) ** 2).sum(0)
    return d.mean()


def lpips(pred, gt, mask, weights, dtype=torch.float64):
    """(V,H,W,3) uint8 codes and masks -> the distance per view, float64 numpy [V], evaluated in `dtype`"""
    pred, gt, mask = np.asarray(pred), np.asarray(gt), np.asarray(mask)
    out = np.zeros(pred.shape[0], np.float64)
    with torch.no_grad():
        for v in range(pred.shape[0]):
            x = network_input(np.stack([composite(pred[v], mask[v]), composite(gt[v], mask[v])]), dtype)
            total = torch.zeros((), dtype=dtype)
            for f, w in zip(features(x, weights, dtype), weights["lin"]):
                total = total + head(f[0], f[1], torch.from_numpy(w).to(dtype))
            out[v] = float(total)
    return out


class Float32Comparator:
    """The same definition evaluated in float32: what a plain float32 implementation of LPIPS returns."""

    def __init__(self, weights):
        self.weights = weights

    def conv(self, x, w, b, relu):
        with torch.no_grad():
            y = F.conv2d(torch.from_numpy(x).float()[None], torch.from_numpy(w).float(),
                         None if b is None else torch.from_numpy(b).float(), padding=1)[0]
            return (F.relu(y) if relu else y).numpy()

    def __call__(self, pred, gt, mask):
        return lpips(pred, gt, mask, self.weights, torch.float32)


def conv64(x, w, b, relu):
    """float64 conv of float32 arrays x (Cin,H,W), w (Cout,Cin,3,3), b (Cout,) or None -> (y, sum |w||x| per output)"""
    with torch.no_grad():
        x64, w64 = torch.from_numpy(x).double()[None], torch.from_numpy(w).double()
        y = F.conv2d(x64, w64, None if b is None else torch.from_numpy(b).double(), padding=1)[0]
        mag = F.conv2d(x64.abs(), w64.abs(), padding=1)[0]
        return (F.relu(y) if relu else y).numpy(), mag.numpy()


def make_views(seed, V, H, W):
    """Seeded evaluation views: a smooth ground truth, a prediction that mixes it with its mirror image and noise, masks that differ per channel.
    -> pred, gt, mask (V,H,W,3) uint8"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    gt = np.empty((V, H, W, 3), np.float64)
    for v in range(V):
        for c in range(3):
            a, b, p = rng.random(3)
            gt[v, :, :, c] = 127.5 + 100.0 * np.sin(6.0 * a * yy / H + 5.0 * b * xx / W + 6.28 * p)
    gt = np.clip(np.rint(gt + rng.normal(0.0, 6.0, gt.shape)), 0, 255)
    pred = np.clip(np.rint(0.6 * gt + 0.4 * gt[:, ::-1, ::-1] + rng.normal(0.0, 30.0, gt.shape)), 0, 255)
    mask = (rng.random((V, H, W, 3)) < 0.8).astype(np.uint8)
    mask[:, : H // 4, : W // 3, :] = 0                              # an outside region, as a real mask has
    mask[:, H // 4, :, 1] = 0                                       # and channels that disagree
    return pred.astype(np.uint8), gt.astype(np.uint8), mask
