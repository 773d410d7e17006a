"""LPIPS, the reference's third novel-view score, on the HIP path (eval_vsdf.py:178, 208-209 -> lpips_tf.py:29-90;
csrc/svs_lpips.hip).

    python -m svs_hip.lpips --lpips-vgg vgg16.pth --lpips-lin vgg_lin.pth --data-dir-root data_s_volsdf --dataset DTU \\
        --scan 106 --rendering-dir exps_result/ours_106/rendering_1562 --views 1 2 9 [--result-from blend] [--json out.json]

prints the reference's four-line SCAN block (svs_hip.nvs prints the first three).  The weights are the user's: the two
public files of the LPIPS v0.1 model, torchvision's `vgg16` state dict and the `lpips` package's `vgg.pth` (the lin layers).
Neither torchvision nor `lpips` is needed to read them, and no weights ship with this project.

RESTATED from the reference: the inputs (the white-composited float32 images SSIM sees, eval_vsdf.py:199-204, each
`x * 2 - 1`, lpips_tf.py:55-56) and the printed line (eval_vsdf.py:277).
OURS / UNPINNED: the network.  lpips_tf.py downloads a frozen graph (net-lin_vgg_v0.1.pb) that is not part of the
reference, so the definition is restated from the published model (net-lin, vgg, version 0.1):
  scaling   (x - shift[c]) / scale[c], shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450)
  features  VGG-16: 3x3 convolutions (stride 1, zero padding 1, bias, ReLU) at torchvision's indices 0,2 | 5,7 | 10,12,14 |
            17,19,21 | 24,26,28 with a 2x2 max-pool (stride 2, floor) before every group but the first;
            taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
  distance  per tap and pixel n(f) = f / (sqrt(sum_c f_c^2) + 1e-10), d = sum_c w[c] (n(f0)_c - n(f1)_c)^2; the taps'
            spatial means added
Parity is with a float64 restatement of this definition on seeded weights (tests/lpips_oracle.py).  Agreement with the
frozen graph on the real weights is not claimed: neither exists where this was written.
"""
import numpy as np
import torch

from . import lib as _lib
from .images import device, to_device
from .ops import _f32, _ptr, _stream

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)              # torchvision vgg16.features
CONV_SHAPE = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512),
              (512, 512), (512, 512), (512, 512), (512, 512))              # (Cin, Cout)
CONV_GROUP = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)                       # a pool precedes every group but the first
TAP_CHANNELS = (64, 128, 256, 512, 512)
_SLICE_END = (4, 9, 16, 23, 30)                                            # the lpips package's slice1..5 of `features`
MIN_SIZE = 16                                                              # relu5_3 needs one pixel


def _read_state(path):
    path = str(path)
    if path.endswith(".npz"):
        with np.load(path) as z:
            return {k: np.asarray(z[k]) for k in z.files}
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(sd).__name__}")
    return {k: v.detach().cpu().numpy() for k, v in sd.items() if torch.is_tensor(v)}


def _pick(sd, names, what, shape, files):
    for n in names:
        if n in sd:
            a = np.asarray(sd[n], np.float32).reshape(-1) if shape is None else np.asarray(sd[n], np.float32)
            if shape is not None and tuple(a.shape) != tuple(shape):
                raise ValueError(f"{what}: {n} has shape {tuple(a.shape)}, expected {tuple(shape)}")
            return np.ascontiguousarray(a)
    raise KeyError(f"{what} is missing from {files}: none of {', '.join(names)}")


def load_weights(vgg_path, lin_path=None):
    """Reads plain state dicts (.pth through torch.load(weights_only=True), or .npz).  Convolutions: torchvision's
    `features.{i}.weight|bias` or the lpips package's `net.slice{s}.{i}.weight|bias`; lin layers: `lin{k}.model.1.weight`
    or `lins.{k}.model.1.weight`, (1,C,1,1).  lin_path=None: everything is in vgg_path.  A missing layer is a KeyError
    that names it, a wrong shape a ValueError.  -> dict(conv=[(weight (Cout,Cin,3,3), bias (Cout,)) x 13], lin=[(C,) x 5])"""
    sd = _read_state(vgg_path)
    files = str(vgg_path)
    if lin_path is not None:
        sd.update(_read_state(lin_path))
        files += " / " + str(lin_path)
    conv = []
    for i, (cin, cout) in zip(CONV_INDEX, CONV_SHAPE):
        s = next(k + 1 for k, end in enumerate(_SLICE_END) if i < end)
        what = f"VGG-16 convolution features.{i} ({cin} -> {cout})"
        w = _pick(sd, (f"features.{i}.weight", f"net.slice{s}.{i}.weight"), what + " weight", (cout, cin, 3, 3), files)
        b = _pick(sd, (f"features.{i}.bias", f"net.slice{s}.{i}.bias"), what + " bias", (cout,), files)
        conv.append((w, b))
    lin = []
    for k, c in enumerate(TAP_CHANNELS):
        w = _pick(sd, (f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight"), f"lin layer {k} ({c} channels)", (1, c, 1, 1), files)
        lin.append(np.ascontiguousarray(w.reshape(c)))
    return dict(conv=conv, lin=lin)


# ---- the single operators (float32 (C,H,W) in and out): what the tests check a layer at a time
def pack_conv3x3(weight):
    """weight (Cout,Cin,3,3) -> the packed device buffer of svs_conv3x3_mfma"""
    L = _lib.load()
    w = _f32(to_device(weight, torch.float32, "lpips", "weight", ndim=(4,)))
    cout, cin = int(w.shape[0]), int(w.shape[1])
    if tuple(w.shape[2:]) != (3, 3) or not L.svs_conv3x3_mfma_supported(cin, cout):
        raise ValueError(f"unsupported convolution weight {tuple(w.shape)}: 3x3 with Cin in 3, 64..512 and Cout in 64..512")
    frag = torch.empty(int(L.svs_conv3x3_mfma_wfrag_bytes(cin, cout)), dtype=torch.uint8, device=w.device)
    _lib.check(L.svs_conv3x3_mfma_pack(_ptr(w), cin, cout, _ptr(frag), _stream()), "svs_conv3x3_mfma_pack")
    return frag


def conv3x3(x, weight, bias=None, relu=True, wfrag=None):
    """relu?(conv2d(x (Cin,H,W), weight (Cout,Cin,3,3), padding 1) + bias) -> (Cout,H,W) float32 device tensor"""
    L = _lib.load()
    x = _f32(to_device(x, torch.float32, "lpips", "x", ndim=(3,)))
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    if int(x.shape[0]) != cin:
        raise ValueError(f"x has {int(x.shape[0])} channels, the weight takes {cin}")
    if wfrag is None:
        wfrag = pack_conv3x3(weight)
    b = None if bias is None else _f32(to_device(bias, torch.float32, "lpips", "bias", ndim=(1,)))
    H, W = int(x.shape[1]), int(x.shape[2])
    out = torch.empty(cout, H, W, dtype=torch.float32, device=x.device)
    _lib.check(L.svs_conv3x3_mfma(_ptr(x), _ptr(wfrag), _ptr(b), _ptr(out), cin, cout, H, W, int(bool(relu)), _stream()),
               "svs_conv3x3_mfma")
    return out


def maxpool2(x):
    """2x2 max-pool, stride 2, floor mode: (C,H,W) -> (C,H//2,W//2)"""
    L = _lib.load()
    x = _f32(to_device(x, torch.float32, "lpips", "x", ndim=(3,)))
    C, H, W = (int(n) for n in x.shape)
    out = torch.empty(C, H // 2, W // 2, dtype=torch.float32, device=x.device)
    _lib.check(L.svs_maxpool2(_ptr(x), _ptr(out), C, H, W, _stream()), "svs_maxpool2")
    return out


def head(f0, f1, w):
    """one tap's distance: the spatial mean of sum_c w[c] (n(f0)_c - n(f1)_c)^2 -> float"""
    L = _lib.load()
    f0 = _f32(to_device(f0, torch.float32, "lpips", "f0", ndim=(3,)))
    f1 = _f32(to_device(f1, torch.float32, "lpips", "f1", ndim=(3,)))
    w = _f32(to_device(w, torch.float32, "lpips", "w", ndim=(1,)))
    if f0.shape != f1.shape or int(w.shape[0]) != int(f0.shape[0]):
        raise ValueError(f"f0 {tuple(f0.shape)}, f1 {tuple(f1.shape)} and w {tuple(w.shape)} do not belong together")
    C, H, W = (int(n) for n in f0.shape)
    out = torch.empty(1, dtype=torch.float64, device=f0.device)
    _lib.check(L.svs_lpips_head(_ptr(f0), _ptr(f1), _ptr(w), C, H, W, _ptr(out), _stream()), "svs_lpips_head")
    return float(out.cpu()[0])


class LpipsNet:
    """The packed network on the device.  weights: load_weights()'s dict (or anything of that layout)."""

    def __init__(self, weights):
        conv, lin = weights["conv"], weights["lin"]
        if len(conv) != len(CONV_SHAPE) or len(lin) != len(TAP_CHANNELS):
            raise ValueError(f"expected {len(CONV_SHAPE)} convolutions and {len(TAP_CHANNELS)} lin layers, "
                             f"got {len(conv)} and {len(lin)}")
        L = _lib.load()
        dev = device("lpips")
        self.net = torch.zeros(int(L.svs_lpips_net_bytes()), dtype=torch.uint8, device=dev)

        def f32_at(offset, n):
            return self.net[offset:offset + 4 * n].view(torch.float32)

        for i, ((w, b), (cin, cout)) in enumerate(zip(conv, CONV_SHAPE)):
            w = _f32(to_device(w, torch.float32, "lpips", f"convolution {i} weight"))
            b = _f32(to_device(b, torch.float32, "lpips", f"convolution {i} bias"))
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise ValueError(f"convolution {i}: weight {tuple(w.shape)} / bias {tuple(b.shape)}, expected "
                                 f"{(cout, cin, 3, 3)} / {(cout,)}")
            frag = self.net[int(L.svs_lpips_net_offset(0, i)):]
            _lib.check(L.svs_conv3x3_mfma_pack(_ptr(w), cin, cout, frag.data_ptr(), _stream()), f"svs_conv3x3_mfma_pack({i})")
            f32_at(int(L.svs_lpips_net_offset(1, i)), cout).copy_(b)
        for k, c in enumerate(TAP_CHANNELS):
            w = _f32(to_device(lin[k], torch.float32, "lpips", f"lin layer {k}")).reshape(-1)
            if int(w.shape[0]) != c:
                raise ValueError(f"lin layer {k}: {int(w.shape[0])} weights, expected {c}")
            f32_at(int(L.svs_lpips_net_offset(2, k)), c).copy_(w)
        self._ws = None

    def score_views(self, pred, gt, mask):
        """pred, gt, mask as for svs_hip.nvs.score_views ((V,H,W,3) uint8, mask nonzero inside; arrays or tensors, host or
        device), at least 16x16.  -> lpips[V] float64 numpy: the distance of the white-composited images."""
        shape = tuple(pred.shape)
        if len(shape) != 4 or shape[3] != 3:
            raise ValueError(f"expected (V,H,W,3) images, got {shape}")
        if tuple(gt.shape) != shape or tuple(mask.shape) != shape:
            raise ValueError(f"pred {shape}, gt {tuple(gt.shape)} and mask {tuple(mask.shape)} differ")
        V, H, W, _ = shape
        if V < 1 or H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"need at least one view of at least {MIN_SIZE}x{MIN_SIZE} pixels (relu5_3 needs one), got {shape}")
        L = _lib.load()
        p, g, m = (to_device(a, torch.uint8, "lpips", what, cast=False) for a, what in ((pred, "pred"), (gt, "gt"), (mask, "mask")))
        need = int(L.svs_lpips_workspace_bytes(V, H, W))
        if need == 0:
            raise ValueError(f"images of {H}x{W} are too large")
        if self._ws is None or self._ws.numel() < need or self._ws.device != p.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=p.device)
        out = torch.empty(V, dtype=torch.float64, device=p.device)
        _lib.check(L.svs_lpips_score(_ptr(p), _ptr(g), _ptr(m), V, H, W, _ptr(self.net), _ptr(self._ws), _ptr(out), _stream()),
                   "svs_lpips_score")
        return out.cpu().numpy()


def main(argv=None):
    from . import nvs
    return nvs.main(argv, require_lpips=True)


if __name__ == "__main__":
    main()
