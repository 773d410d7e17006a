"""torch-tensor wrappers for the CasMVSNet cost-volume kernels (csrc/svs_costvol.hip)."""
import ctypes
import os
import weakref

import numpy as np
import torch

from . import lib as _lib
from .ops import _f32, _ptr, _ptr_array, _stream
from .tensor_cache import Derived, TensorCache


def relative_projection(src_proj, ref_proj):
    """models/CasMVSNet.py:622-625 and :290-292 on the host, in float64: proj (2,4,4) arrays / tensors ->
    12 floats: rows of (src @ inv(ref))[:3,:3] then [:3,3]."""
    def comb(P):
        P = np.asarray(P.detach().cpu() if torch.is_tensor(P) else P, np.float64)
        out = P[0].copy()
        out[:3, :4] = P[1][:3, :3] @ P[0][:3, :4]
        return out
    rel = comb(src_proj) @ np.linalg.inv(comb(ref_proj))
    return list(rel[:3, :3].reshape(-1)) + list(rel[:3, 3])


_HOST_CACHE = TensorCache(entries=64)
_RT_CACHE = TensorCache(entries=64)
# bounded by bytes (a 32 x 1200 x 1600 float32 map and its copy are 490 MB), not by entries; `clear_caches()` drops everything
# at the end of a scan / stage loop.  A raw-pointer writer does not bump the version counter (svs_hip/tensor_cache.py): the
# FeatureNet wrappers hand out fresh tensors.
_HWC_CACHE = TensorCache(nbytes=int(os.environ.get("SVS_HWC_CACHE_BYTES", str(1 << 30))))
_WFRAG_CACHE = TensorCache()               # the 3-D U-Net's weight fragments: a few MB per model, never dropped
_W2D_CACHE = TensorCache(entries=65)
_W2D_MFMA_CACHE = TensorCache(entries=65)
_DECONV_FRAG_CACHE = TensorCache(entries=65)
_EXTRACTORS = weakref.WeakSet()             # live feature-extractor wrappers: clear_caches() drops their tables and workspaces


def host_copy(t):
    """numpy copy of a small device tensor whose VALUES are launch arguments (projection matrices, the depth range):
    one device-to-host copy per distinct tensor, cached on storage + version -- the sample of a scan is the same
    tensor in every stage and every stage-loop iteration, so the stage loop runs without host synchronisation."""
    return _HOST_CACHE.get(t, lambda: t.detach().cpu().numpy())


def _rot_trans(proj_matrices):
    """(1,V,2,4,4) projection matrices -> ctypes float[12*(V-1)] for svs_warp_variance (host launch arguments).
    Cached per tensor like host_copy: a stage's matrices are the same tensor in every iteration of the stage loop."""
    def make():
        P = host_copy(proj_matrices)[0]
        n_src = P.shape[0] - 1
        rt = (ctypes.c_float * (12 * n_src))()
        for v in range(n_src):
            for k, x in enumerate(relative_projection(P[v + 1], P[0])):
                rt[12 * v + k] = float(x)
        return rt
    return _RT_CACHE.get(proj_matrices, make)


def _hwc(f):
    """(C,H,W) source feature map -> its channel-last copy (H,W,C), cached per tensor (storage + version): a view's
    features are built once per scan and warped in every cost-volume build of the stage loop."""
    def make():
        C, H, W = f.shape
        o = torch.empty(H, W, C, device=f.device)
        _lib.check(_lib.load().svs_chw_to_hwc(_ptr(_f32(f)), _ptr(o), C, H, W, _stream()), "svs_chw_to_hwc")
        return o
    return _HWC_CACHE.get(f, make, nbytes=2 * f.numel() * 4)


def clear_caches():
    """Drop the cached channel-last feature maps and projection constants, the feature extractors' tables and workspaces, and
    the prior look-up's per-view constants (end of a scan / stage loop; StageLoop calls it per scan, VolOpt.get_mvs_input per
    stage)."""
    _HWC_CACHE.clear()
    _RT_CACHE.clear()
    _DECONV_FRAG_CACHE.clear()
    for net in list(_EXTRACTORS):
        net.forget()
    from . import ops
    ops.clear_lookup_caches()


class SplitVolume:
    """A (C,D,H,W) volume in the form conv0 of the regularisation U-Net reads (include/svolsdf_hip.h,
    svs_split_volume_dims): fp16 hi / mid parts, channel-last 16-byte units, zero border.  The buffers are cached per
    shape: the border is zeroed once, producers rewrite the interior."""
    _cache = {}

    def __init__(self, C, D, H, W, device):
        L = _lib.load()
        self.C, self.D, self.H, self.W = C, D, H, W
        self.shape = (1, C, D, H, W)
        # (one buffer per shape AND stream: views processed on concurrent streams must not share it)
        key = (C, D, H, W, str(device), torch.cuda.current_stream(device).cuda_stream if torch.device(device).type == "cuda" else 0)
        buf = SplitVolume._cache.get(key)
        if buf is None:
            if len(SplitVolume._cache) >= 16:
                SplitVolume._cache.clear()
            nbytes = L.svs_split_volume_dims(C, D, H, W, None)
            buf = SplitVolume._cache[key] = torch.zeros(nbytes // 2, dtype=torch.float16, device=device)
        self.buf = buf
        self.device = buf.device
        # the buffer is shared by every SplitVolume of this shape and stream: a new one takes it over, and a holder of an
        # older object must not read it any more (`check_current`, called by the consumers)
        self._key = key
        self.generation = SplitVolume._generation[key] = SplitVolume._generation.get(key, 0) + 1

    _generation = {}

    def check_current(self):
        if SplitVolume._generation.get(self._key) != self.generation:
            raise RuntimeError("this SplitVolume's buffer has been reused by a later volume of the same shape on the same "
                               "stream (the buffers are cached per shape); consume a split volume before building the next")

    @staticmethod
    def pack(x):
        """float32 (C,D,H,W) -> SplitVolume"""
        L = _lib.load()
        x = _f32(x)
        C, D, H, W = x.shape
        sv = SplitVolume(C, D, H, W, x.device)
        _lib.check(L.svs_split_volume_pack(_ptr(x), _ptr(sv.buf), C, D, H, W, _stream()), "svs_split_volume_pack")
        return sv

    def float(self):
        """back to float32 (C,D,H,W): hi + mid (tests)"""
        self.check_current()
        L = _lib.load()
        dims = (ctypes.c_int * 2)()
        L.svs_split_volume_dims(self.C, self.D, self.H, self.W, dims)
        Hp, Wp = dims[0], dims[1]
        G = self.C // 8
        v = self.buf.view(self.D + 2, Hp, 2, G, Wp, 8)[1:self.D + 1, 1:self.H + 1, :, :, 1:self.W + 1].float()
        return (v[:, :, 0] + v[:, :, 1]).permute(2, 4, 0, 1, 3).reshape(self.C, self.D, self.H, self.W)


def pair_supported(C, Cout):
    return C in (8, 16, 32) and Cout <= 8


def split_fits(C, D, H, W):
    """Can svs_warp_variance_split produce this volume?  Its producer addresses the split volume and the feature maps with
    32-bit byte offsets: the bounds are those of launch_warp_reuse2 (csrc/svs_costvol.hip, THE BOUNDS OF THE SPLIT FORM)."""
    return _lib.load().svs_split_volume_dims(C, D, H, W, None) < (1 << 32) and H * W * C * 4 < (1 << 31)


def _warp_inputs(features, proj_matrices, depth_values):
    """What both cost-volume builders hand to the library: the reference feature (C,H,W), the channel-last source features,
    the relative projections and the hypotheses (D,H,W)."""
    ref = _f32(features[0][0])
    return ref, [_hwc(f[0]) for f in features[1:]], _rot_trans(proj_matrices), _f32(depth_values[0])


def warp_variance(features, proj_matrices, depth_values, split=False):
    """DepthNet.forward step 2 (models/CasMVSNet.py:611-642).  features: list of (1,C,H,W) (reference first),
    proj_matrices: (1,V,2,4,4), depth_values (1,D,H,W) -> variance (1,C,D,H,W), or with split=True the same values
    as a SplitVolume (the producer side of the fused conv0, svs_conv3d_pair) where `split_fits`."""
    L = _lib.load()
    ref, hwc, rt, dv = _warp_inputs(features, proj_matrices, depth_values)
    (C, H, W), D = ref.shape, dv.shape[0]
    if split and split_fits(C, D, H, W):
        sv = SplitVolume(C, D, H, W, ref.device)
        _lib.check(L.svs_warp_variance_split(_ptr(ref), _ptr_array(hwc), rt, len(hwc), C, D, H, W, _ptr(dv), _ptr(sv.buf),
                                             _stream()), "svs_warp_variance_split")
        return sv
    var = torch.empty(1, C, D, H, W, device=ref.device)
    _lib.check(L.svs_warp_variance(_ptr(ref), _ptr_array(hwc), rt, len(hwc), C, D, H, W, _ptr(dv), _ptr(var), 0, _stream()),
               "svs_warp_variance")
    return var


def homo_warp(src_fea, src_rel, depth_values):
    """homo_warping alone (models/CasMVSNet.py:280-315).  src_fea (C,H,W), src_rel: 12 floats
    (rows of (src_proj @ inv(ref_proj))[:3,:3], then [:3,3]), depth_values (D,H,W) -> (C,D,H,W)."""
    L = _lib.load()
    src = _f32(src_fea)
    C, H, W = src.shape
    dv = _f32(depth_values)
    D = dv.shape[0]
    hwc = torch.empty(H, W, C, device=src.device)
    _lib.check(L.svs_chw_to_hwc(_ptr(src), _ptr(hwc), C, H, W, _stream()), "svs_chw_to_hwc")
    rt = (ctypes.c_float * 12)(*[float(x) for x in src_rel])
    out = torch.empty(C, D, H, W, device=src.device)
    _lib.check(L.svs_warp_variance(_ptr(src), _ptr_array([hwc]), rt, 1, C, D, H, W, _ptr(dv), _ptr(out), 1, _stream()),
               "svs_warp_variance")
    return out


def _packed_fragments(weight, cache, tag, nbytes, pack, what):
    """The MFMA A fragments of a weight tensor, packed on the device by the library and cached per tensor (address + version)
    under `tag`: nbytes(L) -> the buffer's size, pack(L, w, frag, stream) -> the library's return code, `what` names the call.
    The float32 copy the packer reads asynchronously is kept with the buffer."""
    def make():
        L = _lib.load()
        w = _f32(weight.detach())
        frag = torch.empty(nbytes(L), dtype=torch.uint8, device=weight.device)
        _lib.check(pack(L, _ptr(w), _ptr(frag), _stream()), what)
        return frag, w
    return cache.get(weight, make, tag=tag)[0]


def mfma_weight_fragments(weight):
    """[Cin][27][Cout] folded float32 weights -> the A fragments of svs_conv3d_mfma"""
    Cin, _, Cout = weight.shape
    return _packed_fragments(weight, _WFRAG_CACHE, "mfma", lambda L: L.svs_conv3d_mfma_wfrag_bytes(Cin),
                             lambda L, w, f, s: L.svs_conv3d_mfma_pack(w, Cin, Cout, f, s), "svs_conv3d_mfma_pack")


def pair_weight_fragments(weight):
    """[Cin][27][Cout <= 8] folded float32 weights -> the A fragments of svs_conv3d_pair"""
    Cin, _, Cout = weight.shape
    return _packed_fragments(weight, _WFRAG_CACHE, "pair", lambda L: L.svs_conv3d_pair_wfrag_bytes(Cin),
                             lambda L, w, f, s: L.svs_conv3d_pair_pack(w, Cin, Cout, f, s), "svs_conv3d_pair_pack")


def rows_weight_fragments(weight):
    """[16][27][Cout <= 16] folded float32 weights -> the A fragments of svs_conv3d_rows"""
    Cin, _, Cout = weight.shape
    return _packed_fragments(weight, _WFRAG_CACHE, "rows", lambda L: L.svs_conv3d_rows_wfrag_bytes(Cin),
                             lambda L, w, f, s: L.svs_conv3d_rows_pack(w, Cin, Cout, f, s), "svs_conv3d_rows_pack")


def s2c8_weight_fragments(weight):
    """[8][27][Cout <= 16] folded float32 weights -> the A fragments of svs_conv3d_s2c8"""
    Cout = weight.shape[2]
    return _packed_fragments(weight, _WFRAG_CACHE, "s2c8", lambda L: L.svs_conv3d_s2c8_wfrag_bytes(),
                             lambda L, w, f, s: L.svs_conv3d_s2c8_pack(w, Cout, f, s), "svs_conv3d_s2c8_pack")


def gemm_weight_fragments(weight, transposed):
    """[Cin][27][Cout] folded float32 weights -> the A fragments of svs_conv3d_gemm"""
    Cin, _, Cout = weight.shape
    t = int(bool(transposed))
    return _packed_fragments(weight, _WFRAG_CACHE, ("gemm", bool(transposed)), lambda L: L.svs_conv3d_gemm_wfrag_bytes(Cin, Cout, t),
                             lambda L, w, f, s: L.svs_conv3d_gemm_pack(w, Cin, Cout, t, f, s), "svs_conv3d_gemm_pack")


def conv2d_pack(weight):
    """(Cout,Cin,k,k) -> [ceil(Cout/8)][Cin][k][k][8] float32, the layout svs_conv2d reads through the scalar cache
    (include/svolsdf_hip.h).  Cached per weight tensor (address + version)."""
    def make():
        Cout, Cin, k, _ = weight.shape
        G = (Cout + 7) // 8
        w = torch.zeros(G * 8, Cin, k, k, device=weight.device, dtype=torch.float32)
        w[:Cout] = weight.detach().float()
        return w.view(G, 8, Cin, k, k).permute(0, 2, 3, 4, 1).contiguous()
    return _W2D_CACHE.get(weight, make)


def conv2d(x, weight, bias=None, add=None, add_upsample2=False, stride=1, relu=False, out=None):
    """FeatureNet convolution (csrc/svs_conv2d.hip): x (Cin,H,W), weight (Cout,Cin,k,k) with BatchNorm folded, padding
    k // 2 -> (Cout,Ho,Wo) = [add +] relu?(conv + bias); add_upsample2: `add` is at half resolution (nearest x2)."""
    L = _lib.load()
    x = _f32(x)
    Cin, H, W = x.shape
    Cout, cin_w, k, k2 = weight.shape
    if cin_w != Cin or k != k2:
        raise ValueError("weight shape does not match the input")
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if out is None:
        out = torch.empty(Cout, Ho, Wo, device=x.device)
    elif tuple(out.shape) != (Cout, Ho, Wo) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("out must be a contiguous float32 (Cout,Ho,Wo) tensor")
    bias = _f32(bias) if bias is not None else None
    add = _f32(add) if add is not None else None
    if add is not None and tuple(add.shape) != ((Cout, Ho // 2, Wo // 2) if add_upsample2 else (Cout, Ho, Wo)):
        raise ValueError("addend shape does not match the output")
    _lib.check(L.svs_conv2d(_ptr(x), _ptr(conv2d_pack(weight)), _ptr(bias), _ptr(add), int(bool(add_upsample2)), _ptr(out), Cin,
                            Cout, H, W, k, stride, int(bool(relu)), _stream()), "svs_conv2d")
    return out


def conv2d_mfma_supported(Cin, Cout, k, stride):
    return bool(_lib.load().svs_conv2d_mfma_supported(int(Cin), int(Cout), int(k), int(stride)))


def conv2d_mfma_frag(weight):
    """(Cout,Cin,k,k) float32 -> the A fragments of svs_conv2d_mfma"""
    Cout, Cin, k, _ = weight.shape
    return _packed_fragments(weight, _W2D_MFMA_CACHE, None, lambda L: L.svs_conv2d_mfma_wfrag_bytes(Cin, Cout, k),
                             lambda L, w, f, s: L.svs_conv2d_mfma_pack(w, Cin, Cout, k, f, s), "svs_conv2d_mfma_pack")


def conv2d_mfma(x, weight, bias=None, stride=1, relu=False):
    """A FeatureNet 3x3 (stride 1) / 5x5 (stride 2) convolution on the matrix cores (csrc/svs_conv2d_mfma.hip): x (Cin,H,W),
    weight (Cout,Cin,k,k), padding k // 2 -> (Cout,Ho,Wo) = relu?(conv + bias), float32 class (fp16x2)."""
    L = _lib.load()
    x = _f32(x)
    Cin, H, W = x.shape
    Cout, cin_w, k, k2 = weight.shape
    if cin_w != Cin or k != k2 or not conv2d_mfma_supported(Cin, Cout, k, stride):
        raise ValueError("shape not supported by svs_conv2d_mfma")
    pad = k // 2
    out = torch.empty(Cout, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, device=x.device)
    bias = _f32(bias) if bias is not None else None
    _lib.check(L.svs_conv2d_mfma(_ptr(x), _ptr(conv2d_mfma_frag(weight)), _ptr(bias), _ptr(out), Cin, Cout, H, W, k, stride,
                                 int(bool(relu)), _stream()), "svs_conv2d_mfma")
    return out


def conv2d_mfma_lateral(lat_in, lat_weight, lat_bias, lat_add, weight, bias=None, relu=False):
    """The FPN's lateral step fused into the 3x3 layer behind it (svs_conv2d_mfma_lateral): lat_in (8,H,W), lat_weight (32,8,1,1),
    lat_add (32,H/2,W/2), weight (Cout<=16,32,3,3) -> (Cout,H,W) = relu?(conv3x3(conv1x1(lat_in) + lat_bias + up2(lat_add)) + bias)."""
    L = _lib.load()
    lat_in, lat_add = _f32(lat_in), _f32(lat_add)
    _, H, W = lat_in.shape
    Cout = weight.shape[0]
    out = torch.empty(Cout, H, W, device=lat_in.device)
    lb = _f32(lat_bias) if lat_bias is not None else None
    bb = _f32(bias) if bias is not None else None
    _lib.check(L.svs_conv2d_mfma_lateral(_ptr(lat_in), _ptr(conv2d_pack(lat_weight)), _ptr(lb), _ptr(lat_add), _ptr(conv2d_mfma_frag(weight)),
                                         _ptr(bb), _ptr(out), Cout, H, W, int(bool(relu)), _stream()), "svs_conv2d_mfma_lateral")
    return out


class _FeatureExtractor:
    """A 2-D feature extractor enqueued by ONE library call: the per-launch host cost of going through Python once per layer
    was as large as the kernels' run time.  Owns the workspace and the pointer tables (cached until a tensor changes;
    clear_caches() drops both through forget()).  A subclass states its layers and which of them run on the matrix cores."""
    LAYERS = 0              # number of layers
    ENTRY = WORKSPACE = ""  # the library's entry point and its workspace-size function
    STRIDES = ()            # layer index -> stride
    TRANSPOSED = ()         # transposed layers: weight (Cin,Cout,3,3), handed over as it is
    ADDEND = ()             # layers that take an addend: float32 kernels

    def __init__(self, base_channels):
        self.b = int(base_channels)
        self.forget()
        _EXTRACTORS.add(self)

    def forget(self):
        self._ws, self._ws_key = None, None
        self._tables = Derived()

    def fragment(self, i, w):
        """the MFMA fragments of layer i, or None: the layer runs on the float32 kernels"""
        raise NotImplementedError

    def _conv_fragment(self, i, w):
        # the 3x3 / 5x5 layers with 8 / 16 / 32 input channels run on the matrix cores (svs_conv2d_mfma)
        # (not conv0.1, 8 -> 8 at full resolution: 15.5 us there against 13.4 on the vector kernel -- a quarter-full M tile)
        if (i not in self.ADDEND and w.shape[2] > 1 and not (w.shape[1] <= 8 and w.shape[2] == 3)
                and conv2d_mfma_supported(w.shape[1], w.shape[0], w.shape[2], self.STRIDES[i])):
            return conv2d_mfma_frag(w)
        return None

    def tables(self, layers):
        """layers: LAYERS (weight, bias or None) pairs in the library's order, convolutions (Cout,Cin,k,k), transposed layers
        (Cin,Cout,3,3) -> pointer tables (cached until a tensor changes)."""
        def make():
            packed = [_f32(w.detach()) if i in self.TRANSPOSED else conv2d_pack(w) for i, (w, _) in enumerate(layers)]
            biases = [None if b is None else _f32(b) for _, b in layers]
            frags = [self.fragment(i, w) for i, (w, _) in enumerate(layers)]
            return (_ptr_array(packed), _ptr_array(biases), packed, biases, layers, _ptr_array(frags), frags)
        return self._tables([t for pair in layers for t in pair if t is not None], make)

    def __call__(self, image, layers):
        """image (3,H,W) -> stage1 (4b,H/4,W/4), stage2 (2b,H/2,W/2), stage3 (b,H,W)."""
        L = _lib.load()
        if len(layers) != self.LAYERS:
            raise ValueError(f"{self.LAYERS} layers expected")
        image = _f32(image)
        _, H, W = image.shape
        if image.shape[0] != 3 or H % 4 or W % 4:
            raise ValueError("image must be (3,H,W) with H, W multiples of 4")
        dev, b = image.device, self.b
        if self._ws_key != (H, W, dev):
            self._ws = torch.empty(getattr(L, self.WORKSPACE)(b, H, W) // 4, device=dev)
            self._ws_key = (H, W, dev)
        tb = self.tables(layers)
        wt, bt, ft = tb[0], tb[1], tb[5]
        s1 = torch.empty(4 * b, H // 4, W // 4, device=dev)
        s2 = torch.empty(2 * b, H // 2, W // 2, device=dev)
        s3 = torch.empty(b, H, W, device=dev)
        _lib.check(getattr(L, self.ENTRY)(_ptr(image), H, W, b, wt, bt, ft, _ptr(self._ws), _ptr(s1), _ptr(s2), _ptr(s3), _stream()),
                   self.ENTRY)
        return s1, s2, s3


_FPN_MFMA = os.environ.get("SVS_FPN_MFMA", "1") != "0"     # A/B: 0 = every layer of the pyramid on the float32 vector kernels


class FeatureNetFpn(_FeatureExtractor):
    """The 13 convolutions of the 'fpn' FeatureNet (svs_featurenet_fpn2)."""
    LAYERS, ENTRY, WORKSPACE = 13, "svs_featurenet_fpn2", "svs_featurenet_fpn_workspace_bytes"
    STRIDES = (1, 1, 2, 1, 1, 2, 1, 1, 1, 1, 1, 1, 1)
    ADDEND = (9, 11)                                       # the lateral 1x1 convolutions

    def fragment(self, i, w):
        return self._conv_fragment(i, w) if _FPN_MFMA else None


# ---------------------------------------------------------------------------------------------------------------------
# UCSNet (models/ucsnet.py; csrc/svs_ucsnet.hip)
# ---------------------------------------------------------------------------------------------------------------------
def deconv2d_mfma_supported(Cin, Cout):
    return bool(_lib.load().svs_deconv2d_mfma_supported(int(Cin), int(Cout)))


def deconv2d_mfma_frag(weight):
    """(Cin,Cout,3,3) float32 -> the A fragments of svs_deconv2d_mfma"""
    Cin, Cout = weight.shape[:2]
    return _packed_fragments(weight, _DECONV_FRAG_CACHE, None, lambda L: L.svs_deconv2d_mfma_wfrag_bytes(Cin, Cout),
                             lambda L, w, f, s: L.svs_deconv2d_mfma_pack(w, Cin, Cout, f, s), "svs_deconv2d_mfma_pack")


def deconv2d(x, weight, bias=None, relu=False, out=None, mfma=None):
    """Deconv2dUnit's transposed convolution (models/ucsnet.py:135, 225: k3, s2, p1, output_padding 1): x (Cin,H,W), weight
    (Cin,Cout,3,3) with BatchNorm folded -> (Cout,2H,2W) = relu?(conv_transpose2d + bias).  out: a contiguous float32
    (C >= Cout, 2H, 2W) tensor whose first Cout channels are written (a concatenation buffer).  mfma: True = svs_deconv2d_mfma
    (raises for unsupported shapes), False = the float32 vector kernel, None = the matrix cores where they support the shape."""
    L = _lib.load()
    x = _f32(x)
    Cin, H, W = x.shape
    if weight.dim() != 4 or weight.shape[0] != Cin or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("weight must be (Cin,Cout,3,3)")
    Cout = weight.shape[1]
    if out is None:
        out = torch.empty(Cout, 2 * H, 2 * W, device=x.device)
    elif (out.dim() != 3 or out.shape[0] < Cout or tuple(out.shape[1:]) != (2 * H, 2 * W) or not out.is_contiguous()
          or out.dtype != torch.float32):
        raise ValueError("out must be a contiguous float32 (C >= Cout, 2H, 2W) tensor")
    if mfma is None:
        mfma = deconv2d_mfma_supported(Cin, Cout)
    elif mfma and not deconv2d_mfma_supported(Cin, Cout):
        raise ValueError("shape not supported by svs_deconv2d_mfma")
    bias = _f32(bias) if bias is not None else None
    if mfma:
        _lib.check(L.svs_deconv2d_mfma(_ptr(x), _ptr(deconv2d_mfma_frag(weight)), _ptr(bias), _ptr(out), 4 * H * W, Cin, Cout, H, W,
                                       int(bool(relu)), _stream()), "svs_deconv2d_mfma")
    else:
        _lib.check(L.svs_deconv2d(_ptr(x), _ptr(_f32(weight.detach())), _ptr(bias), _ptr(out), 4 * H * W, Cin, Cout, H, W,
                                  int(bool(relu)), _stream()), "svs_deconv2d")
    return out


class FeatureNetUnet(_FeatureExtractor):
    """The 15 layers of UCSNet's FeatExtNet (models/ucsnet.py:237-302; svs_featurenet_unet); the two concatenations are formed
    in place in the workspace."""
    LAYERS, ENTRY, WORKSPACE = 15, "svs_featurenet_unet", "svs_featurenet_unet_workspace_bytes"
    STRIDES = (1, 1, 2, 1, 1, 2, 1, 1, 1, 2, 1, 1, 2, 1, 1)
    TRANSPOSED = (9, 12)

    def __init__(self, base_channels, mfma=None, deconv_mfma=None):
        """mfma = False: every layer on the float32 kernels.  deconv_mfma: True / False = both transposed layers on the matrix
        cores / on the float32 kernel (the A/B comparison of tools/bench_ucsnet.py); None = the default, see fragment()."""
        self.mfma = True if mfma is None else bool(mfma)
        self.deconv_mfma = (None if self.mfma else False) if deconv_mfma is None else bool(deconv_mfma)
        super().__init__(base_channels)

    def fragment(self, i, w):
        if i not in self.TRANSPOSED:
            return self._conv_fragment(i, w) if self.mfma else None
        # deconv1.deconv (32 -> 16) on the matrix cores: 0.017 ms against 0.041 at 288 x 384 -> 576 x 768.  Not
        # deconv2.deconv (16 -> 8, a half-full M tile): alone it is not faster there, 0.039 ms against 0.038 at
        # 576 x 768 -> 1152 x 1536 with overlapping ranges, cause not established; inside the extractor the choice
        # moves the 0.51 ms per image by about 1 % the other way (profiles/ucsnet_bench.txt)
        on = w.shape[1] > 8 if self.deconv_mfma is None else self.deconv_mfma
        return deconv2d_mfma_frag(w) if on and deconv2d_mfma_supported(w.shape[0], w.shape[1]) else None


def _tail(entry, reg, depth_values, lamb=None):
    """One softmax tail (csrc/svs_costvol.hip: launch_tail): reg (D,H,W), depth_values (D,H,W) -> prob (D,H,W), depth (H,W), conf
    (H,W), index (H,W int32); with lamb also the per-pixel uncertainty (H,W)."""
    L = _lib.load()
    reg, dv = _f32(reg), _f32(depth_values)
    D, H, W = reg.shape
    dev = reg.device
    prob = torch.empty(D, H, W, device=dev)
    depth, conf = torch.empty(H, W, device=dev), torch.empty(H, W, device=dev)
    idx = torch.empty(H, W, dtype=torch.int32, device=dev)
    args = (_ptr(reg), _ptr(dv), D, H, W)
    out = (_ptr(prob), _ptr(depth), _ptr(conf), _ptr(idx))
    if lamb is None:
        _lib.check(getattr(L, entry)(*args, *out, _stream()), entry)
        return prob, depth, conf, idx
    var = torch.empty(H, W, device=dev)
    _lib.check(getattr(L, entry)(*args, float(lamb), *out, _ptr(var), _stream()), entry)
    return prob, depth, conf, idx, var


def prob_depth_conf_var(reg, depth_values, lamb):
    """compute_depth's tail (models/ucsnet.py:381-394): reg (D,H,W), depth_values (D,H,W) -> prob (D,H,W), depth (H,W), conf
    (H,W), index (H,W int32) as prob_depth_conf gives them, and variance (H,W) = lamb * sqrt(sum_d prob_d (z_d - depth)^2)."""
    return _tail("svs_prob_depth_conf_var", reg, depth_values, lamb)


def uncertainty_hypotheses(prev_depth, prev_var, hw, ndepth, dmin=None, dmax=None, inverse=False, device=None):
    """uncertainty_aware_samples (models/ucsnet.py:44-72) -> (D,) + hw.  prev_depth None: stage 1, D planes dmin..dmax (linear,
    or linear in 1/depth), the same for every pixel (svs_depth_hypotheses).  Else prev_depth, prev_var (Hp,Wp): both resized
    bilinearly to hw, D samples from cur - min(cur, var) to cur + var."""
    L = _lib.load()
    Hs, Ws = hw
    if prev_depth is None:
        return depth_hypotheses(None, (Hs, Ws), ndepth, 1, dmin, dmax, 0.0, inverse, device)
    pd, pv = _f32(prev_depth), _f32(prev_var)
    out = torch.empty(max(int(ndepth), 0), Hs, Ws, device=pd.device)
    _lib.check(L.svs_uncertainty_hypotheses(_ptr(pd), pd.shape[-2], pd.shape[-1], _ptr(pv), pv.shape[-2], pv.shape[-1], Hs, Ws,
                                            int(ndepth), _ptr(out), _stream()), "svs_uncertainty_hypotheses")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# TransMVSNet (models/transmvs.py; csrc/svs_transmvs.hip, the tail in csrc/svs_costvol.hip)
# ---------------------------------------------------------------------------------------------------------------------
def deform_conv2d(x, offset_mask, weight, bias=None, scale=None, shift=None, relu=False):
    """DCN.forward behind its conv_offset_mask (models/dcn.py:68-80: torchvision's deform_conv2d, 3x3, stride 1, padding 1, one
    offset group, modulated): x (32,H,W), offset_mask (27,H,W) the raw conv_offset_mask output (channels 2k, 2k+1 = dy, dx of
    tap k = 3 ky + kx; channel 18+k -> sigmoid = its mask), weight (Cout <= 32,32,3,3) -> (Cout,H,W) =
    relu?(scale * (deform_conv + bias) + shift); scale / shift (both or neither): the folded BatchNorm behind the layer."""
    L = _lib.load()
    x, om = _f32(x), _f32(offset_mask)
    Cin, H, W = x.shape
    Cout = weight.shape[0]
    if Cin != 32 or tuple(om.shape) != (27, H, W) or tuple(weight.shape[1:]) != (32, 3, 3):
        raise ValueError("deform_conv2d: x (32,H,W), offset_mask (27,H,W), weight (Cout,32,3,3)")
    if (scale is None) != (shift is None):
        raise ValueError("deform_conv2d: scale and shift come together")
    opt = lambda t: _f32(t) if t is not None else None
    bias, scale, shift = opt(bias), opt(scale), opt(shift)
    out = torch.empty(Cout, H, W, device=x.device)
    _lib.check(L.svs_deform_conv2d(_ptr(x), _ptr(om), _ptr(conv2d_pack(weight)), _ptr(bias), _ptr(scale), _ptr(shift), _ptr(out),
                                   Cout, H, W, int(bool(relu)), _stream()), "svs_deform_conv2d")
    return out


_PE_DIV = []


def _pe_div_term():
    """PositionEncodingSine(32, temp_bug_fix=True)'s eight frequencies, in float32 as models/position_encoding.py:43 forms them."""
    if not _PE_DIV:
        import math
        div = torch.exp(torch.arange(0, 16, 2).float() * (-math.log(10000.0) / 16))
        _PE_DIV.append((ctypes.c_float * 8)(*[float(v) for v in div]))
    return _PE_DIV[0]


def fmt_tokens_in(feature):
    """(32,H,W) -> (H*W,32) tokens with PositionEncodingSine added (models/FMT.py:147, 163)."""
    L = _lib.load()
    f = _f32(feature)
    C, H, W = f.shape
    if C != 32:
        raise ValueError("the transformer's d_model is 32")
    tok = torch.empty(H * W, 32, device=f.device)
    _lib.check(L.svs_fmt_tokens_in(_ptr(f), H, W, _pe_div_term(), _ptr(tok), _stream()), "svs_fmt_tokens_in")
    return tok


def fmt_tokens_out(tokens, hw):
    """(H*W,32) tokens -> (32,H,W)"""
    L = _lib.load()
    t = _f32(tokens)
    H, W = hw
    if tuple(t.shape) != (H * W, 32):
        raise ValueError("tokens must be (H*W,32)")
    out = torch.empty(32, H, W, device=t.device)
    _lib.check(L.svs_fmt_tokens_out(_ptr(t), H, W, _ptr(out), _stream()), "svs_fmt_tokens_out")
    return out


def fmt_kv(source, k_w, k_b, v_w, v_b):
    """LinearAttention's sums over the S source tokens (models/FMT.py:24-32): source (S,32) -> 160 floats, KV[h][m][d] =
    sum_s K[s,h,d] V[s,h,m] (128) then Ksum[h][d] (32), K = elu(W_k s + b_k) + 1, V = W_v s + b_v.  Summed in a fixed order:
    two calls on the same input give the same bits."""
    L = _lib.load()
    src = _f32(source)
    S = src.shape[0]
    if src.dim() != 2 or src.shape[1] != 32:
        raise ValueError("source must be (S,32)")
    ws = torch.empty(L.svs_fmt_kv_workspace_bytes(S) // 4, device=src.device)
    out = torch.empty(160, device=src.device)
    _lib.check(L.svs_fmt_kv(_ptr(src), S, _ptr(_f32(k_w)), _ptr(_f32(k_b)), _ptr(_f32(v_w)), _ptr(_f32(v_b)), _ptr(ws), _ptr(out),
                            _stream()), "svs_fmt_kv")
    return out


def fmt_layer(x, kvsum, weights):
    """EncoderLayer.forward (models/FMT.py:96-111) for the query tokens x (L,32), given fmt_kv's sums of its source.  weights: the
    12 tensors query_projection.{weight,bias}, out_projection.{weight,bias}, linear1.{weight,bias}, linear2.{weight,bias},
    norm1.{weight,bias}, norm2.{weight,bias}."""
    L = _lib.load()
    x = _f32(x)
    if x.dim() != 2 or x.shape[1] != 32 or len(weights) != 12 or kvsum.numel() != 160:
        raise ValueError("fmt_layer: x (L,32), 160 sums, 12 weight tensors")
    ws = [_f32(w) for w in weights]
    out = torch.empty_like(x)
    _lib.check(L.svs_fmt_layer(_ptr(x), x.shape[0], _ptr(_f32(kvsum)), _ptr_array(ws), _ptr(out), _stream()), "svs_fmt_layer")
    return out


def pathway_step(x, weight, y):
    """_upsample_add(dim_reduction(x), y) (models/FMT.py:196-223): x (Cin,h,w), weight (Cin/2,Cin,1,1), y (Cin/2,2h,2w) ->
    bilinear_x2(conv1x1(x)) + y, align_corners=False, the reduction first."""
    L = _lib.load()
    x, y = _f32(x), _f32(y)
    Cin, h, w = x.shape
    if tuple(weight.shape[:2]) != (Cin // 2, Cin) or tuple(y.shape) != (Cin // 2, 2 * h, 2 * w):
        raise ValueError("pathway_step: shapes do not match")
    out = torch.empty_like(y)
    _lib.check(L.svs_pathway_step(_ptr(x), _ptr(_f32(weight.detach().reshape(Cin // 2, Cin))), _ptr(y), _ptr(out), Cin, h, w,
                                  _stream()), "svs_pathway_step")
    return out


def warp_similarity(features, proj_matrices, depth_values, view_weights=None, net=None):
    """DepthNet.forward steps 1-2 (models/TransMVSNet.py:52-91) with the homo_warping of models/module.py:285-324.  features: list
    of (1,C,H,W) (reference first), proj_matrices (1,V,2,4,4), depth_values (1,D,H,W).  view_weights None (stage 1): net = the
    177 folded floats of pixel_wise_net, the weights are max_d sigmoid(net(sim_v)); else (1,V-1,H/2,W/2), the previous stage's,
    read at (y/2, x/2).  -> similarity (1,1,D,H,W), the weights at this stage's size (1,V-1,H,W)."""
    L = _lib.load()
    ref, hwc, rt, dv = _warp_inputs(features, proj_matrices, depth_values)
    (C, H, W), D, dev, n_src = ref.shape, dv.shape[0], ref.device, len(hwc)
    if view_weights is not None:
        pw = _f32(view_weights[0])
        if tuple(pw.shape) != (n_src, H // 2, W // 2) or H % 2 or W % 2:
            raise ValueError("view_weights must be (1,V-1,H/2,W/2)")
    else:
        pw = None
        if net is None or net.numel() != 177:
            raise ValueError("stage 1 needs pixel_wise_net's 177 folded floats")
        net = _f32(net)
    ws = torch.empty(L.svs_warp_similarity_workspace_bytes(n_src, D, H, W) // 4, device=dev)
    sim = torch.empty(1, 1, D, H, W, device=dev)
    w_out = torch.empty(1, n_src, H, W, device=dev)
    _lib.check(L.svs_warp_similarity(_ptr(ref), _ptr_array(hwc), rt, n_src, C, D, H, W, _ptr(dv), _ptr(pw),
                                     _ptr(net) if pw is None else None, _ptr(ws), _ptr(sim), _ptr(w_out), _stream()),
               "svs_warp_similarity")
    return sim, w_out


def prob_wta(reg, depth_values):
    """TransMVSNet's tail (models/TransMVSNet.py:100-109, 225-227): reg (D,H,W), depth_values (D,H,W) -> prob (D,H,W) as
    prob_depth_conf gives it, index (H,W int32) = the first argmax, depth = depth_values[index], conf = prob[index]."""
    return _tail("svs_prob_wta", reg, depth_values)


_GEMM_ON = [True]


def gemm_enabled(on=None):
    """The MFMA implicit-GEMM path for the strided / transposed / coarse layers (svs_conv3d_gemm); off = the VALU direct
    convolutions (kept for A/B measurements and as the fall-back for channel counts the GEMM kernel does not cover)."""
    if on is not None:
        _GEMM_ON[0] = bool(on)
    return _GEMM_ON[0]


def rows_supported(Cin, Cout):
    return Cin == 16 and Cout <= 16


def conv3d(x, weight, bias=None, skip=None, stride=1, transposed=False, relu=True, split_out=False):
    """x (Cin,D,H,W); weight [Cin][27][Cout] folded; -> (Cout,Do,Ho,Wo).  split_out: return the result as a SplitVolume (the
    stride-2 convolution from 8 to 16 channels only: conv1 feeding conv2).  bias [Cout] and skip (Cout,Do,Ho,Wo) may be views
    (a slice of a larger volume): the kernels read contiguous float32 copies of them."""
    L = _lib.load()
    bias = _f32(bias) if bias is not None else None
    skip = _f32(skip) if skip is not None else None
    if isinstance(x, SplitVolume):
        Cout = weight.shape[2]
        rows = x.C == 16 and Cout > 8                # conv2 (channel rows); otherwise conv0 (x-pair rows, Cout <= 8)
        fused = (not transposed and stride == 1 and skip is None
                 and (rows_supported(x.C, Cout) if rows else pair_supported(x.C, Cout)))
        if fused:
            x.check_current()
            out = torch.empty((Cout, x.D, x.H, x.W), device=x.device)
            if rows:
                _lib.check(L.svs_conv3d_rows(_ptr(x.buf), _ptr(rows_weight_fragments(weight)), _ptr(bias), _ptr(out), x.C, Cout,
                                             x.D, x.H, x.W, int(relu), _stream()), "svs_conv3d_rows")
            else:
                _lib.check(L.svs_conv3d_pair(_ptr(x.buf), _ptr(pair_weight_fragments(weight)), _ptr(bias), _ptr(out), x.C, Cout,
                                             x.D, x.H, x.W, int(relu), _stream()), "svs_conv3d_pair")
            return out
        x = x.float()                # no fused form for this layer: back to the float32 volume
    x = _f32(x)
    Cin, D, H, W = x.shape
    Cout = weight.shape[2]
    if not transposed and stride == 1 and Cout == 1:
        out = torch.empty((1, D, H, W), device=x.device)
        _lib.check(L.svs_conv3d_c1(_ptr(x), _ptr(_f32(weight)), _ptr(bias), _ptr(skip), _ptr(out), Cin, D, H, W, int(relu),
                                   _stream()), "svs_conv3d_c1")
        return out
    if not transposed and stride == 1 and Cin in (8, 16, 32) and Cout <= 16:
        frag = mfma_weight_fragments(weight)
        out = torch.empty((Cout, D, H, W), device=x.device)
        _lib.check(L.svs_conv3d_mfma(_ptr(x), _ptr(frag), _ptr(bias), _ptr(skip), _ptr(out), Cin, Cout, D, H, W,
                                     int(relu), _stream()), "svs_conv3d_mfma")
        return out
    if transposed:
        shp = (Cout, 2 * D, 2 * H, 2 * W)
    else:
        shp = (Cout, (D - 1) // stride + 1, (H - 1) // stride + 1, (W - 1) // stride + 1)
    out = torch.empty(shp, device=x.device)
    if not transposed and stride == 2 and Cin == 8 and Cout <= 16 and W % 2 == 0:
        frag = s2c8_weight_fragments(weight)
        if split_out and Cout == 16 and skip is None:
            sv = SplitVolume(Cout, *shp[1:], x.device)
            _lib.check(L.svs_conv3d_s2c8(_ptr(x), _ptr(frag), _ptr(bias), None, None, _ptr(sv.buf), Cout, D, H, W, int(relu),
                                         _stream()), "svs_conv3d_s2c8")
            return sv
        _lib.check(L.svs_conv3d_s2c8(_ptr(x), _ptr(frag), _ptr(bias), _ptr(skip), _ptr(out), None, Cout, D, H, W, int(relu),
                                     _stream()), "svs_conv3d_s2c8")
        return out
    if gemm_enabled() and L.svs_conv3d_gemm_supported(Cin, Cout):
        frag = gemm_weight_fragments(weight, transposed)
        _lib.check(L.svs_conv3d_gemm(_ptr(x), _ptr(frag), _ptr(bias), _ptr(skip), _ptr(out), Cin, Cout, D, H, W, stride,
                                     int(transposed), int(relu), _stream()), "svs_conv3d_gemm")
        return out
    _lib.check(L.svs_conv3d(_ptr(x), _ptr(weight), _ptr(bias), _ptr(skip), _ptr(out), Cin, Cout, D, H, W, stride,
                            int(transposed), int(relu), _stream()), "svs_conv3d")
    return out


def prob_depth_conf(reg, depth_values):
    """reg (D,H,W), depth_values (D,H,W) -> prob (D,H,W), depth (H,W), conf (H,W), index (H,W int32)."""
    return _tail("svs_prob_depth_conf", reg, depth_values)


def depth_hypotheses(prev_depth, img_hw, ndepth, scale, dmin, dmax, pix_interval, inverse, device):
    """models/CasMVSNet.py:733-751 -> (D, H/scale, W/scale)."""
    L = _lib.load()
    H, W = img_hw
    out = torch.empty(ndepth, H // scale, W // scale, device=device)
    pd = _f32(prev_depth) if prev_depth is not None else None
    Hp, Wp = (pd.shape[-2], pd.shape[-1]) if pd is not None else (0, 0)
    _lib.check(L.svs_depth_hypotheses(_ptr(pd), Hp, Wp, H, W, ndepth, scale, float(dmin), float(dmax),
                                      float(pix_interval), int(bool(inverse)), _ptr(out), _stream()),
               "svs_depth_hypotheses")
    return out
