"""The A-fragment layouts of svs_conv3d_mfma / _pair / _rows / _s2c8 as torch index arithmetic: the builders svs_hip/costvol.py
used before the library packed these layouts on the device (svs_conv3d_*_pack), kept word for word as the restatement the
device packer is checked against (tests/test_gpu_costvol.py).  They run on whatever device the weight tensor lives on.  Also
the test weights those checks and tests/golden/make_convfrag_fixture.py share.  Nothing here imports svs_hip."""
import numpy as np
import torch

# what the fp16 split meets at its edges: zeros of both signs, an exact value, a value at the edge of fp16's normal range, one
# beyond fp16's range (hi = inf, mid = -inf) and one below its subnormals (hi = mid = 0)
SPECIALS = (0.0, -0.0, 1.0, 6.1e-5, 70000.0, 1e-9)


def make_weight(shape, seed):
    """float32 CPU tensor: normal x 0.05 from a frozen stream (numpy's legacy generator), SPECIALS written over entries spread
    through the tensor, the first and the last among them: they land in rows the packers keep and beside the ones they pad."""
    w = (np.random.RandomState(seed).standard_normal(shape) * 0.05).astype(np.float32)
    flat = w.reshape(-1)
    for i, v in enumerate(SPECIALS * 3):
        flat[(i * 2654435761 + seed) % flat.size] = v
    flat[0], flat[-1] = SPECIALS[4], SPECIALS[1]
    return torch.from_numpy(w)


def _hi_mid(w, ok):
    """float32 fragment values (zero where not ok) -> (KS, 2, 64, 8) fp16: the hi piece and what it leaves, stacked per k-step"""
    w = torch.where(ok, w, torch.zeros_like(w)).float()
    hi = w.half()
    return torch.stack([hi, (w - hi.float()).half()], 1).contiguous()


def mfma_weight_fragments(weight):
    """[Cin][27][Cout] folded float32 weights -> the fp16 hi / mid A fragments of svs_conv3d_mfma
    ([k-step][piece][lane][8] fp16, see include/svolsdf_hip.h).  One-time repacking per layer (cached)."""
    Cin, _, Cout = weight.shape
    dev = weight.device
    KS = (27 * Cin + 31) // 32
    s = torch.arange(KS, device=dev).view(KS, 1, 1)
    lane = torch.arange(64, device=dev).view(1, 64, 1)
    j = torch.arange(8, device=dev).view(1, 1, 8)
    kk = 32 * s + 8 * (lane >> 4) + j
    tap, ci, co = kk // Cin, kk % Cin, (lane & 15).expand(KS, 64, 8)
    ok = (tap < 27) & (co < Cout)
    w = weight[ci.clamp(max=Cin - 1), tap.clamp(max=26), co.clamp(max=Cout - 1)]
    return _hi_mid(w, ok)


def pair_weight_fragments(weight):
    """[Cin][27][Cout <= 8] folded float32 weights -> the fp16 hi / mid A fragments of svs_conv3d_pair
    ([k-step][piece][lane][8] fp16, include/svolsdf_hip.h): row m = (channel m & 7, x parity m >> 3),
    k = (((kd*3+kh)*4 + t)*G + g)*8 + c8 carries the weight of tap (kd, kh, kw = t - parity)."""
    Cin, _, Cout = weight.shape
    dev = weight.device
    G = Cin // 8
    KS = 9 * G
    s = torch.arange(KS, device=dev).view(KS, 1, 1)
    lane = torch.arange(64, device=dev).view(1, 64, 1)
    j = torch.arange(8, device=dev).view(1, 1, 8)
    kk = 32 * s + 8 * (lane >> 4) + j
    c8, g, t, row9 = kk % 8, (kk // 8) % G, (kk // (8 * G)) % 4, kk // (32 * G)
    m = (lane & 15).expand(KS, 64, 8)
    co, kw = m & 7, t - (m >> 3)
    ok = (kw >= 0) & (kw <= 2) & (co < Cout)
    w = weight[8 * g + c8, (row9 * 3 + kw.clamp(0, 2)), co.clamp(max=Cout - 1)]
    return _hi_mid(w, ok)


def rows_weight_fragments(weight):
    """[16][27][Cout <= 16] folded float32 weights -> the fp16 hi / mid A fragments of svs_conv3d_rows
    ([k-step][piece][lane][8], include/svolsdf_hip.h): k-step s, lane group kg = combination 4 s + kg = tap * G + g."""
    Cin, _, Cout = weight.shape
    dev = weight.device
    G = Cin // 8
    KS = (27 * G + 3) // 4
    s = torch.arange(KS, device=dev).view(KS, 1, 1)
    lane = torch.arange(64, device=dev).view(1, 64, 1)
    j = torch.arange(8, device=dev).view(1, 1, 8)
    c = 4 * s + (lane >> 4)
    tap, g = (c // G).expand(KS, 64, 8), (c % G).expand(KS, 64, 8)
    co = (lane & 15).expand(KS, 64, 8)
    ok = (tap < 27) & (co < Cout)
    w = weight[8 * g + j, tap.clamp(max=26), co.clamp(max=Cout - 1)]
    return _hi_mid(w, ok)


def s2c8_weight_fragments(weight):
    """[8][27][Cout <= 16] folded float32 weights -> the fp16 hi / mid A fragments of svs_conv3d_s2c8
    ([9 k-steps][piece][lane][8], include/svolsdf_hip.h)."""
    Cin, _, Cout = weight.shape
    dev = weight.device
    s = torch.arange(9, device=dev).view(9, 1, 1)
    lane = torch.arange(64, device=dev).view(1, 64, 1)
    j = torch.arange(8, device=dev).view(1, 1, 8).expand(9, 64, 8)
    kx, q = s // 3, s % 3
    row = (lane >> 4) + 4 * q
    co = (lane & 15).expand(9, 64, 8)
    ok = ((row < 9) & (co < Cout)).expand(9, 64, 8)
    tap = (row.clamp(max=8) * 3 + kx).expand(9, 64, 8)
    w = weight[j, tap, co.clamp(max=Cout - 1)]
    return _hi_mid(w, ok)


# The layouts that were packed on the device before there was one packer, as tests/golden/convfrag_packed.npz records them
# (tests/golden/make_convfrag_fixture.py): key -> (kind, weight shape, argument of the packer).  conv2d: (Cout,Cin,k,k);
# deconv2d: (Cin,Cout,3,3); gemm: [Cin][27][Cout] and the `transposed` flag -- the host passes 0 or 1, and 1 selects by
# (Cin, Cout) one of three forms inside the library: 8 classes (8 -> 6), x-parities paired (8 -> 8), whole cells (16 -> 8).
PACKED_CASES = {
    "conv2d_8_16_3": ("conv2d", (16, 8, 3, 3), None),
    "conv2d_32_32_3": ("conv2d", (32, 32, 3, 3), None),
    "conv2d_16_20_5": ("conv2d", (20, 16, 5, 5), None),
    "deconv2d_16_8": ("deconv2d", (16, 8, 3, 3), None),
    "deconv2d_32_16": ("deconv2d", (32, 16, 3, 3), None),
    "gemm_8_16": ("gemm", (8, 27, 16), False),
    "gemm_64_64": ("gemm", (64, 27, 64), False),
    "gemm_t_8_6": ("gemm", (8, 27, 6), True),
    "gemm_t_8_8": ("gemm", (8, 27, 8), True),
    "gemm_t_16_8": ("gemm", (16, 27, 8), True),
}


def packed_case_weight(key):
    return make_weight(PACKED_CASES[key][1], 1000 + sorted(PACKED_CASES).index(key))
