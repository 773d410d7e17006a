"""TEST INFRASTRUCTURE ONLY -- the float64 references, the dispatch restatement and the case table of
tests/test_gpu_conv3d_gemm.py, built here (torch on the host, no GPU import) so that tests/test_conv3d_cases_cpu.py can show
without a GPU that the references are right, that the table reaches every kernel instance the launchers can start, and that
the bound of the GPU test is one a correct float32 evaluation meets on exactly these inputs.

Layers: the 3x3x3 convolutions of the cost-regularisation U-Net in the library's folded layout, weight [Cin][27][Cout]
(models/CasMVSNet.py:_Block3d.folded), through svs_hip.costvol.conv3d -- the call the models make."""
import collections
import functools
import itertools

import numpy as np
import torch

F32 = np.float32
F64 = np.float64

# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def conv_tail(raw, bias, skip, relu):
    """The kernels' epilogue on a raw convolution: bias, then ReLU, then + skip (csrc/svs_conv_gemm.hip:237-241, :331-334;
    tests/test_gpu_costvol.py::test_conv3d_one_output_channel)."""
    y = raw if bias is None else raw + np.asarray(bias, F64).reshape(-1, 1, 1, 1)
    if relu:
        y = np.maximum(y, 0.0)
    return y if skip is None else y + np.asarray(skip, F64)


def ref_conv3d_raw(x, w, stride=1, transposed=False, dtype=torch.float64):
    """x (Cin,D,H,W), w [Cin][27][Cout] -> the convolution alone, (Cout,Do,Ho,Wo), evaluated by torch on the host in `dtype`."""
    Cin, _, Cout = w.shape
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)[None]
    wt = torch.from_numpy(np.ascontiguousarray(w)).to(dtype)
    with torch.no_grad():
        if transposed:
            y = torch.nn.functional.conv_transpose3d(xt, wt.reshape(Cin, 3, 3, 3, Cout).permute(0, 4, 1, 2, 3), stride=2, padding=1,
                                                     output_padding=1)
        else:
            y = torch.nn.functional.conv3d(xt, wt.permute(2, 0, 1).reshape(Cout, Cin, 3, 3, 3), stride=stride, padding=1)
    return y[0].numpy()


def ref_conv3d(x, w, bias=None, skip=None, stride=1, transposed=False, relu=True):
    """float64: [skip +] relu?(conv(x, w) + bias), the layer svs_hip.costvol.conv3d computes."""
    return conv_tail(ref_conv3d_raw(x, w, stride, transposed), bias, skip, relu)


def ref_deconv3d_direct(x, w):
    """ConvTranspose3d(k3, s2, p1, output_padding 1) as the plain sum it is: input voxel i and kernel index k meet in output
    o = 2 i - 1 + k per axis.  numpy float64, one step per (input voxel, tap): tiny sizes only."""
    Cin, D, H, W = x.shape
    Cout = w.shape[2]
    out = np.zeros((Cout, 2 * D, 2 * H, 2 * W), F64)
    x64, w64 = np.asarray(x, F64), np.asarray(w, F64)
    for iz, iy, ix in itertools.product(range(D), range(H), range(W)):
        for kz, ky, kx in itertools.product(range(3), repeat=3):
            oz, oy, ox = 2 * iz - 1 + kz, 2 * iy - 1 + ky, 2 * ix - 1 + kx
            if oz < 0 or oy < 0 or ox < 0:                   # (the upper end always fits: output_padding = 1)
                continue
            out[:, oz, oy, ox] += x64[:, iz, iy, ix] @ w64[:, (kz * 3 + ky) * 3 + kx, :]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------
KSPLIT_TILES = 2048                                  # csrc/svs_conv_gemm.hip:441 kKsplitTiles


def m_tiles(rows):                                   # csrc/svs_conv_gemm.hip:470
    return 1 if rows <= 16 else (2 if rows <= 32 else 4)


def deconv_mode(Cin, Cout):                          # csrc/svs_conv_gemm.hip:472-475
    if (Cin, Cout) in ((16, 8), (32, 16)):
        return 3
    return 2 if (Cout <= 32 and Cout % 4 == 0) else 1


def out_shape(shape, stride, transposed):
    """csrc/svs_conv_gemm.hip:511, :521 (and csrc/svs_costvol.hip:1195, :1200)"""
    return tuple(2 * n for n in shape) if transposed else tuple((n - 1) // stride + 1 for n in shape)


def gemm_tiles(Cin, Cout, shape, stride, transposed):
    """(mode, MT, tiles) of svs_conv3d_gemm: csrc/svs_conv_gemm.hip:509-524"""
    D, H, W = shape
    if transposed:
        mode = deconv_mode(Cin, Cout)
        per_class = D * H * ((W + 15) // 16)         # :512 rows = Di * Hi, xtiles over the INPUT width
        if mode == 3:
            return 3, Cout // 8, per_class           # :515
        if mode == 2:
            return 2, m_tiles(2 * Cout), 4 * per_class   # :518
        return 1, m_tiles(Cout), 8 * per_class       # :519
    Do, Ho, Wo = out_shape(shape, stride, False)
    return 0, m_tiles(Cout), Do * Ho * ((Wo + 15) // 16)   # :521-523


def expected_path(Cin, Cout, shape, stride, transposed, split_input=False, gemm=True):
    """The entry and the template instance svs_hip.costvol.conv3d and the launchers behind it choose.  Restates, in the order
    of the `if`s of svs_hip/costvol.py:656-715:
      :663-678  a SplitVolume input: svs_conv3d_rows / svs_conv3d_pair where fused (stride 1, no skip), else the float32 volume
      :682      stride 1, Cout = 1                               -> ("c1",)
      :687      stride 1, Cin in 8/16/32, Cout <= 16             -> ("mfma",)
      :698      stride 2, Cin = 8, Cout <= 16, W even            -> ("s2c8",)
      :708      gemm_enabled() and svs_conv3d_gemm_supported (csrc/svs_conv_gemm.hip:489) -> the GEMM kernels:
                  ("cell", CIN, MTC)                 deconv_cell_kernel<CIN, MTC>               (:514-517)
                  ("gemm", CIN, MT, MODE, KSPLIT)    conv_gemm_kernel<CIN, MT, MODE, KSPLIT>    (:444-457: KSPLIT = tiles <= 2048)
      :713      svs_conv3d (csrc/svs_costvol.hip:1185-1218): ("valu", "deconv8") transposed; else with
                  wgs16 = ceil(Do Ho ceil(Wo / 4) / 256) ceil(Cout / 16): < 768 -> "conv8x1"; Cout <= 8 -> "conv8x4"; else "conv16x4"
    """
    D, H, W = shape
    if split_input and not transposed and stride == 1:
        if Cin == 16 and Cout > 8:
            if Cout <= 16:                           # rows_supported
                return ("rows",)
        elif Cin in (8, 16, 32) and Cout <= 8:       # pair_supported
            return ("pair",)
    if not transposed and stride == 1 and Cout == 1:
        return ("c1",)
    if not transposed and stride == 1 and Cin in (8, 16, 32) and Cout <= 16:
        return ("mfma",)
    if not transposed and stride == 2 and Cin == 8 and Cout <= 16 and W % 2 == 0:
        return ("s2c8",)
    if gemm and Cin in (8, 16, 32, 64) and 1 <= Cout <= 64:
        mode, MT, tiles = gemm_tiles(Cin, Cout, shape, stride, transposed)
        if mode == 3:
            return ("cell", Cin, MT)
        return ("gemm", Cin, MT, mode, tiles <= KSPLIT_TILES)
    if transposed:
        return ("valu", "deconv8")
    Do, Ho, Wo = out_shape(shape, stride, False)
    total = Do * Ho * ((Wo + 3) // 4)
    wgs16 = ((total + 255) // 256) * ((Cout + 15) // 16)
    if wgs16 < 768:
        return ("valu", "conv8x1")
    return ("valu", "conv8x4" if Cout <= 8 else "conv16x4")


def is_float32_path(path):
    """the float32 FMA kernels (2e-6 of the output scale, the bound of test_conv3d_one_output_channel); the others run fp16x2
    operands on the matrix cores (3e-6, the bound of test_conv3d_pair_vs_float64 / test_conv3d_rows_from_split_volume)"""
    return path[0] in ("valu", "c1")


def tolerance(path):
    return 2e-6 if is_float32_path(path) else 3e-6


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
# variants: (bias, skip, relu)
BOTH = ((1, 1, 1), (0, 0, 0))
ALL8 = tuple(itertools.product((1, 0), repeat=3))

Case = collections.namedtuple("Case", "name Cin Cout shape stride transposed variants gemm")


def _case(Cin, Cout, shape, stride=1, transposed=False, variants=BOTH, gemm=True):
    name = f"{'t' if transposed else 'c'}{Cin}-{Cout}_{'x'.join(str(n) for n in shape)}" + ("" if transposed else f"_s{stride}")
    return Case(name + ("" if gemm else "_valu"), Cin, Cout, tuple(shape), 2 if transposed else stride, bool(transposed), variants,
                bool(gemm))


def _build():
    c = []
    # ---- mode 0, KSPLIT (tiles <= 2048): every CIN x MT; W of 1, 15, 16, 17, 33; D = 1, H = 1; odd and even sides under stride 2
    # (a stride-1 layer from 8/16/32 channels with Cout <= 16 is svs_conv3d_mfma's, a stride-2 one from 8 channels with even W
    # svs_conv3d_s2c8's: MT = 1 from those channel counts is reached with stride 2, from 8 channels with odd W)
    for args in [(8, 5, (5, 7, 33), 2), (8, 16, (4, 6, 31), 2), (8, 24, (3, 5, 17), 1), (8, 24, (6, 4, 30), 2),
                 (8, 33, (2, 3, 15), 1), (8, 64, (7, 8, 2), 2),
                 (16, 5, (1, 9, 35), 2), (16, 16, (8, 1, 32), 2), (16, 24, (1, 4, 16), 1), (16, 33, (5, 5, 5), 2),
                 (16, 64, (2, 2, 33), 1),
                 (32, 16, (3, 4, 66), 2), (32, 5, (2, 2, 1), 2), (32, 24, (4, 1, 15), 1), (32, 64, (1, 1, 1), 1),
                 (32, 33, (9, 3, 29), 2), (32, 24, (32, 32, 17), 1),                      # exactly 2048 tiles
                 (64, 5, (3, 3, 17), 1), (64, 16, (4, 5, 32), 2), (64, 24, (5, 6, 34), 2), (64, 33, (2, 5, 16), 1),
                 (64, 1, (3, 2, 7), 2), (64, 64, (32, 32, 17), 1)]:                       # exactly 2048 tiles
        c.append(_case(*args))
    # ---- mode 0, more than 2048 tiles: narrow ragged rows.  Output (25,41,17): 2050 tiles, half of them one column wide;
    # (3,683,7): 2049; (7,293,9): 2051 -- the last workgroup has 2, 1 and 3 live waves
    for args in [(8, 16, (49, 81, 33), 2), (8, 24, (3, 683, 7), 1), (8, 33, (14, 586, 18), 2),
                 (16, 5, (6, 1365, 13), 2), (16, 24, (7, 293, 9), 1), (16, 64, (25, 41, 17), 1),
                 (32, 16, (13, 585, 17), 2), (32, 24, (25, 41, 17), 1), (32, 33, (3, 683, 7), 1),
                 (64, 5, (7, 293, 9), 1), (64, 24, (50, 81, 34), 2), (64, 64, (25, 41, 17), 1)]:
        c.append(_case(*args))
    # ---- mode 1 (transposed, 8 parity classes: Cout > 32 or not a multiple of 4), KSPLIT: 8 rows xtiles <= 2048.  Class 0 has
    # one tap: KS = 1 for Cin 8 and 16 (waves 1..3 of the workgroup own no k-step), 2 for Cin 64
    for args in [(8, 6, (3, 5, 15)), (8, 18, (2, 3, 17)), (8, 64, (1, 1, 1)),
                 (16, 6, (1, 4, 16)), (16, 30, (4, 1, 1)), (16, 33, (5, 2, 17)),
                 (32, 6, (2, 2, 33)), (32, 18, (3, 3, 3)), (32, 33, (2, 3, 16)),
                 (64, 6, (2, 3, 5)), (64, 30, (1, 2, 15)), (64, 64, (4, 4, 16)), (64, 33, (16, 16, 3))]:   # last: exactly 2048
        c.append(_case(*args, transposed=True))
    # ---- mode 1, more than 2048 tiles: inputs (3,43,17): 2064, (1,257,3): 2056, (7,37,2): 2072
    for args in [(8, 6, (3, 43, 17)), (8, 18, (1, 257, 3)), (8, 33, (7, 37, 2)),
                 (16, 6, (1, 257, 3)), (16, 18, (7, 37, 2)), (16, 64, (3, 43, 17)),
                 (32, 6, (7, 37, 2)), (32, 30, (3, 43, 17)), (32, 64, (1, 257, 3)),
                 (64, 6, (3, 43, 17)), (64, 18, (1, 257, 3)), (64, 64, (7, 37, 2))]:
        c.append(_case(*args, transposed=True))
    # ---- mode 2 (transposed, x-parities paired: Cout <= 32, a multiple of 4), KSPLIT: 4 rows xtiles <= 2048.  MT = m_tiles(2 Cout):
    # Cout 4 -> 8 of 16 rows, 12 -> 24 of 32, 20 -> 40 of 64 (partly filled M tiles, the zero rows of GemmMap mode 2)
    for args in [(8, 4, (3, 5, 15)), (8, 12, (2, 3, 17)), (8, 32, (1, 1, 1)),
                 (16, 4, (5, 2, 17)), (16, 12, (1, 4, 16)), (16, 20, (4, 4, 33)),
                 (32, 8, (2, 3, 16)), (32, 12, (3, 1, 1)), (32, 32, (3, 5, 15)),
                 (64, 4, (1, 2, 15)), (64, 16, (2, 2, 33)), (64, 20, (4, 4, 16)), (64, 32, (16, 16, 17))]:   # last: exactly 2048
        c.append(_case(*args, transposed=True))
    # ---- mode 2, more than 2048 tiles: inputs (19,27,3): 2052, (9,29,17): 2088, (3,171,1): 2052
    for args in [(8, 4, (19, 27, 3)), (8, 12, (3, 171, 1)), (8, 20, (9, 29, 17)),
                 (16, 4, (9, 29, 17)), (16, 16, (19, 27, 3)), (16, 32, (3, 171, 1)),
                 (32, 8, (3, 171, 1)), (32, 12, (19, 27, 3)), (32, 32, (9, 29, 17)),
                 (64, 8, (19, 27, 3)), (64, 12, (9, 29, 17)), (64, 20, (3, 171, 1))]:
        c.append(_case(*args, transposed=True))
    # ---- mode 3 (deconv_cell_kernel): odd sides, Wi below / at / just above a 16-column tile, last workgroups with dead waves
    for cin, cout in ((16, 8), (32, 16)):
        for shape in ((1, 1, 1), (3, 5, 15), (2, 3, 16), (5, 2, 17), (4, 4, 33)):
            c.append(_case(cin, cout, shape, transposed=True, variants=ALL8))
    # ---- the neighbours the same dispatcher owns
    c += [_case(8, 8, (5, 7, 37)), _case(16, 16, (3, 9, 19)), _case(32, 5, (2, 4, 33))]                  # svs_conv3d_mfma + skip
    c += [_case(8, 16, (5, 7, 38), 2), _case(8, 12, (6, 9, 70), 2)]                                      # svs_conv3d_s2c8 + skip
    c += [_case(8, 1, (5, 7, 37)), _case(16, 1, (3, 5, 8))]                                              # svs_conv3d_c1, both kernels
    # the GEMM refuses these channel counts: the float32 fall-back with the GEMM switched on
    c += [_case(4, 8, (5, 7, 37)), _case(4, 6, (3, 4, 5), transposed=True), _case(12, 16, (9, 6, 33), 2)]
    # the fall-back under gemm_enabled(False): transposed; the input-channel chunks (64 = 8 chunks)
    c += [_case(16, 8, (3, 5, 15), transposed=True, gemm=False), _case(8, 12, (2, 3, 17), transposed=True, gemm=False),
          _case(64, 24, (3, 5, 17), 1, gemm=False), _case(64, 16, (4, 5, 31), 2, gemm=False)]
    # both sides of its wgs16 < 768 rule: outputs (59,64,206) = 767 workgroups, (48,64,253) = 768.  (Two input channels: what
    # is looked at here is the choice of kernel and its indexing over ~780 000 output voxels, the smallest size with 768)
    for cout in (8, 16):
        c += [_case(2, cout, (59, 64, 206), 1, gemm=False), _case(2, cout, (48, 64, 253), 1, gemm=False),
              _case(2, cout, (117, 128, 411), 2, gemm=False), _case(2, cout, (96, 127, 505), 2, gemm=False)]
    names = [k.name for k in c]
    assert len(set(names)) == len(names), "case names must be unique"
    return tuple(c)


CASES = _build()
BY_NAME = {k.name: k for k in CASES}


def case_path(k):
    return expected_path(k.Cin, k.Cout, k.shape, k.stride, k.transposed, gemm=k.gemm)


def _seed(k):
    return (1000003 * k.Cin + 7919 * k.Cout + 101 * k.shape[0] + 11 * k.shape[1] + k.shape[2] + (500 if k.transposed else k.stride)
            + (250 if not k.gemm else 0))


def case_inputs(k):
    """-> x (Cin,D,H,W) ~ N(0,1), w [Cin][27][Cout] ~ N(0,1) / sqrt(27 Cin), bias [Cout], skip (Cout,Do,Ho,Wo), float32, seeded per
    case.  One z-plane of the first channel is +0.0 and one y-plane of the last channel -0.0, so that the border and ReLU paths
    meet zeros of both signs."""
    rng = np.random.default_rng(_seed(k))
    D, H, W = k.shape
    x = rng.standard_normal((k.Cin, D, H, W)).astype(F32)
    x[0, D // 2] = 0.0
    x[-1, :, H // 2] = -0.0
    w = (rng.standard_normal((k.Cin, 27, k.Cout)) / np.sqrt(27 * k.Cin)).astype(F32)
    bias = rng.standard_normal(k.Cout).astype(F32)
    skip = rng.standard_normal((k.Cout,) + out_shape(k.shape, k.stride, k.transposed)).astype(F32)
    return x, w, bias, skip


@functools.lru_cache(maxsize=None)
def _raw_small(name):
    k = BY_NAME[name]
    x, w, _, _ = case_inputs(k)
    return ref_conv3d_raw(x, w, k.stride, k.transposed)


def case_raw_reference(k):
    """The float64 convolution of a case, computed once per process for the cases several tests share (the large fall-back
    volumes, ~100 MB each, are used by one test each and not kept)."""
    if k.Cout * int(np.prod(out_shape(k.shape, k.stride, k.transposed))) > (1 << 21):
        x, w, _, _ = case_inputs(k)
        return ref_conv3d_raw(x, w, k.stride, k.transposed)
    return _raw_small(k.name)


def variant_args(k, variant, bias, skip):
    b, s, r = variant
    return (bias if b else None), (skip if s else None), bool(r)
