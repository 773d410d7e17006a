"""Without a GPU: the references of tests/conv3d_cases.py are right, its case table reaches every kernel instance the 3-D
convolution launchers can start, and the bounds of tests/test_gpu_conv3d_gemm.py are ones that a correct float32 evaluation of
exactly these inputs meets."""
import itertools

import numpy as np
import pytest
import torch

import casmvs_oracle as corc
import conv3d_cases as cc

F32 = np.float32
F64 = np.float64


@pytest.mark.parametrize("cin,cout,shape", [(3, 2, (1, 1, 1)), (4, 5, (3, 1, 5)), (2, 3, (1, 3, 3))])
def test_transposed_references_agree(cin, cout, shape):
    """ref_conv3d(transposed=True) (torch's conv_transpose3d on the re-laid weights) == ref_deconv3d_direct (the plain sum over
    o = 2 i - 1 + k) == the oracle's Deconv3d block with an identity BatchNorm, to 1e-12."""
    rng = np.random.default_rng(cin + shape[2])
    x = rng.standard_normal((cin,) + shape)
    w = rng.standard_normal((cin, 27, cout)) / np.sqrt(27 * cin)
    direct = cc.ref_deconv3d_direct(x, w)
    got = cc.ref_conv3d(x, w, transposed=True, relu=False)
    assert got.shape == direct.shape == (cout,) + tuple(2 * n for n in shape)
    assert np.abs(got - direct).max() <= 1e-12
    # every tap matters: the reference is not, say, all zeros off the even outputs
    assert (np.abs(direct) > 1e-3).mean() > 0.9
    params = {"up.conv.weight": w.reshape(cin, 3, 3, 3, cout).transpose(0, 4, 1, 2, 3).copy(),
              "up.bn.weight": np.full(cout, np.sqrt(1.0 + 1e-5)), "up.bn.bias": np.zeros(cout),
              "up.bn.running_mean": np.zeros(cout), "up.bn.running_var": np.ones(cout)}
    _, _, deconv = corc.costreg_blocks_torch(params, torch.float64)
    block = deconv(torch.from_numpy(x)[None], "up")[0].numpy()
    assert np.abs(block - np.maximum(direct, 0.0)).max() <= 1e-12
    assert np.abs(cc.ref_conv3d(x, w, transposed=True, relu=True) - block).max() <= 1e-12


def test_convolution_reference_is_the_oracles_block():
    """ref_conv3d (stride 1 and 2, odd sides) == the oracle's Conv3d block with an identity BatchNorm, and a direct sum at one
    output voxel per corner: the tap order (kz*3 + ky)*3 + kx of the folded layout."""
    rng = np.random.default_rng(5)
    cin, cout, shape = 3, 4, (3, 4, 5)
    x = rng.standard_normal((cin,) + shape)
    w = rng.standard_normal((cin, 27, cout))
    params = {"c.conv.weight": w.transpose(2, 0, 1).reshape(cout, cin, 3, 3, 3).copy(),
              "c.bn.weight": np.full(cout, np.sqrt(1.0 + 1e-5)), "c.bn.bias": np.zeros(cout),
              "c.bn.running_mean": np.zeros(cout), "c.bn.running_var": np.ones(cout)}
    _, conv, _ = corc.costreg_blocks_torch(params, torch.float64)
    for stride in (1, 2):
        ref = cc.ref_conv3d(x, w, stride=stride, relu=True)
        assert ref.shape == (cout,) + cc.out_shape(shape, stride, False)
        assert np.abs(conv(torch.from_numpy(x)[None], "c", stride)[0].numpy() - ref).max() <= 1e-12
        raw = cc.ref_conv3d(x, w, stride=stride, relu=False)
        xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (1, 1)))
        for zo, yo, xo in itertools.product(*[(0, n - 1) for n in raw.shape[1:]]):
            win = xp[:, zo * stride:zo * stride + 3, yo * stride:yo * stride + 3, xo * stride:xo * stride + 3].reshape(cin, 27)
            assert np.abs(np.einsum("ct,cto->o", win, w) - raw[:, zo, yo, xo]).max() <= 1e-12


def test_tail_order_is_bias_relu_skip():
    raw = np.array([-2.0, 0.5]).reshape(2, 1, 1, 1)
    got = cc.conv_tail(raw, np.array([1.0, -1.0]), np.array([10.0, 20.0]).reshape(2, 1, 1, 1), True)
    assert got.reshape(-1).tolist() == [10.0, 20.0]
    assert cc.conv_tail(raw, None, None, False) is raw


def test_inputs_carry_signed_zeros_and_are_seeded():
    for k in cc.CASES:
        if int(np.prod(k.shape)) > 4096:
            continue
        x, w, b, s = cc.case_inputs(k)
        zeros = x == 0
        assert zeros.any() and np.signbit(x[zeros]).any() and not np.signbit(x[zeros]).all(), k.name
        assert (~zeros).any(), k.name
        x2 = cc.case_inputs(k)[0]
        assert np.array_equal(x, x2)
        assert s.shape == (k.Cout,) + cc.out_shape(k.shape, k.stride, k.transposed) and w.shape == (k.Cin, 27, k.Cout)


# every kernel instance the launchers of csrc/svs_conv_gemm.hip (launch_mt, launch_cin, svs_conv3d_gemm), csrc/svs_costvol.hip
# (svs_conv3d, svs_conv3d_c1), svs_conv3d_mfma and svs_conv3d_s2c8 can start from svs_hip.costvol.conv3d on a float32 volume,
# written out
INSTANCES = (
    [("gemm", cin, mt, mode, ksplit) for mode in (0, 1, 2) for cin in (8, 16, 32, 64) for mt in (1, 2, 4) for ksplit in (True, False)]
    + [("cell", 16, 1), ("cell", 32, 2), ("s2c8",), ("mfma",), ("c1",),
       ("valu", "deconv8"), ("valu", "conv8x1"), ("valu", "conv8x4"), ("valu", "conv16x4")])
# instances of that list that no argument of costvol.conv3d reaches, with the reason.  None today: launch_mt knows the M tile
# counts 1, 2 and 4 only (m_tiles never gives 3); every CIN reaches MT = 1 in mode 0 through stride 2 (stride 1 with Cout <= 16
# from 8 / 16 / 32 channels is svs_conv3d_mfma's; from 8 channels the width must also be odd, or svs_conv3d_s2c8 takes it); in
# mode 2 MT = m_tiles(2 Cout) is 1 for Cout 4 and 8, 2 for 12 and 16, 4 from 20 on, and the two pairs deconv_mode gives to the
# cell kernel, (16, 8) and (32, 16), leave Cout = 4 and Cout = 12 for those M tile counts; mode 1 has Cout 1..3, 5..7, ... for
# MT = 1, 17..31 outside the multiples of 4 for MT = 2 and 33..64 for MT = 4 from every CIN
UNREACHABLE = {}


def test_table_reaches_every_kernel_instance():
    assert len(set(INSTANCES)) == len(INSTANCES) == 72 + 9
    reached = {}
    for k in cc.CASES:
        reached.setdefault(cc.case_path(k), []).append(k.name)
    missing = [i for i in INSTANCES if i not in reached and i not in UNREACHABLE]
    assert not missing, f"no case runs {missing}"
    assert not [i for i in UNREACHABLE if i in reached], "an instance listed as unreachable is reached"
    assert not [p for p in reached if p not in INSTANCES], "a case takes a path the instance list does not know"
    assert len(UNREACHABLE) == 0                       # the cap on instances left out


def test_table_holds_the_edges_it_claims():
    """The dispatch edges by their numbers: tile counts on both sides of 2048 and the three counts that leave 1, 2 and 3 live
    waves in the last workgroup; widths; D = 1 and H = 1; both parities of every side under stride 2; the fall-back's 767 / 768
    workgroups; the cell kernel's shapes and variants."""
    tiles = {}
    for k in cc.CASES:
        p = cc.case_path(k)
        if p[0] == "gemm":
            tiles.setdefault((p[3], p[1]), set()).add(cc.gemm_tiles(k.Cin, k.Cout, k.shape, k.stride, k.transposed)[2])
    for cin in (32, 64):
        assert 2048 in tiles[(0, cin)] and max(tiles[(0, cin)]) > 2048
    assert {2049, 2050, 2051} <= set().union(*[tiles[(0, c)] for c in (8, 16, 32, 64)])
    for mode in (1, 2):
        every = set().union(*[tiles[(mode, c)] for c in (8, 16, 32, 64)])
        assert 2048 in every and max(every) > 2048 and min(every) < 64
    m0 = [k for k in cc.CASES if cc.case_path(k)[0] == "gemm" and not k.transposed]
    assert {1, 15, 16, 17, 33} <= {cc.out_shape(k.shape, k.stride, False)[2] for k in m0}
    assert any(k.shape[0] == 1 for k in m0) and any(k.shape[1] == 1 for k in m0)
    for axis in range(3):
        assert {0, 1} == {k.shape[axis] % 2 for k in m0 if k.stride == 2}
    assert {5, 16, 24, 33, 64} <= {k.Cout for k in m0} and {1, 2} == {k.stride for k in m0}
    m1 = [k for k in cc.CASES if cc.case_path(k)[0] == "gemm" and cc.case_path(k)[3] == 1]
    m2 = [k for k in cc.CASES if cc.case_path(k)[0] == "gemm" and cc.case_path(k)[3] == 2]
    assert {6, 33, 64} <= {k.Cout for k in m1} and {8, 16, 64} <= {k.Cin for k in m1}
    assert any(k.Cin == 8 and cc.case_path(k)[4] for k in m1)                    # class 0: KS = 1 under KSPLIT
    assert {4, 12, 20, 32} <= {k.Cout for k in m2} and {8, 32, 64} <= {k.Cin for k in m2}
    assert {1, 15, 17} <= {k.shape[2] for k in m2}
    cell = [k for k in cc.CASES if cc.case_path(k)[0] == "cell"]
    for pair in ((16, 8), (32, 16)):
        assert {k.shape for k in cell if (k.Cin, k.Cout) == pair} == {(1, 1, 1), (3, 5, 15), (2, 3, 16), (5, 2, 17), (4, 4, 33)}
    assert all(set(k.variants) == set(itertools.product((0, 1), repeat=3)) for k in cell)
    wgs = set()
    for k in cc.CASES:
        if cc.case_path(k)[0] == "valu" and not k.transposed:
            Do, Ho, Wo = cc.out_shape(k.shape, k.stride, False)
            wgs.add((k.stride, k.Cout, (Do * Ho * ((Wo + 3) // 4) + 255) // 256 * ((k.Cout + 15) // 16)))
    assert {(s, c, n) for s in (1, 2) for c in (8, 16) for n in (767, 768)} <= wgs
    assert any(k.Cin == 4 and k.gemm and cc.case_path(k)[0] == "valu" for k in cc.CASES)
    assert all(any(v[1] for v in k.variants) for k in cc.CASES)                  # every case runs with a skip once
    # ~20 000 output voxels x 64 channels, except the fall-back's 768-workgroup volumes (two input channels)
    for k in cc.CASES:
        n = k.Cout * int(np.prod(cc.out_shape(k.shape, k.stride, k.transposed)))
        assert n <= 20000 * 64 or (k.Cin == 2 and cc.case_path(k)[0] == "valu"), k.name


def test_expected_path_for_the_u_net_layers():
    """The rules against what is known of the network (base 8, stage 1 of config 3: 32 x 192 x 128 x 160): conv0 / conv2 on the
    split-volume kernels, conv1 on s2c8, conv3..conv7 on the GEMM (conv6 with 4608 tiles: not KSPLIT), conv9 / conv11 on the
    cell kernel, prob on c1."""
    assert cc.expected_path(32, 8, (192, 128, 160), 1, False, split_input=True) == ("pair",)
    assert cc.expected_path(8, 16, (192, 128, 160), 2, False) == ("s2c8",)
    assert cc.expected_path(16, 16, (96, 64, 80), 1, False, split_input=True) == ("rows",)
    assert cc.expected_path(16, 16, (96, 64, 80), 1, False) == ("mfma",)
    assert cc.expected_path(16, 32, (96, 64, 80), 2, False) == ("gemm", 16, 2, 0, False)
    assert cc.expected_path(32, 32, (48, 32, 40), 1, False) == ("gemm", 32, 2, 0, False)
    assert cc.expected_path(32, 64, (48, 32, 40), 2, False) == ("gemm", 32, 4, 0, True)
    assert cc.gemm_tiles(64, 64, (24, 16, 20), 1, False)[2] == 768
    assert cc.gemm_tiles(64, 64, (48, 48, 32), 1, False)[2] == 4608
    assert cc.expected_path(64, 64, (48, 48, 32), 1, False) == ("gemm", 64, 4, 0, False)
    assert cc.gemm_tiles(64, 32, (24, 16, 20), 2, True) == (2, 4, 4 * 24 * 16 * 2)               # conv7: 3072 tiles
    assert cc.expected_path(64, 32, (24, 16, 20), 2, True) == ("gemm", 64, 4, 2, False)
    assert cc.expected_path(64, 32, (12, 8, 10), 2, True) == ("gemm", 64, 4, 2, True)
    assert cc.expected_path(32, 16, (48, 32, 40), 2, True) == ("cell", 32, 2)
    assert cc.expected_path(16, 8, (96, 64, 80), 2, True) == ("cell", 16, 1)
    assert cc.expected_path(8, 1, (192, 128, 160), 1, False) == ("c1",)
    assert cc.expected_path(64, 32, (24, 16, 20), 2, True, gemm=False) == ("valu", "deconv8")


@pytest.mark.parametrize("name", [k.name for k in cc.CASES])
def test_float32_torch_meets_the_bound(name):
    """For every case and variant, a plain float32 torch evaluation on the host stays within the bound the GPU test sets for the
    case's path (conv3d_cases.tolerance) of the float64 reference: the bound is not set where a correct evaluation fails."""
    k = cc.BY_NAME[name]
    x, w, bias, skip = cc.case_inputs(k)
    raw64 = cc.case_raw_reference(k)
    raw32 = cc.ref_conv3d_raw(x, w, k.stride, k.transposed, dtype=torch.float32)
    assert raw32.dtype == F32 and raw64.dtype == F64 and raw32.shape == raw64.shape
    tol = cc.tolerance(cc.case_path(k))
    for variant in k.variants:
        b, s, relu = cc.variant_args(k, variant, bias, skip)
        ref = cc.conv_tail(raw64, b, s, relu)
        y = raw32 if b is None else raw32 + b.reshape(-1, 1, 1, 1)
        y = np.maximum(y, F32(0)) if relu else y
        y = y if s is None else y + s
        assert y.dtype == F32
        ratio = np.abs(y - ref).max() / (tol * np.abs(ref).max())
        assert ratio <= 1.0, f"{name} {variant}: float32 torch at {ratio:.3f} of the bound"
