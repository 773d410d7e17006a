"""The 3x3x3 convolutions of the cost-regularisation U-Net, layer by layer, against float64: every instance of
conv_gemm_kernel<CIN, MT, MODE, KSPLIT> and deconv_cell_kernel (csrc/svs_conv_gemm.hip), and the neighbours the same dispatcher
owns (svs_conv3d_mfma and svs_conv3d_s2c8 with a skip operand, svs_conv3d_c1, the float32 fall-back svs_conv3d), through
svs_hip.costvol.conv3d -- the call the models make.

The cases, their inputs and the float64 references come from tests/conv3d_cases.py; tests/test_conv3d_cases_cpu.py shows without
a GPU that the references are right, that the table reaches every kernel instance, and that plain float32 torch meets the
bounds used here on the same inputs.  Bounds: 3e-6 of the output scale for the fp16x2 matrix-core kernels (the bound of
test_conv3d_pair_vs_float64 and test_conv3d_rows_from_split_volume: same format, same accumulation), 2e-6 for the float32
kernels (test_conv3d_one_output_channel).  Every test prints the figures it asserts on (pytest -s); the module prints the
worst ratio per kernel instance at its end (recorded in profiles/conv3d_gemm_parity.txt)."""
import numpy as np
import pytest
import torch

import casmvs_oracle as corc
import conv3d_cases as cc
import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
SVS_EINVAL, SVS_ESHAPE = -1, -2
ENTRY = {"gemm": "svs_conv3d_gemm", "cell": "svs_conv3d_gemm", "valu": "svs_conv3d", "mfma": "svs_conv3d_mfma",
         "s2c8": "svs_conv3d_s2c8", "c1": "svs_conv3d_c1"}
WORST = {}                      # kernel instance -> worst |got - ref| / (tol max|ref|) over the module


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst |got - ref| / (tol * max|ref|) per kernel instance (tol: 3e-6 fp16x2, 2e-6 float32)")
    for path in sorted(WORST, key=str):
        print(f"  {str(path):40s} {WORST[path]:.3f}")


@pytest.fixture()
def entries(monkeypatch):
    """the names the wrappers hand to lib.check, in call order: which entry of the library ran"""
    from svs_hip import lib
    seen, real = [], lib.check

    def check(rc, what=""):
        seen.append(what)
        return real(rc, what)
    monkeypatch.setattr(lib, "check", check)
    return seen


def G(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def take(t):
    """Host copy of a kernel's output; the device buffer is then filled with NaN, so that a later launch which is handed the same
    memory by the allocator cannot pass on what an earlier one left there (the finiteness assertions see every unwritten element)."""
    out = t.cpu().numpy()
    t.fill_(float("nan"))
    return out


def conv(k, x, w, bias, skip, relu, gemm=None):
    """costvol.conv3d of a case with the GEMM switch of the case (or `gemm`), restored afterwards"""
    from svs_hip import costvol
    before = costvol.gemm_enabled()
    try:
        costvol.gemm_enabled(k.gemm if gemm is None else gemm)
        return costvol.conv3d(x, w, bias, skip=skip, stride=k.stride, transposed=k.transposed, relu=relu)
    finally:
        costvol.gemm_enabled(before)
        assert costvol.gemm_enabled() == before


def ratio_of(got, ref, tol):
    return float(np.abs(got.astype(F64) - ref).max() / (tol * np.abs(ref).max()))


@pytest.mark.parametrize("name", [k.name for k in cc.CASES])
def test_conv3d_vs_float64(dev, entries, name):
    """Every case of conv3d_cases.CASES and each of its (bias, skip, ReLU) variants: the output's shape, every element finite
    (the output buffer holds NaN where the allocator hands back an earlier one), |got - ref| <= tol max|ref| elementwise, and the
    entry of the library that ran is the one conv3d_cases.expected_path names.  Transposed cases run their skip variant twice:
    with the skip tensor allocated on its own and as a non-contiguous slice of a wider volume, bit for bit the same."""
    from svs_hip import costvol, lib
    k = cc.BY_NAME[name]
    path = cc.case_path(k)
    tol = cc.tolerance(path)
    assert bool(lib.load().svs_conv3d_gemm_supported(k.Cin, k.Cout)) == (k.Cin in (8, 16, 32, 64) and 1 <= k.Cout <= 64)
    assert costvol.gemm_enabled() is True
    x, w, bias, skip = cc.case_inputs(k)
    raw = cc.case_raw_reference(k)
    dx, dw, db, ds = G(x, dev), G(w, dev), G(bias, dev), G(skip, dev)
    wide = torch.zeros(skip.shape[:3] + (skip.shape[3] + 3,), device=dev)
    wide[..., 1:-2] = ds
    for variant in k.variants:
        b, s, relu = cc.variant_args(k, variant, db, ds)
        ref = cc.conv_tail(raw, bias if variant[0] else None, skip if variant[1] else None, relu)
        del entries[:]
        out = conv(k, dx, dw, b, s, relu)
        assert entries and entries[-1] == ENTRY[path[0]], f"{name}: {entries} ran, {path} expected"
        assert tuple(out.shape) == ref.shape
        twin = None
        if k.transposed and s is not None:
            view = wide[..., 1:-2]
            assert not view.is_contiguous()
            twin = conv(k, dx, dw, b, view, relu)
        got = take(out)
        assert np.isfinite(got).all(), f"{name} {variant}: {int((~np.isfinite(got)).sum())} elements not written / not finite"
        r = ratio_of(got, ref, tol)
        WORST[path] = max(WORST.get(path, 0.0), r)
        print(f"{name} {variant} {path}: {r:.3f} of the bound")
        assert r <= 1.0, f"{name} {variant} {path}: at {r:.3f} of {tol:g} max|ref|"
        if twin is not None:
            assert np.array_equal(take(twin), got), f"{name} {variant}: a sliced skip tensor gives another result"


GUARDED = [k.name for k in cc.CASES if k.transposed and k.gemm and cc.case_path(k)[0] in ("gemm", "cell")
           and (cc.case_path(k)[0] == "cell" or cc.case_path(k)[3] == 2) and k.shape[2] in (1, 15, 17)]


@pytest.mark.parametrize("name", GUARDED)
def test_transposed_writes_its_volume_and_nothing_else(dev, name):
    """Modes 2 and 3 store both x-parities of a voxel at once (the cell kernel as one float2): with Wi of 1, 15 and 17 the C
    entry, called with `out` inside a larger sentinel-filled buffer, writes all 2 Wi columns of every row -- no element of the
    volume keeps the sentinel, all of them match the reference -- and leaves the 64 floats before and after it untouched."""
    from svs_hip import costvol, lib
    from svs_hip.ops import _ptr, _stream
    k = cc.BY_NAME[name]
    assert k.shape[2] in (1, 15, 17)
    path = cc.case_path(k)
    x, w, bias, skip = cc.case_inputs(k)
    ref = cc.conv_tail(cc.case_raw_reference(k), bias, skip, True)
    dx, dw, db, ds = G(x, dev), G(w, dev), G(bias, dev), G(skip, dev)
    frag = costvol.gemm_weight_fragments(dw, True)
    guard, n, sentinel = 64, ref.size, -777.25
    buf = torch.full((n + 2 * guard,), sentinel, device=dev)
    D, H, W = k.shape
    lib.check(lib.load().svs_conv3d_gemm(_ptr(dx), _ptr(frag), _ptr(db), _ptr(ds), buf.data_ptr() + 4 * guard, k.Cin, k.Cout, D, H, W,
                                         2, 1, 1, _stream()), "svs_conv3d_gemm")
    got = buf.cpu().numpy()
    assert (got[:guard] == sentinel).all() and (got[guard + n:] == sentinel).all(), f"{name}: written outside the volume"
    vol = got[guard:guard + n].reshape(ref.shape)
    assert (vol != sentinel).all(), f"{name}: {int((vol == sentinel).sum())} elements of the volume not written"
    assert vol.shape[3] == 2 * W
    r = ratio_of(vol, ref, cc.tolerance(path))
    print(f"{name} {path}: {r:.3f} of the bound inside the guard band")
    assert r <= 1.0


LINEAR = {"c64-24_5x6x34_s2": 0, "t16-33_5x2x17": 1, "t16-20_4x4x33": 2, "t32-16_5x2x17": 3}


@pytest.mark.parametrize("name", list(LINEAR))
def test_linear_in_the_input(dev, name):
    """One case per mode, ReLU off: f(2 x) - 2 (f(x) - b) - b = 0 to the case's bound -- the property
    test_conv0_full_size_pair_vs_channel_rows uses.  (Doubling is exact in both fp16 pieces, so what is left is the rounding of
    the bias additions.)"""
    k = cc.BY_NAME[name]
    path = cc.case_path(k)
    assert (3 if path[0] == "cell" else path[3]) == LINEAR[name]
    x, w, bias, _ = cc.case_inputs(k)
    scale = np.abs(cc.conv_tail(cc.case_raw_reference(k), bias, None, False)).max()
    dw, db = G(w, dev), G(bias, dev)
    f1 = take(conv(k, G(x, dev), dw, db, None, False)).astype(F64)
    f2 = take(conv(k, G(2.0 * x, dev), dw, db, None, False)).astype(F64)
    assert np.isfinite(f1).all() and np.isfinite(f2).all()
    b = bias.astype(F64).reshape(-1, 1, 1, 1)
    r = float(np.abs(f2 - 2.0 * (f1 - b) - b).max() / (cc.tolerance(path) * scale))
    print(f"{name} {path}: linearity at {r:.3f} of the bound")
    assert r <= 1.0


@pytest.mark.parametrize("name", [k.name for k in cc.CASES if k.gemm and cc.case_path(k)[0] in ("gemm", "cell")])
def test_gemm_against_fallback(dev, entries, name):
    """Every case both paths accept: the matrix-core kernels and the float32 direct convolution (gemm_enabled(False)) are two
    independent evaluations of the layer and agree to the GEMM's bound, with bias, ReLU and skip."""
    k = cc.BY_NAME[name]
    x, w, bias, skip = cc.case_inputs(k)
    scale = np.abs(cc.conv_tail(cc.case_raw_reference(k), bias, skip, True)).max()
    dx, dw, db, ds = G(x, dev), G(w, dev), G(bias, dev), G(skip, dev)
    a = take(conv(k, dx, dw, db, ds, True))
    assert entries[-1] == "svs_conv3d_gemm"
    b = take(conv(k, dx, dw, db, ds, True, gemm=False))
    assert entries[-1] == "svs_conv3d"
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
    r = float(np.abs(a.astype(F64) - b).max() / (3e-6 * scale))
    print(f"{name} {cc.case_path(k)}: GEMM against the fall-back at {r:.3f} of the bound")
    assert r <= 1.0


@pytest.mark.parametrize("cin,shape", [(32, (16, 16, 24)), (16, (8, 24, 16)), (8, (8, 8, 8)), (16, (8, 24, 40)), (8, (24, 8, 40))])
def test_costreg_vs_float64(dev, cin, shape):
    """The whole U-Net against the oracle's float64 network: the three volumes of test_costreg_vs_torch_reference and two whose
    coarse levels have odd sides, (8,24,40) -> (1,3,5) and (24,8,40) -> (3,1,5) (the network needs multiples of 8).  Maximum and
    mean error of the HIP network are at most 8 times those of float32 torch on the same input: fp16x2 operands carry 22 bits
    against float32's 24 (a factor of 4) and both operands of a product are rounded (a factor of 2).
    Measured on an MI355X over the five volumes and both input forms (float32 volume, split volume): maximum error 0.95 to 1.26
    times float32 torch's, mean error 1.12 to 1.50 times (profiles/conv3d_gemm_parity.txt, section 3)."""
    from models.CasMVSNet import CostRegNet
    from svs_hip import costvol
    params = synth.make_costreg_params(7 + cin, cin)
    net = CostRegNet(cin, 8)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    net.to(dev).eval()
    x = np.random.default_rng(cin + shape[2]).normal(0, 1, (cin,) + shape).astype(F32)
    ref = corc.cost_reg_net_torch(params, x, dtype=torch.float64)
    assert ref.dtype == F64 and ref.shape == shape
    e32 = np.abs(corc.cost_reg_net_torch(params, x).astype(F64) - ref)
    for tag, inp in (("float32 volume", lambda: G(x, dev)[None]), ("split volume", lambda: costvol.SplitVolume.pack(G(x, dev)))):
        y = take(net(inp())[0, 0])
        assert y.shape == ref.shape and np.isfinite(y).all()
        e = np.abs(y.astype(F64) - ref)
        print(f"U-Net {cin} x {shape}, {tag}: max error {e.max():.3e} = {e.max() / e32.max():.2f} x float32 torch's {e32.max():.3e}, "
              f"mean {e.mean():.3e} = {e.mean() / e32.mean():.2f} x {e32.mean():.3e}")
        assert e.max() <= 8.0 * e32.max() and e.mean() <= 8.0 * e32.mean()


def test_conv3d_gemm_arguments(dev):
    """svs_conv3d_gemm and svs_conv3d_gemm_pack reject null pointers, stride 3, Cin = 12, Cout = 65 and a zero extent with their
    codes, and a rejected call leaves a sentinel-filled output as it was."""
    from svs_hip import costvol, lib
    from svs_hip.ops import _ptr, _stream
    L = lib.load()
    assert not L.svs_conv3d_gemm_supported(12, 8) and not L.svs_conv3d_gemm_supported(8, 65) and not L.svs_conv3d_gemm_supported(8, 0)
    assert L.svs_conv3d_gemm_wfrag_bytes(12, 8, 0) == 0 and L.svs_conv3d_gemm_wfrag_bytes(8, 65, 1) == 0
    x = torch.randn(8, 2, 3, 4, device=dev)
    w = torch.randn(8, 27, 8, device=dev)
    sentinel = -777.25
    nbytes = L.svs_conv3d_gemm_wfrag_bytes(8, 8, 0)
    assert nbytes > 0
    frag = torch.full((nbytes // 4,), sentinel, device=dev)
    for args, code in [((None, 8, 8, 0, _ptr(frag)), SVS_EINVAL), ((_ptr(w), 8, 8, 0, None), SVS_EINVAL),
                       ((_ptr(w), 12, 8, 0, _ptr(frag)), SVS_EINVAL), ((_ptr(w), 8, 65, 0, _ptr(frag)), SVS_EINVAL),
                       ((_ptr(w), 8, 0, 1, _ptr(frag)), SVS_EINVAL)]:
        assert L.svs_conv3d_gemm_pack(*args, _stream()) == code, args
        assert L.svs_last_error_string()
    torch.cuda.synchronize()
    assert bool((frag == sentinel).all())
    good = costvol.gemm_weight_fragments(w, False)
    out = torch.full((8 * 4 * 6 * 8,), sentinel, device=dev)      # room for the transposed output, the larger of the two
    ok = dict(inp=_ptr(x), frag=_ptr(good), out=_ptr(out), Cin=8, Cout=8, D=2, H=3, W=4, stride=1)
    for change, code in [(dict(inp=None), SVS_EINVAL), (dict(frag=None), SVS_EINVAL), (dict(out=None), SVS_EINVAL),
                         (dict(stride=3), SVS_EINVAL), (dict(stride=0), SVS_EINVAL), (dict(D=0), SVS_EINVAL), (dict(H=0), SVS_EINVAL),
                         (dict(W=0), SVS_EINVAL), (dict(W=-4), SVS_EINVAL), (dict(Cin=12), SVS_ESHAPE), (dict(Cout=65), SVS_ESHAPE),
                         (dict(Cout=0), SVS_ESHAPE)]:
        a = dict(ok, **change)
        for transposed in (0, 1):
            rc = L.svs_conv3d_gemm(a["inp"], a["frag"], None, None, a["out"], a["Cin"], a["Cout"], a["D"], a["H"], a["W"], a["stride"],
                                   transposed, 1, _stream())
            assert rc == code, (change, transposed, rc)
            with pytest.raises(lib.SvsError):
                lib.check(rc, "svs_conv3d_gemm")
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())
    # and the accepted call writes exactly its volume
    assert L.svs_conv3d_gemm(ok["inp"], ok["frag"], None, None, ok["out"], 8, 8, 2, 3, 4, 1, 0, 1, _stream()) == 0
    n = 8 * 2 * 3 * 4
    assert bool((out[:n] != sentinel).all()) and bool((out[n:] == sentinel).all())
