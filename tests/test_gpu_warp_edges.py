"""The fused warp + variance builders (csrc/svs_costvol.hip) against float64 off the image: every instance of
warp_variance_kernel<C, NS> (float32 volume, and raw_warp = homo_warping alone) and of warp_variance_reuse2_kernel<C, NS, 4> (the
split-volume producer, the default in every MVS backbone), through svs_hip.costvol.warp_variance / homo_warp -- the calls the
models make -- on geometry whose samples cross all four borders, leave and enter the image between the planes of one four-plane
run, project with q.z <= 0, take the division fall-back, and meet hypotheses of 0, < 0, +inf and NaN.

The cases, their inputs and the float64 reference come from tests/warp_cases.py; tests/test_warp_cases_cpu.py shows without a GPU
that the reference is torch's grid_sample, that the table reaches every instance, corner state, depth transition and tail
(counted), and that every mutant of the reference misses the bound used here by a factor of 100.  Bound: per C, 4 x the largest
figure max |comparator - ref| / max |ref| of the oracle's float32 numpy evaluation among the cases of that C, relative to each
case's output scale, on every voxel.  Every test prints comparator figure, bound and HIP figure (pytest -s); the module prints
the worst ratio per kernel instance at its end (recorded in profiles/warp_edges_parity.txt)."""
import ctypes

import numpy as np
import pytest
import torch

import warp_cases as wc

pytestmark = pytest.mark.gpu
SVS_ESHAPE = -2
ROWS = {}                       # kernel instance -> (comparator figure, bound, HIP figure) of its worst case


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nkernel instance                              comparator      bound        HIP    HIP / bound")
    for key in sorted(ROWS, key=str):
        c, b, h = ROWS[key]
        print(f"  {str(key):40s} {c:10.3e} {b:10.3e} {h:10.3e} {h / b:10.3f}")


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


def nan_block(shape, dev):
    """a NaN-filled block of the size of the output to come, handed back to the caching allocator: the wrapper's torch.empty
    of that size starts from NaN"""
    torch.full(shape, float("nan"), device=dev)


def record(key, comparator, bound, hip):
    if key not in ROWS or hip / bound > ROWS[key][2] / ROWS[key][1]:
        ROWS[key] = (comparator, bound, hip)


def device_inputs(k, dev):
    feats, P, dv = wc.features(k), wc.case_projs(k), wc.depths(k)
    return [G(f, dev)[None] for f in feats], G(P, dev)[None], G(np.array(dv), dev)[None]


@pytest.mark.parametrize("name", [k.name for k in wc.CASES])
def test_variance_vs_float64(dev, entries, name):
    """costvol.warp_variance of a case, float32 volume: svs_warp_variance ran, every element written and finite,
    |got - ref| <= bound(C) max|ref| on every voxel."""
    from svs_hip import costvol
    k = wc.BY_NAME[name]
    ref, _, _ = wc.reference(k)
    args = device_inputs(k, dev)
    nan_block((1, k.C, k.D, k.H, k.W), dev)
    del entries[:]
    out = costvol.warp_variance(*args)
    assert entries[-1] == "svs_warp_variance" and "svs_warp_variance_split" not in entries
    assert tuple(out.shape) == (1, k.C, k.D, k.H, k.W)
    got = take(out)[0]
    assert np.isfinite(got).all(), f"{name}: {int((~np.isfinite(got)).sum())} elements not written / not finite"
    fig, bound, comp = wc.figure(got, ref), wc.bound(k.C), wc.comparator_figures(k.C)[name][0]
    record(("float32", k.C, k.NS), comp, bound, fig)
    print(f"{name} warp_variance_kernel<{k.C},{k.NS}>: comparator {comp:.3e}, bound {bound:.3e}, HIP {fig:.3e} = {fig / bound:.3f} of the bound")
    assert fig <= bound


@pytest.mark.parametrize("name", [k.name for k in wc.CASES])
def test_split_producer_vs_float64(dev, entries, name):
    """costvol.warp_variance(..., split=True) of a case, the whole split buffer holding NaN beforehand: svs_warp_variance_split
    ran (split_fits: the producer with corner reuse), every unit of the interior is written and finite, nothing outside the
    interior is written, .float() meets the float64 reference at the bound, and SplitVolume.pack of the float32 kernel's result
    gives the producer's pieces bit for bit."""
    from svs_hip import costvol
    k = wc.BY_NAME[name]
    C, D, H, W = k.C, k.D, k.H, k.W
    ref, _, _ = wc.reference(k)
    args = device_inputs(k, dev)
    assert costvol.split_fits(C, D, H, W)
    buf = costvol.SplitVolume(C, D, H, W, dev).buf              # the cached buffer of this shape: the producer's target
    try:
        buf.fill_(float("nan"))
        del entries[:]
        sv = costvol.warp_variance(*args, split=True)
        assert entries[-1] == "svs_warp_variance_split" and "svs_warp_variance" not in entries
        assert isinstance(sv, costvol.SplitVolume) and sv.buf.data_ptr() == buf.data_ptr()
        Hp, Wp = 4 * ((H + 3) // 4) + 2, 32 * ((W + 31) // 32) + 4
        assert buf.numel() * 2 == wc.split_volume_bytes(C, D, H, W)
        produced = buf.clone()
        v6 = produced.view(D + 2, Hp, 2, C // 8, Wp, 8)
        inner = v6[1:D + 1, 1:H + 1, :, :, 1:W + 1]
        assert bool(torch.isfinite(inner).all()), f"{name}: {int((~torch.isfinite(inner)).sum())} interior halves not written / not finite"
        border = v6.clone()
        border[1:D + 1, 1:H + 1, :, :, 1:W + 1] = float("nan")
        assert bool(torch.isnan(border).all()), f"{name}: {int((~torch.isnan(border)).sum())} halves written outside the interior"
        got = sv.float().cpu().numpy()
        assert got.shape == ref.shape and np.isfinite(got).all()
        fig, bound, comp = wc.figure(got, ref), wc.bound(C), wc.comparator_figures(C)[name][0]
        record(("split", C, k.NS), comp, bound, fig)
        print(f"{name} warp_variance_reuse2_kernel<{C},{k.NS},4>: comparator {comp:.3e}, bound {bound:.3e}, HIP {fig:.3e} = "
              f"{fig / bound:.3f} of the bound")
        # the float32 kernel's values, split by the packer: the same bits
        f32 = costvol.warp_variance(*args)[0]
        assert entries[-1] == "svs_warp_variance"
        buf.zero_()
        sv2 = costvol.SplitVolume.pack(f32)
        assert sv2.buf.data_ptr() == buf.data_ptr()
        packed = buf.view(D + 2, Hp, 2, C // 8, Wp, 8)[1:D + 1, 1:H + 1, :, :, 1:W + 1]
        differ = int((packed.contiguous().view(torch.int16) != inner.contiguous().view(torch.int16)).sum())
        assert differ == 0, f"{name}: {differ} halves of the producer differ from the packed float32 volume"
        with pytest.raises(RuntimeError, match="reused"):
            sv.float()
        assert fig <= bound
    finally:
        buf.zero_()                                             # the border of the cached buffer is zero again


@pytest.mark.parametrize("name", [k.name for k in wc.CASES])
def test_raw_warp_vs_float64(dev, entries, name):
    """costvol.homo_warp of source 0 of a case (warp_variance_kernel in raw_warp mode, one source): every element finite, the
    float64 reference met at the raw bound of the C, got > 0 exactly where the reference has a corner of positive weight inside
    the image (strictly positive features) and got == 0 everywhere else."""
    from svs_hip import costvol
    k = wc.BY_NAME[name]
    _, ref, info = wc.reference(k)
    rot, trans = wc.rot_trans(k)[0]
    rel = [float(v) for v in rot.reshape(-1)] + [float(v) for v in trans]
    nan_block((k.C, k.D, k.H, k.W), dev)
    del entries[:]
    out = costvol.homo_warp(G(wc.features(k)[1], dev), rel, G(np.array(wc.depths(k)), dev))
    assert entries == ["svs_chw_to_hwc", "svs_warp_variance"]
    got = take(out)
    assert got.shape == ref.shape and np.isfinite(got).all()
    want = np.broadcast_to((info[0]["n_pos"] > 0)[None], got.shape)
    assert np.array_equal(got > 0, want), f"{name}: {int(((got > 0) != want).sum())} elements sampled where they must not be, or not sampled"
    assert (got[~want] == 0).all()
    fig, bound, comp = wc.figure(got, ref), wc.bound(k.C, raw=True), wc.comparator_figures(k.C)[name][1]
    record(("raw", k.C), comp, bound, fig)
    print(f"{name} warp_variance_kernel<{k.C},1> raw_warp: comparator {comp:.3e}, bound {bound:.3e}, HIP {fig:.3e} = {fig / bound:.3f} of the bound")
    assert fig <= bound


def test_rejected_sizes(dev):
    """H < 2, W < 2, D < 1, five sources and C = 12 return SVS_ESHAPE from both entries and write nothing."""
    from svs_hip import lib
    from svs_hip.ops import _ptr, _ptr_array, _stream
    L = lib.load()
    C, D, H, W = 8, 2, 3, 5
    sentinel = -777.25
    ref = torch.ones(C, H, W, device=dev)
    hwc = [torch.ones(H, W, C, device=dev) for _ in range(5)]
    dv = torch.full((D, H, W), 10.0, device=dev)
    rt = (ctypes.c_float * 60)(*([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] * 5))
    out = torch.full((16 * D * H * W,), sentinel, device=dev)
    split = torch.full((L.svs_split_volume_dims(16, D, H, W, None) // 2,), sentinel, dtype=torch.float16, device=dev)
    ok = dict(n_src=2, C=C, D=D, H=H, W=W)
    for change in (dict(H=1), dict(W=1), dict(D=0), dict(n_src=5), dict(C=12), dict(n_src=0), dict(H=0), dict(W=-3)):
        a = dict(ok, **change)
        for raw in (0, 1):
            rc = L.svs_warp_variance(_ptr(ref), _ptr_array(hwc), rt, a["n_src"], a["C"], a["D"], a["H"], a["W"], _ptr(dv), _ptr(out), raw,
                                     _stream())
            assert rc == SVS_ESHAPE, (change, raw, rc)
            with pytest.raises(lib.SvsError):
                lib.check(rc, "svs_warp_variance")
        rc = L.svs_warp_variance_split(_ptr(ref), _ptr_array(hwc), rt, a["n_src"], a["C"], a["D"], a["H"], a["W"], _ptr(dv), _ptr(split),
                                       _stream())
        assert rc == SVS_ESHAPE, (change, rc)
        assert L.svs_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()) and bool((split == sentinel).all())
    # and the accepted call writes exactly its volume
    assert L.svs_warp_variance(_ptr(ref), _ptr_array(hwc), rt, 2, C, D, H, W, _ptr(dv), _ptr(out), 0, _stream()) == 0
    n = C * D * H * W
    assert bool((out[:n] != sentinel).all()) and bool((out[n:] == sentinel).all())
