"""GPU parity: the HIP path (through the C-ABI) against the oracle on seeded inputs and the golden fixtures.
Floating point: <= 1e-4 abs (north_star); sampler indices and every sampler float: bit-exact."""
import os

import numpy as np
import pytest
import torch

import svs_oracle as orc
import synth

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from svs_hip import ops as _ops
    return _ops


def _pack(dev, ops, params):
    pk = ops.PackedMlp(dev)
    t = lambda k: torch.from_numpy(params[k]).to(dev)
    pk.pack_sdf([t(f"implicit_network.lin{l}.weight_v") for l in range(9)],
                [t(f"implicit_network.lin{l}.weight_g") for l in range(9)],
                [t(f"implicit_network.lin{l}.bias") for l in range(9)])
    pk.pack_rgb([t(f"rendering_network.lin{l}.weight_v") for l in range(5)],
                [t(f"rendering_network.lin{l}.weight_g") for l in range(5)],
                [t(f"rendering_network.lin{l}.bias") for l in range(5)])
    return pk, params


@pytest.fixture(scope="module")
def packed(dev, ops):
    return _pack(dev, ops, synth.make_params(0))


@pytest.fixture(scope="module")
def packed_w1(dev, ops):
    """the trained-scale weight set (synth.make_trained_params): gains up to ~3x, activations ~15, d sdf/dx ~20"""
    return _pack(dev, ops, synth.make_trained_params(1))


def G(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------------
def test_numeric_contract_exp(dev, golden_dir):
    import ctypes
    from svs_hip import lib
    L = lib.load()
    # the device's exp / expm1 / row sum against what torch's own routines returned (fixture `primitives`)
    g = dict(np.load(os.path.join(golden_dir, "primitives.npz")))
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    xd = G(g["x"], dev)
    y1, y2 = torch.empty_like(xd), torch.empty_like(xd)
    lib.check(L.svs_selftest_exp(P(xd), P(y1), P(y2), xd.numel(), s))
    for mine, ref in ((y1.cpu().numpy(), g["expf"]), (y2.cpu().numpy(), g["expm1f"])):
        ok = (mine.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(mine) & np.isnan(ref))
        assert ok.all(), (g["x"][~ok][:8], mine[~ok][:8], ref[~ok][:8])
    off = o = 0
    for m in g["sum_lens"]:
        m = int(m)
        nr = 8 if m <= 160 else (2 if m <= 641 else 1)
        if m <= 16000:
            rows = G(g["sum_rows"][off:off + nr * m].reshape(nr, m), dev)
            tg = torch.empty(nr, device=dev)
            lib.check(L.svs_selftest_rowsum(P(rows), P(tg), nr, m, s))
            assert np.array_equal(tg.cpu().numpy(), g["sum_out"][o:o + nr]), m
        off += nr * m
        o += nr
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-104, 89, 200000), -np.logspace(-12, 2, 20000), rng.normal(0, 1e-6, 1000),
                        [0.0, -0.0, 88.7228, 88.73, -103.9, -104.1, np.inf, -np.inf]]).astype(F32)
    xd = G(x, dev)
    y1, y2 = torch.empty_like(xd), torch.empty_like(xd)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    lib.check(L.svs_selftest_exp(P(xd), P(y1), P(y2), x.size, s))
    assert np.array_equal(y1.cpu().numpy().view(np.uint32), orc.ref_exp(x).view(np.uint32))
    assert np.array_equal(y2.cpu().numpy().view(np.uint32), orc.ref_expm1(x).view(np.uint32))
    # IEEE float32 division and sqrt are correctly rounded on the device
    a = (rng.normal(0, 1, 300000) * 10.0 ** rng.integers(-20, 20, 300000)).astype(F32)
    b = (rng.normal(0, 1, 300000) * 10.0 ** rng.integers(-20, 20, 300000)).astype(F32)
    ad, bd = G(a, dev), G(b, dev)
    q, r = torch.empty_like(ad), torch.empty_like(ad)
    lib.check(L.svs_selftest_arith(P(ad), P(bd), P(q), P(r), a.size, s))
    with np.errstate(all="ignore"):
        assert np.array_equal(q.cpu().numpy().view(np.uint32), (a / b).view(np.uint32))
        assert np.array_equal(r.cpu().numpy().view(np.uint32), np.sqrt(np.abs(a)).view(np.uint32))
    for m in (1, 63, 64, 127, 128, 255, 256, 383, 640, 768):
        xx = (rng.uniform(0, 1, (37, m)) * 10.0 ** rng.integers(-6, 4, (37, m))).astype(F32)
        xg = G(xx, dev)
        yg, tg = torch.empty_like(xg), torch.empty(37, device=dev)
        lib.check(L.svs_selftest_cumsum(P(xg), P(yg), P(tg), 37, m, s))
        assert np.array_equal(yg.cpu().numpy().view(np.uint32), orc.canon_cumsum(xx).view(np.uint32)), m
        lib.check(L.svs_selftest_rowsum(P(xg), P(tg), 37, m, s))
        assert np.array_equal(tg.cpu().numpy().view(np.uint32), orc.ref_sum(xx)[:, 0].view(np.uint32)), m


def test_eikonal_points(dev, ops):
    """svs_eikonal_points (network.py:258-266): [the uniform draws ; cam + z_eik * dirs], one product and one sum per
    component like the reference's broadcast expression -- bit-equal to numpy's float32 evaluation, ragged ray counts."""
    rs = np.random.default_rng(4)
    for R in (1, 37, 256, 1000):
        uni = rs.uniform(-3, 3, (R, 3)).astype(F32)
        cam = rs.standard_normal(3).astype(F32)
        z = rs.uniform(0.1, 5.5, (R, 1)).astype(F32)
        dirs = rs.standard_normal((R, 3)).astype(F32)
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        got = ops.eikonal_points(G(uni, dev), G(cam, dev), G(z, dev), G(dirs, dev)).cpu().numpy()
        want = np.concatenate([uni, cam[None, :] + z * dirs], 0)
        assert got.shape == (2 * R, 3) and np.array_equal(got, want)


def test_stage_in(dev, ops):
    """svs_stage_in: a pinned host buffer read by a kernel into device memory == a copy; sizes with a tail of 1..3 words,
    a large buffer, and buffers the kernel does not take (unaligned views, byte tensors) through the fallback copy."""
    rs = np.random.default_rng(6)
    for n in (1, 3, 4, 7, 1021, 200000):
        src = torch.from_numpy(rs.standard_normal(n).astype(F32)).pin_memory()
        dst = torch.zeros(n, device=dev)
        assert ops.stage_in(dst, src) is dst
        assert torch.equal(dst.cpu(), src)
    src = torch.arange(64, dtype=torch.int32).pin_memory()
    dst = torch.zeros(64, dtype=torch.int32, device=dev)
    ops.stage_in(dst, src)
    assert torch.equal(dst.cpu(), src)
    base = torch.from_numpy(rs.standard_normal(33).astype(F32)).pin_memory()
    dst = torch.zeros(32, device=dev)
    ops.stage_in(dst, base[1:])                       # 4-byte aligned only: fallback
    assert torch.equal(dst.cpu(), base[1:])
    b = torch.arange(7, dtype=torch.uint8).pin_memory()
    d = torch.zeros(7, dtype=torch.uint8, device=dev)
    ops.stage_in(d, b)                                # not a multiple of 4 bytes: fallback
    assert torch.equal(d.cpu(), b)


def test_split_last(dev, ops):
    """svs_split_last (network_bg.py:60-62): z[:, :-1] dense and z[:, -1] in one launch."""
    rs = np.random.default_rng(5)
    for R, n in ((1, 2), (37, 98), (256, 98), (1000, 5)):
        z = rs.standard_normal((R, n)).astype(F32)
        head, last = ops.split_last(G(z, dev))
        assert np.array_equal(head.cpu().numpy(), z[:, :-1]) and np.array_equal(last.cpu().numpy(), z[:, -1])


def test_rays(dev, ops, golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "rays.npz")))
    for t in "ab":
        dirs, cam, ds = ops.rays_from_uv(G(g[t + "_uv"], dev), G(g[t + "_pose"], dev), G(g[t + "_K"], dev))
        # bit for bit (F.normalize's norm = sqrt(fma(z, z, fma(y, y, x*x))), svs::norm3)
        assert np.array_equal(dirs.cpu().numpy(), g[t + "_dirs"]) and np.array_equal(cam.cpu().numpy(), g[t + "_cam"])
        assert np.array_equal(ds.cpu().numpy(), g[t + "_depth_scale"])


@pytest.mark.parametrize("name", ["sdf_mlp", "sdf_mlp_w1"])
def test_sdf_mlp_golden(dev, ops, packed, packed_w1, golden_dir, name):
    pk, params = packed_w1 if name.endswith("w1") else packed
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    src = ops.PointSource(points=G(g["x"], dev))
    sdf = ops.sdf_vals(pk, src, 3.0, 20.0)
    np.testing.assert_allclose(sdf.cpu().numpy(), g["sdf_vals"], atol=1e-4)
    sdf2, grad, feat, hbuf, rows = ops.sdf_outputs(pk, src, 3.0, 20.0, want_feature_rows=True)
    np.testing.assert_allclose(sdf2.cpu().numpy(), g["sdf"], atol=1e-4)
    np.testing.assert_allclose(rows.cpu().numpy(), g["feat"], atol=1e-4, rtol=2e-5)
    print(name, "max |sdf err|", float(np.abs(sdf2.cpu().numpy() - g["sdf"]).max()), "max |feat err|",
          float(np.abs(rows.cpu().numpy() - g["feat"]).max()), "max |grad err|", float(np.abs(grad.cpu().numpy() - g["grad"]).max()))
    np.testing.assert_allclose(grad.cpu().numpy(), g["grad"], atol=2e-4, rtol=1e-4)
    _, graw, _, _, _ = ops.sdf_outputs(pk, src, 0.0, 20.0)
    np.testing.assert_allclose(graw.cpu().numpy(), g["grad_raw"], atol=2e-4, rtol=1e-4)
    # radiance MLP fed with the reference's own inputs needs tiles: go through the chain instead
    layers = orc.effective_weights(params, "rendering_network", 5)
    d = np.random.default_rng(3).normal(0, 1, g["x"].shape).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rgb = ops.rgb_eval(pk, src, grad, G(d, dev), feat)
    ref = orc.rgb_mlp_forward(layers, g["x"], g["grad"], d, g["feat"])
    np.testing.assert_allclose(rgb.cpu().numpy(), ref, atol=1e-4)


@pytest.mark.parametrize("P", [1, 31, 128, 1000, 4099])
def test_sdf_mlp_ragged(dev, ops, packed, P):
    pk, params = packed
    layers = orc.effective_weights(params, "implicit_network", 9)
    x = np.random.default_rng(P).uniform(-2.5, 2.5, (P, 3)).astype(F32)
    src = ops.PointSource(points=G(x, dev))
    sdf = ops.sdf_vals(pk, src, 3.0, 20.0).cpu().numpy()
    np.testing.assert_allclose(sdf, orc.sdf_vals(layers, x), atol=1e-4)
    s_ref, f_ref, g_ref = orc.sdf_outputs(layers, x)
    sdf2, grad, feat, hbuf, rows = ops.sdf_outputs(pk, src, 3.0, 20.0, want_feature_rows=True)
    np.testing.assert_allclose(sdf2.cpu().numpy(), s_ref, atol=1e-4)
    np.testing.assert_allclose(rows.cpu().numpy(), f_ref, atol=1e-4)
    np.testing.assert_allclose(grad.cpu().numpy(), g_ref, atol=2e-4, rtol=1e-4)


def test_sdf_ray_mode(dev, ops, packed):
    pk, params = packed
    layers = orc.effective_weights(params, "implicit_network", 9)
    K, pose = synth.make_camera()
    uv = synth.make_uv(40, seed=5)
    dirs, cam, _ = orc.rays_from_uv(uv, pose, K)
    z = np.sort(np.random.default_rng(1).uniform(0.5, 5.0, (40, 98)), -1).astype(F32)
    pts = (cam[None, None] + z[:, :, None] * dirs[:, None, :]).astype(F32).reshape(-1, 3)
    src = ops.PointSource(cam=G(cam, dev), dirs=G(dirs, dev), z=G(z, dev))
    np.testing.assert_allclose(ops.sdf_vals(pk, src, 3.0, 20.0).cpu().numpy(), orc.sdf_vals(layers, pts), atol=1e-4)


def test_composite_golden(dev, ops, golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "composite.npz")))
    R, S = g["z"].shape
    ds = np.linspace(0.8, 1.0, R).astype(F32)[:, None]
    nrm = np.random.default_rng(2).normal(0, 1, (R, S, 3)).astype(F32)
    out = ops.composite(G(g["z"], dev), G(g["sdf"], dev), G(g["rgb"], dev), G(ds, dev),
                        torch.tensor(float(g["beta_param"]), device=dev), 1e-4, normals=G(nrm, dev))
    ref = orc.composite(g["z"], g["sdf"], g["rgb"], orc.get_beta(g["beta_param"]), ds, normals=nrm)
    assert np.array_equal(out["weights"].cpu().numpy().view(np.uint32), ref["weights"].view(np.uint32))
    assert np.array_equal(out["weights"].cpu().numpy(), g["weights"])            # ... and the REFERENCE, bit for bit
    for k in ("rgb_values", "depth_values", "depth_vals", "normal_map"):
        np.testing.assert_allclose(out[k].cpu().numpy(), ref[k], atol=2e-6, err_msg=k)


def forward_edge_scene(S, seed, R=3):
    """Inputs of test_composite_forward_edges / test_composite_bg_forward_edges (beta parameter 0.02): z sorted in [0.5, 5],
    sdf ~ N(0, 0.2), colours in [0, 1], normals, depth_scale in [0.8, 1]."""
    rs = np.random.default_rng(seed)
    z = np.sort(rs.uniform(0.5, 5.0, (R, S)), -1).astype(F32)
    sdf = rs.normal(0, 0.2, (R, S)).astype(F32)
    rgb = rs.uniform(0, 1, (R, S, 3)).astype(F32)
    nrm = rs.normal(0, 1, (R, S, 3)).astype(F32)
    ds = rs.uniform(0.8, 1.0, (R, 1)).astype(F32)
    return z, sdf, rgb, nrm, ds


def assert_f32_reduction(name, got, want, n, scale=None):
    """A float32 sum of n terms (or a quotient of two) against its float64 value `want`, formed from the same float32 terms:
    every term carries at most a few roundings of its own (products, the normalisation of a normal: the + 4) and every
    addition one more on the partial sum, so |got - want| <= (n + 4) 2^-23 scale with scale = sum |term|: `want` itself
    where no term is negative, handed in where the terms change sign."""
    scale = np.abs(want) if scale is None else scale
    err = np.abs(got.astype(np.float64).reshape(want.shape) - want)
    bound = (n + 4) * 2.0 ** -23 * scale
    print(f"{name}: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f} (n = {n})")
    assert (err <= bound).all(), (name, err.max(), bound[err > bound].min())


@pytest.mark.parametrize("S", [2, 63, 64, 65, 256])
def test_composite_forward_edges(dev, ops, S):
    """The forward kernel where its lane-strided loops cross a multiple of 64 and at the limits the entry point accepts: the
    weights bit for bit the oracle's, depth_vals bit for bit z * depth_scale, and the reduced outputs within the float32
    summation bound of the float64 sums over the weights the kernel returned."""
    z, sdf, rgb, nrm, ds = forward_edge_scene(S, seed=S)
    out = ops.composite(G(z, dev), G(sdf.reshape(-1, 1), dev), G(rgb.reshape(-1, 3), dev), G(ds, dev),
                        torch.tensor(0.02, device=dev), 1e-4, normals=G(nrm.reshape(-1, 3), dev))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    ref = orc.composite(z, sdf, rgb, orc.get_beta(0.02), ds, normals=nrm)
    assert np.array_equal(out["weights"].view(np.uint32), ref["weights"].view(np.uint32))
    assert np.array_equal(out["depth_vals"].view(np.uint32), (z * ds).astype(F32).view(np.uint32))
    w, z64, ds64, n64 = (a.astype(np.float64) for a in (out["weights"], z, ds, nrm))
    assert_f32_reduction("rgb_values", out["rgb_values"], (w[:, :, None] * rgb).sum(1), S)
    assert_f32_reduction("depth_values", out["depth_values"], ds64 * ((w * z64).sum(1, keepdims=True) /
                                                                      (w.sum(1, keepdims=True) + 1e-8)), S)
    nhat = n64 / np.sqrt((n64 * n64).sum(-1, keepdims=True))
    assert_f32_reduction("normal_map", out["normal_map"], (w[:, :, None] * nhat).sum(1), S,
                         scale=(w[:, :, None] * np.abs(nhat)).sum(1))


def _oracle_sampler(params, dirs, cam, beta_param, fast, training=False, rng=None):
    layers = orc.effective_weights(params, "implicit_network", 9)
    trace = []
    z, z_eik = orc.error_bound_sampler(lambda p: orc.sdf_vals(layers, p), dirs, cam, orc.get_beta(beta_param),
                                       fast=fast, training=training, rng=rng, trace=trace)
    return z, z_eik, trace


@pytest.mark.parametrize("beta_param,fast,training", [(0.1, -1, False), (0.01, -1, False), (0.001, -1, False),
                                                      (0.01, 1, False), (0.01, 2, False), (0.01, 0, False),
                                                      (0.05, 1, True)])
def test_sampler_bit_exact(dev, ops, packed, beta_param, fast, training):
    """Sampler replayed on the oracle's per-round sdf: every index and every float bit-identical."""
    pk, params = packed
    K, pose = synth.make_camera(center=(0.1, 0.05, -2.5), tilt=0.1)
    R = 48
    uv = synth.make_uv(R, seed=7, margin=0.1)
    dirs, cam, _ = orc.rays_from_uv(uv, pose, K)
    rng = synth.make_train_rng(R, seed=9) if training else None
    z_ref, zeik_ref, trace = _oracle_sampler(params, dirs, cam, beta_param, fast, training, rng)
    trng = None
    if training:
        trng = dict(jitter=G(rng["jitter"], dev), u=G(rng["u"], dev), perm=G(rng["perm"].astype(np.int32), dev),
                    eik_idx=G(rng["eik_idx"].astype(np.int32), dev))
    dbg = {}
    z, z_eik = ops.sample_rays(pk, G(cam, dev), G(dirs, dev), float(beta_param), near=1e-4,
                               scene_bounding_sphere=3.0, sphere_scale=20.0, sdf_clamp_radius=3.0, fast=fast,
                               training=training, rng=trng, debug=dbg,
                               sdf_override=[G(t["samples_sdf"], dev) for t in trace])
    torch.cuda.synchronize()
    for i, t in enumerate(trace):
        d = dbg["rounds"][i]
        n = t["n"]
        assert np.array_equal(d["z"].cpu().numpy()[:, :n].view(np.uint32), t["z"].view(np.uint32)), f"round {i} bins"
        assert np.array_equal(d["sdf"].cpu().numpy()[:, :n].view(np.uint32), t["sdf"].view(np.uint32)), f"round {i} sdf"
        assert np.array_equal(d["beta"].cpu().numpy().view(np.uint32), t["beta"].view(np.uint32)), f"round {i} beta"
        assert np.array_equal(d["cdf"].cpu().numpy()[:, :n].view(np.uint32), t["cdf"].view(np.uint32)), f"round {i} cdf"
        N = t["inds"].shape[1]
        assert np.array_equal(d["inds"].cpu().numpy()[:, :N].astype(np.int64), t["inds"]), f"round {i} inds"
        if t["upsample"]:
            assert np.array_equal(d["samples"].cpu().numpy()[:, :N].view(np.uint32), t["samples"].view(np.uint32))
    assert np.array_equal(z.cpu().numpy().view(np.uint32), z_ref.view(np.uint32))
    if training:
        assert np.array_equal(z_eik.cpu().numpy().view(np.uint32), zeik_ref.view(np.uint32))


@pytest.mark.parametrize("name", ["sampler_eval_b0.1_f-1", "sampler_eval_b0.01_f-1", "sampler_eval_b0.01_f2", "sampler_eval_b0.001_f-1",
                                  "sampler_eval_b0.01_f0", "sampler_eval_b0.01_f1"])
def test_sampler_golden_chain(dev, ops, packed, golden_dir, name):
    """HIP sampler, all rounds chained, on the reference's own per-round sdf (fixture): the final sample set is the
    REFERENCE's bit for bit on every ray."""
    pk, _ = packed
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    nr = int(g["n_rounds"])
    z, _ = ops.sample_rays(pk, G(g["cam"], dev), G(g["dirs"], dev), float(g["beta_param"]), near=1e-4,
                           scene_bounding_sphere=3.0, sphere_scale=20.0, sdf_clamp_radius=3.0, fast=int(g["fast"]),
                           inv_4log=float(g["inv_4log"]),
                           sdf_override=[G(g[f"sdf_{i}"].reshape(g["dirs"].shape[0], -1), dev) for i in range(nr)])
    assert np.array_equal(z.cpu().numpy().view(np.uint32), g["z"].view(np.uint32))


@pytest.mark.parametrize("beta", ["0.1", "0.01", "0.001"])
def test_sampler_r256_on_reference_sdf(dev, ops, packed, golden_dir, beta):
    """256 rays, all rounds (5 at beta <= 0.01), on the REFERENCE's per-round sdf values (fixture sampler256_*), checked
    against the REFERENCE itself: every searchsorted index (49 152 / 147 456 / 147 456), the cdf entries that bracket every
    u, beta per round, the merged bins and the final sample set of all 256 rays are the reference's, bit for bit -- and the
    oracle's chain likewise."""
    pk, params = packed
    g = dict(np.load(os.path.join(golden_dir, f"sampler256_b{beta}.npz")))
    R, nr = g["dirs"].shape[0], int(g["n_rounds"])
    sdfs = [g[f"sdf_{i}"].reshape(R, -1) for i in range(nr)]
    trace = []
    z_ref, _ = orc.error_bound_sampler(None, g["dirs"], g["cam"], orc.get_beta(g["beta_param"]), fast=-1,
                                       inv_4log=g["inv_4log"], sdf_override=sdfs, trace=trace)
    dbg = {}
    z, _ = ops.sample_rays(pk, G(g["cam"], dev), G(g["dirs"], dev), float(g["beta_param"]), near=1e-4,
                           scene_bounding_sphere=3.0, sphere_scale=20.0, sdf_clamp_radius=3.0, fast=-1,
                           inv_4log=float(g["inv_4log"]), debug=dbg, sdf_override=[G(t, dev) for t in sdfs])
    torch.cuda.synchronize()
    assert len(dbg["rounds"]) >= len(trace) == nr
    n_idx = 0
    for i, t in enumerate(trace):
        d, n, N = dbg["rounds"][i], t["n"], t["inds"].shape[1]
        ref = g[f"inds_{i}"].astype(np.int64)
        inds = d["inds"].cpu().numpy()[:, :N].astype(np.int64)
        cdf = d["cdf"].cpu().numpy()[:, :n]
        assert np.array_equal(d["beta"].cpu().numpy().view(np.uint32), g[f"beta_{i}"].view(np.uint32)), f"round {i} beta"
        assert np.array_equal(inds, ref), f"round {i}: {(inds != ref).sum()} indices differ from the reference's"
        assert np.array_equal(np.take_along_axis(cdf, np.maximum(ref - 1, 0), 1), g[f"cdf_lo_{i}"]), f"round {i} cdf"
        assert np.array_equal(np.take_along_axis(cdf, np.minimum(ref, n - 1), 1), g[f"cdf_hi_{i}"]), f"round {i} cdf"
        assert np.array_equal(cdf.view(np.uint32), t["cdf"].view(np.uint32)), f"round {i} cdf vs oracle"
        if f"zmerged_{i}" in g and i + 1 < nr:
            assert np.array_equal(dbg["rounds"][i + 1]["z"].cpu().numpy()[:, :n + N], g[f"zmerged_{i}"]), f"round {i} merged bins"
        n_idx += ref.size
    assert np.array_equal(z.cpu().numpy().view(np.uint32), z_ref.view(np.uint32))
    assert np.array_equal(z.cpu().numpy().view(np.uint32), g["z"].view(np.uint32))
    print(f"sampler256_b{beta}: 0 of {n_idx} indices differ from the reference's; 256/256 rays reproduce its final samples bit for bit")


def test_sampler_r256_train_and_background(dev, ops, packed, golden_dir):
    """The HIP sampler on the reference's 256-ray TRAIN-mode run (jitter, random u, randperm extras, eikonal pick) and on
    its background-model run (sphere-exit far, near = 0, add_tiny): final samples bit for bit the reference's."""
    pk, _ = packed
    g = dict(np.load(os.path.join(golden_dir, "sampler256_train_b0.05.npz")))
    rng = synth.make_train_rng(256, seed=int(g["rng_seed"]))
    trng = dict(jitter=G(rng["jitter"], dev), u=G(rng["u"], dev), perm=G(rng["perm"].astype(np.int32), dev),
                eik_idx=G(rng["eik_idx"].astype(np.int32), dev))
    z, z_eik = ops.sample_rays(pk, G(g["cam"], dev), G(g["dirs"], dev), float(g["beta_param"]), near=1e-4, scene_bounding_sphere=3.0,
                               sphere_scale=20.0, sdf_clamp_radius=3.0, fast=1, training=True, rng=trng,
                               inv_4log=float(g["inv_4log"]), sdf_override=[G(g["sdf_0"], dev)])
    assert np.array_equal(z.cpu().numpy(), g["z"]) and np.array_equal(z_eik.cpu().numpy(), g["z_eik"])
    g = dict(np.load(os.path.join(golden_dir, "sampler256_bg_b0.01.npz")))
    nr = int(g["n_rounds"])
    z, _ = ops.sample_rays(pk, G(g["cam"], dev), G(g["dirs"], dev), float(g["beta_param"]), near=0.0, scene_bounding_sphere=3.0,
                           sphere_scale=1.0, sdf_clamp_radius=0.0, fast=-1, inverse_sphere_bg=True, add_tiny=1e-6,
                           inv_4log=float(g["inv_4log"]), sdf_override=[G(g[f"sdf_{i}"], dev) for i in range(nr)])
    assert np.array_equal(z.cpu().numpy(), g["z"])


def _moved(out, g, tol=3e-4, max_frac=0.06):
    """Samples whose position differs from the reference's.  The sampler itself is the reference's bit for bit
    (test_sampler_r256_on_reference_sdf); what differs at model level are the SDF values it is fed: the fused MLP's agree with
    torch's to ~2e-6 (as any two evaluation orders do), and the inverse-CDF map is ill-conditioned in two places -- where the
    cdf is flat (transmittance ~ 0 behind the surface, denom clamped to 1e-5: one ulp of cdf becomes up to 1e-2 of a bin) and at
    a near-tie of u with a cdf entry (the sample jumps to the neighbouring bin; rare, and it can carry weight).  Either way
    the quadrature changes by less than the tests' bounds on the INTEGRATED outputs, which are asserted on every ray; the
    per-sample arrays are compared on the samples that did not move, and those must be nearly all."""
    moved = np.abs(out["depth_vals"] - g["depth_vals"]) > tol
    assert moved.mean() < max_frac, moved.mean()
    return moved


@pytest.mark.parametrize("beta", ["0.1", "0.01", "0.001"])
def test_model_forward_r256(dev, golden_dir, beta):
    """VolSDFNetwork.forward (HIP, eval, fast = -1, up to five sampler rounds) on 256 rays against the reference (fixture
    forward256_*): colours to 1e-4, depths and normals to 2e-4 on EVERY ray."""
    g = dict(np.load(os.path.join(golden_dir, f"forward256_b{beta}.npz")))
    m, _ = _model(dev, float(g["beta_param"]))
    m.eval()
    inp = {"intrinsics": G(g["K"], dev)[None], "uv": G(g["uv"], dev)[None], "pose": G(g["pose"], dev)[None]}
    with torch.no_grad():
        out = {k: v.cpu().numpy() for k, v in m(inp, fast=-1).items() if torch.is_tensor(v)}
    moved = _moved(out, g, 5e-3)
    print(f"forward256_b{beta}: max err on ALL 256 rays: rgb {np.abs(out['rgb_values'] - g['rgb_values']).max():.2e}, "
          f"depth {np.abs(out['depth_values'].reshape(-1) - g['depth_values'].reshape(-1)).max():.2e}, "
          f"normal {np.abs(out['normal_map'] - g['normal_map']).max():.2e}; {int(moved.sum())} of {moved.size} samples moved "
          f"(largest weight among them {max(g['weights'][moved].max(initial=0.0), out['weights'][moved].max(initial=0.0)):.1e})")
    np.testing.assert_allclose(out["rgb_values"], g["rgb_values"], atol=1e-4)
    np.testing.assert_allclose(out["depth_values"].reshape(-1), g["depth_values"].reshape(-1), atol=2e-4)
    np.testing.assert_allclose(out["normal_map"], g["normal_map"], atol=2e-4)


def test_sampler_end_to_end(dev, ops, packed):
    """Sampler driving the HIP MLP (no override): z within float tolerance of the oracle chain."""
    pk, params = packed
    K, pose = synth.make_camera(center=(0.1, 0.05, -2.5), tilt=0.1)
    R = 64
    uv = synth.make_uv(R, seed=11, margin=0.1)
    dirs, cam, _ = orc.rays_from_uv(uv, pose, K)
    z_ref, _, trace = _oracle_sampler(params, dirs, cam, 0.1, -1)
    z, _ = ops.sample_rays(pk, G(cam, dev), G(dirs, dev), 0.1, near=1e-4,
                           scene_bounding_sphere=3.0, sphere_scale=20.0, sdf_clamp_radius=3.0, fast=-1)
    same = np.abs(z.cpu().numpy() - z_ref).max(-1) < 3e-4
    assert same.mean() >= 0.9, same.mean()


# ------------------------------------------------------------------------------------------------------
# whole model through the reference's call surface
# ------------------------------------------------------------------------------------------------------
def _model(dev, beta, wset="w0"):
    from volsdf.utils.conf import dtu_model_conf
    from volsdf.model.network import VolSDFNetwork
    params = synth.WEIGHT_SETS[wset]()
    m = VolSDFNetwork(dtu_model_conf())
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["density.beta"] = torch.tensor(beta, dtype=torch.float32)
    m.load_state_dict(sd, strict=True)
    return m.to(dev), params


def test_packed_streams_follow_invalidate_packed(dev, ops):
    """A write torch does not see (`bias.data.add_`, like the fused optimiser kernel: no version bump) leaves the packed
    streams as they are -- the documented limit of svs_hip/tensor_cache.py, asserted so that it is a decision --, and
    invalidate_packed() repacks BOTH PackedMlp objects: the model's and the SDF network's own (mesh.py's net.packed())."""
    m, _ = _model(dev, 0.1)
    net = m.implicit_network
    own, pk = net.packed(), m.packed_mlp()
    assert own is not pk
    bits = lambda *streams: [t.view(torch.int32) for t in streams]     # (fp16 pairs: compared as bits, not as floats)
    before = [t.clone() for t in bits(own.sdf_stream, pk.sdf_stream, pk.rgb_stream)]
    for bias in (net.lin3.bias, m.rendering_network.lin2.bias):
        version = bias._version
        bias.data.add_(1.0)
        assert bias._version == version
    assert net.packed() is own and m.packed_mlp() is pk
    for a, b in zip(before, bits(own.sdf_stream, pk.sdf_stream, pk.rgb_stream)):
        assert torch.equal(a, b)
    m.invalidate_packed()
    assert net.packed() is own and m.packed_mlp() is pk
    fresh = ops.PackedMlp(dev)
    sdf_p, rgb_p = m.mlp_params()
    fresh.pack_sdf(*sdf_p)
    fresh.pack_rgb(*rgb_p)
    for a, b, old in zip(bits(fresh.sdf_stream, fresh.sdf_stream, fresh.rgb_stream),
                         bits(own.sdf_stream, pk.sdf_stream, pk.rgb_stream), before):
        assert torch.equal(a, b) and not torch.equal(b, old)


def test_host_copy_of_a_recycled_device_address(dev, ops):
    """_host_f32 of a (4,4) device tensor allocated into the block a freed one left (torch's caching allocator hands it
    straight back; a fresh tensor's version is 0 again) is the second tensor's values, not the first one's cached copy"""
    ops.clear_lookup_caches()
    first = torch.arange(16, dtype=torch.float32, device=dev).reshape(4, 4)
    assert torch.equal(ops._host_f32(first), torch.arange(16, dtype=torch.float32).reshape(4, 4))
    del first
    second = torch.full((4, 4), 7.0, device=dev)
    assert torch.equal(ops._host_f32(second), torch.full((4, 4), 7.0))


@pytest.mark.parametrize("tag", ["eval_b0.1", "eval_b0.01", "eval_b0.01_f1", "train", "w1_eval", "w1_train"])
def test_model_forward_golden(dev, golden_dir, tag):
    """VolSDFNetwork.forward (HIP) against the reference's outputs (fixtures; w1_*: the trained-scale weight set):
    colours to 1e-4, depths / normals to 2e-4 on every ray; per-sample arrays where the sample did not move (`_moved`)."""
    g = dict(np.load(os.path.join(golden_dir, "forward_" + tag + ".npz")))
    m, _ = _model(dev, float(g["beta_param"]), "w1" if tag.startswith("w1") else "w0")
    training = tag.endswith("train")
    m.train(training)
    R = g["uv"].shape[0]
    inp = {"intrinsics": G(g["K"], dev)[None], "uv": G(g["uv"], dev)[None], "pose": G(g["pose"], dev)[None]}
    if training:
        # feed the fixture's draws through torch's CPU RNG call sites, in the reference's order
        draws = synth.make_train_rng(R, seed=int(g["rng_seed"]))
        from rng_inject import inject_rng
        with inject_rng(draws):
            out = m(inp, fast=int(g["fast"]))
    else:
        out = m(inp, fast=int(g["fast"]))
    out = {k: v.detach().cpu().numpy() for k, v in out.items()}
    moved = _moved(out, g)
    print(f"forward_{tag}: {int(moved.sum())} of {moved.size} samples moved; rgb max err on all rays "
          f"{np.abs(out['rgb_values'] - g['rgb_values']).max():.2e}")
    np.testing.assert_allclose(out["xyz"][~moved], g["xyz"][~moved], atol=3e-4)
    np.testing.assert_allclose(out["rgb_values"], g["rgb_values"], atol=1e-4)
    np.testing.assert_allclose(out["depth_values"], g["depth_values"], atol=2e-4)
    assert np.abs(out["weights"][~moved] - g["weights"][~moved]).mean() < 5e-5        # (a moved neighbour re-weights its interval)
    if training:
        np.testing.assert_allclose(out["grad_theta"][:R], g["grad_theta"][:R], atol=2e-4)
    else:
        np.testing.assert_allclose(out["normal_map"], g["normal_map"], atol=2e-4)


def test_model_forward_r256_train(dev, golden_dir):
    """VolSDFNetwork.forward in TRAIN mode (fast = 1; jitter, random u, randperm extras, eikonal points fed through torch's
    CPU RNG call sites) on 256 rays against the reference (forward256_train_b0.05): colours / depths / eikonal gradients on
    every ray."""
    from rng_inject import inject_rng
    g = dict(np.load(os.path.join(golden_dir, "forward256_train_b0.05.npz")))
    m, _ = _model(dev, float(g["beta_param"]))
    m.train()
    inp = {"intrinsics": G(g["K"], dev)[None], "uv": G(g["uv"], dev)[None], "pose": G(g["pose"], dev)[None]}
    with inject_rng(synth.make_train_rng(256, seed=int(g["rng_seed"]))):
        out = {k: v.detach().cpu().numpy() for k, v in m(inp, fast=1).items() if torch.is_tensor(v)}
    moved = _moved(out, g)
    print(f"forward256_train: rgb max err on all rays {np.abs(out['rgb_values'] - g['rgb_values']).max():.2e}, "
          f"{int(moved.sum())} of {moved.size} samples moved")
    np.testing.assert_allclose(out["rgb_values"], g["rgb_values"], atol=1e-4)
    np.testing.assert_allclose(out["depth_values"], g["depth_values"], atol=2e-4)
    np.testing.assert_allclose(out["grad_theta"][:256], g["grad_theta"][:256], atol=2e-4)       # the uniform eikonal points
    np.testing.assert_allclose(out["grad_theta"][256:], g["grad_theta"][256:], atol=5e-3)       # at the sampler's extra depths


def test_model_forward_r1024_train(dev, golden_dir):
    """The bench geometry (configs[1]): VolSDFNetwork.forward in TRAIN mode on 1024 rays against the REFERENCE's forward
    (fixture forward1024_train_b0.05; round 4 pinned this size only in eval mode and against the oracle): colours to 1e-4,
    depths to 2e-4, eikonal gradients on every ray; per-sample weights on every 8th ray where the sample did not move."""
    from rng_inject import inject_rng
    g = dict(np.load(os.path.join(golden_dir, "forward1024_train_b0.05.npz")))
    m, _ = _model(dev, float(g["beta_param"]))
    m.train()
    inp = {"intrinsics": G(g["K"], dev)[None], "uv": G(g["uv"], dev)[None], "pose": G(g["pose"], dev)[None]}
    with inject_rng(synth.make_train_rng(1024, seed=int(g["rng_seed"]))):
        out = {k: v.detach().cpu().numpy() for k, v in m(inp, fast=1).items() if torch.is_tensor(v)}
    ev = int(g["every"])
    sub = dict(depth_vals=out["depth_vals"][::ev])
    moved = _moved(sub, g)
    print(f"forward1024_train: rgb max err on all rays {np.abs(out['rgb_values'] - g['rgb_values']).max():.2e}, "
          f"{int(moved.sum())} of {moved.size} samples (every {ev}th ray) moved")
    np.testing.assert_allclose(out["rgb_values"], g["rgb_values"], atol=1e-4)
    # depths: 2e-4 on every ray that hits the surface; a ray that misses it (depth ~ 5 = far) integrates a flat tail in which
    # one sample sitting in the neighbouring bin -- a near-tie of a random u with a cdf entry, the numpy oracle lands in the
    # same bin as the kernels (tests/test_oracle_golden.py::test_forward_r1024_train) -- moves the depth by 4e-3: one ray here
    dd = np.abs(out["depth_values"] - g["depth_values"]).reshape(-1)
    assert (dd > 2e-4).sum() <= 2 and dd.max() < 1e-2, np.sort(dd)[-4:]
    # ... and ONLY on rays that miss the surface (reference depth = the far bound, 5): every ray that hits it holds 2e-4
    assert np.all(g["depth_values"].reshape(-1)[dd > 2e-4] > 4.5), g["depth_values"].reshape(-1)[dd > 2e-4]
    np.testing.assert_allclose(out["grad_theta"][:1024], g["grad_theta"][:1024], atol=2e-4)     # the uniform eikonal points
    np.testing.assert_allclose(out["grad_theta"][1024:], g["grad_theta"][1024:], atol=5e-3)     # at the sampler's extra depths
    rays = ~moved.any(1)         # (a moved sample changes its neighbours' interval lengths, hence their weights)
    assert rays.mean() > 0.9
    np.testing.assert_allclose(out["weights"][::ev][rays], g["weights"][rays], atol=1e-4)


def test_model_forward_vs_oracle_1024(dev):
    """Full-size batch (1024 rays): integrated outputs against the oracle within 1e-4 / 2e-4 on every ray."""
    m, params = _model(dev, 0.1)
    m.eval()
    K, pose = synth.make_camera()
    uv = synth.make_uv(1024, seed=31)
    inp = {"intrinsics": G(K, dev)[None], "uv": G(uv, dev)[None], "pose": G(pose, dev)[None]}
    out = {k: v.cpu().numpy() for k, v in m(inp, fast=1).items() if torch.is_tensor(v)}
    ref = orc.render_forward(params, uv, pose, K, beta_param=F32(0.1), fast=1)
    _moved(out, ref)
    np.testing.assert_allclose(out["rgb_values"], ref["rgb_values"], atol=1e-4)
    np.testing.assert_allclose(out["depth_values"], ref["depth_values"], atol=2e-4)


# ------------------------------------------------------------------------------------------------------
# a10 / a11
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cost_mapping_inv0_v0", "cost_mapping_inv0_v2", "cost_mapping_inv1_v0",
                                  "cost_mapping_inv1_v2"])
def test_cost_lookup_golden(dev, ops, golden_dir, name):
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    views = synth.make_mvs_views(int(g["seed"]))
    dv = [dict(K=v["K"], c2w=v["c2w"], cost=G(v["cost"], dev), z_mvs=G(v["z_mvs"], dev)) for v in views]
    pj, pi, valid = ops.cost_lookup(dv, int(g["view_index"]), (576, 768), xyz=G(g["xyz"], dev),
                                    inverse_depth=bool(g["inverse_depth"]))
    assert np.array_equal(valid.cpu().numpy(), g["valid"])
    np.testing.assert_allclose(pj.cpu().numpy(), g["pj"], atol=3e-6)
    np.testing.assert_allclose(pi.cpu().numpy(), g["pi"], atol=3e-6)


def test_cost_lookup_ray_mode_full_size(dev, ops):
    """1024 x 98 points against the oracle; ray-parametrised input (cam + z*dir formed in the kernel)."""
    views = synth.make_mvs_views(9, D=192, Hc=72, Wc=96)
    K, pose = views[1]["K"], views[1]["c2w"]
    uv = synth.make_uv(1024, seed=41, margin=0.02)
    dirs, cam, _ = orc.rays_from_uv(uv, pose, K)
    z = np.sort(np.random.default_rng(2).uniform(0.2, 5.5, (1024, 98)), -1).astype(F32)
    xyz = (cam[None, None] + z[:, :, None] * dirs[:, None, :]).astype(F32)
    pj_r, pi_r, valid_r = orc.cost_mapping(xyz, 1, views, (576, 768))
    dv = [dict(K=v["K"], c2w=v["c2w"], cost=G(v["cost"], dev), z_mvs=G(v["z_mvs"], dev)) for v in views]
    pj, pi, valid = ops.cost_lookup(dv, 1, (576, 768), cam=G(cam, dev), dirs=G(dirs, dev), z=G(z, dev))
    agree = valid.cpu().numpy() == valid_r
    assert agree.mean() > 0.9999          # a point exactly on a frustum bound may fall either side
    # D = 192: one float32 ulp of the normalised depth moves the trilinear weight by ~1e-5
    np.testing.assert_allclose(pj.cpu().numpy()[agree], pj_r[agree], atol=5e-5)
    np.testing.assert_allclose(pi.cpu().numpy()[agree], pi_r[agree], atol=5e-5)
    assert np.abs(pj.cpu().numpy()[agree] - pj_r[agree]).mean() < 1e-7


@pytest.mark.parametrize("it", [0, 100, 250])
def test_loss_kernel(dev, ops, golden_dir, it):
    g = dict(np.load(os.path.join(golden_dir, "loss.npz")))
    kw = dict(eikonal_weight=0.1, rgb_weight=1.0, mvs_weight=1.0, sparse_weight=1.0, gce=0.5, confi=1e-3, anneal_rgb=200)
    annealed = it < 200
    anneal = 1.0 - it / 200 if annealed else 0.0
    target = g["rgb_smooth"] if annealed else g["rgb"]
    losses, grads = ops.loss_fwd_bwd(G(g["rgb_values"], dev), G(target, dev), G(g["weights"], dev),
                                     G(g["depth_values"], dev), grad_theta=G(g["grad_theta"], dev), pi=G(g["pi"], dev),
                                     pj=G(g["pj"], dev), rgb_weight=1.0, eikonal_weight=0.1, mvs_weight=1.0,
                                     sparse_weight=1.0, gce=0.5, confi=1e-3, annealed=annealed, anneal_sparse=anneal)
    l = losses.cpu().numpy()
    for i, k in enumerate(("rgb_loss", "eikonal_loss", "mvs_loss", "sparse_loss", "loss")):
        np.testing.assert_allclose(l[i], g[f"it{it}_{k}"], rtol=3e-6, atol=1e-7, err_msg=k)
    # gradients: float64 autograd of oracle/torch_ref.loss_fn (pinned to the reference by test_torch_ref_loss_grid)
    import torch_ref as tref
    t = {k: torch.tensor(g[k], dtype=torch.float64, requires_grad=k in ("rgb_values", "grad_theta", "weights", "depth_values"))
         for k in ("rgb_values", "grad_theta", "weights", "pi", "pj", "depth_values")}
    T = lambda a: torch.tensor(a, dtype=torch.float64).reshape(-1, 3)
    tref.loss_fn(t, T(g["rgb"]), T(g["rgb_smooth"]), it, **kw).backward()
    for k in ("rgb_values", "grad_theta", "weights", "depth_values"):
        ref = t[k].grad.numpy() if t[k].grad is not None else np.zeros_like(g[k])
        np.testing.assert_allclose(grads[k].cpu().numpy().reshape(ref.shape), ref, rtol=2e-5, atol=1e-8, err_msg=k)


def test_fp16x2_accuracy_class(dev):
    """The fp16x2 MLP kernels (two-piece fp16 operands on the 16-bit matrix cores, float32 accumulation) are in the
    accuracy class of the float32-MFMA kernels: on 16 384 random points inside the bounding sphere, the error of sdf,
    d sdf/dx and the feature vector against a float64 evaluation is within 2.5x (5x for the input gradient, whose
    small intermediate values sit on fp16's absolute floor of 2^-25) of the float32 kernels' error and far inside the
    1e-4 / 2e-4 parity bounds.  Measured: sdf 1.8e-6 vs 1.6e-6, gradient 1.0e-5 vs 2.9e-6, feature 2.5e-6 vs 3.0e-6."""
    import torch_ref as tref
    from svs_hip import ops
    params = synth.make_params(0)
    lay = lambda k: [G(params[f"implicit_network.lin{l}.{k}"], dev) for l in range(9)]
    v, g, b = lay("weight_v"), [t.reshape(-1) for t in lay("weight_g")], lay("bias")
    rs = np.random.default_rng(8)
    P = 16384
    x = rs.uniform(-1.5, 1.5, (P, 3)).astype(F32)
    p64 = tref.to_torch(params, torch.float64, requires_grad=False)
    xt = torch.tensor(x, dtype=torch.float64)
    sdf64, feat64, grad64 = tref.sdf_outputs(p64, xt, 3.0, 20.0)
    sdf64, feat64, grad64 = sdf64.detach().numpy(), feat64.detach().numpy(), grad64.detach().numpy()
    err = {}
    for prec in (ops.F32, ops.F16X2):
        pk = ops.PackedMlp(dev, precision=prec)
        pk.pack_sdf(v, g, b)
        sdf, grad, _, _, rows = ops.sdf_outputs(pk, ops.PointSource(points=G(x, dev)), 3.0, 20.0, want_feature_rows=True)
        only = ops.sdf_vals(pk, ops.PointSource(points=G(x, dev)), 3.0, 20.0)
        err[prec] = (np.abs(sdf.cpu().numpy() - sdf64).max(), np.abs(grad.cpu().numpy() - grad64).max(),
                     np.abs(rows.cpu().numpy() - feat64).max(), np.abs(only.cpu().numpy() - sdf64).max())
    print("max |err| vs float64 (sdf, grad, feature, sdf_only): float32 MFMA", err[ops.F32], " fp16x2", err[ops.F16X2])
    for e32, e16, bound, fac in zip(err[ops.F32], err[ops.F16X2], (1e-4, 2e-4, 1e-4, 1e-4), (2.5, 5.0, 2.5, 2.5)):
        assert e16 < bound and e16 < fac * e32 + 1e-6, (e32, e16)
