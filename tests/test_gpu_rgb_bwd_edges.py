"""Edges of the radiance backward sweep (csrc/svs_mlp_bwd_h2.hip: rgb_bwd_h2_kernel) through MlpBackward.run, as
test_gpu_backward.py::test_mlp_backward_vs_autograd drives it: the sweep leaves the stores of a tile in flight across the
barrier that hands the next weight chunk over (Stream::advance_keep<N>, N = 2 stores per tile with f16x2_half, 4 with f16x2),
and a miscounted N shows as garbage in the gradients or as bits that change from run to run.

Main-point counts asked for: 1, 31, 32, 33, 127, 128, 129, 257.  MlpBackward.accumulate refuses a count that is no multiple
of 32 (NotImplementedError: "rays*samples of a group must be a multiple of 32"), so each count runs at the nearest count it
accepts -- 32, 32, 32, 32, 128, 128, 128, 256 -- and the ragged wave tile cannot be reached through this harness.  What the
accepted counts still cover: one live wave of four (32), a full workgroup (128), two (256); 160 and 288 are added for a last
workgroup with ONE live wave tile and three dead waves behind full workgroups.  Cases that share a count share one run."""
import numpy as np
import pytest
import torch

import svs_oracle as orc
import synth
import torch_ref as tref

pytestmark = pytest.mark.gpu
F32 = np.float32
S = 32                      # samples per ray: the main points are R * S
NE = 96                     # eikonal points behind them, as in test_mlp_backward_vs_autograd
COUNTS = [1, 31, 32, 33, 127, 128, 129, 257, 160, 288]
# per-tensor max error over the tensor's max entry against float64 autograd: the bounds of test_mlp_backward_vs_autograd
BOUND = {"f16x2": 3e-5, "f16x2_half": 2e-3}


def accepted(n):
    """the multiple of 32 nearest to n (at least 32)"""
    return max(32, 32 * int(round(n / 32.0)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from svs_hip import ops as _ops
    return _ops


def G(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


_cases = {}


def case(P):
    """Inputs of P main points and the float64 autograd gradients of every parameter (computed once per count)."""
    if P in _cases:
        return _cases[P]
    params = synth.make_params(0)
    rng = np.random.default_rng(1000 + P)
    K, pose = synth.make_camera()
    R = P // S
    uv = synth.make_uv(R, seed=3)
    dirs, cam, _ = orc.rays_from_uv(uv, pose, K)
    z = np.sort(rng.uniform(0.3, 5.9, (R, S)), -1).astype(F32)      # far samples leave the r=3 sphere -> clamp
    x_main = (cam[None, None] + z[:, :, None] * dirs[:, None, :]).astype(F32).reshape(-1, 3)
    x_eik = rng.uniform(-1.5, 1.5, (NE, 3)).astype(F32)
    Wr = rng.normal(0, 1, (P, 3)).astype(F32)
    ws = rng.normal(0, 1, (P, 1)).astype(F32)
    Wg = rng.normal(0, 0.1, (NE, 3)).astype(F32)

    p = tref.to_torch(params, torch.float64, True)
    p["density.beta"].requires_grad_(False)
    xm = torch.tensor(x_main.astype(np.float64), requires_grad=True)
    out = tref.sdf_mlp(p, xm)
    sphere = 20.0 * (3.0 - xm.norm(2, 1, keepdim=True))
    sdf_c = torch.minimum(out[:, :1], sphere)
    grad = torch.autograd.grad(sdf_c.sum(), xm, create_graph=True)[0]
    dflat = torch.tensor(np.repeat(dirs[:, None, :], S, 1).reshape(-1, 3).astype(np.float64))
    rgb = tref.rgb_mlp(p, xm, grad, dflat, out[:, 1:])
    xe = torch.tensor(x_eik.astype(np.float64), requires_grad=True)
    gt = torch.autograd.grad(tref.sdf_mlp(p, xe)[:, :1].sum(), xe, create_graph=True)[0]
    loss = (rgb * torch.tensor(Wr, dtype=torch.float64)).sum() + (sdf_c * torch.tensor(ws, dtype=torch.float64)).sum() \
        + (gt * torch.tensor(Wg, dtype=torch.float64)).sum()
    loss.backward()
    ref = {}
    for net, n in (("rendering_network", 5), ("implicit_network", 9)):
        for l in range(n):
            for name in ("weight_v", "weight_g", "bias"):
                ref[f"{net}.lin{l}.{name}"] = p[f"{net}.lin{l}.{name}"].grad.numpy().copy()
    _cases[P] = dict(params=params, cam=cam, dirs=dirs, z=z, x_eik=x_eik, Wr=Wr, ws=ws, Wg=Wg, R=R, ref=ref)
    return _cases[P]


def hip_grads(c, precision, dev, ops, runs=1):
    """Forward + MlpBackward.run on the HIP kernels, `runs` times from the same inputs: [{parameter name: gradient (numpy)}]."""
    from svs_hip.train import MlpBackward, TrainStreams
    prec = {"f16x2": ops.F16X2, "f16x2_half": ops.F16X2_HALF}[precision]
    params, R = c["params"], c["R"]
    P = R * S
    pk = ops.PackedMlp(dev, precision=prec)
    t = lambda k: G(params[k], dev)
    sdf_p = ([t(f"implicit_network.lin{l}.weight_v") for l in range(9)], [t(f"implicit_network.lin{l}.weight_g") for l in range(9)],
             [t(f"implicit_network.lin{l}.bias") for l in range(9)])
    rgb_p = ([t(f"rendering_network.lin{l}.weight_v") for l in range(5)], [t(f"rendering_network.lin{l}.weight_g") for l in range(5)],
             [t(f"rendering_network.lin{l}.bias") for l in range(5)])
    pk.pack_sdf(*sdf_p)
    pk.pack_rgb(*rgb_p)
    keep = {}
    cam, dirs, z = G(c["cam"], dev), G(c["dirs"], dev), G(c["z"], dev)
    src = ops.PointSource(points=G(c["x_eik"], dev), cam=cam, dirs=dirs, z=z)
    _, gradients, feat_tiles, _, _ = ops.sdf_outputs(pk, src, 3.0, 20.0, clamp_n=P, keep=keep)
    ops.rgb_eval(pk, ops.PointSource(cam=cam, dirs=dirs, z=z), gradients[:P], dirs, feat_tiles, keep=keep)
    bw = MlpBackward(dev, streams=TrainStreams(dev, precision=prec))
    res = []
    for _ in range(runs):
        sdf_g, rgb_g = bw.run(sdf_p, rgb_p, keep, G(c["Wr"], dev), G(c["ws"], dev), G(c["Wg"], dev))
        torch.cuda.synchronize()
        got = {}
        for net, grads in (("rendering_network", rgb_g), ("implicit_network", sdf_g)):
            for l, triple in enumerate(grads):
                for name, g in zip(("weight_v", "weight_g", "bias"), triple):
                    got[f"{net}.lin{l}.{name}"] = g.detach().cpu().numpy().copy()
        res.append(got)
    return res


_grads = {}


@pytest.mark.parametrize("precision", ["f16x2", "f16x2_half"])
@pytest.mark.parametrize("n_main", COUNTS)
def test_rgb_bwd_edges_vs_autograd(dev, ops, precision, n_main):
    """(a) every radiance parameter gradient, and every SDF parameter gradient (they carry what flows back through feat_bar
    and d_normals), against float64 autograd."""
    P = accepted(n_main)
    c = case(P)
    if (P, precision) not in _grads:
        _grads[(P, precision)] = hip_grads(c, precision, dev, ops)[0]
    got = _grads[(P, precision)]
    worst = ("", 0.0)
    for name, ref in c["ref"].items():
        e = rel_err(got[name].reshape(ref.shape), ref)
        if e > worst[1]:
            worst = (name, e)
    print(f"{precision} n_main {n_main} -> {P}: worst relative gradient error {worst[1]:.3e} ({worst[0]})")
    for name, ref in c["ref"].items():
        e = rel_err(got[name].reshape(ref.shape), ref)
        assert e < BOUND[precision], (name, P, e)


@pytest.mark.parametrize("precision", ["f16x2", "f16x2_half"])
@pytest.mark.parametrize("P", sorted({accepted(n) for n in COUNTS}))
def test_rgb_bwd_edges_deterministic(dev, ops, precision, P):
    """(b) in deterministic mode (SVS_DETERMINISTIC=1 = svs_set_deterministic(1)) two runs of the same input give equal bits."""
    from svs_hip import lib
    L = lib.load()
    was = L.svs_set_deterministic(1)
    try:
        first, second = hip_grads(case(P), precision, dev, ops, runs=2)
    finally:
        L.svs_set_deterministic(was)
    for name in first:
        assert np.array_equal(first[name].view(np.uint32), second[name].view(np.uint32)), (name, P)
        assert np.isfinite(first[name]).all(), (name, P)
