"""The fused loss kernel (svs_loss: loss_rays_kernel + loss_reduce_kernel) against the reference's VolSDFLoss in float64
(tests/golden/loss_grid.npz, make_fixtures.fx_loss_grid) over gce in {0, 0.5, 1}, the MVS / sparsity switches, both
annealing phases, batches with and without pi / pj and grad_theta, the three confidence classes of a ray, zero weights,
zero-norm and unit-norm grad_theta rows, and shapes from one ray of one sample to S = 256 (four samples per lane), R not
a multiple of the four units of a block and eikonal counts that are not multiples of 64."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TERMS = ("rgb_loss", "eikonal_loss", "mvs_loss", "sparse_loss", "loss")
GRADS = ("rgb_values", "grad_theta", "weights", "depth_values")
N_CASES = 27


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def grid(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "loss_grid.npz")))
    assert len(g["cases"]) == N_CASES
    return g


def _run(dev, g, c, norm=None, on_device=False):
    from svs_hip import ops
    k, j = (int(x) for x in g["cases"][c])
    R, S, n_eik = (int(x) for x in g["shapes"][k])
    gce, mvs_w, has_pi, it, sp_w = (float(x) for x in g["settings"][j])
    anneal_rgb = int(g["anneal_rgb"])
    annealed = sp_w > 0 and anneal_rgb > 0 and it < anneal_rgb          # loss.py:101-104
    anneal = 1.0 - it / anneal_rgb if annealed else 0.0
    G = lambda n: torch.from_numpy(np.ascontiguousarray(g[f"s{k}_{n}"])).to(dev)
    opt = lambda n, on: G(n) if on else None
    scal = dict(annealed=annealed, anneal_sparse=anneal)
    if on_device:           # the run-time values on the device; the host scalars say the opposite and must be ignored
        scal = dict(annealed=not annealed, anneal_sparse=0.5 - anneal,
                    anneal_dev=torch.tensor([1.0 if annealed else 0.0, anneal], dtype=torch.float32, device=dev))
    losses, grads = ops.loss_fwd_bwd(G("rgb_values"), G("rgb_smooth" if annealed else "rgb"), G("weights"),
                                     G("depth_values"), grad_theta=opt("grad_theta", n_eik), pi=opt("pi", has_pi),
                                     pj=opt("pj", has_pi), rgb_weight=1.0, eikonal_weight=0.1, mvs_weight=mvs_w,
                                     sparse_weight=sp_w, gce=gce, confi=float(g["confi"]), norm=norm, **scal)
    torch.cuda.synchronize()
    return (R, S, n_eik), losses.cpu(), {n: (v.cpu() if v is not None else None) for n, v in grads.items()}


@pytest.mark.parametrize("c", range(N_CASES))
def test_loss_grid(dev, grid, c):
    """Each case three times: against the reference (losses to 3e-6, gradients to 2e-5 of each array's max); with
    norm = (2R, 2 n_eik), what each of two equal ray groups passes, where every loss and gradient is exactly half of the
    whole-batch run (divisions by powers of two are exact); and with the annealing phase read on the device (anneal_dev),
    which gives the host-scalar path's bits."""
    (R, S, n_eik), losses, grads = _run(dev, grid, c)
    l = losses.numpy().astype(np.float64)
    assert np.isfinite(l).all()
    ref = np.array([float(grid[f"c{c}_{n}"]) for n in TERMS])
    for i, n in enumerate(TERMS[:4]):
        assert abs(l[i] - ref[i]) <= 3e-6 * abs(ref[i]), (n, l[i], ref[i])
    # the total: 3e-6 of the sum of the weighted terms' magnitudes (with gce = 1 the MVS term is negative, the others not)
    k, j = (int(x) for x in grid["cases"][c])
    _, mvs_w, _, it, sp_w = grid["settings"][j]
    anneal = 1.0 - it / 200 if (sp_w > 0 and it < 200) else 0.0
    scale = abs(ref[0]) + 0.1 * abs(ref[1]) + mvs_w * abs(ref[2]) + sp_w * anneal * abs(ref[3])
    assert abs(l[4] - ref[4]) <= 3e-6 * scale, (l[4], ref[4], scale)
    worst = {}
    for n in GRADS:
        if n == "grad_theta" and not n_eik:
            assert grads[n] is None
            continue
        r = grid[f"c{c}_d_{n}"]
        got = grads[n].numpy().reshape(r.shape).astype(np.float64)
        assert np.isfinite(got).all(), n
        tol = 2e-5 * np.abs(r).max()
        worst[n] = np.abs(got - r).max() / (np.abs(r).max() or 1.0)
        assert np.abs(got - r).max() <= tol, (n, worst[n])
    print(f"case {c} R={R} S={S} n_eik={n_eik}: loss rel {np.abs(l[:4] - ref[:4]).max() / (np.abs(ref[:4]).max() or 1):.1e}"
          f" grads rel-to-max {max(worst.values()):.1e}")
    l2, g2 = _run(dev, grid, c, norm=(2 * R, 2 * n_eik))[1:]
    assert torch.equal(l2, losses * 0.5)
    l3, g3 = _run(dev, grid, c, on_device=True)[1:]
    assert torch.equal(l3, losses)
    for n in GRADS:
        if grads[n] is not None:
            assert torch.equal(g2[n], grads[n] * 0.5), n
            assert torch.equal(g3[n], grads[n]), n
