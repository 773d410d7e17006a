"""svs_clip_guard_adam (csrc/svs_optim.hip) at the edges of its input space: lengths with a scalar tail and past one pass
of the grid-stride loop, gradient norms on both sides of max_norm, max_norm = 0, non-finite gradients, a float32 norm that
overflows, long runs with other hyper-parameters, the info[] outputs and a rejected (misaligned) call.

References: a float64 restatement of clip_grad_norm_(max_norm) -> NaN/Inf guard -> Adam, following the contract at the top
of svs_optim.hip (a non-finite gradient is zeroed and the step still runs; max_norm <= 0 disables clipping), and torch's
float32 CPU torch.optim.Adam driven through the same sequence."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32 = np.float32
GRID_PASS = 2048 * 256 * 4          # entries one pass of adam_kernel's grid covers


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def ulp32(x):
    return float(np.spacing(F32(np.abs(x).max())))


def ref_f64(p0, grads, max_norm, lr, betas, eps):
    """float64 clip_grad_norm_ -> guard -> Adam; returns p, m, v and the per-step (norm, dropped)."""
    b1, b2 = betas
    p, m, v = p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size)
    info = []
    for t, g32 in enumerate(grads, 1):
        g = g32.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            norm = float(np.sqrt((g * g).sum()))
        drop = not np.isfinite(g).all()
        info.append((norm, drop))
        if drop:
            g = np.zeros_like(g)
        elif max_norm > 0:
            g = g * min(1.0, max_norm / (norm + 1e-6))
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    return p, m, v, info


def ref_torch32(p0, grads, max_norm, lr, betas, eps):
    """torch.optim.Adam in float32 on the CPU, after the guard and clip_grad_norm_ (skipped for max_norm <= 0)."""
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        if not torch.isfinite(p.grad).all():
            p.grad.zero_()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
    st = opt.state_dict()["state"][0]
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def run_fused(dev, p0, grads, on_device, **hp):
    """FusedAdam over the gradient sequence; step as an argument or (on_device) from the device counter."""
    from svs_hip.trainer import FusedAdam
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dev))
    opt = FusedAdam([p], **hp)
    if on_device:
        opt.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    gd = torch.from_numpy(np.stack(grads)).to(dev)
    for k in range(len(grads)):
        p.grad.copy_(gd[k])
        opt.step()
    torch.cuda.synchronize()
    if on_device:
        assert int(opt.step_dev) == len(grads)
    return [t.detach().clone() for t in (opt.fp.flat, opt.fp.grad, opt.exp_avg, opt.exp_avg_sq, opt.info)]


def _grads(n, steps, target_norm, seed):
    rs = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        g = rs.normal(0, 1, n)
        out.append((g * (target_norm / np.sqrt((g * g).sum()))).astype(F32))
    return out


def _check(dev, p0, grads, max_norm=1.0, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, torch32=True):
    hp = dict(max_norm=max_norm, lr=lr, betas=betas, eps=eps)
    a = run_fused(dev, p0, grads, False, **hp)
    b = run_fused(dev, p0, grads, True, **hp)
    for x, y in zip(a, b):                                    # step as an argument == the device step counter, bit for bit
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    p, g, m, v, info = [t.cpu().numpy() for t in a]
    assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all()
    rp, rm, rv, rinfo = ref_f64(p0, grads, **hp)
    norm, drop = rinfo[-1]
    assert info[1] == (1.0 if drop else 0.0)
    if np.isfinite(norm):
        assert abs(float(info[0]) - norm) <= 1e-6 * norm
    else:
        assert not np.isfinite(info[0])
    if drop:
        assert not g.any()                                    # the dropped gradient stays visible as zeros
    err = np.abs(p - rp).max()
    # a few steps: a few float32 roundings of each parameter per step; the moments 2e-6 of each array's scale
    bound = 4 * len(grads) * ulp32(rp)
    bm, bv = 2e-6 * np.abs(rm).max(), 2e-6 * np.abs(rv).max()
    if torch32:
        tp, tm, tv = ref_torch32(p0, grads, **hp)
        if len(grads) > 10:
            # long runs: no less accurate than torch's own float32 Adam (up to a few ulps of the parameters); the float32
            # averages of both drift from float64 by far more than one rounding
            bound = 2 * np.abs(tp - rp).max() + 4 * ulp32(rp)
            bm, bv = bm + 2 * np.abs(tm - rm).max(), bv + 2 * np.abs(tv - rv).max()
        elif p0.size < 10 ** 6:
            # (over millions of entries torch's float32 norm is itself off by ~1e-5, which its clipped gradient inherits)
            np.testing.assert_allclose(p, tp, rtol=0, atol=3e-7)
            np.testing.assert_allclose(m, tm, rtol=2e-6, atol=5e-9)
            np.testing.assert_allclose(v, tv, rtol=2e-6, atol=1e-11)
    print(f"n={p0.size} steps={len(grads)} |p - f64| = {err:.3e} (bound {bound:.3e}), m {np.abs(m - rm).max():.2e} "
          f"(bound {bm:.2e}) v {np.abs(v - rv).max():.2e} (bound {bv:.2e}) info[0] rel "
          f"{abs(float(info[0]) - norm) / norm if np.isfinite(norm) and norm else 0.0:.2e}")
    assert err <= bound
    assert np.abs(m - rm).max() <= bm + 1e-30
    assert np.abs(v - rv).max() <= bv + 1e-30


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4097, GRID_PASS + 3, 2 * GRID_PASS + 7])
@pytest.mark.parametrize("target_norm", [0.4, 7.0])       # below / above max_norm = 1
def test_adam_lengths_and_clipping(dev, n, target_norm):
    p0 = np.linspace(-0.5, 0.5, n).astype(F32)
    _check(dev, p0, _grads(n, 3, target_norm, seed=n))


@pytest.mark.parametrize("n", [5, 4097])
def test_adam_max_norm_zero_disables_clipping(dev, n):
    p0 = np.linspace(-0.5, 0.5, n).astype(F32)
    _check(dev, p0, _grads(n, 3, 7.0, seed=n + 1), max_norm=0.0)


@pytest.mark.parametrize("n", [5, 4097])
@pytest.mark.parametrize("kind", ["nan", "+inf", "-inf", "1e20"])
def test_adam_non_finite_and_overflowing_gradients(dev, n, kind):
    """The bad entry sits in the second of three steps, at the scalar tail for n = 5; 1e20 entries are finite but their
    float32 sum of squares overflows (the kernel forms the norm in float64 and clips; float32 torch sees an inf norm)."""
    p0 = np.linspace(-0.5, 0.5, n).astype(F32)
    grads = _grads(n, 3, 2.0, seed=3 * n)
    if kind == "1e20":
        grads[1][0] = grads[1][n - 1] = 1e20
    else:
        grads[1][n - 1] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
    _check(dev, p0, grads[:2], torch32=kind != "1e20")       # info[] of the step that holds the bad entry
    _check(dev, p0, grads, torch32=kind != "1e20")


@pytest.mark.parametrize("hp", [dict(lr=1e-3, betas=(0.5, 0.99), eps=1e-6), dict()])
def test_adam_long_run(dev, hp):
    """2000 steps: the bias corrections go from their first values to ~1; gradient norms vary around max_norm."""
    n, steps = 4097, 2000
    rs = np.random.default_rng(11)
    scale = rs.uniform(0.2, 3.0, steps)
    grads = [(rs.normal(0, 1, n) * (s / np.sqrt(n))).astype(F32) for s in scale]
    p0 = np.linspace(-0.5, 0.5, n).astype(F32)
    _check(dev, p0, grads, **hp)


def test_adam_misaligned_call_changes_nothing(dev):
    """A buffer 4 bytes off 16-byte alignment: SVS_EINVAL, and the parameters, moments, gradient, step counter and
    workspace are as before the call (the check used to run after the statistics launch had bumped the counter)."""
    from svs_hip import lib
    from svs_hip.ops import _ptr, _stream
    L = lib.load()
    n = 1000
    gen = torch.Generator(device="cpu").manual_seed(3)
    bufs = [torch.randn(n + 4, generator=gen).to(dev) for _ in range(4)]          # params, grads, exp_avg, exp_avg_sq
    bufs[3].abs_()
    ws = torch.full((L.svs_adam_workspace_bytes() // 4,), 7, dtype=torch.int32, device=dev)
    counter = torch.full((1,), 5, dtype=torch.int32, device=dev)
    info = torch.full((2,), -3.0, device=dev)
    before = [t.clone() for t in bufs + [ws, counter, info]]
    for which in range(4):
        args = [b.data_ptr() + (4 if k == which else 0) for k, b in enumerate(bufs)]
        rc = L.svs_clip_guard_adam(*args, n, 0, _ptr(counter), 1.0, 5e-4, 0.9, 0.999, 1e-8, _ptr(ws), _ptr(info), _stream())
        assert rc == -1                                        # SVS_EINVAL
        torch.cuda.synchronize()
        for x, y in zip(bufs + [ws, counter, info], before):
            assert torch.equal(x, y)
    # and the aligned call on the same buffers runs and advances the counter
    rc = L.svs_clip_guard_adam(*[b.data_ptr() for b in bufs], n, 0, _ptr(counter), 1.0, 5e-4, 0.9, 0.999, 1e-8,
                               _ptr(ws), _ptr(info), _stream())
    assert rc == 0
    assert int(counter) == 6
