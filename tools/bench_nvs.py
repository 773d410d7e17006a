"""Novel-view scores of one synthetic DTU scan (svs_hip.nvs.score_views, csrc/svs_nvs.hip): 25 evaluation views at 576x768.

    python tools/bench_nvs.py [--views 25] [--hw 576 768] [--iters 50] [--warmup 5] [--no-oracle]

Prints one JSON line: device ms per scan (events around svs_nvs_score on device-resident uint8 inputs; no file I/O and
no host copies), the kernel launches per call, the algorithmic bytes per scan and the share of the HBM peak they imply,
and the numpy oracle's CPU time for the same scan for scale.  Needs the MI355X: there is no CPU path.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-volsdf_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X HBM3E, spec


def algorithmic_bytes(V, H, W, tiles):
    """Every array touched once: the three (V,H,W,3) uint8 inputs, the per-tile partial records written and read back
    (40 bytes each), the (V,3) float64 output."""
    inputs = 3 * V * H * W * 3
    partials = 2 * V * tiles * 40
    return dict(inputs=inputs, partials=partials, out=V * 24, total=inputs + partials + V * 24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=25)
    ap.add_argument("--hw", type=int, nargs=2, default=(576, 768))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true", help="skip the CPU oracle timing")
    a = ap.parse_args()
    import numpy as np
    import torch
    from svs_hip import lib
    from svs_hip.ops import _ptr, _stream
    if not torch.cuda.is_available():
        raise SystemExit("bench_nvs.py needs the GPU (there is no CPU path)")
    V, (H, W) = a.views, a.hw
    rng = np.random.default_rng(a.seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (40 + 150 * yy / H + 50 * np.sin(xx / 5.0))[None, ..., None]
    gt = np.clip(np.rint(base + rng.normal(0, 15, (V, H, W, 3))), 0, 255).astype(np.uint8)
    pred = np.clip(gt.astype(int) + np.rint(rng.normal(0, 6, gt.shape)).astype(int), 0, 255).astype(np.uint8)
    mask = (rng.random(gt.shape) < 0.8).astype(np.uint8)
    dev = torch.device("cuda:0")
    L = lib.load()
    p, g, m = (torch.from_numpy(x).to(dev) for x in (pred, gt, mask))
    ws = torch.empty(int(L.svs_nvs_workspace_bytes(V, H, W)), dtype=torch.uint8, device=dev)
    out = torch.empty(V, 3, dtype=torch.float64, device=dev)

    def call():
        lib.check(L.svs_nvs_score(_ptr(p), _ptr(g), _ptr(m), V, H, W, _ptr(ws), _ptr(out), _stream()), "svs_nvs_score")

    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        call()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.iters
    r = out.cpu().numpy()
    assert np.isfinite(r).all() and (r[:, 2] > 0).all() and (r[:, 2] < 1).all()
    tiles = ((W + 63) // 64) * ((H + 15) // 16)
    b = algorithmic_bytes(V, H, W, tiles)
    res = dict(metric="nvs_ms_per_scan", views=V, hw=[H, W], iters=a.iters, ms_per_scan=round(ms, 4),
               kernel_launches_per_call=2, algorithmic_bytes_per_scan=b["total"], bytes_by_part=b,
               hbm_peak_fraction=round(b["total"] / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 4),
               device=torch.cuda.get_device_name(0))
    if not a.no_oracle:
        import nvs_oracle
        t = time.perf_counter()
        want_p, want_s = nvs_oracle.score_views(pred, gt, mask)
        res["oracle_cpu_s_per_scan"] = round(time.perf_counter() - t, 3)
        with np.errstate(divide="ignore", invalid="ignore"):
            psnr = -10.0 * np.log10(r[:, 0] / (255.0 * 255.0) / r[:, 1])
        res["max_abs_diff_vs_oracle"] = dict(psnr_db=float(np.abs(psnr - want_p).max()),
                                             ssim=float(np.abs(r[:, 2] - want_s).max()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
