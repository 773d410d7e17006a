"""Image-based rendering of one evaluation view (svs_hip.ibr.blend_view, csrc/svs_ibr.hip) at the DTU / BlendedMVS size.

    python tools/bench_ibr.py [--hw 576 768] [--n-src 3] [--iters 50] [--warmup 5] [--no-oracle]

Prints one JSON line: device ms per view (events around blend_view on device-resident inputs: geometry, ray directions,
weights and blend; no file I/O), the algorithmic bytes per view and the share of the HBM peak they imply, the kernel
launches per view, and the numpy oracle's CPU time for the same view for scale.  Needs the MI355X: there is no CPU path.
"""
import argparse
import json
import os
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-volsdf_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "oracle"),
          os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X HBM3E, spec


def algorithmic_bytes(n, H, W):
    """Every array each launch must touch, read or written once: svs_fuse_view (per-source outputs only), the n+1
    svs_rays_from_uv fields, svs_ibr_weights (both kernels) and svs_ibr_laplacian_blend (pyrDown x3, three levels)."""
    hw, nj = H * W, n + 1
    fuse = hw * (4 + 4 + 4 * n) + hw * (8 + 3) + n * hw * (1 + 4 + 4 + 4)      # depths + confidence in, outputs
    rays = nj * hw * (8 + 12 + 4)                                              # uv in, dirs + depth_scale out
    weights = n * hw * (8 + 1 + 12 + 12) + hw * (12 + 12) + nj * hw * (12 + 4) + n * hw   # gathers counted once
    erode = n * hw + nj * hw * 4 + nj * hw * 4
    blend = 0
    for lv in range(3):                                                        # pyrDown: level lv -> lv+1
        blend += nj * (hw >> (2 * lv)) * 16 + nj * (hw >> (2 * lv + 2)) * 16
    for lv in range(3):                                                        # blend level lv: g, m, coarse g, out
        blend += nj * (hw >> (2 * lv)) * 16 + nj * (hw >> (2 * lv + 2)) * 12 + (hw >> (2 * lv + 2)) * 12 + (hw >> (2 * lv)) * 12
    return dict(fuse_view=fuse, rays=rays, weights=weights + erode, blend=blend, total=fuse + rays + weights + erode + blend)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, nargs=2, default=(576, 768))
    ap.add_argument("--n-src", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=52)
    ap.add_argument("--no-oracle", action="store_true", help="skip the CPU oracle timing")
    a = ap.parse_args()
    import torch
    import synth
    from svs_hip import ibr
    if not torch.cuda.is_available():
        raise SystemExit("bench_ibr.py needs the GPU (there is no CPU path)")
    H, W = a.hw
    n = a.n_src
    views = synth.make_fusion_views(a.seed, hw=(H, W), n_views=n + 1)
    dev = torch.device("cuda:0")

    def on_dev(v, img=True):
        d = dict(K=v["K"], E=v["E"], depth=torch.from_numpy(v["depth"]).to(dev))
        if img:
            d["img"] = torch.from_numpy(v["img"]).to(dev)
        return d

    ref = on_dev(views[1], img=False)
    srcs = [on_dev(views[k]) for k in range(n + 1) if k != 1]
    pred = torch.from_numpy(views[1]["img"]).to(dev)
    for _ in range(a.warmup):
        out = ibr.blend_view(ref, srcs, pred)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        out = ibr.blend_view(ref, srcs, pred)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.iters
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    b = algorithmic_bytes(n, H, W)
    res = dict(metric="ibr_ms_per_view", hw=[H, W], n_src=n, iters=a.iters, ms_per_view=round(ms, 4),
               algorithmic_bytes_per_view=b["total"], bytes_by_stage=b,
               hbm_peak_fraction=round(b["total"] / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 4),
               kernel_launches_per_view=2 + (n + 1) + 2 + 6,         # confidence fill + fuse, rays, weights, blend
               host_to_device_copies_per_view=1 + 2 * (n + 1),
               device=torch.cuda.get_device_name(0))
    if not a.no_oracle:
        import ibr_oracle
        t = time.perf_counter()
        ibr_oracle.blend_view(views[1], [views[k] for k in range(n + 1) if k != 1], views[1]["img"])
        res["oracle_cpu_s_per_view"] = round(time.perf_counter() - t, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
