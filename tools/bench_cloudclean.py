#!/usr/bin/env python3
"""Times the cloud cleaning of svs_hip.cloudclean on a synthetic cloud (no dataset needed): --points points on a noisy unit
sphere plus 1 % floaters, uniform in the box around it.

    python tools/bench_cloudclean.py [--points 5000000] [--repeats 3] [--host-subset 200000] [--cdist-subset 65536]
                                     [--out profiles/cloudclean_bench.txt]

Per phase: milliseconds (after one untimed call, the median of --repeats host-clock intervals that end in a device
synchronise), the bytes the phase has to read and write at the least, and its entry-point calls and kernel launches.  grid
build is svs_cloud_nn without queries (the grid alone); the two neighbour phases include it once per chunk of 2^20 queries,
as `clouds.knn` calls the library, or once when the cloud goes in one call.  Beside them: the same neighbours from sklearn's
kd-tree on the host for a subset, and from torch.cdist + topk on the device for a smaller one (float64, in row blocks), both
compared with the kernel's.
Needs the GPU.
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-volsdf_amd"))


def median_ms(torch, fn, repeats):
    fn()                                   # warm-up: code objects, allocator
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)[len(out) // 2]


def make_cloud(torch, n, floaters=0.01, noise=5e-4):
    g = torch.Generator(device="cuda").manual_seed(0)
    d = torch.randn((n, 3), generator=g, device="cuda", dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True) * (1.0 + noise * torch.randn((n, 1), generator=g, device="cuda", dtype=torch.float64))
    f = (torch.rand((int(n * floaters), 3), generator=g, device="cuda", dtype=torch.float64) - 0.5) * 3.0
    pts = torch.cat([d, f])
    return pts[torch.randperm(pts.shape[0], generator=g, device="cuda")].contiguous()


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--points", type=int, default=5_000_000)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--host-subset", type=int, default=200_000)
    p.add_argument("--cdist-subset", type=int, default=65536)
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import numpy as np
    import torch
    from svs_hip import clouds, lib
    from svs_hip.ops import _ptr, _stream

    L = lib.load()
    pts = make_cloud(torch, a.points)
    n = pts.shape[0]
    K_OUT, K_NRM, CHUNK = 20, 16, 1 << 20
    radius = clouds.default_radius(pts, K_OUT)
    chunks = (n + CHUNK - 1) // CHUNK
    lines = [f"svs_hip.cloudclean: {a.points} points on a noisy unit sphere + {n - a.points} uniform floaters = {n} points; outlier "
             f"score over k = {K_OUT}, normals over k = {K_NRM}, search radius {radius:.4g} (four cells); warm-up, then the median of "
             f"{a.repeats} calls"]
    ms, nbytes, calls, box = {}, {}, {}, {}

    lo, hi = clouds._origin([pts], 1e-6)
    cell = clouds.knn_cell(lo, hi, n, K_OUT)
    ws = torch.empty(L.svs_cloud_grid_bytes(n), dtype=torch.uint8, device=pts.device)
    org = (ctypes.c_double * 3)(*[float(v) for v in lo])
    one = torch.empty(1, dtype=torch.float64, device=pts.device)

    def grid():
        lib.check(L.svs_cloud_nn(_ptr(pts), n, _ptr(pts), 0, org, float(cell), float(radius), _ptr(ws), _ptr(one), None, _stream()),
                  "svs_cloud_nn")
    ms["grid build"] = median_ms(torch, grid, a.repeats)
    nbytes["grid build"] = n * (24 + 12 + 2 * 12 + 24 + 24) + 2 * n * 16
    calls["grid build"] = "1 call, 4 launches + the radix sort's"

    def scores_chunked():
        box["mean_chunked"] = clouds.knn_mean(pts, K_OUT, radius, chunk=CHUNK)
    ms[f"knn k={K_OUT} in chunks"] = median_ms(torch, scores_chunked, a.repeats)
    nbytes[f"knn k={K_OUT} in chunks"] = n * (24 + 8)
    calls[f"knn k={K_OUT} in chunks"] = f"{chunks} calls, each a grid build + 1 launch; rows in the cloud's (random) order"

    def scores():
        box["mean"] = clouds.knn_mean(pts, K_OUT, radius, chunk=n)
    ms[f"knn k={K_OUT} (scores)"] = median_ms(torch, scores, a.repeats)
    nbytes[f"knn k={K_OUT} (scores)"] = n * (24 + 8)
    calls[f"knn k={K_OUT} (scores)"] = "1 call, a grid build + 1 launch; rows in the grid's sorted order"
    assert torch.equal(box["mean"], box["mean_chunked"])

    def stats():
        box["stats"] = clouds.outlier_stats(box["mean"])
    ms["stats"] = median_ms(torch, stats, a.repeats)
    nbytes["stats"] = 2 * n * 8
    calls["stats"] = "1 call, 4 launches, 24 B read back"
    thr = box["stats"]["mean"] + 2.0 * box["stats"]["std"]

    def mask():
        box["keep"] = clouds.threshold_mask(box["mean"], thr)
    ms["mask"] = median_ms(torch, mask, a.repeats)
    nbytes["mask"] = n * 9
    calls["mask"] = "1 call, 1 launch"

    def compact():
        box["kept"] = clouds.compact(pts, box["keep"])
    ms["compaction"] = median_ms(torch, compact, a.repeats)
    m = box["kept"].shape[0]
    nbytes["compaction"] = n * (24 + 1 + 8) + m * 24
    calls["compaction"] = "1 call, the mask scan + 1 launch, 4 B read back"
    kept = box["kept"]
    radius_n = clouds.default_radius(kept, K_NRM)

    def neighbours():
        box["idx"] = clouds.knn(kept, kept, K_NRM, radius_n, exclude_same_index=True, chunk=m)[1]
    ms[f"knn k={K_NRM} (records)"] = median_ms(torch, neighbours, a.repeats)
    nbytes[f"knn k={K_NRM} (records)"] = m * (24 + K_NRM * 12)
    calls[f"knn k={K_NRM} (records)"] = "1 call, a grid build + 1 launch; sorted order"
    centres = torch.tensor([[4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 4.0]], dtype=torch.float64, device=pts.device)

    def normals():
        box["normals"] = clouds.normals_from_neighbors(kept, box["idx"], True, None, centres)
    ms["normals"] = median_ms(torch, normals, a.repeats)
    nbytes["normals"] = m * (24 + K_NRM * 4 + 2 * (K_NRM + 1) * 24 + 16)
    calls["normals"] = "1 call, 1 launch"

    for k in ms:
        lines.append(f"  {k:<22} {ms[k]:10.3f} ms  {nbytes[k] / 1e6:9.1f} MB  {calls[k]}")
    total = sum(ms.values()) - ms["grid build"] - ms[f"knn k={K_OUT} in chunks"]
    lines.append(f"  kept {m} of {n} points (threshold {thr:.6g}); the phases of a cleaning (all but the grid build alone and the chunked "
                 f"variant) add up to {total:.1f} ms")
    floaters_kept = int((box["keep"] & ((pts.norm(dim=1) - 1.0).abs() > 0.01)).sum())
    lines.append(f"  points farther than 0.01 from the sphere that were kept: {floaters_kept} of {int(((pts.norm(dim=1) - 1.0).abs() > 0.01).sum())}")

    # the same neighbours elsewhere
    sub = pts[:min(a.host_subset, n)].contiguous()
    r_sub = clouds.default_radius(sub, K_OUT)
    t_dev = median_ms(torch, lambda: box.__setitem__("sub", clouds.knn(sub, sub, K_OUT, r_sub, exclude_same_index=True)), a.repeats)
    try:
        from sklearn.neighbors import NearestNeighbors
        host = sub.cpu().numpy()
        t0 = time.perf_counter()
        hd, hi_ = NearestNeighbors(n_neighbors=K_OUT + 1, algorithm="kd_tree").fit(host).kneighbors(host)
        t_host = (time.perf_counter() - t0) * 1e3
        gd, gi = box["sub"][0].cpu().numpy(), box["sub"][1].cpu().numpy()
        inside = np.isfinite(gd)
        agree = float((gi[inside] == hi_[:, 1:][inside]).mean())
        exact = float((gd[inside] == hd[:, 1:][inside]).mean())
        lines.append(f"  {sub.shape[0]} points, k = {K_OUT}: kernel {t_dev:.2f} ms, sklearn kd-tree on the host {t_host:.0f} ms "
                     f"({t_host / t_dev:.0f} x); inside the radius the same index in {100 * agree:.4f} % and the same distance bits in "
                     f"{100 * exact:.4f} % of the slots")
    except ImportError:
        lines.append(f"  {sub.shape[0]} points, k = {K_OUT}: kernel {t_dev:.2f} ms; sklearn is not installed, no host figure")
    small = pts[:min(a.cdist_subset, n)].contiguous()
    r_small = clouds.default_radius(small, K_OUT)
    t_k = median_ms(torch, lambda: box.__setitem__("small", clouds.knn(small, small, K_OUT, r_small, exclude_same_index=True)), a.repeats)

    def cdist_topk():
        out = []
        for s in range(0, small.shape[0], 8192):
            d = torch.cdist(small[s:s + 8192], small)
            out.append(torch.topk(d, K_OUT + 1, dim=1, largest=False)[1][:, 1:])
        box["cdist"] = torch.cat(out)
    t_c = median_ms(torch, cdist_topk, a.repeats)
    ok = box["small"][1] >= 0
    agree = float((box["small"][1][ok] == box["cdist"][ok]).double().mean())
    lines.append(f"  {small.shape[0]} points, k = {K_OUT}: kernel {t_k:.2f} ms, torch.cdist + topk on the device (float64, blocks of 8192 "
                 f"rows) {t_c:.1f} ms ({t_c / t_k:.0f} x); the same index in {100 * agree:.4f} % of the slots inside the radius")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
