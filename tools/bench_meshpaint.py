#!/usr/bin/env python3
"""Times svs_hip.meshpaint on a synthetic mesh (no dataset needed): the marching-cubes mesh of tools/bench_meshview.py (a sphere
and a floor at --resolution), painted from 16 synthetic 1152x1536 photographs on a ring around it.

    python tools/bench_meshpaint.py [--resolution 512 [48 ...]] [--views 16] [--repeats 5] [--inner 10] [--out profiles/meshpaint_bench.txt]

Per phase: milliseconds (after one untimed call, the median of --repeats host-clock intervals that end in a device
synchronise, each over --inner back-to-back calls, divided by --inner), and the bytes the phase has to move.  paint is
svs_mesh_paint alone on ready depth maps; beside it the bytes it gathers, their rate against the achievable HBM rate
tools/bench_tsdf.py uses, and the time of the same arithmetic written in torch ops on the same inputs (a float64
projection, index gathers as grid_sample does them, a weighted sum), whose accumulators are compared with the kernel's.
Needs the GPU.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-volsdf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_ACHIEVABLE = 6.3e12                    # bytes/s: a float4 copy on one MI355X (tools/bench_tsdf.py)


def median_ms(torch, fn, repeats, inner=1):
    fn()                                   # warm-up: code objects, allocator
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / inner)
    return sorted(out)[len(out) // 2]


def make_images(torch, n, H, W):
    """smooth seeded photographs with noise on top -> [(H,W,3) uint8 device tensors]"""
    g = torch.Generator(device="cuda").manual_seed(0)
    ys = torch.linspace(0, 1, H, device="cuda")[:, None, None]
    xs = torch.linspace(0, 1, W, device="cuda")[None, :, None]
    out = []
    for i in range(n):
        phase = torch.tensor([0.3 * i, 0.5 * i + 1.0, 0.7 * i + 2.0], device="cuda")
        smooth = 0.5 + 0.4 * torch.sin(6.0 * xs + 4.0 * ys + phase)
        noise = 0.1 * (torch.rand((H, W, 3), generator=g, device="cuda") - 0.5)
        out.append(((smooth + noise).clamp(0, 1) * 255).round().to(torch.uint8).contiguous())
    return out


def torch_paint(torch, verts, normals, mats, depth, images, near, rel, abs_tol, cos_min, power):
    """svs_mesh_paint's blend in torch ops, float64, view by view -> acc (V,4), (vertex, view) pairs inside an image, pairs
    that contribute"""
    p = verts.double()
    n = normals.double()
    V = p.shape[0]
    acc = torch.zeros((V, 4), dtype=torch.float64, device=p.device)
    lit = torch.isfinite(n).all(1) & ~(n == 0).all(1)
    inside_pairs = torch.zeros((), dtype=torch.int64, device=p.device)
    used_pairs = torch.zeros((), dtype=torch.int64, device=p.device)
    n_views, H, W = depth.shape
    for v in range(n_views):
        K, E = mats[v, :9].reshape(3, 3), mats[v, 9:].reshape(3, 4)
        cam = p @ E[:, :3].T + E[:, 3]
        q = cam @ K.T
        x, y, z = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], cam[:, 2]
        ok = lit & (z > near) & torch.isfinite(z) & torch.isfinite(x) & torch.isfinite(y)
        ok &= (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
        inside_pairs += ok.sum()
        xs, ys = torch.where(ok, x, torch.zeros_like(x)), torch.where(ok, y, torch.zeros_like(y))
        iu, iv = torch.floor(xs + 0.5).long(), torch.floor(ys + 0.5).long()
        d = depth[v][iv, iu].double()
        ok &= (d == 0) | (z <= d * (1.0 + rel) + abs_tol)
        eye = -(E[:, :3].T @ E[:, 3])
        t = eye - p
        c = ((n * t).sum(1) / t.norm(dim=1)).abs()
        ok &= c >= cos_min
        w = torch.where(ok, c ** power, torch.zeros_like(c))
        used_pairs += ok.sum()
        x0, y0 = torch.floor(xs), torch.floor(ys)
        fx, fy = (xs - x0)[:, None], (ys - y0)[:, None]
        ix0, iy0 = x0.long(), y0.long()
        ix1, iy1 = (ix0 + 1).clamp(max=W - 1), (iy0 + 1).clamp(max=H - 1)
        img = images[v]
        col = ((1 - fx) * img[iy0, ix0].double() + fx * img[iy0, ix1].double()) * (1 - fy) + \
              ((1 - fx) * img[iy1, ix0].double() + fx * img[iy1, ix1].double()) * fy
        acc[:, :3] += w[:, None] * col
        acc[:, 3] += w
    return acc, inside_pairs, used_pairs


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--resolution", type=int, nargs="+", default=[512], help="one run per grid resolution")
    p.add_argument("--views", type=int, default=16)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--inner", type=int, default=10, help="back-to-back calls per timed interval")
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import numpy as np
    import torch
    import bench_meshview as bmv
    from svs_hip import lib, mesh, meshpaint as mpt, meshview as mvw

    text = "\n".join(bench(a, r, np, torch, bmv, lib, mesh, mpt, mvw) for r in a.resolution)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def bench(a, resolution, np, torch, bmv, lib, mesh, mpt, mvw):
    """one run -> its lines"""
    from svs_hip import views as svs_views
    if a.views > mvw.MAX_VIEWS:
        raise SystemExit(f"--views: at most {mvw.MAX_VIEWS} (one launch of svs_mesh_paint is what is timed)")
    H, W = bmv.H, bmv.W
    views = bmv.make_views(np, a.views)
    verts, faces = bmv.make_mesh(torch, mesh, resolution)
    verts, faces, _ = svs_views.mesh_args(verts, faces)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    images = make_images(torch, a.views, H, W)
    mats = svs_views.mats(views, verts.device)
    rules = dict(near=1e-6, rel=0.01, abs_tol=0.0, cos_min=0.1, power=2)
    lines = [f"svs_hip.meshpaint: marching cubes of a sphere and a floor at {resolution}^3 = {V} vertices, {F} faces; {a.views} views of "
             f"{H} x {W}; warm-up, then the median of {a.repeats} intervals of {a.inner} calls each"]
    ms, nbytes = {}, {}

    box = {}
    def normals():
        box["normals"] = mpt.vertex_normals(verts, faces)
    ms["normals"] = median_ms(torch, normals, a.repeats, a.inner)
    nbytes["normals"] = F * (12 + 3 * 12 + 9 * 8) + V * (24 + 12)
    def raster():
        box["depth"] = mvw.rasterize(verts, faces, views, H, W)["depth"]
    ms["raster"] = median_ms(torch, raster, a.repeats, 1)
    nrm, depth = box["normals"], box["depth"]
    acc = torch.zeros((V, 4), dtype=torch.float64, device=verts.device)
    def paint():
        lib.check(mpt.paint_raw(verts, nrm, mats, a.views, H, W, depth, images, None, acc, flags=0, **rules), "svs_mesh_paint")
    ms["paint"] = median_ms(torch, paint, a.repeats, a.inner)
    acc.zero_()
    paint()
    ref = {}
    def formulation():
        ref["acc"], ref["inside"], ref["used"] = torch_paint(torch, verts, nrm, mats, depth, images, **rules)
    ms["paint in torch ops"] = median_ms(torch, formulation, a.repeats, 1)
    inside, used = int(ref["inside"]), int(ref["used"])
    nbytes["paint"] = V * (12 + 12 + 32 + 32) + inside * 4 + used * 12
    scale = ref["acc"].abs().clamp(min=1e-300)
    agree = float(((acc - ref["acc"]).abs() / scale)[ref["acc"] != 0].max()) if used else 0.0
    same_support = bool(((acc == 0) == (ref["acc"] == 0)).all())
    def finish():
        box["colors"], box["painted"] = mpt.finish(acc)
    ms["finish"] = median_ms(torch, finish, a.repeats, a.inner)
    nbytes["finish"] = V * (32 + 3 + 4)
    colors0, painted0 = box["colors"].clone(), box["painted"].clone()
    rounds = {}
    def spread():
        c, q = colors0.clone(), painted0.clone()
        rounds["n"] = mpt.spread(faces, c, q)
        box["colors"], box["painted"] = c, q
    ms["spread"] = median_ms(torch, spread, a.repeats, 1)
    nbytes["spread"] = (rounds["n"] + 1) * (F * (12 + 12) + V * (16 + 16))
    def download():
        box["host"] = box["colors"].cpu().numpy(), box["painted"].cpu().numpy()
    ms["download"] = median_ms(torch, download, a.repeats, 1)
    nbytes["download"] = V * 7

    for k in ("normals", "raster", "paint", "finish", "spread", "download", "paint in torch ops"):
        lines.append(f"  {k:<19} {ms[k]:10.3f} ms" + (f"  {nbytes[k] / 1e6:9.1f} MB" if k in nbytes else ""))
    rate = nbytes["paint"] / (ms["paint"] * 1e-3)
    painted = box["host"][1]
    lines.append(f"  paint gathers {nbytes['paint'] / 1e6:.1f} MB ({V} vertices x 88 B of positions, normals and accumulators, {inside} (vertex, view) "
                 f"pairs inside an image x 4 B of depth, {used} contributing pairs x 12 B of taps) in {ms['paint']:.3f} ms = {rate / 1e12:.3f} TB/s = "
                 f"{100 * rate / HBM_ACHIEVABLE:.1f} % of the achievable HBM rate ({HBM_ACHIEVABLE / 1e12:.1f} TB/s)")
    lines.append(f"  the torch formulation takes {ms['paint in torch ops'] / ms['paint']:.1f} times the kernel's time; its accumulators agree with "
                 f"the kernel's to {agree:.1e} relative, zero in the same places: {same_support}")
    lines.append(f"  painted by a view: {int((painted == 1).sum())} vertices; filled in {rounds['n']} rounds: {int((painted > 1).sum())}; never "
                 f"reached: {int((painted == 0).sum())}")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
