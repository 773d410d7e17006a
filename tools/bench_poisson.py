#!/usr/bin/env python3
"""Times svs_hip.poisson on a synthetic cloud (no dataset needed): --points seeded points on a sphere and a floor with exact
normals, meshed on a --resolution^3 grid.

    python tools/bench_poisson.py [--resolution 256 [512 ...]] [--points 5000000] [--repeats 7] [--out profiles/poisson_bench.txt]
    python tools/bench_poisson.py --resolution 256 --screen 4 --out profiles/poisson_screen_bench.txt

Per phase the milliseconds (after one untimed call, the median and the spread of --repeats host-clock intervals that end in a
device synchronise, as tools/bench_meshsimplify.py takes them): the sort alone (torch.sort of the same cell keys: the splat's
own sort is inside its entry point), the splat, divergence, the solve, sample, marching cubes, the trim, the colours and the
download.  For the solve: iterations, ms per iteration, the bytes an iteration moves as counted from csrc/svs_poisson.hip, and
that rate against a float4 copy measured in the same run; beside it the same recurrence written with torch slicing ops on
the device.  --screen S: after that the screened solve (`solve_screened`, W passed as field[3]) on the same right-hand side:
its iterations and ms per iteration beside the unscreened ones, its counted 56 B per node against the same copy, and its
recurrence in torch ops.  Needs the GPU.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-volsdf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HALF = 1.0                                 # the grid spans [-HALF, HALF]^3
TORCH_ITERATIONS = 50                      # the torch formulation is timed over this many iterations


def make_cloud(torch, n, seed=0):
    """60 % of the points on a sphere of radius 0.55 around (0, 0, 0.1), 40 % on the floor z = -0.6 below it, |x|, |y| <= 0.8 ->
    pts (n,3) float64, normals (n,3) float32, rgb (n,3) uint8 on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ns = int(0.6 * n)
    d = torch.randn(ns, 3, generator=g, device="cuda", dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    sphere = d * 0.55 + torch.tensor([0.0, 0.0, 0.1], dtype=torch.float64, device="cuda")
    xy = (torch.rand(n - ns, 2, generator=g, device="cuda", dtype=torch.float64) * 2 - 1) * 0.8
    floor = torch.cat([xy, torch.full((n - ns, 1), -0.6, dtype=torch.float64, device="cuda")], 1)
    up = torch.zeros(n - ns, 3, dtype=torch.float64, device="cuda")
    up[:, 2] = 1.0
    rgb = torch.randint(0, 256, (n, 3), generator=g, device="cuda", dtype=torch.uint8)
    return torch.cat([sphere, floor]).contiguous(), torch.cat([d, up]).float().contiguous(), rgb


def torch_apply(torch, x, inv_h2):
    s = torch.zeros_like(x)
    s[1:] += x[:-1]; s[:-1] += x[1:]
    s[:, 1:] += x[:, :-1]; s[:, :-1] += x[:, 1:]
    s[:, :, 1:] += x[:, :, :-1]; s[:, :, :-1] += x[:, :, 1:]
    return (6.0 * x - s) * inv_h2


def torch_cg(torch, rhs, h, iterations):
    """the recurrence of svs_poisson_cg in torch ops: float32 vectors, float64 dot products kept on the device, no host
    synchronisation -> x"""
    inv_h2 = 1.0 / (h * h)
    x = torch.zeros_like(rhs)
    r = rhs.clone()
    p = r.clone()
    rr = (r.double() * r.double()).sum()
    for _ in range(iterations):
        q = torch_apply(torch, p, inv_h2)
        alpha = rr / (p.double() * q.double()).sum()
        x += alpha.float() * p
        r -= alpha.float() * q
        rn = (r.double() * r.double()).sum()
        p = r + (rn / rr).float() * p
        rr = rn
    return x


def torch_pcg(torch, rhs, W, weight, h, iterations):
    """the recurrence of svs_screened_pcg in torch ops, as `torch_cg` does svs_poisson_cg's; z = r / d is a temporary -> x"""
    inv_h2 = 1.0 / (h * h)
    d = 6.0 * inv_h2 + weight * W
    x = torch.zeros_like(rhs)
    r = rhs.clone()
    p = r / d
    rz = (r.double() * p.double()).sum()
    for _ in range(iterations):
        q = torch_apply(torch, p, inv_h2) + (weight * W) * p
        alpha = rz / (p.double() * q.double()).sum()
        x += alpha.float() * p
        r -= alpha.float() * q
        z = r / d
        rzn = (r.double() * z.double()).sum()
        p = z + (rzn / rz).float() * p
        rz = rzn
    return x


def screened_lines(a, torch, timed_ms, ps, field, rhs, counted, h, nodes, per, copy_rate):
    """--screen S: the screened solve beside the unscreened one of the same run (per: its ms per iteration) -> lines"""
    box = {}
    weight, density = ps.screen_weight(field[3], counted, a.screen, h)

    def solve():
        box["x"], box["info"] = ps.solve_screened(rhs, field[3], weight, h)
    ms = timed_ms(torch, solve, a.repeats)
    info = box["info"]
    per_s = ms[0] / max(info["iterations"], 1)

    def in_torch():
        box["xt"] = torch_pcg(torch, rhs, field[3], weight, h, TORCH_ITERATIONS)
    per_torch = timed_ms(torch, in_torch, max(1, a.repeats // 2))[0] / TORCH_ITERATIONS
    ideal = 56 * nodes
    return [f"  screened solve, screen {a.screen:g} (weight {weight:.6g}, {density:.3f} points per touched node, W as field[3], "
            f"{'16-byte aligned' if field[3].data_ptr() % 16 == 0 else 'not 16-byte aligned'}): {ms[0]:10.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})",
            f"  screened: {info['iterations']} iterations to a recursive residual of {info['residual']:.3e} (converged: {info['converged']}), "
            f"{per_s:.4f} ms per iteration against {per:.4f} unscreened = {per_s / per:.3f} times; 56 / 44 of the unscreened time is {per * 56 / 44:.4f} ms",
            f"  a screened iteration moves {ideal / 1e6:.1f} MB (56 B per node: W once more in each of the three passes) = "
            f"{ideal / (per_s * 1e-3) / 1e12:.3f} TB/s = {100 * ideal / (per_s * 1e-3) / copy_rate:.1f} % of the float4 copy's rate",
            f"  the screened recurrence in torch ops: {per_torch:.4f} ms per iteration = {per_torch / per_s:.2f} times ours; its x after "
            f"{TORCH_ITERATIONS} iterations is finite: {bool(torch.isfinite(box['xt']).all())}"]


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--resolution", type=int, nargs="+", default=[256], help="one run per grid resolution")
    p.add_argument("--points", type=int, default=5000000)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--out", default=None)
    p.add_argument("--screen", type=float, default=None, metavar="S", help="also time the screened solve at this screen value, on the "
                                                                           "same cloud in the same run (no default value)")
    a = p.parse_args(argv)
    if a.screen is not None and not (a.screen > 0 and a.screen < float("inf")):
        p.error("--screen must be positive and finite")
    import numpy as np
    import torch
    from bench_meshsimplify import timed_ms
    from svs_hip import mesh, poisson as ps

    text = "\n".join(bench(a, r, np, torch, timed_ms, mesh, ps) for r in a.resolution)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def bench(a, resolution, np, torch, timed_ms, mesh, ps):
    """one run -> its lines"""
    pts, nrm, rgb = make_cloud(torch, a.points)
    n = int(pts.shape[0])
    dims = (resolution,) * 3
    nodes = resolution ** 3
    h = 2 * HALF / (resolution - 1)
    origin = np.full(3, -HALF)
    t0, t1, t2 = ps.stencil_tile()
    lines = [f"svs_hip.poisson: {n} points on a sphere and a floor into a {resolution}^3 grid = {nodes} nodes, voxel {h:.6f}; "
             f"warm-up, then the median (min .. max) of {a.repeats} intervals"]
    box, ms_ = {}, {}
    src = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    copy = timed_ms(torch, lambda: dst.copy_(src), a.repeats)
    copy_rate = 2 * src.numel() * 4 / (copy[0] * 1e-3)
    del src, dst
    keys = (torch.floor((pts - torch.as_tensor(origin, device="cuda")) / h).long().clamp_(0, resolution - 2)
            * torch.tensor([(resolution - 1) ** 2, resolution - 1, 1], device="cuda")).sum(1).int()
    ms_["sort alone (torch.sort)"] = timed_ms(torch, lambda: torch.sort(keys, stable=True), a.repeats)
    del keys

    def splat():
        box["field"], box["counted"], box["skipped"] = ps.splat(pts, nrm, dims, origin, h)
    ms_["splat (with its sort)"] = timed_ms(torch, splat, a.repeats)
    field = box["field"]

    def divergence():
        box["rhs"] = ps.divergence(field, h)
    ms_["divergence"] = timed_ms(torch, divergence, a.repeats)
    rhs = box["rhs"]

    def solve():
        box["x"], box["info"] = ps.solve(rhs, h)
    ms_["solve"] = timed_ms(torch, solve, a.repeats)
    x, info = box["x"], box["info"]

    def sample():
        box["level"] = ps.sample(x, pts, origin, h)[1]
    ms_["sample"] = timed_ms(torch, sample, a.repeats)
    level = box["level"]

    def cubes():
        box["mesh"] = mesh.marching_cubes(x, level, (h,) * 3, return_cells=True)
    ms_["marching cubes"] = timed_ms(torch, cubes, a.repeats)
    verts, faces, cells = box["mesh"]

    def trim():
        keep = ps.face_keep(field[3], cells, 2.0)
        box["trimmed"] = mesh.compact(verts, faces[keep.bool()])
    ms_["trim"] = timed_ms(torch, trim, a.repeats)
    tv, tf = box["trimmed"]
    world = (tv.double() + torch.as_tensor(origin, device="cuda")).contiguous()

    def colours():
        box["rgb"] = ps.nearest_colors(pts, rgb, world, h)
    ms_["colours"] = timed_ms(torch, colours, a.repeats)

    def download():
        box["host"] = (world.float().cpu().numpy(), tf.cpu().numpy(), box["rgb"].cpu().numpy())
    ms_["download"] = timed_ms(torch, download, a.repeats)

    def in_torch():
        box["xt"] = torch_cg(torch, rhs, h, TORCH_ITERATIONS)
    ms_[f"{TORCH_ITERATIONS} iterations in torch ops"] = timed_ms(torch, in_torch, max(1, a.repeats // 2))

    for k, m in ms_.items():
        lines.append(f"  {k:<28} {m[0]:10.3f} ms ({m[1]:.3f} .. {m[2]:.3f})")
    it = max(info["iterations"], 1)
    per = ms_["solve"][0] / it
    # per node and iteration: the stencil reads p once (plus the tile's halo: one row and column around t1 x t2 nodes, one
    # plane at either end of t0) and writes q; the axpys read x, p, r, q and write x, r; the direction update reads r, p and writes p
    halo = (t1 + 2) * (t2 + 2) / (t1 * t2) * (t0 + 2) / t0
    ideal, counted = 44 * nodes, (40 + 4 * halo) * nodes
    per_torch = ms_[f"{TORCH_ITERATIONS} iterations in torch ops"][0] / TORCH_ITERATIONS
    lines.append(f"  counted {box['counted']}, skipped {box['skipped']}; level {level:.6g}; faces {int(faces.shape[0])} -> {int(tf.shape[0])}, "
                 f"{int(tv.shape[0])} vertices")
    lines.append(f"  solve: {info['iterations']} iterations to a recursive residual of {info['residual']:.3e} (converged: {info['converged']}, "
                 f"tol 1e-4, max_iter {4 * resolution}), {per:.4f} ms per iteration, five launches each")
    lines.append(f"  an iteration moves {ideal / 1e6:.1f} MB (44 B per node; {counted / 1e6:.1f} MB with the stencil tile's halo, {halo:.3f} reads of "
                 f"p per node) = {ideal / (per * 1e-3) / 1e12:.3f} TB/s; a float4 copy of 2 x 256 MiB in this run: {copy[0]:.3f} ms = "
                 f"{copy_rate / 1e12:.3f} TB/s; the solve runs at {100 * ideal / (per * 1e-3) / copy_rate:.1f} % of the copy's rate")
    lines.append(f"  the same recurrence in torch slicing ops (float32 vectors, float64 dots, no host synchronisation): {per_torch:.4f} ms per "
                 f"iteration = {per_torch / per:.2f} times ours; its x after {TORCH_ITERATIONS} iterations is finite: {bool(torch.isfinite(box['xt']).all())}")
    if a.screen is not None:
        lines += screened_lines(a, torch, timed_ms, ps, field, rhs, box["counted"], h, nodes, per, copy_rate)
    return "\n".join(lines)


if __name__ == "__main__":
    main()
