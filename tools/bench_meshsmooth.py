#!/usr/bin/env python3
"""Times svs_hip.meshsmooth on a synthetic mesh (no dataset needed): the marching-cubes mesh of tools/bench_meshview.py (a
sphere and a floor at --resolution).

    python tools/bench_meshsmooth.py [--resolution 512 [48 ...]] [--repeats 7] [--out profiles/meshsmooth_bench.txt]

Per phase -- the adjacency build, one Taubin iteration (a lambda and a mu pass), one normal-filter pass, one vertex-update
pass -- the milliseconds (after one untimed call, the median and the spread of --repeats host-clock intervals that end in a
device synchronise), the bytes the phase has to move at the least (every array it reads or writes once; the sorts' passes
for the build) and the rate that makes, against a float4 copy timed in the same run; and the same pass formed with torch ops
(a directed-edge list and index_add_ in float64: float atomics, an order that changes from run to run).  Needs the GPU.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-volsdf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COPY_BYTES = 1 << 28                       # the float4 copy: 256 MiB read and as many written


def timed_ms(torch, fn, repeats):
    """-> (median, min, max) of `repeats` intervals after one untimed call"""
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def rows_of(torch, start):
    """the row of every entry of a compressed list"""
    n = start.shape[0] - 1
    return torch.repeat_interleave(torch.arange(n, device=start.device), (start[1:] - start[:-1]).to(torch.int64))


def torch_taubin_pass(torch, x, row, col, deg, move, s):
    m = torch.zeros_like(x).index_add_(0, row, x[col])
    return torch.where(move[:, None], x + s * (m / deg[:, None] - x), x)


def torch_visits(torch, faces, adj):
    """(f, g) for every face g a face f meets at one of its corners, g != f (an edge neighbour twice)"""
    vf = adj["vert_face"].to(torch.int64)
    row = rows_of(torch, adj["face_start"])                      # the vertex of every (vertex, face) entry
    deg = (adj["face_start"][1:] - adj["face_start"][:-1]).to(torch.int64)
    reps = deg[row]                                              # every entry meets its vertex's whole list
    f = torch.repeat_interleave(vf, reps)
    first = torch.repeat_interleave(adj["face_start"][:-1].to(torch.int64)[row], reps)
    begin = torch.cumsum(reps, 0) - reps
    g = vf[first + (torch.arange(f.shape[0], device=f.device) - torch.repeat_interleave(begin, reps))]
    keep = f != g
    return f[keep], g[keep]


def torch_normal_pass(torch, n, area, cent, vf, vg, rs, rn):
    d2 = ((cent[vg] - cent[vf]) ** 2).sum(1)
    q2 = ((n[vf] - n[vg]) ** 2).sum(1)
    a, b = 1 - d2 / (rs * rs), 1 - q2 / (rn * rn)
    w = torch.where((a > 0) & (b > 0), area[vg] * a * a * b * b, torch.zeros_like(a))
    s = (area[:, None] * n).index_add_(0, vf, w[:, None] * n[vg])
    return s / s.norm(dim=1, keepdim=True)


def torch_vertex_pass(torch, x, normals, faces64, row, vf, deg, move):
    P = x[faces64[vf]]
    d = ((P[:, 0] + P[:, 1]) + P[:, 2]) / 3.0 - x[row]
    nn = normals[vf]
    acc = torch.zeros_like(x).index_add_(0, row, nn * (nn * d).sum(1, keepdim=True))
    return torch.where(move[:, None], x + acc / deg[:, None], x)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--resolution", type=int, nargs="+", default=[512], help="one run per grid resolution")
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import torch
    import bench_meshview as bmv
    from svs_hip import lib, mesh, meshsmooth as sm, views

    text = "\n".join(bench(a, r, torch, bmv, lib, mesh, sm, views) for r in a.resolution)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def bench(a, resolution, torch, bmv, lib, mesh, sm, views):
    """one run -> its lines"""
    verts, faces = bmv.make_mesh(torch, mesh, resolution)
    verts, faces, _ = views.mesh_args(verts, faces)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    lines = [f"svs_hip.meshsmooth: marching cubes of a sphere and a floor at {resolution}^3 = {V} vertices, {F} faces; "
             f"warm-up, then the median (min .. max) of {a.repeats} intervals"]
    src = torch.empty(COPY_BYTES // 4, dtype=torch.float32, device=verts.device).normal_()
    dst = torch.empty_like(src)
    copy = timed_ms(torch, lambda: dst.copy_(src), a.repeats)
    copy_rate = 2 * COPY_BYTES / (copy[0] * 1e-3)
    lines.append(f"  float4 copy of {COPY_BYTES >> 20} MiB: {copy[0]:.3f} ms ({copy[1]:.3f} .. {copy[2]:.3f}) = {copy_rate / 1e12:.2f} TB/s")
    del src, dst
    box = {}

    ws = torch.empty(lib.load().svs_mesh_smooth_workspace_bytes(V, F), dtype=torch.uint8, device=verts.device)

    def build():
        box["adj"] = sm.adjacency_raw(verts, faces, ws)
    t = {"adjacency": timed_ms(torch, build, a.repeats)}
    adj = sm.adjacency(verts, faces)
    c = adj["counts"]
    E2, FV = 2 * c["edges"], c["valid_faces"]
    lines.append(f"  workspace {ws.numel() / 1e6:.1f} MB; {c['edges']} edges ({c['boundary_edges']} boundary, {c['nonmanifold_edges']} non-manifold), {FV} valid faces, mean valence "
                 f"{E2 / max(V, 1):.2f}, mean edge {adj['mean_edge']:.6f}")
    bits = max(V, 1).bit_length()
    pair_passes, corner_passes = (32 + bits + 7) // 8, (bits + 7) // 8
    nbytes = {"adjacency": F * (12 + 36 + 48 + 24 + 1) + pair_passes * 2 * 8 * 6 * F + corner_passes * 2 * 8 * 3 * F
              + 6 * F * (8 + 1) + 6 * F * (1 + 4) + 6 * F * (8 + 1 + 4) + E2 * 5 + (V + 1) * 8 + V * 4}
    rs, rn = 2.0 * adj["mean_edge"], 0.6
    x, tmp = sm._working(verts)
    x0 = x.clone()

    def taubin():
        sm.taubin_raw(x, tmp, adj, 1, 0.5, -0.53, sm.BOUNDARY_MODES["fixed"])
    t["taubin iteration"] = timed_ms(torch, taubin, a.repeats)
    nbytes["taubin iteration"] = 2 * (V * (24 + 24 + 4 + 4) + E2 * (4 + 1))
    x.copy_(x0)
    normals, areas, cent = sm.face_frames_raw(x, faces, adj)
    n0 = normals.clone()

    def nfilter():
        sm.normal_filter_raw(normals, areas, cent, faces, V, adj, 1, rs, rn)
    t["normal-filter pass"] = timed_ms(torch, nfilter, a.repeats)
    nbytes["normal-filter pass"] = F * (24 + 24 + 24 + 8 + 12 + 1) + (V + 1) * 4 + 3 * FV * 4
    normals.copy_(n0)
    sm.normal_filter_raw(normals, areas, cent, faces, V, adj, 1, rs, rn)
    n1 = normals.clone()

    def update():
        sm.vertex_update_raw(x, tmp, normals, faces, adj, 1, sm.BOUNDARY_MODES["fixed"])
    t["vertex-update pass"] = timed_ms(torch, update, a.repeats)
    nbytes["vertex-update pass"] = V * (24 + 24 + 4 + 4) + F * (12 + 24) + 3 * FV * 4
    # the same passes in torch ops; the lists they need are built outside the timed part
    flags = adj["flags"]
    move = ((flags & sm.USED) != 0) & ((flags & sm.BOUNDARY) == 0)
    row, col = rows_of(torch, adj["nbr_start"]), adj["nbr"].to(torch.int64)
    deg = (adj["nbr_start"][1:] - adj["nbr_start"][:-1]).to(torch.float64).clamp_(min=1)

    def torch_taubin():
        box["taubin"] = torch_taubin_pass(torch, torch_taubin_pass(torch, x0, row, col, deg, move, 0.5), row, col, deg, move, -0.53)
    tt = {"taubin iteration": timed_ms(torch, torch_taubin, a.repeats)}
    vf, vg = torch_visits(torch, faces, adj)

    def torch_nfilter():
        box["normals"] = torch_normal_pass(torch, n0, areas, cent, vf, vg, rs, rn)
    tt["normal-filter pass"] = timed_ms(torch, torch_nfilter, a.repeats)
    frow, fcol = rows_of(torch, adj["face_start"]), adj["vert_face"].to(torch.int64)
    fdeg = (adj["face_start"][1:] - adj["face_start"][:-1]).to(torch.float64).clamp_(min=1)
    faces64 = faces.to(torch.int64)

    def torch_update():
        box["update"] = torch_vertex_pass(torch, x0, n1, faces64, frow, fcol, fdeg, move)
    tt["vertex-update pass"] = timed_ms(torch, torch_update, a.repeats)
    # what the kernels gave for the same inputs, against the torch formulation (sums in another order: a rounding apart)
    x.copy_(x0)
    taubin()
    dev = {"taubin iteration": float((x - box["taubin"]).abs().max())}
    ok = adj["face_valid"] != 0
    dev["normal-filter pass"] = float((n1 - box["normals"])[ok].abs().max())
    x.copy_(x0)
    normals.copy_(n1)
    update()
    dev["vertex-update pass"] = float((x - box["update"]).abs().max())
    for k in ("adjacency", "taubin iteration", "normal-filter pass", "vertex-update pass"):
        m = t[k]
        rate = nbytes[k] / (m[0] * 1e-3)
        line = (f"  {k:<19} {m[0]:9.3f} ms ({m[1]:.3f} .. {m[2]:.3f})  {nbytes[k] / 1e6:8.1f} MB at the least = {rate / 1e12:.3f} TB/s = "
                f"{100 * rate / copy_rate:.1f} % of the copy's rate")
        if k in tt:
            line += (f"; torch ops {tt[k][0]:.3f} ms ({tt[k][1]:.3f} .. {tt[k][2]:.3f}) = {tt[k][0] / m[0]:.2f} times; largest difference "
                     f"{dev[k]:.2e}")
        lines.append(line)
    lines.append(f"  the build sorts {6 * F} directed pairs of 8 bytes in {pair_passes} passes and {3 * F} (vertex, face) pairs in "
                 f"{corner_passes}; {len(vf)} (face, face) visits per normal-filter pass")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
