#!/usr/bin/env python3
"""Times svs_hip.meshsimplify on a synthetic mesh (no dataset needed): the marching-cubes mesh of tools/bench_meshview.py (a
sphere and a floor at --resolution), simplified to 10 % and to 1 % of its faces.

    python tools/bench_meshsimplify.py [--resolution 512 [48 ...]] [--ratios 0.1 0.01] [--repeats 7] [--out profiles/meshsimplify_bench.txt]

Per target: the search for the cell size (16 tries of the two cheap passes), then per phase at that cell size the
milliseconds (after one untimed call, the median and the spread of --repeats host-clock intervals that end in a device
synchronise), the bytes the phase has to move at the least, and the entry points called.  Beside the solve phase: its counted
traffic against the achievable HBM rate tools/bench_tsdf.py uses, and the time of the same per-cell sums formed with torch ops
(float64 terms per (face, corner) pair, one index_add_ into the cells).  Last, what the simplification cost:
`meshsimplify.distance` between the two surfaces in units of the voxel.  Needs the GPU.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-volsdf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_ACHIEVABLE = 6.3e12                    # bytes/s: a float4 copy on one MI355X (tools/bench_tsdf.py)


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


def torch_sums(torch, verts, faces, vert_cell, n_cells, origin, h):
    """the 13 float64 sums per cell of svs_mesh_cluster_solve in torch ops (every face taken as valid) -> (n_cells,13)"""
    v = verts.to(torch.float64)
    f = faces.to(torch.int64)
    P = v[f]                                                   # (F,3,3)
    n = torch.linalg.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    L = n.norm(dim=1)
    ok = L > 0
    P, n, L, f = P[ok], n[ok], L[ok], f[ok]
    o = torch.as_tensor(origin, dtype=torch.float64, device=v.device)
    sums = torch.zeros((n_cells, 13), dtype=torch.float64, device=v.device)
    for k in range(3):
        c = o + (torch.floor((P[:, k] - o) * (1.0 / h)) + 0.5) * h
        d = -(n * (P[:, 0] - c)).sum(1)
        terms = torch.stack([n[:, 0] * n[:, 0] / L, n[:, 0] * n[:, 1] / L, n[:, 0] * n[:, 2] / L, n[:, 1] * n[:, 1] / L, n[:, 1] * n[:, 2] / L,
                             n[:, 2] * n[:, 2] / L, n[:, 0] * d / L, n[:, 1] * d / L, n[:, 2] * d / L, d * d / L,
                             P[:, k, 0] - c[:, 0], P[:, k, 1] - c[:, 1], P[:, k, 2] - c[:, 2]], 1)
        sums.index_add_(0, vert_cell[f[:, k]].to(torch.int64), terms)
    return sums


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--resolution", type=int, nargs="+", default=[512], help="one run per grid resolution")
    p.add_argument("--ratios", type=float, nargs="+", default=[0.1, 0.01])
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import numpy as np
    import torch
    import bench_meshview as bmv
    from svs_hip import lib, mesh, meshsimplify as ms, views

    text = "\n".join(bench(a, r, np, torch, bmv, lib, mesh, ms, views) for r in a.resolution)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def bench(a, resolution, np, torch, bmv, lib, mesh, ms, views):
    """one run -> its lines"""
    verts, faces = bmv.make_mesh(torch, mesh, resolution)
    verts, faces, _ = views.mesh_args(verts, faces)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    voxel = 2 * bmv.HALF / (resolution - 1)
    lines = [f"svs_hip.meshsimplify: marching cubes of a sphere and a floor at {resolution}^3 = {V} vertices, {F} faces, voxel {voxel:.6f}; "
             f"warm-up, then the median (min .. max) of {a.repeats} intervals"]
    ws = ms._workspace(verts, faces)
    host_v, host_f = verts.cpu().numpy(), faces.cpu().numpy()
    for ratio in a.ratios:
        box = {}
        def search():
            box["out"] = ms.simplify(verts, faces, ratio=ratio, return_info=True)
        calls = dict(ms.ENTRY_CALLS)
        t_search = timed_ms(torch, search, max(1, a.repeats // 2))
        per_search = {k: (ms.ENTRY_CALLS[k] - calls[k]) // (max(1, a.repeats // 2) + 1) for k in calls}
        info = box["out"][-1]
        h, origin = info["cell"], info["origin"]
        new_v, new_f = box["out"][0], box["out"][1]
        C, M = int(new_v.shape[0]), int(new_f.shape[0])
        lines.append(f" ratio {ratio}: cell {h:.6f} = {h / voxel:.2f} voxels after {len(info['tried'])} tries -> {C} vertices, {M} faces "
                     f"({100.0 * M / F:.2f} % of the faces)")
        ms_, nbytes = {}, {}
        def cells():
            box["cells"] = ms.cells_raw(verts, faces, origin, h, ws)
        ms_["cells"] = timed_ms(torch, cells, a.repeats)
        vert_cell, n_cells = box["cells"]
        # faces read with their corners, one byte marked per corner; keys and indices written, sorted (8 passes of 8 bits), scanned
        nbytes["cells"] = F * (12 + 36 + 3) + V * (1 + 12 + 12) + 8 * 2 * 12 * V + V * (12 + 1 + 4 + 4 + 4)
        out_v = torch.empty((n_cells, 3), dtype=torch.float32, device=verts.device)
        out_i = torch.empty(n_cells, dtype=torch.int32, device=verts.device)
        out_e = torch.empty(n_cells, dtype=torch.float64, device=verts.device)
        org = ms._host_origin(origin)
        def solve():
            lib.check(lib.load().svs_mesh_cluster_solve(ms._ptr(verts), V, ms._ptr(faces), F, None, org, h, 1e-3, ms._ptr(vert_cell), n_cells,
                                                        ms._ptr(ws), ms._ptr(out_v), None, ms._ptr(out_i), ms._ptr(out_e), ms._stream()),
                      "svs_mesh_cluster_solve")
        ms_["solve"] = timed_ms(torch, solve, a.repeats)
        pairs = 3 * F
        segs = pairs // 64 + n_cells
        passes = (max(n_cells, 1).bit_length() + 7) // 8
        # pair keys (faces, corners, ranks; 8 B per pair out), the sort's passes, runs and segment flags and their scan, the
        # gather of every pair's face (4 + 12 + 36 B), segment sums out and in, the cells' outputs
        nbytes["solve"] = (F * (12 + 36 + 12) + pairs * 8) + passes * 2 * 8 * pairs + pairs * (4 + 1 + 1 + 4 + 4) \
            + pairs * (4 + 12 + 36) + 2 * 128 * segs + n_cells * (12 + 4 + 8 + 16)
        def count():
            box["count"] = ms.faces_count_raw(verts, faces, vert_cell, n_cells, ws)
            box["n"] = int(box["count"][2].item())
        ms_["faces"] = timed_ms(torch, count, a.repeats)
        key_passes = (42 + max(n_cells, 1).bit_length() + 7) // 8
        nbytes["faces"] = F * (12 + 36 + 12 + 12) + key_passes * 2 * 12 * F + F * (12 + 1 + 1 + 4) + M * 12
        def sums():
            box["sums"] = torch_sums(torch, verts, faces, vert_cell, n_cells, origin, h)
        ms_["sums in torch ops"] = timed_ms(torch, sums, max(1, a.repeats // 2))
        lines.append(f"  {'search':<19} {t_search[0]:10.3f} ms ({t_search[1]:.3f} .. {t_search[2]:.3f})  entry calls "
                     + ", ".join(f"{k} {v}" for k, v in per_search.items()))
        for k in ("cells", "solve", "faces", "sums in torch ops"):
            m = ms_[k]
            lines.append(f"  {k:<19} {m[0]:10.3f} ms ({m[1]:.3f} .. {m[2]:.3f})" + (f"  {nbytes[k] / 1e6:9.1f} MB" if k in nbytes else ""))
        rate = nbytes["solve"] / (ms_["solve"][0] * 1e-3)
        lines.append(f"  solve moves at least {nbytes['solve'] / 1e6:.1f} MB ({pairs} pairs, {passes} sort passes, at most {segs} segments, {n_cells} "
                     f"cells) in {ms_['solve'][0]:.3f} ms = {rate / 1e12:.3f} TB/s = {100 * rate / HBM_ACHIEVABLE:.1f} % of the achievable HBM "
                     f"rate ({HBM_ACHIEVABLE / 1e12:.1f} TB/s)")
        codes = out_i.cpu().numpy()
        finite = bool(torch.isfinite(box["sums"]).all())
        lines.append(f"  the torch formulation of the sums alone (no sort, no solve; float64 atomics, an order that changes from run to run) "
                     f"takes {ms_['sums in torch ops'][0] / ms_['solve'][0]:.2f} times the solve phase's time; all finite: {finite}")
        lines.append(f"  cells by rank 0..3: {np.bincount(codes & 3, minlength=4).tolist()}, fallbacks {int((codes >> 2).sum())}")
        t0 = time.perf_counter()
        d = ms.distance(host_v, host_f, new_v, new_f, voxel)
        lines.append(f"  distance (sampled {voxel:.6f} apart: {d['samples_a']} and {d['samples_b']} points, {time.perf_counter() - t0:.1f} s): in -> out mean "
                     f"{d['a_to_b_mean'] / voxel:.3f} max {d['a_to_b_max'] / voxel:.3f} voxels, out -> in mean {d['b_to_a_mean'] / voxel:.3f} max "
                     f"{d['b_to_a_max'] / voxel:.3f} voxels; the cell is {h / voxel:.2f} voxels")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
