#!/usr/bin/env python3
"""Times svs_hip.tsdf on a synthetic scan (no dataset needed): three 1152x1536 views of a sphere, a 400^3 volume.

    python tools/bench_tsdf.py [--resolution 400] [--repeats 5] [--out profiles/tsdf_bench.txt]

Per phase: milliseconds and the bytes the algorithm has to move, computed from the shapes and the observed voxel count.
integrate is timed with device events around Volume.integrate (the upload of 63 doubles of camera matrices and the one
launch; the median of --repeats calls into one volume: every launch reads and writes the same voxels); the other phases are host-clock intervals that end in a device synchronise,
torch's scans and indexing included.  Beside integrate: its volume traffic against the achievable HBM rate, the same
launch with one view and without colours (what the time follows: bytes or views), and the same integration written in
torch ops on the same device.  Needs the GPU.
"""
import argparse
import os
import sys
import tempfile
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-volsdf_amd"))

HBM_ACHIEVABLE = 6.3e12                    # bytes/s: a float4 copy on one MI355X (8 TB/s is the specification)
H, W = 1152, 1536
CENTRE, RADIUS = (0.07, -0.04, 0.11), 0.5
EYES = ((2.03, 0.31, 0.42), (1.9, 0.62, 0.5), (1.95, 0.0, 0.28))


def look_at(np, eye):
    eye = np.asarray(eye, np.float64)
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    E = np.eye(4)
    E[:3, :3] = np.stack([right, np.cross(fwd, right), fwd])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def make_views(np):
    """host arrays, as a scan's files deliver them: K, E, depth (camera z of the first hit, 0 on a miss), img"""
    K = np.array([[1471.2, 0, 760.8], [0, 1461.6, 561.6], [0, 0, 1]])
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T
    views = []
    for eye in EYES:
        E = look_at(np, eye)
        c = E[:3, :3] @ np.asarray(CENTRE) + E[:3, 3]
        a, b = (rays * rays).sum(-1), rays @ c
        disc = b * b - a * (c @ c - RADIUS * RADIUS)
        s = (b - np.sqrt(np.maximum(disc, 0.0))) / a
        depth = np.where((disc > 0) & (s > 0), s, 0.0).astype(np.float32)
        world = (rays * depth[..., None] - E[:3, 3]) @ E[:3, :3]
        img = np.clip(0.5 + 0.8 * (world - np.asarray(CENTRE)), 0, 1).astype(np.float32)
        views.append(dict(K=K, E=E, depth=depth, img=img))
    return views


def torch_integrate(torch, vol, views, slabs=50):
    """svs_tsdf_integrate's arithmetic in torch ops (float64), a slab of the first axis at a time, in place on vol's arrays"""
    dev = vol.tsdf.device
    n0, n1, n2 = vol.shape
    o = torch.as_tensor(vol.origin, dtype=torch.float64, device=dev)
    j, k = torch.arange(n1, dtype=torch.float64, device=dev), torch.arange(n2, dtype=torch.float64, device=dev)
    step = (n0 + slabs - 1) // slabs
    for i0 in range(0, n0, step):
        i1 = min(n0, i0 + step)
        i = torch.arange(i0, i1, dtype=torch.float64, device=dev)
        px, py, pz = (o[0] + i * vol.voxel)[:, None, None], (o[1] + j * vol.voxel)[None, :, None], (o[2] + k * vol.voxel)[None, None, :]
        st = torch.zeros(i1 - i0, n1, n2, dtype=torch.float64, device=dev)
        sn = torch.zeros_like(st)
        sc = torch.zeros(3, i1 - i0, n1, n2, dtype=torch.float64, device=dev)
        for v in views:
            E, K = (torch.as_tensor(v[m], dtype=torch.float64, device=dev) for m in ("E", "K"))
            cx = E[0, 0] * px + E[0, 1] * py + E[0, 2] * pz + E[0, 3]
            cy = E[1, 0] * px + E[1, 1] * py + E[1, 2] * pz + E[1, 3]
            cz = E[2, 0] * px + E[2, 1] * py + E[2, 2] * pz + E[2, 3]
            qz = K[2, 0] * cx + K[2, 1] * cy + K[2, 2] * cz
            fu = torch.floor((K[0, 0] * cx + K[0, 1] * cy + K[0, 2] * cz) / qz + 0.5)
            fv = torch.floor((K[1, 0] * cx + K[1, 1] * cy + K[1, 2] * cz) / qz + 0.5)
            ok = (cz > 0) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            pix = torch.where(ok, fv * W + fu, torch.zeros_like(fu)).long()
            d = v["depth_d"].reshape(-1)[pix]
            ok &= torch.isfinite(d) & (d > 0)
            sdf = d.double() - cz
            ok &= sdf >= -vol.trunc
            st += torch.where(ok, torch.clamp(sdf / vol.trunc, max=1.0), torch.zeros_like(sdf))
            sn += ok
            col = v["img_d"].reshape(-1, 3)[pix.reshape(-1)].double().reshape(pix.shape + (3,))
            sc += torch.where(ok[None], col.permute(3, 0, 1, 2), torch.zeros_like(sc))
        seen = sn > 0
        w_old = vol.weight[i0:i1].double()
        w_new = w_old + sn
        vol.tsdf[i0:i1] = torch.where(seen, (w_old * vol.tsdf[i0:i1].double() + st) / w_new, vol.tsdf[i0:i1].double()).float()
        vol.rgb[:, i0:i1] = torch.where(seen[None], (w_old[None] * vol.rgb[:, i0:i1].double() + sc) / w_new[None],
                                        vol.rgb[:, i0:i1].double()).float()
        vol.weight[i0:i1] = torch.where(seen, w_new, w_old).float()


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--resolution", type=int, default=400)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import numpy as np
    import torch
    from svs_hip import mesh, ply, tsdf
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf needs the GPU")
    n = a.resolution
    voxel = 1.6 / n
    origin = np.asarray(CENTRE) - voxel * (n - 1) / 2
    shape = (n, n, n)
    host_views = make_views(np)

    def sync_ms(t0):
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def event_ms(fn, repeats):
        times = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return float(np.median(times)), times

    ms = OrderedDict()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    views = [dict(v, depth=torch.from_numpy(v["depth"]).cuda(), img=torch.from_numpy(v["img"]).cuda()) for v in host_views]
    ms["upload"] = sync_ms(t0)
    up_bytes = sum(v["depth"].nbytes + v["img"].nbytes for v in host_views)

    for k in tsdf.ENTRY_CALLS:
        tsdf.ENTRY_CALLS[k] = 0
    vol = tsdf.Volume(origin, shape, voxel)
    vol.integrate(views)                                                    # warm-up; the volume now holds one pass
    ms["integrate"], spread = event_ms(lambda: vol.integrate(views), a.repeats)
    launches_per_call = vol.launches // (a.repeats + 1)
    observed = int((vol.weight > 0).sum())
    total = n ** 3
    # variants that show what the time follows
    one_view, _ = event_ms(lambda: vol.integrate(views[:1]), a.repeats)
    plain = tsdf.Volume(origin, shape, voxel, colors=False)
    plain.integrate(views)
    no_color, _ = event_ms(lambda: plain.integrate(views), a.repeats)
    single = tsdf.Volume(origin, shape, voxel)
    single.integrate(views[:1])
    observed_one = int((single.weight > 0).sum())
    # every voxel in front of the surface: a constant depth behind the volume, so that almost all voxels are observed
    far_views = [dict(v, depth=torch.full_like(v["depth"], 10.0)) for v in views]
    dense = tsdf.Volume(origin, shape, voxel)
    dense.integrate(far_views)
    dense_ms, _ = event_ms(lambda: dense.integrate(far_views), a.repeats)
    observed_dense = int((dense.weight > 0).sum())
    del plain, single, dense, far_views

    # the product path once, on a fresh volume, with the phases of Volume.mesh
    vol = tsdf.Volume(origin, shape, voxel)
    vol.integrate(views)
    for rep in range(2):                                                    # the second of two runs
        for k in mesh.ENTRY_CALLS:
            mesh.ENTRY_CALLS[k] = 0
        sec = OrderedDict()
        verts, faces, rgb = vol.mesh(timers=sec)
    ws = sec.pop("workspace_bytes", 0)
    for k in ("scan", "classify", "emit", "keep", "colors"):
        ms[k] = sec.get(k, 0.0) * 1e3
    t0 = time.perf_counter()
    v, f, c = verts.cpu().numpy(), faces.cpu().numpy(), rgb.cpu().numpy()
    ms["download"] = sync_ms(t0)
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        ply.write(os.path.join(tmp, "tsdf.ply"), v, c, f)
        ms["write"] = (time.perf_counter() - t0) * 1e3
        file_bytes = os.path.getsize(os.path.join(tmp, "tsdf.ply"))

    # the same integration in torch ops, against the kernel's volume
    for d in views:
        d["depth_d"], d["img_d"] = d["depth"], d["img"]
    ref = tsdf.Volume(origin, shape, voxel)
    torch_integrate(torch, ref, views)                                      # warm-up (allocator, kernels)
    torch.cuda.synchronize()
    ref = tsdf.Volume(origin, shape, voxel)
    t0 = time.perf_counter()
    torch_integrate(torch, ref, views)
    torch_ms = sync_ms(t0)
    same_w = int((ref.weight != vol.weight).sum())
    diff = float((ref.tsdf - vol.tsdf).abs().max())
    diff_c = float((ref.rgb - vol.rgb).abs().max())

    moved = {"upload": up_bytes, "integrate": 40 * observed, "classify": 6 * total,
             "emit": 12 * verts.shape[0] + 12 * (faces.shape[0]), "download": 15 * len(v) + 12 * len(f), "write": file_bytes}
    lines = [f"svs_hip.tsdf, three {H}x{W} views of a sphere, volume {n}^3 = {total} voxels, voxel {voxel:.6f}, trunc {vol.trunc:.6f}",
             f"observed voxels {observed} ({100.0 * observed / total:.1f} %); mesh {len(v)} vertices, {len(f)} faces",
             f"C entry points: integrate {launches_per_call} launch per call of 3 views; Volume.mesh: classify 1, emit 1, keep 1, colours 1 "
             f"(svs_hip.mesh counts {dict((k, c) for k, c in mesh.ENTRY_CALLS.items() if c)})"]
    for k, t in ms.items():
        extra = f"  {moved[k] / 1e6:10.1f} MB" if k in moved else ""
        lines.append(f"  {k:<10s} {t:10.3f} ms{extra}")
    rate = moved["integrate"] / (ms["integrate"] * 1e-3)
    lines += [
        f"integrate, device events, {a.repeats} launches: " + ", ".join(f"{t:.3f}" for t in spread) + " ms",
        f"  volume traffic of the observed voxels: 40 B x {observed} = {moved['integrate'] / 1e6:.1f} MB (20 B read, 20 B written; "
        f"unobserved groups of four are neither read nor written; the whole volume would be {40 * total / 1e6:.1f} MB)",
        f"  -> {rate / 1e12:.3f} TB/s = {100 * rate / HBM_ACHIEVABLE:.1f} % of the achievable HBM rate ({HBM_ACHIEVABLE / 1e12:.1f} TB/s); "
        f"at that rate the bytes alone take {moved['integrate'] / HBM_ACHIEVABLE * 1e3:.3f} ms",
        f"  the same launch with one view: {one_view:.3f} ms ({observed_one} voxels observed by that view, "
        f"{40 * observed_one / 1e6:.1f} MB); three views without colours: {no_color:.3f} ms ({16 * observed / 1e6:.1f} MB)",
        f"  projections: {3.0 * total / (ms['integrate'] * 1e-3) / 1e9:.1f} G (voxel, view) pairs per second over all {total} voxels x 3 views",
        f"  the same three cameras with a constant depth of 10 (every voxel inside a view is observed): {dense_ms:.3f} ms, "
        f"{observed_dense} voxels = {40 * observed_dense / 1e6:.1f} MB -> {40 * observed_dense / (dense_ms * 1e-3) / 1e12:.3f} TB/s = "
        f"{100 * 40 * observed_dense / (dense_ms * 1e-3) / HBM_ACHIEVABLE:.1f} % of the achievable HBM rate",
        f"the same integration in torch ops (float64, 50 slabs, host clock, one pass): {torch_ms:.1f} ms = "
        f"{torch_ms / ms['integrate']:.0f} x the kernel; against the kernel's volume: {same_w} weights differ, "
        f"max |tsdf| difference {diff:.3g}, max colour difference {diff_c:.3g}",
        f"peak memory allocated inside marching_cubes: {ws / 1e6:.1f} MB",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
