#!/usr/bin/env python3
"""Times svs_hip.meshview on a synthetic mesh (no dataset needed): the marching-cubes mesh of an analytic sphere-plus-floor SDF
at --resolution, rendered into 16 synthetic 1152x1536 views on a ring around it.

    python tools/bench_meshview.py [--resolution 512 [48 ...]] [--views 16] [--repeats 3] [--out profiles/meshview_bench.txt]

Per phase: milliseconds (the median of --repeats, each a host-clock interval that ends in a device synchronise), launches and
the bytes the phase has to move.  raster small / raster large are the two paths of svs_mesh_raster alone (its flags 2 and 4:
the list is built in both), raster is the whole entry.  Beside them: the share of (view, face) pairs on each path, the
atomics actually issued (counted by a run under flag 1, which is not timed) and their byte rate beside the chip-wide rate of
global float atomics on an MI355X.  Needs the GPU.
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-volsdf_amd"))

ATOMIC_RATE = 1.3e12                       # bytes/s: global float atomic adds, chip-wide, on one MI355X
H, W = 1152, 1536
CENTRE, RADIUS, FLOOR = (0.013, -0.021, 0.007), 0.6, -0.62
HALF = 1.0                                 # the SDF grid spans [-HALF, HALF]^3


def look_at(np, eye):
    eye = np.asarray(eye, np.float64)
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    E = np.eye(4)
    E[:3, :3] = np.stack([right, np.cross(fwd, right), fwd])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def make_views(np, n):
    K = np.array([[1471.2, 0, 760.8], [0, 1461.6, 561.6], [0, 0, 1]])
    return [dict(K=K, E=look_at(np, (2.4 * np.cos(a), 2.4 * np.sin(a), 0.9 + 0.3 * np.sin(3 * a))))
            for a in 2 * np.pi * (np.arange(n) + 0.13) / n]


def make_mesh(torch, mesh, resolution):
    """the zero set of min(|p - c| - r, p.z - floor) on a resolution^3 grid over [-HALF, HALF]^3 -> verts, faces on the device"""
    ax = torch.linspace(-HALF, HALF, resolution, device="cuda")
    x, y, z = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    sdf = torch.minimum(torch.sqrt((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2 + (z - CENTRE[2]) ** 2) - RADIUS,
                        (z - FLOOR).expand(resolution, resolution, resolution)).contiguous()
    sp = 2 * HALF / (resolution - 1)
    verts, faces = mesh.marching_cubes(sdf, 0.0, (sp, sp, sp))
    return (verts - HALF).contiguous(), faces


def median_ms(torch, fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)[len(out) // 2]


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--resolution", type=int, nargs="+", default=[512], help="one run per grid resolution")
    p.add_argument("--views", type=int, default=16)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    from datasets.data_io import save_pfm
    from svs_hip import mesh, meshview as mvw

    text = "\n".join(bench(a, r, np, torch, Image, save_pfm, mesh, mvw) for r in a.resolution)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def bench(a, resolution, np, torch, Image, save_pfm, mesh, mvw):
    """one run -> its lines"""
    from svs_hip import views as svs_views
    views = make_views(np, a.views)
    verts, faces = make_mesh(torch, mesh, resolution)
    n_verts, n_faces = int(verts.shape[0]), int(faces.shape[0])
    host_v, host_f = verts.cpu().numpy(), faces.cpu().numpy()
    rng = np.random.default_rng(0)
    host_c = rng.integers(0, 256, (n_verts, 3)).astype(np.uint8)
    lines = [f"svs_hip.meshview: marching cubes of a sphere and a floor at {resolution}^3 = {n_verts} vertices, {n_faces} faces; "
             f"{a.views} views of {H} x {W}; median of {a.repeats}"]
    ms, nbytes, launches = {}, {}, {}

    box = {}
    def upload():
        box["v"], box["f"], box["c"] = svs_views.mesh_args(host_v, host_f, host_c)
    ms["upload"] = median_ms(torch, upload, a.repeats)
    nbytes["upload"] = host_v.nbytes + host_f.nbytes + host_c.nbytes
    v_d, f_d, c_d = box["v"], box["f"], box["c"]
    mats = svs_views.mats(views, v_d.device)
    n_chunks = (n_faces + mvw.FACE_CHUNK - 1) // mvw.FACE_CHUNK
    zbuf = mvw.new_zbuf(a.views, H, W)
    for name, flags in (("raster small", mvw.FLAG_SMALL_ONLY), ("raster large", mvw.FLAG_LARGE_ONLY), ("raster", 0)):
        def run(flags=flags):
            zbuf.fill_(-1)
            mvw.raster_into(zbuf, v_d, f_d, mats, flags=flags)
        fill = median_ms(torch, lambda: zbuf.fill_(-1), a.repeats)
        ms[name] = median_ms(torch, run, a.repeats) - fill
        launches[name] = n_chunks
    counts = {}
    zbuf.fill_(-1)
    mvw.raster_into(zbuf, v_d, f_d, mats, flags=mvw.FLAG_COUNT, stats=counts)
    zbuf.fill_(-1)
    mvw.raster_into(zbuf, v_d, f_d, mats)
    nbytes["raster"] = a.views * (host_f.nbytes + 3 * 12 * n_faces) + 8 * counts["atomics"]
    res = {}
    def resolve():
        res.update(mvw.resolve(zbuf, v_d, f_d, mats, colors=c_d, normals=True, shade=True))
    ms["resolve"] = median_ms(torch, resolve, a.repeats)
    nbytes["resolve"] = a.views * H * W * (8 + 4 + 4 + 12 + 3)
    launches["resolve"] = 1
    vis = {}
    def visibility():
        vis["seen"], vis["off"] = mvw.visibility(v_d, views, res["depth"])
    ms["visibility"] = median_ms(torch, visibility, a.repeats)
    nbytes["visibility"] = host_v.nbytes + 8 * n_verts + 4 * a.views * n_verts
    launches["visibility"] = (a.views + mvw.MAX_VIEWS - 1) // mvw.MAX_VIEWS
    down = {}
    def download():
        down["depth"], down["shade"] = res["depth"].cpu().numpy(), res["shade"].cpu().numpy()
    ms["download"] = median_ms(torch, download, a.repeats)
    nbytes["download"] = a.views * H * W * 7
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        for i in range(a.views):
            save_pfm(os.path.join(tmp, f"{i:08}.pfm"), down["depth"][i])
            Image.fromarray(down["shade"][i]).save(os.path.join(tmp, f"{i:08}.png"), compress_level=1)
        ms["file writing"] = (time.perf_counter() - t0) * 1e3
        nbytes["file writing"] = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))

    for k in ("upload", "raster small", "raster large", "raster", "resolve", "visibility", "download", "file writing"):
        lines.append(f"  {k:<13} {ms[k]:9.3f} ms" + (f"  {launches[k]} entry calls" if k in launches else "")
                     + (f"  {nbytes[k] / 1e6:9.1f} MB" if k in nbytes else ""))
    pairs = a.views * n_faces
    drawn = counts["large"] + counts["small"]
    covered = int((res["depth"] > 0).sum())
    lines.append(f"  (view, face) pairs {pairs}: {counts['small']} walked by their lane ({counts['small'] / pairs:.1%}), {counts['large']} "
                 f"through the list ({counts['large'] / pairs:.2%}), {pairs - drawn} skipped or without a pixel ({1 - drawn / pairs:.1%})")
    rate = 8 * counts["atomics"] / (ms["raster"] * 1e-3)
    lines.append(f"  atomics issued (counted): {counts['atomics']} for {covered} covered pixels ({counts['atomics'] / max(covered, 1):.2f} per "
                 f"covered pixel); {8 * counts['atomics'] / 1e6:.1f} MB of 64-bit minima in {ms['raster']:.3f} ms = {rate / 1e9:.1f} GB/s, "
                 f"{rate / ATOMIC_RATE:.1%} of the {ATOMIC_RATE / 1e12:.1f} TB/s chip-wide rate of global float atomics")
    lines.append(f"  visible from at least one view: {float((vis['seen'] > 0).float().mean()):.3f} of the vertices")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
