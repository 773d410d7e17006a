#!/usr/bin/env python3
"""Times svs_hip.meshtexture on a synthetic mesh (no dataset needed): the marching-cubes mesh of tools/bench_meshpaint.py (a
sphere and a floor at --resolution) simplified to 10 % of its faces by svs_hip.meshsimplify, textured from 16 synthetic
1152x1536 photographs on a ring around it.

    python tools/bench_meshtexture.py [--resolution 512 48] [--size 4096 8192] [--views 16] [--out profiles/meshtexture_bench.txt]

Per phase: milliseconds after one untimed call -- the median and the range of 7 host-clock intervals that end in a device
synchronise -- for slots, uv, raster, bake, finish, one rendered view, the download and the PNG.  bake is svs_mesh_atlas_bake
alone on ready depth maps; beside it the bytes it must move at the least (acc read and written, the face data once), the
time of a float4 copy of as many bytes in the same run, and the time of the same gather written in torch ops on the same
texel points, whose accumulators are compared with the kernel's.  Needs the GPU.
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-volsdf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

REPEATS = 7


def timed(torch, fn, repeats=REPEATS):
    """-> (median, min, max) ms of `repeats` intervals after one untimed call"""
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


def texel_points(torch, verts, normals, faces, chart, slot_face, size, cell):
    """the atlas's texel points and unit normals in torch ops (what svs_mesh_atlas_bake works out per lane)
    -> flat texel index (N,), points (N,3), normals (N,3) float64"""
    n = size // cell
    n_slots = int(slot_face.shape[0])
    rows = ((n_slots + 1) // 2 + n - 1) // n * cell
    j, i = torch.meshgrid(torch.arange(rows, device=verts.device), torch.arange(size, device=verts.device), indexing="ij")
    qx, qy = i // cell, j // cell
    li, lj = i - qx * cell, j - qy * cell
    h = (li + lj > cell - 2).long()
    slot = 2 * (qy * n + qx) + h
    has = (i < n * cell) & (slot < n_slots)
    at = has.nonzero(as_tuple=True)
    slot, li, lj, h = slot[at], li[at].double(), lj[at].double(), h[at]
    f = slot_face[slot].long()
    r = (chart[f] & 3).long()
    tri = faces[f].long()
    idx = torch.stack([tri.gather(1, ((r + k) % 3)[:, None])[:, 0] for k in range(3)], 1)
    lo = h == 0
    b1 = torch.where(lo, (li - 1) / (cell - 5), ((cell - 2) - li) / (cell - 4))
    b2 = torch.where(lo, (lj - 1) / (cell - 5), ((cell - 2) - lj) / (cell - 4))
    b = torch.stack([1.0 - b1 - b2, b1, b2], 1).clamp(min=0.0)
    b = b / b.sum(1, keepdim=True)
    p = (b[:, :, None] * verts.double()[idx]).sum(1)
    m = (b[:, :, None] * normals.double()[idx]).sum(1)
    return at[0] * size + at[1], p, m / m.norm(dim=1, keepdim=True)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--resolution", type=int, nargs="+", default=[512, 48], help="one run per grid resolution")
    p.add_argument("--size", type=int, nargs="+", default=[4096, 8192], help="one run per atlas size")
    p.add_argument("--views", type=int, default=16)
    p.add_argument("--ratio", type=float, default=0.1, help="the share of its faces the mesh is simplified to")
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    text = "\n".join(bench(a, r, s) for r in a.resolution for s in a.size)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def bench(a, resolution, size):
    """one run -> its lines"""
    import numpy as np
    import torch
    from PIL import Image
    import bench_meshpaint as bmp
    import bench_meshview as bmv
    from svs_hip import lib, mesh, meshpaint, meshsimplify, meshtexture as mtx, meshview
    from svs_hip import views as svs_views
    if a.views > meshview.MAX_VIEWS:
        raise SystemExit(f"--views: at most {meshview.MAX_VIEWS} (one launch of svs_mesh_atlas_bake is what is timed)")
    H, W = bmv.H, bmv.W
    views = bmv.make_views(np, a.views)
    full_v, full_f = bmv.make_mesh(torch, mesh, resolution)
    verts, faces = meshsimplify.simplify(full_v, full_f, ratio=a.ratio)[:2]
    verts, faces, _ = svs_views.mesh_args(verts, faces)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    images = bmp.make_images(torch, a.views, H, W)
    mats = svs_views.mats(views, verts.device)
    rules = dict(near=1e-6, rel=0.01, abs_tol=0.0, cos_min=0.1, power=2)
    ms, box = {}, {}

    def slots():
        box["chart"], box["n"] = mtx.slots(verts, faces)
    ms["slots"] = timed(torch, slots)
    chart, n_slots = box["chart"], box["n"]
    cell = mtx.cell_for(n_slots, size)
    rows = mtx.rows_for(n_slots, size, cell)

    def uv():
        box["uv"], box["slot_face"] = mtx.layout(chart, n_slots, size, cell)
    ms["uv"] = timed(torch, uv)
    slot_face = box["slot_face"]
    normals = meshpaint.vertex_normals(verts, faces)
    colors = meshpaint.paint(verts, faces, views, images)[0]

    def raster():
        box["depth"] = meshview.rasterize(verts, faces, views, H, W)["depth"]
    ms["raster"] = timed(torch, raster)
    depth = box["depth"]
    acc = torch.zeros((rows, size, 4), dtype=torch.float64, device=verts.device)

    def bake():
        lib.check(mtx.bake_raw(verts, normals, faces, chart, slot_face, size, cell, mats, a.views, H, W, depth, images, None, acc,
                               flags=0, **rules), "svs_mesh_atlas_bake")
    ms["bake"] = timed(torch, bake)

    def bake_cell_major():
        lib.check(mtx.bake_raw(verts, normals, faces, chart, slot_face, size, cell, mats, a.views, H, W, depth, images, None, acc,
                               flags=lib.ATLAS_CELL_MAJOR, **rules), "svs_mesh_atlas_bake")
    ms["bake, cell-major"] = timed(torch, bake_cell_major)
    acc.zero_()
    bake_cell_major()
    by_cell = acc.clone()
    acc.zero_()
    bake()
    same_bytes = bool(torch.equal(acc.view(torch.int64), by_cell.view(torch.int64)))
    del by_cell

    def finish():
        box["atlas"], box["covered"] = mtx.finish(acc, faces, V, chart, slot_face, size, cell, colors)
    ms["finish"] = timed(torch, finish)
    atlas = box["atlas"]
    face1 = meshview.rasterize(verts, faces, views[:1], H, W)["face"]

    def render():
        box["rgb"] = mtx.render(verts, faces, chart, atlas, cell, views[:1], H, W, face=face1)[0]
    ms["render one view"] = timed(torch, render)

    def download():
        box["host"] = atlas.cpu().numpy()
    ms["download"] = timed(torch, download)
    with tempfile.TemporaryDirectory() as tmp:
        def png():
            Image.fromarray(box["host"]).save(os.path.join(tmp, "atlas.png"), compress_level=1)
        ms["png"] = timed(torch, png, 3)
        png_bytes = os.path.getsize(os.path.join(tmp, "atlas.png"))

    # the least bake must move: acc read and written, the face data (chart, slot_face, indices, corners, normals) once
    least = rows * size * 64 + n_slots * (4 + 4 + 12 + 36 + 36)
    src = torch.empty(least // 32 + 1, 4, dtype=torch.float32, device=verts.device)       # half read, half written
    dst = torch.empty_like(src)
    ms["float4 copy"] = timed(torch, lambda: dst.copy_(src))

    flat, pts, nrm = texel_points(torch, verts, normals, faces, chart, slot_face, size, cell)
    ref = {}

    def formulation():
        ref["acc"], ref["inside"], ref["used"] = bmp.torch_paint(torch, pts, nrm, mats, depth, images, **rules)
    ms["bake in torch ops"] = timed(torch, formulation, 3)
    got = acc.reshape(-1, 4)[flat]
    scale = ref["acc"].abs().clamp(min=1e-300)
    live = ref["acc"] != 0
    agree = float(((got - ref["acc"]).abs() / scale)[live].max()) if bool(live.any()) else 0.0
    same_support = bool(((got == 0) == (ref["acc"] == 0)).all())

    covered = box["covered"]
    lines = [f"svs_hip.meshtexture: marching cubes of a sphere and a floor at {resolution}^3 = {int(full_f.shape[0])} faces, simplified to "
             f"{F} faces ({V} vertices, {n_slots} valid); atlas {size} x {size}, cell {cell}, {rows} rows hold charts; {a.views} views of "
             f"{H} x {W}; warm-up, then median (min .. max) of {REPEATS} intervals"]
    for k in ("slots", "uv", "raster", "bake", "bake, cell-major", "finish", "render one view", "download", "png", "float4 copy", "bake in torch ops"):
        med, lo, hi = ms[k]
        lines.append(f"  {k:<19} {med:10.3f} ms  ({lo:.3f} .. {hi:.3f})")
    rate = least / (ms["bake"][0] * 1e-3)
    lines.append(f"  bake must move at least {least / 1e6:.1f} MB ({rows} x {size} texels x 64 B of accumulators read and written, {n_slots} "
                 f"faces x 92 B once) = {rate / 1e12:.3f} TB/s at its median; a float4 copy that moves as many bytes (half read, half written) takes "
                 f"{ms['float4 copy'][0]:.3f} ms: bake takes {ms['bake'][0] / ms['float4 copy'][0]:.1f} times that")
    lines.append(f"  lanes cell by cell instead of row by row: {ms['bake, cell-major'][0]:.3f} ms against {ms['bake'][0]:.3f} ms, the same bytes: "
                 f"{same_bytes}")
    lines.append(f"  the torch formulation takes {ms['bake in torch ops'][0] / ms['bake'][0]:.1f} times the kernel's time; its accumulators agree "
                 f"with the kernel's to {agree:.1e} relative, zero in the same places: {same_support}")
    lines.append(f"  texels baked from a view: {int((covered == 1).sum())}; from vertex colours: {int((covered == 2).sum())}; without a face: "
                 f"{int((covered == 0).sum())}; the PNG holds {png_bytes / 1e6:.1f} MB")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
