"""A triangle mesh made smaller on the HIP path (csrc/svs_meshsimplify.hip): vertex clustering with quadric error metrics.

    python -m svs_hip.meshsimplify --ply exps_mvs/tsdf/mvsnet106_l3.ply --ply-out small.ply (--cell H | --faces N | --ratio R) \\
        [--tol T] [--report]

A marching-cubes mesh (`svs_hip.mesh`, `svs_hip.tsdf`) has one vertex per crossed grid edge: its density is set by the voxel,
not by the shape.  Here the vertices inside a cell of a uniform grid become one vertex, placed where the planes of the
faces that touch the cell meet best (Lindstrom, "Out-of-core simplification of large polygonal models", 2000); faces that
collapse or repeat are dropped.  No priority queue, no serial collapses, one fixed order of every sum: the same bytes in
every run.

OURS throughout: the reference has no such step.  The arithmetic is fixed in include/svolsdf_hip.h and restated in float64
in tests/meshsimplify_oracle.py.

    cluster(verts, faces, cell, ...)            one cell size -> (verts, faces[, colors][, info])
    simplify(verts, faces, cell= | target_faces= | ratio=, ...)   a cell size, or a search for one that meets a face count
    distance(verts_a, faces_a, verts_b, faces_b, thresh)           what the simplification cost: one-sided surface distances
    simplify_ply(ply_in, ply_out, ...)          files in and out; what the command line runs
"""
import argparse
import ctypes
import math
import time
from collections import OrderedDict

import numpy as np
import torch

from . import clouds
from . import lib as _lib
from . import ply as _ply
from .images import seconds_line, tick
from .ops import _ptr, _stream
from .views import launches_since, mesh_args

MAX_CELLS_PER_AXIS = 1 << 21
ENTRY_CALLS = {"cells": 0, "solve": 0, "faces_count": 0, "faces_emit": 0}   # C entry points called, not kernels
PHASES = ("read", "upload", "search", "cells", "solve", "faces", "download", "write", "report")


def _host_origin(origin):
    return (ctypes.c_double * 3)(*[float(v) for v in np.asarray(origin, np.float64).reshape(3)])


def default_origin(verts, cell):
    """The cloud operators' origin rule (the box of `svs_cloud_bounds` less 1e-6) over the finite vertices -> (3,) float64;
    ValueError when (max - origin) / cell reaches 2^21 cells on an axis."""
    pts = verts.to(torch.float64)
    pts = pts[torch.isfinite(pts).all(1)].contiguous()
    if pts.shape[0] == 0:
        return np.zeros(3)
    lo, hi = clouds._origin([pts], 1e-6)
    if float((hi - lo).max()) / float(cell) >= MAX_CELLS_PER_AXIS:
        raise ValueError(f"svs_mesh_cluster_cells: the mesh's extent / cell exceeds the 2^21 cells per axis of the grid (cell {cell})")
    return lo


def check_origin(verts, origin, cell):
    """an origin the caller gives: (3,) float64; ValueError when (max - origin) / cell reaches 2^21 cells on an axis"""
    origin = np.asarray(origin, np.float64).reshape(3)
    finite = verts[torch.isfinite(verts).all(1)]
    if finite.shape[0] and float((finite.max(0).values.to(torch.float64).cpu().numpy() - origin).max()) / float(cell) >= MAX_CELLS_PER_AXIS:
        raise ValueError(f"svs_mesh_cluster_cells: the mesh's extent / cell exceeds the 2^21 cells per axis of the grid (cell {cell})")
    return origin


def _workspace(verts, faces):
    n = _lib.load().svs_mesh_cluster_workspace_bytes(int(verts.shape[0]), int(faces.shape[0]))
    return torch.empty(n, dtype=torch.uint8, device=verts.device)


def _check_cell(cell, tol=1e-3):
    if not (cell > 0) or not math.isfinite(cell):
        raise ValueError(f"svs_mesh_cluster_cells: the cell size must be positive and finite, got {cell}")
    if not (0 < tol < 1):
        raise ValueError(f"svs_mesh_cluster_solve: tol must lie in (0,1), got {tol}")


def cells_raw(verts, faces, origin, cell, ws):
    """One call of svs_mesh_cluster_cells on device tensors -> (vert_cell (V,) int32, n_cells)"""
    vert_cell = torch.empty(verts.shape[0], dtype=torch.int32, device=verts.device)
    n_cells = ctypes.c_int(0)
    rc = _lib.load().svs_mesh_cluster_cells(_ptr(verts), int(verts.shape[0]), _ptr(faces), int(faces.shape[0]), _host_origin(origin),
                                            float(cell), _ptr(ws), _ptr(vert_cell), ctypes.byref(n_cells), _stream())
    ENTRY_CALLS["cells"] += 1
    _lib.check(rc, "svs_mesh_cluster_cells")
    return vert_cell, int(n_cells.value)


def faces_count_raw(verts, faces, vert_cell, n_cells, ws):
    """One call of svs_mesh_cluster_faces_count -> (keep (F,) uint8, offsets (F,) int32, count: a device int)"""
    n = int(faces.shape[0])
    keep = torch.empty(n, dtype=torch.uint8, device=verts.device)
    offsets = torch.empty(n, dtype=torch.int32, device=verts.device)
    count = torch.zeros(1, dtype=torch.int32, device=verts.device)
    rc = _lib.load().svs_mesh_cluster_faces_count(_ptr(verts), int(verts.shape[0]), _ptr(faces), n, _ptr(vert_cell), int(n_cells),
                                                  _ptr(ws), _ptr(keep), _ptr(offsets), _ptr(count), _stream())
    ENTRY_CALLS["faces_count"] += 1
    _lib.check(rc, "svs_mesh_cluster_faces_count")
    return keep, offsets, count


def count_faces(verts, faces, cell, origin=None, ws=None):
    """The faces `cluster` would return at this cell size, by the cheap passes alone (cells and the face count; no sums, no
    solve) -> (faces, cells)"""
    verts, faces, _ = mesh_args(verts, faces)
    _check_cell(cell)
    origin = default_origin(verts, cell) if origin is None else check_origin(verts, origin, cell)
    ws = _workspace(verts, faces) if ws is None else ws
    vert_cell, n_cells = cells_raw(verts, faces, origin, cell, ws)
    return int(faces_count_raw(verts, faces, vert_cell, n_cells, ws)[2].item()), n_cells


def cluster(verts, faces, cell, origin=None, colors=None, tol=1e-3, return_info=False, seconds=None):
    """verts (V,3), faces (F,3), colors (V,3) uint8 or None: arrays or tensors.  cell: the cell size; origin (3,): the grid's
    corner, <= every coordinate (default: `default_origin`).  -> (verts (C,3) float32, faces (M,3) int32[, colors (C,3)
    uint8][, info]) on the device; info: dict(vert_cell (V,) int32: the output vertex of every input vertex, -1 when no
    valid face uses it; info (C,) int32: kept directions | fallback << 2; err (C,) float64: the quadric error; origin, cell).
    Faces with bad indices, corners that are not finite or no area are ignored.  seconds: a dict of phase timers
    (which makes every phase wait for the device)."""
    verts, faces, colors = mesh_args(verts, faces, colors)
    cell = float(cell)
    _check_cell(cell, tol)
    L = _lib.load()
    dev = verts.device
    t0 = time.perf_counter()
    origin = np.asarray(default_origin(verts, cell), np.float64).reshape(3) if origin is None else check_origin(verts, origin, cell)
    ws = _workspace(verts, faces)
    vert_cell, n_cells = cells_raw(verts, faces, origin, cell, ws)
    t0 = tick(seconds, "cells", t0)
    out_verts = torch.empty((n_cells, 3), dtype=torch.float32, device=dev)
    out_colors = None if colors is None else torch.empty((n_cells, 3), dtype=torch.uint8, device=dev)
    info = torch.empty(n_cells, dtype=torch.int32, device=dev)
    err = torch.empty(n_cells, dtype=torch.float64, device=dev)
    rc = L.svs_mesh_cluster_solve(_ptr(verts), int(verts.shape[0]), _ptr(faces), int(faces.shape[0]), _ptr(colors), _host_origin(origin),
                                  cell, float(tol), _ptr(vert_cell), n_cells, _ptr(ws), _ptr(out_verts), _ptr(out_colors), _ptr(info),
                                  _ptr(err), _stream())
    ENTRY_CALLS["solve"] += 1
    _lib.check(rc, "svs_mesh_cluster_solve")
    t0 = tick(seconds, "solve", t0)
    keep, offsets, count = faces_count_raw(verts, faces, vert_cell, n_cells, ws)
    out_faces = torch.empty((int(count.item()), 3), dtype=torch.int32, device=dev)
    if out_faces.shape[0]:
        rc = L.svs_mesh_cluster_faces_emit(_ptr(faces), int(faces.shape[0]), _ptr(vert_cell), _ptr(keep), _ptr(offsets), _ptr(out_faces),
                                           _stream())
        ENTRY_CALLS["faces_emit"] += 1
        _lib.check(rc, "svs_mesh_cluster_faces_emit")
    tick(seconds, "faces", t0)
    out = (out_verts, out_faces) + (() if colors is None else (out_colors,))
    if return_info:
        out += (dict(vert_cell=vert_cell, info=info, err=err, origin=origin, cell=cell),)
    return out


def search_bracket(verts, faces):
    """(mean edge length, box diagonal) over the faces with indices in range and finite corners: the two ends of
    `simplify`'s search"""
    v = verts.to(torch.float64)
    f = faces.to(torch.int64)
    f = f[((f >= 0) & (f < v.shape[0])).all(1)]
    tri = v[f]
    tri = tri[torch.isfinite(tri).all(2).all(1)]
    if tri.shape[0] == 0:
        raise ValueError("svs_mesh_cluster: no face with finite corners to take a cell size from")
    edge = torch.stack([(tri[:, a] - tri[:, b]).norm(dim=1) for a, b in ((0, 1), (1, 2), (2, 0))]).mean()
    pts = tri.reshape(-1, 3)
    diag = (pts.max(0).values - pts.min(0).values).norm()
    lo, hi = float(edge), float(diag)
    if not (0 < lo < hi) or not math.isfinite(hi):
        raise ValueError(f"svs_mesh_cluster: cannot search between a mean edge of {lo} and a box diagonal of {hi}")
    return lo, hi


def bisect(count, lo, hi, target, tries=16):
    """log(cell) bisected between lo and hi, `tries` times: a count that meets the target moves the search to finer cells,
    one that does not to coarser ones.  -> (the finest cell tried whose count meets the target, or None; [(cell, count)])"""
    a, b = math.log(lo), math.log(hi)
    best, tried = None, []
    for _ in range(int(tries)):
        mid = 0.5 * (a + b)
        h = float(math.exp(mid))
        n = int(count(h))
        tried.append((h, n))
        if n <= target:
            best = h if best is None or h < best else best
            b = mid
        else:
            a = mid
    return best, tried


def simplify(verts, faces, *, cell=None, target_faces=None, ratio=None, colors=None, tol=1e-3, tries=16, return_info=False,
             seconds=None):
    """Exactly one of cell (the cell size), target_faces (at most this many faces) and ratio (at most ratio * F faces, ratio in
    (0,1)).  With a face target, log(cell) is bisected `tries` times between the mesh's mean edge length and its box diagonal
    with the cheap passes alone (`count_faces`: no sums, no solve), and the finest cell size tried whose face count meets the
    target is taken.  The face count is not strictly monotone in the cell size (a coarser grid that falls differently can
    keep a few more faces), so the answer is the best of the tries, not an optimum.  ValueError when not even the box
    diagonal meets the target.  -> `cluster`'s tuple; info also has tried: [(cell, faces)], bracket: the search's two ends."""
    if sum(x is not None for x in (cell, target_faces, ratio)) != 1:
        raise ValueError("svs_mesh_cluster: give exactly one of cell, target_faces and ratio")
    verts, faces, colors = mesh_args(verts, faces, colors)
    tried, bracket = [], None
    t0 = time.perf_counter()
    if cell is None:
        if ratio is not None:
            if not (0 < ratio < 1):
                raise ValueError(f"svs_mesh_cluster: ratio must lie in (0,1), got {ratio}")
            target_faces = int(ratio * int(faces.shape[0]))
        if target_faces < 0 or int(tries) < 1:
            raise ValueError(f"svs_mesh_cluster: target_faces must not be negative and tries at least 1, got {target_faces} and {tries}")
        bracket = search_bracket(verts, faces)
        ws = _workspace(verts, faces)
        cell, tried = bisect(lambda h: count_faces(verts, faces, h, ws=ws)[0], bracket[0], bracket[1], int(target_faces), tries)
        if cell is None:
            n = count_faces(verts, faces, bracket[1], ws=ws)[0]
            tried.append((bracket[1], n))
            if n > target_faces:
                raise ValueError(f"svs_mesh_cluster: no cell size up to the box diagonal {bracket[1]:.6g} gives {target_faces} faces or fewer")
            cell = bracket[1]
    tick(seconds, "search", t0)
    out = cluster(verts, faces, cell, colors=colors, tol=tol, return_info=True, seconds=seconds)
    out[-1].update(tried=tried, bracket=bracket)
    return out if return_info else out[:-1]


def distance(verts_a, faces_a, verts_b, faces_b, thresh):
    """Both surfaces sampled about `thresh` apart (`clouds.sample_mesh`), nearest neighbours by `clouds.nearest_neighbor` ->
    dict(a_to_b_mean, a_to_b_max, b_to_a_mean, b_to_a_max, mean: the mean of the two means, max: the larger maximum, samples_a,
    samples_b)"""
    def host(v, f):
        v = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, np.float64).reshape(-1, 3)
        f = np.asarray(f.detach().cpu() if torch.is_tensor(f) else f, np.int64).reshape(-1, 3)
        return v, f
    a = clouds.sample_mesh(*host(verts_a, faces_a), thresh)
    b = clouds.sample_mesh(*host(verts_b, faces_b), thresh)
    if a.shape[0] == 0 or b.shape[0] == 0:
        raise ValueError("svs_mesh_cluster: distance needs two meshes with vertices")
    both = torch.cat([a, b])
    ext = both.max(0).values - both.min(0).values
    radius = float(ext.norm()) + float(thresh)
    out = {}
    for name, ref, query in (("a_to_b", b, a), ("b_to_a", a, b)):
        # the search radius is the box diagonal: every result is exact; the grid keeps it within 4096 cells
        cell = max(float(ext.max()) / (1 << 20), min(radius, 2.0 * float(ext.max()) / max(ref.shape[0], 1) ** 0.5), radius / 4000.0)
        d = clouds.nearest_neighbor(ref, query, radius, cell=cell)
        out[name + "_mean"], out[name + "_max"] = float(d.mean()), float(d.max())
    out.update(mean=0.5 * (out["a_to_b_mean"] + out["b_to_a_mean"]), max=max(out["a_to_b_max"], out["b_to_a_max"]),
               samples_a=int(a.shape[0]), samples_b=int(b.shape[0]))
    return out


def simplify_ply(ply_in, ply_out, *, cell=None, target_faces=None, ratio=None, tol=1e-3, tries=16, report=False, report_thresh=None,
                 log=None):
    """The mesh file ply_in (`ply.read_mesh`; its colours are kept when it has them) simplified into ply_out (`ply.write`).
    report: also `distance` between the two, sampled at report_thresh (default: half the cell size).
    -> (verts, faces, colors or None: host arrays, stats: dict(files, faces_in, faces_out, verts_in, verts_out, cell, ranks: cells
    by kept directions [0..3], fallbacks, tried, distance or None, launches, seconds per phase))"""
    sec = OrderedDict((k, 0.0) for k in PHASES)
    calls = dict(ENTRY_CALLS)
    t0 = time.perf_counter()
    verts, faces, colors = _ply.read_mesh_colors(ply_in)
    t0 = tick(sec, "read", t0)
    verts_d, faces_d, colors_d = mesh_args(verts, faces, colors)
    tick(sec, "upload", t0)
    out = simplify(verts_d, faces_d, cell=cell, target_faces=target_faces, ratio=ratio, colors=colors_d, tol=tol, tries=tries,
                   return_info=True, seconds=sec)
    info = out[-1]
    t0 = time.perf_counter()
    new_v, new_f = out[0].cpu().numpy(), out[1].cpu().numpy()
    new_c = out[2].cpu().numpy() if colors is not None else None
    codes = info["info"].cpu().numpy()
    t0 = tick(sec, "download", t0)
    _ply.write(ply_out, new_v, new_c, new_f)
    t0 = tick(sec, "write", t0)
    dist = None
    if report and len(new_f):
        dist = distance(verts, faces, new_v, new_f, report_thresh if report_thresh is not None else 0.5 * info["cell"])
        tick(sec, "report", t0)
    stats = dict(files=dict(ply=ply_out), faces_in=len(faces), faces_out=len(new_f), verts_in=len(verts), verts_out=len(new_v),
                 cell=info["cell"], ranks=np.bincount(codes & 3, minlength=4).tolist(), fallbacks=int((codes >> 2).sum()),
                 tried=info["tried"], distance=dist, launches=launches_since(ENTRY_CALLS, calls), seconds=sec)
    if log is not None:
        log(f"meshsimplify: {ply_in}: faces {len(faces)} -> {len(new_f)}, vertices {len(verts)} -> {len(new_v)}, cell {info['cell']:.6g}"
            + (f" after {len(info['tried'])} tries" if info["tried"] else "") + f" -> {ply_out}")
        log("cells by rank 0..3: " + " ".join(map(str, stats["ranks"])) + f", fallbacks {stats['fallbacks']}")
        if dist is not None:
            log(f"distance in -> out mean {dist['a_to_b_mean']:.6g} max {dist['a_to_b_max']:.6g}, out -> in mean {dist['b_to_a_mean']:.6g} "
                f"max {dist['b_to_a_max']:.6g} ({dist['mean'] / info['cell']:.4f} and {dist['max'] / info['cell']:.4f} cells)")
        log(seconds_line(sec))
    return new_v, new_f, new_c, stats


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Simplifies a mesh on the GPU: vertex clustering with quadric error metrics")
    p.add_argument("--ply", required=True, help="the mesh (a PLY with faces; vertex colours are kept)")
    p.add_argument("--ply-out", required=True, help="the simplified mesh")
    how = p.add_mutually_exclusive_group(required=True)
    how.add_argument("--cell", type=float, default=None, help="the cell size")
    how.add_argument("--faces", type=int, default=None, help="at most this many faces: the cell size is searched")
    how.add_argument("--ratio", type=float, default=None, help="at most this share of the faces, in (0,1): the cell size is searched")
    p.add_argument("--tol", type=float, default=1e-3, help="directions with an eigenvalue above tol * the largest are solved for")
    p.add_argument("--tries", type=int, default=16, help="steps of the search")
    p.add_argument("--report", action="store_true", help="print the distance between the two surfaces")
    a = p.parse_args(argv)
    if a.cell is not None and not (a.cell > 0 and math.isfinite(a.cell)):
        p.error("--cell must be positive")
    if a.faces is not None and a.faces < 0:
        p.error("--faces must not be negative")
    if a.ratio is not None and not (0 < a.ratio < 1):
        p.error("--ratio lies in (0,1)")
    if not (0 < a.tol < 1) or a.tries < 1:
        p.error("--tol lies in (0,1) and --tries is at least 1")
    return a


def main(argv=None):
    a = parse_args(argv)
    return simplify_ply(a.ply, a.ply_out, cell=a.cell, target_faces=a.faces, ratio=a.ratio, tol=a.tol, tries=a.tries, report=a.report,
                        log=print)


if __name__ == "__main__":
    main()
