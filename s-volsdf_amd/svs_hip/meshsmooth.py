"""A triangle mesh made smoother on the HIP path (csrc/svs_meshsmooth.hip): the mesh's connectivity, Taubin's shrink-free
smoothing and a feature-preserving denoiser.

    python -m svs_hip.meshsmooth --ply exps_mvs/tsdf/mvsnet106_l3.ply --ply-out smooth.ply [--method taubin|denoise] [--iters N] \\
        [--lambda L --mu M] [--normal-iters N --vertex-iters N --rn R --rs R] [--boundary fixed|curve|free] [--report]

A marching-cubes mesh over a volume fused from noisy depth (`svs_hip.tsdf`, `svs_hip.poisson`, `svs_hip.mesh`) carries voxel
staircases and depth noise.  `taubin` moves every vertex towards the mean of its neighbours and then away from it again
(Taubin 1995: lambda | mu), which removes the noise without the shrinkage of a plain Laplacian.  `denoise` filters the face
normals bilaterally (Zheng et al. 2011, local scheme; Tukey biweights in place of the Gaussians, so no exp) and then moves
the vertices to fit them (Sun et al. 2007): creases sharper than the normal support stay creases.  Every pass is a gather
in one fixed order: the same bytes in every run.

OURS throughout: the reference has no such step.  The arithmetic is fixed in include/svolsdf_hip.h and restated in float64
in tests/meshsmooth_oracle.py.  The defaults rest on synthetic shapes only.

    adjacency(verts, faces)                     neighbours and faces per vertex, boundary and non-manifold edges
    taubin(verts, faces, iters, lam, mu, ...)   -> (verts, faces[, info])
    denoise(verts, faces, normal_iters, ...)    -> (verts, faces[, info])
    report(verts_in, verts_out, faces)          what the smoothing did: displacement, volume, surface distance
    smooth_ply(ply_in, ply_out, method, ...)    files in and out; what the command line runs
"""
import argparse
import ctypes
import math
import time
from collections import OrderedDict

import numpy as np
import torch

from . import lib as _lib
from . import meshsimplify
from . import ply as _ply
from .images import seconds_line, tick
from .ops import _ptr, _stream
from .views import launches_since, mesh_args

BOUNDARY_MODES = {"fixed": _lib.SMOOTH_FIXED, "curve": _lib.SMOOTH_CURVE, "free": _lib.SMOOTH_FREE}
USED, BOUNDARY, NONMANIFOLD = _lib.MESH_USED, _lib.MESH_BOUNDARY, _lib.MESH_NONMANIFOLD
MAX_FACES = (2 ** 31 - 1) // 6
ENTRY_CALLS = {"adjacency": 0, "taubin": 0, "face_frames": 0, "normal_filter": 0, "vertex_update": 0}   # C entry points called
PHASES = ("read", "upload", "adjacency", "smooth", "download", "write", "report")


def _require(ok, entry, why):
    if not ok:
        raise ValueError(f"{entry}: {why}")


def _mode(entry, boundary, allowed):
    _require(boundary in allowed, entry, f"boundary must be one of {', '.join(allowed)}, got {boundary!r}")
    return BOUNDARY_MODES[boundary]


def _iters(entry, what, n):
    _require(isinstance(n, (int, np.integer)) and not isinstance(n, bool) and n >= 0, entry, f"{what} must be an integer >= 0, got {n!r}")
    return int(n)


def adjacency_raw(verts, faces, ws=None):
    """One call of svs_mesh_adjacency on device tensors -> `adjacency`'s dict without mean_edge"""
    V, F = int(verts.shape[0]), int(faces.shape[0])
    _require(F <= MAX_FACES, "svs_mesh_adjacency", f"more than {MAX_FACES} faces")
    L = _lib.load()
    dev = verts.device
    ws = torch.empty(L.svs_mesh_smooth_workspace_bytes(V, F), dtype=torch.uint8, device=dev) if ws is None else ws
    nbr_start = torch.empty(V + 1, dtype=torch.int32, device=dev)
    face_start = torch.empty(V + 1, dtype=torch.int32, device=dev)
    nbr = torch.empty(6 * F, dtype=torch.int32, device=dev)
    nbr_boundary = torch.empty(6 * F, dtype=torch.uint8, device=dev)
    vert_face = torch.empty(3 * F, dtype=torch.int32, device=dev)
    face_valid = torch.empty(F, dtype=torch.uint8, device=dev)
    flags = torch.empty(V, dtype=torch.int32, device=dev)
    counts = (ctypes.c_int * 4)()
    rc = L.svs_mesh_adjacency(_ptr(verts), V, _ptr(faces), F, _ptr(ws), _ptr(nbr_start), _ptr(nbr), _ptr(nbr_boundary), _ptr(face_start),
                              _ptr(vert_face), _ptr(face_valid), _ptr(flags), counts, _stream())
    ENTRY_CALLS["adjacency"] += 1
    _lib.check(rc, "svs_mesh_adjacency")
    edges, boundary_edges, nonmanifold_edges, valid_faces = (int(c) for c in counts)
    return dict(nbr_start=nbr_start, nbr=nbr[:2 * edges], nbr_boundary=nbr_boundary[:2 * edges], face_start=face_start,
                vert_face=vert_face[:3 * valid_faces], face_valid=face_valid, flags=flags,
                counts=dict(edges=edges, boundary_edges=boundary_edges, nonmanifold_edges=nonmanifold_edges, valid_faces=valid_faces))


def adjacency(verts, faces):
    """verts (V,3), faces (F,3): arrays or tensors -> dict of device arrays: nbr_start (V+1,) int32, nbr (E2,) int32: each
    distinct neighbour of a vertex once, ascending; nbr_boundary (E2,) uint8: 1 where that edge has one face; face_start
    (V+1,) int32, vert_face: the valid faces of a vertex, ascending; face_valid (F,) uint8; flags (V,) int32: USED |
    BOUNDARY | NONMANIFOLD; and of host values: counts = dict(edges, boundary_edges, nonmanifold_edges, valid_faces),
    mean_edge (`meshsimplify.search_bracket`'s first value; None for a mesh without a face with finite corners)."""
    verts, faces, _ = mesh_args(verts, faces)
    adj = adjacency_raw(verts, faces)
    try:
        adj["mean_edge"] = meshsimplify.search_bracket(verts, faces)[0]
    except ValueError:
        adj["mean_edge"] = None
    return adj


def _working(verts):
    x = verts.to(torch.float64).contiguous()
    return x, torch.empty_like(x)


def _narrow(x, verts, adj):
    """float32 of the working array; a vertex no valid face uses (one that is not finite among them) keeps its input bits"""
    return torch.where(((adj["flags"] & USED) != 0)[:, None], x.to(torch.float32), verts)


def taubin_raw(x, tmp, adj, iters, lam, mu, boundary):
    """One call of svs_mesh_taubin on the float64 working array x (V,3), in place"""
    rc = _lib.load().svs_mesh_taubin(_ptr(x), _ptr(tmp), int(x.shape[0]), _ptr(adj["nbr_start"]), _ptr(adj["nbr"]), _ptr(adj["nbr_boundary"]),
                                     _ptr(adj["flags"]), int(iters), float(lam), float(mu), int(boundary), _stream())
    ENTRY_CALLS["taubin"] += 1
    _lib.check(rc, "svs_mesh_taubin")
    return x


def taubin(verts, faces, iters=10, lam=0.5, mu=-0.53, boundary="fixed", adj=None, return_info=False):
    """`iters` iterations of a pass with factor lam, then one with factor mu (mu = 0: a plain Laplacian, which shrinks).
    boundary: "fixed" (boundary vertices stay), "curve" (they move along the boundary alone) or "free".  adj: `adjacency`
    of the same mesh, when the caller has it.  -> (verts (V,3) float32, faces as given[, info: dict(adj, iters, lam, mu,
    boundary)]) on the device.  Faces pass through untouched, the invalid ones too; vertices no valid face uses keep their bits."""
    name = "svs_mesh_taubin"
    verts, faces, _ = mesh_args(verts, faces)
    iters = _iters(name, "iters", iters)
    _require(0 < lam <= 1, name, f"lam must lie in (0,1], got {lam}")
    _require(-2 <= mu <= 0, name, f"mu must lie in [-2,0], got {mu}")
    mode = _mode(name, boundary, ("fixed", "curve", "free"))
    adj = adjacency(verts, faces) if adj is None else adj
    out = verts.clone()
    if iters > 0 and verts.shape[0]:
        x, tmp = _working(verts)
        out = _narrow(taubin_raw(x, tmp, adj, iters, lam, mu, mode), verts, adj)
    return (out, faces) + ((dict(adj=adj, iters=iters, lam=float(lam), mu=float(mu), boundary=boundary),) if return_info else ())


def face_frames_raw(x, faces, adj):
    """One call of svs_mesh_face_frames -> (normals (F,3), areas (F,), centroids (F,3)) float64"""
    F = int(faces.shape[0])
    normals = torch.empty((F, 3), dtype=torch.float64, device=x.device)
    areas = torch.empty(F, dtype=torch.float64, device=x.device)
    cent = torch.empty((F, 3), dtype=torch.float64, device=x.device)
    rc = _lib.load().svs_mesh_face_frames(_ptr(x), int(x.shape[0]), _ptr(faces), _ptr(adj["face_valid"]), F, _ptr(normals), _ptr(areas),
                                          _ptr(cent), _stream())
    ENTRY_CALLS["face_frames"] += 1
    _lib.check(rc, "svs_mesh_face_frames")
    return normals, areas, cent


def normal_filter_raw(normals, areas, cent, faces, n_verts, adj, iters, rs, rn):
    """One call of svs_mesh_normal_filter on normals (F,3) float64, in place"""
    tmp = torch.empty_like(normals)
    rc = _lib.load().svs_mesh_normal_filter(_ptr(faces), _ptr(adj["face_valid"]), int(faces.shape[0]), int(n_verts), _ptr(adj["face_start"]),
                                            _ptr(adj["vert_face"]), _ptr(areas), _ptr(cent), _ptr(normals), _ptr(tmp), int(iters), float(rs),
                                            float(rn), _stream())
    ENTRY_CALLS["normal_filter"] += 1
    _lib.check(rc, "svs_mesh_normal_filter")
    return normals


def vertex_update_raw(x, tmp, normals, faces, adj, iters, boundary):
    """One call of svs_mesh_vertex_update on the float64 working array x (V,3), in place"""
    rc = _lib.load().svs_mesh_vertex_update(_ptr(x), _ptr(tmp), int(x.shape[0]), _ptr(faces), int(faces.shape[0]), _ptr(adj["face_start"]),
                                            _ptr(adj["vert_face"]), _ptr(adj["flags"]), _ptr(normals), int(iters), int(boundary), _stream())
    ENTRY_CALLS["vertex_update"] += 1
    _lib.check(rc, "svs_mesh_vertex_update")
    return x


def denoise(verts, faces, normal_iters=5, vertex_iters=10, rn=0.6, rs=None, boundary="fixed", adj=None, return_info=False):
    """Bilateral normal filtering, then the vertex update.  rn in (0,2]: the support on |n_f - n_g| (0.6 is the chord of
    about 35 degrees: faces across a sharper crease do not see each other); rs > 0: the spatial support on the distance of
    two centroids (default: 2 mean edges).  boundary: "fixed" or "free".  -> (verts (V,3) float32, faces as given[, info:
    dict(adj, normals (F,3) float64: the filtered ones, rs, rn, normal_iters, vertex_iters, boundary)]) on the device."""
    verts, faces, _ = mesh_args(verts, faces)
    normal_iters = _iters("svs_mesh_normal_filter", "normal_iters", normal_iters)
    vertex_iters = _iters("svs_mesh_vertex_update", "vertex_iters", vertex_iters)
    _require(0 < rn <= 2, "svs_mesh_normal_filter", f"rn must lie in (0,2], got {rn}")
    _require(rs is None or (rs > 0 and math.isfinite(rs)), "svs_mesh_normal_filter", f"rs must be positive and finite, got {rs}")
    mode = _mode("svs_mesh_vertex_update", boundary, ("fixed", "free"))
    adj = adjacency(verts, faces) if adj is None else adj
    if rs is None:
        rs = 2.0 * adj["mean_edge"] if adj["mean_edge"] is not None else 1.0      # no face to filter: any support serves
    x, tmp = _working(verts)
    normals, areas, cent = face_frames_raw(x, faces, adj)
    normal_filter_raw(normals, areas, cent, faces, verts.shape[0], adj, normal_iters, rs, rn)
    out = verts.clone()
    if vertex_iters > 0 and verts.shape[0]:
        out = _narrow(vertex_update_raw(x, tmp, normals, faces, adj, vertex_iters, mode), verts, adj)
    info = dict(adj=adj, normals=normals, rs=float(rs), rn=float(rn), normal_iters=normal_iters, vertex_iters=vertex_iters, boundary=boundary)
    return (out, faces) + ((info,) if return_info else ())


def signed_volume(verts, faces, face_valid=None):
    """sum over the faces (the valid ones, given face_valid) of P0 . (P1 x P2) / 6, a float64 torch sum"""
    f = faces.to(torch.int64)
    if face_valid is not None:
        f = f[face_valid != 0]
    P = verts.to(torch.float64)[f]
    return float((P[:, 0] * torch.cross(P[:, 1], P[:, 2], dim=1)).sum() / 6.0)


def report(verts_in, verts_out, faces, adj=None):
    """-> dict(mean_edge, displacement_mean, displacement_max: in mean edges, over the vertices valid faces use; volume_in,
    volume_out: signed, over the valid faces; distance: `meshsimplify.distance` of the two surfaces sampled half a mean edge
    apart)"""
    verts_in, faces, _ = mesh_args(verts_in, faces)
    verts_out = mesh_args(verts_out, faces)[0]
    adj = adjacency(verts_in, faces) if adj is None else adj
    _require(adj["mean_edge"] is not None and adj["counts"]["valid_faces"] > 0, "svs_mesh_adjacency", "report needs a mesh with a valid face")
    used = (adj["flags"] & USED) != 0
    edge = adj["mean_edge"]
    d = (verts_out.to(torch.float64) - verts_in.to(torch.float64))[used].norm(dim=1) / edge
    f = faces[adj["face_valid"] != 0]
    return dict(mean_edge=edge, displacement_mean=float(d.mean()), displacement_max=float(d.max()),
                volume_in=signed_volume(verts_in, f), volume_out=signed_volume(verts_out, f),
                distance=meshsimplify.distance(verts_in, f, verts_out, f, 0.5 * edge))


_report = report                                            # smooth_ply has a switch of that name


def smooth_ply(ply_in, ply_out, method="taubin", *, iters=10, lam=0.5, mu=-0.53, normal_iters=5, vertex_iters=10, rn=0.6, rs=None,
               boundary="fixed", report=False, log=None):
    """The mesh file ply_in (`ply.read_mesh`; its colours are kept when it has them) smoothed into ply_out (`ply.write`).
    method "taubin": iters, lam, mu; "denoise": normal_iters, vertex_iters, rn, rs.  report: also `report` of the two.
    -> (verts, faces, colors or None: host arrays, stats: dict(files, method, faces, verts, counts, flags: vertices by flag
    value [0..7], mean_edge, report or None, launches, seconds per phase))"""
    _require(method in ("taubin", "denoise"), "svs_mesh_smooth", f"method must be taubin or denoise, got {method!r}")
    sec = OrderedDict((k, 0.0) for k in PHASES)
    calls = dict(ENTRY_CALLS)
    t0 = time.perf_counter()
    verts, faces, colors = _ply.read_mesh_colors(ply_in)
    t0 = tick(sec, "read", t0)
    verts_d, faces_d, _ = mesh_args(verts, faces)
    t0 = tick(sec, "upload", t0)
    adj = adjacency(verts_d, faces_d)
    t0 = tick(sec, "adjacency", t0)
    if method == "taubin":
        out = taubin(verts_d, faces_d, iters, lam, mu, boundary, adj=adj)[0]
    else:
        out = denoise(verts_d, faces_d, normal_iters, vertex_iters, rn, rs, boundary, adj=adj)[0]
    t0 = tick(sec, "smooth", t0)
    new_v = out.cpu().numpy()
    flags = np.bincount(adj["flags"].cpu().numpy(), minlength=8).tolist()
    t0 = tick(sec, "download", t0)
    _ply.write(ply_out, new_v, colors, faces)
    t0 = tick(sec, "write", t0)
    rep = None
    if report and adj["counts"]["valid_faces"]:
        rep = _report(verts_d, out, faces_d, adj=adj)
        tick(sec, "report", t0)
    stats = dict(files=dict(ply=ply_out), method=method, faces=len(faces), verts=len(verts), counts=adj["counts"], flags=flags,
                 mean_edge=adj["mean_edge"], report=rep, launches=launches_since(ENTRY_CALLS, calls), seconds=sec)
    if log is not None:
        c = adj["counts"]
        log(f"meshsmooth: {ply_in}: {method}, {len(verts)} vertices, {len(faces)} faces ({c['valid_faces']} valid), {c['edges']} edges "
            f"({c['boundary_edges']} boundary, {c['nonmanifold_edges']} non-manifold), boundary {boundary} -> {ply_out}")
        log("vertices by flags 0..7: " + " ".join(map(str, flags)))
        if rep is not None:
            log(f"displacement mean {rep['displacement_mean']:.6g} max {rep['displacement_max']:.6g} mean edges ({rep['mean_edge']:.6g}), "
                f"volume {rep['volume_in']:.6g} -> {rep['volume_out']:.6g}, distance mean {rep['distance']['mean']:.6g} "
                f"max {rep['distance']['max']:.6g}")
        log(seconds_line(sec))
    return new_v, faces, colors, stats


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Smooths a mesh on the GPU: Taubin smoothing or bilateral normal filtering")
    p.add_argument("--ply", required=True, help="the mesh (a PLY with faces; vertex colours are kept)")
    p.add_argument("--ply-out", required=True, help="the smoothed mesh")
    p.add_argument("--method", choices=("taubin", "denoise"), default="taubin")
    p.add_argument("--iters", type=int, default=10, help="taubin: iterations")
    p.add_argument("--lambda", dest="lam", type=float, default=0.5, help="taubin: the factor of the first pass, in (0,1]")
    p.add_argument("--mu", type=float, default=-0.53, help="taubin: the factor of the second pass, in [-2,0]; 0: a plain Laplacian")
    p.add_argument("--normal-iters", type=int, default=5, help="denoise: passes over the face normals")
    p.add_argument("--vertex-iters", type=int, default=10, help="denoise: passes over the vertices")
    p.add_argument("--rn", type=float, default=0.6, help="denoise: the support on the difference of two normals, in (0,2]")
    p.add_argument("--rs", type=float, default=None, help="denoise: the spatial support (default: two mean edges)")
    p.add_argument("--boundary", choices=("fixed", "curve", "free"), default="fixed")
    p.add_argument("--report", action="store_true", help="print displacement, volume and the distance between the two surfaces")
    a = p.parse_args(argv)
    if a.iters < 0 or a.normal_iters < 0 or a.vertex_iters < 0:
        p.error("--iters, --normal-iters and --vertex-iters must not be negative")
    if not (0 < a.lam <= 1) or not (-2 <= a.mu <= 0):
        p.error("--lambda lies in (0,1] and --mu in [-2,0]")
    if not (0 < a.rn <= 2) or (a.rs is not None and not (a.rs > 0 and math.isfinite(a.rs))):
        p.error("--rn lies in (0,2] and --rs is positive")
    if a.method == "denoise" and a.boundary == "curve":
        p.error("--boundary curve goes with --method taubin only")
    return a


def main(argv=None):
    a = parse_args(argv)
    return smooth_ply(a.ply, a.ply_out, a.method, iters=a.iters, lam=a.lam, mu=a.mu, normal_iters=a.normal_iters,
                      vertex_iters=a.vertex_iters, rn=a.rn, rs=a.rs, boundary=a.boundary, report=a.report, log=print)


if __name__ == "__main__":
    main()
