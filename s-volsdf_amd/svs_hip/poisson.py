"""A cleaned cloud meshed on the HIP path (csrc/svs_poisson.hip): Poisson surface reconstruction on one dense grid.

    python -m svs_hip.poisson --ply exps_mvs/clean/mvsnet106_l3.ply --ply-out exps_mvs/poisson/mvsnet106_l3.ply --voxel 1.5 \\
        [--pad 4] [--min-density 2.0] [--tol 1e-4] [--max-iter N] [--bounds x0 y0 z0 x1 y1 z1] [--largest] [--raw] [--screen S]

`svs_hip.cloudclean` writes a cloud with oriented normals; this module is what reads them back.  The normals are splatted
into a grid vector field, a Poisson equation is solved for a function that is smaller inside than outside, its level set at
the mean over the cloud is extracted by `mesh.marching_cubes`, and the faces the cloud does not support are trimmed
(Kazhdan, Bolitho and Hoppe, "Poisson surface reconstruction", 2006, on one dense grid, without octree).  Screening (Kazhdan
and Hoppe, "Screened Poisson surface reconstruction", 2013) is opt-in, `screen=S`: the points then also hold the solution at
the level, through the diagonal term weight * W (the point term lumped onto the splat's weight plane), and the solve is
preconditioned by the operator's diagonal; without it every stage is what it was.
Unlike `svs_hip.mesh` it needs no checkpoint, unlike `svs_hip.tsdf` no depth maps or cameras; what comes out is what
`meshview`, `meshpaint`, `meshsimplify` and `evals.eval_dtu --mode mesh` take.

OURS throughout: the reference has no such step.  The arithmetic is fixed in include/svolsdf_hip.h and restated in float64 in
tests/poisson_oracle.py.

    splat(pts, normals, dims, origin, voxel)    -> field (4,n0,n1,n2): Vx, Vy, Vz, W; counted, skipped
    divergence(field, voxel)                    -> rhs
    apply(x, voxel)                             -> A x, the 7-point operator with 0 beyond the grid
    solve(rhs, voxel, tol, max_iter, check_every)   conjugate gradients -> x, dict(iterations, residual, converged)
    screen_weight(W, counted, screen, voxel)    -> weight = screen / (density voxel^2), density = points per touched node
    apply_screened(x, W, weight, voxel)         -> (A + diag(weight W)) x
    solve_screened(rhs, W, weight, voxel, ...)      diagonally preconditioned conjugate gradients -> what solve returns
    sample(x, pts, origin, voxel)               -> values at the points, their mean (the level), counted
    face_keep(W, cells, min_density)            -> the trim's mask
    reconstruct(xyz, normals, rgb, voxel=...)   all of it -> host arrays;  reconstruct_ply: files in and out

SETTINGS: `pad` (default 4 voxels around the cloud's box) and `min_density` (default 2.0: a face survives when the splat
weights of its cell's eight nodes sum to two points' worth) rest on synthetic spheres and hemispheres only
(NOTES/poisson.md); nobody has tried them on a real scan.  `screen` has no default value: 1, 4 and 16 were tried on a
synthetic sphere of uneven density only (NOTES/poisson_screen.md), none on a real scan.
"""
import argparse
import ctypes
import math
import os
import time
from collections import OrderedDict

import numpy as np
import torch

from . import clouds
from . import lib as _lib
from . import mesh as _mesh
from . import ply as _ply
from .images import seconds_line, tick, to_device
from .ops import _ptr, _stream
from .tsdf import MAX_VOXELS, bounds_from_points
from .views import launches_since

ENTRY_CALLS = {"splat": 0, "divergence": 0, "apply": 0, "cg": 0, "sample": 0, "keep": 0}   # C entry points called, not kernels
SCREENED_CALLS = {"apply": 0, "pcg": 0}                     # the svs_screened_* entries: reported only when screening is on
PHASES = ("read", "upload", "splat", "divergence", "solve", "sample", "scan", "classify", "emit", "trim", "colors", "download", "write")
_D3 = ctypes.c_double * 3


def stencil_tile():
    """the stencil workgroup's extent along axes 0, 1, 2 (dispatch edges for the tests)"""
    t = (ctypes.c_int * 3)()
    _lib.check(_lib.load().svs_poisson_tile(t), "svs_poisson_tile")
    return tuple(t)


def _check_voxel(voxel, name):
    voxel = float(voxel)
    if not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError(f"{name}: the voxel must be positive and finite, got {voxel}")
    return voxel


def _volume(x, name, planes=None):
    """a float32 device volume whose memory is contiguous, as it is (a view at an odd offset stays one) -> (x, n0, n1, n2)"""
    want = 3 if planes is None else 4
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype is torch.float32 and x.dim() == want):
        raise TypeError(f"{name}: a {want}-D float32 device tensor")
    if planes is not None and x.shape[0] != planes:
        raise ValueError(f"{name}: {planes} planes expected, got {x.shape[0]}")
    if not x.is_contiguous():
        x = x.contiguous()
    return (x,) + tuple(int(s) for s in x.shape[-3:])


def splat(pts, normals, dims, origin, voxel):
    """pts (n,3) float64, normals (n,3) float32 (used as given), dims (n0,n1,n2), origin (3,), voxel -> (field (4,n0,n1,n2)
    float32 on the device: Vx, Vy, Vz, W; counted; skipped).  A point outside the cells of the grid or with a coordinate or
    normal that is not finite is skipped.  ValueError for an empty cloud and for one whose points are all skipped."""
    pts = to_device(pts, torch.float64, "poisson", "pts", ndim=(2,))
    normals = to_device(normals, torch.float32, "poisson", "normals", ndim=(2,))
    if pts.shape[1:] != (3,) or tuple(normals.shape) != tuple(pts.shape):
        raise ValueError(f"svs_poisson_splat: pts (n,3) and normals (n,3) expected, got {tuple(pts.shape)} and {tuple(normals.shape)}")
    n = int(pts.shape[0])
    if n == 0:
        raise ValueError("svs_poisson_splat: empty cloud (no points)")
    n0, n1, n2 = (int(d) for d in dims)
    voxel = _check_voxel(voxel, "svs_poisson_splat")
    L = _lib.load()
    ws = torch.empty(L.svs_poisson_splat_workspace_bytes(n, n0, n1, n2), dtype=torch.uint8, device=pts.device)
    field = torch.empty((4, n0, n1, n2), dtype=torch.float32, device=pts.device)
    counts = (ctypes.c_int * 2)()
    rc = L.svs_poisson_splat(_ptr(pts), _ptr(normals), n, n0, n1, n2, _D3(*[float(o) for o in np.asarray(origin, np.float64).reshape(3)]),
                             voxel, _ptr(ws), _ptr(field), counts, _stream())
    ENTRY_CALLS["splat"] += 1
    _lib.check(rc, "svs_poisson_splat")
    if counts[0] == 0:
        raise ValueError(f"svs_poisson_splat: all {n} points were skipped (outside the grid's cells, or not finite)")
    return field, int(counts[0]), int(counts[1])


def divergence(field, voxel):
    """field (4,n0,n1,n2) -> rhs (n0,n1,n2) float32: minus the central-difference divergence of (Vx, Vy, Vz), 0 beyond the grid"""
    field, n0, n1, n2 = _volume(field, "svs_poisson_divergence", planes=4)
    rhs = torch.empty((n0, n1, n2), dtype=torch.float32, device=field.device)
    rc = _lib.load().svs_poisson_divergence(_ptr(field), n0, n1, n2, _check_voxel(voxel, "svs_poisson_divergence"), _ptr(rhs), _stream())
    ENTRY_CALLS["divergence"] += 1
    _lib.check(rc, "svs_poisson_divergence")
    return rhs


def apply(x, voxel, out=None):
    """x (n0,n1,n2) float32 -> A x = (6 x - the six neighbours) / voxel^2 with 0 beyond the grid.  out: where to write it
    (a contiguous float32 volume of the same shape, e.g. a view at an odd offset)."""
    x, n0, n1, n2 = _volume(x, "svs_poisson_apply")
    y = torch.empty_like(x) if out is None else _volume(out, "svs_poisson_apply")[0]
    if tuple(y.shape) != (n0, n1, n2):
        raise ValueError(f"svs_poisson_apply: out has shape {tuple(y.shape)}, x {tuple(x.shape)}")
    rc = _lib.load().svs_poisson_apply(_ptr(x), n0, n1, n2, _check_voxel(voxel, "svs_poisson_apply"), _ptr(y), _stream())
    ENTRY_CALLS["apply"] += 1
    _lib.check(rc, "svs_poisson_apply")
    return y


def solve(rhs, voxel, tol=1e-4, max_iter=None, check_every=32, out=None):
    """Conjugate gradients for A x = rhs from x = 0 -> (x (n0,n1,n2) float32, dict(iterations, residual: the recursive
    sqrt(r.r / rhs.rhs) at the end, converged)).  max_iter=None: 4 * max(dims).  The residual is looked at every check_every
    iterations (one 8-byte download) and at max_iter.  ValueError "no normal field" for a zero right-hand side."""
    rhs, n0, n1, n2 = _volume(rhs, "svs_poisson_cg")
    max_iter = 4 * max(n0, n1, n2) if max_iter is None else int(max_iter)
    if not (0 < tol < 1) or max_iter < 1 or int(check_every) < 1:
        raise ValueError(f"svs_poisson_cg: tol in (0,1), max_iter and check_every at least 1, got {tol}, {max_iter}, {check_every}")
    L = _lib.load()
    x = torch.empty_like(rhs) if out is None else _volume(out, "svs_poisson_cg")[0]
    ws = torch.empty(L.svs_poisson_cg_workspace_bytes(n0, n1, n2), dtype=torch.uint8, device=rhs.device)
    it, res, conv = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_int(0)
    rc = L.svs_poisson_cg(_ptr(rhs), n0, n1, n2, _check_voxel(voxel, "svs_poisson_cg"), float(tol), max_iter, int(check_every), _ptr(ws),
                          _ptr(x), ctypes.byref(it), ctypes.byref(res), ctypes.byref(conv), _stream())
    ENTRY_CALLS["cg"] += 1
    if rc == _lib.EINVAL and b"no normal field" in (L.svs_last_error_string() or b""):
        raise ValueError("svs_poisson_cg: no normal field (the right-hand side is zero or not finite)")
    _lib.check(rc, "svs_poisson_cg")
    return x, dict(iterations=int(it.value), residual=float(res.value), converged=bool(conv.value))


def _check_weight(weight, name):
    weight = float(weight)
    if not (weight >= 0 and math.isfinite(weight)):
        raise ValueError(f"{name}: the screening weight must be finite and not negative, got {weight}")
    return weight


def screen_weight(W, counted, screen, voxel):
    """-> (weight, density).  density = counted / the number of nodes the splat touched (W != 0): the points per touched node.
    weight = screen / (density * voxel * voxel): the right-hand side grows with the cloud's density and the Laplacian does not,
    so dividing by the density makes one `screen` mean the same for a thin and a dense cloud, and the voxel factor makes it
    independent of the unit of length.  W: the splat's weight plane `field[3]` (a tensor on any device, or an array)."""
    touched = int(torch.count_nonzero(torch.as_tensor(W)))
    if touched == 0 or int(counted) < 1:
        raise ValueError(f"svs_screened: no density (counted {counted}, {touched} nodes with a weight)")
    density = int(counted) / touched
    return float(screen) / (density * _check_voxel(voxel, "svs_screened") ** 2), density


def apply_screened(x, W, weight, voxel, out=None):
    """x, W (n0,n1,n2) float32 -> (A + diag(weight W)) x, A as in `apply`.  W: the splat's weight plane, as it is (`field[3]`
    is a view at an offset that need not be 16-byte aligned: no copy is made).  out: as in `apply`."""
    name = "svs_screened_apply"
    x, n0, n1, n2 = _volume(x, name)
    W = _volume(W, name)[0]
    y = torch.empty_like(x) if out is None else _volume(out, name)[0]
    if tuple(y.shape) != (n0, n1, n2) or tuple(W.shape) != (n0, n1, n2):
        raise ValueError(f"{name}: out has shape {tuple(y.shape)}, W {tuple(W.shape)}, x {tuple(x.shape)}")
    rc = _lib.load().svs_screened_apply(_ptr(x), _ptr(W), n0, n1, n2, _check_voxel(voxel, name), _check_weight(weight, name), _ptr(y),
                                        _stream())
    SCREENED_CALLS["apply"] += 1
    _lib.check(rc, name)
    return y


def solve_screened(rhs, W, weight, voxel, tol=1e-4, max_iter=None, check_every=32, out=None):
    """Conjugate gradients preconditioned by the diagonal 6 / voxel^2 + weight W for (A + diag(weight W)) x = rhs from x = 0
    -> what `solve` returns; its arguments are `solve`'s, W and weight `apply_screened`'s."""
    name = "svs_screened_pcg"
    rhs, n0, n1, n2 = _volume(rhs, name)
    W = _volume(W, name)[0]
    if tuple(W.shape) != (n0, n1, n2):
        raise ValueError(f"{name}: W has shape {tuple(W.shape)}, rhs {tuple(rhs.shape)}")
    max_iter = 4 * max(n0, n1, n2) if max_iter is None else int(max_iter)
    if not (0 < tol < 1) or max_iter < 1 or int(check_every) < 1:
        raise ValueError(f"{name}: tol in (0,1), max_iter and check_every at least 1, got {tol}, {max_iter}, {check_every}")
    L = _lib.load()
    x = torch.empty_like(rhs) if out is None else _volume(out, name)[0]
    ws = torch.empty(L.svs_screened_pcg_workspace_bytes(n0, n1, n2), dtype=torch.uint8, device=rhs.device)
    it, res, conv = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_int(0)
    rc = L.svs_screened_pcg(_ptr(rhs), _ptr(W), n0, n1, n2, _check_voxel(voxel, name), _check_weight(weight, name), float(tol), max_iter,
                            int(check_every), _ptr(ws), _ptr(x), ctypes.byref(it), ctypes.byref(res), ctypes.byref(conv), _stream())
    SCREENED_CALLS["pcg"] += 1
    if rc == _lib.EINVAL and b"no normal field" in (L.svs_last_error_string() or b""):
        raise ValueError(f"{name}: no normal field (the right-hand side is zero or not finite)")
    _lib.check(rc, name)
    return x, dict(iterations=int(it.value), residual=float(res.value), converged=bool(conv.value))


def sample(x, pts, origin, voxel):
    """x (n0,n1,n2) float32, pts (n,3) float64 -> (values (n,) float64 on the device: trilinear, NaN where `splat` skips the
    point for its position; level: their mean over the counted points; counted)"""
    x, n0, n1, n2 = _volume(x, "svs_poisson_sample")
    pts = to_device(pts, torch.float64, "poisson", "pts", ndim=(2,))
    n = int(pts.shape[0])
    if n == 0:
        raise ValueError("svs_poisson_sample: empty cloud (no points)")
    L = _lib.load()
    ws = torch.empty(L.svs_poisson_sample_workspace_bytes(n), dtype=torch.uint8, device=x.device)
    vals = torch.empty(n, dtype=torch.float64, device=x.device)
    level, counted = ctypes.c_double(0.0), ctypes.c_int(0)
    rc = L.svs_poisson_sample(_ptr(x), n0, n1, n2, _D3(*[float(o) for o in np.asarray(origin, np.float64).reshape(3)]),
                              _check_voxel(voxel, "svs_poisson_sample"), _ptr(pts), n, _ptr(ws), _ptr(vals), ctypes.byref(level),
                              ctypes.byref(counted), _stream())
    ENTRY_CALLS["sample"] += 1
    _lib.check(rc, "svs_poisson_sample")
    return vals, float(level.value), int(counted.value)


def face_keep(W, cells, min_density):
    """keep (F,) uint8: 1 where the splat weights W of the eight nodes of the face's cell sum to min_density or more.  cells:
    (F,) int32 node indices (`mesh.marching_cubes(..., return_cells=True)`).  Not `tsdf.face_keep`'s rule."""
    W, n0, n1, n2 = _volume(W, "svs_poisson_face_keep")
    cells = cells.to(torch.int32).contiguous()
    keep = torch.empty(cells.shape[0], dtype=torch.uint8, device=W.device)
    rc = _lib.load().svs_poisson_face_keep(_ptr(W), n0, n1, n2, _ptr(cells), int(cells.shape[0]), float(min_density), _ptr(keep), _stream())
    ENTRY_CALLS["keep"] += 1
    _lib.check(rc, "svs_poisson_face_keep")
    return keep


def nearest_colors(pts, rgb, verts, voxel):
    """verts (V,3) -> (V,3) uint8: the colour of the nearest cloud point with finite coordinates (`clouds.nearest_neighbor` on
    a grid of voxel-sized cells: a vertex of the level set lies within a few voxels of the cloud unless the mesh is untrimmed)"""
    ok = torch.isfinite(pts).all(1)
    ref, src = pts[ok].contiguous(), rgb[ok]
    both = torch.cat([ref, verts.double()])
    radius = float((both.max(0).values - both.min(0).values).norm()) + float(voxel)        # the box diagonal: every result is exact
    idx = clouds.nearest_neighbor(ref, verts.double().contiguous(), radius, cell=float(voxel), return_index=True)[1]
    return src[idx.long().clamp_(0, ref.shape[0] - 1)]


def grid_from_points(xyz, voxel, pad=4, bounds=None, max_voxels=MAX_VOXELS):
    """-> origin (3,) float64, dims: `tsdf.bounds_from_points` over the finite points padded by `pad` voxels, or over
    bounds (x0,y0,z0,x1,y1,z1) as they are"""
    if bounds is not None:
        return bounds_from_points(np.asarray(bounds, np.float64).reshape(2, 3), voxel, 0.0, max_voxels)
    xyz = np.asarray(xyz.detach().cpu() if torch.is_tensor(xyz) else xyz, np.float64).reshape(-1, 3)
    xyz = xyz[np.isfinite(xyz).all(1)]
    if len(xyz) == 0:
        raise ValueError("svs_poisson_splat: empty cloud (no finite points to bound the grid with)")
    return bounds_from_points(np.stack([xyz.min(0), xyz.max(0)]), voxel, float(pad) * float(voxel), max_voxels)


def check_screen(screen):
    """None or 0 -> None (the unscreened path); a positive finite number -> float; anything else: ValueError naming `screen`"""
    if screen is None:
        return None
    if isinstance(screen, bool) or not isinstance(screen, (int, float)) or not (screen >= 0 and math.isfinite(screen)):
        raise ValueError(f"svs_poisson: screen must be None, 0 or a positive finite number, got {screen!r}")
    return float(screen) or None


def reconstruct(xyz, normals, rgb=None, voxel=None, pad=4, min_density=2.0, tol=1e-4, max_iter=None, bounds=None, largest=False,
                seconds=None, check_every=32, screen=None):
    """xyz (n,3), normals (n,3) pointing out of the surface, rgb (n,3) uint8 or None: arrays or tensors; voxel: the node
    spacing (required).  -> dict(verts (V,3) float32, faces (F,3) int32, rgb (V,3) uint8 or None: host arrays, stats:
    dict(grid, origin, counted, skipped, iterations, residual, converged, level, faces_before, faces_after)).
    The grid is `grid_from_points` (pad voxels around the cloud, MAX_VOXELS at most); the level is the solution's mean over
    the counted points; min_density: the trim (None or 0: no trim); vertex colours are those of the nearest cloud point
    (`clouds.nearest_neighbor`); largest=True: `mesh.largest_component`.  max_iter=None: 4 * max(dims).
    pad=4 and min_density=2.0 rest on synthetic spheres and hemispheres only; nobody has tried them on a real scan.
    screen: None or 0: the unscreened solve (`solve`); a positive value: the points also pull the solution towards the
    level with the weight `screen_weight` derives from it (`solve_screened`), which keeps the level set on the points of a
    cloud of uneven density; stats hold screen, screen_weight and density (None when it is off).  screen has no default value: 1, 4
    and 16 were tried on a synthetic sphere of uneven density only (NOTES/poisson_screen.md), and nobody has tried them on
    a real scan either.
    seconds: a dict of phase timers (which makes every phase wait for the device)."""
    if voxel is None:
        raise ValueError("svs_poisson: give voxel, the node spacing")
    voxel = _check_voxel(voxel, "svs_poisson")
    screen = check_screen(screen)
    t0 = time.perf_counter()
    origin, dims = grid_from_points(xyz, voxel, pad, bounds)
    pts = to_device(xyz, torch.float64, "poisson", "xyz", ndim=(2,))
    nrm = to_device(normals, torch.float32, "poisson", "normals", ndim=(2,))
    t0 = tick(seconds, "upload", t0)
    field, counted, skipped = splat(pts, nrm, dims, origin, voxel)
    t0 = tick(seconds, "splat", t0)
    rhs = divergence(field, voxel)
    t0 = tick(seconds, "divergence", t0)
    if screen is None:
        x, info = solve(rhs, voxel, tol=tol, max_iter=max_iter, check_every=check_every)
        screened = dict(screen=None, screen_weight=None, density=None)
    else:
        weight, density = screen_weight(field[3], counted, screen, voxel)
        x, info = solve_screened(rhs, field[3], weight, voxel, tol=tol, max_iter=max_iter, check_every=check_every)
        screened = dict(screen=screen, screen_weight=weight, density=density)
    del rhs
    t0 = tick(seconds, "solve", t0)
    _, level, _ = sample(x, pts, origin, voxel)
    t0 = tick(seconds, "sample", t0)
    verts, faces, cells = _mesh.marching_cubes(x, level, (voxel,) * 3, timers=seconds, return_cells=True)
    if seconds is not None:
        seconds.pop("workspace_bytes", None)
    t0 = time.perf_counter()
    faces_before = int(faces.shape[0])
    if min_density:
        faces = faces[face_keep(field[3], cells, min_density).bool()]
        if faces.shape[0] == 0:
            raise ValueError(f"svs_poisson: no face is kept at min_density {min_density} ({faces_before} faces cross the level)")
        verts, faces = _mesh.compact(verts, faces)
    if largest:
        verts, faces = _mesh.largest_component(verts, faces)
    verts = (verts.double() + torch.as_tensor(origin, dtype=torch.float64, device=verts.device)).float()
    t0 = tick(seconds, "trim", t0)
    colors = None
    if rgb is not None:
        colors = nearest_colors(pts, to_device(rgb, torch.uint8, "poisson", "rgb", ndim=(2,)), verts, voxel)
        t0 = tick(seconds, "colors", t0)
    out = dict(verts=verts.cpu().numpy(), faces=faces.cpu().numpy(), rgb=None if colors is None else colors.cpu().numpy(),
               stats=dict(grid=tuple(dims), origin=origin, counted=counted, skipped=skipped, iterations=info["iterations"],
                          residual=info["residual"], converged=info["converged"], level=level, faces_before=faces_before,
                          faces_after=int(faces.shape[0]), **screened))
    tick(seconds, "download", t0)
    return out


def reconstruct_ply(ply_in, ply_out, voxel, pad=4, min_density=2.0, tol=1e-4, max_iter=None, bounds=None, largest=False, log=None,
                    screen=None):
    """The cloud file ply_in (`ply.read_points`, `ply.read_point_normals`: what `svs_hip.cloudclean` writes) meshed into
    ply_out (`ply.write`).  ValueError naming nx ny nz for a file without normals (`cloudclean.clean_ply` estimates them).
    screen: as in `reconstruct` (no default value; nobody has tried one on a real scan).
    -> `reconstruct`'s dict; its stats also hold files, launches and seconds per phase, and with screening on
    screened_launches (the svs_screened_* entries, which `launches` does not count)."""
    screen = check_screen(screen)
    sec = OrderedDict((k, 0.0) for k in PHASES)
    calls, screened_calls = dict(ENTRY_CALLS), dict(SCREENED_CALLS)
    t0 = time.perf_counter()
    xyz, rgb = _ply.read_points(ply_in)
    normals = _ply.read_point_normals(ply_in)
    if normals is None:
        raise ValueError(f"svs_poisson: {ply_in} has no nx ny nz properties: the cloud needs oriented normals "
                         "(python -m svs_hip.cloudclean writes them)")
    tick(sec, "read", t0)
    out = reconstruct(xyz, normals, rgb, voxel=voxel, pad=pad, min_density=min_density, tol=tol, max_iter=max_iter, bounds=bounds,
                      largest=largest, seconds=sec, screen=screen)
    t0 = time.perf_counter()
    os.makedirs(os.path.dirname(ply_out) or ".", exist_ok=True)
    _ply.write(ply_out, out["verts"], out["rgb"], out["faces"])
    tick(sec, "write", t0)
    st = out["stats"]
    st.update(files=dict(ply=ply_out), launches=launches_since(ENTRY_CALLS, calls), seconds=sec, n_verts=len(out["verts"]))
    if screen is not None:
        st.update(screened_launches=launches_since(SCREENED_CALLS, screened_calls))
    if log is not None:
        g = st["grid"]
        screened = "" if screen is None else f"screen {screen:g} (weight {st['screen_weight']:.6g}, {st['density']:.3g} points per touched node), "
        log(f"poisson: {ply_in}: {st['counted']} points counted, {st['skipped']} skipped, grid {g[0]} x {g[1]} x {g[2]}, " + screened
            + f"{st['iterations']} iterations to {st['residual']:.3g}" + ("" if st["converged"] else " (not converged)")
            + f", level {st['level']:.6g}, faces {st['faces_before']} -> {st['faces_after']} -> {ply_out}")
        log(seconds_line(sec))
    return out


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Meshes a point cloud with oriented normals on the GPU: grid Poisson surface "
                                            "reconstruction -> a PLY that evals.eval_dtu --mode mesh reads")
    p.add_argument("--ply", required=True, help="the cloud: a PLY with x y z nx ny nz [red green blue] (svs_hip.cloudclean's output)")
    p.add_argument("--ply-out", required=True, help="the mesh")
    p.add_argument("--voxel", type=float, required=True, help="node spacing in world units")
    p.add_argument("--pad", type=float, default=4.0, help="voxels of empty grid around the cloud's box")
    p.add_argument("--min-density", type=float, default=2.0, help="a face survives when the splat weights of its cell's eight "
                                                                  "nodes sum to this many points")
    p.add_argument("--tol", type=float, default=1e-4, help="relative residual the solve stops at")
    p.add_argument("--max-iter", type=int, default=None, help="iterations at most (default: 4 * the longest axis)")
    p.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                   help="the grid's box (default: the cloud's, padded)")
    p.add_argument("--largest", action="store_true", help="keep the largest component by area")
    p.add_argument("--raw", action="store_true", help="no trim: every face of the level set")
    p.add_argument("--screen", type=float, default=None, metavar="S",
                   help="screened reconstruction: the points also hold the solution at the level, with a weight of S over the "
                        "cloud's density (0 or absent: off).  No default value: 1, 4 and 16 were tried on a synthetic sphere of "
                        "uneven density only, none on a real scan")
    a = p.parse_args(argv)
    if not (a.voxel > 0 and math.isfinite(a.voxel)):
        p.error("--voxel must be positive")
    if not (0 < a.tol < 1):
        p.error("--tol lies in (0,1)")
    if a.max_iter is not None and a.max_iter < 1:
        p.error("--max-iter must be at least 1")
    if a.pad < 0 or a.min_density < 0:
        p.error("--pad and --min-density must not be negative")
    if a.screen is not None and not (a.screen >= 0 and math.isfinite(a.screen)):
        p.error("--screen must be finite and not negative")
    return a


def main(argv=None):
    a = parse_args(argv)
    return reconstruct_ply(a.ply, a.ply_out, a.voxel, pad=a.pad, min_density=None if a.raw else a.min_density, tol=a.tol,
                           max_iter=a.max_iter, bounds=a.bounds, largest=a.largest, log=print, screen=a.screen)


if __name__ == "__main__":
    main()
