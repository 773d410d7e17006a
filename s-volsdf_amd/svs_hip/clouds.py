"""The operators on device point clouds: the Python faces of csrc/svs_cloud.hip, csrc/svs_chamfer.hip, the mesh sampler
(svs_mesh_sample_*) and csrc/svs_cloudknn.hip (k neighbours, outlier scores, normals: what `svs_hip.cloudclean` is written in).  Both Chamfer evaluators (evals/eval_dtu.py, evals/eval_bmvs.py) are written in these; the files under
evals/ keep what mirrors the reference's scripts (protocol, file layout, flags).  Clouds are (n,3) float64 device tensors
unless a function says otherwise; arrays and host tensors are uploaded (`images.to_device`).
"""
import ctypes

import numpy as np
import torch

from . import lib as _lib
from .images import device, to_device
from .ops import _ptr, _stream


def _origin(clouds, pad):
    """Padded bounding box of the clouds (one library call per cloud, one read-back for all)."""
    L = _lib.load()
    clouds = [c for c in clouds if c.shape[0]]
    dev = clouds[0].device
    ws = torch.empty(L.svs_cloud_bounds_workspace_bytes() // 8, dtype=torch.float64, device=dev)
    box = torch.empty(len(clouds), 6, dtype=torch.float64, device=dev)
    for k, c in enumerate(clouds):
        _lib.check(L.svs_cloud_bounds(_ptr(c), c.shape[0], _ptr(ws), _ptr(box[k]), _stream()), "svs_cloud_bounds")
    box = box.cpu().numpy()
    return box[:, :3].min(0) - pad, box[:, 3:].max(0) + pad


def nearest_neighbor(ref, query, max_radius, cell=None, return_index=False):
    """dist (nq,) float64 [, idx (nq,) int32]: NearestNeighbors(n_neighbors=1).fit(ref).kneighbors(query) for
    neighbours closer than max_radius (larger results are upper bounds, inf if nothing is near)."""
    L = _lib.load()
    ref, query = to_device(ref, torch.float64, "clouds"), to_device(query, torch.float64, "clouds")
    nr, nq = ref.shape[0], query.shape[0]
    dist = torch.empty(nq, dtype=torch.float64, device=ref.device)
    idx = torch.empty(nq, dtype=torch.int32, device=ref.device) if return_index else None
    if nr == 0:
        raise ValueError("Found array with 0 sample(s) while a minimum of 1 is required by NearestNeighbors.")   # sklearn's fit
    if nq == 0:
        return (dist, idx) if return_index else dist
    lo, hi = _origin([ref, query], 1e-6)
    if cell is None:
        # about two points per cell of the surface the cloud samples; never more than 2^20 cells per axis
        ext = float((hi - lo).max())
        cell = max(ext / (1 << 20), min(max_radius, 2.0 * ext / max(nr, 1) ** 0.5))
    ws = torch.empty(L.svs_cloud_grid_bytes(nr), dtype=torch.uint8, device=ref.device)
    org = (ctypes.c_double * 3)(*[float(v) for v in lo])
    _lib.check(L.svs_cloud_nn(_ptr(ref), nr, _ptr(query), nq, org, float(cell), float(max_radius), _ptr(ws), _ptr(dist), _ptr(idx),
                              _stream()), "svs_cloud_nn")
    return (dist, idx) if return_index else dist


def sample_mesh(vertices, triangles, thresh):
    """The cloud the reference's mesh mode evaluates (evals/eval_dtu.py:65-90): the vertices followed by the points of a
    regular grid on every triangle of non-zero area, spaced so that the samples are about `thresh` apart.  The
    per-triangle quantities are the script's numpy expressions; the points come from the library.  Returns (n,3) float64
    on the device."""
    L = _lib.load()
    vertices = np.asarray(vertices, np.float64)
    tri_vert = vertices[np.asarray(triangles)]
    v1 = tri_vert[:, 1] - tri_vert[:, 0]
    v2 = tri_vert[:, 2] - tri_vert[:, 0]
    l1 = np.linalg.norm(v1, axis=-1, keepdims=True)
    l2 = np.linalg.norm(v2, axis=-1, keepdims=True)
    area2 = np.linalg.norm(np.cross(v1, v2), axis=-1, keepdims=True)
    non_zero_area = (area2 > 0)[:, 0]
    l1, l2, area2, v1, v2, tri_vert = [arr[non_zero_area] for arr in [l1, l2, area2, v1, v2, tri_vert]]
    thr = thresh * np.sqrt(l1 * l2 / area2)
    n1 = np.floor(l1 / thr)
    n2 = np.floor(l2 / thr)
    verts_d = to_device(vertices, torch.float64, "clouds")
    n_tri = len(n1)
    if n_tri == 0:
        return verts_d
    if not (np.isfinite(n1).all() and np.isfinite(n2).all()):
        raise ValueError("sample_mesh: a triangle's sample counts are not finite")
    rec = torch.from_numpy(np.ascontiguousarray(np.concatenate([n1, n2, v1, v2, tri_vert[:, 0]], 1))).to(device("clouds"))
    counts = torch.empty(n_tri, dtype=torch.int64, device=rec.device)
    _lib.check(L.svs_mesh_sample_count(_ptr(rec), n_tri, _ptr(counts), _stream()), "svs_mesh_sample_count")
    ends = torch.cumsum(counts, 0)
    offsets = (ends - counts).contiguous()
    total = int(ends[-1].item())
    out = torch.empty(verts_d.shape[0] + total, 3, dtype=torch.float64, device=rec.device)
    out[:verts_d.shape[0]] = verts_d
    new_pts = out[verts_d.shape[0]:]
    if total:
        _lib.check(L.svs_mesh_sample_points(_ptr(rec), n_tri, _ptr(offsets), _ptr(new_pts), _stream()), "svs_mesh_sample_points")
    return out


def radius_downsample(pts, radius):
    """Boolean keep-mask (n,) of the greedy radius down-sampling in index order (eval_dtu.py:104-118)."""
    L = _lib.load()
    pts = to_device(pts, torch.float64, "clouds")
    n = pts.shape[0]
    state = torch.empty(n, dtype=torch.uint8, device=pts.device)
    if n == 0:
        return state.bool()
    lo, hi = _origin([pts], 1e-6)
    if float((hi - lo).max()) / radius >= (1 << 21):
        raise ValueError("cloud extent / radius exceeds the 2^21 cells per axis of the grid")
    ws = torch.empty(L.svs_cloud_grid_bytes(n), dtype=torch.uint8, device=pts.device)
    org = (ctypes.c_double * 3)(*[float(v) for v in lo])
    open_ = torch.zeros(1, dtype=torch.int32, device=pts.device)
    _lib.check(L.svs_cloud_downsample_begin(_ptr(pts), n, org, float(radius), _ptr(ws), _ptr(state), _stream()),
               "svs_cloud_downsample_begin")
    for _ in range(n + 1):
        _lib.check(L.svs_cloud_downsample_round(org, n, float(radius), _ptr(ws), _ptr(state), _ptr(open_), _stream()),
                   "svs_cloud_downsample_round")
        if int(open_.item()) == 0:
            break
    return state == 1


def compact(pts, mask):
    L = _lib.load()
    pts = to_device(pts, torch.float64, "clouds")
    n = pts.shape[0]
    mask = mask.to(torch.uint8).contiguous()
    out = torch.empty_like(pts)
    ws = torch.empty(max(n, 1), dtype=torch.int32, device=pts.device)
    count = torch.zeros(1, dtype=torch.int32, device=pts.device)
    _lib.check(L.svs_cloud_compact(_ptr(pts), _ptr(mask), n, _ptr(ws), _ptr(out), _ptr(count), _stream()), "svs_cloud_compact")
    return out[:int(count.item())]


def mean_below(dist, max_dist):
    L = _lib.load()
    ws = torch.empty(L.svs_cloud_mean_workspace_bytes() // 8, dtype=torch.float64, device=dist.device)
    out = torch.empty(2, dtype=torch.float64, device=dist.device)
    _lib.check(L.svs_cloud_mean_below(_ptr(dist), dist.shape[0], float(max_dist), _ptr(ws), _ptr(out), _stream()), "svs_cloud_mean_below")
    return float(out[0].item())


def obs_filter(points, BB, res, patch_size, obs):
    """The observation-mask filter of eval_dtu.py:124-135 -> (inbound (n,) uint8: inside BB padded by patch_size, in_obs (n,)
    uint8: inbound and on a set voxel of obs).  BB (2,3) float32, res: the voxel size, obs (d0,d1,d2) uint8 on the device."""
    n = points.shape[0]
    inbound = torch.empty(n, dtype=torch.uint8, device=points.device)
    in_obs = torch.empty(n, dtype=torch.uint8, device=points.device)
    bb = (ctypes.c_float * 6)(*[float(v) for v in np.asarray(BB, np.float32).reshape(-1)])
    _lib.check(_lib.load().svs_cloud_obs_filter(_ptr(points), n, bb, float(res), float(patch_size), _ptr(obs), *obs.shape,
                                                _ptr(inbound), _ptr(in_obs), _stream()), "svs_cloud_obs_filter")
    return inbound, in_obs


def plane_side(points, plane):
    """above (n,) uint8: the points on the positive side of plane (4,) (eval_dtu.py:145-146)"""
    above = torch.empty(points.shape[0], dtype=torch.uint8, device=points.device)
    p = (ctypes.c_double * 4)(*[float(v) for v in np.asarray(plane, np.float64).reshape(-1)])
    _lib.check(_lib.load().svs_cloud_plane_side(_ptr(points), points.shape[0], p, _ptr(above), _stream()), "svs_cloud_plane_side")
    return above


def _raw_cloud(a):
    """(n,3) on the device in the dtype the file gave: float32 stays float32 (half the upload), the rest is float64"""
    if not torch.is_tensor(a):
        a = np.asarray(a)
        a = torch.from_numpy(np.ascontiguousarray(a, np.float32 if a.dtype == np.float32 else np.float64))
    a = a.detach().to(device("clouds"))
    return (a if a.dtype in (torch.float32, torch.float64) else a.to(torch.float64)).reshape(-1, 3).contiguous()


def prepare_cloud(pts, relative_scale, scale_mat=None):
    """The cloud the kd-tree sees, (n,3) float64 on the device: `.astype('float32')`, [scan 5: the (4,4) scale_mat,]
    `/= relative_scale` (evals/eval_bmvs.py:127-134,187,196-197)."""
    L = _lib.load()
    pts = _raw_cloud(pts)
    out = torch.empty(pts.shape[0], 3, dtype=torch.float64, device=pts.device)
    mat = None
    if scale_mat is not None:
        m = np.ascontiguousarray(np.asarray(scale_mat, np.float64))
        if m.shape != (4, 4):
            raise ValueError("Transformation matrix must be (4, 4)!")
        mat = (ctypes.c_double * 16)(*m.reshape(-1))
    _lib.check(L.svs_cloud_prepare(_ptr(pts), int(pts.dtype == torch.float64), pts.shape[0], mat, float(relative_scale), _ptr(out),
                                   _stream()), "svs_cloud_prepare")
    return out


def error_colors(dist, max_dist=20, vis_dist=10, select=None):
    """The colour step of both scripts (evals/eval_bmvs.py:232-246, evals/eval_dtu.py:173-187) -> (rgb_f64 (n,3) float64,
    rgb_u8 (n,3) uint8) on the device.  White to red up to vis_dist, red up to max_dist, green from max_dist on.
    select (n,): the rows of the full cloud that `dist` belongs to, in order; the others are blue."""
    L = _lib.load()
    dist = to_device(dist, torch.float64, "clouds")
    rank = None
    if select is not None:
        select = select.detach().to(device=dist.device)
        select = (select if select.dtype == torch.uint8 else (select != 0).to(torch.uint8)).contiguous()
        chosen = (select != 0).to(torch.int32)
        rank = torch.cumsum(chosen, 0, dtype=torch.int32) - chosen          # selected rows before each row
    n_full = dist.shape[0] if select is None else select.shape[0]
    rgb = torch.empty(n_full, 3, dtype=torch.float64, device=dist.device)
    rgb_u8 = torch.empty(n_full, 3, dtype=torch.uint8, device=dist.device)
    _lib.check(L.svs_cloud_error_colors(_ptr(dist), dist.shape[0], _ptr(select), _ptr(rank), n_full, float(max_dist), float(vis_dist),
                                        _ptr(rgb), _ptr(rgb_u8), _stream()), "svs_cloud_error_colors")
    return rgb, rgb_u8


# ---- k nearest neighbours, statistical outliers, normals (csrc/svs_cloudknn.hip) ----------------------------------------------
KNN_MAX_K = 32


def knn_cell(lo, hi, n_ref, k, max_radius=None):
    """The default cell size of `knn`: `nearest_neighbor`'s (2 ext / sqrt(n): about two points per cell of the surface the
    cloud samples) times sqrt(k) / 2, i.e. ext * sqrt(k / n) -- about k points per cell of a surface cloud, so that the ring
    of radius one cell around the query (pi k points) nearly always completes the list; never more than max_radius, never
    more than 2^20 cells per axis.  lo, hi: the box of both clouds, ext its longest side."""
    ext = float((np.asarray(hi) - np.asarray(lo)).max())
    cell = ext * (k / max(n_ref, 1)) ** 0.5
    if max_radius is not None:
        cell = min(float(max_radius), cell)
    return max(ext / (1 << 20), cell, 1e-300)


def _search_radius(lo, hi, max_radius):
    """max_radius, or twice the diagonal of the box when that is smaller: no two points of the box are that far apart, so
    the neighbours are the same, and the rings a search may walk stay bounded by the box"""
    return min(float(max_radius), 2.0 * float(np.linalg.norm(np.asarray(hi) - np.asarray(lo))))


def _knn(ref, query, k, max_radius, exclude_same_index, cell, chunk, records, want_mean):
    L = _lib.load()
    same = query is ref
    ref = to_device(ref, torch.float64, "clouds")
    query = ref if same else to_device(query, torch.float64, "clouds")
    nr, nq, k = ref.shape[0], query.shape[0], int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"knn: k must be in [1,{KNN_MAX_K}], got {k}")
    if not max_radius > 0:
        raise ValueError(f"knn: max_radius must be positive, got {max_radius}")
    dev = ref.device
    dist = torch.full((nq, k), float("inf"), dtype=torch.float64, device=dev) if records else None
    idx = torch.full((nq, k), -1, dtype=torch.int32, device=dev) if records else None
    mean = torch.full((nq,), float("inf"), dtype=torch.float64, device=dev) if want_mean else None
    if nq and nr:
        lo, hi = _origin([ref] if same else [ref, query], 1e-6)
        if cell is None:
            cell = knn_cell(lo, hi, nr, k, max_radius)
        ws = torch.empty(L.svs_cloud_grid_bytes(nr), dtype=torch.uint8, device=dev)
        org = (ctypes.c_double * 3)(*[float(v) for v in lo])
        chunk, radius = max(int(chunk), 1), _search_radius(lo, hi, max_radius)
        for a in range(0, nq, chunk):
            b = min(a + chunk, nq)
            _lib.check(L.svs_cloud_knn(_ptr(ref), nr, _ptr(query[a:b]), b - a, org, float(cell), k, radius,
                                       1 + a if exclude_same_index else 0, _ptr(ws), _ptr(dist[a:b]) if records else None,
                                       _ptr(idx[a:b]) if records else None, _ptr(mean[a:b]) if want_mean else None, _stream()),
                       "svs_cloud_knn")
    return dist, idx, mean


def knn(ref, query, k, max_radius, exclude_same_index=False, cell=None, return_mean=False, chunk=1 << 20):
    """The k nearest points of `ref` to every point of `query`, 1 <= k <= 32 -> (dist (nq,k) float64 ascending, idx (nq,k)
    int32 [, mean (nq,) float64]) on the device.  Neighbours are ordered by (squared distance, index): ties go to the lower
    index.  A slot whose neighbour is not strictly closer than max_radius, or that does not exist (fewer than k points),
    holds inf / -1; mean is the mean of a row's finite slots, inf if it has none.  exclude_same_index: `query` is `ref`
    (or its first rows) and a point is not its own neighbour.  cell: the grid's cell size, default `knn_cell` (the rule is
    stated there); the result does not depend on it.  Queries go to the library `chunk` rows at a time; a cloud against
    itself (`query is ref`) in ONE call is walked in the grid's sorted order, which is faster when its rows are in no spatial
    order."""
    dist, idx, mean = _knn(ref, query, k, max_radius, exclude_same_index, cell, chunk, True, return_mean)
    return (dist, idx, mean) if return_mean else (dist, idx)


def knn_mean(pts, k, max_radius, cell=None, chunk=1 << 20):
    """mean (n,) float64 of `knn(pts, pts, k, max_radius, exclude_same_index=True, return_mean=True)` alone: the n * k
    records are not written."""
    pts = to_device(pts, torch.float64, "clouds")
    return _knn(pts, pts, k, max_radius, True, cell, chunk, False, True)[2]


def default_radius(pts, k):
    """The search radius the cleaning functions take when none is given: four of `knn_cell`'s cells, about 4 sqrt(k) point
    spacings of a surface cloud.  A point with fewer than k neighbours inside it is averaged over those it has."""
    pts = to_device(pts, torch.float64, "clouds")
    if pts.shape[0] == 0:
        return 1.0
    lo, hi = _origin([pts], 1e-6)
    return 4.0 * knn_cell(lo, hi, pts.shape[0], k)


def outlier_stats(mean):
    """dict(count, mean, std) over the finite entries of mean (n,) float64: sample standard deviation (count - 1), 0 below
    two entries; one fixed summation order."""
    L = _lib.load()
    mean = to_device(mean, torch.float64, "clouds")
    if mean.shape[0] == 0:
        return dict(count=0, mean=0.0, std=0.0)
    ws = torch.empty(L.svs_cloud_outlier_workspace_bytes() // 8, dtype=torch.float64, device=mean.device)
    out = torch.empty(3, dtype=torch.float64, device=mean.device)
    _lib.check(L.svs_cloud_outlier_stats(_ptr(mean), mean.shape[0], _ptr(ws), _ptr(out), _stream()), "svs_cloud_outlier_stats")
    c, m, s = out.cpu().tolist()
    return dict(count=int(c), mean=m, std=s)


def threshold_mask(mean, threshold):
    """keep (n,) bool: mean <= threshold, False for an entry that is not finite"""
    L = _lib.load()
    mean = to_device(mean, torch.float64, "clouds")
    keep = torch.empty(mean.shape[0], dtype=torch.uint8, device=mean.device)
    if mean.shape[0] == 0:
        return keep != 0
    _lib.check(L.svs_cloud_outlier_mask(_ptr(mean), mean.shape[0], float(threshold), _ptr(keep), _stream()), "svs_cloud_outlier_mask")
    return keep != 0


def outlier_mask(pts, k=20, std_ratio=2.0, max_radius=None):
    """Statistical outlier removal: a point's score is the mean distance to its k nearest other points (those closer than
    max_radius, default `default_radius`); it is kept when score <= mean + std_ratio * std of the finite scores.  A point
    with no neighbour inside max_radius is dropped.  -> (keep (n,) bool on the device, dict(count, mean, std, threshold,
    max_radius, k, std_ratio))"""
    pts = to_device(pts, torch.float64, "clouds")
    if max_radius is None:
        max_radius = default_radius(pts, k)
    mean = knn_mean(pts, k, max_radius, chunk=max(pts.shape[0], 1))      # one call: the library walks the cloud in sorted order
    stats = outlier_stats(mean)
    stats.update(threshold=stats["mean"] + std_ratio * stats["std"], max_radius=float(max_radius), k=int(k), std_ratio=float(std_ratio))
    return threshold_mask(mean, stats["threshold"]), stats


def normals_from_neighbors(pts, idx, include_self=True, view_index=None, centres=None):
    """(normals (n,3) float32 unit, curvature (n,) float32) from the neighbour table idx (n,k) int32 of `knn` (-1: none):
    the eigenvector of the smallest eigenvalue l0 of the covariance of the neighbours (and the point), curvature l0 / (l0 +
    l1 + l2).  centres (n_views,3): the normal faces centres[view_index[i]], or the nearest centre without view_index; None:
    the sign is the solver's.  Fewer than three points: zeros."""
    L = _lib.load()
    pts = to_device(pts, torch.float64, "clouds")
    idx = to_device(idx, torch.int32, "clouds")
    n = pts.shape[0]
    if idx.ndim != 2 or idx.shape[0] != n:
        raise ValueError(f"idx: expected ({n},k), got {tuple(idx.shape)}")
    if view_index is not None and centres is None:
        raise ValueError("view_index needs centres")
    c = None if centres is None else to_device(centres, torch.float64, "clouds").reshape(-1, 3)
    v = None
    if view_index is not None:
        v = to_device(view_index, torch.int32, "clouds").reshape(-1)
        if v.shape[0] != n:
            raise ValueError(f"{v.shape[0]} view indices for {n} points")
    normals = torch.zeros(n, 3, dtype=torch.float32, device=pts.device)
    curvature = torch.zeros(n, dtype=torch.float32, device=pts.device)
    if n:
        _lib.check(L.svs_cloud_normals(_ptr(pts), n, _ptr(idx), idx.shape[1], int(bool(include_self)), _ptr(v), _ptr(c),
                                       0 if c is None else c.shape[0], _ptr(normals), _ptr(curvature), _stream()), "svs_cloud_normals")
    return normals, curvature


def estimate_normals(pts, k=16, max_radius=None, view_index=None, centres=None):
    """PCA normals over a point and its k nearest neighbours (closer than max_radius, default `default_radius`) ->
    (normals (n,3) float32, curvature (n,) float32) on the device; orientation as `normals_from_neighbors`."""
    pts = to_device(pts, torch.float64, "clouds")
    if max_radius is None:
        max_radius = default_radius(pts, k)
    _, idx = knn(pts, pts, k, max_radius, exclude_same_index=True, chunk=max(pts.shape[0], 1))      # (one call: the sorted walk)
    return normals_from_neighbors(pts, idx, True, view_index, centres)
