"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the BlendedMVS Chamfer protocol (evals/eval_bmvs.py:127-134,187-246) and
of the colour step that evals/eval_dtu.py:173-187 shares with it: numpy for the bookkeeping, scikit-learn's kd-tree for the
searches, called as the script calls it.  PINNED by tests/golden/chamfer_bmvs_ref.npz, the reference's two scripts run end
to end on synthetic scans (tests/golden/make_bmvs_chamfer_fixture.py).  Only tests and tools/bench_chamfer_bmvs.py --host
import this module.
"""
import numpy as np
import sklearn.neighbors as skln


def prepare(pts, relative_scale, scale_mat=None):
    """(n,3) float64: `.astype('float32')`, [scan 5: scale_mat,] `/= relative_scale` (:127-134,187,196-197).  A float32
    array divided in place by a Python float is divided in float32; with scale_mat the cloud is float64 from the product on,
    whose sums are written here left to right (the script's np.dot leaves their order to the host's BLAS)."""
    x = np.asarray(pts).astype('float32')
    if scale_mat is None:
        return (x / np.float32(relative_scale)).astype(np.float64)
    m = np.asarray(scale_mat, np.float64)
    p = x.astype(np.float64)
    t = np.stack([((m[a, 0] * p[:, 0] + m[a, 1] * p[:, 1]) + m[a, 2] * p[:, 2]) + m[a, 3] for a in range(3)], 1)
    return t / relative_scale


def nn_distance(ref, query, n_jobs):
    """:204-211 / :219-220 -> dist (nq,)"""
    nn_engine = skln.NearestNeighbors(n_neighbors=1, radius=0.2, algorithm='kd_tree', n_jobs=n_jobs)
    nn_engine.fit(ref)
    d, _ = nn_engine.kneighbors(query, n_neighbors=1, return_distance=True)
    return d[:, 0]


def evaluate_scan(data_pcd, gt_pcd, relative_scale, scale_mat=None, max_dist=20, n_jobs=2):
    """:127-223,251 after the shuffle (data_pcd is taken in the given order)."""
    data = prepare(data_pcd, relative_scale, scale_mat)
    gt = prepare(gt_pcd, relative_scale)
    dist_d2s = nn_distance(gt, data, n_jobs)
    mean_d2s = dist_d2s[dist_d2s < max_dist].mean()
    dist_s2d = nn_distance(data, gt, n_jobs)
    mean_s2d = dist_s2d[dist_s2d < max_dist].mean()
    return (mean_d2s, mean_s2d, (mean_d2s + mean_s2d) / 2), dict(data_pcd=data, gt_pcd=gt, dist_d2s=dist_d2s, dist_s2d=dist_s2d)


def colors_u8(c):
    """what the error cloud's PLY stores of a colour in [0, 1]"""
    return np.rint(np.clip(c, 0.0, 1.0) * 255.0).astype(np.uint8)


def error_colors(dist, max_dist=20, vis_dist=10, select=None):
    """eval_bmvs.py:232-246 (select None) and eval_dtu.py:173-187 (select: mask over the full cloud of the rows `dist`
    belongs to) -> (rgb float64, rgb uint8)."""
    R = np.array([[1, 0, 0]], dtype=np.float64)
    G = np.array([[0, 1, 0]], dtype=np.float64)
    B = np.array([[0, 0, 1]], dtype=np.float64)
    W = np.array([[1, 1, 1]], dtype=np.float64)
    dist = np.asarray(dist, np.float64).reshape(-1, 1)
    alpha = dist.clip(max=vis_dist) / vis_dist
    color = R * alpha + W * (1 - alpha)
    color[dist[:, 0] >= max_dist] = G
    if select is not None:
        full = np.tile(B, (len(select), 1))
        full[np.where(np.asarray(select) != 0)[0]] = color
        color = full
    return color, colors_u8(color)


def color_classes(rgb):
    """-> counts (blue, green, saturated, graded) of an (n,3) colour array, float64 or uint8: not evaluated; d >= max_dist;
    vis_dist <= d < max_dist (pure red); d < vis_dist (white to red)."""
    rgb = np.asarray(rgb)
    rgb = rgb / 255.0 if rgb.dtype == np.uint8 else rgb.astype(np.float64)
    blue = (rgb == [0, 0, 1]).all(1)
    green = (rgb == [0, 1, 0]).all(1)
    sat = (rgb == [1, 0, 0]).all(1)
    return np.array([blue.sum(), green.sum(), sat.sum(), len(rgb) - blue.sum() - green.sum() - sat.sum()], np.int64)
