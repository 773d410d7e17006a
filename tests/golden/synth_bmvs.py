"""Synthetic stand-in for one BlendedMVS Chamfer evaluation (the inputs of evals/eval_bmvs.py): seeded, so that the fixture
generator and the tests build the same scan."""
import numpy as np

from evals.eval_bmvs import RELATIVE_SCALE

HALF_AXES = np.array([150.0, 105.0, 75.0])        # the ground-truth ellipsoid, DTU millimetres
HOLE_Z = -40.0                                    # the prediction has nothing at or below this height


def make_bmvs_scan(seed, scan, n_pred=20000, n_gt=8000):
    """-> dict(data_pcd (n,3) float64, gt_pcd (n_gt,3) float64, relative_scale, scale_mat (4,4) or None), in the scan's own
    BlendedMVS units.  The ground truth is an ellipsoid shell; the prediction lies on the same shell with 1.5 mm noise, a
    tenth of it displaced by a further N(0, 25 mm) (errors on both sides of the 10 mm and 20 mm thresholds), and misses
    everything with z <= -40 mm (a hole: ground-truth points with no neighbour within 20 mm).  For scan 5 the prediction
    is stored in the frame that `scale_mat` -- a fixed similarity, scale 1.7 plus a translation -- maps back."""
    rng = np.random.default_rng(seed)
    rel = RELATIVE_SCALE[scan]

    def shell(n):
        d = rng.normal(0, 1, (n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return d * HALF_AXES

    gt = shell(n_gt)
    pred = shell(n_pred) + rng.normal(0, 1.5, (n_pred, 3))
    far = rng.permutation(n_pred)[:n_pred // 10]
    pred[far] += rng.normal(0, 25.0, (len(far), 3))
    pred = pred[pred[:, 2] > HOLE_Z]
    gt, pred = gt * rel, pred * rel
    scale_mat = None
    if scan == 5:
        scale_mat = np.eye(4)
        scale_mat[:3, :3] *= 1.7
        scale_mat[:3, 3] = np.array([0.31, -0.12, 0.07])
        pred = (pred - scale_mat[:3, 3]) / 1.7
    return dict(data_pcd=pred, gt_pcd=gt, relative_scale=rel, scale_mat=scale_mat)

