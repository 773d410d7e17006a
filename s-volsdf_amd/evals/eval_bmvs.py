"""BlendedMVS Chamfer evaluation on the HIP path (reference: evals/eval_bmvs.py:56-79,102-252), with its
error clouds (`-ve/--visualize_error`).

The reference brings a BlendedMVS cloud to the DTU scale (`relative_scale = cam_scale_mat[scan] / cam_scale_DTU`) and
then follows the DTU settings (max_dist = 20) without down-sampling or masks.  As in evals/eval_dtu.py the protocol is
exposed as functions on arrays (`evaluate_scan`), on the file layout (`evaluate_scan_files`) and as `main(argv)` with the
script's flags.  Every per-point step runs on the GPU through the operators of svs_hip/clouds.py: the float32 bookkeeping
of the clouds (`prepare_cloud`), the searches and means, the colour step (`error_colors`).  Host code: the PLY reader and
writer (svs_hip/ply.py) and the random order of the prediction.
"""
import argparse
import os
import sys

import numpy as np
import torch

from svs_hip import ply
from svs_hip.clouds import error_colors, mean_below, nearest_neighbor, prepare_cloud
from svs_hip.scans import scan2hash  # noqa: F401  -- re-exported, as the reference's module defines it

# relative_scale of evals/eval_bmvs.py:115: BlendedMVS scale_mat_0[0,0] of scans 1..9 over DTU scan114's (`get_scales`)
RELATIVE_SCALE = {1: 0.0010051393651899145, 2: 0.0015733906993148704, 3: 0.0012326845045689896, 4: 0.0015294108512811993,
                  5: 0.007349738091050388, 6: 0.01192223325424887, 7: 0.001284409757598681, 8: 0.0014762879597404273,
                  9: 0.022978406132555827}
SCANS = (1, 2, 3, 4, 5, 6, 7, 8, 9)
MATRIX_SCAN = 5            # the one scan whose prediction goes through its scale_mat first (:129-134)


def get_scales(data_dir_root):
    """evals/eval_bmvs.py:56-79 -> (DTU_scale, {scan: BlendedMVS scale}, {scan: ratio}) from the cameras.npz files."""
    def scale(data_dir, scan_id):
        cams = np.load(os.path.join(data_dir_root, data_dir, f"scan{scan_id}", "cameras.npz"))
        assert cams["scale_mat_0"].astype(np.float32)[0, 0] == cams["scale_mat_1"].astype(np.float32)[0, 0]
        return cams["scale_mat_0"].astype(np.float64)[0, 0]
    dtu_scale = scale("DTU", 114)
    bmvs_scale = {scan_id: scale("BlendedMVS", scan_id) for scan_id in SCANS}
    return dtu_scale, bmvs_scale, {scan_id: s / dtu_scale for scan_id, s in bmvs_scale.items()}


def shuffle_rows(pts, shuffle_rng=None):
    """`np.random.default_rng().shuffle(pts, axis=0)` (:201-202) as an index shuffle: the same draws, so the same order.
    shuffle_rng: None = unseeded like the script, False = keep the order."""
    if shuffle_rng is False:
        return pts
    perm = np.arange(len(pts))
    (np.random.default_rng() if shuffle_rng is None else shuffle_rng).shuffle(perm)
    return pts[torch.from_numpy(perm).to(pts.device)] if torch.is_tensor(pts) else np.asarray(pts)[perm]


def evaluate_scan(data_pcd, gt_pcd, relative_scale, scale_mat=None, max_dist=20, shuffle_rng=None, details=False):
    """evals/eval_bmvs.py:127-134,187-223,251 for one scan -> (mean_d2s, mean_s2d, over_all) in DTU millimetres.
    data_pcd (n,3): the prediction; gt_pcd (m,3): the ground-truth samples; scale_mat: scan 5's (4,4) matrix, applied to
    the prediction only.  details=True adds a dict: the prepared clouds and both distance arrays, on the device."""
    data = prepare_cloud(shuffle_rows(data_pcd, shuffle_rng), relative_scale, scale_mat)
    gt = prepare_cloud(gt_pcd, relative_scale)
    if data.shape[0] == 0 or gt.shape[0] == 0:               # sklearn's fit / kneighbors, caught by the script (:209-222)
        raise ValueError("Found array with 0 sample(s) while a minimum of 1 is required by NearestNeighbors.")
    dist_d2s = nearest_neighbor(gt, data, max_dist)
    mean_d2s = mean_below(dist_d2s, max_dist)
    dist_s2d = nearest_neighbor(data, gt, max_dist)
    mean_s2d = mean_below(dist_s2d, max_dist)
    over_all = (mean_d2s + mean_s2d) / 2
    if details:
        return (mean_d2s, mean_s2d, over_all), dict(data_pcd=data, gt_pcd=gt, dist_d2s=dist_d2s, dist_s2d=dist_s2d)
    return mean_d2s, mean_s2d, over_all


def evaluate_scan_files(scan, datadir, data_dir_root, no_crop=False, visualize_error=False, **kw):
    """The reference's file layout (:114,125,131-133,139,183-184,230,241,246): {datadir}/mvsnet{scan:03}_l3.ply against
    {data_dir_root}/BlendedMVS/stl/scan{scan}_crop.ply (scan{scan}.ply with no_crop); scan 5 reads scale_mat_0 of
    {data_dir_root}/BlendedMVS/scan5/cameras.npz.  visualize_error writes {datadir}/result/{scan}_d2s.ply (the prediction
    in its shuffled order) and {scan}_s2d.ply (the ground truth)."""
    data_pcd, _ = ply.read_points(os.path.join(datadir, "mvsnet{:0>3}_l3.ply".format(scan)))
    scale_mat = None
    if scan == MATRIX_SCAN:
        scale_mat = np.load(os.path.join(data_dir_root, "BlendedMVS", f"scan{scan}", "cameras.npz"))["scale_mat_0"]
    gt_file = os.path.join(data_dir_root, "BlendedMVS", "stl", f"scan{scan}.ply" if no_crop else f"scan{scan}_crop.ply")
    assert os.path.exists(gt_file), gt_file
    gt_pcd, _ = ply.read_points(gt_file)
    want_details = kw.pop("details", False)
    res, d = evaluate_scan(data_pcd, gt_pcd, RELATIVE_SCALE[scan], scale_mat=scale_mat, details=True, **kw)
    if visualize_error:
        vis_out_dir = os.path.join(datadir, "result")
        os.makedirs(vis_out_dir, exist_ok=True)
        max_dist = kw.get("max_dist", 20)
        ply.write(f"{vis_out_dir}/{scan}_d2s.ply", d["data_pcd"], error_colors(d["dist_d2s"], max_dist, 10)[1], coords="double")
        ply.write(f"{vis_out_dir}/{scan}_s2d.ply", d["gt_pcd"], error_colors(d["dist_s2d"], max_dist, 10)[1], coords="double")
    return (res, d) if want_details else res


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--sample', type=int, default=100000)
    parser.add_argument('--scan', type=int, default=-1)
    parser.add_argument('--datadir', type=str, default='', help='pred point cloud')
    parser.add_argument('--dataset_dir', type=str, default='bmvs/dataset_textured_meshes', help='GT mesh')
    parser.add_argument('--data_dir_root', type=str, default='data_s_volsdf', help='GT data dir')
    parser.add_argument('--save_gt', action='store_true')
    parser.add_argument('-ve', '--visualize_error', action='store_true')
    parser.add_argument('--no_crop', action='store_true', help='NOT [eval only above the ground plane & using object masks]')
    args = parser.parse_args(argv)
    if args.save_gt:
        sys.exit("--save_gt is not provided: it samples the BlendedMVS textured meshes with open3d's unseeded sampler; "
                 "the data package already holds the sampled clouds under BlendedMVS/stl/")
    scans = list(SCANS)
    if args.scan in scans:
        scans = [args.scan]
    results = {}
    print("ply_name, chamfer(mm)")
    for scan in scans:
        try:
            r = evaluate_scan_files(scan, args.datadir, args.data_dir_root, no_crop=args.no_crop, visualize_error=args.visualize_error)
        except (OSError, ValueError):
            continue                                          # a missing or empty cloud: the script's `except: continue`
        print('scan{:0>3} {:.2f} {:.2f} {:.2f}'.format(scan, r[0], r[1], r[2]))
        results[scan] = r
    return results


if __name__ == '__main__':
    main()
