"""DTU Chamfer evaluation on the HIP path (reference: evals/eval_dtu.py:52-196, modes 'pcd' and 'mesh'; SURVEY.md
section 8 row f4).

The reference is a command-line script around sklearn's kd-tree; the protocol is exposed here as functions on arrays
(`evaluate_scan`) and on the DTU file layout (`evaluate_scan_files`, `main`).  Every per-point step runs on the GPU
through the operators of svs_hip/clouds.py: greedy radius down-sampling, observation-mask filter, both nearest-neighbour
passes, the truncated means.  Only the file readers (svs_hip/ply.py, .mat) and the random shuffle of the input order are
host code.
"""
import argparse
import os

import numpy as np
import torch

from svs_hip import ply
from svs_hip.clouds import (compact, error_colors, mean_below, nearest_neighbor, obs_filter, plane_side, radius_downsample,
                            sample_mesh)
from svs_hip.images import to_device


def trun_n_d(n, d):
    return int(n * 10 ** d) / 10 ** d


def evaluate_scan(data_pcd, stl, ObsMask, BB, Res, ground_plane, downsample_density=0.2, patch_size=60, max_dist=20,
                  shuffle_rng=None, details=False, visualize=None):
    """evals/eval_dtu.py:99-192 for one scan -> (mean_d2s accuracy, mean_s2d completeness, overall) in mm.
    data_pcd (n,3): predicted cloud; stl (m,3): ground-truth scan; ObsMask (d0,d1,d2), BB (2,3), Res: ObsMask*.mat;
    ground_plane (4,): Plane*.mat 'P'.  shuffle_rng: numpy Generator for the reference's random index shuffle (:100-101;
    None = a fresh default_rng() like the reference, False = keep the given order).
    visualize=vis_dist: the result is followed by the details dict, which then also holds the error clouds of :173-187, the
    colours of data_down (`data_color`, `data_color_u8`) and of stl (`stl_color`, `stl_color_u8`)."""
    data_pcd = np.array(data_pcd, np.float64)
    if shuffle_rng is not False:
        (np.random.default_rng() if shuffle_rng is None else shuffle_rng).shuffle(data_pcd, axis=0)
    pts = to_device(data_pcd, torch.float64, "clouds")
    keep = radius_downsample(pts, downsample_density)
    data_down = compact(pts, keep)

    obs = torch.from_numpy(np.ascontiguousarray(np.asarray(ObsMask) != 0).astype(np.uint8)).to(pts.device)
    inbound, in_obs = obs_filter(data_down, BB, np.asarray(Res, np.float64).reshape(-1)[0], patch_size, obs)
    data_in = compact(data_down, inbound)
    data_in_obs = compact(data_down, in_obs)

    stl_d = to_device(stl, torch.float64, "clouds")
    dist_d2s = nearest_neighbor(stl_d, data_in_obs, max_dist)
    mean_d2s = mean_below(dist_d2s, max_dist)

    above = plane_side(stl_d, ground_plane)
    stl_above = compact(stl_d, above)
    dist_s2d = nearest_neighbor(data_in, stl_above, max_dist)
    mean_s2d = mean_below(dist_s2d, max_dist)
    over_all = (mean_d2s + mean_s2d) / 2
    if details or visualize is not None:
        d = dict(data_pcd=data_pcd, keep=keep, data_down=data_down, data_in=data_in, data_in_obs=data_in_obs, dist_d2s=dist_d2s,
                 stl_above=stl_above, dist_s2d=dist_s2d, in_obs=in_obs, above=above)
        if visualize is not None:
            d["stl"] = stl_d
            d["data_color"], d["data_color_u8"] = error_colors(dist_d2s, max_dist, visualize, select=in_obs)
            d["stl_color"], d["stl_color_u8"] = error_colors(dist_s2d, max_dist, visualize, select=above)
        return (mean_d2s, mean_s2d, over_all), d
    return mean_d2s, mean_s2d, over_all


def evaluate_scan_files(scan, datadir, dataset_dir, mode="pcd", **kw):
    """The reference's file layout (eval_dtu.py:59,121,139,158-161): {datadir}/mvsnet{scan:03}_l3.ply against
    {dataset_dir}/ObsMask/ObsMask{scan}_10.mat, Plane{scan}.mat (scan 82 uses Plane83) and Points/stl/stl{scan:03}_total.ply.
    mode 'mesh': the prediction is a triangle mesh, sampled at the down-sampling density first (:62-90)."""
    from scipy.io import loadmat
    pred = os.path.join(datadir, "mvsnet{:0>3}_l3.ply".format(scan))
    if mode == "mesh":
        vertices, triangles = ply.read_mesh(pred)
        data_pcd = sample_mesh(vertices, triangles, kw.get("downsample_density", 0.2)).cpu().numpy()
    else:
        data_pcd, _ = ply.read_points(pred)
    obs = loadmat(f"{dataset_dir}/ObsMask/ObsMask{scan}_10.mat")
    stl, _ = ply.read_points(f"{dataset_dir}/Points/stl/stl{scan:03}_total.ply")
    plane = loadmat(f"{dataset_dir}/ObsMask/Plane{83 if scan == 82 else scan}.mat")["P"]
    return evaluate_scan(data_pcd, stl, obs["ObsMask"], obs["BB"], obs["Res"], plane, **kw)


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--datadir', type=str, default='', help='pred point cloud')
    parser.add_argument('--data_dir_root', type=str, default='data_s_volsdf', help='GT data dir')
    parser.add_argument('--scan', type=int, default=-1)
    parser.add_argument('--mode', type=str, default='pcd', choices=['mesh', 'pcd'])
    parser.add_argument('--downsample_density', type=float, default=0.2)
    parser.add_argument('--patch_size', type=float, default=60)
    parser.add_argument('--max_dist', type=float, default=20)
    parser.add_argument('--visualize_threshold', type=float, default=10)
    parser.add_argument('-ve', '--visualize_error', action='store_true')
    args = parser.parse_args(argv)
    dataset_dir = os.path.join(args.data_dir_root, 'DTU', 'DTU_MVS_Data')
    scans = [21, 34, 38, 82, 24, 37, 40, 106, 110, 114, 118]
    if args.scan in scans:
        scans = [args.scan]
    results = []
    print("ply_name, accuracy(mm), completeness(mm), overall(mm)")
    for scan in scans:
        try:
            r = evaluate_scan_files(scan, args.datadir, dataset_dir, mode=args.mode, downsample_density=args.downsample_density,
                                    patch_size=args.patch_size, max_dist=args.max_dist,
                                    visualize=args.visualize_threshold if args.visualize_error else None)
            if args.visualize_error:                          # the error clouds of :169-187
                r, d = r
                vis_out_dir = os.path.join(args.datadir, 'result')
                os.makedirs(vis_out_dir, exist_ok=True)
                ply.write(f'{vis_out_dir}/vis_{scan:03}_d2s.ply', d["data_down"], d["data_color_u8"], coords="double")
                ply.write(f'{vis_out_dir}/vis_{scan:03}_s2d.ply', d["stl"], d["stl_color_u8"], coords="double")
        except (OSError, ValueError):
            r = (10000., 10000., 10000.)                      # the reference's fallback row (:163-167)
        print('scan{:0>3} {:.2f} {:.2f} {:.2f}'.format(scan, trun_n_d(r[0], 2), trun_n_d(r[1], 2), trun_n_d(r[2], 2)))
        results.append(list(r))
    results = np.array(results).mean(0)
    print('mean_err {:.3f} {:.3f} {:.3f}'.format(results[0], results[1], results[2]))
    return results


if __name__ == '__main__':
    main()
