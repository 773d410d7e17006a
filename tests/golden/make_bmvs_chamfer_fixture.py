"""Generator of tests/golden/chamfer_bmvs_ref.npz: the REFERENCE's evaluation scripts themselves, run as __main__ through
runpy on synthetic scans laid out in their directory structure, with --visualize_error.

    python tests/golden/make_bmvs_chamfer_fixture.py

  evals/eval_bmvs.py  on synth_bmvs.make_bmvs_scan for scans 4 and 5 (5 is the scan that goes through scale_mat_0)
  evals/eval_dtu.py   on synth.make_dtu_scan(31), the scan of chamfer_ref.npz, for the error clouds of that script

Substitutions, none in the algorithm: open3d (not installed) is a stub whose read_point_cloud parses the binary PLYs written
below with numpy and whose write_point_cloud records the points and colours it is given; trimesh (not installed) is a stub
whose transformations.transform_points is trimesh's own expression, np.dot(matrix, [p;1].T).T[:, :3]; the scripts' unseeded
np.random.default_rng() is seeded so that the shuffled order can be stored.  Arrays only are stored, no reference source.
"""
import contextlib
import io
import os
import runpy
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "s-volsdf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import bmvs_chamfer_oracle as borc  # noqa: E402
import ref_shim                     # noqa: E402
import synth                        # noqa: E402
import synth_bmvs                   # noqa: E402

EVERY = 7
HEAD = 2048
WRITTEN = {}                         # file -> (points, colours) of the stub's write_point_cloud


def write_ply(fn, pts):
    with open(fn, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\n"
                 "property double z\nend_header\n" % len(pts)).encode())
        np.ascontiguousarray(pts, "<f8").tofile(f)


def read_point_cloud(fn):
    with open(fn, "rb") as f:
        while f.readline().strip() != b"end_header":
            pass
        pts = np.fromfile(f, "<f8").reshape(-1, 3)
    return types.SimpleNamespace(points=pts)


def install_stubs():
    o3d = types.ModuleType("open3d")
    o3d.io = types.SimpleNamespace(
        read_point_cloud=read_point_cloud,
        write_point_cloud=lambda fn, pcd: WRITTEN.__setitem__(os.path.basename(fn), (np.array(pcd.points), np.array(pcd.colors))))
    o3d.geometry = types.SimpleNamespace(PointCloud=lambda: types.SimpleNamespace(points=None, colors=None))
    o3d.utility = types.SimpleNamespace(Vector3dVector=np.asarray)
    sys.modules["open3d"] = o3d

    def transform_points(points, matrix):
        points = np.asanyarray(points, dtype=np.float64)
        stack = np.column_stack((points, np.ones(len(points))))
        return np.dot(matrix, stack.T).T[:, :3]

    tm = types.ModuleType("trimesh")
    tm.transformations = types.SimpleNamespace(transform_points=transform_points)
    sys.modules["trimesh"] = tm


def run_script(name, argv, shuffle_seed):
    """-> (the script's globals, what it printed)"""
    real_rng, real_argv = np.random.default_rng, sys.argv
    sys.argv = [name] + argv
    np.random.default_rng = lambda *a: real_rng(*a) if a else real_rng(shuffle_seed)
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            g = runpy.run_path(os.path.join(ref_shim.REFERENCE_ROOT, "evals", name), run_name="__main__")
    finally:
        np.random.default_rng = real_rng
        sys.argv = real_argv
    return g, out.getvalue()


def color_record(prefix, colors):
    return {f"{prefix}_rows": colors[::EVERY], f"{prefix}_classes": borc.color_classes(colors), f"{prefix}_colsum": colors.sum(0),
            f"{prefix}_n": np.asarray(len(colors))}


def bmvs(scan, seed, shuffle_seed):
    sc = synth_bmvs.make_bmvs_scan(seed, scan)
    with tempfile.TemporaryDirectory() as td:
        root = os.path.join(td, "root", "BlendedMVS")
        os.makedirs(os.path.join(root, "stl")); os.makedirs(os.path.join(root, f"scan{scan}")); os.makedirs(os.path.join(td, "pred"))
        write_ply(os.path.join(root, "stl", f"scan{scan}_crop.ply"), sc["gt_pcd"])
        write_ply(os.path.join(td, "pred", f"mvsnet{scan:03}_l3.ply"), sc["data_pcd"])
        if sc["scale_mat"] is not None:
            np.savez(os.path.join(root, f"scan{scan}", "cameras.npz"), scale_mat_0=sc["scale_mat"])
        g, printed = run_script("eval_bmvs.py", ["--data_dir_root", os.path.join(td, "root"), "--datadir", os.path.join(td, "pred"),
                                                 "--scan", str(scan), "-ve"], shuffle_seed)
    k = f"s{scan}"
    rec = {f"{k}_seed": np.asarray(seed), f"{k}_shuffle_seed": np.asarray(shuffle_seed),
           f"{k}_data_head": np.asarray(g["data_pcd"][:HEAD], np.float64), f"{k}_n_data": np.asarray(len(g["data_pcd"])),
           f"{k}_dist_d2s": g["dist_d2s"][:, 0], f"{k}_dist_s2d": g["dist_s2d"][:, 0],
           f"{k}_means": np.asarray([g["mean_d2s"], g["mean_s2d"], g["over_all"]]),
           f"{k}_row": np.asarray(printed.strip().splitlines()[-1])}
    for side in ("d2s", "s2d"):
        pts, colors = WRITTEN[f"{scan}_{side}.ply"]
        assert len(pts) == len(colors) == len(g[f"dist_{side}"])
        rec.update(color_record(f"{k}_color_{side}", colors))
    print(f"   scan {scan}: {printed.strip().splitlines()[-1]}; d2s classes {rec[f'{k}_color_d2s_classes']} of {len(g['dist_d2s'])}, "
          f"s2d classes {rec[f'{k}_color_s2d_classes']} of {len(g['dist_s2d'])}")
    return rec, sc, g


def dtu(seed, shuffle_seed):
    from scipy.io import savemat
    scan = 24
    sc = synth.make_dtu_scan(seed)
    with tempfile.TemporaryDirectory() as td:
        ds = os.path.join(td, "root", "DTU", "DTU_MVS_Data")
        os.makedirs(os.path.join(ds, "ObsMask")); os.makedirs(os.path.join(ds, "Points", "stl")); os.makedirs(os.path.join(td, "pred"))
        savemat(os.path.join(ds, "ObsMask", f"ObsMask{scan}_10.mat"), dict(ObsMask=sc["ObsMask"], BB=sc["BB"], Res=sc["Res"]))
        savemat(os.path.join(ds, "ObsMask", f"Plane{scan}.mat"), dict(P=sc["P"]))
        write_ply(os.path.join(ds, "Points", "stl", f"stl{scan:03}_total.ply"), sc["stl"])
        write_ply(os.path.join(td, "pred", f"mvsnet{scan:03}_l3.ply"), sc["data_pcd"])
        g, printed = run_script("eval_dtu.py", ["--data_dir_root", os.path.join(td, "root"), "--datadir", os.path.join(td, "pred"),
                                                "--scan", str(scan), "-ve"], shuffle_seed)
    rec = {"dtu_seed": np.asarray(seed), "dtu_shuffle_seed": np.asarray(shuffle_seed), "dtu_vis_dist": np.asarray(g["vis_dist"]),
           "dtu_means": np.asarray([g["mean_d2s"], g["mean_s2d"], g["over_all"]])}
    for side, n in (("d2s", len(g["data_down"])), ("s2d", len(g["stl"]))):
        pts, colors = WRITTEN[f"vis_{scan:03}_{side}.ply"]
        assert len(pts) == len(colors) == n
        rec.update(color_record(f"dtu_color_{side}", colors))
    print(f"   dtu: d2s classes {rec['dtu_color_d2s_classes']} of {len(g['data_down'])}, s2d classes {rec['dtu_color_s2d_classes']} "
          f"of {len(g['stl'])}")
    return rec


def main():
    install_stubs()
    rec = {"every": np.asarray(EVERY)}
    for scan, seed, shuffle_seed in ((4, 41, 79), (5, 42, 80)):
        r, sc, g = bmvs(scan, seed, shuffle_seed)
        rec.update(r)
        # the oracle restates what the script just did: the same order, the same distances
        perm = np.arange(len(sc["data_pcd"]))
        np.random.default_rng(shuffle_seed).shuffle(perm)
        _, d = borc.evaluate_scan(sc["data_pcd"][perm], sc["gt_pcd"], sc["relative_scale"], sc["scale_mat"], n_jobs=-1)
        if scan == 4:
            assert np.array_equal(d["data_pcd"], g["data_pcd"]) and np.array_equal(d["dist_d2s"], g["dist_d2s"][:, 0])
            assert np.array_equal(d["dist_s2d"], g["dist_s2d"][:, 0])
        else:
            np.testing.assert_allclose(d["data_pcd"], g["data_pcd"], rtol=1e-13, atol=0)
    rec.update(dtu(31, 77))
    out = os.path.join(HERE, "chamfer_bmvs_ref.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
