#!/usr/bin/env python3
"""Times evals.eval_bmvs on a BlendedMVS-sized synthetic evaluation (no dataset needed): the generator of the tests
(tests/golden/synth_bmvs.py) scaled up to 5.3 M predicted points -- three 1152 x 1536 views -- against 100 K ground-truth
samples, with the error clouds.

    python tools/bench_chamfer_bmvs.py [--pred 5308416] [--gt 100000] [--repeats 3] [--host] [--out profiles/bmvs_chamfer_bench.txt]

Per phase: milliseconds (host clock around a device synchronise; the first of --repeats runs warms up, the fastest and the
last of the others are printed), the bytes the phase has to move, computed from the shapes, and the launches of this
library's kernels (rocPRIM's radix sort inside the grid build launches its own).  These are whole-phase figures, not kernel
times.  Every phase has a time limit sized to it; a phase that overruns ends the run after it has been reported, before
anything else is started.  --host adds scikit-learn's kd-tree on the same machine (n_jobs=16), the reference's way.
Needs the GPU.
"""
import argparse
import os
import sys
import tempfile
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "s-volsdf_amd")):
    sys.path.insert(0, p)

SCAN = 4
# seconds; the s2d search is the open one (see the module text of the profile): far queries probe every cell in reach
LIMITS = dict(upload=20, prepare=5, d2s_search=60, s2d_search=120, means=5, colours=5, download=20, write=60)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--pred", type=int, default=3 * 1152 * 1536)
    p.add_argument("--gt", type=int, default=100000)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--host", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import numpy as np
    import torch
    import synth_bmvs
    from svs_hip import clouds, ply
    from svs_hip.clouds import mean_below, nearest_neighbor
    if not torch.cuda.is_available():
        raise SystemExit("bench_chamfer_bmvs needs the GPU")
    max_dist, vis_dist = 20, 10
    sc = synth_bmvs.make_bmvs_scan(1, SCAN, n_pred=int(a.pred / 0.75), n_gt=a.gt)
    assert len(sc["data_pcd"]) >= a.pred, "the hole took more of the prediction than expected"
    pred = np.ascontiguousarray(sc["data_pcd"][:a.pred], np.float32)             # what the fused PLY stores
    gt = np.ascontiguousarray(sc["gt_pcd"], np.float32)
    rel = sc["relative_scale"]
    dev = torch.device("cuda", torch.cuda.current_device())
    runs = []
    overrun = None
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(a.repeats):
            sec = OrderedDict()

            def phase(name, fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                sec[name] = time.perf_counter() - t0
                return r
            pred_d, gt_d = phase("upload", lambda: (torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)))
            data, ref = phase("prepare", lambda: (clouds.prepare_cloud(pred_d, rel), clouds.prepare_cloud(gt_d, rel)))
            d2s = phase("d2s_search", lambda: nearest_neighbor(ref, data, max_dist))
            if sec["d2s_search"] <= LIMITS["d2s_search"]:
                s2d = phase("s2d_search", lambda: nearest_neighbor(data, ref, max_dist))
            if all(sec[k] <= LIMITS[k] for k in sec) and "s2d_search" in sec:
                means = phase("means", lambda: (mean_below(d2s, max_dist), mean_below(s2d, max_dist)))
                cols = phase("colours", lambda: (clouds.error_colors(d2s, max_dist, vis_dist), clouds.error_colors(s2d, max_dist, vis_dist)))
                host = phase("download", lambda: (data.cpu().numpy(), cols[0][1].cpu().numpy(), ref.cpu().numpy(), cols[1][1].cpu().numpy()))
                phase("write", lambda: (ply.write(os.path.join(tmp, "d2s.ply"), host[0], host[1], coords="double"),
                                        ply.write(os.path.join(tmp, "s2d.ply"), host[2], host[3], coords="double")))
            runs.append(sec)
            print(f"run {rep}: " + ", ".join(f"{k} {v * 1e3:.1f} ms" for k, v in sec.items()), flush=True)
            late = [k for k in sec if sec[k] > LIMITS[k]]
            if late:
                overrun = f"phase {late[0]} took {sec[late[0]]:.1f} s, over its limit of {LIMITS[late[0]]} s: the run ends here"
                break
        far_d2s = float((d2s >= max_dist).double().mean()) if "d2s_search" in runs[-1] else float("nan")
        far_s2d = float((s2d >= max_dist).double().mean()) if "s2d_search" in runs[-1] else float("nan")
    n, m = len(pred), len(gt)
    moved = dict(upload=12 * (n + m), prepare=(12 + 24) * (n + m), d2s_search=24 * (n + m) + 8 * n, s2d_search=24 * (n + m) + 8 * m,
                 means=8 * (n + m), colours=(8 + 24 + 3) * (n + m), download=27 * (n + m), write=27 * (n + m))
    launches = dict(upload=0, prepare=2, d2s_search=9, s2d_search=9, means=4, colours=2, download=0, write=0)
    timed = runs[1:] if len(runs) > 1 else runs
    lines = [f"evals.eval_bmvs on a synthetic BlendedMVS evaluation (tests/golden/synth_bmvs.py, scan {SCAN}'s scale): {n} predicted points, "
             f"{m} ground-truth points, max_dist {max_dist}, MEASURED on {torch.cuda.get_device_name(0)}",
             f"{len(runs)} runs in one process, the first warms up; ms are the fastest / the last of the others"]
    if "means" in runs[-1]:
        lines.append("accuracy %.4f mm, completeness %.4f mm, overall %.4f mm" % (means[0], means[1], (means[0] + means[1]) / 2))
    lines.append(f"queries with no neighbour closer than max_dist: d2s {100 * far_d2s:.2f} % of {n}, s2d {100 * far_s2d:.2f} % of {m}")
    lines.append(f"  {'phase':<11s} {'fastest ms':>11s} {'last ms':>11s} {'first ms':>11s} {'MB':>9s} {'GB/s':>8s}  launches")
    for k in LIMITS:
        t = [r[k] for r in timed if k in r]
        if not t:
            continue
        lines.append(f"  {k:<11s} {min(t) * 1e3:11.2f} {t[-1] * 1e3:11.2f} {runs[0][k] * 1e3:11.2f} {moved[k] / 1e6:9.1f} "
                     f"{moved[k] / min(t) / 1e9:8.1f}  {launches[k]}")
    total = [sum(r.values()) for r in timed]
    lines.append(f"  {'all phases':<11s} {min(total) * 1e3:11.2f} {total[-1] * 1e3:11.2f} {sum(runs[0].values()) * 1e3:11.2f}")
    if overrun:
        lines.append(overrun)
    if a.host and not overrun:
        import bmvs_chamfer_oracle as borc
        t0 = time.perf_counter()
        h_data, h_ref = borc.prepare(pred, rel), borc.prepare(gt, rel)
        t1 = time.perf_counter()
        h_d2s = borc.nn_distance(h_ref, h_data, 16)
        t2 = time.perf_counter()
        h_s2d = borc.nn_distance(h_data, h_ref, 16)
        t3 = time.perf_counter()
        h_means = (h_d2s[h_d2s < max_dist].mean(), h_s2d[h_s2d < max_dist].mean())
        lines.append(f"host, numpy + scikit-learn kd_tree, n_jobs=16, one run: prepare {1e3 * (t1 - t0):.0f} ms, d2s search (fit + query) "
                     f"{1e3 * (t2 - t1):.0f} ms, s2d search {1e3 * (t3 - t2):.0f} ms; accuracy {h_means[0]:.4f} mm, completeness "
                     f"{h_means[1]:.4f} mm")
        lines.append("device against host: accuracy differs by %.3g, completeness by %.3g (relative)" % (
            abs(means[0] - h_means[0]) / h_means[0], abs(means[1] - h_means[1]) / h_means[1]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
