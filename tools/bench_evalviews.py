"""One evaluation view of a synthetic DTU-layout scan, checkpoint-free: render, finish, download and file writing of
svs_hip.evalviews (csrc/svs_evalviews.hip) at 576x768.

    python tools/bench_evalviews.py [--hw 576 768] [--split-n-pixels 512] [--reps 5] [--dir DIR]

The model is the DTU mirror model with its geometric initialisation (a sphere of radius 0.6, beta = 0.1 from the model
section), `fast=-1`: the sampler launches its max_total_iters = 5 up-sampling rounds and decides per 512-ray group on the
device which of them still change anything (the number of groups that converged early is not read back, so it is not
reported).  Times are medians over --reps with the device drained at every phase boundary:
  render    renderer.render_image with the four keys the finish reads
  finish    svs_view_finish + the percentile bounds (torch.sort / cumsum) + svs_view_depth_colors; `finish_kernel_ms` is
            svs_view_finish alone, with the bytes it moves and their share of the HBM peak
  download  the four images to the host
  write     three PNG files and the PFM
and, as the only baseline there is (the reference's script cannot start here), the way the same products were obtained
before this module: render_image with all default keys, every tensor to the host, the numpy oracle
(tests/evalviews_oracle.py) on the host.  Prints one JSON line.  Needs the MI355X: there is no CPU path."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-volsdf_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X HBM3E, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, nargs=2, default=(576, 768))
    ap.add_argument("--split-n-pixels", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", help="where the scan and the output folder are written (default: a temporary directory)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import evalviews_oracle as eo
    import scene_oracle as so
    from svs_hip import evalviews as ev, scene
    from svs_hip.renderer import render_image
    if not torch.cuda.is_available():
        raise SystemExit("bench_evalviews.py needs the GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    hw = tuple(a.hw)
    N = hw[0] * hw[1]
    root = a.dir or tempfile.mkdtemp(prefix="bench_evalviews_")
    try:
        so.write_scan(root, "DTU", 24, 3, hw, mask_views=(0, 1, 2))
        ds = scene.SceneDataset("DTU", list(hw), scan_id=24, data_dir_root=root)
        torch.manual_seed(0)
        model = ev.build_model("DTU").to(dev).eval()
        _, model_input, _ = ds.collate_fn([ds[1]])
        inp = {k: t.to(dev) for k, t in model_input.items()}
        out_folder = os.path.join(root, "out")
        os.makedirs(os.path.join(out_folder, "depth_est"), exist_ok=True)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return r, (time.perf_counter() - t0) * 1e3

        ms = {k: [] for k in ("render", "finish", "finish_kernel", "download", "write", "old_render", "old_download",
                              "old_numpy")}
        for rep in range(a.reps + 1):                       # the first pass warms up and is dropped
            out, t = timed(lambda: render_image(model, inp, N, split_n_pixels=a.split_n_pixels, keys=ev.RENDER_KEYS))
            ms["render"].append(t)
            ev.LAUNCHES.update(finish=0, colors=0)
            res, t = timed(lambda: ev.finish_view(out, hw, ds.scale_factor))
            ms["finish"].append(t)
            launches = dict(ev.LAUNCHES)
            _, t = timed(lambda: ev.finish_arrays(out["rgb_values"], out["normal_map"], out["depth_values"],
                                                  out["weights"], ds.scale_factor))
            ms["finish_kernel"].append(t)
            host, t = timed(lambda: {k: (v.cpu().numpy() if v is not None else None) for k, v in res.items()})
            ms["download"].append(t)
            t0 = time.perf_counter()
            ev.write_view(out_folder, 1, host)
            ms["write"].append((time.perf_counter() - t0) * 1e3)
            S = int(out["weights"].shape[1])
            del out, res
            full, t = timed(lambda: render_image(model, inp, N, split_n_pixels=a.split_n_pixels))
            ms["old_render"].append(t)
            cpu, t = timed(lambda: {k: v.cpu().numpy() for k, v in full.items()})
            ms["old_download"].append(t)
            old_bytes = sum(v.nbytes for v in cpu.values())
            del full
            t0 = time.perf_counter()
            o = eo.finish(cpu["rgb_values"], cpu["normal_map"], cpu["depth_values"], cpu["weights"], ds.scale_factor)
            table = ev.turbo_table()
            if table is not None:
                acc = o["acc"].astype(np.float32)
                lo, hi = eo.depth_bounds(cpu["depth_values"], acc)
                eo.depth_colors(cpu["depth_values"], acc, lo, hi, table, hw)
            ms["old_numpy"].append((time.perf_counter() - t0) * 1e3)
            del cpu
        med = {k: round(statistics.median(v[1:]), 3) for k, v in ms.items()}
        finish_bytes = N * (S * 4 + 12 + 12 + 4) + N * (3 + 3 + 4 + 4)
        res = dict(metric="evalviews_ms_per_view", hw=list(hw), samples_per_ray=S, split_n_pixels=a.split_n_pixels,
                   beta=float(model.density.get_beta().detach().cpu().reshape(-1)[0]) if hasattr(model.density, "get_beta") else None,
                   sampler_rounds_launched=int(model.ray_sampler.max_total_iters), reps=a.reps, ms=med,
                   entry_point_calls=launches, kernel_launches=launches["finish"] + launches["colors"],
                   finish_bytes=finish_bytes,
                   finish_hbm_peak_fraction=round(finish_bytes / (med["finish_kernel"] * 1e-3) / HBM_PEAK_BYTES_PER_S, 4),
                   downloaded_bytes=N * (3 + 3 + 4 + 4 + (3 if ev.turbo_table() is not None else 0)),
                   old_downloaded_bytes=old_bytes,
                   new_total_ms=round(med["render"] + med["finish"] + med["download"] + med["write"], 2),
                   old_total_ms=round(med["old_render"] + med["old_download"] + med["old_numpy"] + med["write"], 2),
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(res))
    finally:
        if not a.dir:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
