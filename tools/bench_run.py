"""The native runner's phase times (svs_hip.run) and the save tail of one full-size view (csrc/svs_preview.hip,
svs_hip.mvsout.save_view(previews=True)).

    python tools/bench_run.py [--hw 1152 1536] [--iters 20] [--no-scan]

1. One toy DTU scan through `run.main` -- the folder tests/test_gpu_run.py writes (49 images of 120x160, views 25 / 22 /
   28, a seeded random CascadeMVSNet with the reference's 192 / 32 / 8 depth planes), max_h=96 max_w=128, 6+ optimisation
   steps: the seconds per phase the runner prints.  The MVS side runs at the reference's 1152x1536.
2. The save tail of one 1152x1536 view with synthetic outputs: ms for the order statistics (one call for the depth's
   quantile, one for the confidence's two percentiles), the two preview launches, the downloads and the file writing, with
   bytes and launches; and the host route it replaces (np.quantile / np.percentile and the per-pixel numpy arithmetic of
   visualize_depth on the downloaded maps).

Prints one JSON line; it asserts nothing.  Needs the MI355X: there is no CPU path.
"""
import argparse
import contextlib
import io
import json
import os
import pathlib
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "s-volsdf_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def events(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def wall(fn, iters, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def toy_scan():
    import torch
    import test_gpu_run as t
    from svs_hip import run
    root = pathlib.Path(tempfile.mkdtemp(prefix="svs_run_bench_"))
    torch.manual_seed(0)
    t.write_toy_root(root)
    out = {}
    for name in ("first", "second"):                    # the second run has warm kernels, allocator and file cache
        text = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(text):
            run.main(t.OVERRIDES + [f"data_dir_root={root}", f"outdir={root / ('out_' + name)}", f"exps_folder={root / 'exps'}"])
        m = re.search(r"scan106 seconds: (.*)", text.getvalue())
        out[name] = dict(total_s=round(time.perf_counter() - t0, 3),
                         phases_s={k: float(v) for k, v in (kv.split(" ") for kv in m.group(1).split(", "))})
    return out


def save_tail(H, W, iters):
    import numpy as np
    import torch
    import run_oracle as ro
    from svs_hip import mvsout
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (600 + 150 * np.sin(xx / 90.0) * np.cos(yy / 70.0) + rng.normal(0, 4, (H, W))).astype(np.float32)
    conf = [rng.uniform(0, 1, (H // s, W // s)).astype(np.float32) for s in (4, 2, 1)]
    G = lambda a: torch.from_numpy(a).cuda()
    outputs = dict(depth=G(depth)[None], photometric_confidence=G(conf[2])[None],
                   stage1=dict(depth=G(depth[::4, ::4].copy())[None], photometric_confidence=G(conf[0])[None]),
                   stage2=dict(depth=G(depth[::2, ::2].copy())[None], photometric_confidence=G(conf[1])[None]),
                   prob_volume=torch.zeros(8, H, W, device="cuda"))
    cam = np.stack([np.eye(4), np.eye(4)]).astype(np.float32)
    img = G(rng.uniform(0, 1, (3, H, W)).astype(np.float32))
    d, c = outputs["depth"][0], mvsout.final_confidence(outputs)
    jet = mvsout.jet_table()
    res = dict(hw=[H, W], n=H * W)
    res["select_depth_1_rank"] = dict(events(lambda: mvsout.quantile(d, 0.01), iters), launches=mvsout.KERNELS_PER_CALL["select"],
                                      bytes_read=4 * 4 * H * W, bytes_down=48)
    res["select_conf_2_ranks"] = dict(events(lambda: mvsout.percentile(c, [5, 95], valid_only=True), iters),
                                      launches=mvsout.KERNELS_PER_CALL["select"], bytes_read=4 * 4 * H * W, bytes_down=48)
    lo, (clo, chi) = mvsout.quantile(d, 0.01), mvsout.percentile(c, [5, 95], valid_only=True)
    three = [d, outputs["stage1"]["depth"], outputs["stage2"]["depth"]]
    px = H * W + (H // 4) * (W // 4) + (H // 2) * (W // 2)
    res["preview_3_depth_maps"] = dict(events(lambda: mvsout.depth_preview(three, lo, 935.0, table=jet), iters), launches=1,
                                       bytes=7 * px)
    res["preview_confidence"] = dict(events(lambda: mvsout.depth_preview([c], clo, chi, direct=True), iters), launches=1,
                                     bytes=5 * H * W)
    col = mvsout.depth_preview(three, lo, 935.0, table=jet) + mvsout.depth_preview([c], clo, chi, direct=True)
    res["download_2_maps_4_previews"] = dict(wall(lambda: [t.cpu() for t in (d, c, *col)], iters),
                                             bytes=8 * H * W + 3 * px + H * W)
    folder = tempfile.mkdtemp(prefix="svs_save_tail_")
    before, down = dict(mvsout.LAUNCHES), dict(mvsout.BYTES_DOWN)
    res["save_view_previews"] = wall(lambda: mvsout.save_view(folder, 25, outputs, cam, img, previews=True, dep_max=935.0), 5, 1)
    res["save_view_plain"] = wall(lambda: mvsout.save_view(folder + "/plain", 25, outputs, cam, img), 5, 1)
    calls = 6 + 6
    res["save_view_previews"]["launches_per_call"] = {k: (mvsout.LAUNCHES[k] - before[k]) * mvsout.KERNELS_PER_CALL[k] / calls
                                                      for k in before if mvsout.LAUNCHES[k] != before[k]}
    res["save_view_previews"]["bytes_down_per_call"] = {k: (mvsout.BYTES_DOWN[k] - down[k]) // 6 for k in down}
    res["save_view_previews"]["file_bytes"] = {f"{s}/{f}": os.path.getsize(os.path.join(folder, s, f))
                                               for s in ("depth_est", "confidence", "images") for f in sorted(os.listdir(os.path.join(folder, s)))}
    # the host route: the maps downloaded, numpy's quantiles and visualize_depth's arithmetic on the CPU
    dh, ch = d.cpu().numpy(), c.cpu().numpy()

    def host(fn, n=3):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        return round(statistics.median(ts), 2)
    res["host_route_ms"] = dict(np_quantile_depth=host(lambda: np.quantile(dh, 0.01)),
                                np_percentiles_conf=host(lambda: (np.percentile(ch, 5), np.percentile(ch, 95))),
                                visualize_depth_color=host(lambda: ro.visualize_depth(dh, lo, 935.0, table=jet)),
                                visualize_depth_direct=host(lambda: ro.visualize_depth(ch, clo, chi, direct=True)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, nargs=2, default=(1152, 1536))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-scan", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_run.py needs the GPU (there is no CPU path)")
    out = dict(save_tail=save_tail(a.hw[0], a.hw[1], a.iters))
    if not a.no_scan:
        out["toy_scan"] = toy_scan()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
