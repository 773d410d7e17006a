"""Loading the MVS inputs of one synthetic DTU-sized scan with svs_hip.mvsdata.MVSDataset (csrc/svs_mvsdata.hip): 49
PNG images of 1200x1600, 3 training views through the x2_mvsres chain (576x768, then 1152x1536), and the folder
create_scene writes for image-based rendering over the DTU id lists (3 + 25 cameras, 3 images).

    python tools/bench_mvsdata.py [--src 1200 1600] [--max-hw 576 768] [--no-x2] [--dir DIR] [--keep]

Writes the scan folder to a temporary directory (three distinct training images; the other files, of which only the
header is read, are copies), then builds the 3 device samples and runs create_scene, each once with
the device drained at every phase boundary, so that the phases add up (decode = PIL on a thread pool, upload = uint8
codes to the device, kernels = the resize passes and the PNG codes, download = the PNG codes), and once without those
drains (what a run pays).  Prints one JSON line: ms per phase, bytes moved, entry-point calls, the kernels' algorithmic
bytes and the share of the HBM peak they imply, and the decodes and resizes against what the reference's loader does for
the same scan -- as COUNTS: no OpenCV is installed to time that loader against, so no speed-up is claimed.  Needs the
MI355X: there is no CPU path.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-volsdf_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_BYTES_PER_S = 8.0e12          # MI355X HBM3E, spec
REFERENCE_PASSES_PER_SCAN = 4          # runner.py:184, 240, 251: the loader is iterated for three stages and the save loop


def algorithmic_bytes(n, src, sizes, channels=3):
    """every array touched once per kernel: the codes read and the float32 image written by each pass"""
    total, cur, item = 0, src, 1
    for k, hw in enumerate(sizes):
        planes = channels if k + 1 < len(sizes) else 4       # the last pass writes imgs (3 planes) and masks (1)
        total += n * (cur[0] * cur[1] * channels * item + hw[0] * hw[1] * planes * 4)
        cur, item = hw, 4
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=49)
    ap.add_argument("--src", type=int, nargs=2, default=(1200, 1600))
    ap.add_argument("--max-hw", type=int, nargs=2, default=(576, 768))
    ap.add_argument("--no-x2", action="store_true")
    ap.add_argument("--dir", help="where the scan folder is written (default: a temporary directory)")
    ap.add_argument("--keep", action="store_true", help="leave the folder in place")
    a = ap.parse_args()
    import torch
    import mvsdata_oracle as mo
    import scene_oracle as so
    from PIL import Image
    from svs_hip import mvsdata, scene
    from svs_hip.images import Phases
    from svs_hip.scans import glob_images
    if not torch.cuda.is_available():
        raise SystemExit("bench_mvsdata.py needs the GPU (there is no CPU path)")
    root = a.dir or tempfile.mkdtemp(prefix="bench_mvsdata_")
    try:
        t = time.perf_counter()
        trains = scene.get_trains_ids("DTU", "scan106", 3)
        evals = [v for v in scene.get_eval_ids("DTU") if v < a.images]
        pairs = {k: [s for s in trains + [0, 1] if s != k][:4] for k in range(a.images)}
        mvs = mo.write_mvs_scan(root, "DTU", 106, a.images, (16, 16), pairs)            # cameras, pairs, the file names
        files = glob_images(os.path.join(root, "DTU", "scan106", "image"))
        for k, v in enumerate(trains):                    # three distinct images; the views that are never decoded are copies
            Image.fromarray(so.synthetic_image(a.src[0], a.src[1], k)).save(files[v])
        for v in range(a.images):
            if v not in trains:
                shutil.copyfile(files[trains[0]], files[v])
        write_s = time.perf_counter() - t
        torch.zeros(1, device="cuda:0")                 # the context and the library are not part of a load
        mvsdata.prepare_views(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), [(16, 16)], png=True)
        torch.cuda.synchronize()
        args = dict(data_dir_root=root, x2_mvsres=not a.no_x2)

        def dataset(ids, sync):
            return mvsdata.MVSDataset(mvs, ["scan106"], "test", 3, "DTU", 192, 1.06, max_h=a.max_hw[0], max_w=a.max_hw[1],
                                      trains_i=list(ids), args=args, phases=Phases(sync=sync))

        def run(fn, ids, sync):
            mvsdata.LAUNCHES.update(resize=0, pack=0, codes=0)
            ds = dataset(ids, sync)
            t0 = time.perf_counter()
            fn(ds)
            torch.cuda.synchronize()
            return ds, (time.perf_counter() - t0) * 1e3, dict(mvsdata.LAUNCHES)

        out = tempfile.mkdtemp(prefix="scene_", dir=root)
        jobs = dict(samples=(lambda ds: ds.device_samples(), trains),
                    create_scene=(lambda ds: mvsdata.create_scene(out, ds, evals), trains + evals))
        res = dict(metric="mvsdata_load_ms_per_scan", images=a.images, src=list(a.src), x2_mvsres=not a.no_x2,
                   write_folder_s=round(write_s, 1), device=torch.cuda.get_device_name(0))
        for name, (fn, ids) in jobs.items():
            ds, phased_ms, calls = run(fn, ids, True)
            _, plain_ms, _ = run(fn, ids, False)
            sizes = ds.passes(*a.src)[0]
            ph = ds.phases
            b = algorithmic_bytes(ds.decoded_views, a.src, sizes)
            k_ms = ph.s["kernels"] * 1e3
            res[name] = dict(views=len(ids), decoded_views=ds.decoded_views, sizes=[list(s) for s in sizes],
                             phase_ms={k: round(v * 1e3, 2) for k, v in ph.s.items()}, total_ms_phased=round(phased_ms, 1),
                             total_ms=round(plain_ms, 1), bytes_uploaded=ph.bytes_up, bytes_downloaded=ph.bytes_down,
                             entry_point_calls=calls, kernel_launches=sum(calls.values()), kernel_algorithmic_bytes=b,
                             kernel_hbm_peak_fraction=round(b / (k_ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 4) if k_ms else None)
        n, per_view = len(trains), len(res["samples"]["sizes"])
        both = dataset(trains + evals, False)
        res["counts_per_scan"] = dict(
            decodes=res["samples"]["decoded_views"], resizes=per_view * res["samples"]["decoded_views"],
            reference_decodes=REFERENCE_PASSES_PER_SCAN * n * n, reference_resizes=REFERENCE_PASSES_PER_SCAN * n * n * per_view,
            create_scene_decodes=res["create_scene"]["decoded_views"],
            reference_create_scene_decodes=sum(len(both.view_ids(i)) for i in range(len(both))))
        print(json.dumps(res))
    finally:
        if not a.keep and not a.dir:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
