"""Loading one synthetic DTU-sized scan with svs_hip.scene.SceneDataset (csrc/svs_scene.hip): 49 PNG images of
1200x1600 resized to 576x768, smoothed, with 25 evaluation masks.

    python tools/bench_scene.py [--images 49] [--src 1200 1600] [--hw 576 768] [--dir DIR] [--keep]

Writes the scan folder (PNG files, cameras.npz, masks) to a temporary directory, builds the dataset once with the device
drained at every phase boundary, so that the phases add up (decode = PIL on a thread pool, upload = uint8 codes to the
device, kernels = resize + smoothing + masks, download = float32 results into the pinned host tensor), once more without
those drains (what a run pays), and a third time with the cache warm.  Prints one JSON line: ms per scan and per image for
every phase, bytes moved, entry-point calls and kernel launches, the kernels' algorithmic bytes and the share of the HBM peak
they imply.  Needs the MI355X: there is no CPU path.  No OpenCV is installed to time the reference's loader against, so no
speed-up is claimed.
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


def algorithmic_bytes(n, n_masks, src, hw):
    """Every array touched once per kernel: codes read and rgb written by the resize, rgb read / intermediate written and
    intermediate read / rgb_smooth written by the two smoothing passes, mask codes read and the mask written."""
    f = hw[0] * hw[1] * 3 * 4
    return dict(resize=n * (src[0] * src[1] * 3 + f), smooth=n * 4 * f, mask=n_masks * (src[0] * src[1] + f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=49)
    ap.add_argument("--src", type=int, nargs=2, default=(1200, 1600))
    ap.add_argument("--hw", type=int, nargs=2, default=(576, 768))
    ap.add_argument("--dir", help="where the scan folder is written (default: a temporary directory)")
    ap.add_argument("--keep", action="store_true", help="leave the folder in place")
    a = ap.parse_args()
    import torch
    import scene_oracle as so
    from svs_hip import scene
    from svs_hip.images import Phases
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene.py needs the GPU (there is no CPU path)")
    root = a.dir or tempfile.mkdtemp(prefix="bench_scene_")
    try:
        t = time.perf_counter()
        eval_ids = [v for v in scene.get_eval_ids("DTU") if v < a.images]
        so.write_scan(root, "DTU", 106, a.images, tuple(a.src), mask_views=[0] + eval_ids, mask_size=tuple(a.src))
        write_s = time.perf_counter() - t
        torch.zeros(1, device="cuda:0")                 # the context and the library are not part of a load
        scene.prepare_images(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), (16, 16))
        torch.cuda.synchronize()
        scene.LAUNCHES.update(resize=0, smooth=0, mask=0)

        def build(phases=None):
            t0 = time.perf_counter()
            ds = scene.SceneDataset("DTU", tuple(a.hw), scan_id=106, num_views=3, data_dir_root=root, phases=phases)
            return ds, (time.perf_counter() - t0) * 1e3

        os.environ["SVS_SCENE_CACHE"] = "0"
        ph = Phases(sync=True)
        ds, phased_ms = build(ph)
        calls = dict(scene.LAUNCHES)
        _, plain_ms = build()
        os.environ["SVS_SCENE_CACHE"] = "1"
        scene.cache_clear()
        _, miss_ms = build()
        ds2, hit_ms = build()
        assert ds2.cache_hit and ds2.rgb_images[0].data_ptr() != ds.rgb_images[0].data_ptr()
        n = ds.n_images
        b = algorithmic_bytes(n, len(ds.mask_views), a.src, a.hw)
        k_ms = ph.s["kernels"] * 1e3
        res = dict(metric="scene_load_ms_per_scan", images=n, src=list(a.src), hw=list(a.hw), masks=len(ds.mask_views),
                   resized=bool(ds.resized), chunk=scene.CHUNK,
                   phase_ms_per_scan={k: round(v * 1e3, 2) for k, v in ph.s.items()},
                   phase_ms_per_image={k: round(v * 1e3 / n, 3) for k, v in ph.s.items()},
                   build_ms_phased=round(phased_ms, 1), build_ms=round(plain_ms, 1), build_ms_cache_miss=round(miss_ms, 1),
                   build_ms_cache_hit=round(hit_ms, 2),
                   bytes_uploaded=ph.bytes_up, bytes_downloaded=ph.bytes_down,
                   entry_point_calls=calls, kernel_launches=calls["resize"] + 2 * calls["smooth"] + calls["mask"],
                   kernel_algorithmic_bytes=b,
                   kernel_hbm_peak_fraction=round(sum(b.values()) / (k_ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 4) if k_ms else None,
                   write_folder_s=round(write_s, 1), device=torch.cuda.get_device_name(0))
        print(json.dumps(res))
    finally:
        if not a.keep and not a.dir:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
