"""The entry points of csrc/svs_mvsout.hip at the sizes of one DTU scan: the three evaluation masks of the training views
(1200x1600, dilated by disk(12), resized to 1152x1536) and one 288x384 / 576x768 / 1152x1536 confidence triple.

    python tools/bench_mvsout.py [--src 1200 1600] [--hw 1152 1536] [--views 3] [--radius 12] [--iters 20] [--host]

Per entry: milliseconds (HIP events around the call on a warm device, median of --iters), the algorithmic bytes (every
array touched once per kernel) and the kernel launches.  --host also times scipy.ndimage.binary_dilation on one mask (a
single run on the CPU), the route the dilation replaces.  Prints one JSON line; it asserts nothing.  Needs the MI355X:
there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-volsdf_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, iters, warmup=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", type=int, nargs=2, default=(1200, 1600))
    ap.add_argument("--hw", type=int, nargs=2, default=(1152, 1536))
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--radius", type=int, default=12)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host", action="store_true", help="also time scipy's binary_dilation on one mask (CPU, single run)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from svs_hip import lib, mvsout
    if not torch.cuda.is_available():
        raise SystemExit("bench_mvsout.py needs the GPU (there is no CPU path)")
    dev = torch.device("cuda:0")
    L = lib.load()
    V, (Hs, Ws), (H, W), r = a.views, a.src, a.hw, a.radius
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:Hs, 0:Ws]
    host_masks = np.stack([(((y - Hs / 2) ** 2 + (x - Ws / 2 - 40 * v) ** 2 <= (0.3 * Hs) ** 2)
                            | (rng.random((Hs, Ws)) < 1e-4)).astype(np.uint8) for v in range(V)])
    masks = torch.from_numpy(host_masks).to(dev)
    conf = [torch.rand(H // 4, W // 4, device=dev), torch.rand(H // 2, W // 2, device=dev), torch.rand(H, W, device=dev)]
    dilated = mvsout.dilate_disk(masks, r)
    words = V * Hs * ((Ws + 63) // 64) * 8
    res = dict(metric="mvsout_ms_per_entry", views=V, src=[Hs, Ws], hw=[H, W], radius=r, iters=a.iters,
               device=torch.cuda.get_device_name(0), entries={})
    for name, fn, nbytes, key in (
            ("svs_mask_dilate_disk", lambda: mvsout.dilate_disk(masks, r), V * Hs * Ws * 2 + 4 * words, "dilate"),
            ("svs_mask_resize_any", lambda: mvsout.resize_any(dilated, H, W), V * (Hs * Ws + H * W), "resize"),
            ("svs_mvs_confidence", lambda: mvsout.confidence_product(*conf, H, W),
             4 * (sum(c.numel() for c in conf) + H * W), "confidence")):
        res["entries"][name] = dict(timed(fn, a.iters), algorithmic_bytes=nbytes, kernel_launches=mvsout.KERNELS_PER_CALL[key])
    # the dilation's kernels alone: the call above also allocates its output and workspace and uploads nothing
    out = torch.empty_like(masks)
    ws = torch.empty(int(L.svs_mask_dilate_workspace_bytes(V, Hs, Ws)) // 8, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    res["entries"]["svs_mask_dilate_disk"]["kernels_only"] = timed(
        lambda: L.svs_mask_dilate_disk(masks.data_ptr(), V, Hs, Ws, r, ws.data_ptr(), out.data_ptr(), stream), a.iters)
    res["eval_mask_ms_per_view_from_host_codes"] = timed(lambda: mvsout.eval_mask(host_masks[0], H, W, r), a.iters)
    if a.host:
        from scipy import ndimage
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
        t0 = time.perf_counter()
        want = ndimage.binary_dilation(host_masks[0] != 0, structure=xx * xx + yy * yy <= r * r)
        res["host_scipy_binary_dilation_s_one_mask"] = round(time.perf_counter() - t0, 3)
        res["host_equals_device"] = bool(np.array_equal(want, dilated[0].cpu().numpy() != 0))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
