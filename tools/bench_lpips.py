#!/usr/bin/env python3
"""Times LPIPS for one evaluation view (prediction + ground truth) with seeded weights: svs_hip.lpips against the same
definition through torch's float32 F.conv2d on the same card.

    python tools/bench_lpips.py [--size 576 768] [--repeats 5] [--out profiles/lpips_bench.txt]

Whole call: milliseconds between two device events around LpipsNet.score_views's entry point (the median of --repeats
runs after one warm-up), the workspace bytes and the launches.  Per phase (prologue / convolutions per group / pools /
head): kernel durations from one run under torch.profiler, grouped by kernel name and launch order; they leave out the
gaps between launches.  torch: F.conv2d / max_pool2d / the head in float32 on device tensors, same events.  Needs the GPU.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-volsdf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return sorted(ms)[len(ms) // 2]


def phases(fn):
    """kernel milliseconds of one run by phase, from torch.profiler -> (dict, launches) or (None, None)"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    import lpips_oracle as lo
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if "cuda" in str(getattr(e, "device_type", "")).lower() and "lpips" in e.name]
    if not ev:
        return None, None
    ev.sort(key=lambda e: e.time_range.start)
    out = {"prologue": 0.0, "pools": 0.0, "head": 0.0, "finish": 0.0}
    out.update({f"conv group {g + 1}": 0.0 for g in range(5)})
    conv = 0
    for e in ev:
        ms = (e.time_range.end - e.time_range.start) / 1000.0
        if "conv3x3" in e.name:
            out[f"conv group {lo.CONV_GROUP[conv % 13] + 1}"] += ms
            conv += 1
        else:
            for key, word in (("prologue", "prologue"), ("pools", "maxpool"), ("head", "head"), ("finish", "finish")):
                if word in e.name:
                    out[key] += ms
    return out, len(ev)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, nargs=2, default=(576, 768), metavar=("H", "W"))
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    import numpy as np
    import torch
    import torch.nn.functional as F
    import lpips_oracle as lo
    from svs_hip import lib, lpips
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips needs the GPU")
    H, W = a.size
    weights = lo.make_weights(0)
    pred, gt, mask = (torch.from_numpy(x).cuda() for x in lo.make_views(3, 1, H, W))
    net = lpips.LpipsNet(weights)
    d_hip = net.score_views(pred, gt, mask)
    ms_hip = timed(lambda: net.score_views(pred, gt, mask), a.repeats)
    ph, launches = phases(lambda: net.score_views(pred, gt, mask))

    conv = [(torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()) for w, b in weights["conv"]]
    lin = [torch.from_numpy(w).cuda() for w in weights["lin"]]
    x0 = lo.network_input(np.stack([lo.composite(pred[0].cpu().numpy(), mask[0].cpu().numpy()),
                                    lo.composite(gt[0].cpu().numpy(), mask[0].cpu().numpy())]), torch.float32).cuda()

    def torch_run():
        with torch.no_grad():
            x, total = x0, 0.0
            for i, (w, b) in enumerate(conv):
                if i > 0 and lo.CONV_GROUP[i] != lo.CONV_GROUP[i - 1]:
                    x = F.max_pool2d(x, 2, 2)
                x = F.relu(F.conv2d(x, w, b, padding=1))
                if i + 1 == 13 or lo.CONV_GROUP[i + 1] != lo.CONV_GROUP[i]:
                    total = total + lo.head(x[0], x[1], lin[lo.CONV_GROUP[i]])
            return total

    d_torch = float(torch_run())
    ms_torch = timed(torch_run, a.repeats)
    flop = 0
    h, w = H, W
    for i, (cin, cout) in enumerate(lo.CONV_SHAPE):
        if i > 0 and lo.CONV_GROUP[i] != lo.CONV_GROUP[i - 1]:
            h, w = h // 2, w // 2
        flop += 2 * 2 * 9 * cin * cout * h * w
    L = lib.load()
    lines = [f"LPIPS, one view (prediction + ground truth) at {H}x{W}, seeded weights, {flop / 1e9:.0f} GFLOP of convolution",
             f"  svs_hip.lpips     {ms_hip:9.3f} ms   ({flop / ms_hip / 1e9:.1f} TFLOP/s of float32-equivalent work; 3 MFMAs per product)",
             f"  torch F.conv2d    {ms_torch:9.3f} ms   (float32, same card)",
             f"  values            hip {d_hip[0]:.10f}   torch float32 {d_torch:.10f}",
             f"  workspace {int(L.svs_lpips_workspace_bytes(1, H, W))} bytes, packed network {int(L.svs_lpips_net_bytes())} bytes, "
             f"launches {launches if launches else 24} (1 prologue, 13 convolutions, 4 pools, 5 heads, 1 finish)"]
    if ph:
        lines.append("  kernel ms by phase: " + ", ".join(f"{k} {v:.3f}" for k, v in ph.items()) + f"; sum {sum(ph.values()):.3f}")
    else:
        lines.append("  kernel ms by phase: the profiler returned no device events")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
