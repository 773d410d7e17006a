"""UCSNet at the workload's size (x2_mvsres: 1152 x 1536, 3 views, ndepths 192, 32, 8) with seeded weights:

  * the feature extractor, ms per image: the default / both transposed layers on the matrix cores / both on the float32 kernel /
    every layer on the float32 kernels, and the two transposed layers alone on both paths (device events, the paths alternating);
  * per stage: the hypotheses kernel, the cost volume (warp + variance + regulariser), the tail with the uncertainty and,
    beside it, the tail without;
  * bytes and launches, counted from the shapes.

    python tools/bench_ucsnet.py [--out FILE (default profiles/ucsnet_bench.txt)] [--hw 1152 1536] [--reps 20]

Needs the GPU: there is no fall-back, and nothing here is a time without one.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "s-volsdf_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests"),
                os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
import ucsnet_oracle as uo  # noqa: E402
from models.ucsnet import UCSNetHip as UCSNet  # noqa: E402  (the mirror, whether or not a checkout is on the path)
from svs_hip import costvol  # noqa: E402


BATCH = 10


def timed(fns, reps):
    """Per function: ms per call as (median, min, max) over `reps` batches of BATCH back-to-back calls, each batch between two
    device events (the enqueue gap of one call is hidden behind the previous call's kernels), the functions alternating."""
    for f in fns:
        f(); f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(BATCH):
                f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b) / BATCH)
    return [(float(np.median(m)), min(m), max(m)) for m in ms]


def fmt(t, digits=3):
    return f"{t[0]:.{digits}f} ({t[1]:.{digits}f} .. {t[2]:.{digits}f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ucsnet_bench.txt"))
    ap.add_argument("--hw", type=int, nargs=2, default=(1152, 1536))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ndepths", type=int, nargs=3, default=(192, 32, 8))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ucsnet needs the GPU")
    dev = torch.device("cuda:0")
    H, W = args.hw
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    m = UCSNet(lamb=1.5, stage_configs=list(args.ndepths))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in uo.ucsnet_state_dict(21).items()}, strict=True)
    m.to(dev).eval()
    fe = m.feature_extraction
    rng = np.random.default_rng(0)
    images = [torch.from_numpy(rng.uniform(0, 1, (3, H, W)).astype(np.float32)).to(dev) for _ in range(3)]
    say(f"UCSNet, {H} x {W}, 3 views, ndepths {list(args.ndepths)}, lamb 1.5, seeded weights; {torch.cuda.get_device_name(0)}")

    # ---- feature extractor
    layers = fe.layers()
    nets = [costvol.FeatureNetUnet(8), costvol.FeatureNetUnet(8, deconv_mfma=False), costvol.FeatureNetUnet(8, mfma=False),
            costvol.FeatureNetUnet(8, deconv_mfma=True)]
    with torch.no_grad():
        outs = [n(images[0], layers) for n in nets]
        t = timed([lambda n=n: n(images[0], layers) for n in nets], args.reps)
    say(f"times: median (min .. max) over batches of {BATCH} calls between device events: they include what the host takes to enqueue")
    say("feature extractor (15 launches from one call), ms per image:")
    say(f"  default (3x3 / 5x5 layers and deconv1.deconv on the matrix cores)  {fmt(t[0])}")
    say(f"  both transposed layers on the matrix cores                        {fmt(t[3])}")
    say(f"  both transposed layers on the float32 kernel                      {fmt(t[1])}")
    say(f"  every layer on the float32 kernels                                {fmt(t[2])}")
    for j in range(3):
        say(f"  stage{j + 1}: max |default - float32 transposed| = {float((outs[0][j] - outs[1][j]).abs().max()):.2e}, "
            f"max |default - all float32| = {float((outs[0][j] - outs[2][j]).abs().max()):.2e} (output scale {float(outs[0][j].abs().max()):.2f})")
    ws = costvol._lib.load().svs_featurenet_unet_workspace_bytes(8, H, W)
    say(f"  workspace {ws / 2 ** 20:.1f} MiB (both concatenations formed in place: no torch.cat copy of "
        f"{(32 * (H // 2) * (W // 2) + 16 * H * W) * 4 / 2 ** 20:.1f} MiB per image)")
    say("transposed layers alone (bias + ReLU), ms per launch and GB/s of input + output:")
    for name, (cin, cout, h, w) in (("deconv1.deconv", (32, 16, H // 4, W // 4)), ("deconv2.deconv", (16, 8, H // 2, W // 2))):
        x = torch.randn(cin, h, w, device=dev)
        wt = torch.randn(cin, cout, 3, 3, device=dev) / np.sqrt(cin * 9 / 4)
        b = torch.randn(cout, device=dev)
        out = torch.empty(2 * cout, 2 * h, 2 * w, device=dev)
        tm, tf = timed([lambda: costvol.deconv2d(x, wt, b, relu=True, out=out, mfma=True),
                        lambda: costvol.deconv2d(x, wt, b, relu=True, out=out, mfma=False)], 2 * args.reps)
        nbytes = (cin * h * w + cout * 4 * h * w) * 4
        ref = torch.nn.functional.conv_transpose2d(x.double()[None], wt.double(), b.double(), stride=2, padding=1, output_padding=1)[0].clamp(min=0)
        errs = []
        for mf in (True, False):
            got = costvol.deconv2d(x, wt, b, relu=True, mfma=mf)
            errs.append(float((got.double() - ref).abs().max() / ref.abs().max()))
        say(f"  {name} {cin}->{cout} ({h} x {w} -> {2 * h} x {2 * w}): svs_deconv2d_mfma {fmt(tm, 4)} ms ({nbytes / tm[0] / 1e6:.0f} GB/s), "
            f"svs_deconv2d {fmt(tf, 4)} ms ({nbytes / tf[0] / 1e6:.0f} GB/s); error against float64 / output scale: {errs[0]:.2e} / {errs[1]:.2e}")
        del x, out, ref

    # ---- the three stages
    with torch.no_grad():
        feats = [fe(im[None]) for im in images]
    _, proj, depth_values = synth.make_mvs_sample(21, img_hw=(H, W))
    sample = dict(imgs=torch.zeros(1, 3, 3, H, W, device=dev), depth_values=torch.from_numpy(depth_values).to(dev)[None],
                  proj_matrices={k: torch.from_numpy(v).to(dev)[None] for k, v in proj.items()})
    outputs, extra = None, None
    say("per stage, ms (hypotheses kernel | cost volume: warp + variance + regulariser | tail with uncertainty | tail without):")
    for st in range(3):
        key = f"stage{st + 1}"
        sc = (4, 2, 1)[st]
        D, h, w = args.ndepths[st], H // sc, W // sc
        fs = [f[key] for f in feats]
        prev = None if st == 0 else (outputs["depth"][0], extra[0])
        dv = costvol.host_copy(sample["depth_values"])[0]
        hypo = (lambda: costvol.uncertainty_hypotheses(None, None, (h, w), D, float(dv[0]), float(dv[-1]), False, dev)) if st == 0 else \
               (lambda: costvol.uncertainty_hypotheses(prev[0], prev[1], (h, w), D))
        hyp = hypo()
        cr = m.cost_regularization[st]

        def volume():
            return cr(costvol.warp_variance(fs, sample["proj_matrices"][key], hyp[None], split=True))[0, 0]
        with torch.no_grad():
            reg = volume()
            t_h, t_v = timed([hypo, volume], max(args.reps // 5, 3))
            t_tv, t_t = timed([lambda: costvol.prob_depth_conf_var(reg, hyp, 1.5), lambda: costvol.prob_depth_conf(reg, hyp)], args.reps)
            outputs, extra = m(st, sample, features=feats, extra=extra, outputs=outputs, int_r=None)
        say(f"  stage {st + 1} (D {D}, {h} x {w}): {fmt(t_h)} | {fmt(t_v)} | {fmt(t_tv)} | {fmt(t_t)}   "
            f"hypotheses {D * h * w * 4 / 2 ** 20:.0f} MiB, cost volume {fs[0].shape[1] * D * h * w * 4 / 2 ** 20:.0f} MiB, "
            f"variance {float(extra.min()):.3g} .. {float(extra.max()):.3g}")
        del reg, hyp
    say("launches per stage beside the regulariser's: 1 hypotheses + 1 warp / variance + 1 tail (the uncertainty adds none)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
