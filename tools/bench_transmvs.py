"""TransMVSNet at the workload's size (x2_mvsres: 1152 x 1536, 3 views, ndepths 192, 32, 8) with seeded weights:

  * the feature extractor, ms per image, and each of its nine deformable layers (offset convolution + svs_deform_conv2d)
    beside a plain-torch composition of the same layer on the same GPU (nine grid_samples plus an einsum);
  * the Feature Matching Transformer of one reference and one source view beside its torch einsum form, and the pathway;
  * per stage: similarity volume, regulariser (its conv0 on one input channel alone as well), winner-take-all tail;
  * operations and bytes, counted from the shapes.

    python tools/bench_transmvs.py [--out FILE (default profiles/transmvs_bench.txt)] [--hw 1152 1536] [--reps 10]

None of these times has a predecessor.  Needs the GPU: there is no fall-back, and nothing here is a time without one.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "s-volsdf_amd"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests"),
                os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

import synth  # noqa: E402
import transmvs_oracle as to  # noqa: E402
from models.blocks import fold_bn as _fold_bn  # noqa: E402
from models.transmvs import TransMVSNetHip  # noqa: E402
from svs_hip import costvol  # noqa: E402

BATCH = 5


def timed(fns, reps):
    """Per function: ms per call as (median, min, max) over `reps` batches of BATCH back-to-back calls, each batch between two
    device events, the functions alternating (two warm-up calls each first)."""
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


def torch_dcn(x, om, weight, bias):
    """the same layer in plain torch on the device: nine grid_samples plus an einsum (float32)"""
    return to.deform_conv2d_tv(x[None], om[None, :18], weight, bias, mask=torch.sigmoid(om[None, 18:]))[0]


def torch_layer(x, source, layer):
    at = layer.attention
    K = Fn.elu(at.key_projection(source).view(-1, 8, 4)) + 1
    V = at.value_projection(source).view(-1, 8, 4)
    Q = Fn.elu(at.query_projection(x).view(-1, 8, 4)) + 1
    KV = torch.einsum("shd,shm->hmd", K, V)
    Z = 1 / (torch.einsum("lhd,hd->lh", Q, K.sum(0)) + 1e-6)
    x = layer.norm1(x + at.out_projection(torch.einsum("lhd,hmd,lh->lhm", Q, KV, Z).reshape(-1, 32)))
    return layer.norm2(x + layer.linear2(Fn.relu(layer.linear1(x))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transmvs_bench.txt"))
    ap.add_argument("--hw", type=int, nargs=2, default=(1152, 1536))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ndepths", type=int, nargs=3, default=(192, 32, 8))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transmvs needs the GPU")
    dev = torch.device("cuda:0")
    H, W = args.hw
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    m = TransMVSNetHip(ndepths=list(args.ndepths), depth_interals_ratio=[4, 2, 1])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in to.transmvs_state_dict().items()}, strict=True)
    m.to(dev).eval()
    rng = np.random.default_rng(0)
    images = [torch.from_numpy(rng.uniform(0, 1, (1, 3, H, W)).astype(np.float32)).to(dev) for _ in range(3)]
    say(f"TransMVSNet, {H} x {W}, 3 views, ndepths {list(args.ndepths)}, seeded weights; {torch.cuda.get_device_name(0)}")
    say(f"times: median (min .. max) over {args.reps} batches of {BATCH} calls between device events: they include what the host takes to enqueue")

    with torch.no_grad():
        # ---- feature extractor
        t = timed([lambda: m.feature(images[0])], args.reps)
        say(f"feature extractor (8 FPN layers, 2 laterals, 3 branches of 1 convolution + 3 deformable layers), ms per image: {fmt(t[0])}")
        say("deformable layers alone, ms: offset convolution (svs_conv2d, 32 -> 27) | svs_deform_conv2d (float32) | torch: 9 grid_samples + einsum; "
            "GFLOP of the 3x3 product; max |kernel - torch| / output scale")
        for name, sc in (("out1", 4), ("out2", 2), ("out3", 1)):
            seq = getattr(m.feature, name)
            h, w = H // sc, W // sc
            x = torch.randn(32, h, w, device=dev).clamp(min=0)
            for i in (1, 4, 7):
                d = seq[i]
                bn = seq[i + 1] if i != 7 else None
                scale, shift = _fold_bn(bn) if bn is not None else (None, None)
                offs = lambda: costvol.conv2d(x, d.conv_offset_mask.weight.detach(), d.conv_offset_mask.bias.detach())
                om = offs()
                t_o, t_k, t_t = timed([offs, lambda: costvol.deform_conv2d(x, om, d.weight.detach(), d.bias.detach(), scale, shift, relu=bn is not None),
                                       lambda: torch_dcn(x, om, d.weight.detach(), d.bias.detach())], max(args.reps // 2, 3))
                got = costvol.deform_conv2d(x, om, d.weight.detach(), d.bias.detach())
                ref = torch_dcn(x, om, d.weight.detach(), d.bias.detach())
                gflop = 2 * 9 * 32 * d.out_channels * h * w / 1e9
                say(f"  {name}.{i} 32->{d.out_channels} at {h} x {w}: {fmt(t_o)} | {fmt(t_k)} ({gflop / t_k[0]:.1f} TFLOP/s) | {fmt(t_t)}; {gflop:.1f} GFLOP; "
                    f"{float((got - ref).abs().max() / ref.abs().max()):.1e}")
                del om, got, ref
            del x
        say("  (a matrix-core form of svs_deform_conv2d is not built: the float32 kernel is the only path)")

        # ---- transformer and pathway
        feats = [m.feature(im) for im in images]
        fm = m.FMT_with_pathway
        h1, w1 = H // 4, W // 4
        L = h1 * w1
        ref_run = lambda: fm.FMT(feats[0]["stage1"], feat="ref")
        ref_tok = ref_run()
        src_run = lambda: fm.FMT(ref_tok, feats[1]["stage1"], feat="src")

        def torch_ref():
            x = (feats[0]["stage1"][0] + to.pos_encoding(h1, w1, torch.float32).to(dev)).reshape(32, -1).t()
            outs = []
            for i in (0, 2, 4, 6):
                x = torch_layer(x, x, fm.FMT.layers[i])
                outs.append(x)
            return outs

        def torch_src():
            x = (feats[1]["stage1"][0] + to.pos_encoding(h1, w1, torch.float32).to(dev)).reshape(32, -1).t()
            for i in range(8):
                x = torch_layer(x, x if i % 2 == 0 else ref_tok[i // 2], fm.FMT.layers[i])
            return x.t().reshape(1, 32, h1, w1)
        t_r, t_s, t_tr, t_ts = timed([ref_run, src_run, torch_ref, torch_src], args.reps)
        err = float((src_run() - torch_src()).abs().max())
        say(f"Feature Matching Transformer, {L} tokens, ms: reference view (4 layers) {fmt(t_r)}, source view (8 layers) {fmt(t_s)}; "
            f"torch einsum form {fmt(t_tr)}, {fmt(t_ts)}; max |kernel - torch| on the source view {err:.1e}")
        t_p = timed([lambda: fm._pathway(feats[1]["stage1"], feats[1])], args.reps)
        say(f"pathway of one view (2 x (reduce + bilinear x2 + add) + 2 smoothing convolutions), ms: {fmt(t_p[0])}")
        t_all = timed([lambda: fm(feats)], max(args.reps // 2, 3))
        say(f"FMT_with_pathway on the 3 views of a sample, ms: {fmt(t_all[0])}")

        # ---- the three stages
        matched = fm(feats)
        _, proj, depth_values = synth.make_mvs_sample(to.FIXTURE_SEED, img_hw=(H, W))
        sample = dict(imgs=torch.zeros(1, 3, 3, H, W, device=dev), depth_values=torch.from_numpy(depth_values).to(dev)[None],
                      proj_matrices={k: torch.from_numpy(v).to(dev)[None] for k, v in proj.items()})
        outputs, extra = None, None
        net = m.DepthNet.pixel_wise_net.folded()
        say("per stage, ms: similarity volume (warp + view weights) | regulariser | of which conv0 (1 -> 8, svs_conv3d) | tail (svs_prob_wta)")
        for st in range(3):
            key = f"stage{st + 1}"
            sc = (4, 2, 1)[st]
            D, h, w = args.ndepths[st], H // sc, W // sc
            fs = [f[key] for f in matched]
            dv = costvol.host_copy(sample["depth_values"])[0]
            interval = (float(dv[-1]) - float(dv[0])) / len(dv)
            hyp = costvol.depth_hypotheses(None if st == 0 else outputs["depth"][0], (H, W), D, sc, float(dv[0]), float(dv[-1]),
                                           0.0 if st == 0 else m.depth_interals_ratio[st] * interval, False, dev)
            cr = m.cost_regularization[st]
            sim_run = lambda: costvol.warp_similarity(fs, sample["proj_matrices"][key], hyp[None], extra, net if extra is None else None)
            sim = sim_run()[0]
            reg = cr(sim)[0, 0]
            t_s, t_r, t_0 = timed([sim_run, lambda: cr(sim), lambda: cr.conv0(sim[0])], max(args.reps // 3, 3))
            t_t = timed([lambda: costvol.prob_wta(reg, hyp)], args.reps)
            outputs, extra = m(st, sample, features=matched, extra=extra, outputs=outputs, int_r=m.depth_interals_ratio[st])
            say(f"  stage {st + 1} (D {D}, {h} x {w}): {fmt(t_s)} | {fmt(t_r)} | {fmt(t_0)} | {fmt(t_t[0])}   volume {D * h * w * 4 / 2 ** 20:.0f} MiB, "
                f"view weights {float(extra.min()):.3g} .. {float(extra.max()):.3g}")
            del sim, reg, hyp
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
