"""Golden vectors of TransMVSNet: imports the REFERENCE's models/TransMVSNet.py (read-only checkout, ref_shim.REFERENCE_ROOT)
on the CPU and stores arrays only -- tests/golden/transmvs_3stage.npz.  No reference source is stored.

Run:  python tests/golden/make_transmvs_fixture.py

torchvision is not installed here: ref_shim stubs `torchvision.ops.deform_conv2d = None`, and before the reference is imported
that stub is replaced by transmvs_oracle.deform_conv2d_tv, the float-preserving restatement (one grid_sample per tap), which
tests/test_transmvs_cpu.py checks three independent ways.

A 64 x 96 image, 3 views, ndepths [16, 8, 8].  Seeded weights (transmvs_oracle.transmvs_state_dict); each property the
default initialisation lacks is asserted below: offsets of several pixels with samples outside the image, features of order 1
at every stage behind the pathway, view weights that vary over the image.  Arrays above transmvs_oracle.PIN_ABOVE elements are
pinned at transmvs_oracle.pin_positions (name_val, name_shape).
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"), os.path.dirname(HERE), HERE):
    sys.path.insert(0, p)
import ref_shim  # noqa: E402

ref_shim.install()
import torch  # noqa: E402

import transmvs_oracle as to  # noqa: E402

sys.modules["torchvision.ops"].deform_conv2d = to.deform_conv2d_tv

torch.set_num_threads(4)
F32 = np.float32


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def main():
    from models.TransMVSNet import TransMVSNet          # the reference's (ref_shim.install() put its checkout first on sys.path)
    assert os.path.realpath(sys.modules["models.TransMVSNet"].__file__).startswith(os.path.realpath(ref_shim.REFERENCE_ROOT))
    arr = {}
    model = TransMVSNet(refine=False, ndepths=list(to.FIXTURE_NDEPTHS), depth_interals_ratio=list(to.FIXTURE_RATIOS), share_cr=False,
                        grad_method="detach", arch_mode="fpn", cr_base_chs=[8, 8, 8])
    sd = to.transmvs_state_dict()
    model.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    model.eval()
    assert "FMT_with_pathway.FMT.pos_encoding.pe" not in model.state_dict() and len(model.state_dict()) == 465
    arr["state_dict_keys"] = np.asarray(list(model.state_dict().keys()))
    arr["state_dict_shapes"] = np.asarray([",".join(str(n) for n in v.shape) for v in model.state_dict().values()])
    for k, v in sd.items():
        if ".norm" in k:
            assert np.abs(v - (1.0 if k.endswith("weight") else 0.0)).min() > 1e-3, k
        if "running_mean" in k:
            assert np.abs(v).max() > 0.05, k
        if "running_var" in k:
            assert np.abs(v - 1).max() > 0.1, k

    # ---- the feature extractor on one image; the offsets every DCN sees
    img = to.fixture_image()
    seen = []
    hooks = [m.conv_offset_mask.register_forward_hook(lambda m, i, o: seen.append(o[0, :18].detach().numpy().copy()))
             for m in model.feature.modules() if hasattr(m, "conv_offset_mask")]
    with torch.no_grad():
        f = model.feature(T(img)[None])
    for h in hooks:
        h.remove()
    assert len(seen) == 9
    for off in seen:
        H, W = off.shape[1:]
        assert np.abs(off).mean() > 1.0 and np.abs(off).max() > 3.0, "offsets of several pixels"
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        outside = 0
        for k in range(9):
            y, x = yy + k // 3 - 1 + off[2 * k], xx + k % 3 - 1 + off[2 * k + 1]
            outside += ((y <= -1) | (y >= H) | (x <= -1) | (x >= W)).sum()
        assert outside > 0, "some samples fall outside the image"
    for k in ("stage1", "stage2", "stage3"):
        to.put(arr, "feat_" + k, f[k][0].numpy())
        assert 0.3 < f[k].std() < 5.0, (k, float(f[k].std()))
    print("  extractor: std", [round(float(f[k].std()), 2) for k in ("stage1", "stage2", "stage3")],
          "mean |offset|", [round(float(np.abs(o).mean()), 2) for o in seen])

    # ---- the transformer and its pathway on the sample's features (the reference overwrites its input: a copy goes in)
    feats, proj, depth_values = to.fixture_sample()
    features = [{k: T(v)[None] for k, v in ft.items()} for ft in copy.deepcopy(feats)]
    ref_outs = []
    orig = model.FMT_with_pathway.FMT.forward

    def wrapped(*a, **kw):
        out = orig(*a, **kw)
        if kw.get("feat") == "ref":
            ref_outs.extend(o[0].detach().numpy().copy() for o in out)
        return out
    model.FMT_with_pathway.FMT.forward = wrapped
    with torch.no_grad():
        features = model.FMT_with_pathway(features)
    model.FMT_with_pathway.FMT.forward = orig
    assert len(ref_outs) == 4
    for i, o in enumerate(ref_outs):
        to.put(arr, f"fmt_ref{i}", o)
    for v in range(3):
        for k in ("stage1", "stage2", "stage3"):
            a = features[v][k][0].numpy()
            if v < 2:
                to.put(arr, f"fmt_v{v}_{k}", a)
            assert 0.3 < a.std() < 5.0, (v, k, float(a.std()))        # every stage's features of order 1
    print("  matched features: std", [[round(float(features[v][k].std()), 2) for k in ("stage1", "stage2", "stage3")] for v in range(3)])

    # ---- three stages
    H, W = to.FIXTURE_HW
    sample = dict(imgs=torch.zeros(1, 3, 3, H, W), depth_values=T(depth_values)[None],
                  proj_matrices={k: T(v)[None] for k, v in proj.items()})
    outputs, extra = None, None
    for st in range(3):
        cap = {}
        cr = model.cost_regularization[st]
        orig = cr.forward

        def wrapped(x, _o=orig, _c=cap):
            _c["sim"] = x.detach().numpy().copy()
            y = _o(x)
            _c["reg"] = y.detach().numpy().copy()
            return y
        cr.forward = wrapped
        with torch.no_grad():
            outputs, extra = model(st, sample, features=features, extra=extra, outputs=outputs,
                                   int_r=model.depth_interals_ratio[st])
        cr.forward = orig
        o = outputs[f"stage{st + 1}"]
        to.put(arr, f"s{st}_similarity", cap["sim"][0, 0])
        arr[f"s{st}_reg"] = cap["reg"][0, 0]                    # whole: the tail and the near-tie cap run on it
        to.put(arr, f"s{st}_prob", o["prob_volume"][0].numpy())
        to.put(arr, f"s{st}_depth_values", o["depth_values"][0].numpy())
        arr[f"s{st}_depth"] = o["depth"][0].numpy().copy()
        arr[f"s{st}_conf"] = o["photometric_confidence"][0].numpy()
        if st == 0:
            arr["s0_view_weights"] = extra[0].numpy().copy()
            w = arr["s0_view_weights"]
            assert w.max() > 10 * w.min() and w.std() > 0.02, (w.min(), w.max(), w.std())     # they vary over the image
        else:
            assert np.array_equal(extra[0].numpy(), to.upsample_nearest2(arr["s0_view_weights"], st))
        gap = to.top_two_gap(arr[f"s{st}_reg"])
        print(f"  stage {st + 1}: depth {arr[f's{st}_depth'].min():.1f} .. {arr[f's{st}_depth'].max():.1f}, view weights "
              f"{extra.min():.2e} .. {extra.max():.3f}, top-two gap below 1e-3 at {100 * (gap < 1e-3).mean():.2f} %, median {np.median(gap):.3f}")
    path = os.path.join(HERE, "transmvs_3stage.npz")
    np.savez_compressed(path, seed=to.FIXTURE_SEED, ndepths=np.asarray(to.FIXTURE_NDEPTHS), ratios=np.asarray(to.FIXTURE_RATIOS), **arr)
    print(f"  wrote transmvs_3stage.npz  ({os.path.getsize(path) / 1024:.1f} KiB)")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
