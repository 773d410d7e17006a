"""Golden vectors of UCSNet: imports the REFERENCE's models/ucsnet.py (read-only checkout, ref_shim.REFERENCE_ROOT) on the CPU
and stores arrays only -- tests/golden/ucsnet_3stage.npz.  No reference source is stored.

Run:  python tests/golden/make_ucsnet_fixture.py

A 64 x 96 image, 3 views, stage_configs [16, 8, 8], lamb 1.5.  Seeded weights (default-initialised ones give a flat
probability: variance about 1.8 everywhere, depth constant to 1e-2): the regularisers from synth.make_costreg_params under
UCSNet's attribute names, the feature extractor from ucsnet_oracle.make_featext_params (BatchNorm with non-trivial running
statistics).  Arrays above ucsnet_oracle.PIN_ABOVE elements are pinned at sampled positions (name_idx, name_val, name_shape).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"), os.path.dirname(HERE), HERE):
    sys.path.insert(0, p)
import ref_shim  # noqa: E402

ref_shim.install()
import torch  # noqa: E402

import ucsnet_oracle as uo  # noqa: E402

torch.set_num_threads(4)
F32 = np.float32


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def main():
    from models.ucsnet import UCSNet           # the reference's (ref_shim.install() put its checkout first on sys.path)
    assert os.path.realpath(sys.modules["models.ucsnet"].__file__).startswith(os.path.realpath(ref_shim.REFERENCE_ROOT))
    arr = {}

    def put(name, a):
        a = np.ascontiguousarray(a)
        if a.size > uo.PIN_ABOVE:
            idx = uo.pin_positions(name, a.size)
            arr[name + "_idx"], arr[name + "_val"], arr[name + "_shape"] = idx, a.reshape(-1)[idx], np.asarray(a.shape)
        else:
            arr[name] = a

    model = UCSNet(lamb=uo.FIXTURE_LAMB, stage_configs=list(uo.FIXTURE_NDEPTHS), grad_method="detach", base_chs=[8, 8, 8],
                   feat_ext_ch=8)
    sd = uo.ucsnet_state_dict()
    model.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    model.eval()
    names = list(model.state_dict().keys())
    arr["state_dict_keys"] = np.asarray(names)
    arr["state_dict_shapes"] = np.asarray([",".join(str(n) for n in v.shape) for v in model.state_dict().values()])

    # ---- the feature extractor on one image, with the transposed layers' raw outputs
    img = uo.fixture_image()
    raw = {}
    fe = model.feature_extraction
    hooks = [fe.deconv1.deconv.conv.register_forward_hook(lambda m, i, o: raw.__setitem__("deconv1_raw", o[0].detach().numpy().copy())),
             fe.deconv2.deconv.conv.register_forward_hook(lambda m, i, o: raw.__setitem__("deconv2_raw", o[0].detach().numpy().copy()))]
    with torch.no_grad():
        f = fe(T(img)[None])
    for h in hooks:
        h.remove()
    for k in ("stage1", "stage2", "stage3"):
        put("feat_" + k, f[k][0].numpy())
    put("feat_deconv1_raw", raw["deconv1_raw"])
    put("feat_deconv2_raw", raw["deconv2_raw"])
    assert np.abs(f["stage3"].numpy()).max() > 0.1

    # ---- three stages
    feats, proj, depth_values = uo.fixture_sample()
    H, W = uo.FIXTURE_HW
    sample = dict(imgs=torch.zeros(1, 3, 3, H, W), depth_values=T(depth_values)[None],
                  proj_matrices={k: T(v)[None] for k, v in proj.items()})
    features = [{k: T(v)[None] for k, v in ft.items()} for ft in feats]
    outputs, extra = None, None
    for st in range(3):
        cap = {}
        cr = model.cost_regularization[st]
        orig = cr.forward

        def wrapped(x, _o=orig, _c=cap):
            _c["variance"] = x.detach().numpy().copy()
            y = _o(x)
            _c["reg"] = y.detach().numpy().copy()
            return y
        cr.forward = wrapped
        outputs, extra = model(st, sample, features=features, extra=extra, outputs=outputs, int_r=None)
        cr.forward = orig
        o = outputs[f"stage{st + 1}"]
        assert extra is o["variance"]
        vol = cap["variance"][0]
        pick = np.random.default_rng(50 + st).choice(vol.size, 4000, replace=False).astype(np.int32)
        arr[f"s{st}_volume_idx"] = pick                       # the cost volume (C,D,H,W) is MBs: 4000 voxels
        arr[f"s{st}_volume_val"] = vol.reshape(-1)[pick]
        arr[f"s{st}_reg"] = cap["reg"][0, 0]                  # whole: the tests run the tail on it
        put(f"s{st}_prob", o["prob_volume"][0].numpy())
        arr[f"s{st}_depth_values"] = o["depth_values"][0].numpy()      # whole, with the logits: the tail runs at every stage
        arr[f"s{st}_depth"] = o["depth"][0].numpy().copy()
        arr[f"s{st}_conf"] = o["photometric_confidence"][0].numpy()
        arr[f"s{st}_variance"] = o["variance"][0].numpy()
        if st == 0:
            v = arr["s0_variance"]
            assert v.max() >= 3.0 * v.min() > 0, (v.min(), v.max())        # the uncertainty varies over the image
            # what runner.py:240-243 does: the rendered depth replaces the MVS depth that seeds stage 2
            smooth = outputs["depth"] * 0.98 + 4.0
            outputs["stage1"]["depth"] = smooth
            outputs["depth"] = smooth
            arr["stage1_depth_override"] = smooth[0].numpy()
        print(f"  stage {st + 1}: depth {arr[f's{st}_depth'].min():.1f} .. {arr[f's{st}_depth'].max():.1f}, variance "
              f"{arr[f's{st}_variance'].min():.3f} .. {arr[f's{st}_variance'].max():.3f}")
    path = os.path.join(HERE, "ucsnet_3stage.npz")
    np.savez_compressed(path, seed=uo.FIXTURE_SEED, ndepths=np.asarray(uo.FIXTURE_NDEPTHS), lamb=uo.FIXTURE_LAMB, **arr)
    print(f"  wrote ucsnet_3stage.npz  ({os.path.getsize(path) / 1024:.1f} KiB)")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
