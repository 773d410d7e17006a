"""Builds tests/golden/evalviews_finish.npz: the reference's per-view finish of evaluation rendering
(eval_vsdf.py:230-262 with volsdf/utils/plots.py's lin2img / visualize_depth / visualize_cmap / weighted_percentile /
matte) run on seeded per-ray arrays.

    python tests/golden/make_evalviews_fixture.py          (needs the reference checkout, see ref_shim.REFERENCE_ROOT)

eval_vsdf.py cannot be imported (TensorFlow, lpips_tf, pyhocon, GPUtil at module level), so the statements that follow
`model_outputs = utils.merge_output(...)` in its rendering branch are taken from the file with `ast` and executed
unmodified with: the reference's own `volsdf.utils.plots` as `plt` (imported through ref_shim with plotly, skimage,
torchvision, trimesh and cv2 stubbed: the finish uses none of them), numpy / torch / PIL, and a `save_pfm` that keeps the
array.  matplotlib 3.9 dropped `matplotlib.cm.get_cmap`, which visualize_depth calls: it is bound to
`matplotlib.colormaps.get_cmap` for the run.  The PNG files the statements write are read back with PIL.

Inputs (48x64 pixels, S = 98): colours in [0,1), normals with components beyond +-1 (codes wrap), depths 1.1..4.3 with a
step and noise, weights whose row sums run from 0 to slightly above 1 (a block of rows below 0.2), scale_factor 2.625.

Stored: the inputs, the reference's four products (rgb / normal / depth colour codes, depth_est), `acc` as the reference
summed it, the two percentile bounds visualize_cmap found (captured from weighted_percentile) and the versions of matplotlib and
numpy that ran.  Arrays only; the colour table is not stored (the tests take it from matplotlib).
"""
import ast
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import ref_shim  # noqa: E402

SEED = 23
H, W, S = 48, 64, 98
SCALE = np.float32(2.625)
VIEW = 7


def make_inputs(seed=SEED, hw=(H, W), n_samples=S):
    """Seeded per-ray arrays in merge_output's shapes: rgb_values (N,3), normal_map (N,3), depth_values (N,), weights (N,S)."""
    h, w = hw
    n = h * w
    rng = np.random.default_rng(seed)
    rgb = rng.random((n, 3)).astype(np.float32)
    normal = (rng.standard_normal((n, 3)) * 0.8).astype(np.float32)
    normal[::97] *= 40.0                                   # far outside [-1, 1]: codes wrap several times
    yy, xx = np.mgrid[0:h, 0:w]
    depth = 1.2 + 1.5 * (xx / w) + 0.8 * (yy / h) + np.where(xx > w // 2, 0.7, 0.0) + rng.normal(0, 0.02, (h, w))
    depth = np.clip(depth, 0.6, 6.0).reshape(-1).astype(np.float32)
    wts = rng.random((n, n_samples)) ** 4
    wts[rng.random((n, n_samples)) < 0.6] = 0.0             # as in a render, most samples of a ray carry no weight
    wts[:, 0] += 1e-3
    target = np.clip(rng.beta(5, 1, n) * 1.02, 0, None)     # row sums: mostly near 1, a few slightly above
    target[(yy < h // 4).reshape(-1) & (xx < w // 3).reshape(-1)] *= 0.15          # a block below 0.2
    target[::53] = 0.0
    wts = (wts / wts.sum(1, keepdims=True) * target[:, None]).astype(np.float32)
    return dict(rgb_values=rgb, normal_map=normal, depth_values=depth, weights=wts)


def reference_finish_statements():
    """The statements of eval_vsdf.py's rendering branch after `model_outputs = utils.merge_output(...)`."""
    path = os.path.join(ref_shim.REFERENCE_ROOT, "eval_vsdf.py")
    tree = ast.parse(open(path).read(), path)
    for node in ast.walk(tree):
        if not isinstance(node, ast.If):
            continue
        for k, st in enumerate(node.orelse):
            if isinstance(st, ast.Assign) and "merge_output" in ast.dump(st.value):
                body = [s for s in node.orelse[k + 1:] if "empty_cache" not in ast.dump(s)]
                return compile(ast.Module(body=body, type_ignores=[]), path, "exec")
    raise RuntimeError("the rendering branch of eval_vsdf.py was not found")


def main():
    import matplotlib
    import matplotlib.cm as cm
    import torch
    from PIL import Image

    ref_shim.install()
    for name in ("plotly", "plotly.graph_objs", "plotly.offline"):
        ref_shim._stub(name)
    ref_shim._stub("plotly.subplots", make_subplots=None)
    sys.modules["skimage"].measure = sys.modules["skimage.measure"]
    if not hasattr(cm, "get_cmap"):
        cm.get_cmap = matplotlib.colormaps.get_cmap
    import volsdf.utils.plots as plots
    assert plots.__file__.startswith(ref_shim.REFERENCE_ROOT)

    seen = {}
    ref_wp = plots.weighted_percentile

    def spy(x, w, ps, assume_sorted=False):
        out = ref_wp(x, w, ps, assume_sorted)
        seen["bounds"] = np.asarray(out, np.float64)
        return out
    plots.weighted_percentile = spy

    inp = make_inputs()
    kept = {}
    out_dir = tempfile.mkdtemp(prefix="svs_evalviews_")
    os.makedirs(os.path.join(out_dir, "depth_est"))
    ns = dict(np=np, torch=torch, Image=Image, plt=plots, img_res=[H, W], total_pixels=H * W, batch_size=1,
              images_dir=out_dir, indices=torch.tensor([VIEW]), eval_dataset=types.SimpleNamespace(scale_factor=SCALE),
              save_pfm=lambda fn, a: kept.update(depth_est=np.array(a), depth_est_name=os.path.basename(fn)),
              model_outputs={"rgb_values": torch.from_numpy(inp["rgb_values"]),
                             "normal_map": torch.from_numpy(inp["normal_map"]),
                             "depth_values": torch.from_numpy(inp["depth_values"]),
                             "weights": torch.from_numpy(inp["weights"])})
    with np.errstate(invalid="ignore"):
        exec(reference_finish_statements(), ns)
    assert kept["depth_est_name"] == "%08d.pfm" % VIEW and kept["depth_est"].dtype == np.float32

    def png(name):
        with Image.open(os.path.join(out_dir, name % VIEW)) as im:
            return np.array(im)
    out = dict(inp, scale_factor=SCALE, img_res=np.array([H, W]), view=np.array(VIEW), seed=np.array(SEED),
               rgb_codes=png("eval_%03d.png"), normal_codes=png("normal_%03d.png"), depth_codes=png("dep_%03d.png"),
               depth_est=kept["depth_est"], acc=np.asarray(ns["acc"], np.float32), bounds=seen["bounds"],
               matplotlib_version=np.array(matplotlib.__version__), numpy_version=np.array(np.__version__))
    for k in ("rgb_codes", "normal_codes", "depth_codes"):
        assert out[k].shape == (H, W, 3) and out[k].dtype == np.uint8
    dst = os.path.join(HERE, "evalviews_finish.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes; bounds", seen["bounds"], "acc range", out["acc"].min(), out["acc"].max())


if __name__ == "__main__":
    main()
