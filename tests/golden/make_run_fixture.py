"""Builds tests/golden/run_config.json and tests/golden/depth_preview.npz on the CPU, from a checkout of the reference.

    python tests/golden/make_run_fixture.py [--reference DIR] [--out-dir DIR]     (DIR: default ref_shim.REFERENCE_ROOT)

run_config.json     {"dtu": {...}, "bmvs": {...}}: the configuration the reference's runner composes for vol=dtu and
                    vol=bmvs, read from its YAML files with PyYAML (hydra is not needed): config/vol/<name>.yaml under the
                    key `vol`, deep-merged with config/base.yaml and then config/ours.yaml, the `defaults` and `hydra` keys
                    dropped.  Settings only.  Under "lists": the scan names of config/lists/dtu.txt and bmvs.txt.
depth_preview.npz   the reference's own helpers/utils.py::visualize_depth -- the function's text is compiled from the
                    checkout at run time (the module itself imports OpenCV), nothing of it is stored -- called with a
                    stand-in `cv2` whose applyColorMap indexes a seeded random 256x3 table (BGR, as OpenCV's would be).
                    Cases at 1x1, 3x5 and 37x53 with NaN, +-inf, values exactly on the bounds, and values for which
                    scaled * 255 lands on and just under an integer; direct False and True; explicit bounds and None
                    bounds (the 5th / 95th percentile of the valid pixels).  Stored: table; per case {name}/depth (the
                    input, before the function clamps it in place), lo, hi (NaN for None), direct, out.
"""
import argparse
import ast
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import ref_shim  # noqa: E402


def deep_merge(base, over):
    out = dict(base)
    for k, v in over.items():
        out[k] = deep_merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


def composed(reference, vol):
    import yaml

    def load(rel):
        with open(os.path.join(reference, "config", rel)) as f:
            return yaml.safe_load(f)
    cfg = deep_merge(deep_merge({"vol": load(f"vol/{vol}.yaml")}, load("base.yaml")), load("ours.yaml"))
    for k in ("defaults", "hydra"):
        cfg.pop(k, None)
    return cfg


def reference_visualize_depth(reference, table):
    """the reference's function, compiled from its file with numpy and a stand-in cv2"""
    path = os.path.join(reference, "helpers", "utils.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "visualize_depth"]
    assert len(body) == 1
    cv2 = types.SimpleNamespace(COLORMAP_JET=2, applyColorMap=lambda codes, cmap: table[codes])
    ns = {"np": np, "cv2": cv2}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns["visualize_depth"]


def preview_inputs():
    """name -> (depth float32 (H,W), lo, hi): lo / hi np.float32, or None for the percentile bounds"""
    rng = np.random.default_rng(20240521)
    f32 = np.float32
    cases = {}
    cases["1x1_inside"] = (np.array([[3.25]], f32), f32(2.0), f32(7.5))
    cases["1x1_nan"] = (np.array([[np.nan]], f32), f32(2.0), f32(7.5))
    cases["1x1_on_hi"] = (np.array([[7.5]], f32), f32(2.0), f32(7.5))
    d = rng.uniform(400.0, 950.0, (3, 5)).astype(f32)
    d[0, 0], d[0, 1], d[1, 2], d[2, 4], d[2, 0] = np.nan, np.inf, -np.inf, 425.0, 935.0     # on lo, on hi
    cases["3x5"] = (d, f32(425.0), f32(935.0))
    cases["3x5_none"] = (d.copy(), None, None)
    d = rng.uniform(-20.0, 280.0, (37, 53)).astype(f32)
    k = np.arange(256, dtype=f32)
    flat = d.reshape(-1)
    flat[:256] = k                                       # scaled * 255 on an integer, or one ulp under it
    flat[256:512] = np.nextafter(k, f32(-1.0))           # just under
    flat[512:768] = np.nextafter(k, f32(300.0))          # just over
    flat[800:806] = [np.nan, np.inf, -np.inf, 0.0, 255.0, -0.0]
    cases["37x53_0_255"] = (d, f32(0.0), f32(255.0))
    d = rng.uniform(0.0, 1.0, (37, 53)).astype(f32) ** 3
    d.reshape(-1)[[5, 77, 1000, 1960]] = [np.nan, np.inf, -np.inf, np.nan]
    lo, hi = f32(0.0123), f32(0.71)
    d.reshape(-1)[[6, 7]] = [lo, hi]
    cases["37x53"] = (d, lo, hi)
    cases["37x53_none"] = (d.copy(), None, None)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SVOLSDF_REFERENCE_ROOT", ref_shim.REFERENCE_ROOT))
    ap.add_argument("--out-dir", default=HERE)
    a = ap.parse_args()

    cfg = {vol: composed(a.reference, vol) for vol in ("dtu", "bmvs")}
    for vol, c in list(cfg.items()):
        print(f"  {vol}: {len(c)} top-level keys, num_pixels {c['vol']['train']['num_pixels']}, near "
              f"{c['vol']['model']['ray_sampler']['near']}, confi {c['vol']['loss']['confi']}")
    cfg["lists"] = {}
    for name in ("dtu", "bmvs"):
        with open(os.path.join(a.reference, "config", "lists", f"{name}.txt")) as f:
            cfg["lists"][name] = [line.strip() for line in f if line.strip()]
    path = os.path.join(a.out_dir, "run_config.json")
    with open(path, "w") as f:
        json.dump(cfg, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")

    table = np.random.default_rng(7).integers(0, 256, (256, 3), dtype=np.uint8)
    visualize_depth = reference_visualize_depth(a.reference, table)
    arr = {"table": table}
    for name, (depth, lo, hi) in preview_inputs().items():
        for direct in (False, True):
            key = f"{name}/{'direct' if direct else 'color'}"
            with np.errstate(invalid="ignore"):
                out = visualize_depth(depth.copy(), depth_min=lo, depth_max=hi, direct=direct)
            arr[f"{key}/depth"] = depth
            arr[f"{key}/lo"] = np.float32(np.nan if lo is None else lo)
            arr[f"{key}/hi"] = np.float32(np.nan if hi is None else hi)
            arr[f"{key}/direct"] = np.asarray(direct)
            arr[f"{key}/out"] = out
            assert out.dtype == np.uint8 and out.shape == depth.shape + (() if direct else (3,))
    path = os.path.join(a.out_dir, "depth_preview.npz")
    np.savez_compressed(path, **arr)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB), {len(preview_inputs())} inputs x 2 modes")


if __name__ == "__main__":
    main()
