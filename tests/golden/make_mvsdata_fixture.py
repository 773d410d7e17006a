"""Builds tests/golden/mvsdata_ref.npz: the reference's own MVSDataset (datasets/general_eval.py:12-273) run on the
synthetic scan folders of tests/mvsdata_oracle.py::CASES.

    python tests/golden/make_mvsdata_fixture.py [--out FILE]     (needs the reference checkout, see ref_shim.REFERENCE_ROOT)

The class is imported unmodified through ref_shim's stubs (the image lacks OpenCV and loguru) with two cv2 names bound to
restatements: cv2.resize to tests/scene_oracle.py::resize_cubic, its result rounded to float32 as cv2 returns it for a
float32 image (a resize to the same size copies), and cv2.decomposeProjectionMatrix to
mvsdata_oracle.decompose_projection_matrix.  The BlendedMVS folder name is taken from the reference's scan2hash at run
time and not stored.

Stored per case ("dtu", "bmvs": every array of every sample; "x2": x2_mvsres at 1200x1600 -> 576x768 -> 1152x1536, host
metadata and the sizes only): {case}/sample{i}/proj_matrices/stage{1,2,3}, depth_values, cam_near_far, filename, view_ids;
{case}/view{id}/imgs|masks, each view's planes once -- the samples of a scan hold the same views in different orders, which
the script asserts before it drops the copies; {case}/metas, scale_factor, interval_scale, hw.
"""
import argparse
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import ref_shim  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "mvsdata_ref.npz"))
    a = ap.parse_args()
    ref_shim.install()
    import cv2
    import mvsdata_oracle as mo
    import scene_oracle as so

    sizes = []

    def resize(img, dsize, interpolation=None):
        assert interpolation == cv2.INTER_CUBIC and img.dtype == np.float32
        sizes.append((int(dsize[1]), int(dsize[0])))
        if img.shape[:2] == (dsize[1], dsize[0]):
            return img.copy()
        return so.resize_cubic(img, (dsize[1], dsize[0])).astype(np.float32)
    cv2.INTER_CUBIC = 2
    cv2.resize = resize
    cv2.decomposeProjectionMatrix = mo.decompose_projection_matrix
    from datasets.general_eval import MVSDataset
    from volsdf.datasets.scene_dataset import scan2hash

    arr = {}
    for name, case in mo.CASES.items():
        root = tempfile.mkdtemp(prefix="svs_mvsdata_")
        try:
            scan = f"scan{case['scan']['scan']}"
            folder = scan2hash(scan) if case["scan"]["dataset"] == "BlendedMVS" else None
            ds = mo.build_case(name, root, MVSDataset, folder=folder)
            del sizes[:]
            if case["x2"]:
                # the sizes and the metadata need the arithmetic only: the resize itself is replaced by an empty image
                cv2.resize = lambda img, dsize, interpolation=None: (sizes.append((int(dsize[1]), int(dsize[0]))),
                                                                     np.zeros((dsize[1], dsize[0], img.shape[2]), np.float32))[1]
                flat = mo.flatten(ds, images=True)
                flat = {k: v for k, v in flat.items() if not k.startswith("view")}
                cv2.resize = resize
            else:
                flat = mo.flatten(ds, images=True)
            flat["metas"] = np.asarray([[m[1]] + list(m[2]) + [-1] * (8 - len(m[2])) for m in ds.metas])
            flat["scale_factor"] = np.asarray(ds.scale_factor)
            flat["interval_scale"] = np.asarray(ds.interval_scale[scan])
            flat["n_images"] = np.asarray(len(ds.image_paths_idr))
            flat["passes"] = np.asarray(sizes[:2 if case["x2"] else 1])
            assert all(s == sizes[k % len(flat["passes"])] for k, s in enumerate(sizes))
            print(f"  {name}: {len(ds)} samples, passes {flat['passes'].tolist()}, views "
                  f"{[flat[f'sample{i}/view_ids'].tolist() for i in range(len(ds))]}, depth "
                  f"{flat['sample0/cam_near_far'].tolist()}")
            arr.update({f"{name}/{k}": v for k, v in flat.items()})
        finally:
            shutil.rmtree(root, ignore_errors=True)
    np.savez_compressed(a.out, **arr)
    print(f"  wrote {a.out} ({os.path.getsize(a.out) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
