"""The float64 gather of the painter and the atlas baker is one function (tests/meshpaint_oracle.py `gather`); before it was
one, `meshpaint_oracle.paint` and `meshtexture_oracle.gather` each held the loop.  tests/golden/paint_gather.npz holds what
those two returned, recorded at the last commit that had both: accumulators and fragile flags on the scene of
test_meshtexture_cpu.py and on the 33 x 33 exact images of test_meshpaint_cpu.py, both modes, with and without normals,
one-sided, masked, power 0 and 2, a second call on top of a first one's accumulators, and the bake of a few faces at cell 6
(float64 points that no float32 holds).  `compute()` is the recipe the file was made by; the test wants every bit of it."""
import os

import numpy as np

import meshpaint_oracle as mp
import meshtexture_cases as cases
import meshtexture_oracle as mt
import meshview_oracle as mv
from test_meshpaint_cpu import exact_images, exact_views, pixel_vertex

SCENE_RULES = [dict(), dict(mode="best"), dict(use_normals=False), dict(use_normals=False, mode="best"), dict(one_sided=True),
               dict(one_sided=True, mode="best", power=1), dict(power=0), dict(power=0, mode="best"), dict(cos_min=0.5, power=8)]
VERTEX_STEP, FACE_STEP, CELL = 8, 48, 6


def _name(prefix, rules, masked):
    return prefix + "/" + ("-".join(f"{k}={v}" for k, v in rules.items()) or "defaults") + ("-masked" if masked else "")


def compute():
    """-> {name: (acc float64, fragile bool)}"""
    out = {}
    # the scene: every VERTEX_STEP-th vertex through `paint`, three cameras, the oracle's own depth maps
    s = cases.scene()
    views = mv.cameras(3)
    depth, images = cases.rastered(s, views)["depth"], cases.photographs(s, views)
    normals = mp.vertex_normals(s["verts"], s["faces"])[0].astype(np.float32)
    at = slice(None, None, VERTEX_STEP)
    for i, rules in enumerate(SCENE_RULES):
        kw = {k: v for k, v in rules.items() if k != "use_normals"}
        n = normals[at] if rules.get("use_normals", True) else None
        for masked in ((False, True) if i < 4 else (i % 2 == 0,)):
            out[_name("scene", rules, masked)] = mp.paint(s["verts"][at], n, views, depth, images, cases.masks_for(3) if masked else None, **kw)
    for mode in ("blend", "best"):                            # two calls: the second starts from the first one's accumulators
        first = mp.paint(s["verts"][at], normals[at], views[:2], depth[:2], images[:2], mode=mode)[0]
        out[f"scene/two-calls-{mode}"] = mp.paint(s["verts"][at], normals[at], views[2:], depth[2:], images[2:], mode=mode, acc=first)
    # the bake: every FACE_STEP-th face in an atlas of its own; texel points and normals are float64 combinations
    faces = s["faces"][::FACE_STEP]
    chart, counts = mt.slots(s["verts"], faces)
    size = cases.atlas_size(counts[0], CELL)
    slot_face = mt.layout(chart, size, CELL)[1]
    for rules, masked in ((dict(), False), (dict(mode="best"), True), (dict(use_normals=False), True),
                          (dict(one_sided=True, power=0, mode="best"), False)):
        kw = {k: v for k, v in rules.items() if k != "use_normals"}
        n = normals if rules.get("use_normals", True) else None
        out[_name("bake", rules, masked)] = mt.bake(s["verts"], n, faces, chart, slot_face, size, CELL, views, depth, images,
                                                    cases.masks_for(3) if masked else None, **kw)
    # the exact images: pixel centres, half pixels, the last column, footprints off the image, and the vertex all three see
    ev, img = exact_views(), exact_images()
    zero = np.zeros((3, 33, 33), np.float32)
    verts = np.array([pixel_vertex(3, 5), pixel_vertex(3.5, 5.5), pixel_vertex(32, 0), pixel_vertex(32.25, 5), pixel_vertex(-0.25, 5),
                      [0, 0, 2.0], pixel_vertex(7.3, 20.6)], np.float32)
    towards = np.tile(np.float32([0, 0, -1]), (len(verts), 1))
    mask = np.ones((33, 33), np.uint8)
    mask[16, 16] = 0
    for mode in ("blend", "best"):
        for tag, n, kw in (("none", None, {}), ("towards", towards, {}), ("away", -towards, {}), ("away-one-sided", -towards, dict(one_sided=True)),
                           ("power0", towards, dict(power=0)), ("cos0.8", towards, dict(cos_min=0.8))):
            for masked in (False, True):
                out[f"exact/{mode}-{tag}" + ("-masked" if masked else "")] = mp.paint(verts, n, ev, zero, img, [mask, None, None] if masked else None,
                                                                                     mode=mode, **kw)
    return out


def test_the_one_gather_reproduces_what_the_two_returned(golden_dir):
    want = np.load(os.path.join(golden_dir, "paint_gather.npz"))
    got = compute()
    assert sorted(want.files) == sorted(f"{k}/{part}" for k in got for part in ("acc", "fragile"))
    baked = 0
    for name, (acc, fragile) in got.items():
        assert acc.dtype == np.float64 and want[name + "/acc"].dtype == np.float64 and fragile.dtype == bool, name
        assert acc.shape == want[name + "/acc"].shape and np.array_equal(acc.view(np.int64), want[name + "/acc"].view(np.int64)), name
        assert np.array_equal(fragile, want[name + "/fragile"]), name
        baked += int((acc[..., 3] > 0).sum())
    assert baked > 1000                                       # the cases are not empty ones
