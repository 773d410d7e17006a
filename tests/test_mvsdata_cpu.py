"""The MVS loader without a GPU (svs_hip/mvsdata.py): the dataset surface on synthetic scan folders against what the
reference's own class returned on them (tests/golden/mvsdata_ref.npz, made by tests/golden/make_mvsdata_fixture.py), with
the image work -- `prepare_views`, the single seam to the GPU -- bound to the oracle (tests/mvsdata_oracle.py); the size
arithmetic, the decode count, create_scene's files, the reference's asserts, and the argument checks of the C entry
points (nothing is launched).

Tolerances: keys, dtypes, shapes, view order, filename, depth_values and cam_near_far equal; proj_matrices as
tests/test_scene_cpu.py compares cameras (1e-5 * max(1, |w|max) for the intrinsics, 1e-5 for the extrinsics: the RQ
decomposition is numpy's here and Gram-Schmidt in the fixture); images within 1e-7 of the oracle."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mvsdata_oracle as mo

REFERENCE = os.environ.get("SVOLSDF_REFERENCE_ROOT", "/root/reference")
HAVE_REFERENCE = os.path.isfile(os.path.join(REFERENCE, "datasets", "general_eval.py"))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMAGE_TOL, CAM_TOL = 1e-7, 1e-5
FOLDER = "0123456789abcdef01234567"          # a made-up BlendedMVS folder name: the real table is the reference's


@pytest.fixture()
def mvsdata(monkeypatch):
    from svs_hip import mvsdata as md
    saved = dict(md._HASH)
    monkeypatch.setattr(md, "prepare_views", mo.prepare_views)
    yield md
    md._HASH.clear()
    md._HASH.update(saved)


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "mvsdata_ref.npz")))


def _case(fix, name):
    return {k[len(name) + 1:]: v for k, v in fix.items() if k.startswith(name + "/")}


def _compare(got, want, images):
    """two flattened datasets (mvsdata_oracle.flatten): see the module docstring"""
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        if "proj_matrices" in k:
            assert w.dtype == np.float32 and w.shape[1:] == (2, 4, 4)
            e_ext = float(np.abs(g[:, 0] - w[:, 0]).max())
            e_int = float(np.abs(g[:, 1] - w[:, 1]).max())
            assert e_ext <= CAM_TOL and e_int <= CAM_TOL * max(1.0, float(np.abs(w[:, 1]).max())), (k, e_ext, e_int)
        elif k.startswith("view"):
            assert images and w.dtype == np.float32
            assert float(np.abs(g - w).max()) <= IMAGE_TOL, k
        else:
            assert np.array_equal(g, w), (k, g, w)


def _flat(ds, scan, images, passes):
    flat = mo.flatten(ds, images=images)
    if not images:
        for i in range(len(ds)):
            flat[f"sample{i}/view_ids"] = np.asarray(ds.view_ids(i))
    flat["metas"] = np.asarray([[m[1]] + list(m[2]) + [-1] * (8 - len(m[2])) for m in ds.metas])
    flat["scale_factor"] = np.asarray(ds.scale_factor)
    flat["interval_scale"] = np.asarray(ds.interval_scale[scan])
    flat["n_images"] = np.asarray(len(ds.image_paths_idr))
    flat["passes"] = np.asarray(passes)
    return flat


@pytest.mark.parametrize("name", ["dtu", "bmvs", "x2"])
def test_dataset_equals_the_reference_fixture(mvsdata, fixture, tmp_path, name):
    md = mvsdata
    md.register_blendedmvs_hash(5, FOLDER)
    ds = mo.build_case(name, str(tmp_path), md.MVSDataset, folder=FOLDER)
    case, want = mo.CASES[name], _case(fixture, name)
    images = not case["x2"]
    assert ds.nviews_max == 5 and isinstance(ds.interval_scale, dict) and ds.decoded_views == 0     # no work in __init__
    for a in ("metas", "image_paths_idr", "intrinsics_idr", "pose_idr", "scale_mat", "scale_factor", "interval_scale",
              "nviews_max", "trains_i", "ndepths", "datapath", "listfile", "mode", "nviews", "data_dir"):
        assert hasattr(ds, a), a
    h, w = case["scan"]["size"]
    got = _flat(ds, ds.listfile[0], images, ds.passes(h, w)[0])
    _compare(got, want, images)
    assert [ds.view_ids(i) for i in range(len(ds))] == [want[f"sample{i}/view_ids"].tolist() for i in range(len(ds))]
    if name == "bmvs":
        assert ds.scale_mat is None and ds.scale_factor == 1.0
        assert float(got["view2/masks"].min()) < 0.5 < float(got["view2/masks"].max())           # a real alpha channel
    if name == "dtu":
        assert ds.scale_mat.shape == (4, 4) and bool((got["view4/masks"] == 1).all())
    if images:
        # the items: the reference's keys, a DataLoader takes them; the device form is the batch of one
        s = ds[1]
        assert list(s) == ["imgs", "masks", "proj_matrices", "depth_values", "cam_near_far", "filename"]
        assert all(isinstance(s[k], np.ndarray) for k in ("imgs", "masks", "depth_values", "cam_near_far"))
        batch = next(iter(torch.utils.data.DataLoader(ds, 1, shuffle=False, num_workers=0)))
        dsamp = ds.device_sample(0)
        assert list(dsamp) == list(batch) and dsamp["filename"] == batch["filename"]
        for k in ("imgs", "masks", "depth_values", "cam_near_far"):
            assert dsamp[k].dtype == batch[k].dtype and torch.equal(dsamp[k], batch[k]), k
        for st in ("stage1", "stage2", "stage3"):
            assert torch.equal(dsamp["proj_matrices"][st], batch["proj_matrices"][st])
        assert dsamp["cam_near_far"].dtype == torch.float64 and tuple(dsamp["imgs"].shape[:3]) == (1, 3, 3)


@pytest.mark.skipif(not HAVE_REFERENCE, reason=f"needs a checkout of the reference at {REFERENCE} (SVOLSDF_REFERENCE_ROOT)")
def test_fixture_is_what_the_live_reference_class_returns(fixture, tmp_path):
    """the same comparison against the live class: the fixture's script, run now, against the committed file (the cameras
    within their tolerance: they go through this machine's LAPACK)"""
    out = str(tmp_path / "live.npz")
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_mvsdata_fixture.py"), "--out", out], check=True, env=env,
                   cwd=str(tmp_path), stdout=subprocess.DEVNULL)
    live = dict(np.load(out))
    _compare(live, fixture, images=True)


def test_size_arithmetic(mvsdata):
    """scale_mvs_input's Python-float expressions give exactly 576x768 and 1152x1536 at the sizes a run meets"""
    md = mvsdata
    for hw in ((1200, 1600), (576, 768), (1152, 1536)):
        h1, w1, sh, sw = md.scaled_size(*hw, 768, 576, base=1)
        assert (h1, w1) == (576, 768) and sh == 576.0 / hw[0] and sw == 768.0 / hw[1]
        assert md.scaled_size(h1, w1, 1536, 1152)[:2] == (1152, 1536)
    assert md.scaled_size(1200, 1600, 768, 576)[:2] == (576, 768)
    assert md.scaled_size(120, 160, 96, 64) == (64, 64, 64.0 / 120, 64.0 / 160)            # 85.33 columns round down
    assert md.scaled_size(100, 160, 96, 64)[:2] == (32, 96)                                # the width sets the scale
    assert md.scaled_size(70, 100, 100, 70) == (64, 96, 64.0 / 70, 96.0 / 100)             # equal sizes still round


def test_x2_assert_and_view_order_cut_to_five(mvsdata, tmp_path):
    md, root = mvsdata, str(tmp_path)
    pairs = {k: [s for s in range(7) if s != k][::-1] for k in range(7)}
    mvs = mo.write_mvs_scan(root, "DTU", 30, 7, (40, 64), pairs)
    ids = [6, 0, 3, 2, 5, 1]
    ds = md.MVSDataset(mvs, ["scan30"], "test", 3, "DTU", 8, 1.06, max_h=32, max_w=64, trains_i=ids,
                       args=dict(data_dir_root=root))                                      # a plain dict will do
    assert ds.view_ids(0) == [6, 5, 3, 2, 1] and ds.view_ids(2) == [3, 6, 5, 2, 1] and len(ds) == 6
    assert ds[0]["imgs"].shape == (5, 3, 32, 32) and ds.sample_meta(0)["proj_matrices"]["stage2"].shape == (5, 2, 4, 4)
    bad = md.MVSDataset(mvs, ["scan30"], "test", 3, "DTU", 8, 1.06, max_h=32, max_w=64, trains_i=ids,
                        args=dict(data_dir_root=root, x2_mvsres=True))
    with pytest.raises(AssertionError):
        bad.sample_meta(0)


def test_every_view_is_decoded_once(mvsdata, monkeypatch, tmp_path):
    md = mvsdata
    calls = []
    monkeypatch.setattr(md, "prepare_views", lambda codes, sizes, png=False: (calls.append(len(codes)),
                                                                               mo.prepare_views(codes, sizes, png))[1])
    ds = mo.build_case("dtu", str(tmp_path), md.MVSDataset)
    first = [ds[i] for i in range(len(ds))]
    for _ in range(3):
        again = [ds[i] for i in range(len(ds))]
        assert all(np.array_equal(a["imgs"], b["imgs"]) for a, b in zip(first, again))
    ds.device_samples()
    assert ds.decoded_views == 3 and sum(calls) == 3
    a, b = ds.view(4), ds.view(4)
    assert a[0].data_ptr() == b[0].data_ptr() and ds.decoded_views == 3
    ds2 = mo.build_case("dtu", str(tmp_path), md.MVSDataset)
    del calls[:]
    ds2.device_samples()
    assert calls == [3] and ds2.decoded_views == 3              # one call for the scan's views


def test_create_scene(mvsdata, tmp_path):
    from helpers.utils import read_camera_parameters
    from PIL import Image
    md, root = mvsdata, str(tmp_path)
    kw = dict(mo.CASES["bmvs"]["scan"])
    md.register_blendedmvs_hash(5, FOLDER)
    mvs = mo.write_mvs_scan(root, folder=FOLDER, **kw)
    trains, evals = [2, 5, 0], [1, 4]
    ds = md.MVSDataset(mvs, ["scan5"], "test", 3, "BlendedMVS", 32, 1.0, max_h=64, max_w=96, trains_i=trains + evals,
                       args=mo.Args(data_dir_root=root, x2_mvsres=False))
    out = str(tmp_path / "ibr")
    assert md.create_scene(out, ds, evals_i=evals) == trains
    assert sorted(os.listdir(os.path.join(out, "scan5", "cams"))) == [f"{i:08d}_cam.txt" for i in sorted(trains + evals)]
    assert sorted(os.listdir(os.path.join(out, "scan5", "images"))) == [f"{i:08d}.png" for i in sorted(trains)]
    assert ds.decoded_views == 3                                 # only the images that are written
    for idx, vid in enumerate(trains + evals):
        meta = ds.sample_meta(idx)
        K, E = read_camera_parameters(os.path.join(out, "scan5", "cams", f"{vid:08d}_cam.txt"))
        cam = meta["proj_matrices"]["stage3"][0]
        assert np.array_equal(K, cam[1, :3, :3]) and np.array_equal(E, cam[0])          # str(float32) round-trips
        last = open(os.path.join(out, "scan5", "cams", f"{vid:08d}_cam.txt")).read().split("\n")[-2]
        assert last == "%.4f %.4f %.4f %.4f" % tuple(meta["cam_near_far"])
    for vid in trains:
        code = np.array(Image.open(os.path.join(ds.image_paths_idr[vid])))
        imgs, _ = mo.prepare_views(code[None], [(32, 96)])
        png = np.array(Image.open(os.path.join(out, "scan5", "images", f"{vid:08d}.png")))
        assert png.dtype == np.uint8 and png.shape == (32, 96, 3)
        assert np.array_equal(png, mo.png_codes(imgs[0].numpy()))
        assert 0 < int((png == 0).all(-1).sum()) < 32 * 96          # rgb * alpha: black where the view is transparent


def test_the_references_asserts(mvsdata, tmp_path):
    md, root = mvsdata, str(tmp_path)
    mvs = mo.write_mvs_scan(root, "DTU", 24, 4, (40, 64), {0: [1, 2], 1: [0, 2], 2: [1, 0], 3: []})
    kw = dict(max_h=32, max_w=64, args=dict(data_dir_root=root))
    ok = md.MVSDataset(mvs, ["scan24"], "test", 3, "DTU", 8, 1.06, trains_i=[2, 0, 1], **kw)
    assert [m[1] for m in ok.metas] == [2, 0, 1] and ok.metas[0] == ("scan24", 2, [1, 0], "scan24")
    with pytest.raises(AssertionError):
        md.MVSDataset(mvs, ["scan24", "scan25"], "test", 3, "DTU", 8, 1.06, trains_i=[2, 0, 1], **kw)
    with pytest.raises(AssertionError):
        md.MVSDataset(mvs, ["scan24"], "train", 3, "DTU", 8, 1.06, trains_i=[2, 0, 1], **kw)
    with pytest.raises(AssertionError):
        md.MVSDataset(mvs, ["scan24"], "test", 3, "BlendedMVS", 8, 1.06, trains_i=[2, 0, 1], **kw)
    with pytest.raises(AssertionError):
        md.MVSDataset(mvs, ["scan24"], "test", 3, "Other", 8, 1, trains_i=[2, 0, 1], **kw)
    with pytest.raises(AssertionError):
        md.MVSDataset(mvs, ["scan24"], "test", 3, "DTU", 8, 1.06, trains_i=None, **kw)
    with pytest.raises(ValueError):                              # view 3 has no sources, view 9 no entry: not in the list
        md.MVSDataset(mvs, ["scan24"], "test", 3, "DTU", 8, 1.06, trains_i=[2, 0, 3], **kw)
    with pytest.raises(ValueError):
        md.MVSDataset(mvs, ["scan24"], "test", 3, "DTU", 8, 1.06, trains_i=[2, 0, 9], **kw)
    with pytest.raises(TypeError):                               # max_h / max_w are required, as the reference's kwargs are
        md.MVSDataset(mvs, ["scan24"], "test", 3, "DTU", 8, 1.06, trains_i=[2, 0, 1], args=dict(data_dir_root=root))


def test_blendedmvs_without_a_folder_name_says_so(mvsdata, monkeypatch, tmp_path):
    md, root = mvsdata, str(tmp_path)
    monkeypatch.setattr("svs_hip.scans._REF_FUNCS", {})
    monkeypatch.delenv("SVS_SCENE_IDS", raising=False)
    kw = dict(mo.CASES["bmvs"]["scan"], scan=8)
    mvs = mo.write_mvs_scan(root, folder=FOLDER, **kw)
    args = (mvs, ["scan8"], "test", 3, "BlendedMVS", 32, 1.0)
    with pytest.raises(LookupError, match="register_blendedmvs_hash"):
        md.MVSDataset(*args, max_h=64, max_w=96, trains_i=[2, 5, 0], args=dict(data_dir_root=root))
    # the JSON route
    table = tmp_path / "ids.json"
    table.write_text('{"BlendedMVS": {"8": {"hash": "%s"}}}' % FOLDER)
    monkeypatch.setenv("SVS_SCENE_IDS", str(table))
    ds = md.MVSDataset(*args, max_h=64, max_w=96, trains_i=[2, 5, 0], args=dict(data_dir_root=root))
    assert md.scan2hash("scan8") == FOLDER and len(ds) == 3 and ds.scale_factor == np.float32(9.7)


@pytest.mark.skipif(not HAVE_REFERENCE, reason=f"needs a checkout of the reference at {REFERENCE} (SVOLSDF_REFERENCE_ROOT)")
def test_folder_names_come_from_a_reference_checkout(mvsdata, monkeypatch):
    md = mvsdata
    monkeypatch.setenv("SVOLSDF_REFERENCE_ROOT", REFERENCE)
    monkeypatch.delenv("SVS_SCENE_IDS", raising=False)
    monkeypatch.setattr("svs_hip.scans._REF_FUNCS", None)
    monkeypatch.setattr("svs_hip.scans._IDS_READ", None)
    md._HASH.clear()
    names = [md.scan2hash(f"scan{i}") for i in range(1, 10)]
    assert len(set(names)) == 9 and all(len(n) == 24 and int(n, 16) >= 0 for n in names)
    with pytest.raises(LookupError):
        md.scan2hash("scan77")


def test_bad_files_raise(mvsdata, tmp_path):
    from PIL import Image
    md, root = mvsdata, str(tmp_path)
    mvs = mo.write_mvs_scan(root, "DTU", 24, 3, (40, 64), {0: [1, 2], 1: [0, 2], 2: [1, 0]})
    Image.fromarray(np.zeros((40, 64), np.uint8)).save(os.path.join(root, "DTU", "scan24", "image", "000001.png"))
    ds = md.MVSDataset(mvs, ["scan24"], "test", 3, "DTU", 8, 1.06, max_h=32, max_w=64, trains_i=[2, 0, 1],
                       args=dict(data_dir_root=root))
    with pytest.raises(ValueError, match="8-bit RGB or RGBA"):
        ds[0]


def test_code_values_are_the_float32_division():
    from svs_hip import mvsdata as md
    codes = np.arange(256, dtype=np.uint8)
    assert md.CODE_VALUES.dtype == np.float32 and np.array_equal(md.CODE_VALUES, mo.code_values(codes))
    assert np.array_equal(md.CODE_VALUES, np.array([np.float32(c) / 255. for c in range(256)], np.float32))
    differ = int((md.CODE_VALUES != codes.astype(np.float32) * np.float32(1.0 / 255.0)).sum())
    print(f"{differ} of 256 codes differ between / 255. and * (1/255)")
    assert 0 < differ < 256                                      # the scene loader's multiply is another function


# ---- the C entry points reject bad arguments before any launch ----
def test_entry_points_check_their_arguments():
    from svs_hip import lib
    L = lib.load()
    d = ctypes.c_void_p(64)                      # never dereferenced
    EINVAL, ESHAPE = -1, -2

    def cubic(src=d, f=0, table=d, V=2, Hs=40, Ws=50, C=3, H=20, W=30, tabs=(d, d, d, d), out=d):
        return L.svs_mvs_resize_cubic(src, f, table, V, Hs, Ws, C, H, W, *tabs, out, None)

    def pack(src=d, f=0, table=d, V=2, Hs=40, Ws=50, C=3, H=20, W=30, tabs=(d, d, d, d), out=d, masks=d):
        return L.svs_mvs_resize_pack(src, f, table, V, Hs, Ws, C, H, W, *tabs, out, masks, None)
    for fn, name in ((cubic, b"svs_mvs_resize_cubic"), (pack, b"svs_mvs_resize_pack")):
        for kw in (dict(src=None), dict(out=None), dict(table=None), dict(tabs=(d, None, d, d)), dict(C=2), dict(C=5),
                   dict(C=1), dict(V=0), dict(V=-1), dict(f=2)):
            assert fn(**kw) == EINVAL, (name, kw)
            assert name in L.svs_last_error_string()
        for kw in (dict(H=0), dict(W=0), dict(Hs=0), dict(Ws=-1), dict(H=70000, W=1), dict(V=70000), dict(H=8192, W=8193)):
            assert fn(**kw) == ESHAPE and name in L.svs_last_error_string(), (name, kw)
    assert pack(masks=None) == EINVAL
    assert L.svs_mvs_codes(None, 4, 4, d, None) == EINVAL and L.svs_mvs_codes(d, 4, 4, None, None) == EINVAL
    assert L.svs_mvs_codes(d, 0, 4, d, None) == ESHAPE and L.svs_mvs_codes(d, 4, -1, d, None) == ESHAPE
    assert b"svs_mvs_codes" in L.svs_last_error_string()
    assert L.svs_version() == 101
