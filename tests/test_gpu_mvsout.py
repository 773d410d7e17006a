"""svs_hip.mvsout on the GPU (csrc/svs_mvsout.hip) against tests/mvsout_oracle.py: the disc dilation and the thresholded
resize of the evaluation masks bit for bit, the final confidence bit for bit against the float32 restatement and within a
derived bound of the float64 one, the argument checks, and the chain outputs -> files -> default-config point cloud."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mvsout_oracle as mo
import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = [(1, 1), (7, 5), (25, 25), (64, 64), (333, 517), (1200, 1600)]
RADII = [0, 1, 12, 32]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _patterns(rng, hw):
    """the masks of one size: random blobs at three densities, empty, full, one pixel in each corner and on each edge"""
    H, W = hw
    out = [mo.blobs(rng, hw, d) for d in (1e-4, 0.01, 0.5)] + [np.zeros(hw, np.uint8), np.full(hw, 255, np.uint8)]
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):
        m = np.zeros(hw, np.uint8)
        m[y, x] = 7
        out.append(m)
    return out


@pytest.mark.parametrize("hw", SIZES)
def test_dilate_disk_is_the_oracle_bit_for_bit(dev, hw):
    from svs_hip import mvsout
    rng = np.random.default_rng(hw[0] * 7 + hw[1])
    pats = _patterns(rng, hw)
    big = hw[0] * hw[1] > 1 << 20
    for r in RADII:
        # V = 1: every pattern on its own (at the full size the three densities only); V = 3: stacks of three
        singles = pats[:3] if big else pats
        for k, m in enumerate(singles):
            got = mvsout.dilate_disk(m, r)
            assert got.dtype == torch.uint8 and tuple(got.shape) == hw and got.is_cuda
            assert np.array_equal(got.cpu().numpy(), mo.dilate(m, r)), (hw, r, k)
        stacks = [pats[:3]] if big else [pats[0:3], pats[3:6], pats[6:9], pats[10:13]]
        for k, st in enumerate(stacks):
            st = np.stack(st)
            got = mvsout.dilate_disk(st, r).cpu().numpy()
            assert got.shape == st.shape and np.array_equal(got, mo.dilate(st, r)), (hw, r, "stack", k)
    if big:
        for m in pats[3:]:                               # empty, full, corners and edges at the evaluation radius
            assert np.array_equal(mvsout.dilate_disk(m, 12).cpu().numpy(), mo.dilate(m, 12))


@pytest.mark.parametrize("src,dst", [((1200, 1600), (1152, 1536)), ((576, 768), (1152, 1536)), ((64, 80), (64, 80)),
                                     ((333, 517), (101, 67)), ((37, 53), (75, 211)), ((1, 9), (5, 3)), ((7, 1), (1, 1))])
def test_resize_any_is_the_oracle_bit_for_bit(dev, src, dst):
    from svs_hip import mvsout
    rng = np.random.default_rng(src[0] + dst[0])
    for V, density in ((1, 0.02), (3, 0.3), (1, 0.0), (1, 1.0)):
        m = np.stack([(rng.random(src) < density).astype(np.uint8) for _ in range(V)])
        got = mvsout.resize_any(m if V > 1 else m[0], *dst).cpu().numpy()
        want = mo.resize_any(m, *dst)
        assert got.dtype == np.uint8 and np.array_equal(got, want if V > 1 else want[0]), (src, dst, V, density)


def test_eval_mask_takes_what_read_img_returns(dev):
    from svs_hip import mvsout
    rng = np.random.default_rng(3)
    codes = mo.blobs(rng, (150, 200), 2e-3)
    want = mo.eval_mask(codes, 72, 96)
    assert 0.05 < want.mean() < 0.95
    rgba = np.concatenate([rng.integers(0, 256, (150, 200, 3)).astype(np.uint8), codes[..., None]], -1)
    for image in (codes, codes.astype(F32) / F32(255.), rgba, rgba.astype(F32) / F32(255.), torch.from_numpy(rgba)):
        got = mvsout.eval_mask(image, 72, 96)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (72, 96) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(mvsout.eval_mask(rgba, 150, 200, radius=3).cpu().numpy(), mo.dilate(codes, 3))


def _maps(rng, sizes):
    maps = [rng.random(s).astype(F32) for s in sizes]
    maps[0].flat[::3] = 0.0
    maps[1].flat[::5] = 1.0
    maps[2].flat[::7] = rng.choice(np.array([0.0, 1.0], F32), maps[2].flat[::7].shape)
    return maps


@pytest.mark.parametrize("sizes,hw", [([(72, 96), (144, 192), (288, 384)], (288, 384)),
                                      ([(288, 384), (576, 768), (1152, 1536)], (1152, 1536)),
                                      ([(31, 45), (50, 77), (101, 67)], (97, 131)),
                                      ([(1, 5), (7, 1), (1, 1)], (9, 11)),
                                      ([(40, 60)] * 3, (40, 60))])
def test_final_confidence_is_the_float32_oracle_bit_for_bit(dev, sizes, hw):
    """Bit for bit against the float32 restatement, and within 14 * 2^-24 = 8.3e-7 of the float64 one.  The bound is
    derived, not measured: inputs and weights lie in [0,1]; a resized map passes two interpolation passes of two
    products and one sum each, at most 6 roundings of at most 2^-24 (half an ulp below 2; the two weights of a tap pair sum
    to 1 within 2^-25); stages 1 and 2 are resized, stage 3 already has the size (H,W) and is taken as it is; the
    product of the three maps, all <= 1, adds 2 roundings: |out - out64| <= (6 + 6 + 2) * 2^-24.  Where all three maps are
    resized the same count gives 20 * 2^-24; the bound asserted stays the cascade's, the stricter one.  The float32
    restatement itself stays below 1.7e-7 on these shapes (tests/test_mvsout_cpu.py asserts the bound for it)."""
    from svs_hip import mvsout
    c = _maps(np.random.default_rng(hw[1]), sizes)
    want = mo.final_confidence(*c, *hw)
    got = mvsout.confidence_product(*c, *hw)
    assert got.dtype == torch.float32 and tuple(got.shape) == hw and got.is_cuda
    got = got.cpu().numpy()
    n_diff = int((got.view(np.int32) != want.view(np.int32)).sum())
    err = float(np.abs(got.astype(np.float64) - mo.final_confidence64(*c, *hw)).max())
    print(f"{sizes} -> {hw}: {n_diff} values differ from the float32 oracle, max |out - float64| {err:.3g}")
    assert n_diff == 0
    assert err <= mo.CONF_BOUND
    # the dict CascadeMVSNet returns, device tensors with a batch axis
    if sizes[2] == hw:
        t = [torch.from_numpy(m)[None].to(dev) for m in c]
        outputs = {"stage1": {"photometric_confidence": t[0]}, "stage2": {"photometric_confidence": t[1]},
                   "stage3": {"photometric_confidence": t[2]}, "photometric_confidence": t[2],
                   "depth": torch.ones(1, *hw, device=dev)}
        assert np.array_equal(mvsout.final_confidence(outputs).cpu().numpy().view(np.int32), want.view(np.int32))


def test_rejected_calls_write_nothing(dev):
    from svs_hip import lib
    L = lib.load()
    EINVAL, ESHAPE = -1, -2
    out = torch.full((3 * 40 * 50,), 0xAB, dtype=torch.uint8, device=dev)
    outf = torch.full((40 * 50,), 123.0, dtype=torch.float32, device=dev)
    mask = torch.ones(3 * 40 * 50, dtype=torch.uint8, device=dev)
    maps = torch.rand(40 * 50, device=dev)
    ws = torch.zeros(int(L.svs_mask_dilate_workspace_bytes(3, 40, 50)) // 8, dtype=torch.int64, device=dev)
    tab_i = torch.zeros(64, dtype=torch.int32, device=dev)
    tab_f = torch.ones(128, dtype=torch.float32, device=dev)
    m, o, of, w, ti, tf, c = (t.data_ptr() for t in (mask, out, outf, ws, tab_i, tab_f, maps))
    assert L.svs_mask_dilate_disk(None, 3, 40, 50, 12, w, o, None) == EINVAL
    assert L.svs_mask_dilate_disk(m, 3, 40, 50, 12, None, o, None) == EINVAL
    assert L.svs_mask_dilate_disk(m, 3, 40, 50, 33, w, o, None) == EINVAL
    assert L.svs_mask_dilate_disk(m, 0, 40, 50, 12, w, o, None) == EINVAL
    assert L.svs_mask_dilate_disk(m, 3, 0, 50, 12, w, o, None) == ESHAPE
    assert L.svs_mask_dilate_disk(m, 3, 40, 0, 12, w, o, None) == ESHAPE
    assert L.svs_mask_resize_any(None, 3, 40, 50, 20, 30, ti, tf, ti, tf, o, None) == EINVAL
    assert L.svs_mask_resize_any(m, 3, 40, 50, 20, 30, ti, None, ti, tf, o, None) == EINVAL
    assert L.svs_mask_resize_any(m, 3, 40, 50, 0, 30, ti, tf, ti, tf, o, None) == ESHAPE
    assert L.svs_mask_resize_any(m, 3, 40, 0, 20, 30, ti, tf, ti, tf, o, None) == ESHAPE
    assert L.svs_mask_resize_any(m, 0, 40, 50, 20, 30, ti, tf, ti, tf, o, None) == EINVAL
    tabs = (ti, tf, ti, tf)
    assert L.svs_mvs_confidence(None, 10, 12, *tabs, c, 20, 25, *tabs, c, 40, 50, *tabs, 40, 50, of, None) == EINVAL
    assert L.svs_mvs_confidence(c, 10, 12, *tabs, c, 20, 25, ti, tf, None, tf, c, 40, 50, *tabs, 40, 50, of, None) == EINVAL
    assert L.svs_mvs_confidence(c, 10, 12, *tabs, c, 0, 25, *tabs, c, 40, 50, *tabs, 40, 50, of, None) == ESHAPE
    assert L.svs_mvs_confidence(c, 10, 12, *tabs, c, 20, 25, *tabs, c, 40, 50, *tabs, 0, 50, of, None) == ESHAPE
    assert b"svs_mvs_confidence" in L.svs_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()) and bool((outf == 123.0).all())
    with pytest.raises(lib.SvsError, match="radius"):
        from svs_hip import mvsout
        mvsout.dilate_disk(np.ones((4, 4), np.uint8), 33)


# ---- end to end ----
def _scene(golden_dir):
    g = np.load(os.path.join(golden_dir, "fusion_geo.npz"))
    hw = tuple(int(v) for v in g["hw"])
    views = synth.make_fusion_views(int(g["seed"]), hw=hw, n_views=3)
    ids = [0, 1, 2]
    return views, ids, [(v, [s for s in ids if s != v]) for v in ids], hw


def _mask_images(hw):
    """evaluation-mask images larger than the depth maps, each cutting away a different part of its view: a disc, the
    left part, an RGBA image whose alpha channel holds an ellipse"""
    Hs, Ws = 3 * hw[0] + 6, 3 * hw[1] + 8
    y, x = np.mgrid[0:Hs, 0:Ws]
    a = (((y - Hs / 2) ** 2 + (x - Ws / 2) ** 2) <= (0.3 * Hs) ** 2).astype(np.uint8) * 255
    b = (x < 0.55 * Ws).astype(np.uint8) * 255
    c = ((((y - 0.4 * Hs) / (0.35 * Hs)) ** 2 + ((x - 0.6 * Ws) / (0.3 * Ws)) ** 2) <= 1).astype(np.uint8) * 200
    rgba = np.concatenate([np.full((Hs, Ws, 3), 255, np.uint8), c[..., None]], -1)
    return {0: np.repeat(a[..., None], 3, -1), 1: b, 2: rgba}


def _final_masks(mask_dir, ids):
    from PIL import Image
    return {v: np.array(Image.open(os.path.join(mask_dir, "{:0>8}_final.png".format(v)))) > 0 for v in ids}


def test_filter_depth_with_evaluation_masks_in_memory(dev, golden_dir, tmp_path):
    from svs_hip import fusion, mvsout
    views, ids, pairs, hw = _scene(golden_dir)
    images = _mask_images(hw)
    gpu_masks = {v: mvsout.eval_mask(images[v].astype(F32) / F32(255.), *hw) for v in ids}
    orc_masks = {v: mo.eval_mask(images[v], *hw) for v in ids}
    for v in ids:
        assert np.array_equal(gpu_masks[v].cpu().numpy(), orc_masks[v]) and 0.1 < orc_masks[v].mean() < 0.9
    kw = dict(conf=0.2, thres_view=1)
    xyz, rgb, stats = fusion.filter_depth(views, pairs, eval_masks=gpu_masks, mask_dir=str(tmp_path / "gpu"), **kw)
    xyz_o, rgb_o, stats_o = fusion.filter_depth(views, pairs, eval_masks=orc_masks, mask_dir=str(tmp_path / "orc"), **kw)
    xyz_n, rgb_n, stats_n = fusion.filter_depth(views, pairs, eval_masks=None, mask_dir=str(tmp_path / "none"), **kw)
    fm, fm_o, fm_n = (_final_masks(str(tmp_path / d), ids) for d in ("gpu", "orc", "none"))
    assert np.array_equal(xyz, xyz_o) and np.array_equal(rgb, rgb_o) and stats == stats_o
    rows, base = [], 0
    for v in ids:
        assert np.array_equal(fm[v], fm_o[v])
        assert np.array_equal(fm[v], fm_n[v] & (orc_masks[v] > 0))          # the mask is applied, and nothing else changes
        assert fm[v].sum() < fm_n[v].sum()                                   # every view loses points
        rows.append(base + (np.cumsum(fm_n[v].reshape(-1)) - 1)[fm[v].reshape(-1)])
        base += int(fm_n[v].sum())
    rows = np.concatenate(rows)
    assert 100 < len(xyz) < len(xyz_n) == base
    # a strict subset of the unmasked cloud, in its order
    assert np.array_equal(xyz, xyz_n[rows]) and np.array_equal(rgb, rgb_n[rows])
    # and the numpy restatement of the whole filter fed with the oracle's masks keeps as many points (within the few
    # pixels whose float64 geometry sits at a threshold: tests/test_gpu_fusion.py)
    want = mo.filter_depth(views, pairs, eval_masks=orc_masks, **kw)
    assert abs(sum(len(w["xyz"]) for w in want) - len(xyz)) <= 3


def test_save_view_then_filter_depth_folder(dev, golden_dir, tmp_path):
    from datasets.data_io import read_pfm
    from helpers.utils import read_camera_parameters, read_img
    from PIL import Image
    from svs_hip import fusion, mvsout
    from svs_hip.ply import read_points
    views, ids, pairs, hw = _scene(golden_dir)
    H, W = hw
    rng = np.random.default_rng(8)
    root, out = tmp_path / "data", tmp_path / "exps" / "scan24"
    images = _mask_images(hw)
    (root / "DTU" / "eval_mask" / "scan24" / "mask").mkdir(parents=True)
    conf = {}
    for v in ids:
        Image.fromarray(images[v]).save(str(root / "DTU" / "eval_mask" / "scan24" / "mask" / "{:0>3}.png".format(v)))
        c = [np.sqrt(rng.random(s)).astype(F32) for s in ((H // 4, W // 4), (H // 2, W // 2), (H, W))]
        outputs = {"depth": torch.from_numpy(views[v]["depth"])[None].to(dev),
                   "photometric_confidence": torch.from_numpy(c[2])[None].to(dev),
                   "stage1": {"photometric_confidence": torch.from_numpy(c[0])[None].to(dev)},
                   "stage2": {"photometric_confidence": c[1][None]}}
        cam = np.zeros((2, 4, 4), F32)
        cam[0] = views[v]["E"]
        cam[1, :3, :3] = views[v]["K"]
        cam[1, 3] = [425.0, 2.5, 192.0, 905.0]
        names = mvsout.save_view(str(out), v, outputs, cam, np.transpose(views[v]["img"], (2, 0, 1)))
        conf[v] = mvsout.final_confidence(outputs).cpu().numpy()
        assert np.array_equal(conf[v].view(np.int32), mo.final_confidence(*c, H, W).view(np.int32))
        assert np.array_equal(np.asarray(read_pfm(names["confidence"])[0]).view(np.int32), conf[v].view(np.int32))
        assert np.array_equal(np.asarray(read_pfm(names["depth_est"])[0]).view(np.int32), views[v]["depth"].view(np.int32))
        K, E = read_camera_parameters(names["cams"])
        assert np.array_equal(K, views[v]["K"]) and np.array_equal(E, views[v]["E"])
        jpg = read_img(names["images"])
        assert jpg.shape == (H, W, 3) and os.path.basename(names["images"]) == "{:0>8}.jpg".format(v)
    kw = dict(conf=0.2, thres_view=1)
    ply = str(tmp_path / "scan24.ply")
    xyz, rgb, stats = fusion.filter_depth_folder(str(out), str(out), ply, ids, eval_mask_root=str(root), dataset="DTU", **kw)
    mem = {v: dict(views[v], confidence=conf[v], img=read_img(str(out / "images" / "{:0>8}.jpg".format(v)))) for v in ids}
    masks = {v: mvsout.eval_mask(read_img(mvsout.eval_mask_path(str(root), "DTU", "scan24", v)), H, W) for v in ids}
    xyz_m, rgb_m, stats_m = fusion.filter_depth(mem, pairs, eval_masks=masks, **kw)
    pts, col = read_points(ply)
    assert len(pts) == len(xyz) == len(xyz_m) > 100
    assert np.array_equal(xyz, xyz_m) and np.array_equal(rgb, rgb_m) and np.array_equal(col, rgb)
    # without the new keywords, and with eval_mask_root=None: today's result
    ply0, ply1 = str(tmp_path / "plain.ply"), str(tmp_path / "none.ply")
    xyz0, rgb0, stats0 = fusion.filter_depth_folder(str(out), str(out), ply0, ids, **kw)
    xyz1, rgb1, stats1 = fusion.filter_depth_folder(str(out), str(out), ply1, ids, eval_mask_root=None, **kw)
    xyz2, rgb2, _ = fusion.filter_depth(mem, pairs, **kw)
    assert np.array_equal(xyz0, xyz1) and np.array_equal(rgb0, rgb1) and stats0 == stats1
    assert open(ply0, "rb").read() == open(ply1, "rb").read()
    assert np.array_equal(xyz0, xyz2) and np.array_equal(rgb0, rgb2)
    assert len(xyz) < len(xyz0)
    # the command line: the same cloud
    ply2 = str(tmp_path / "cli.ply")
    mvsout.main(["--scan-folder", str(out), "--out-folder", str(out), "--ply", ply2, "--views", "0", "1", "2",
                 "--data-dir-root", str(root), "--dataset", "DTU", "--conf", "0.2"])
    assert open(ply2, "rb").read() == open(ply, "rb").read()
