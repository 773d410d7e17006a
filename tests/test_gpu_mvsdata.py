"""GPU parity of the MVS loader (csrc/svs_mvsdata.hip, svs_hip/mvsdata.py) against the float64 chain of
tests/mvsdata_oracle.py (read_img's float32 code / 255., tests/scene_oracle.py::resize_cubic once or twice with the
float32 source coordinate of the parity definition, then the alpha product).  Synthetic arrays and folders only.

Bounds (derived, not measured; `_bounds`):
  e        1e-5 absolute: the bound tests/test_gpu_scene.py derives for one cubic pass over values in about [-0.2, 1.2]
           ((gamma_4 + 2u) 1.375^2 1.2 ~ 1e-6 for both directions, a factor of ten left for the float32 rounding of the
           coefficients).  The value of a code adds nothing: it is the same float32 on both sides.
  resize   one pass: e.  Two passes (x2_mvsres): the second pass reads the first one's result, whose error it amplifies by
           at most the 2-D absolute weight sum of Keys' kernel, 1.375^2 = 1.890625, and adds its own e:
           e2 = 1.890625 e + e = 2.890625e-5.  This bounds `masks` (the resized alpha) and `imgs` of an RGB view.
  product  RGBA: imgs = rgb * alpha after the resize.  |r' a' - r a| <= |r' - r| |a| + |a' - a| |r'| <= e_n (|rgb| + |alpha|)
           with the maxima of |rgb| and |alpha| taken from the oracle's own resized values (Keys' kernel overshoots [0,1]).
  exact    equal sizes (a copy of the table's values and one float32 product) and svs_mvs_codes (a float32 multiply, a
           clip, a truncation) are compared bit for bit.
Observed maxima are printed by each test (pytest -s) and recorded in INTEGRATION.md."""
import os

import numpy as np
import pytest
import torch

import mvsdata_oracle as mo
import scene_oracle as so

pytestmark = pytest.mark.gpu
E_PASS = 1e-5                                   # tests/test_gpu_scene.py::RGB_TOL
KEYS_ABS_SUM_2D = 1.375 ** 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def mvsdata(dev):
    from svs_hip import mvsdata as md
    saved = dict(md._HASH)
    yield md
    md._HASH.clear()
    md._HASH.update(saved)


def _bounds(n_passes, want_resized):
    """-> the bound of the resized values after n passes, and of imgs (the product for an RGBA view)"""
    e_n = E_PASS
    for _ in range(n_passes - 1):
        e_n = KEYS_ABS_SUM_2D * e_n + E_PASS
    if want_resized.shape[-1] == 4:
        return e_n, e_n * (float(np.abs(want_resized[..., :3]).max()) + float(np.abs(want_resized[..., 3]).max()))
    return e_n, e_n


@pytest.mark.parametrize("C", [3, 4])
def test_equal_sizes_are_the_code_values_bit_for_bit(mvsdata, C):
    codes = np.stack([mo.all_codes(32, 64, C, 10 * C + v) for v in range(2)])
    assert all(set(np.unique(codes[..., c])) == set(range(256)) for c in range(C))
    imgs, masks = mvsdata.prepare_views(codes, [(32, 64)])
    assert imgs.is_cuda and imgs.dtype == masks.dtype == torch.float32
    assert tuple(imgs.shape) == (2, 3, 32, 64) and tuple(masks.shape) == (2, 1, 32, 64)
    val = np.float32(codes) / 255.
    assert val.dtype == np.float32
    rgb = val[..., :3].transpose(0, 3, 1, 2)
    if C == 4:
        alpha = val[..., 3:].transpose(0, 3, 1, 2)
        assert np.array_equal(masks.cpu().numpy(), alpha) and np.array_equal(imgs.cpu().numpy(), rgb * alpha)
    else:
        assert np.array_equal(imgs.cpu().numpy(), rgb) and bool((masks == 1).all())
    # the same through two equal-size passes (the chain's float32 source path) and through the channel-last entry point
    again = mvsdata.prepare_views(torch.from_numpy(codes).to("cuda:0"), [(32, 64), (32, 64)])
    assert torch.equal(again[0], imgs) and torch.equal(again[1], masks)


def test_codes_are_numpys(mvsdata, dev):
    from svs_hip import lib
    from svs_hip.ops import _ptr, _stream
    L = lib.load()
    k = np.arange(256, dtype=np.float32) / 255.
    edge = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
                           (np.arange(256, dtype=np.float32) + np.float32(0.99)) / 255.])
    rng = np.random.default_rng(5)
    vals = np.concatenate([edge, rng.uniform(-0.5, 1.5, 3 * 40 * 64 - edge.size - 8).astype(np.float32),
                           np.array([-0.0, 0.0, 1.0, -1e-30, 1e30, -1e30, np.inf, -np.inf], np.float32)])
    img = rng.permutation(vals).reshape(3, 40, 64).astype(np.float32)
    want = np.clip(np.transpose(img, (1, 2, 0)) * 255, 0, 255).astype(np.uint8)
    d = torch.from_numpy(img).to(dev)
    out = torch.full((40, 64, 3), 77, dtype=torch.uint8, device=dev)
    assert L.svs_mvs_codes(_ptr(d), 40, 64, _ptr(out), _stream()) == 0
    assert np.array_equal(out.cpu().numpy(), want)
    assert set(np.unique(want)) == set(range(256))
    # through the seam: the PNG codes of a resized RGBA view are numpy's of the device's own imgs
    codes = mo.rgba_image(50, 70, 3)[None]
    imgs, masks, png = mvsdata.prepare_views(codes, [(32, 64)], png=True)
    assert png.dtype == torch.uint8 and tuple(png.shape) == (1, 32, 64, 3)
    assert np.array_equal(png[0].cpu().numpy(), mo.png_codes(imgs[0].cpu().numpy()))


def _view(H, W, C, seed):
    return mo.rgba_image(H, W, seed) if C == 4 else so.synthetic_image(H, W, seed)


@pytest.mark.parametrize("src,C,sizes,V", [
    ((1200, 1600), 3, [(576, 768), (1152, 1536)], 1),            # a DTU view through the x2_mvsres chain
    ((100, 160), 4, [(32, 96)], 3),                              # a small RGBA view, one pass
    ((150, 200), 4, [(72, 96), (144, 192)], 2),                  # RGBA through two passes
    ((72, 96), 3, [(144, 192)], 2),                              # an upscale
    ((72, 96), 4, [(160, 224)], 1),
    ((33, 47), 4, [(67, 259)], 1),                               # a non-rational ratio, both directions
    ((100, 130), 3, [(64, 96)], 2),
    ((576, 768), 3, [(576, 768), (1152, 1536)], 1),              # the first pass of the chain is a copy
])
def test_resized_views(mvsdata, src, C, sizes, V):
    codes = np.stack([_view(src[0], src[1], C, 40 + v) for v in range(V)])
    imgs, masks = mvsdata.prepare_views(codes, sizes)
    H, W = sizes[-1]
    assert imgs.is_cuda and tuple(imgs.shape) == (V, 3, H, W) and tuple(masks.shape) == (V, 1, H, W)
    want_imgs, want_masks, want_resized = mo.views64(codes, sizes)
    before = [tuple(src)] + [tuple(s) for s in sizes[:-1]]
    n_passes = sum(tuple(s) != b for s, b in zip(sizes, before))              # a pass to the same size is a copy
    tol_resized, tol_imgs = _bounds(max(1, n_passes), want_resized)
    e_imgs = float(np.abs(imgs.cpu().numpy() - want_imgs).max())
    e_masks = float(np.abs(masks.cpu().numpy() - want_masks).max())
    print(f"{src} C={C} -> {sizes}: max |imgs - oracle| {e_imgs:.3g} (bound {tol_imgs:.3g}), "
          f"max |masks - oracle| {e_masks:.3g} (bound {tol_resized:.3g}), oracle range "
          f"[{want_resized.min():.3f}, {want_resized.max():.3f}]")
    assert e_imgs <= tol_imgs and e_masks <= tol_resized
    if C == 3:
        assert bool((masks == 1).all())
    # the channel-last entry point alone gives the planes' values before the product
    from svs_hip import lib
    from svs_hip.ops import _ptr, _stream
    from svs_hip.images import cubic_table, tables_device
    if len(sizes) == 1 and tuple(src) != tuple(sizes[0]):
        L = lib.load()
        d = torch.from_numpy(codes).to("cuda:0")
        out = torch.empty(V, H, W, C, dtype=torch.float32, device="cuda:0")
        tabs = tables_device(cubic_table, H, W, src[0], src[1], d.device)
        table = torch.from_numpy(mvsdata.CODE_VALUES).to("cuda:0")
        assert L.svs_mvs_resize_cubic(_ptr(d), 0, _ptr(table), V, src[0], src[1], C, H, W, *[_ptr(t) for t in tabs],
                                      _ptr(out), _stream()) == 0
        planes = out.permute(0, 3, 1, 2)
        if C == 4:
            assert torch.equal(planes[:, 3:], masks) and torch.equal(planes[:, :3] * planes[:, 3:], imgs)
        else:
            assert torch.equal(planes, imgs)


def test_rejected_calls_write_nothing(mvsdata, dev):
    from svs_hip import lib
    from svs_hip.ops import _ptr, _stream
    from svs_hip.images import cubic_table, tables_device
    L = lib.load()
    EINVAL, ESHAPE = -1, -2
    codes = torch.from_numpy(mo.rgba_image(40, 50, 1)[None]).to(dev)
    table = torch.from_numpy(mvsdata.CODE_VALUES).to(dev)
    tabs = [_ptr(t) for t in tables_device(cubic_table, 20, 30, 40, 50, dev)]
    out = torch.full((1, 20, 30, 4), 7.0, device=dev)
    imgs, masks = torch.full((1, 3, 20, 30), 7.0, device=dev), torch.full((1, 1, 20, 30), 7.0, device=dev)
    png = torch.full((20, 30, 3), 7, dtype=torch.uint8, device=dev)

    def cubic(src=_ptr(codes), table=_ptr(table), C=4, H=20, tabs=tabs, out=_ptr(out)):
        return L.svs_mvs_resize_cubic(src, 0, table, 1, 40, 50, C, H, 30, *tabs, out, _stream())

    def pack(src=_ptr(codes), table=_ptr(table), C=4, H=20, tabs=tabs, imgs=_ptr(imgs), masks=_ptr(masks)):
        return L.svs_mvs_resize_pack(src, 0, table, 1, 40, 50, C, H, 30, *tabs, imgs, masks, _stream())
    for fn in (cubic, pack):
        assert fn(src=None) == EINVAL and fn(table=None) == EINVAL and fn(tabs=[None] + tabs[1:]) == EINVAL
        assert fn(C=2) == EINVAL and fn(H=0) == ESHAPE
    assert cubic(out=None) == EINVAL and pack(imgs=None) == EINVAL and pack(masks=None) == EINVAL
    assert L.svs_mvs_codes(None, 20, 30, _ptr(png), _stream()) == EINVAL
    assert L.svs_mvs_codes(_ptr(imgs), 0, 30, _ptr(png), _stream()) == ESHAPE
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (out, imgs, masks, png))
    assert cubic() == 0 and pack() == 0 and L.svs_mvs_codes(_ptr(imgs), 20, 30, _ptr(png), _stream()) == 0
    torch.cuda.synchronize()
    assert not any(bool((t == 7).any()) for t in (out, imgs, masks))
    with pytest.raises(TypeError):
        mvsdata.prepare_views(np.zeros((1, 20, 30, 3), np.float32), [(16, 16)])
    with pytest.raises(ValueError):
        mvsdata.prepare_views(np.zeros((1, 20, 30, 2), np.uint8), [(16, 16)])
    with pytest.raises(ValueError):
        mvsdata.prepare_views(np.zeros((1, 20, 30, 3), np.uint8), [(0, 16)])
    with pytest.raises(lib.SvsError):
        mvsdata.prepare_views(np.zeros((1, 20, 30, 3), np.uint8), [(70000, 16)])


def _write_three_view_scan(root, size):
    """a DTU-layout folder of three views whose cameras are those of synth.make_mvs_sample: small rotations, baselines of
    30 units, the scene at the DTU depth range -- so that the warped features land inside the images"""
    import synth
    inst = so.write_scan(root, "DTU", 24, 3, size, seed=2)
    _, proj, _ = synth.make_mvs_sample(11, img_hw=(size[0] // 2, size[1] // 2), n_views=3, numdepth=16)
    cams = {}
    for v in range(3):
        K = proj["stage3"][v, 1].astype(np.float64).copy()
        K[:2, :3] *= 2.0                                        # the files are twice the size the dataset scales them to
        cams[f"world_mat_{v}"] = K @ proj["stage3"][v, 0].astype(np.float64)
        cams[f"scale_mat_{v}"] = np.diag([90.0, 90.0, 90.0, 1.0])
    np.savez(os.path.join(inst, "cameras.npz"), **cams)
    mvs = os.path.join(root, "DTU", "mvs_data")
    os.makedirs(os.path.join(mvs, "scan24"))
    open(os.path.join(mvs, "scan24", "pair.txt"), "w").write(mo.pair_text({0: [1, 2], 1: [0, 2], 2: [1, 0]}))
    return mvs


def _leaves(x, path=""):
    if torch.is_tensor(x):
        yield path, x
    elif isinstance(x, dict):
        for k, v in x.items():
            yield from _leaves(v, f"{path}/{k}")
    elif isinstance(x, (list, tuple)):
        for k, v in enumerate(x):
            yield from _leaves(v, f"{path}/{k}")


def _to_device(x, dev):
    """helpers/utils.py::tocuda"""
    if torch.is_tensor(x):
        return x.to(dev)
    if isinstance(x, dict):
        return {k: _to_device(v, dev) for k, v in x.items()}
    if isinstance(x, list):
        return [_to_device(v, dev) for v in x]
    return x


def test_device_samples_feed_the_cost_volume(mvsdata, dev, tmp_path):
    import synth
    from models.CasMVSNet import CascadeMVSNet
    from svs_hip.stage_loop import StageLoop
    md, root = mvsdata, str(tmp_path)
    H, W = 64, 96
    mvs = _write_three_view_scan(root, (2 * H, 2 * W))
    ds = md.MVSDataset(mvs, ["scan24"], "test", 3, "DTU", 16, 1.06, max_h=H, max_w=W, trains_i=[1, 0, 2],
                       args=dict(data_dir_root=root, x2_mvsres=False))
    samples = ds.device_samples()
    assert ds.decoded_views == 3 and md.LAUNCHES["pack"] >= 1
    for i, s in enumerate(samples):
        assert s["imgs"].is_cuda and tuple(s["imgs"].shape) == (1, 3, 3, H, W) and tuple(s["masks"].shape) == (1, 3, 1, H, W)
        assert tuple(s["proj_matrices"]["stage1"].shape) == (1, 3, 2, 4, 4) and s["proj_matrices"]["stage1"].is_cuda
        assert tuple(s["depth_values"].shape) == (1, 16) and s["cam_near_far"].dtype == torch.float64
        assert s["filename"] == ["scan24/{}/%08d{}" % ds.view_ids(i)[0]]
    # the images are the oracle's, within one pass's bound
    code = so.read_image(ds.image_paths_idr[0])
    want, _, _ = mo.views64(code[None], [(H, W)])
    err = float(np.abs(ds.view(0)[0].cpu().numpy() - want[0]).max())
    print(f"dataset view 0: max |imgs - oracle| {err:.3g}")
    assert err <= E_PASS

    torch.manual_seed(0)
    model = CascadeMVSNet(refine=False, ndepths=[16, 8, 8], depth_interals_ratio=[4.0, 2.0, 1.0], share_cr=False,
                          cr_base_chs=[8, 8, 8], grad_method="detach")
    model.feature.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_featurenet_params(3).items()})
    for st, cin in enumerate((32, 16, 8)):
        model.cost_regularization[st].load_state_dict(
            {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_costreg_params(50 + st, cin).items()})
    model.to(dev).eval()
    loop = StageLoop(model)
    outs, extras = loop.cost_volumes(0, samples, [None] * 3)
    assert loop.feature_calls == 3
    for o in outs:
        assert set(o) >= {"stage1", "depth", "photometric_confidence", "prob_volume", "depth_values"}
        assert tuple(o["depth"].shape) == (1, H // 4, W // 4) and tuple(o["photometric_confidence"].shape) == (1, H // 4, W // 4)
        assert tuple(o["prob_volume"].shape) == (1, 16, H // 4, W // 4)
        assert all(bool(torch.isfinite(t).all()) for _, t in _leaves(o))
        assert 425.0 <= float(o["depth"].min()) and float(o["depth"].max()) <= 425.0 + 2.65 * 16
    # the reference's route: numpy items through a DataLoader, then to the device
    loader = torch.utils.data.DataLoader(ds, 1, shuffle=False, num_workers=0, drop_last=False)
    host_samples = [_to_device(b, dev) for b in loader]
    assert ds.decoded_views == 3
    for a, b in zip(samples, host_samples):
        la, lb = dict(_leaves(a)), dict(_leaves(b))
        assert list(la) == list(lb) and a["filename"] == b["filename"]
        assert all(la[k].dtype == lb[k].dtype and torch.equal(la[k], lb[k]) for k in la)
    loop2 = StageLoop(model)
    outs2, _ = loop2.cost_volumes(0, host_samples, [None] * 3)
    assert loop2.feature_calls == 3
    for a, b in zip(outs, outs2):
        la, lb = dict(_leaves(a)), dict(_leaves(b))
        assert list(la) == list(lb) and all(torch.equal(la[k], lb[k]) for k in la)


def test_create_scene_and_the_command_line(mvsdata, tmp_path, capsys):
    from PIL import Image
    md, root = mvsdata, str(tmp_path)
    md.register_blendedmvs_hash(5, "0123456789abcdef01234567")
    kw = dict(mo.CASES["bmvs"]["scan"])
    mvs = mo.write_mvs_scan(root, folder="0123456789abcdef01234567", **kw)
    trains, evals = [2, 5, 0], [1, 4]
    ds = md.MVSDataset(mvs, ["scan5"], "test", 3, "BlendedMVS", 32, 1.0, max_h=64, max_w=96, trains_i=trains + evals,
                       args=dict(data_dir_root=root))
    out = str(tmp_path / "ibr")
    assert md.create_scene(out, ds, evals_i=evals) == trains and ds.decoded_views == 3
    assert len(os.listdir(os.path.join(out, "scan5", "cams"))) == 5
    for vid in trains:
        png = np.array(Image.open(os.path.join(out, "scan5", "images", f"{vid:08d}.png")))
        assert np.array_equal(png, mo.png_codes(ds.view(vid)[0].cpu().numpy()))
        code = so.read_image(ds.image_paths_idr[vid])
        want = mo.png_codes(mo.prepare_views(code[None], [(32, 96)])[0][0].numpy())
        off = np.abs(png.astype(int) - want.astype(int))
        # against the float32 oracle a code may flip by one where value * 255 lies within the resize bound of an integer:
        # 2 * 255 * e ~ 0.5 % of uniformly spread values
        assert int(off.max()) <= 1 and float((off > 0).mean()) <= 2 * 255 * E_PASS
    # the command line on a DTU folder (the DTU id lists are the project's own)
    root2 = str(tmp_path / "dtu")
    n = 49
    mo.write_mvs_scan(root2, "DTU", 106, n, (60, 80), {k: [s for s in (25, 22, 28, 0, 1) if s != k] for k in range(n)})
    md.main(["--data-dir-root", root2, "--dataset", "DTU", "--scan", "106", "--max-h", "32", "--max-w", "64", "--no-x2",
             "--create-scene", str(tmp_path / "ibr2")])
    text = capsys.readouterr().out
    assert "3 samples, 3 views decoded" in text and "60x80 -> 32x32" in text and "kernels" in text
    assert sorted(os.listdir(str(tmp_path / "ibr2" / "scan106" / "images"))) == [f"{i:08d}.png" for i in (22, 25, 28)]
    assert len(os.listdir(str(tmp_path / "ibr2" / "scan106" / "cams"))) == 3 + len(md._scene.get_eval_ids("DTU"))
