"""GPU parity of image-based rendering (simple_ibr.py:116-235, csrc/svs_ibr.hip) through the C-ABI and svs_hip.ibr,
against the reference-generated fixture ibr_blend.npz and the numpy oracle (which reproduces the fixture bit for bit:
tests/test_ibr_cpu.py).  The kernels run in float32 where the reference's pyramids are float64: 1e-5 absolute.

Where a weight sits within 1e-6 of the 0.2 threshold, `w > 0.2` may legitimately flip between float32 evaluation orders;
that changes the eroded masks in the pixel's 5x5 neighbourhood, and the blend within the pyramid's reach of those
pixels.  REACH bounds that reach: four levels of 5x5 pyrDown (2 + 4 + 8 = 14 level-0 pixels down to level 3) and the
pyrUps back (8 + 4 + 2 = 14), plus the erosion's 2, rounded up."""
import os

import numpy as np
import pytest
import torch

import ibr_oracle as io_
import synth
from ibr_cases import REACH, TOL, dilate, near_threshold, run_blend, run_weights
from make_ibr_fixture import digest

pytestmark = pytest.mark.gpu
SVS_EINVAL, SVS_ESHAPE = -1, -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ibr_blend.npz")))


@pytest.fixture(scope="module")
def views(golden, tmp_path_factory):
    """{eval id: (ref, srcs, pred, oracle result)}, the oracle checked against the fixture's digests."""
    scan, out, v = io_.fixture_views(golden, tmp_path_factory.mktemp("ibr"))
    res = {}
    for vid, (ref, srcs, pred) in v.items():
        o = io_.blend_view(ref, srcs, pred)
        assert digest(o["fill"]) == str(golden[f"sha_fill_{vid}"]) and digest(o["masks"]) == str(golden[f"sha_masks_{vid}"])
        assert digest(o["blend"]) == str(golden[f"sha_blend_{vid}"])
        res[vid] = (ref, srcs, pred, o)
    return scan, out, res


def test_blend_stage_matches_reference(dev, views):
    """svs_ibr_laplacian_blend on the arrays the reference handed to Laplacian_Blending == its float64 result."""
    from svs_hip import lib
    L = lib.load()
    for vid, (_, _, _, o) in views[2].items():
        got = run_blend(L, o["fill"], o["masks"][..., 0], dev)
        err = np.abs(got - o["blend"])
        assert err.max() <= TOL, (vid, float(err.max()))


def test_weights_stage_matches_reference(dev, views):
    """svs_ibr_weights from the fixture's geometric masks and maps: fill images and masks within 1e-5, masks excepted only
    in the 5x5 neighbourhood of weights within 1e-6 of the 0.2 threshold."""
    from svs_hip import lib
    L = lib.load()
    for vid, (ref, srcs, pred, o) in views[2].items():
        fill, masks = run_weights(L, [s["img"] for s in srcs], o["src_dirs"], o["ref_dir"], pred, o["geo"], o["x2d"],
                                  o["y2d"], dev)
        assert np.abs(fill - o["fill"]).max() <= TOL, vid
        tie = dilate(near_threshold(o["weights"]), 2)
        assert tie.sum() <= 25 * 8, int(tie.sum())
        err = np.abs(masks - o["masks"][..., 0])[:, ~tie]
        assert err.max() <= TOL, (vid, float(err.max()))
        assert (masks[:-1] > 0).any()


def _compare_blend(got, want_f64, bad):
    """got (H,W,3) float32 vs the float64 reference outside `bad` (pixels within the reach of a legitimate flip);
    PNG pixels: exact except where the reference value x 255 is within 1e-3 of an integer (then off by at most 1)."""
    keep = ~dilate(bad, REACH)
    assert keep.mean() > 0.9, float(keep.mean())
    err = np.abs(got - want_f64)[keep]
    assert err.max() <= TOL, float(err.max())
    png, ref_png = (got.astype(np.float64) * 255).astype(np.uint8), (want_f64 * 255).astype(np.uint8)
    v = want_f64 * 255
    edge = np.abs(v - np.rint(v)) < 1e-3
    diff = png.astype(int) - ref_png.astype(int)
    assert np.all(diff[keep & ~edge.any(-1)] == 0)
    assert np.abs(diff[keep]).max() <= 1


def test_blend_view_end_to_end(dev, views):
    """svs_hip.ibr.blend_view on the fixture's views: geometric masks equal the reference's, blend within 1e-5."""
    from svs_hip import ibr
    for vid, (ref, srcs, pred, o) in views[2].items():
        out, st = ibr.blend_view(ref, srcs, pred, return_stages=True)
        geo = st["src_mask"].cpu().numpy().astype(bool)
        diff = (geo != o["geo"]).any(0)
        assert diff.mean() <= 2e-3, int(diff.sum())
        _compare_blend(out.cpu().numpy(), o["blend"], dilate(diff, 2) | dilate(near_threshold(o["weights"]), 2))


def test_image_based_render_files(dev, views, golden):
    """The file-level entry writes eval_blend_XXX.png whose pixels match the reference's PNG (off by one only where the
    reference's value x 255 sits within 1e-3 of an integer)."""
    from PIL import Image
    from svs_hip import ibr
    scan, out, res = views
    written = ibr.image_based_render(scan, out, [int(v) for v in golden["eval_ids"]], [int(v) for v in golden["src_ids"]])
    assert len(written) == len(res)
    for vid, (_, _, _, o) in res.items():
        got = np.array(Image.open(os.path.join(out, "eval_blend_{:0>3}.png".format(vid))))
        want = golden[f"png_{vid}"]
        assert got.shape == want.shape and got.dtype == np.uint8
        v = o["blend"] * 255
        edge = (np.abs(v - np.rint(v)) < 1e-3)
        d = got.astype(int) - want.astype(int)
        bad = dilate(near_threshold(o["weights"]), 2)
        keep = ~dilate(bad, REACH)[..., None].repeat(3, -1)
        assert np.all(d[keep & ~edge] == 0), int((d[keep & ~edge] != 0).sum())
        assert np.abs(d[keep]).max() <= 1


def test_full_size_vs_oracle(dev):
    """576x768 with three sources (the DTU / BlendedMVS evaluation size)."""
    from svs_hip import ibr
    v = synth.make_fusion_views(52, hw=(576, 768), n_views=4)
    ref, srcs, pred = v[1], [v[0], v[2], v[3]], v[1]["img"]
    o = io_.blend_view(ref, srcs, pred)
    out, st = ibr.blend_view(ref, srcs, pred, return_stages=True)
    geo = st["src_mask"].cpu().numpy().astype(bool)
    diff = (geo != o["geo"]).any(0)
    assert diff.mean() <= 2e-3, int(diff.sum())
    tie = near_threshold(o["weights"])
    assert tie.sum() <= 64, int(tie.sum())
    bad = dilate(diff, 2) | dilate(tie, 2)
    fill = st["fill"].cpu().numpy()
    keep = ~bad
    assert np.abs(fill - o["fill"])[:, keep].max() <= TOL
    assert np.abs(st["masks"].cpu().numpy() - o["masks"][..., 0])[:, keep].max() <= TOL
    assert (o["masks"][:-1] > 0).mean() > 1e-3
    _compare_blend(out.cpu().numpy(), o["blend"], bad)


def test_rejected_calls_write_nothing(dev):
    from svs_hip import lib
    from svs_hip.ops import _ptr, _ptr_array, _stream
    L = lib.load()
    H, W, n = 16, 24, 3
    a = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731
    imgs, dirs = [a(H, W, 3) for _ in range(17)], [a(H, W, 3) for _ in range(17)]
    rd, pr, mx, my = a(H, W, 3), a(H, W, 3), a(17, H, W), a(17, H, W)
    g = torch.zeros(17, H, W, dtype=torch.uint8, device=dev)
    ws = torch.full((int(L.svs_ibr_workspace_bytes(16, H, W)),), 7, dtype=torch.uint8, device=dev)
    fill = torch.full((18, H, W, 3), 7.0, device=dev)
    masks = torch.full((18, H, W), 7.0, device=dev)
    out = torch.full((H, W, 3), 7.0, device=dev)

    def weights(n_, h, w, **over):
        p = dict(imgs=_ptr_array(imgs), dirs=_ptr_array(dirs), rd=_ptr(rd), pr=_ptr(pr), g=_ptr(g), mx=_ptr(mx), my=_ptr(my),
                 ws=_ptr(ws), fill=_ptr(fill), masks=_ptr(masks))
        p.update(over)
        return L.svs_ibr_weights(p["imgs"], p["dirs"], p["rd"], p["pr"], p["g"], p["mx"], p["my"], n_, h, w, p["ws"],
                                 p["fill"], p["masks"], _stream())

    def blend(n_, h, w, **over):
        p = dict(fill=_ptr(fill), masks=_ptr(masks), ws=_ptr(ws), out=_ptr(out))
        p.update(over)
        return L.svs_ibr_laplacian_blend(p["fill"], p["masks"], n_, h, w, p["ws"], p["out"], _stream())

    for h, w in ((12, 24), (16, 20), (0, 24), (16, -8)):
        assert weights(n, h, w) == SVS_ESHAPE and blend(n, h, w) == SVS_ESHAPE
    for n_ in (0, 17, -1):
        assert weights(n_, H, W) == SVS_EINVAL and blend(n_, H, W) == SVS_EINVAL
    for k in ("imgs", "dirs", "rd", "pr", "g", "mx", "my", "ws", "fill", "masks"):
        assert weights(n, H, W, **{k: None}) == SVS_EINVAL, k
    for k in ("fill", "masks", "ws", "out"):
        assert blend(n, H, W, **{k: None}) == SVS_EINVAL, k
    torch.cuda.synchronize()
    for t in (fill, masks, out):
        assert bool((t == 7.0).all())
    assert bool((ws == 7).all())
    # and a valid call does write
    assert weights(n, H, W) == 0 and blend(n, H, W) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


def test_shape_errors_before_gpu_work(dev):
    from svs_hip import ibr
    v = synth.make_fusion_views(3, hw=(16, 24), n_views=2)
    with pytest.raises(AssertionError):
        ibr.blend_view(v[0], [dict(v[1], depth=v[1]["depth"][:8])], v[0]["img"])
    with pytest.raises(AssertionError):
        ibr.blend_view(v[0], [v[1]], v[0]["img"][:8])
    w = synth.make_fusion_views(3, hw=(20, 24), n_views=2)
    with pytest.raises(ValueError):
        ibr.blend_view(w[0], [w[1]], w[0]["img"])
    with pytest.raises(ValueError):
        ibr.blend_view(v[0], [], v[0]["img"])
