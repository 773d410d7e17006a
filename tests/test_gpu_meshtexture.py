"""svs_hip.meshtexture on the GPU against the float64 oracle (tests/meshtexture_oracle.py): slots, rotations and the layout at
their edges, the bake over the table of tests/meshtexture_cases.py, the conversion to codes in all its branches, the
renderer, repeatability, bad input, empty input, the folder path, the command line, the runner key, and what a texture is for.

Comparison rule, test_gpu_meshpaint.py's.  The oracle is given what the device was given: the depth maps the GPU rasterised
and the float32 vertex normals the GPU computed.  At most 0.1 % of the texels with a face may be `fragile` (a decision within
1e-9 of flipping; tests/test_meshtexture_cpu.py shows the oracle itself stays under that cap on every case); outside them
`acc` agrees to 1e-12 relative (meshpaint's bound and argument: every term is non-negative, a term costs about 30 float64
operations after the nine of the texel's point and the twenty of its normal, and there are at most 17 views), and `atlas` and
`covered` are exactly the oracle's.  Slots, rotations, uv, slot_face and the conversion to codes are exact everywhere."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import meshpaint_oracle as mp
import meshtexture_cases as cases
import meshtexture_oracle as mt
import meshview_oracle as mv
import tsdf_oracle as to
from svs_hip import lib, meshpaint, meshtexture, meshview, obj
from svs_hip import views as svs_views
from svs_hip.lib import SvsError
from test_gpu_meshview import VIEW_IDS, scan_folder  # noqa: F401  -- the scan folder fixture and its view ids

pytestmark = pytest.mark.gpu
ACC_TOL = 1e-12
DEV = "cuda"
H, W = cases.H, cases.W


def _np(t):
    return None if t is None else t.cpu().numpy()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(DEV)


# ---- slots, uv, slot_face ------------------------------------------------------------------------------------------------------
def _layout_case(verts, faces, size, cell, what):
    """slots and layout on the GPU, every integer and every float32 equal to the oracle's -> chart, slot_face (numpy)"""
    chart, n_valid = meshtexture.slots(verts, faces)
    want_chart, counts = mt.slots(verts, faces)
    assert chart.dtype == torch.int32 and np.array_equal(_np(chart), want_chart), what
    assert n_valid == counts[0]
    uv, slot_face = meshtexture.layout(chart, n_valid, size, cell)
    want_uv, want_slot_face = mt.layout(want_chart, size, cell)
    assert uv.dtype == torch.float32 and tuple(uv.shape) == (len(faces), 3, 2) and slot_face.dtype == torch.int32
    assert np.array_equal(_np(uv).view(np.uint32), want_uv.view(np.uint32)), what
    assert np.array_equal(_np(slot_face), want_slot_face), what
    return want_chart, want_slot_face


def _fan(n_faces, seed=0):
    """n_faces generic triangles on vertices of their own"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(3 * max(n_faces, 1), 3)).astype(np.float32), np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


@pytest.mark.parametrize("n_faces", [0, 1, 2, 3, 18, 255, 256, 257, 4097])
def test_slots_and_layout_counts(n_faces):
    """0 to 3 faces (an odd count leaves the last cell's upper half empty), exactly 2 n n faces, the block edges of the
    kernels (256) and of the scan (4096)"""
    verts, faces = _fan(n_faces, seed=n_faces)
    n = 1
    while 2 * n * n < n_faces:
        n += 1
    for cell, size in ((6, 6 * n), (7, 7 * n + 3), (6, 6 * n + 2)):
        _layout_case(verts, faces, size, cell, f"{n_faces} faces, cell {cell}, atlas {size}")


def test_layout_is_full_at_2nn_and_refuses_one_more():
    verts, faces = _fan(19)
    chart, slot_face = _layout_case(verts, faces[:18], 20, 6, "18 faces in 3 x 3 cells, an unused margin of 2 texels")
    assert slot_face.tolist() == list(range(18))
    chart, n_valid = meshtexture.slots(verts, faces)
    assert n_valid == 19
    calls = dict(meshtexture.ENTRY_CALLS)
    for size, cell, named in ((20, 6, "19 charts"), (20, 5, "cell"), (5, 6, "cell"), (40000, 6, "atlas")):
        with pytest.raises(SvsError, match=f"svs_mesh_atlas_uv.*{named}"):
            meshtexture.layout(chart, n_valid, size, cell)
    assert meshtexture.ENTRY_CALLS["uv"] - calls["uv"] == 4
    with pytest.raises(ValueError, match="19.*11"):
        meshtexture.cell_for(19, 11)
    assert meshtexture.cell_for(19, 24) == 6 and meshtexture.cell_for(18, 20) == 6


@pytest.mark.parametrize("where", ["first", "last", "interleaved"])
def test_invalid_faces_take_no_slot(where):
    verts, faces = _fan(40, seed=7)
    verts[5] = np.nan
    bad = np.array([[0, 1, 120], [-1, 2, 3], [3, 4, 5], [0, 0, 1], [6, 7, 2 ** 31 - 1]], np.int32)
    if where == "first":
        faces = np.concatenate([bad, faces])
    elif where == "last":
        faces = np.concatenate([faces, bad])
    else:
        out = []
        for k, f in enumerate(faces):
            out += [f, bad[k % len(bad)]] if k % 3 == 0 else [f]
        faces = np.array(out, np.int32)
    chart, slot_face = _layout_case(verts, faces, 6 * 5 + 1, 6, where)
    assert (chart < 0).sum() >= len(bad) and len(slot_face) == (chart >= 0).sum()


def test_rotations_and_ties_of_the_cpu_test():
    iso = np.array([[0, 0, 0], [2, 0, 0], [1, 5, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    faces = np.array([[0, 1, 2], [2, 0, 1], [1, 2, 0], [3, 4, 5], [5, 3, 4]], np.int32)
    chart, _ = _layout_case(iso, faces, 18, 6, "ties")
    assert (chart & 3).tolist() == [0, 1, 0, 0, 0]


# ---- bake ----------------------------------------------------------------------------------------------------------------------
def _check_acc(got, want, fragile, has, what):
    n = int(has.sum())
    n_frag = int(fragile.sum())
    assert n_frag <= 0.001 * n, f"{what}: {n_frag} fragile texels of {n}"
    ok = ~fragile
    g, w = got[ok], want[ok]
    assert np.array_equal(g == 0, w == 0), f"{what}: the accumulators are not empty in the same places"
    with np.errstate(all="ignore"):
        ratio = np.where(w != 0, np.abs(g - w) / (ACC_TOL * np.abs(w)), 0.0)
    worst = float(ratio.max(initial=0.0))
    print(f"{what}: {n} texels with a face, {n_frag} fragile, {int((want[..., 3] > 0).sum())} baked, acc error {worst:.4f} of the bound")
    assert worst <= 1.0
    return ok


def _bake(s, views, images, masks, size, cell, rules, what, colors=None):
    """texture on the GPU and by the oracle on the same depth maps and normals, compared by the rule -> dict of both sides"""
    rules = dict(rules)
    mode = rules.get("mode", "blend")
    colors = s.get("colors") if colors is None else colors
    depth = meshview.rasterize(s["verts"], s["faces"], views, H, W)["depth"]
    stats = {}
    tex = meshtexture.texture(s["verts"], s["faces"], views, images, masks, size=size, cell=cell, vert_colors=colors, depth=depth,
                              stats=stats, **rules)
    assert tex["atlas"].dtype == torch.uint8 and tuple(tex["atlas"].shape) == (size, size, 3) and tex["atlas"].is_cuda
    assert tex["covered"].dtype == torch.uint8 and tuple(tex["covered"].shape) == (size, size) and tex["cell"] == cell
    chart, counts = mt.slots(s["verts"], s["faces"])
    uv, slot_face = mt.layout(chart, size, cell)
    assert np.array_equal(_np(tex["chart"]), chart) and np.array_equal(_np(tex["uv"]), uv) and stats["n_slots"] == counts[0]
    assert np.array_equal(_np(stats["slot_face"]), slot_face)
    normals = _np(stats["normals"])
    assert (normals is None) == (not rules.get("use_normals", True))
    kw = {k: v for k, v in rules.items() if k != "use_normals"}
    want, fragile = mt.bake(s["verts"], normals, s["faces"], chart, slot_face, size, cell, views, _np(depth), images, masks, **kw)
    has = mt.texels(s["faces"], len(s["verts"]), chart, slot_face, size, cell)[0]
    acc = _np(stats["acc"])
    assert acc.shape == want.shape == (mt.rows_of(counts[0], size, cell), size, 4)
    ok = _check_acc(acc, want, fragile, has, what)
    atlas, covered = mt.finish(want, s["faces"], len(s["verts"]), chart, slot_face, size, cell, colors, mode)
    rows = acc.shape[0]
    assert np.array_equal(_np(tex["atlas"])[:rows][ok], atlas[:rows][ok]) and np.array_equal(_np(tex["covered"])[:rows][ok], covered[:rows][ok])
    assert np.array_equal(_np(tex["atlas"])[rows:], atlas[rows:]) and not _np(tex["covered"])[rows:].any()
    return dict(tex=tex, acc=acc, want=want, fragile=fragile, has=has, chart=chart, slot_face=slot_face, depth=depth, normals=normals,
                atlas=atlas, covered=covered)


def test_the_rules_list_is_meshpaints():
    from test_gpu_meshpaint import RULES
    assert cases.RULES == RULES


@pytest.mark.parametrize("c", cases.BAKE_CASES, ids=lambda c: c["name"])
def test_bake_table(c):
    i = cases.case_inputs(c)
    calls = dict(meshtexture.ENTRY_CALLS)
    res = _bake(i["s"], i["views"], i["images"], i["masks"], i["size"], i["cell"], i["rules"], c["name"])
    assert meshtexture.ENTRY_CALLS["bake"] - calls["bake"] == (c["n_views"] + 15) // 16      # 17 views: accumulated in two launches
    assert meshtexture.ENTRY_CALLS["finish"] - calls["finish"] == 1 and meshtexture.ENTRY_CALLS["slots"] - calls["slots"] == 1
    covered = res["covered"]
    assert set(np.unique(covered[:res["acc"].shape[0]][res["has"]])) <= {1, 2} and not covered[:res["acc"].shape[0]][~res["has"]].any()
    if c["rules"].get("cos_min") == 1.0:
        assert not (covered == 1).any() and (covered == 2).sum() == res["has"].sum()
    else:
        assert (covered == 1).sum() > 0.1 * res["has"].sum()


@pytest.mark.parametrize("size,cell,n_faces", [(16, 6, 8), (17, 6, 7), (16, 16, 2), (17, 16, 1), (6, 6, 2), (7, 7, 1), (20, 6, 18)])
def test_bake_small_atlases(size, cell, n_faces):
    """atlases of 16 x 16 texels (one workgroup exactly) and 17 x 17 (one texel row into the second), the smallest atlas,
    cell 7, an odd count whose last upper half stays empty, and an unused margin"""
    s = cases.scene()
    views = mv.cameras(3)
    zbuf = cases.rastered(s, views)["face"][0]
    seen = np.unique(zbuf[zbuf >= 0])[:n_faces]                  # faces the first camera sees
    assert len(seen) == n_faces
    part = dict(verts=s["verts"], faces=s["faces"][seen], colors=s["colors"])
    res = _bake(part, views, cases.photographs(s, views), None, size, cell, {}, f"{n_faces} faces, atlas {size}, cell {cell}")
    assert (res["covered"] == 1).sum() > 0
    if n_faces % 2:
        n = size // cell
        q = n_faces // 2
        j, i = np.nonzero(res["covered"][(q // n) * cell:(q // n + 1) * cell, (q % n) * cell:(q % n + 1) * cell] == 0)
        assert len(i) and (i + j > cell - 2).all()               # the last cell's upper half: not touched
    assert (_np(res["tex"]["atlas"])[res["covered"] == 0] == 128).all()


# ---- finish --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["blend", "best"])
def test_finish_is_exact_on_the_oracles_acc(mode):
    i = cases.case_inputs(dict(n_views=3, seed=0, rules=dict(mode=mode), masked=True, cell=16))
    s, size, cell = i["s"], i["size"], i["cell"]
    views = i["views"]
    r = cases.rastered(s, views)
    normals = mp.vertex_normals(s["verts"], s["faces"])[0].astype(np.float32)
    uv, slot_face = mt.layout(s["chart"], size, cell)
    acc = mt.bake(s["verts"], normals, s["faces"], s["chart"], slot_face, size, cell, views, r["depth"], i["images"], i["masks"], mode=mode)[0]
    faces_d, chart_d, slot_d, colors_d = _dev(s["faces"]), _dev(s["chart"]), _dev(slot_face), _dev(s["colors"])
    flags = meshpaint.flags_of(mode)
    for acc_in, colors, fill in ((acc, s["colors"], (128, 128, 128)), (acc, None, (1, 2, 3)), (None, s["colors"], (9, 8, 7)), (None, None, (5, 5, 5))):
        atlas, covered = meshtexture.finish(None if acc_in is None else _dev(acc_in), faces_d, len(s["verts"]), chart_d, slot_d, size, cell,
                                            None if colors is None else colors_d, flags, fill)
        want_atlas, want_covered = mt.finish(acc_in, s["faces"], len(s["verts"]), s["chart"], slot_face, size, cell, colors, mode, fill)
        assert np.array_equal(_np(atlas), want_atlas) and np.array_equal(_np(covered), want_covered)
        kinds = set(np.unique(want_covered))
        assert kinds == {(True, True): {0, 1, 2}, (True, False): {0, 1}, (False, True): {0, 2}, (False, False): {0}}[(acc_in is not None, colors is not None)]
    with pytest.raises(ValueError, match="svs_mesh_atlas_finish"):
        meshtexture.finish(_dev(acc[:-1]), faces_d, len(s["verts"]), chart_d, slot_d, size, cell, colors_d, flags)


# ---- render --------------------------------------------------------------------------------------------------------------------
def _render_case(verts, faces, views, atlas, chart, cell, what, min_pixels):
    verts_d, faces_d = svs_views.mesh_args(verts, faces)[:2]
    rgb, face = meshtexture.render(verts_d, faces_d, _dev(chart), _dev(atlas), cell, views, H, W, fill=(7, 77, 177))
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (len(views), H, W, 3) and face.dtype == torch.int32
    want, fragile = mt.render(_np(face), verts, faces, chart, views, atlas, cell, fill=(7, 77, 177))
    drawn = (_np(face) >= 0) & (chart[np.maximum(_np(face), 0)] >= 0)
    n, n_frag = int(drawn.sum()), int(fragile.sum())
    print(f"{what}: {n} pixels with a textured face, {n_frag} fragile")
    assert n >= min_pixels and n_frag <= 0.001 * n
    assert np.array_equal(_np(rgb)[~fragile], want[~fragile])
    assert (_np(rgb)[_np(face) < 0] == (7, 77, 177)).all()       # untouched where no face is seen
    return _np(rgb), _np(face)


def test_render_the_scene():
    s = cases.scene()
    rng = np.random.default_rng(2)
    for cell in (6, 16):
        size = cases.atlas_size(s["n_valid"], cell)
        atlas = rng.integers(0, 256, (size, size, 3)).astype(np.uint8)       # noise: every tap differs from its neighbours
        _render_case(s["verts"], s["faces"], mv.cameras(17, seed=3), atlas, s["chart"], cell, f"the scene, cell {cell}", 10000)


def test_render_a_bipyramid_edge_on():
    """an octahedron seen from a point in the plane of one of its faces: that face projects to a line"""
    verts = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 0.5], [0, 0, -0.5]], np.float32)
    faces = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [1, 0, 5], [2, 1, 5], [3, 2, 5], [0, 3, 5]], np.int32)
    K = np.array([[40.0, 0, 31.5], [0, 40.0, 23.5], [0, 0, 1]])
    views = [dict(K=K, E=to.look_at((2.0, -0.5, -0.25))), dict(K=K, E=to.look_at((0.5, 0.5, 2.0))), dict(K=K, E=to.look_at((2.7, 0.4, 0.9)))]
    # (no camera on an axis of symmetry: there whole rows of pixels land on integer atlas coordinates, and all are fragile)
    chart = mt.slots(verts, faces)[0]
    atlas = np.random.default_rng(4).integers(0, 256, (36, 36, 3)).astype(np.uint8)
    _render_case(verts, faces, views, atlas, chart, 9, "bipyramid", 500)


# ---- other cases ---------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_unaligned_tensors():
    s = cases.scene()
    views = mv.cameras(17, seed=3)
    rng = np.random.default_rng(8)
    images = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(17)]
    verts, faces = svs_views.mesh_args(s["verts"], s["faces"])[:2]
    depth = meshview.rasterize(verts, faces, views, H, W)["depth"]
    cell, size = 6, cases.atlas_size(s["n_valid"], 6)

    def shifted(t):                                              # the same values one element into a larger allocation
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        flat[1:] = t.reshape(-1)
        return flat[1:].view(t.shape)
    for mode in ("blend", "best"):
        runs = []
        for v, f in ((verts, faces), (verts, faces), (shifted(verts), shifted(faces))):
            stats = {}
            tex = meshtexture.texture(v, f, views, images, size=size, cell=cell, vert_colors=s["colors"], depth=depth, stats=stats, mode=mode)
            runs.append((stats["acc"].view(torch.int64), tex["atlas"], tex["covered"], tex["uv"].view(torch.int32), tex["chart"]))
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert torch.equal(a, b)
        assert int((runs[0][2] == 1).sum()) > 1000


def test_both_lane_orders_give_the_same_bytes():
    s = cases.scene()
    views = mv.cameras(3)
    images = cases.photographs(s, views)
    verts, faces = svs_views.mesh_args(s["verts"], s["faces"])[:2]
    normals = meshpaint.vertex_normals(verts, faces)
    depth = meshview.rasterize(verts, faces, views, H, W)["depth"]
    chart, n_valid = meshtexture.slots(verts, faces)
    for cell, size in ((6, cases.atlas_size(n_valid, 6)), (16, cases.atlas_size(n_valid, 16)), (7, 7 * 19)):
        slot_face = meshtexture.layout(chart, n_valid, size, cell)[1]
        by_row, by_cell = (meshtexture.bake(verts, faces, chart, slot_face, size, cell, views, images, normals=normals, depth=depth, order=o)
                           for o in ("row", "cell"))
        assert torch.equal(by_row.view(torch.int64), by_cell.view(torch.int64)) and int((by_row[..., 3] > 0).sum()) > 1000
    with pytest.raises(ValueError, match="svs_mesh_atlas_bake: order"):
        meshtexture.bake(verts, faces, chart, slot_face, size, cell, views, images, depth=depth, order="column")


def test_bad_input_is_skipped():
    """indices out of range and NaN, infinite and overflowing vertices take no slot; faces that use them are never
    dereferenced; the rest of the atlas is what the clean mesh gives in the same slots"""
    s = cases.scene()
    views = mv.cameras(3)
    images = cases.photographs(s, views)
    n = len(s["verts"])
    verts = np.concatenate([s["verts"], [[np.nan, 0.1, 0.2], [np.inf, 0.0, 0.0], [3e38, 3e38, 3e38]]]).astype(np.float32)
    # (a face whose corners are finite counts towards its vertices' normals, so the overflowing vertex meets no clean one)
    extra = np.array([[0, 1, len(verts)], [-1, 0, 1], [2 ** 31 - 1, 3, 4], [0, 1, n], [5, n + 1, 6], [n + 2, n + 2, n], [n, n + 1, n + 2]], np.int32)
    faces = np.concatenate([s["faces"], extra])
    colors = np.concatenate([s["colors"], np.zeros((3, 3), np.uint8)])
    cell, size = 16, cases.atlas_size(s["n_valid"], 16)
    bad = _bake(dict(verts=verts, faces=faces), views, images, None, size, cell, {}, "bad input", colors=colors)
    clean = _bake(s, views, images, None, size, cell, {}, "clean")
    assert (bad["chart"][len(s["faces"]):] == -1).all() and np.array_equal(bad["chart"][:len(s["faces"])], clean["chart"])
    both = ~bad["fragile"] & ~clean["fragile"]
    assert np.array_equal(_np(bad["tex"]["covered"]), _np(clean["tex"]["covered"]))
    assert np.array_equal(bad["acc"][both], clean["acc"][both])
    # a chart array that lies (slots beyond the count, rotation 3) is refused per entry, not followed
    chart = _dev(bad["chart"]).clone()
    first, second = (int(f) for f in bad["slot_face"][:2])
    chart[first], chart[second] = 4 * 100000, 4 * 1 + 3
    uv, slot_face = meshtexture.layout(chart, len(bad["slot_face"]), size, cell)
    assert (_np(uv)[[first, second]] == 0).all() and (_np(slot_face)[:2] == -1).all() and (_np(slot_face)[2:] >= 0).all()


def test_empty_mesh_and_zero_views_touch_nothing():
    s = cases.scene()
    views = mv.cameras(2)
    images = cases.photographs(s, views)
    tex = meshtexture.texture(s["verts"][:0], s["faces"][:0], views, images, size=12, fill=(1, 2, 3))
    assert tex["cell"] == 12 and tuple(tex["chart"].shape) == (0,) and tuple(tex["uv"].shape) == (0, 3, 2)
    assert (_np(tex["atlas"]) == (1, 2, 3)).all() and not _np(tex["covered"]).any()
    stats = {}
    tex = meshtexture.texture(s["verts"], s["faces"][:0], views, images, size=12, fill=(1, 2, 3), stats=stats)
    assert (_np(tex["atlas"]) == (1, 2, 3)).all() and tuple(stats["acc"].shape) == (0, 12, 4)
    with pytest.raises(ValueError, match="svs_mesh_atlas_bake: no views"):
        meshtexture.texture(s["verts"], s["faces"], [], [])
    # zero views at the entry itself: nothing is touched
    verts, faces = svs_views.mesh_args(s["verts"], s["faces"])[:2]
    chart, n_valid = meshtexture.slots(verts, faces)
    size, cell = cases.atlas_size(n_valid, 6), 6
    slot_face = meshtexture.layout(chart, n_valid, size, cell)[1]
    acc = torch.full((meshtexture.rows_for(n_valid, size, cell), size, 4), 3.5, dtype=torch.float64, device=DEV)
    mats = svs_views.mats(views, DEV)
    depth = torch.zeros((2, H, W), device=DEV)
    rc = meshtexture.bake_raw(verts, None, faces, chart, slot_face, size, cell, mats, 0, H, W, depth, [], None, acc)
    assert rc == 0 and float((acc - 3.5).abs().sum()) == 0
    rgb = torch.full((2, H, W, 3), 9, dtype=torch.uint8, device=DEV)
    face = torch.full((2, H, W), -1, dtype=torch.int32, device=DEV)
    assert meshtexture.render_raw(face, verts, faces, chart, mats, torch.zeros((size, size, 3), dtype=torch.uint8, device=DEV), cell, rgb) == 0
    assert int((rgb != 9).sum()) == 0
    # errors are the painter's, under this entry's name, and come before any launch
    dev_images = [_dev(im) for im in images]
    for kw in (dict(power=9), dict(cos_min=1.5), dict(near=0.0), dict(rel=-0.1), dict(flags=4)):
        rc = meshtexture.bake_raw(verts, None, faces, chart, slot_face, size, cell, mats, 2, H, W, depth, dev_images, None, acc, **kw)
        with pytest.raises(SvsError, match="svs_mesh_atlas_bake: "):
            lib.check(rc, "svs_mesh_atlas_bake")
    rc = meshtexture.bake_raw(verts, None, faces, chart, slot_face, size, 5, mats, 2, H, W, depth, dev_images, None, acc)
    assert rc == lib.ESHAPE
    rc = meshtexture.bake_raw(verts, None, faces, chart, slot_face, size, cell, mats, 2, H, W, depth, [dev_images[0], None], None, acc)
    with pytest.raises(SvsError, match="svs_mesh_atlas_bake: view 1"):
        lib.check(rc, "svs_mesh_atlas_bake")
    torch.cuda.synchronize()
    assert float((acc - 3.5).abs().sum()) == 0


# ---- the folder, the command, the runner -----------------------------------------------------------------------------------------
def _check_obj(path, verts, faces, tex):
    got = obj.read(path)
    chart = _np(tex["chart"])
    assert np.array_equal(got["verts"].astype(np.float32), np.asarray(verts, np.float32)) and np.array_equal(got["faces"], np.asarray(faces)[chart >= 0])
    assert np.array_equal(got["uv"].astype(np.float32), _np(tex["uv"])[chart >= 0]) and np.array_equal(got["atlas"], _np(tex["atlas"]))
    return got


def test_texture_folder_and_command(scan_folder):
    folder = str(scan_folder["folder"])
    out = str(scan_folder["root"] / "textured" / "sphere.obj")
    tex, stats = meshtexture.texture_folder(scan_folder["ply"], folder, VIEW_IDS, out, size=256)
    views = meshview.folder_cameras(folder, VIEW_IDS)
    images = meshpaint.folder_images(folder, VIEW_IDS)
    direct = meshtexture.texture(scan_folder["verts"], scan_folder["faces"], views, images, size=256, vert_colors=scan_folder["colors"])
    for k in ("atlas", "covered", "uv", "chart"):
        assert torch.equal(tex[k], direct[k])
    assert tex["cell"] == direct["cell"] == stats["cell"] == meshtexture.cell_for(int((tex["chart"] >= 0).sum()), 256)
    _check_obj(out, scan_folder["verts"], scan_folder["faces"], tex)
    assert stats["files"] == dict(obj=out, mtl=out[:-4] + ".mtl", png=out[:-4] + ".png") and all(os.path.exists(p) for p in stats["files"].values())
    assert stats["faces_written"] + stats["faces_left_out"] == stats["n_faces"] == len(scan_folder["faces"]) and stats["faces_left_out"] == 2 * 32
    assert stats["texels_baked"] == int((tex["covered"] == 1).sum()) > 1000 and stats["texels_from_vertices"] == int((tex["covered"] == 2).sum()) > 0
    assert stats["holdout"] is None and stats["launches"] == dict(slots=1, uv=1, bake=1, finish=1, render=0)
    assert list(stats["seconds"]) == ["read", "upload", "paint", "slots", "normals", "raster", "bake", "finish", "score", "download", "write"]
    assert stats["seconds"]["bake"] > 0 and stats["seconds"]["paint"] == 0           # the PLY has colours: nothing is painted first
    # the command: two views baked, the third held out, a PLY without colours (painted first)
    from svs_hip import ply
    bare = str(scan_folder["root"] / "bare.ply")
    ply.write(bare, scan_folder["verts"], None, scan_folder["faces"])
    cmd_out = str(scan_folder["root"] / "textured" / "cmd" / "two.obj")
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        tex2, st2 = meshtexture.main(["--ply", bare, "--scan-folder", folder, "--views", str(VIEW_IDS[0]), str(VIEW_IDS[1]), "--holdout",
                                      str(VIEW_IDS[2]), "--obj-out", cmd_out, "--size", "300", "--cell", "8", "--mode", "best", "--fill", "1", "2", "3"])
    assert "seconds: read" in text.getvalue() and cmd_out in text.getvalue() and "held-out views 28" in text.getvalue()
    painted = meshpaint.paint(scan_folder["verts"], scan_folder["faces"], views[:2], images[:2], mode="best", fill=(1, 2, 3))[0]
    direct = meshtexture.texture(scan_folder["verts"], scan_folder["faces"], views[:2], images[:2], size=300, cell=8, vert_colors=painted,
                                 mode="best", fill=(1, 2, 3))
    assert torch.equal(tex2["atlas"], direct["atlas"]) and tex2["cell"] == 8 and st2["seconds"]["paint"] > 0
    _check_obj(cmd_out, scan_folder["verts"], scan_folder["faces"], tex2)
    want = meshtexture.consistency(scan_folder["verts"], scan_folder["faces"], tex2, painted, views[2:], images[2:])
    assert st2["holdout"] == want and want["baked"]["n"] == want["vertex"]["n"] > 100 and np.isfinite(want["baked"]["psnr"])
    assert st2["launches"]["render"] == 2
    # the score is the oracle's on the device's picture
    rgb, face = meshtexture.render(scan_folder["verts"], scan_folder["faces"], tex2["chart"], tex2["atlas"], 8, views[2:], H, W)
    ref = mt.score(_np(rgb), _np(face), _np(tex2["chart"]), images[2:])
    assert ref["n"] == want["baked"]["n"] and abs(ref["psnr"] - want["baked"]["psnr"]) < 1e-9 and abs(ref["mad"] - want["baked"]["mad"]) < 1e-9


def test_runner_key(scan_folder):
    from svs_hip import ply, run
    root = scan_folder["root"]
    base = [f"outdir={root}", "filter_only=true", "eval_mask=false", "testlist=scan106", "+tsdf_voxel=0.05", "+tsdf_trunc=0.12"]
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(base + ["+tsdf_simplify=0.25", "+tsdf_texture=512"])
    out = root / "tsdf_texture" / "mvsnet106_l3.obj"
    assert all(os.path.exists(str(out)[:-4] + ext) for ext in (".obj", ".mtl", ".png"))
    assert text.getvalue().count("scan106 tsdf texture seconds: read ") == 1 and str(out) in text.getvalue()
    stats = res["textured_meshes"]["scan106"]
    sv, sf = ply.read_mesh(str(root / "tsdf_simple" / "mvsnet106_l3.ply"))       # the simplified mesh is the one textured
    got = obj.read(str(out))
    assert stats["n_faces"] == len(sf) and stats["size"] == 512 and got["atlas"].shape == (512, 512, 3)
    assert np.array_equal(got["verts"].astype(np.float32), sv.astype(np.float32)) and len(got["faces"]) == stats["faces_written"] > 100
    assert stats["texels_baked"] > 1000
    with contextlib.redirect_stdout(io.StringIO()):
        res = run.main(base + ["+tsdf_texture=128"])                           # without the other keys: the TSDF mesh itself
    assert res["textured_meshes"]["scan106"]["n_faces"] == len(ply.read_mesh(str(root / "tsdf" / "mvsnet106_l3.ply"))[1])
    with pytest.raises(ValueError, match="tsdf_texture"):
        run.main([f"outdir={root}", "filter_only=true", "testlist=scan106", "+tsdf_texture=512"])


# ---- what it is for --------------------------------------------------------------------------------------------------------------
def test_a_baked_atlas_beats_the_vertex_colours_on_held_out_views():
    """the held-out comparison of tests/test_meshtexture_cpu.py on the device's atlas, rendered by the device"""
    from test_meshtexture_cpu import held_out_scores
    p = cases.pattern_scene()
    b, h = p["bake"], p["held"]
    state = {}

    def bake_fn(p, size, cell):
        tex = meshtexture.texture(p["verts"], p["faces"], b["views"], b["images"], b["masks"], size=size, cell=cell, vert_colors=p["colors"],
                                  depth=b["depth"])
        verts, faces, colors = svs_views.mesh_args(p["verts"], p["faces"], p["colors"])
        slot_face = meshtexture.layout(tex["chart"], p["n_valid"], size, cell)[1]
        state.update(tex=tex, verts=verts, faces=faces)
        return tex["atlas"], meshtexture.vertex_atlas(faces, len(p["verts"]), tex["chart"], slot_face, size, cell, colors)

    def render_fn(atlas):
        return _np(meshtexture.render(state["verts"], state["faces"], state["tex"]["chart"], atlas, state["tex"]["cell"], h["views"], H, W,
                                      face=_dev(h["face"]))[0])
    baked, plain = held_out_scores(bake_fn, render_fn)
    print(f"held-out views on the device: {baked['n']} pixels; baked atlas PSNR {baked['psnr']:.2f} dB, mean |difference| {baked['mad']:.2f} "
          f"codes; vertex colours {plain['psnr']:.2f} dB, {plain['mad']:.2f} codes")
    assert baked["n"] == plain["n"] > 1000 and baked["psnr"] > plain["psnr"] and baked["mad"] < plain["mad"]
    # `consistency` gives the same two figures from its own rasterisation when the device's face map is the oracle's
    both = meshtexture.consistency(p["verts"], p["faces"], state["tex"], p["colors"], h["views"], h["images"], h["masks"])
    assert both["baked"]["psnr"] > both["vertex"]["psnr"]
