"""svs_hip.meshtexture without a GPU: the layout's tap-ownership property in exact arithmetic, ranks and rotations on hand-made
faces, `cell_for`, the OBJ round trip, the runner key, the oracle's gather against meshpaint's, the oracle's own fragile
share on every case of the table, and what a texture is for: a baked atlas beats the vertex colours on held-out views."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import meshpaint_oracle as mp
import meshtexture_cases as cases
import meshtexture_oracle as mt
import meshview_oracle as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build():
    spec = importlib.util.spec_from_file_location("svs_build", os.path.join(ROOT, "s-volsdf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the layout ------------------------------------------------------------------------------------------------------------
def _inside(h, c, X, Y):
    """the closed triangle of chart h in quarter texels (X = 4 x), exact in integers"""
    if h == 0:
        return (X >= 4) & (Y >= 4) & (X + Y <= 4 * (c - 3))
    return (X <= 4 * (c - 2)) & (Y <= 4 * (c - 2)) & (X + Y >= 4 * c)


@pytest.mark.parametrize("c", range(6, 41))
def test_every_tap_of_a_chart_belongs_to_it(c):
    """At every point of a chart's closed triangle, every bilinear tap with a non-zero weight (step 6 of svs_mesh_paint:
    x0 = floor(x) with weight 1 - fx > 0 always, x0 + 1 with weight fx, non-zero iff fx > 0; likewise y) is a texel of the
    same cell that belongs to the same chart.  EXACT: the set of taps is constant on every piece of the arrangement of the
    integer lines (open unit squares, open unit edges, lattice points); the triangles' corners are lattice points and their
    sides run along lattice lines or lattice diagonals, so every piece that meets a closed triangle holds a point of it with
    coordinates in quarters (a lattice point, an edge's midpoint, or a square's (1/4, 1/4), centre or (3/4, 3/4)).  All such
    points are walked, in integers."""
    Y, X = np.meshgrid(np.arange(0, 4 * c + 1), np.arange(0, 4 * c + 1), indexing="ij")
    violations = 0
    for h in (0, 1):
        A = mt.corners(h, c)
        at = _inside(h, c, X, Y)
        assert all(_inside(h, c, 4 * a[0], 4 * a[1]) for a in A) and at.sum() > 0
        x, y = X[at], Y[at]
        for dx in (0, 1):
            for dy in (0, 1):
                live = ((dx == 0) | (x % 4 > 0)) & ((dy == 0) | (y % 4 > 0))      # the tap's weight is not zero
                i, j = x // 4 + dx, y // 4 + dy
                bad = live & ~((i >= 0) & (i < c) & (j >= 0) & (j < c) & (mt.owner(i, j, c) == h))
                violations += int(bad.sum())
    assert violations == 0
    # the share of a cell's texels inside one of its two closed triangles
    j, i = np.meshgrid(np.arange(c), np.arange(c), indexing="ij")
    share = (_inside(0, c, 4 * i, 4 * j) | _inside(1, c, 4 * i, 4 * j)).sum() / (c * c)
    want = {6: 0.25, 16: 0.66, 32: 0.82}.get(c)
    assert want is None or abs(share - want) < 0.005
    # a texel centre's barycentrics are those of its chart: the corners come out as unit vectors, the hypotenuse has b0 = 0
    faces = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    chart = np.array([0, 4], np.int32)
    has, idx, b = mt.texels(faces, 3, chart, np.array([0, 1], np.int32), c, c)
    assert has.all() and has.shape == (c, c)
    for h in (0, 1):
        A = mt.corners(h, c)
        for k in range(3):
            assert np.array_equal(b[A[k, 1], A[k, 0]], np.eye(3)[k]) and np.array_equal(idx[A[k, 1], A[k, 0]], faces[h])
    assert (np.abs(b.sum(-1) - 1) < 1e-15).all() and (b >= 0).all()


def test_ranks_rotations_and_ties():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0.5, np.sqrt(0.75), 0],            # 0 1 2: equilateral in float64? not in float32
                      [0, 0, 1], [2, 0, 1], [0, 2, 1],                          # 3 4 5: right isosceles, the long edge opposite 3
                      [0, 0, 2], [3, 0, 2], [0, 1, 2],                          # 6 7 8: scalene
                      [0, 0, 3], [1, 0, 3], [2, 0, 3], [np.nan, 0, 0]], np.float32)
    eq = np.array([[0, 0, 4], [2, 0, 4], [0, 2, 4], [2, 2, 4]], np.float32)      # exact ties: 13 14 15 16
    verts = np.concatenate([verts, eq])
    faces = np.array([[9, 10, 11],        # collinear: not valid
                      [3, 4, 5],          # d = (8, 4, 4): r = 0
                      [4, 5, 3],          # d = (4, 4, 8): r = 2
                      [5, 3, 4],          # d = (4, 8, 4): r = 1
                      [0, 1, 99],         # index out of range
                      [13, 14, 15],       # d = (8, 4, 4): r = 0
                      [14, 16, 15],       # legs 2 and 2 at 16, corners: d_0 = |15-16|^2 = 4, d_1 = |14-15|^2 = 8, d_2 = 4: r = 1
                      [13, 14, 13],       # a repeated index: zero area
                      [0, 1, 12],         # a NaN corner
                      [6, 7, 8],          # d_0 = |8-7|^2 = 10, d_1 = |6-8|^2 = 1, d_2 = 9: r = 0
                      [-1, 0, 1]], np.int32)
    chart, counts = mt.slots(verts, faces)
    assert counts == [6, 5]
    assert chart.tolist() == [-1, 0 * 4 + 0, 1 * 4 + 2, 2 * 4 + 1, -1, 3 * 4 + 0, 4 * 4 + 1, -1, -1, 5 * 4 + 0, -1]
    # two equal longest edges: the first corner whose opposite edge is longest wins
    iso = np.array([[0, 0, 0], [2, 0, 0], [1, 5, 0]], np.float32)                 # d = (26, 26, 4)
    for tri, r in (([0, 1, 2], 0), ([2, 0, 1], 1), ([1, 2, 0], 0)):              # d = (26,26,4), (4,26,26), (26,4,26)
        assert mt.slots(iso, np.array([tri], np.int32))[0].tolist() == [r]
    # all three equal (exactly, in float32): r = 0
    same = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    assert mt.slots(same, np.array([[0, 1, 2], [2, 0, 1]], np.int32))[0].tolist() == [0, 4]
    # the layout: slot s in cell s >> 1, half s & 1; an odd count leaves the last upper half empty
    uv, slot_face = mt.layout(chart, 20, 6)
    assert slot_face.tolist() == [1, 2, 3, 5, 6, 9] and (uv[chart < 0] == 0).all()
    T = mt.corner_texels(chart, 20, 6)
    assert T[1].tolist() == [[1, 1], [2, 1], [1, 2]]                             # slot 0, r = 0: lower half of cell 0
    assert T[2].tolist() == [[2, 4], [4, 2], [4, 4]]                             # slot 1, r = 2: corner 2 at A0 of the upper half
    assert T[3].tolist() == [[6 + 1, 2], [6 + 1, 1], [6 + 2, 1]]                 # slot 2, r = 1: cell 1, corner 1 at A0
    assert T[9].tolist() == [[16, 4], [14, 4], [16, 2]]                          # slot 5: upper half of cell 2 (n = 3)
    assert np.array_equal(uv[1, 0], np.float32([1.5 / 20, 1 - 1.5 / 20]))
    for bad in (dict(S=20, c=5), dict(S=5, c=6), dict(S=11, c=6)):               # c < 6, S < c, 2 n n = 2 < 6
        with pytest.raises(ValueError):
            mt.layout(chart, **bad)


def test_cell_for_at_its_edges():
    from svs_hip import meshtexture
    assert meshtexture.cell_for(0, 4096) == 4096 and meshtexture.cell_for(2, 4096) == 4096 and meshtexture.cell_for(3, 4096) == 2048
    assert meshtexture.cell_for(8, 64) == 32 and meshtexture.cell_for(9, 64) == 21 and meshtexture.cell_for(2 * 10 * 10, 64) == 6
    assert meshtexture.cell_for(141_000, 4096) == 15 and 2 * (4096 // 15) ** 2 >= 141_000 > 2 * (4096 // 16) ** 2
    with pytest.raises(ValueError, match="201.*64"):
        meshtexture.cell_for(201, 64)
    with pytest.raises(ValueError, match="1 .*5"):
        meshtexture.cell_for(1, 5)
    with pytest.raises(ValueError, match="51.*31"):
        meshtexture.cell_for(51, 31)                                              # 2 (31 // 6)^2 = 50
    for n, size in ((1, 6), (50, 31), (33, 31), (1000, 300)):
        c = meshtexture.cell_for(n, size)
        assert c >= 6 and 2 * (size // c) ** 2 >= n and (c == size or 2 * (size // (c + 1)) ** 2 < n)
        mt.check_layout(n, size, c)
    assert meshtexture.rows_for(0, 20, 6) == 0 and meshtexture.rows_for(1, 20, 6) == 6 and meshtexture.rows_for(6, 20, 6) == 6
    assert meshtexture.rows_for(7, 20, 6) == 12 and meshtexture.rows_for(18, 20, 6) == 18 == mt.rows_of(18, 20, 6)


def test_obj_round_trip(tmp_path):
    from svs_hip import obj
    rng = np.random.default_rng(3)
    verts = rng.normal(size=(7, 3)).astype(np.float32)
    faces = np.array([[0, 1, 2], [2, 3, 4], [0, 1, 9], [4, 5, 6], [6, 0, 3]], np.int32)
    chart = np.array([0, 6, -1, 9, 13], np.int32)
    uv = rng.random((5, 3, 2)).astype(np.float32)
    atlas = rng.integers(0, 256, (20, 20, 3)).astype(np.uint8)
    path = str(tmp_path / "out" / "mesh.obj")
    assert obj.write(path, verts, faces, uv, chart, atlas) == 1
    first = {ext: open(path[:-4] + ext, "rb").read() for ext in (".obj", ".mtl", ".png")}
    got = obj.read(path)
    assert np.array_equal(got["verts"].astype(np.float32), verts) and np.array_equal(got["faces"], faces[chart >= 0])
    assert np.array_equal(got["uv"].astype(np.float32), uv[chart >= 0]) and np.array_equal(got["atlas"], atlas)
    assert got["mtl"] == path[:-4] + ".mtl" and got["png"] == path[:-4] + ".png"
    text = first[".obj"].decode("ascii").splitlines()
    assert text[0] == "mtllib mesh.mtl" and sum(t.startswith("v ") for t in text) == 7 and sum(t.startswith("vt ") for t in text) == 12
    assert "usemtl atlas" in text and text[-1] == "f 7/10 1/11 4/12" and text[-4] == "f 1/1 2/2 3/3"
    assert b"map_Kd mesh.png" in first[".mtl"]
    assert obj.write(path, verts, faces, uv, chart, atlas) == 1                  # byte-stable on a second write
    assert first == {ext: open(path[:-4] + ext, "rb").read() for ext in (".obj", ".mtl", ".png")}
    with pytest.raises(ValueError, match=".obj"):
        obj.write(str(tmp_path / "mesh.ply"), verts, faces, uv, chart, atlas)
    with pytest.raises(ValueError, match="obj.write"):
        obj.write(path, verts, faces, uv[:4], chart, atlas)


def test_runner_carries_the_key(tmp_path):
    from svs_hip import run
    args = run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", "+tsdf_texture=2048"])
    assert args["tsdf_texture"] == 2048 and run.check_tsdf_texture(args) == 2048
    assert "tsdf_texture" not in run.default_args() and run.check_tsdf_texture(run.default_args()) is None
    with pytest.raises(KeyError):
        run.apply_overrides(run.default_args(), ["tsdf_texture=2048"])
    alone = run.apply_overrides(run.default_args(), ["+tsdf_texture=2048", f"outdir={tmp_path / 'out'}"])
    with pytest.raises(ValueError, match="tsdf_texture.*tsdf_voxel"):
        run.run_help(alone, select_device=False)
    assert not os.path.exists(tmp_path / "out")                                   # refused before anything is made
    for bad in ("63", "16385", "0.5", "2048.0", "true", "big", "-64"):
        with pytest.raises(ValueError, match="tsdf_texture"):
            run.check_tsdf_texture(run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", f"+tsdf_texture={bad}"]))
    for good in (64, 16384):
        assert run.check_tsdf_texture(run.apply_overrides(run.default_args(), ["+tsdf_voxel=1.5", f"+tsdf_texture={good}"])) == good
    assert run.tsdf_texture_obj_name("o", "scan106") == os.path.join("o", "tsdf_texture", "mvsnet106_l3.obj")
    assert "+tsdf_texture=S" in run.__doc__


def test_symbols_unit_and_command_line():
    from svs_hip import lib, meshtexture
    for name, nargs in (("svs_mesh_atlas_slots", 8), ("svs_mesh_atlas_uv", 8), ("svs_mesh_atlas_bake", 25), ("svs_mesh_atlas_finish", 14),
                        ("svs_mesh_atlas_render", 16)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
    assert lib.SIGNATURES["svs_mesh_atlas_bake"][1][16] is ctypes.POINTER(ctypes.c_void_p)      # images: a host array
    assert lib.ABI_VERSION == 101
    assert _build().UNITS["svs_meshtexture.hip"] == ["-ffp-contract=off"]
    assert meshtexture.RULES == dict(meshtexture._mp.RULES, mode="blend") and meshtexture.MIN_CELL == mt.MIN_CELL == 6
    base = ["--ply", "in.ply", "--scan-folder", "scan1", "--views", "1", "2", "--obj-out", "out.obj"]
    a = meshtexture.parse_args(base)
    assert (a.size, a.cell, a.holdout, a.mode, a.fill) == (4096, None, [], "blend", [128, 128, 128])
    a = meshtexture.parse_args(base + ["--size", "512", "--cell", "9", "--holdout", "3", "--mode", "best", "--no-normals", "--one-sided"])
    assert (a.size, a.cell, a.holdout, a.mode, a.no_normals, a.one_sided) == (512, 9, [3], "best", True, True)
    for bad in (["--size", "5"], ["--cell", "5"], ["--size", "64", "--cell", "65"], ["--holdout", "2"], ["--power", "9"],
                ["--cos-min", "2"], ["--rel", "-1"], ["--mode", "mean"], ["--fill", "0", "0", "256"], ["--obj-out", "out.ply"]):
        with pytest.raises(SystemExit):
            meshtexture.parse_args(base + bad)
    with pytest.raises(TypeError, match="svs_mesh_atlas_bake.*spread_rounds"):
        meshtexture._rules(dict(spread_rounds=3))
    with pytest.raises(ValueError, match="svs_mesh_paint"):
        meshtexture._rules(dict(power=9))
    with pytest.raises(ValueError, match="svs_mesh_paint"):
        meshtexture._rules(dict(mode="mean"))


# ---- the gather ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rules", cases.RULES, ids=lambda r: "-".join(f"{k}={v}" for k, v in r.items()) or "defaults")
def test_gather_is_meshpaints_on_float32_points(rules):
    """on points and normals that float32 holds, `gather` returns `meshpaint_oracle.paint`'s accumulators and fragile flags
    bit for bit: the two loops are one statement list"""
    s = cases.scene()
    views = mv.cameras(3)
    r = cases.rastered(s, views)
    images, masks = cases.photographs(s, views), cases.masks_for(3)
    kw = {k: v for k, v in rules.items() if k != "use_normals"}
    normals = None
    if rules.get("use_normals", True):
        normals = mp.vertex_normals(s["verts"], s["faces"])[0].astype(np.float32)
    want, want_fragile = mp.paint(s["verts"], normals, views, r["depth"], images, masks, **kw)
    p = s["verts"].astype(np.float64)
    n64 = None if normals is None else normals.astype(np.float64)
    lit = None if normals is None else np.isfinite(n64).all(1) & ~(n64 == 0).all(1)
    got, got_fragile = mt.gather(p, n64, lit, views, r["depth"], images, masks, **kw)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)) and np.array_equal(got_fragile, want_fragile)
    assert rules.get("cos_min") == 1.0 or (want[:, 3] > 0).sum() > 100


# ---- the table ---------------------------------------------------------------------------------------------------------------
def _oracle_bake(c):
    i = cases.case_inputs(c)
    s = i["s"]
    r = cases.rastered(s, i["views"])
    normals = None
    if i["rules"].pop("use_normals", True):
        normals = mp.vertex_normals(s["verts"], s["faces"])[0].astype(np.float32)
    uv, slot_face = mt.layout(s["chart"], i["size"], i["cell"])
    acc, fragile = mt.bake(s["verts"], normals, s["faces"], s["chart"], slot_face, i["size"], i["cell"], i["views"], r["depth"],
                           i["images"], i["masks"], **i["rules"])
    return i, slot_face, acc, fragile


@pytest.mark.parametrize("c", cases.BAKE_CASES, ids=lambda c: c["name"])
def test_the_oracles_fragile_share(c):
    """at most 0.1 % of the texels with a face are fragile in the oracle itself, on every case of the table: the cap the GPU
    tests use is one the reference is known to meet"""
    i, slot_face, acc, fragile = _oracle_bake(c)
    has = mt.texels(i["s"]["faces"], len(i["s"]["verts"]), i["s"]["chart"], slot_face, i["size"], i["cell"])[0]
    n = int(has.sum())
    print(f"{c['name']}: {n} texels with a face of {has.size}, {int(fragile.sum())} fragile, {int((acc[..., 3] > 0).sum())} baked")
    assert n > 0.2 * has.size and not fragile[~has].any() and fragile.sum() <= 0.001 * n
    assert (acc[~has] == 0).all()
    if c["rules"].get("cos_min") != 1.0:
        assert (acc[..., 3] > 0).sum() > 0.1 * n


# ---- what it is for -----------------------------------------------------------------------------------------------------------
def held_out_scores(bake_fn=None, render_fn=None):
    """the patterned scene baked from four views at cell 16 and rendered into the two held-out ones, through the baked atlas
    and through the vertex-colour atlas -> (baked score, vertex score).  bake_fn / render_fn: the device's, for the GPU test"""
    p = cases.pattern_scene()
    cell = 16
    size = cases.atlas_size(p["n_valid"], cell)
    uv, slot_face = mt.layout(p["chart"], size, cell)
    b, h = p["bake"], p["held"]
    if bake_fn is None:
        normals = mp.vertex_normals(p["verts"], p["faces"])[0].astype(np.float32)
        acc = mt.bake(p["verts"], normals, p["faces"], p["chart"], slot_face, size, cell, b["views"], b["depth"], b["images"], b["masks"])[0]
        baked = mt.finish(acc, p["faces"], len(p["verts"]), p["chart"], slot_face, size, cell, p["colors"])[0]
        plain = mt.finish(None, p["faces"], len(p["verts"]), p["chart"], slot_face, size, cell, p["colors"])[0]
    else:
        baked, plain = bake_fn(p, size, cell)
    render = render_fn or (lambda atlas: mt.render(h["face"], p["verts"], p["faces"], p["chart"], h["views"], atlas, cell)[0])
    return tuple(mt.score(render(a), h["face"], p["chart"], h["images"], h["masks"]) for a in (baked, plain))


def test_a_baked_atlas_beats_the_vertex_colours_on_held_out_views():
    """`meshview_oracle.scene(12, 24)` photographed per pixel in an analytic pattern whose period is a few pixels and under a
    face: the atlas baked from four views scores a strictly higher PSNR on two held-out views than the atlas of the
    interpolated vertex colours (the pattern itself at the vertices: the best colours a vertex can have).  No margin is fixed.
    Measured: baked 13.70 dB (mean |difference| 35.98 codes), vertex colours 9.60 dB (67.97 codes), over 4178 pixels."""
    baked, plain = held_out_scores()
    print(f"held-out views: {baked['n']} pixels; baked atlas PSNR {baked['psnr']:.2f} dB, mean |difference| {baked['mad']:.2f} codes; "
          f"vertex colours {plain['psnr']:.2f} dB, {plain['mad']:.2f} codes")
    assert baked["n"] == plain["n"] > 1000
    assert baked["psnr"] > plain["psnr"] and baked["mad"] < plain["mad"]
