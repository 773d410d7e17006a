"""svs_hip.mesh without a GPU: the generated marching-cubes table (every case, closed oriented manifolds with the float64
oracle), the grid axes, the DTU box lookup and the mesh PLY."""
import importlib.util
import os

import numpy as np
import pytest

import mesh_oracle as mo
from svs_hip import mc_table, mesh, ply, scans

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_reproduces_the_committed_table():
    gen = _generator()
    header, pycopy = gen.render(gen.build_table())
    assert open(gen.HEADER).read() == header
    assert open(gen.PYCOPY).read() == pycopy


def test_every_case_uses_exactly_its_sign_changing_edges():
    assert len(mc_table.TRIANGLES) == 256 and mc_table.MAX_TRIS == max(len(t) for t in mc_table.TRIANGLES)
    for case, tris in enumerate(mc_table.TRIANGLES):
        crossing = {e for e, (a, b) in enumerate(mc_table.EDGE_CORNERS) if ((case >> a) & 1) != ((case >> b) & 1)}
        used = {e for t in tris for e in t}
        assert used == crossing, case                       # every vertex on a crossing edge, every crossing edge used
        for t in tris:
            assert len(set(t)) == 3, (case, t)
    assert mc_table.TRIANGLES[0] == () and mc_table.TRIANGLES[255] == ()


def test_ambiguous_face_cuts_off_the_inside_corners():
    """Case 9: corners 0 and 3 inside, diagonal on the face axis 2 = 0.  The rule cuts each inside corner off: two separate
    triangles, each on the three edges that meet at its corner, and the outside corners stay connected.  The other
    rule would join the two into one piece.  Pinned here because a regenerated table passes the byte comparison."""
    assert mc_table.EDGE_CORNERS[0] == (0, 1) and (0, 3) not in mc_table.EDGE_CORNERS        # 0 and 3: a face diagonal
    at = lambda c: {e for e, p in enumerate(mc_table.EDGE_CORNERS) if c in p}              # noqa: E731
    assert sorted(map(sorted, map(set, mc_table.TRIANGLES[9]))) == sorted([sorted(at(0)), sorted(at(3))])
    verts, faces, _ = mo.marching_cubes(_embedded(9), 0.0)
    assert len(np.unique(mo.vertex_labels(len(verts), faces))) == 2                        # two bodies, not one
    outside = mo.marching_cubes(-_embedded(9)[1:3, 1:3, 1:3], 0.0)                          # the complement in one cell
    assert len(outside[1]) == 4 and len(np.unique(mo.vertex_labels(len(outside[0]), outside[1]))) == 1


def _embedded(case):
    vol = np.ones((4, 4, 4))
    for c in range(8):
        if (case >> c) & 1:
            vol[1 + (c & 1), 1 + ((c >> 1) & 1), 1 + ((c >> 2) & 1)] = -1.0
    return vol


def test_every_case_gives_a_closed_oriented_manifold():
    for case in range(1, 256):
        verts, faces, _ = mo.marching_cubes(_embedded(case), 0.0)
        assert len(faces) > 0, case
        assert mo.is_closed_oriented_manifold(faces), case
        assert mo.signed_volume(verts, faces) > 0, case      # normals towards increasing value: the inside is enclosed


@pytest.mark.parametrize("seed", range(24))
def test_random_sign_volumes_are_closed_oriented_manifolds(seed):
    """the only inputs where two ambiguous faces meet (and where a fan diagonal could lie in a shared face)"""
    rng = np.random.default_rng(seed)
    vol = np.ones((6, 5, 7))
    vol[1:-1, 1:-1, 1:-1] = rng.choice([-1.0, 1.0], size=(4, 3, 5))
    verts, faces, _ = mo.marching_cubes(vol, 0.0)
    assert mo.is_closed_oriented_manifold(faces)
    assert mo.signed_volume(verts, faces) > 0


# ---- grid axes ---------------------------------------------------------------------------------------------------------
def test_get_grid_uniform():
    g = mesh.get_grid_uniform(100, [-1.5, 1.5])
    assert g["shortest_axis_length"] == 2.0 and g["shortest_axis_index"] == 0
    for a in g["xyz"]:
        assert a.dtype == np.float64 and np.array_equal(a, np.linspace(-1.5, 1.5, 100))


@pytest.mark.parametrize("shortest", [0, 1, 2])
def test_get_grid_from_points_end_rule(shortest):
    """Binary fractions throughout, so every length is exact: the shortest axis spans [0,1], eps 1/8 and resolution 11 give
    a step of 1/8.  An axis spanning [0,2] runs from -1/8 up to, not including, 2 + 1/8 + 1/8: 19 nodes, the last at
    2 + 1/8 (18 without the extra step, 20 with an inclusive end).  An axis spanning [0, 1.5 + 2^-20] ends a hair later:
    one more node than [0, 1.5] would get."""
    import torch
    others = [a for a in range(3) if a != shortest]
    hi = np.zeros(3)
    hi[shortest], hi[others[0]], hi[others[1]] = 1.0, 2.0, 1.5 + 2.0 ** -20
    pts = torch.tensor(np.stack([np.zeros(3), hi]), dtype=torch.float32)
    g = mesh.get_grid(pts, 11, eps=0.125)
    assert g["shortest_axis_index"] == shortest and g["shortest_axis_length"] == 1.25
    assert np.array_equal(g["xyz"][shortest], np.linspace(-0.125, 1.125, 11))
    a = g["xyz"][others[0]]
    assert len(a) == 19 and a[0] == -0.125 and a[-1] == 2.125 and np.array_equal(a, -0.125 + 0.125 * np.arange(19))
    b = g["xyz"][others[1]]
    assert len(b) == 16 and b[-1] == 1.75
    assert len(mesh.get_grid(torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.5, 1.5]]), 11, eps=0.125)["xyz"][1]) == 15 or shortest != 0
    assert mesh.grid_spacing(g) == g["xyz"][0][2] - g["xyz"][0][1]


def test_get_grid_from_explicit_bounds_rounds_the_stop_to_float32():
    """With explicit bounds the reference holds float32 tensors: 1.5 + 2^-30 is 1.5 there, the stop is exactly 1.75 and the
    axis has 15 nodes; float64 arithmetic on the unrounded bound would give 16."""
    mn, mx = np.zeros(3), np.array([1.0, 2.0, 1.5 + 2.0 ** -30])
    g = mesh.get_grid(None, 11, input_min=mn - 0.0, input_max=mx, eps=0.125)
    assert g["shortest_axis_index"] == 0 and len(g["xyz"][1]) == 19 and len(g["xyz"][2]) == 15
    g0 = mesh.get_grid(None, 11, input_min=mn, input_max=mx, eps=0.0)        # the coarse grid of surface_by_grid
    assert np.array_equal(g0["xyz"][0], np.linspace(0.0, 1.0, 11))
    assert len(g0["xyz"][1]) == 21 and g0["xyz"][1][-1] == 2.0


# ---- box lookup, PLY -----------------------------------------------------------------------------------------------------
def test_dtu_box_lookup(tmp_path):
    os.makedirs(tmp_path / "DTU")
    boxes = {str(s): np.full((2, 3), float(s)) for s in (24, 83, 106)}
    np.savez(tmp_path / "DTU" / "bbs.npz", **boxes)
    assert [scans.dtu_box_scan(s) for s in (82, 21, 34, 38, 24, 83, 106)] == [83, 24, 24, 24, 24, 83, 106]
    for scan, want in ((82, 83), (21, 24), (34, 24), (38, 24), (106, 106), (83, 83)):
        assert np.array_equal(scans.dtu_box(str(tmp_path), scan), boxes[str(want)])
    with pytest.raises(LookupError):
        scans.dtu_box(str(tmp_path), 55)


def test_ply_mesh_round_trip(tmp_path):
    from svs_hip.ply import read_mesh
    rng = np.random.default_rng(3)
    verts = rng.standard_normal((37, 3)).astype(np.float32)
    faces = rng.integers(0, 37, size=(51, 3)).astype(np.int32)
    fn = str(tmp_path / "m.ply")
    ply.write(fn, verts, faces=faces)
    v, f = read_mesh(fn)
    assert v.dtype == np.float64 and np.array_equal(v, verts.astype(np.float64))
    assert np.array_equal(f, faces.astype(np.int64))
    head = open(fn, "rb").read(400).split(b"end_header\n")[0].decode("ascii")
    assert "format binary_little_endian 1.0" in head and "property list uchar int vertex_indices" in head
    assert "nx" not in head
    assert os.path.getsize(fn) == len(head) + len("end_header\n") + 37 * 12 + 51 * 13


def test_oracle_clip_and_components_on_a_known_mesh():
    """the oracle's own pieces on a tetrahedron pair: two components, and a cut that leaves boundary edges on the plane"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    verts = np.concatenate([v, 3 * v + 5])
    faces = np.concatenate([f, f + 4])
    assert mo.vertex_labels(8, faces).tolist() == [0, 0, 0, 0, 4, 4, 4, 4]
    assert set(mo.largest_component_faces(verts, faces).tolist()) == {4, 5, 6, 7}
    cv, cf = mo.clip_halfspace(v, f, [0.25, 0, 0], [1, 0, 0])
    assert (cv[:, 0] >= 0.25 - 1e-15).all() and len(cf) == 3
    for a, b in mo.boundary_edges(cf):
        assert abs(cv[a, 0] - 0.25) < 1e-15 and abs(cv[b, 0] - 0.25) < 1e-15
