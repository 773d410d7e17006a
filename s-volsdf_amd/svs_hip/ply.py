"""Every PLY byte this project reads or writes: one header parser, the point and mesh readers the Chamfer evaluators take
their clouds from (what open3d.io.read_point_cloud / read_triangle_mesh give the reference, evals/eval_dtu.py:65-68,96-97,
139-140), and the one writer behind the fused cloud (runner.py:389-400 through plyfile), the error clouds
(evals/eval_bmvs.py:241,246), the meshes of `svs_hip.mesh` and `svs_hip.tsdf` and the cleaned cloud with normals of
`svs_hip.cloudclean`.  Host code only.
"""
import numpy as np
import torch

_PLY_TYPES = {"float": "f4", "float32": "f4", "double": "f8", "float64": "f8", "uchar": "u1", "uint8": "u1", "char": "i1",
              "int8": "i1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4",
              "uint": "u4", "uint32": "u4"}
_ORDER = {"binary_little_endian": "<", "binary_big_endian": ">", "ascii": None}
_RGB = ("red", "green", "blue")


def read_header(fh):
    """fh: a file opened in binary mode, at its start; left at the first byte after the header.  -> (format, elements),
    elements: [[name, count, properties], ...] in file order, a property (name, type) or, for a list, (name, count type,
    item type) in numpy's type codes.  `comment` and `obj_info` lines are skipped.  ValueError for a file that does not
    start with `ply`, a header without end_header, or a format other than ascii / binary_little_endian / binary_big_endian."""
    if fh.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    fmt, elements = None, []
    while True:
        line = fh.readline()
        if not line:
            raise ValueError("PLY header without end_header")
        tok = line.decode("ascii").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]) if tok[1] == "list"
                                   else (tok[2], _PLY_TYPES[tok[1]]))
        elif tok[0] == "end_header":
            break
    if fmt not in _ORDER:
        raise ValueError(f"PLY format {fmt!r}: only {', '.join(_ORDER)}")
    return fmt, elements


def _columns(fh, fmt, n, props):
    """the n records of an element without list properties -> {property name: column}"""
    if fmt == "ascii":
        rows = np.loadtxt(fh, max_rows=n, ndmin=2) if n else np.zeros((0, len(props)))
        return {q[0]: rows[:, i] for i, q in enumerate(props)}
    rec = np.fromfile(fh, dtype=[(q[0], _ORDER[fmt] + q[1]) for q in props], count=n)
    return {q[0]: rec[q[0]] for q in props}


def _lists(fh, fmt, n, props, want):
    """the n records of an element with list properties, record by record -> the lists of the properties named in `want`
    as triangles, fanned around their first item; every other property is stepped over"""
    order, out = _ORDER[fmt], []
    for _ in range(n):
        if fmt == "ascii":
            tok = fh.readline().split()
            at = 0
        for q in props:
            if len(q) == 2:
                if fmt == "ascii":
                    at += 1
                else:
                    fh.read(np.dtype(q[1]).itemsize)
                continue
            if fmt == "ascii":
                k = int(tok[at]); items = [int(float(v)) for v in tok[at + 1:at + 1 + k]]; at += 1 + k
            else:
                k = int(np.frombuffer(fh.read(np.dtype(q[1]).itemsize), order + q[1])[0])
                items = np.frombuffer(fh.read(k * np.dtype(q[2]).itemsize), order + q[2]).astype(np.int64).tolist()
            if q[0] in want:
                out.extend((items[0], items[i], items[i + 1]) for i in range(1, k - 1))
    return out


def _read(filename, faces):
    """walks the elements in file order, as far as the vertices (and, with faces, to the end) -> (vertex columns, triangles);
    ValueError for a file without a vertex element or with a list property inside it"""
    with open(filename, "rb") as fh:
        fmt, elements = read_header(fh)
        cols, tris = None, []
        for name, n, props in elements:
            if any(len(q) == 3 for q in props):
                if name == "vertex":
                    raise ValueError("list property in the vertex element")
                tris += _lists(fh, fmt, n, props, ("vertex_indices", "vertex_index") if faces and name == "face" else ())
                continue
            got = _columns(fh, fmt, n, props)
            if name == "vertex":
                cols = got
                if not faces:
                    break
    if cols is None:
        raise ValueError("PLY file without a vertex element")
    return cols, tris


def read_points(filename):
    """-> (xyz (n,3) float64, rgb (n,3) uint8 or None): the vertex element of an ascii / binary PLY, wherever it stands
    among the elements.  ValueError for a list property in the vertex element."""
    cols, _ = _read(filename, faces=False)
    pts = np.stack([np.asarray(cols[k], np.float64) for k in "xyz"], 1)
    rgb = np.stack([np.asarray(cols[k], np.uint8) for k in _RGB], 1) if "red" in cols else None
    return pts, rgb


def read_point_normals(filename):
    """-> (n,3) float32: the nx, ny, nz of the vertex element, or None for a file without them"""
    cols, _ = _read(filename, faces=False)
    if not all("n" + k in cols for k in "xyz"):
        return None
    return np.stack([np.asarray(cols["n" + k], np.float32) for k in "xyz"], 1)


def read_mesh(filename):
    """-> (vertices (n,3) float64, triangles (m,3) int64) of an ascii / binary PLY with a face element whose list property
    is vertex_indices or vertex_index.  Faces with more than three corners are fanned around their first corner, as
    open3d's reader does.  ValueError for a file without a vertex element."""
    cols, tris = _read(filename, faces=True)
    vertices = np.stack([np.asarray(cols[k], np.float64) for k in "xyz"], 1)
    return vertices, np.asarray(tris, np.int64).reshape(-1, 3)


def read_mesh_colors(filename):
    """-> `read_mesh`'s vertices and triangles, and `read_points`' rgb (n,3) uint8 or None"""
    return read_mesh(filename) + (read_points(filename)[1],)


def _host(a, dtype):
    return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype).reshape(-1, 3)


def write(filename, xyz, rgb=None, faces=None, coords="float", normals=None):
    """Binary little-endian PLY.  xyz (n,3) as `coords` ("float" or "double") x, y, z; normals: optional (n,3), float nx,
    ny, nz after them (the order MeshLab and Open3D read); rgb: optional (n,3), uchar red, green, blue last (ValueError when
    either count differs from the vertices'); faces: optional (m,3), a second element of `list uchar int vertex_indices`
    records (as trimesh's export).  Arrays, host or device tensors.  A float cloud with colours is the file of
    runner.py:389-400, a double one the error cloud of both evaluators, one with normals the cleaned cloud of
    `svs_hip.cloudclean`."""
    t = {"float": "<f4", "double": "<f8"}.get(coords)
    if t is None:
        raise ValueError(f"coords: 'float' or 'double', got {coords!r}")
    v = np.ascontiguousarray(_host(xyz, t))
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v) + "".join(f"property {coords} {k}\n" for k in "xyz")
    fields, cols = [("p", t, (3,))], [v]
    if normals is not None:
        nrm = _host(normals, "<f4")
        if len(nrm) != len(v):
            raise ValueError(f"{len(nrm)} normals for {len(v)} vertices")
        fields.append(("n", "<f4", (3,))); cols.append(nrm)
        head += "".join(f"property float n{k}\n" for k in "xyz")
    if rgb is not None:
        c = _host(rgb, np.uint8)
        if len(c) != len(v):
            raise ValueError(f"{len(c)} colours for {len(v)} vertices")
        fields.append(("c", "u1", (3,))); cols.append(c)
        head += "".join(f"property uchar {k}\n" for k in _RGB)
    if len(fields) > 1:
        rec = np.empty(len(v), dtype=fields)
        for f_, col in zip(fields, cols):
            rec[f_[0]] = col
        v = rec
    if faces is not None:
        f = _host(faces, None)
        corner = np.empty(len(f), dtype=[("n", "u1"), ("v", "<i4", (3,))])
        corner["n"], corner["v"] = 3, f
        head += "element face %d\nproperty list uchar int vertex_indices\n" % len(f)
    with open(filename, "wb") as fh:
        fh.write((head + "end_header\n").encode("ascii"))
        v.tofile(fh)
        if faces is not None:
            corner.tofile(fh)
