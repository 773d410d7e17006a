"""Every OBJ / MTL byte this project reads or writes, as `ply.py` holds every PLY byte: the textured mesh of
`svs_hip.meshtexture` as three files, the mesh with its texture coordinates (.obj), its one material (.mtl) and the atlas
(.png).  Host code only.
"""
import os

import numpy as np
import torch

MATERIAL = "atlas"


def _host(a, dtype=None):
    return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype)


def _names(path):
    if not path.lower().endswith(".obj"):
        raise ValueError(f"an OBJ file's name ends in .obj, got {path!r}")
    return path[:-4] + ".mtl", path[:-4] + ".png"


def write(path, verts, faces, uv, chart, atlas):
    """verts (V,3), faces (F,3), uv (F,3,2) per face corner in the OBJ convention, chart (F,) (a face with chart -1 has no
    place in the atlas and is left out), atlas (S,S,3) uint8 with row 0 on top: arrays, host or device tensors.  Writes
    `path` (mtllib, every vertex as `v` in %.9g, three `vt` in %.9g per written face, usemtl, `f a/ta b/tb c/tc` 1-based with
    ta = 3 f' + k + 1 for corner k of the f'-th written face), path[:-4] + ".mtl" (one material whose map_Kd names the
    picture) and path[:-4] + ".png".  -> the number of faces left out"""
    mtl, png = _names(path)
    from PIL import Image
    verts = _host(verts, np.float64).reshape(-1, 3)
    faces = _host(faces, np.int64).reshape(-1, 3)
    uv = _host(uv, np.float64).reshape(-1, 3, 2)
    chart = _host(chart, np.int64).reshape(-1)
    atlas = np.ascontiguousarray(_host(atlas, np.uint8))
    if not (len(faces) == len(uv) == len(chart)) or atlas.ndim != 3 or atlas.shape[2] != 3:
        raise ValueError(f"obj.write: {len(faces)} faces, {len(uv)} uv triples, {len(chart)} charts, an atlas of {atlas.shape}")
    keep = chart >= 0
    f, t = faces[keep] + 1, uv[keep].reshape(-1, 2)
    ta = np.arange(1, 3 * len(f) + 1, dtype=np.int64).reshape(-1, 3)
    lines = [f"mtllib {os.path.basename(mtl)}\n"]
    lines += ["v %.9g %.9g %.9g\n" % tuple(p) for p in verts]
    lines += ["vt %.9g %.9g\n" % tuple(p) for p in t]
    lines.append(f"usemtl {MATERIAL}\n")
    lines += ["f %d/%d %d/%d %d/%d\n" % (a[0], b[0], a[1], b[1], a[2], b[2]) for a, b in zip(f, ta)]
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w", encoding="ascii", newline="\n") as fh:
        fh.writelines(lines)
    with open(mtl, "w", encoding="ascii", newline="\n") as fh:
        fh.write(f"newmtl {MATERIAL}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {os.path.basename(png)}\n")
    Image.fromarray(atlas).save(png, compress_level=1)
    return int((~keep).sum())


def read(path):
    """What `write` wrote -> dict(verts (V,3) float64, faces (F',3) int64 0-based, uv (F',3,2) float64 per face corner,
    atlas (S,S,3) uint8, mtl, png: the two other files' names).  ValueError for a face without texture coordinates."""
    from PIL import Image
    verts, vt, faces, ft, mtllib = [], [], [], [], None
    with open(path, "r", encoding="ascii") as fh:
        for line in fh:
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if tok[0] == "v":
                verts.append([float(x) for x in tok[1:4]])
            elif tok[0] == "vt":
                vt.append([float(x) for x in tok[1:3]])
            elif tok[0] == "f":
                pairs = [x.split("/") for x in tok[1:4]]
                if any(len(q) < 2 or not q[1] for q in pairs):
                    raise ValueError(f"{path}: a face without texture coordinates: {line.strip()!r}")
                faces.append([int(q[0]) - 1 for q in pairs])
                ft.append([int(q[1]) - 1 for q in pairs])
            elif tok[0] == "mtllib":
                mtllib = tok[1]
    folder = os.path.dirname(path)
    mtl = os.path.join(folder, mtllib) if mtllib else None
    png = None
    if mtl:
        with open(mtl, "r", encoding="ascii") as fh:
            for line in fh:
                tok = line.split()
                if tok and tok[0] == "map_Kd":
                    png = os.path.join(folder, tok[1])
    vt = np.asarray(vt, np.float64).reshape(-1, 2)
    ft = np.asarray(ft, np.int64).reshape(-1, 3)
    atlas = np.asarray(Image.open(png).convert("RGB"), np.uint8) if png else None
    return dict(verts=np.asarray(verts, np.float64).reshape(-1, 3), faces=np.asarray(faces, np.int64).reshape(-1, 3),
                uv=vt[ft] if len(ft) else np.zeros((0, 3, 2)), atlas=atlas, mtl=mtl, png=png)
