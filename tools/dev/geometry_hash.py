"""tools/dev/geometry_hash.py: SHA-256 of every output array of the geometry units that share the sorted-run headers
(svs_meshsmooth.hip, svs_meshsimplify.hip, svs_poisson.hip, svs_cloud.hip, svs_cloudknn.hip), on seeded inputs from the tests'
oracle modules -- two builds of the library that claim the same bytes (SVS_LIB_PATH selects one) must print the same lines.
Dev aid in the manner of det_hash.py, GPU only."""
import hashlib, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "s-volsdf_amd"), os.path.join(ROOT, "tests")]
import cloudclean_oracle as co                                           # noqa: E402
import meshsimplify_oracle as so                                         # noqa: E402
import meshsmooth_oracle as mo                                           # noqa: E402
import poisson_oracle as po                                              # noqa: E402
from svs_hip import clouds, lib as _lib, meshsimplify, meshsmooth, poisson   # noqa: E402


def sha(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return f"{hashlib.sha256(a.tobytes()).hexdigest()[:16]}{list(a.shape)}"


def line(what, named):
    print(what + ": " + " ".join(f"{k} {sha(v) if hasattr(v, 'shape') else v}" for k, v in named))


L = _lib.load()
print("library:", os.environ.get("SVS_LIB_PATH", "(default)"))
print("bytes: " + " ".join(f"cloud_grid({n}) {L.svs_cloud_grid_bytes(n)}" for n in (0, 1, 2049, 1 << 20, 10_000_000)))

for name, (v, f) in (("bad_input", mo.bad_input()[:2]), ("icosphere3", mo.icosphere(3))):
    tv, tf = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    adj = meshsmooth.adjacency(tv, tf)
    line(f"adjacency {name}", [(k, adj[k]) for k in ("nbr_start", "nbr", "nbr_boundary", "face_start", "vert_face", "face_valid", "flags")]
         + [("counts", sorted(adj["counts"].items()))])
    for boundary in ("fixed", "curve", "free"):
        line(f"taubin {name} {boundary}", [("verts", meshsmooth.taubin(tv, tf, iters=3, boundary=boundary, adj=adj)[0])])
    for boundary in ("fixed", "free"):
        line(f"denoise {name} {boundary}", [("verts", meshsmooth.denoise(tv, tf, normal_iters=3, vertex_iters=3, boundary=boundary, adj=adj)[0])])

for name in ("sphere_0.3", "fan_4097"):
    v, f, h, o = so.case(name)
    col = np.random.default_rng(1).integers(0, 256, (len(v), 3)).astype(np.uint8)
    ov, of, oc, info = meshsimplify.cluster(v, f, h, origin=o, colors=col, return_info=True)
    line(f"cluster {name}", [("verts", ov), ("faces", of), ("colors", oc), ("vert_cell", info["vert_cell"]), ("info", info["info"]),
                             ("err", info["err"])])

for name in ("7x6x13", "segment"):
    pts, nrm, dims, origin, h = po.segment_case() if name == "segment" else po.splat_case(name)
    field, counted, skipped = poisson.splat(pts, nrm, dims, origin, h)
    line(f"splat {name}", [("field", field), ("counted", counted), ("skipped", skipped)])

pts = torch.from_numpy(co.random_cloud(2049, 0)).cuda()
for excl in (False, True):
    dist, idx, mean = clouds.knn(pts, pts, 20, 1e9, exclude_same_index=excl, return_mean=True)
    line(f"knn 2049 exclude_same_index={excl}", [("dist", dist), ("idx", idx), ("mean", mean)])
q = torch.from_numpy(co.random_cloud(303, 1, scale=1.3)).cuda()
dist, idx = clouds.nearest_neighbor(pts, q, 0.5, return_index=True)
line("nearest_neighbor 2049 <- 303", [("dist", dist), ("idx", idx)])
for radius in (0.05, 0.2):
    line(f"radius_downsample 2049 r={radius}", [("keep", clouds.radius_downsample(pts, radius).to(torch.uint8))])
torch.cuda.synchronize()
