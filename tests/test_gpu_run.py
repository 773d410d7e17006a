"""svs_hip.run on the GPU: the order statistics and colour previews of csrc/svs_preview.hip, `mvsout.save_view(previews=
True)`, and `run.main` end to end on a toy DTU scan.

Selection is compared with np.sort bit for bit.  One exception is forced by np.sort itself: it orders by `<`, so where
-0.0 and +0.0 both occur it places them as its algorithm happens to (checked: not by sign); the kernel's order is total,
-0.0 before +0.0.  A zero is therefore compared with np.sort as a zero, and its sign against the total order
(run_oracle.key_order), which is bit for bit np.sort everywhere else (tests/test_run_cpu.py).

The end-to-end scan runs at max_h=96 max_w=128 with the reference's ndepths, as run_help insists.  Its depth maps are
1152x1536, not 192x256: with x2_mvsres (which run_help also insists on) the MVS loader's second resize always ends at
1152x1536 (datasets/general_eval.py:226-229), whatever max_h / max_w are; 96x128 only makes the first resize land on
img_res.  The run is made once per module and shared.
"""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

import run_oracle as ro
import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPAN = 4096                                                  # elements per workgroup of the counting kernel


# ---- selection ---------------------------------------------------------------------------------------------------------------
def select_inputs(n, seed):
    rng = np.random.default_rng(seed)
    out = {"uniform": rng.uniform(425.0, 935.0, n).astype(F32),
           "constant": np.full(n, 0.37, F32),
           "two_values": rng.choice(F32([1.5, -2.25]), n, p=[0.9, 0.1]).astype(F32),
           "mixed_zeros": (rng.normal(0, 1, n) * rng.integers(0, 2, n)).astype(F32) * rng.choice(F32([1, -1]), n),
           "denormals": (rng.integers(-2000, 2000, n).astype(np.int32).astype(np.float64) * 1.4e-45).astype(F32),
           "with_inf": rng.normal(0, 1e3, n).astype(F32), "one_nan": rng.normal(5, 1, n).astype(F32)}
    out["with_inf"][rng.integers(0, n, max(n // 7, 1))] = np.inf
    out["one_nan"][rng.integers(0, n)] = np.nan
    return out


def check_pairs(a, ranks, what):
    from svs_hip import mvsout
    n = a.size
    pairs, counts = mvsout.select_sorted_pairs(torch.from_numpy(a).cuda(), ranks)
    srt, total = np.sort(a), ro.key_order(a)
    idx = np.array([[k, min(k + 1, n - 1)] for k in ranks])
    assert pairs.dtype == F32 and pairs.shape == (len(ranks), 2)
    assert ro.same_bits(pairs, srt[idx]), (what, ranks, pairs, srt[idx])
    want = total[idx]
    exact = pairs.view(np.uint32) == want.view(np.uint32)
    assert np.all(exact | (np.isnan(pairs) & np.isnan(want))), (what, ranks, pairs, want)        # the signs of the zeros too
    assert counts == dict(nan=int(np.isnan(a).sum()), posinf=int(np.isposinf(a).sum()), neginf=int(np.isneginf(a).sum())), what


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, SPAN - 1, SPAN, SPAN + 1, 70001])
def test_select_is_np_sort(n):
    from svs_hip import mvsout
    for name, a in select_inputs(n, 100 + n).items():
        k01 = int(np.floor(0.01 * (n - 1)))
        for ranks in ([0], [n - 1], [k01], [0, n - 1, k01, (n - 1) // 2]):
            check_pairs(a, ranks, (name, n))
        d = torch.from_numpy(a).cuda()
        with np.errstate(invalid="ignore"):
            for q in (0.01, 0.5, 1.0):
                got, want = mvsout.quantile(d, q), np.quantile(a, q)
                assert got.dtype == F32 and ro.same_bits(got, want), (name, n, q, got, want)
            for p in (5, 95):
                got, want = mvsout.percentile(d, p), np.percentile(a, p)
                assert ro.same_bits(got, want), (name, n, p, got, want)
    one_nan = select_inputs(n, 100 + n)["one_nan"]
    assert np.isnan(mvsout.quantile(torch.from_numpy(one_nan).cuda(), 0.01))


def test_select_is_the_same_every_time_and_checks_its_arguments():
    from svs_hip import mvsout
    a = select_inputs(70001, 3)["mixed_zeros"]
    d = torch.from_numpy(a).cuda()
    first = mvsout.select_sorted_pairs(d, [5, 700, 35000, 70000])[0]
    for _ in range(3):
        assert np.array_equal(mvsout.select_sorted_pairs(d, [5, 700, 35000, 70000])[0].view(np.uint32), first.view(np.uint32))
    n0 = mvsout.LAUNCHES["select"]
    mvsout.quantile(d.reshape(1, 70001), [0.01, 0.05, 0.95])              # any shape; all ranks share one call
    assert mvsout.LAUNCHES["select"] == n0 + 1
    with pytest.raises(ValueError):
        mvsout.select_sorted_pairs(d, [70001])
    with pytest.raises(ValueError):
        mvsout.select_sorted_pairs(d, [0, 1, 2, 3, 4])
    with pytest.raises(TypeError):
        mvsout.select_sorted_pairs(d.double(), [0])


# ---- previews ------------------------------------------------------------------------------------------------------------------
def test_depth_preview_is_the_references_function():
    from svs_hip import mvsout
    g = np.load(os.path.join(GOLDEN, "depth_preview.npz"))
    table = g["table"]
    names = sorted({k.rsplit("/", 1)[0] for k in g.files if "/" in k})
    assert len(names) == 16
    for key in names:
        depth, direct = g[f"{key}/depth"], bool(g[f"{key}/direct"])
        lo, hi = g[f"{key}/lo"], g[f"{key}/hi"]
        if np.isnan(lo):                                    # None bounds: the 5th / 95th percentile of the valid pixels
            lo, hi = mvsout.percentile(torch.from_numpy(depth).cuda(), [5, 95], valid_only=True)
            valid = depth[np.isfinite(depth)]
            assert lo.view(np.uint32) == np.percentile(valid, 5).view(np.uint32)
            assert hi.view(np.uint32) == np.percentile(valid, 95).view(np.uint32)
        got = mvsout.depth_preview([depth], lo, hi, direct=direct, table=table)[0].cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, g[f"{key}/out"]), key


def test_depth_preview_many_maps_and_degenerate_bounds():
    from svs_hip import mvsout
    rng = np.random.default_rng(4)
    table = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    maps = [rng.uniform(400, 950, s).astype(F32) for s in ((37, 53), (9, 13), (1, 300))]
    maps[1][2, 3], maps[2][0, 7] = np.nan, np.inf
    n0 = mvsout.LAUNCHES["preview"]
    for direct in (False, True):
        outs = mvsout.depth_preview([torch.from_numpy(m).cuda() for m in maps], F32(425.5), F32(930.25), direct=direct, table=table)
        for m, o in zip(maps, outs):
            assert np.array_equal(o.cpu().numpy(), ro.visualize_depth(m, 425.5, 930.25, direct=direct, table=table))
    assert mvsout.LAUNCHES["preview"] == n0 + 2              # one launch for the three maps
    for lo, hi in ((5.0, 5.0), (7.0, 5.0), (np.nan, 5.0), (5.0, np.nan)):
        for direct in (False, True):
            out = mvsout.depth_preview([maps[0]], lo, hi, direct=direct, table=table)[0]
            assert out.shape == maps[0].shape + (() if direct else (3,)) and not bool(out.any())
    jet = mvsout.jet_table()
    if jet is not None:                                      # matplotlib's jet: blue end for far (code 0 -> row 255 is red)
        assert jet.shape == (256, 3) and jet.dtype == np.uint8 and jet[0, 2] > jet[0, 0] and jet[255, 0] > jet[255, 2]


# ---- save_view -----------------------------------------------------------------------------------------------------------------
def toy_cascade(ndepths, ratios):
    from models.CasMVSNet import CascadeMVSNet
    model = CascadeMVSNet(refine=False, ndepths=ndepths, depth_interals_ratio=ratios, share_cr=False, cr_base_chs=[8, 8, 8],
                          grad_method="detach")
    model.feature.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_featurenet_params(3).items()})
    for st, cin in enumerate((32, 16, 8)):
        model.cost_regularization[st].load_state_dict(
            {k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_costreg_params(50 + st, cin).items()})
    return model


def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def check_previews(names, dep_max, table):
    """the four PNGs against the numpy restatement applied to the PFMs read back (and, for the two coarser stages, to
    the maps handed in)"""
    from datasets.data_io import read_pfm
    depth, conf = (np.ascontiguousarray(read_pfm(names[k])[0]) for k in ("depth_est", "confidence"))
    lo = np.quantile(depth, 0.01)
    assert np.array_equal(read_png(names["depth_png"]), ro.visualize_depth(depth, lo, F32(dep_max), table=table))
    assert np.array_equal(read_png(names["confidence_png"]), ro.visualize_depth(conf, direct=True))
    return depth, conf, lo


def test_save_view_with_previews(tmp_path):
    from svs_hip import mvsout
    from svs_hip.stage_loop import StageLoop
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    G = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    model = toy_cascade([16, 8, 8], [4.0, 2.0, 1.0]).to(dev).eval()
    H, W = 64, 96
    rng = np.random.default_rng(1)
    _, proj, depth_values = synth.make_mvs_sample(11, img_hw=(H, W), numdepth=16)
    sample = dict(imgs=G(rng.uniform(0, 1, (1, 3, 3, H, W)).astype(F32)), depth_values=G(depth_values)[None],
                  proj_matrices={k: G(v)[None] for k, v in proj.items()}, filename=["scan24/{}/00000007{}"])
    loop = StageLoop(model)
    outs, extra = [None], [None]
    for stage in range(3):
        outs, extra = loop.cost_volumes(stage, [sample], outs, extra)
    outputs = outs[0]
    assert outputs["depth"].shape == (1, H, W) and outputs["stage1"]["depth"].shape == (1, 16, 24)
    table = np.random.default_rng(8).integers(0, 256, (256, 3), dtype=np.uint8)
    dep_max = float(sample["depth_values"].max())
    before, down = dict(mvsout.LAUNCHES), dict(mvsout.BYTES_DOWN)
    names = mvsout.save_view(str(tmp_path), 7, outputs, sample["proj_matrices"]["stage3"][0, 0], sample["imgs"][0, 0],
                             previews=True, dep_max=dep_max, table=table)
    # no per-pixel work left to torch: one confidence launch, two selections (depth; confidence), two preview launches
    delta = {k: mvsout.LAUNCHES[k] - before[k] for k in before}
    assert delta == dict(dilate=0, resize=0, confidence=1, select=2, preview=2), delta
    moved = {k: mvsout.BYTES_DOWN[k] - down[k] for k in down}
    assert moved == dict(select=2 * 48, maps=2 * 4 * H * W, previews=3 * H * W + 3 * 16 * 24 + 3 * 32 * 48 + H * W), moved
    assert sorted(os.listdir(tmp_path / "depth_est")) == ["00000007.pfm", "00000007.png", "00000007_1.png", "00000007_2.png"]
    assert sorted(os.listdir(tmp_path / "confidence")) == ["00000007.pfm", "00000007_final.png"]
    depth, conf, lo = check_previews(names, dep_max, table)
    assert np.array_equal(depth, outputs["depth"][0].cpu().numpy())
    assert np.array_equal(conf, mvsout.final_confidence(outputs).cpu().numpy())
    for k, st in (("depth_1_png", "stage1"), ("depth_2_png", "stage2")):
        want = ro.visualize_depth(outputs[st]["depth"][0].cpu().numpy(), lo, F32(dep_max), table=table)
        assert np.array_equal(read_png(names[k]), want), k
    # previews=False: today's files and nothing else
    names0 = mvsout.save_view(str(tmp_path / "plain"), 7, outputs, sample["proj_matrices"]["stage3"][0, 0], sample["imgs"][0, 0])
    assert sorted(names0) == ["cams", "confidence", "depth_est", "images"]
    assert sorted(os.listdir(tmp_path / "plain" / "depth_est")) == ["00000007.pfm"]
    for k in ("depth_est", "confidence"):
        assert open(names0[k], "rb").read() == open(names[k], "rb").read()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
VIEWS = (25, 22, 28)
OVERRIDES = ["testlist=scan106", "max_h=96", "max_w=128", "opt_stepNs=[6,0,0]", "filter_dist=10000", "filter_diff=10000",
             "ndepths=192,32,8", "depth_inter_r=1,0.5,0.5"]


def write_toy_root(root):
    import mvsdata_oracle as mo
    import scene_oracle as so
    from PIL import Image
    mo.write_mvs_scan(str(root), "DTU", 106, 49, (120, 160), {25: [22, 28], 22: [25, 28], 28: [22, 25]}, seed=2)
    mdir = root / "DTU" / "eval_mask" / "scan106" / "mask"
    os.makedirs(mdir, exist_ok=True)
    for v in range(49):                                      # (the scene loader reads the masks of the evaluation views too)
        m = np.roll(so.synthetic_mask(120, 160), 2 * v, axis=1)
        Image.fromarray(np.repeat((m * 255)[..., None], 3, 2).astype(np.uint8)).save(mdir / f"{v:03d}.png")
    os.makedirs(root / "mvs_models")
    torch.save({"model": toy_cascade([192, 32, 8], [1.0, 0.5, 0.5]).state_dict()}, root / "mvs_models" / "casmvsnet.ckpt")


def run_main(root, out, extra=()):
    from svs_hip import run
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = run.main(OVERRIDES + [f"data_dir_root={root}", f"outdir={out}", f"exps_folder={root / 'exps'}"] + list(extra))
    return res, text.getvalue()


@pytest.fixture(scope="module")
def scan_run(tmp_path_factory):
    root = tmp_path_factory.mktemp("run_root")
    torch.manual_seed(0)
    write_toy_root(root)
    out = root / "out"
    res, text = run_main(root, out)
    return dict(root=root, out=out, res=res, text=text)


def view_files(out):
    files = []
    for v in VIEWS:
        files += [f"depth_est/{v:08}.pfm", f"depth_est/{v:08}.png", f"depth_est/{v:08}_1.png", f"depth_est/{v:08}_2.png",
                  f"confidence/{v:08}.pfm", f"confidence/{v:08}_final.png", f"cams/{v:08}_cam.txt", f"images/{v:08}.jpg"]
    return sorted(files)


def listed(folder, subs):
    return sorted(f"{s}/{f}" for s in subs for f in os.listdir(os.path.join(folder, s)))


def test_run_main_writes_the_scan(scan_run):
    from datasets.data_io import read_pfm
    from svs_hip import mvsout
    from svs_hip.ply import read_points
    out, res, text = scan_run["out"], scan_run["res"], scan_run["text"]
    assert sorted(os.listdir(out)) == ["all_scans.yaml", "mvsnet106_l3.ply", "scan106"]
    scan = out / "scan106"
    assert sorted(os.listdir(scan)) == ["args.yaml", "cams", "confidence", "depth_est", "images", "mask"]
    assert listed(scan, ("depth_est", "confidence", "cams", "images")) == view_files(out)
    assert sorted(os.listdir(scan / "mask")) == sorted(f"{v:08}_{t}.png" for v in VIEWS for t in ("photo", "geo", "final"))
    import yaml
    with open(scan / "args.yaml") as f:
        saved = yaml.safe_load(f)
    assert saved["max_h"] == 96 and saved["vol"]["dataset"]["img_res"] == [96, 128] and saved["opt_stepNs"] == [6, 0, 0]
    one = res["scans"]["scan106"]
    assert one["loop"].feature_calls == 3 and one["vol_opt"].iter_step >= 6
    # x2_mvsres ends at 1152x1536 whatever max_h / max_w are (see the module's docstring)
    jet = mvsout.jet_table()
    for v, names in zip(VIEWS, one["files"]):
        depth = read_pfm(names["depth_est"])[0]
        assert depth.shape == (1152, 1536) and depth.dtype == F32 and np.isfinite(depth).all()
        assert read_pfm(names["confidence"])[0].shape == (1152, 1536)
        assert read_png(names["images"]).shape == (1152, 1536, 3)
        if jet is not None:
            # the sample's depth_values (general_eval.py:256-258 for DTU: 425 + 2.5 * interval_scale * k)
            dep_max = np.arange(425, 2.5 * 1.06 * (192 - 0.5) + 425, 2.5 * 1.06, dtype=F32).max()
            check_previews(names, dep_max, jet)
            # stage 1's depth is the volume-rendered one that was handed off, at img_res; stage 2's is the network's
            assert read_png(names["depth_1_png"]).shape == (96, 128, 3) and read_png(names["depth_2_png"]).shape == (576, 768, 3)
    # the console: the reference's lines and the seconds per phase
    assert "parameter adjust - scan106" in text and "loading model casmvsnet" in text and "gpu -> auto" in text
    assert text.count("photo/geo/final-mask:") == 3 and "mvs_depth replaced by vol_depth at stg=0 in 0,1,2" in text
    m = re.search(r"scan106 seconds: load ([\d.]+), mvs0 ([\d.]+), mvs1 ([\d.]+), mvs2 ([\d.]+), optimise ([\d.]+), "
                  r"render ([\d.]+), save ([\d.]+), fusion ([\d.]+)", text)
    assert m and all(float(x) > 0 for x in m.groups()), text[-600:]
    xyz, rgb, stats = res["clouds"]["scan106"]
    pts, col = read_points(str(out / "mvsnet106_l3.ply"))
    print(f"points {len(xyz)}, masks {stats}")
    assert len(stats) == 3 and pts.shape[0] == xyz.shape[0] > 0 and rgb.shape == xyz.shape


def test_filter_only_leaves_the_maps_and_fuses_the_same_cloud(scan_run):
    from svs_hip.ply import read_points
    out = scan_run["out"]
    ply = str(out / "mvsnet106_l3.ply")
    pfms = [out / "scan106" / f for f in view_files(out) if f.endswith(".pfm")]
    before = {p: (os.stat(p).st_mtime_ns, open(p, "rb").read()) for p in pfms}
    pts0, col0 = read_points(ply)
    os.remove(ply)
    res, text = run_main(scan_run["root"], out, ["filter_only=true"])
    assert res["scans"] == {} and "loading model" not in text and text.count("photo/geo/final-mask:") == 3
    assert {p: (os.stat(p).st_mtime_ns, open(p, "rb").read()) for p in pfms} == before
    pts1, col1 = read_points(ply)
    # The fusion's order is fixed -- views in trains_i order, the surviving pixels of a view in row-major order
    # (svs_fuse_points compacts by a prefix sum over the mask, not by arrival) -- so the files would compare equal as they
    # are; sorted rows keep this test about the points, not about that order.
    rows0 = np.concatenate([pts0, col0.astype(np.float64)], 1)
    rows1 = np.concatenate([pts1, col1.astype(np.float64)], 1)
    assert rows0.shape == rows1.shape and rows0.shape[0] > 0
    assert np.array_equal(rows0[np.lexsort(rows0.T[::-1])], rows1[np.lexsort(rows1.T[::-1])])


def test_ablate_runs_mvs_only(scan_run):
    out = scan_run["root"] / "out_ablate"
    res, text = run_main(scan_run["root"], out, ["ablate=true"])
    one = res["scans"]["scan106"]
    assert one["vol_opt"] is None and one["loop"].feature_calls == 3 and "render volsdf" not in text
    assert listed(out / "scan106", ("depth_est", "confidence", "cams", "images")) == view_files(out)
    assert os.path.exists(out / "mvsnet106_l3.ply")
    from datasets.data_io import read_pfm
    a = read_pfm(str(out / "scan106" / "depth_est" / "00000025.pfm"))[0]
    b = read_pfm(str(scan_run["out"] / "scan106" / "depth_est" / "00000025.pfm"))[0]
    assert a.shape == b.shape and np.isfinite(a).all() and not np.array_equal(a, b)      # (no rendered depth was handed off)
