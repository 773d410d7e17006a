"""A scan list end to end on the GPU: the reference's runner.py (:46-71, :111-299, :412-459) and helpers/help.py::run_help
on this project's own modules, as a library and as a command.  No checkout of the reference, no hydra / omegaconf /
loguru / GPUtil / OpenCV / scikit-image / plyfile.

    python -m svs_hip.run testlist=scan106 data_dir_root=data_s_volsdf [vol=bmvs] [opt_stepNs=[1000,0,0]] [key=value ...]

Per scan: cost volumes per stage (`StageLoop`) -> volume optimisation (`VolOpt`) -> the rendered depth handed to the next
stage -> depth, confidence, camera, image and preview files (`mvsout.save_view`) -> depth fusion (`fusion.
filter_depth_folder`) -> {outdir}/mvsnet{scan:03}_l3.ply.

    default_args(vol)        the configuration the reference composes from config/ours.yaml -> base.yaml -> vol/<vol>.yaml,
                             restated here as a plain nested dict (what `VolOpt` takes); the two loaders are this project's
    apply_overrides(a, argv) hydra's command-line form: key=value, dotted keys, +key=value, vol=dtu|bmvs
    run_help(args)           derived values, the six assertions (ValueError naming the key), all_scans.yaml, the device
    save_depth / save_scene_depth / pcd_filter / clean_clouds / create_scenes / main
    +tsdf_voxel=V [+tsdf_trunc=T]   after the point clouds, every scan's depth maps meshed by `svs_hip.tsdf` into
                             {outdir}/tsdf/mvsnet{scan:03}_l3.ply (`python -m evals.eval_dtu --datadir {outdir}/tsdf --mode mesh`)
    +tsdf_views=true         with +tsdf_voxel: every scan's TSDF mesh rendered into its training views by `svs_hip.meshview`,
                             {outdir}/tsdf/scanNNN/mesh_depth/{id:08}.pfm and mesh_shade/{id:08}.png
    +tsdf_simplify=R         with +tsdf_voxel: every scan's TSDF mesh also simplified to at most R (in (0,1)) of its faces by
                             `svs_hip.meshsimplify`, {outdir}/tsdf_simple/mvsnet{scan:03}_l3.ply
                             (`python -m evals.eval_dtu --datadir {outdir}/tsdf_simple --mode mesh`)
    +tsdf_smooth=N [+tsdf_smooth_method=taubin|denoise]   with +tsdf_voxel: every scan's TSDF mesh also smoothed by
                             `svs_hip.meshsmooth` (N iterations, boundary fixed), {outdir}/tsdf_smooth/mvsnet{scan:03}_l3.ply;
                             +tsdf_simplify then simplifies the smoothed mesh
    +tsdf_texture=S          with +tsdf_voxel: a texture atlas of S x S texels (S in [64, 16384]) baked by `svs_hip.meshtexture`
                             from every scan's training views for its simplified (+tsdf_simplify), else smoothed (+tsdf_smooth),
                             else plain TSDF mesh, {outdir}/tsdf_texture/mvsnet{scan:03}_l3.{obj,mtl,png}
    +cloud_clean=true [+cloud_k=20 +cloud_std_ratio=2.0 +cloud_normal_k=16]   after the point clouds, every scan's cloud
                             without its statistical outliers and with oriented normals (`svs_hip.cloudclean`), in
                             {outdir}/clean/mvsnet{scan:03}_l3.ply (`python -m evals.eval_dtu --datadir {outdir}/clean`)
    +cloud_poisson=V         with +cloud_clean=true: every scan's cleaned cloud meshed by `svs_hip.poisson` on a grid of node
                             spacing V, {outdir}/poisson/mvsnet{scan:03}_l3.ply
                             (`python -m evals.eval_dtu --datadir {outdir}/poisson --mode mesh`)
    +cloud_poisson_screen=S  with +cloud_poisson: the screened reconstruction (`poisson.reconstruct(screen=S)`, S positive).
                             It has no default value: 1, 4 and 16 were tried on a synthetic sphere of uneven density only

Differences from the reference, all deliberate: `gpu: auto` keeps the current device (there is no GPUtil probe) and an
integer selects it with torch.cuda.set_device; `prevent_oom` is taken as given; the five-second sleep before the first
scan is gone; the point clouds are fused one scan after the other in this process (no worker pool, no further GPU
processes); log lines go through print.  Under a process group (WORLD_SIZE > 1) the runner refuses to start: data-parallel
runs keep going through svs_hip/launch.py.
"""
import copy
import os
import sys
import time
from collections import OrderedDict

from volsdf.utils.conf import attr_view, bmvs_model_conf, dtu_model_conf, to_plain

VOLS = ("dtu", "bmvs")
MVS_MODELS = {"casmvsnet": "casmvsnet.ckpt", "ucsnet": "ucsnet.ckpt", "transmvsnet": "model_dtu.ckpt"}   # runner.py:128-147
PHASES = ("load", "mvs0", "mvs1", "mvs2", "optimise", "render", "save", "fusion")

# save_depth's per-scene adjustments (runner.py:51-65)
DTU_SPARSE_WEIGHT = {"scan37": 0.1, "scan24": 0}
BMVS_NO_SPARSE = ("scan2", "scan3", "scan7", "scan9")
BMVS_INVERSE_DEPTH = ("scan1", "scan2", "scan5", "scan6", "scan8", "scan9")


def info(msg):
    print(msg, flush=True)


# ---- configuration -----------------------------------------------------------------------------------------------------
def vol_group(name):
    """The `vol` group: config/vol/<name>.yaml overlaid with the `vol` section of config/ours.yaml."""
    if name not in VOLS:
        raise ValueError(f"vol: expected one of {VOLS}, got {name!r}")
    dtu = name == "dtu"
    model = to_plain(dtu_model_conf(near=1e-4) if dtu else bmvs_model_conf())
    model["ray_sampler"]["near"] = 1e-4                                  # ours.yaml:22-24, for both datasets
    return dict(
        train=dict(expname="ours",                                       # (ours.yaml; the group files say dtu / bmvs)
                   dataset_class="svs_hip.scene.SceneDataset",           # the reference: volsdf.datasets.scene_dataset.SceneDataset
                   model_class="volsdf.model.network.VolSDFNetwork" if dtu else "volsdf.model.network_bg.VolSDFNetworkBG",
                   loss_class="volsdf.model.loss.VolSDFLoss", learning_rate=5.0e-4, num_pixels=512, checkpoint_freq=100,
                   plot_freq=500, render_freq=500, split_n_pixels=500),
        plot=dict(plot_nimgs=1, resolution=100, grid_boundary=[-1.5, 1.5]),
        loss=dict(eikonal_weight=0.1, mvs_weight=1.0, rgb_weight=1.0, rgb_loss="torch.nn.L1Loss", sparse_weight=1.0,
                  confi=1.0e-3, gce=0.5, anneal_rgb=200),
        dataset=dict(data_dir="DTU" if dtu else "BlendedMVS", img_res=[576, 768], scan_id=114 if dtu else 1, num_views=3),
        model=model)


def default_args(vol="dtu"):
    """config/base.yaml under config/ours.yaml, with the `vol` group of `vol_group(vol)`: a plain nested dict."""
    return dict(
        vol=vol_group(vol),
        # general
        gpu="auto", num_view=3, testlist="scan106", outdir="exps_mvs", exps_folder="exps_vsdf",
        # data
        data_dir_root="data_s_volsdf", max_h=576, max_w=768, trains_i="25,22,28",
        # VolSDF
        use_mvs=True, opt_stepNs=[100000, 0, 0], grad_clip=True,
        # MVS
        mvs_model_name="casmvsnet", ndepths="192,32,8", depth_inter_r="1,0.5,0.5", use_nerf_d=[1, 0, 0], x2_mvsres=True,
        inverse_depth=False, prevent_oom=False, ablate=False, share_cr=False, cr_base_chs="8,8,8", grad_method="detach",
        interval_scale=1.06, numdepth=192, num_workers=0, batch_size=1,
        # evaluation
        eval_mask=True, filter_only=False, filter_dist=1, filter_diff=0.01, conf=0.0, thres_view=1, num_worker=4,
        # this project's: the MVS loader (the reference imports datasets.general_eval.MVSDataset)
        mvs_dataset_class="svs_hip.mvsdata.MVSDataset")


def parse_value(text):
    """The right-hand side of an override: yaml.safe_load, and a number YAML 1.1 reads as a string (1e4) as a number."""
    import yaml
    v = yaml.safe_load(text)
    if isinstance(v, str):
        for cast in (int, float):
            try:
                return cast(v)
            except ValueError:
                pass
    return v


def apply_overrides(args, overrides):
    """hydra's command-line form on a plain dict, in place: `key=value`, `a.b.c=value`, `+key=value` (a key that need not
    exist), `vol=dtu|bmvs` (the whole group; later `vol.x=` overrides apply to it).  A key that does not exist and has no
    `+` is a KeyError naming it.  -> args"""
    overrides = list(overrides)
    for ov in overrides:                                                 # the group first, whatever its position
        key, sep, text = ov.partition("=")
        if key.lstrip("+") == "vol" and sep:
            args["vol"] = vol_group(str(parse_value(text)))
    for ov in overrides:
        key, sep, text = ov.partition("=")
        if not sep or not key.lstrip("+"):
            raise ValueError(f"override {ov!r}: expected key=value")
        add = key.startswith("+")
        key = key.lstrip("+")
        if key == "vol":
            continue
        parts, cur = key.split("."), args
        for k, part in enumerate(parts[:-1]):
            if not isinstance(cur.get(part), dict):
                if not add:
                    raise KeyError(f"unknown key {'.'.join(parts[:k + 1])!r} in override {ov!r} (prefix a new key with +)")
                cur[part] = {}
            cur = cur[part]
        if parts[-1] not in cur and not add:
            raise KeyError(f"unknown key {key!r} in override {ov!r} (prefix a new key with +)")
        cur[parts[-1]] = parse_value(text)
    return args


def _require(ok, key, why):
    if not ok:
        raise ValueError(f"{key}: {why}")


def check_tsdf_simplify(args):
    """+tsdf_simplify=R: a ratio in (0,1), and only together with +tsdf_voxel (ValueError naming the key) -> R or None"""
    r = args.get("tsdf_simplify")
    if r is None:
        return None
    _require(isinstance(r, (int, float)) and not isinstance(r, bool) and 0 < r < 1, "tsdf_simplify", f"a ratio in (0,1), got {r!r}")
    _require(bool(args.get("tsdf_voxel")), "tsdf_simplify", "simplifies the TSDF meshes: give +tsdf_voxel=V as well")
    return float(r)


def check_tsdf_smooth(args):
    """+tsdf_smooth=N [+tsdf_smooth_method=taubin|denoise]: a positive integer and one of the two names, and only together
    with +tsdf_voxel (ValueError naming the key) -> (N, method) or None"""
    n, method = args.get("tsdf_smooth"), args.get("tsdf_smooth_method")
    if n is None:
        _require(method is None, "tsdf_smooth_method", "names the method of +tsdf_smooth=N: give that as well")
        return None
    _require(isinstance(n, int) and not isinstance(n, bool) and n > 0, "tsdf_smooth", f"a positive number of iterations, got {n!r}")
    method = "taubin" if method is None else method
    _require(method in ("taubin", "denoise"), "tsdf_smooth_method", f"taubin or denoise, got {method!r}")
    _require(bool(args.get("tsdf_voxel")), "tsdf_smooth", "smooths the TSDF meshes: give +tsdf_voxel=V as well")
    return int(n), method


def check_tsdf_texture(args):
    """+tsdf_texture=S: an atlas size in [64, 16384], and only together with +tsdf_voxel (ValueError naming the key) -> S or None"""
    size = args.get("tsdf_texture")
    if size is None:
        return None
    _require(isinstance(size, int) and not isinstance(size, bool) and 64 <= size <= 16384, "tsdf_texture",
             f"an atlas size in [64, 16384], got {size!r}")
    _require(bool(args.get("tsdf_voxel")), "tsdf_texture", "textures the TSDF meshes: give +tsdf_voxel=V as well")
    return int(size)


def check_cloud_poisson(args):
    """+cloud_poisson=V: a positive node spacing, and only together with +cloud_clean=true, whose normals it meshes (ValueError
    naming the key) -> V or None"""
    v = args.get("cloud_poisson")
    if v is None:
        return None
    _require(isinstance(v, (int, float)) and not isinstance(v, bool) and v > 0, "cloud_poisson", f"a positive node spacing, got {v!r}")
    _require(bool(args.get("cloud_clean")), "cloud_poisson", "meshes the cleaned clouds: give +cloud_clean=true as well")
    return float(v)


def check_cloud_poisson_screen(args):
    """+cloud_poisson_screen=S: a positive finite screen value, and only together with +cloud_poisson=V (ValueError naming
    the key) -> S or None"""
    s = args.get("cloud_poisson_screen")
    if s is None:
        return None
    _require(isinstance(s, (int, float)) and not isinstance(s, bool) and 0 < s < float("inf"), "cloud_poisson_screen",
             f"a positive finite screen value, got {s!r}")
    _require(args.get("cloud_poisson") is not None, "cloud_poisson_screen", "screens the Poisson meshes: give +cloud_poisson=V as well")
    return float(s)


def save_yaml(path, args):
    import yaml
    with open(path, "w") as f:
        yaml.safe_dump(to_plain(args), f)


def run_help(args, select_device=True):
    """helpers/help.py::run_help on the plain dict, in place: the device, the derived values, the six assertions
    (:48-53, as ValueError naming the key), outdir and all_scans.yaml (unless filter_only).  -> args"""
    a = attr_view(args)
    check_tsdf_simplify(args)
    check_tsdf_smooth(args)
    check_tsdf_texture(args)
    check_cloud_poisson(args)
    check_cloud_poisson_screen(args)
    if select_device and args["gpu"] != "auto":
        import torch
        torch.cuda.set_device(int(args["gpu"]))
    info(f"gpu -> {args['gpu']}")
    args["vol"]["dataset"]["img_res"] = [args["max_h"], args["max_w"]]
    args["vol"]["dataset"]["num_views"] = args["num_view"]
    if a.vol.dataset.data_dir != "DTU":
        args["interval_scale"] = 1.0
    _require(len([int(nd) for nd in str(args["ndepths"]).split(",") if nd]) == 3, "ndepths", "three stages are expected")
    _require(args["depth_inter_r"] == "1,0.5,0.5", "depth_inter_r", f"must be '1,0.5,0.5', got {args['depth_inter_r']!r}")
    _require(args["ndepths"] == "192,32,8", "ndepths", f"must be '192,32,8', got {args['ndepths']!r}")
    _require(list(args["use_nerf_d"]) == [1, 0, 0], "use_nerf_d", f"must be [1,0,0], got {args['use_nerf_d']!r}")
    _require(bool(args["x2_mvsres"]), "x2_mvsres", "must be true")
    _require(a.vol.dataset.data_dir in ("BlendedMVS", "DTU"), "vol.dataset.data_dir",
             f"must be BlendedMVS or DTU, got {a.vol.dataset.data_dir!r}")
    os.makedirs(args["outdir"], exist_ok=True)
    if not args["filter_only"]:
        save_yaml(os.path.join(args["outdir"], "all_scans.yaml"), args)
    return args


def read_testlist(testlist):
    """runner.py:436-441: the lines of a .txt file, or a comma list"""
    testlist = str(testlist)
    if "txt" in testlist:
        with open(testlist) as f:
            return [line.rstrip() for line in f.readlines()]
    return [x for x in testlist.replace(" ", "").split(",") if x]


def ply_name(outdir, scan):
    """runner.py:412-418"""
    assert "scan" in scan
    return os.path.join(outdir, "mvsnet{:0>3}_l3.ply".format(int(scan[4:])))


# ---- the per-scan loop ---------------------------------------------------------------------------------------------------
def scene_adjustments(data_dir, scene, sparse_weight, inverse_depth):
    """runner.py:51-65 -> the sparse_weight and inverse_depth the scan runs with"""
    if data_dir == "DTU":
        sparse_weight = DTU_SPARSE_WEIGHT.get(scene, sparse_weight)
    elif data_dir == "BlendedMVS":
        if scene in BMVS_NO_SPARSE:
            sparse_weight = 0
        if scene in BMVS_INVERSE_DEPTH:
            inverse_depth = True
    return sparse_weight, inverse_depth


def save_depth(args, testlist, scan_fn=None):
    """runner.py:46-71: every scan with its own sparse_weight / inverse_depth, the configured values restored after
    each.  scan_fn(args, scene): what runs a scan (default `save_scene_depth`).  -> {scene: what scan_fn returned}"""
    scan_fn = scan_fn or save_scene_depth
    out = OrderedDict()
    for scene in testlist:
        info(f"parameter adjust - {scene}")
        keep = args["vol"]["loss"]["sparse_weight"], args["inverse_depth"]
        args["vol"]["loss"]["sparse_weight"], args["inverse_depth"] = scene_adjustments(
            args["vol"]["dataset"]["data_dir"], scene, *keep)
        if args["inverse_depth"] and not keep[1]:
            info("    inverse_D=[True,False,False]")
        info(f"    inverse depth={args['inverse_depth']} sparse_weight={args['vol']['loss']['sparse_weight']}")
        try:
            out[scene] = scan_fn(args, scene)
        finally:
            args["vol"]["loss"]["sparse_weight"], args["inverse_depth"] = keep
    return out


def _ints(text):
    return [int(x) for x in str(text).split(",") if x]


def build_model(args):
    """runner.py:127-154: the network named by mvs_model_name with its checkpoint's 'model' entry, strictly, on the GPU"""
    import torch
    name = args["mvs_model_name"]
    if name not in MVS_MODELS:
        raise NotImplementedError(f"mvs_model_name: expected one of {tuple(MVS_MODELS)}, got {name!r}")
    ndepths = _ints(args["ndepths"])
    ratios = [float(x) for x in str(args["depth_inter_r"]).split(",") if x]
    if name == "casmvsnet":
        from models.CasMVSNet import CascadeMVSNet
        model = CascadeMVSNet(refine=False, ndepths=ndepths, depth_interals_ratio=ratios, share_cr=args["share_cr"],
                              cr_base_chs=_ints(args["cr_base_chs"]), grad_method=args["grad_method"])
    elif name == "ucsnet":
        from models.ucsnet import UCSNetHip
        model = UCSNetHip(stage_configs=ndepths, lamb=1.5)
    else:
        from models.transmvs import TransMVSNetHip
        model = TransMVSNetHip(refine=False, ndepths=ndepths, depth_interals_ratio=ratios, share_cr=args["share_cr"],
                               cr_base_chs=_ints(args["cr_base_chs"]), grad_method=args["grad_method"])
    info("loading model {}".format(name))
    path = os.path.join(args["data_dir_root"], "mvs_models", MVS_MODELS[name])
    state = torch.load(path, map_location=torch.device("cpu"))
    model.load_state_dict(state["model"], strict=True)
    return model.cuda().eval()


def mvs_dataset(args, scene, trains_i, phases=None):
    import volsdf.utils.general as utils
    cls = utils.get_class(args["mvs_dataset_class"])
    data_dir = args["vol"]["dataset"]["data_dir"]
    kw = dict(phases=phases) if phases is not None and cls.__module__ == "svs_hip.mvsdata" else {}
    return cls(os.path.join(args["data_dir_root"], data_dir, "mvs_data"), [scene], "test", args["num_view"], data_dir,
               args["numdepth"], args["interval_scale"], max_h=args["max_h"], max_w=args["max_w"], trains_i=trains_i,
               args=attr_view(args), **kw)


def _device_samples(ds):
    """the scan's samples as DataLoader(batch_size=1) + tocuda deliver them (runner.py:122,185)"""
    if hasattr(ds, "device_samples"):
        return ds.device_samples()
    import torch

    def put(v):
        if isinstance(v, dict):
            return {k: put(x) for k, x in v.items()}
        return v.cuda() if torch.is_tensor(v) else v
    return [put(s) for s in torch.utils.data.DataLoader(ds, 1, shuffle=False, num_workers=0, drop_last=False)]


def save_scene_depth(args, scene):
    """runner.py:111-299 for one scan.  -> dict(loop, vol_opt, clock: the seconds per phase of PHASES (the device is drained
    at every boundary so that they add up), files: [save_view's names per view])"""
    import torch
    from . import mvsout
    from .images import Phases
    from .scans import get_trains_ids
    from .stage_loop import StageLoop
    from volsdf.vsdf import VolOpt
    os.makedirs(os.path.join(args["outdir"], scene), exist_ok=True)
    save_yaml(os.path.join(args["outdir"], scene, "args.yaml"), args)
    clock, t0 = Phases(PHASES, sync=True), time.perf_counter()

    trains_i = get_trains_ids(args["vol"]["dataset"]["data_dir"], scene, args["num_view"])
    ds = mvs_dataset(args, scene, trains_i)
    samples = _device_samples(ds)
    torch.cuda.empty_cache()
    model = build_model(args)
    use_nerf_d, opt_stepNs = list(args["use_nerf_d"]), list(args["opt_stepNs"])

    vol_opt = None
    if not args["ablate"]:
        # the reference's VolOpt writes the scan's id into the shared `dataset` section, where its preview dataset reads it
        # (vsdf.py:76-78,147); here sections are copies, so the id goes in up front.  args.yaml keeps the configured one.
        vol_args = copy.deepcopy(args)
        vol_args["vol"]["dataset"]["scan_id"] = int(scene[4:])
        vol_opt = VolOpt(args=vol_args, batch_size=1, is_continue=args.get("is_continue", False), timestamp="latest",
                         checkpoint="latest", scan=scene)
        vol_opt.trains_i = trains_i
        assert vol_opt.trains_i == vol_opt.train_dataset.trains_ids()
    t0 = clock.add("load", t0)

    loop = StageLoop(model)
    loop.clear()
    img_n = len(samples)
    view_extra_samples, outs_samples = [None] * img_n, [None] * img_n
    depths = [None] * img_n
    for stage_idx in range(3):
        int_r = None if args["mvs_model_name"] == "ucsnet" else model.depth_interals_ratio[stage_idx]
        # (a) cost volume
        outs, view_extras = loop.cost_volumes(stage_idx, samples, outs_samples, view_extra_samples, int_r=int_r,
                                              inverse_depth=args["inverse_depth"], prevent_oom=args["prevent_oom"])
        t0 = clock.add(f"mvs{stage_idx}", t0)
        info(f"time(gen cost volume)={clock.s[f'mvs{stage_idx}']:.2f}")
        # (b) volume optimisation
        if not args["ablate"] and opt_stepNs[stage_idx] > 0 and use_nerf_d[stage_idx] > 0:
            vol_opt.gen_dataset(stage_idx)
            vol_opt.stg = stage_idx
            vol_opt.loss.set_stg(stage_idx)
            vol_opt.get_mvs_input(outs)
            epoch = vol_opt.run(opt_stepNs[stage_idx]) if opt_stepNs[stage_idx] > 1 else 0
            t0 = clock.add("optimise", t0)
            info(f"render volsdf at {vol_opt.plots_dir} ..")
            for i, id_k in enumerate(trains_i):
                depths[i], _ = vol_opt.render_mvs(id_k, epoch)
            info(f"mvs_depth replaced by vol_depth at stg={stage_idx} in 0,1,2")
            outs = StageLoop.hand_off_depth(outs, stage_idx, depths)
            t0 = clock.add("render", t0)
        outs_samples, view_extra_samples = outs, view_extras

    files = []
    for sample, outputs in zip(samples, outs_samples):
        view = int(sample["filename"][0].split("/")[-1][:8])
        files.append(mvsout.save_view(os.path.join(args["outdir"], scene), view, outputs,
                                      sample["proj_matrices"]["stage3"][0, 0], sample["imgs"][0, 0], previews=True,
                                      dep_max=float(sample["depth_values"].max())))
    clock.add("save", t0)
    del outs_samples, view_extra_samples
    loop.clear()
    torch.cuda.empty_cache()
    return dict(loop=loop, vol_opt=vol_opt, clock=clock, files=files)


def pcd_filter(args, testlist, clocks=None):
    """runner.py:301-432 without the worker pool: `fusion.filter_depth_folder` per scan, one after the other, in this
    process.  -> {scene: (xyz, rgb, stats)}"""
    from . import fusion
    from .scans import get_trains_ids
    data_dir = args["vol"]["dataset"]["data_dir"]
    out = OrderedDict()
    for scan in testlist:
        t0 = time.perf_counter()
        folder, ply = os.path.join(args["outdir"], scan), ply_name(args["outdir"], scan)
        masks = dict(eval_mask_root=args["data_dir_root"], dataset=data_dir) if args["eval_mask"] else {}
        xyz, rgb, stats = fusion.filter_depth_folder(folder, folder, ply, get_trains_ids(data_dir, scan, args["num_view"]),
                                                     conf=args["conf"], filter_dist=args["filter_dist"],
                                                     filter_diff=args["filter_diff"], thres_view=args["thres_view"], **masks)
        for v, photo, geo, final in stats:
            info("processing {}, ref-view{:0>2}, photo/geo/final-mask:{:.3f}/{:.3f}/{:.3f}".format(folder, v, photo, geo, final))
        info(f"saving the final MVS result to {ply}")
        if clocks is not None and scan in clocks:
            clocks[scan].add("fusion", t0)
        out[scan] = (xyz, rgb, stats)
    return out


def tsdf_ply_name(outdir, scan):
    """the mesh of a scan: the point cloud's name one folder down, where `evals.eval_dtu --mode mesh` finds it"""
    return ply_name(os.path.join(outdir, "tsdf"), scan)


def tsdf_meshes(args, testlist):
    """+tsdf_voxel=V [+tsdf_trunc=T]: every scan's filtered depth maps meshed by `tsdf.fuse_folder` into
    {outdir}/tsdf/mvsnet{scan:03}_l3.ply, with the filter settings and evaluation masks of `pcd_filter`; one time line per
    scan.  -> {scene: fuse_folder's stats}"""
    from . import tsdf
    from .scans import get_trains_ids
    data_dir = args["vol"]["dataset"]["data_dir"]
    out = OrderedDict()
    for scan in testlist:
        folder = os.path.join(args["outdir"], scan)
        masks = dict(eval_mask_root=args["data_dir_root"], dataset=data_dir) if args["eval_mask"] else {}
        stats = tsdf.fuse_folder(folder, folder, get_trains_ids(data_dir, scan, args["num_view"]), args["tsdf_voxel"],
                                 trunc=args.get("tsdf_trunc"), ply=tsdf_ply_name(args["outdir"], scan), conf=args["conf"],
                                 filter_dist=args["filter_dist"], filter_diff=args["filter_diff"],
                                 thres_view=args["thres_view"], **masks)[3]
        info(f"saving the TSDF mesh to {stats['file']} ({stats['n_verts']} vertices, {stats['n_faces']} faces)")
        info(f"{scan} tsdf seconds: " + ", ".join(f"{k} {v:.3f}" for k, v in stats["seconds"].items()))
        out[scan] = stats
    return out


def tsdf_views(args, testlist):
    """+tsdf_views=true: every scan's TSDF mesh (`tsdf_meshes`) rendered into that scan's training views by
    `meshview.view_folder`, under {outdir}/tsdf/{scan}/; one time line per scan.  -> {scene: view_folder's stats}"""
    from . import meshview
    from .scans import get_trains_ids
    data_dir = args["vol"]["dataset"]["data_dir"]
    out = OrderedDict()
    for scan in testlist:
        folder = os.path.join(args["outdir"], scan)
        stats = meshview.view_folder(tsdf_ply_name(args["outdir"], scan), folder, os.path.join(args["outdir"], "tsdf", scan),
                                     get_trains_ids(data_dir, scan, args["num_view"]))[1]
        info(f"saving the TSDF mesh's views to {os.path.dirname(stats['files']['depth'][0])} and "
             f"{os.path.dirname(stats['files']['shade'][0])}")
        info(f"{scan} tsdf views seconds: " + ", ".join(f"{k} {v:.3f}" for k, v in stats["seconds"].items()))
        out[scan] = stats
    return out


def tsdf_simple_ply_name(outdir, scan):
    """the simplified TSDF mesh of a scan, where `evals.eval_dtu --datadir {outdir}/tsdf_simple --mode mesh` finds it"""
    return ply_name(os.path.join(outdir, "tsdf_simple"), scan)


def tsdf_smooth_ply_name(outdir, scan):
    """the smoothed TSDF mesh of a scan, where `evals.eval_dtu --datadir {outdir}/tsdf_smooth --mode mesh` finds it"""
    return ply_name(os.path.join(outdir, "tsdf_smooth"), scan)


def tsdf_smoothed(args, testlist):
    """+tsdf_smooth=N [+tsdf_smooth_method=M]: every scan's TSDF mesh (`tsdf_meshes`) smoothed by `meshsmooth.smooth_ply` into
    {outdir}/tsdf_smooth/mvsnet{scan:03}_l3.ply -- taubin: N iterations; denoise: N vertex and max(1, N // 2) normal
    iterations; the boundary fixed, because TSDF meshes are open surfaces; one time line per scan.
    -> {scene: smooth_ply's stats}"""
    from . import meshsmooth
    n, method = check_tsdf_smooth(args)
    out = OrderedDict()
    for scan in testlist:
        ply = tsdf_smooth_ply_name(args["outdir"], scan)
        os.makedirs(os.path.dirname(ply), exist_ok=True)
        stats = meshsmooth.smooth_ply(tsdf_ply_name(args["outdir"], scan), ply, method, iters=n, vertex_iters=n,
                                      normal_iters=max(1, n // 2), boundary="fixed")[3]
        info(f"saving the smoothed TSDF mesh to {ply} ({method}, {n} iterations, {stats['faces']} faces, "
             f"{stats['counts']['boundary_edges']} boundary edges)")
        info(f"{scan} tsdf smooth seconds: " + ", ".join(f"{k} {v:.3f}" for k, v in stats["seconds"].items()))
        out[scan] = stats
    return out


def tsdf_simplified(args, testlist):
    """+tsdf_simplify=R: every scan's TSDF mesh (`tsdf_meshes`; with +tsdf_smooth the smoothed one, `tsdf_smoothed`) simplified
    by `meshsimplify.simplify_ply` to at most R of its faces, into {outdir}/tsdf_simple/mvsnet{scan:03}_l3.ply; one time line
    per scan.  -> {scene: simplify_ply's stats}"""
    from . import meshsimplify
    ratio = check_tsdf_simplify(args)
    source = tsdf_smooth_ply_name if args.get("tsdf_smooth") is not None else tsdf_ply_name
    out = OrderedDict()
    for scan in testlist:
        ply = tsdf_simple_ply_name(args["outdir"], scan)
        os.makedirs(os.path.dirname(ply), exist_ok=True)
        stats = meshsimplify.simplify_ply(source(args["outdir"], scan), ply, ratio=ratio)[3]
        info(f"saving the simplified TSDF mesh to {ply} ({stats['faces_out']} of {stats['faces_in']} faces, cell {stats['cell']:.6g})")
        info(f"{scan} tsdf simplify seconds: " + ", ".join(f"{k} {v:.3f}" for k, v in stats["seconds"].items()))
        out[scan] = stats
    return out


def tsdf_texture_obj_name(outdir, scan):
    """the textured TSDF mesh of a scan: the point cloud's name in {outdir}/tsdf_texture, as an OBJ beside its MTL and PNG"""
    return ply_name(os.path.join(outdir, "tsdf_texture"), scan)[:-4] + ".obj"


def tsdf_textured(args, testlist):
    """+tsdf_texture=S: every scan's TSDF mesh -- the simplified one with +tsdf_simplify, else the smoothed one with
    +tsdf_smooth, else `tsdf_meshes`' -- textured from the scan's training views by `meshtexture.texture_folder` into
    {outdir}/tsdf_texture/mvsnet{scan:03}_l3.{obj,mtl,png}; one time line per scan.  -> {scene: texture_folder's stats}"""
    from . import meshtexture
    from .scans import get_trains_ids
    size = check_tsdf_texture(args)
    data_dir = args["vol"]["dataset"]["data_dir"]
    source = (tsdf_simple_ply_name if args.get("tsdf_simplify") is not None else
              tsdf_smooth_ply_name if args.get("tsdf_smooth") is not None else tsdf_ply_name)
    out = OrderedDict()
    for scan in testlist:
        obj = tsdf_texture_obj_name(args["outdir"], scan)
        stats = meshtexture.texture_folder(source(args["outdir"], scan), os.path.join(args["outdir"], scan),
                                           get_trains_ids(data_dir, scan, args["num_view"]), obj, size=size)[1]
        info(f"saving the textured TSDF mesh to {obj} ({stats['faces_written']} faces, atlas {size} x {size}, cell {stats['cell']}, "
             f"{stats['texels_baked']} texels baked, {stats['texels_from_vertices']} from vertex colours)")
        info(f"{scan} tsdf texture seconds: " + ", ".join(f"{k} {v:.3f}" for k, v in stats["seconds"].items()))
        out[scan] = stats
    return out


def clean_ply_name(outdir, scan):
    """the cleaned cloud of a scan: the point cloud's name one folder down, where `evals.eval_dtu --datadir` finds it"""
    return ply_name(os.path.join(outdir, "clean"), scan)


def clean_clouds(args, testlist):
    """+cloud_clean=true [+cloud_k=20 +cloud_std_ratio=2.0 +cloud_normal_k=16]: every scan's views fused with the settings
    and evaluation masks of `pcd_filter`, cleaned by `cloudclean.clean_folder` into {outdir}/clean/mvsnet{scan:03}_l3.ply; one
    time line per scan.  -> {scene: clean_folder's stats}"""
    from . import cloudclean
    from .scans import get_trains_ids
    data_dir = args["vol"]["dataset"]["data_dir"]
    out = OrderedDict()
    for scan in testlist:
        folder, ply = os.path.join(args["outdir"], scan), clean_ply_name(args["outdir"], scan)
        os.makedirs(os.path.dirname(ply), exist_ok=True)
        masks = dict(eval_mask_root=args["data_dir_root"], dataset=data_dir) if args["eval_mask"] else {}
        stats = cloudclean.clean_folder(folder, folder, get_trains_ids(data_dir, scan, args["num_view"]), ply,
                                        k=int(args.get("cloud_k", 20)), std_ratio=float(args.get("cloud_std_ratio", 2.0)),
                                        normal_k=int(args.get("cloud_normal_k", 16)), conf=args["conf"],
                                        filter_dist=args["filter_dist"], filter_diff=args["filter_diff"],
                                        thres_view=args["thres_view"], **masks)["stats"]
        info(f"saving the cleaned cloud to {ply} ({stats['points_kept']} of {stats['points_in']} points, "
             f"threshold {stats['threshold']:.6g})")
        info(f"{scan} cloud clean seconds: " + ", ".join(f"{k} {v:.3f}" for k, v in stats["seconds"].items()))
        out[scan] = stats
    return out


def poisson_ply_name(outdir, scan):
    """the Poisson mesh of a scan's cleaned cloud, where `evals.eval_dtu --datadir {outdir}/poisson --mode mesh` finds it"""
    return ply_name(os.path.join(outdir, "poisson"), scan)


def poisson_meshes(args, testlist):
    """+cloud_poisson=V: every scan's cleaned cloud (`clean_clouds`) meshed by `poisson.reconstruct_ply` on a grid of node
    spacing V into {outdir}/poisson/mvsnet{scan:03}_l3.ply, screened with +cloud_poisson_screen=S; one time line per scan.
    -> {scene: reconstruct_ply's stats}"""
    from . import poisson
    voxel, screen = check_cloud_poisson(args), check_cloud_poisson_screen(args)
    out = OrderedDict()
    for scan in testlist:
        ply = poisson_ply_name(args["outdir"], scan)
        stats = poisson.reconstruct_ply(clean_ply_name(args["outdir"], scan), ply, voxel, screen=screen)["stats"]
        g = stats["grid"]
        info(f"saving the Poisson mesh to {ply} ({stats['n_verts']} vertices, {stats['faces_after']} of {stats['faces_before']} faces, "
             f"grid {g[0]} x {g[1]} x {g[2]}, {stats['iterations']} iterations" + ("" if screen is None else f", screen {screen:g}") + ")")
        info(f"{scan} cloud poisson seconds: " + ", ".join(f"{k} {v:.3f}" for k, v in stats["seconds"].items()))
        out[scan] = stats
    return out


def create_scenes(args, testlist):
    """runner.py:74-108, 447-452: the folder of cameras and images that image-based rendering reads, per scan"""
    from . import mvsdata
    from .scans import get_eval_ids, get_trains_ids
    args["x2_mvsres"] = False
    assert args["num_view"] == 3
    data_dir = args["vol"]["dataset"]["data_dir"]
    out = OrderedDict()
    for scene in testlist:
        evals_i = get_eval_ids(data_dir, int(scene[4:]))
        trains_i = get_trains_ids(data_dir, scene, args["num_view"])
        ds = mvs_dataset(args, scene, trains_i + [i for i in evals_i if i not in trains_i])
        out[scene] = mvsdata.create_scene(args["outdir"], ds, evals_i)
    return out


def main(argv=None, scan_fn=None):
    """-> dict(args, testlist, scans: {scene: save_scene_depth's dict}, clouds: {scene: (xyz, rgb, stats)})"""
    argv = list(sys.argv[1:] if argv is None else argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError("svs_hip.run drives one process; under a process group (WORLD_SIZE > 1) run the reference's "
                           "runner.py through svs_hip/launch.py, which shards the optimisation over the ranks")
    vol = "dtu"
    for ov in argv:
        if ov.lstrip("+").startswith("vol="):
            vol = ov.partition("=")[2]
    args = apply_overrides(default_args(vol), argv)
    args = run_help(args)
    info("svs_hip.run " + " ".join(argv))
    testlist = read_testlist(args["testlist"])
    info(f"{testlist} {args['outdir']} {args['exps_folder']}")
    result = dict(args=args, testlist=testlist, scans=OrderedDict(), clouds=OrderedDict())
    if args.get("create_scene", False):
        result["scenes"] = create_scenes(args, testlist)
        return result
    if not args["filter_only"]:
        result["scans"] = save_depth(args, testlist, scan_fn)
    clocks = {s: r["clock"] for s, r in result["scans"].items() if isinstance(r, dict) and "clock" in r}
    result["clouds"] = pcd_filter(args, testlist, clocks)
    for scene, clock in clocks.items():
        info(f"{scene} seconds: " + ", ".join(f"{k} {v:.3f}" for k, v in clock.s.items()))
    if args.get("tsdf_voxel"):
        result["meshes"] = tsdf_meshes(args, testlist)
        if args.get("tsdf_views"):
            result["mesh_views"] = tsdf_views(args, testlist)
        if args.get("tsdf_smooth") is not None:
            result["smooth_meshes"] = tsdf_smoothed(args, testlist)
        if args.get("tsdf_simplify") is not None:
            result["simple_meshes"] = tsdf_simplified(args, testlist)
        if args.get("tsdf_texture") is not None:
            result["textured_meshes"] = tsdf_textured(args, testlist)
    if args.get("cloud_clean"):
        result["clean"] = clean_clouds(args, testlist)
        if args.get("cloud_poisson") is not None:
            result["poisson"] = poisson_meshes(args, testlist)
    return result


if __name__ == "__main__":
    main()
