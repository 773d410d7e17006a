"""tools/dev/step_trace.py: the launch sequence of the train step as the launch plan records it (graph="plan": plan.info and
plan.describe(), one line per node in issue order -- stream, kernel, grid, block, LDS, events waited for / recorded) for four
configurations: two explicit ray groups with an MVS prior (DTU model, background model), a padded batch, and the measured
976 + 48 split of 1024 rays with the small group's jobs folded.  Two commits that claim the same launches must print the same
lines.  Dev aid, GPU only."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "s-volsdf_amd"), os.path.join(ROOT, "tests", "golden")]
import synth                                                             # noqa: E402
from svs_hip.trainer import TrainStep                                    # noqa: E402
from volsdf.model.loss import VolSDFLoss                                 # noqa: E402
from volsdf.utils.conf import bmvs_model_conf, dtu_model_conf            # noqa: E402

dev = torch.device("cuda:0")
G = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def trace(name, kind, R, groups, prior):
    K, pose = synth.make_camera()
    inp = {"intrinsics": G(K)[None], "uv": G(synth.make_uv(R, seed=4))[None], "pose": G(pose)[None]}
    rs = np.random.default_rng(6)
    gt = {k: G(rs.uniform(0, 1, (1, R, 3)).astype(np.float32)) for k in ("rgb", "rgb_smooth")}
    mvs = None
    if prior:
        mvs = dict(views=[dict(K=v["K"], c2w=v["c2w"], cost=G(v["cost"]), z_mvs=G(v["z_mvs"])) for v in synth.make_mvs_views(2)],
                   same_view=0, img_res=(576, 768), inverse_depth=False)
    torch.manual_seed(3)
    if kind == "dtu":
        from volsdf.model.network import VolSDFNetwork
        m = VolSDFNetwork(dtu_model_conf())
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_params(0).items()}, strict=True)
    else:
        from volsdf.model.network_bg import VolSDFNetworkBG
        m = VolSDFNetworkBG(bmvs_model_conf())
    loss = VolSDFLoss(rgb_loss="torch.nn.L1Loss", eikonal_weight=0.1, rgb_weight=1.0, mvs_weight=1.0, sparse_weight=1.0,
                      anneal_rgb=200, gce=0.5, confi=1e-3)
    loss.iter_step = 250
    ts = TrainStep(m.to(dev).train(), loss, groups=groups, graph="plan")
    torch.manual_seed(13)
    for _ in range(2):                                   # an eager step, then the capture and its first replay
        ts(inp, gt, mvs=mvs)
    torch.cuda.synchronize()
    plans = [c.plan for c in ts._captured.values() if c.plan is not None]
    assert len(plans) == 1
    print(f"==== {name}: {kind} R={R} groups={groups} prior={prior}")
    print(plans[0].info)
    print(plans[0].describe())


trace("two groups", "dtu", 128, [(0, 64), (64, 128)], True)
trace("two groups, background", "bmvs", 128, [(0, 64), (64, 128)], True)
trace("padded batch", "dtu", 100, None, False)
trace("auto split, folded", "dtu", 1024, "auto", False)
