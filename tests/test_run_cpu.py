"""svs_hip.run without a GPU: the configuration against the reference's composed YAML (tests/golden/run_config.json),
override parsing, run_help, the per-scene adjustments with an injected scan function, the testlist forms and file names;
and the host arithmetic of the save tail: numpy's quantile rule and the preview restatement the GPU tests compare with."""
import copy
import json
import os

import numpy as np
import pytest

import run_oracle as ro
from svs_hip import mvsout, run

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def composed():
    with open(os.path.join(GOLDEN, "run_config.json")) as f:
        return json.load(f)


def helped(args, tmp_path, **kw):
    args["outdir"] = str(tmp_path / "out")
    args.update(kw)
    return run.run_help(args, select_device=False)


def assert_same(ours, want, path=""):
    assert type(ours) is type(want) or (isinstance(ours, (int, float)) and isinstance(want, (int, float))), path
    if isinstance(want, dict):
        assert sorted(ours) == sorted(want), path
        for k in want:
            assert_same(ours[k], want[k], f"{path}.{k}")
    else:
        assert ours == want, path


@pytest.mark.parametrize("vol", ["dtu", "bmvs"])
def test_default_args_are_the_references_composed_configuration(vol, composed, tmp_path):
    want = copy.deepcopy(composed[vol])
    assert len(want) == 35 and want["vol"]["train"]["num_pixels"] == 512
    assert want["vol"]["model"]["ray_sampler"]["near"] == 1e-4 and want["vol"]["loss"]["confi"] == 0.001
    # what run_help derives (help.py:35-38)
    want["vol"]["dataset"]["img_res"] = [want["max_h"], want["max_w"]]
    want["vol"]["dataset"]["num_views"] = want["num_view"]
    if vol == "bmvs":
        want["interval_scale"] = 1.0
    want["outdir"] = str(tmp_path / "out")
    ours = helped(run.default_args(vol), tmp_path)
    # the two loaders are this project's own, deliberately
    assert ours.pop("mvs_dataset_class") == "svs_hip.mvsdata.MVSDataset"
    assert ours["vol"]["train"].pop("dataset_class") == "svs_hip.scene.SceneDataset"
    assert want["vol"]["train"].pop("dataset_class") == "volsdf.datasets.scene_dataset.SceneDataset"
    assert_same(ours, want)
    # ... and they resolve, as does everything VolOpt looks up by name
    import volsdf.utils.general as utils
    from svs_hip.mvsdata import MVSDataset
    from svs_hip.scene import SceneDataset
    assert utils.get_class("svs_hip.scene.SceneDataset") is SceneDataset
    assert utils.get_class("svs_hip.mvsdata.MVSDataset") is MVSDataset
    for k in ("model_class", "loss_class"):
        assert utils.get_class(ours["vol"]["train"][k]).__name__ == want["vol"]["train"][k].rsplit(".", 1)[1]


def test_default_args_are_plain_and_what_volopt_reads():
    import yaml
    from volsdf.utils.conf import Conf, attr_view
    a = run.default_args("bmvs")
    assert yaml.safe_load(yaml.safe_dump(a)) == a                          # plain: dicts, lists, numbers, strings
    v = attr_view(a)
    assert v.exps_folder == "exps_vsdf" and v.vol.dataset.data_dir == "BlendedMVS" and v.grad_clip is True
    conf = Conf(a["vol"])
    assert conf.get_int("train.num_pixels") == 512 and conf.get_string("train.ckpt_dir", "") == ""
    assert conf.get_config("model.bg_network")["rendering_network"]["mode"] == "nerf"
    assert "sphere_scale" not in a["vol"]["model"]["implicit_network"]
    assert run.default_args("dtu")["vol"]["model"]["implicit_network"]["sphere_scale"] == 20.0
    with pytest.raises(ValueError, match="vol"):
        run.default_args("eth3d")


def test_overrides():
    a = run.apply_overrides(run.default_args(), ["testlist=scan24,scan37", "opt_stepNs=[1000,0,0]", "vol.loss.sparse_weight=0.1",
                                                 "+create_scene=true", "filter_only=true", "gpu=3", "filter_dist=1e4",
                                                 "vol.model.ray_sampler.N_samples=32", "+extra.deep.key=[1,2]",
                                                 "data_dir_root=/data/s volsdf", "ndepths=192,32,8", "conf=0.25"])
    assert a["testlist"] == "scan24,scan37" and a["opt_stepNs"] == [1000, 0, 0] and a["vol"]["loss"]["sparse_weight"] == 0.1
    assert a["create_scene"] is True and a["filter_only"] is True and a["gpu"] == 3 and a["filter_dist"] == 1e4
    assert a["vol"]["model"]["ray_sampler"]["N_samples"] == 32 and a["extra"] == {"deep": {"key": [1, 2]}}
    assert a["data_dir_root"] == "/data/s volsdf" and a["ndepths"] == "192,32,8" and a["conf"] == 0.25
    # the group switches as a whole, wherever it stands, and dotted overrides land on the new group
    b = run.apply_overrides(run.default_args(), ["vol.train.num_pixels=256", "vol=bmvs"])
    want = run.vol_group("bmvs")
    want["train"]["num_pixels"] = 256
    assert b["vol"] == want and b["vol"]["dataset"]["data_dir"] == "BlendedMVS" and "bg_network" in b["vol"]["model"]
    with pytest.raises(KeyError, match="create_scene"):
        run.apply_overrides(run.default_args(), ["create_scene=true"])
    with pytest.raises(KeyError, match="vol.loss.sparse"):
        run.apply_overrides(run.default_args(), ["vol.loss.sparse=1"])
    with pytest.raises(ValueError, match="key=value"):
        run.apply_overrides(run.default_args(), ["testlist"])
    with pytest.raises(ValueError, match="vol"):
        run.apply_overrides(run.default_args(), ["vol=eth3d"])


def test_run_help(tmp_path, capsys):
    a = helped(run.default_args("bmvs"), tmp_path, max_h=96, max_w=128, num_view=3)
    assert a["vol"]["dataset"]["img_res"] == [96, 128] and a["vol"]["dataset"]["num_views"] == 3 and a["interval_scale"] == 1.0
    assert helped(run.default_args("dtu"), tmp_path)["interval_scale"] == 1.06
    assert "gpu -> auto" in capsys.readouterr().out
    import yaml
    with open(tmp_path / "out" / "all_scans.yaml") as f:
        assert yaml.safe_load(f) == helped(run.default_args("dtu"), tmp_path)
    os.remove(tmp_path / "out" / "all_scans.yaml")
    helped(run.default_args(), tmp_path, filter_only=True)
    assert not os.path.exists(tmp_path / "out" / "all_scans.yaml")
    a = run.default_args()
    a["vol"]["dataset"]["data_dir"] = "ETH3D"
    for key, bad in (("ndepths", dict(ndepths="192,32")), ("depth_inter_r", dict(depth_inter_r="4,2,1")),
                     ("ndepths", dict(ndepths="48,32,8")), ("use_nerf_d", dict(use_nerf_d=[1, 1, 0])),
                     ("x2_mvsres", dict(x2_mvsres=False)), ("vol.dataset.data_dir", None)):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            helped(a if bad is None else run.default_args(), tmp_path, **(bad or {}))


# runner.py:51-65, written out: scene -> (sparse_weight, inverse_depth) with the configured 1.0 / False elsewhere
ADJUSTED = {"DTU": {"scan37": (0.1, False), "scan24": (0, False)},
            "BlendedMVS": {"scan1": (1.0, True), "scan2": (0, True), "scan3": (0, False), "scan5": (1.0, True),
                           "scan6": (1.0, True), "scan7": (0, False), "scan8": (1.0, True), "scan9": (0, True)}}


@pytest.mark.parametrize("vol", ["dtu", "bmvs"])
def test_per_scene_adjustments_and_restore(vol, composed, capsys):
    scans = composed["lists"][vol]
    assert len(scans) == (11 if vol == "dtu" else 9)
    args = run.default_args(vol)
    data_dir = args["vol"]["dataset"]["data_dir"]
    seen = {}

    def scan_fn(a, scene):
        assert a is args
        seen[scene] = (a["vol"]["loss"]["sparse_weight"], a["inverse_depth"])
        return scene.upper()
    out = run.save_depth(args, scans, scan_fn)
    assert list(out) == scans and out[scans[0]] == scans[0].upper()
    assert seen == {s: ADJUSTED[data_dir].get(s, (1.0, False)) for s in scans}
    assert args["vol"]["loss"]["sparse_weight"] == 1.0 and args["inverse_depth"] is False
    text = capsys.readouterr().out
    assert f"parameter adjust - {scans[0]}" in text and text.count("inverse_D=[True,False,False]") == (0 if vol == "dtu" else 6)
    # the configured values, not the defaults, are what is restored -- also when the scan fails
    args["vol"]["loss"]["sparse_weight"], args["inverse_depth"] = 0.5, True

    def failing(a, scene):
        raise RuntimeError(scene)
    with pytest.raises(RuntimeError):
        run.save_depth(args, ["scan24" if vol == "dtu" else "scan2"], failing)
    assert args["vol"]["loss"]["sparse_weight"] == 0.5 and args["inverse_depth"] is True


def test_testlist_forms_and_file_names(tmp_path):
    assert run.read_testlist("scan106") == ["scan106"]
    assert run.read_testlist("scan24, scan37,,scan106") == ["scan24", "scan37", "scan106"]
    lst = tmp_path / "list.txt"
    lst.write_text("scan1\nscan2 \nscan9\n")
    assert run.read_testlist(str(lst)) == ["scan1", "scan2", "scan9"]
    assert run.ply_name("out", "scan106") == os.path.join("out", "mvsnet106_l3.ply")
    assert run.ply_name("out", "scan9") == os.path.join("out", "mvsnet009_l3.ply")
    assert run.MVS_MODELS == {"casmvsnet": "casmvsnet.ckpt", "ucsnet": "ucsnet.ckpt", "transmvsnet": "model_dtu.ckpt"}


def test_main_drives_the_scans_and_refuses_a_process_group(tmp_path, monkeypatch):
    calls = []

    def scan_fn(a, scene):
        calls.append((scene, a["vol"]["loss"]["sparse_weight"], a["opt_stepNs"]))
        return None
    monkeypatch.setattr(run, "pcd_filter", lambda args, testlist, clocks=None: {s: None for s in testlist})
    out = run.main([f"outdir={tmp_path / 'o'}", "testlist=scan37,scan40", "opt_stepNs=[5,0,0]"], scan_fn=scan_fn)
    assert calls == [("scan37", 0.1, [5, 0, 0]), ("scan40", 1.0, [5, 0, 0])] and list(out["clouds"]) == ["scan37", "scan40"]
    assert os.path.exists(tmp_path / "o" / "all_scans.yaml")
    del calls[:]
    run.main([f"outdir={tmp_path / 'o'}", "filter_only=true"], scan_fn=scan_fn)
    assert calls == []
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="launch.py"):
        run.main([f"outdir={tmp_path / 'o'}"], scan_fn=scan_fn)


# ---- the host arithmetic of the save tail ------------------------------------------------------------------------------------
def maps():
    rng = np.random.default_rng(5)
    out = {n: rng.normal(500, 80, n).astype(np.float32) for n in (1, 2, 7, 100, 101, 12288)}
    out["ties"] = rng.integers(0, 3, 1000).astype(np.float32)
    out["inf"] = np.concatenate([rng.normal(0, 1, 50).astype(np.float32), np.float32([np.inf, np.inf, -np.inf])])
    return out


@pytest.mark.parametrize("q", [0.0, 0.01, 0.05, 0.5, 0.95, 1.0])
def test_quantile_rule_is_numpys(q):
    for name, a in maps().items():
        with np.errstate(invalid="ignore"):
            want_q, want_p = np.quantile(a, q), np.percentile(a, q * 100)
        got_q = mvsout.quantile(a, q, select=ro.sort_select)
        got_p = mvsout.percentile(a, q * 100, select=ro.sort_select)
        assert got_q.dtype == np.float32 and ro.same_bits(got_q, want_q), (name, q, got_q, want_q)
        assert ro.same_bits(got_p, want_p), (name, q, got_p, want_p)
    a = maps()[101].copy()
    a[17] = np.nan
    assert np.isnan(mvsout.quantile(a, q, select=ro.sort_select)) and np.isnan(np.quantile(a, q))


def test_percentile_of_the_valid_pixels():
    rng = np.random.default_rng(9)
    a = rng.normal(0, 1, 400).astype(np.float32)
    a[[3, 50, 51, 399]] = [np.nan, np.inf, -np.inf, -np.inf]
    valid = a[np.isfinite(a)]
    got = mvsout.percentile(a, [5, 95, 100, 0], valid_only=True, select=ro.sort_select)
    want = np.float32([np.percentile(valid, p) for p in (5, 95, 100, 0)])
    assert ro.same_bits(got, want), (got, want)
    with pytest.raises(ValueError):
        mvsout.percentile(np.float32([np.nan, np.inf]), 5, valid_only=True, select=ro.sort_select)


def test_preview_restatement_is_the_references_function():
    g = np.load(os.path.join(GOLDEN, "depth_preview.npz"))
    names = sorted({k.rsplit("/", 1)[0] for k in g.files if "/" in k})
    assert len(names) == 16
    for key in names:
        lo, hi = g[f"{key}/lo"], g[f"{key}/hi"]
        got = ro.visualize_depth(g[f"{key}/depth"], None if np.isnan(lo) else lo, None if np.isnan(hi) else hi,
                                 direct=bool(g[f"{key}/direct"]), table=g["table"])
        assert np.array_equal(got, g[f"{key}/out"]), key
    assert not ro.visualize_depth(np.ones((2, 3), np.float32), 1.0, 1.0, table=g["table"]).any()


def test_key_order_is_np_sort_up_to_the_zeros():
    rng = np.random.default_rng(2)
    a = rng.normal(0, 1, 5000).astype(np.float32)
    a[rng.integers(0, 5000, 600)] = 0.0
    a[rng.integers(0, 5000, 600)] = -0.0
    a[[1, 2, 3, 4]] = [np.inf, -np.inf, np.nan, 1e-42]
    s = ro.key_order(a)
    assert ro.same_bits(s, np.sort(a))
    zeros = s[s == 0]
    neg = int(np.signbit(zeros).sum())
    assert neg > 0 and np.signbit(zeros[:neg]).all() and not np.signbit(zeros[neg:]).any()
