"""What svs_hip/scans.py knows about a scan, without a GPU: the one registry behind the BlendedMVS id tables and folder
names (hand registration, the JSON file SVS_SCENE_IDS names, the reference checkout, in that order, field by field), the
single compile of the reference's functions, and the opening of a scan folder against what the two dataset classes
expose for it."""
import builtins
import json
import os

import numpy as np
import pytest

import mvsdata_oracle as mo

REFERENCE = os.environ.get("SVOLSDF_REFERENCE_ROOT", "/root/reference")
F8, F10 = "0123456789abcdef01234567", "fedcba9876543210fedcba98"     # made-up folder names
IDS9 = dict(train=[4, 1, 2], eval=[0, 3], near={str(i): [4, 1, 2][i % 3] for i in range(6)})
IDS10 = dict(train=[5, 0, 3], train_interp=[3, 0, 5], eval=[1, 2, 4], near={"1": 5, "2": 0, "4": 3}, hash=F10)


@pytest.fixture()
def scans(monkeypatch, tmp_path):
    """the module with an empty registry, no reference checkout, and the mixed file in the environment"""
    from svs_hip import scans as sc
    saved = dict(sc._BMVS)
    sc._BMVS.clear()
    table = tmp_path / "ids.json"
    table.write_text(json.dumps({"BlendedMVS": {"8": {"hash": F8}, "9": IDS9, "10": IDS10}}))
    monkeypatch.setenv("SVS_SCENE_IDS", str(table))
    monkeypatch.setattr(sc, "_REF_FUNCS", {})
    monkeypatch.setattr(sc, "_IDS_READ", None)
    yield sc
    sc._BMVS.clear()
    sc._BMVS.update(saved)


def test_a_mixed_json_file(scans, monkeypatch):
    table, opens, real_open = os.environ["SVS_SCENE_IDS"], [], builtins.open

    def counting_open(file, *a, **kw):
        if str(file) == table:
            opens.append(file)
        return real_open(file, *a, **kw)
    monkeypatch.setattr(builtins, "open", counting_open)
    assert scans.scan2hash("scan8") == F8
    with pytest.raises(LookupError, match="register_blendedmvs_hash"):
        scans.scan2hash("scan9")
    assert scans.scan2hash("scan10") == F10
    with pytest.raises(LookupError, match="register_blendedmvs_hash"):
        scans.scan2hash("scan11")
    assert len(opens) <= 1                                       # the folder names: one open of the file at most
    n = len(opens)
    with pytest.raises(LookupError, match="register_blendedmvs_ids"):      # not a KeyError: the entry has no "eval"
        scans.get_eval_ids("BlendedMVS", 8)
    with pytest.raises(LookupError, match="register_blendedmvs_ids"):
        scans.get_trains_ids("BlendedMVS", "scan8", 3)
    with pytest.raises(LookupError, match="register_blendedmvs_ids"):
        scans.get_near_id("BlendedMVS", 8, 0)
    assert scans.get_trains_ids("BlendedMVS", "scan9", 3) == [4, 1, 2]
    assert scans.get_trains_ids("BlendedMVS", "scan9", 3, for_interp=True) == [4, 1, 2]
    assert scans.get_eval_ids("BlendedMVS", 9) == [0, 3] and scans.get_near_id("BlendedMVS", 9, 5) == 2
    assert scans.get_trains_ids("BlendedMVS", "scan10", 3) == [5, 0, 3]
    assert scans.get_trains_ids("BlendedMVS", "scan10", 3, for_interp=True) == [3, 0, 5]
    assert scans.get_eval_ids("BlendedMVS", "10") == [1, 2, 4] and scans.get_near_id("BlendedMVS", 10, 4) == 3
    assert len(opens) - n <= 1                                   # the id tables: likewise
    with pytest.raises(AssertionError):                          # the reference's assert
        scans.get_trains_ids("BlendedMVS", "scan10", 4)


def test_the_ids_are_asked_first(scans):
    """the other order of the two lookup families over the same file"""
    assert scans.get_eval_ids("BlendedMVS", 9) == [0, 3]
    with pytest.raises(LookupError, match="register_blendedmvs_ids"):
        scans.get_eval_ids("BlendedMVS", 8)
    assert scans.scan2hash("scan8") == F8 and scans.scan2hash("scan10") == F10


def test_a_hand_registration_is_not_overwritten(scans):
    from svs_hip import mvsdata, scene
    assert scene.register_blendedmvs_ids is scans.register_blendedmvs_ids and scene.get_eval_ids is scans.get_eval_ids
    assert scene.get_trains_ids is scans.get_trains_ids and scene.get_near_id is scans.get_near_id
    assert mvsdata.scan2hash is scans.scan2hash and mvsdata.register_blendedmvs_hash is scans.register_blendedmvs_hash
    mvsdata.register_blendedmvs_hash(8, "by-hand")               # before the file is read
    scene.register_blendedmvs_ids(10, train=[2, 1, 4], eval=[5], near={5: 2})
    assert scans.scan2hash("scan10") == F10                      # the file fills what nobody registered
    assert scans.scan2hash("scan8") == "by-hand"
    assert scans.get_trains_ids("BlendedMVS", "scan10", 3) == [2, 1, 4] and scans.get_eval_ids("BlendedMVS", 10) == [5]
    assert scans.get_trains_ids("BlendedMVS", "scan10", 3, for_interp=True) == [2, 1, 4]
    assert scans.get_near_id("BlendedMVS", 10, 5) == 2
    scans.register_blendedmvs_hash(10, "later")                  # and a later registration replaces the file's value
    assert scans.scan2hash("scan10") == "later" and scans.get_eval_ids("BlendedMVS", 10) == [5]


@pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "volsdf", "vsdf.py")),
                    reason=f"needs a checkout of the reference at {REFERENCE} (SVOLSDF_REFERENCE_ROOT)")
def test_the_reference_file_is_compiled_once(scans, monkeypatch):
    monkeypatch.setenv("SVOLSDF_REFERENCE_ROOT", REFERENCE)
    monkeypatch.delenv("SVS_SCENE_IDS")
    monkeypatch.setattr(scans, "_REF_FUNCS", None)
    parses, real_parse = [], scans.ast.parse

    def counting_parse(*a, **kw):
        parses.append(a[1:])
        return real_parse(*a, **kw)
    monkeypatch.setattr(scans.ast, "parse", counting_parse)
    train = scans.get_trains_ids("BlendedMVS", "scan3", 3)
    assert len(train) == 3 and len(scans.get_eval_ids("BlendedMVS", 3)) == 12
    assert scans.get_near_id("BlendedMVS", 3, 0) in train and len(scans.scan2hash("scan3")) == 24
    assert len(parses) == 1 and set(scans._reference_functions()) == {"get_trains_ids", "get_eval_ids", "get_near_id",
                                                                      "scan2hash"}


@pytest.mark.parametrize("own_cameras", [True, False])
def test_open_scan_is_what_both_datasets_open(monkeypatch, tmp_path, own_cameras):
    from svs_hip import mvsdata, scans, scene
    root, n = str(tmp_path), 4
    mvs = mo.write_mvs_scan(root, "DTU", 24, n, (40, 64), {0: [1, 2], 1: [0, 2], 2: [1, 0], 3: [0, 1]},
                            own_cameras=own_cameras)                     # scene_oracle.write_scan's folder plus the pair file
    inst, image_dir, cam_file, paths = scans.open_scan(root, "DTU", 24)
    assert inst == os.path.join(root, "DTU", "scan24") and image_dir == f"{inst}/image"
    assert ("scan114" in cam_file) == (not own_cameras) and os.path.isfile(cam_file)
    assert paths == sorted(paths) and [os.path.basename(p) for p in paths] == [f"{i:06d}.png" for i in range(n)]
    scale_mats, world_mats = scans.read_cameras(cam_file, n)
    assert len(scale_mats) == len(world_mats) == n
    assert all(m.dtype == np.float32 and m.shape == (4, 4) for m in scale_mats + world_mats)
    cams = np.load(cam_file)
    assert all(np.array_equal(scale_mats[i], cams[f"scale_mat_{i}"].astype(np.float32)) and
               np.array_equal(world_mats[i], cams[f"world_mat_{i}"].astype(np.float32)) for i in range(n))

    # the image work is not this test's subject
    monkeypatch.setattr(scene, "_cached_images", lambda *a, **kw: ([], [], [], True, False))
    sd = scene.SceneDataset("DTU", (20, 32), scan_id=24, num_views=3, data_dir_root=root)
    md = mvsdata.MVSDataset(mvs, ["scan24"], "test", 3, "DTU", 8, 1.06, max_h=32, max_w=64, trains_i=[2, 0, 1],
                            args=dict(data_dir_root=root))
    assert sd.cam_file == cam_file and sd.n_images == n and md.image_paths_idr == paths
    assert sd.scale_factor == scale_mats[0][0, 0] and md.scale_factor == scale_mats[0][0, 0]
    assert type(sd.scale_factor) is np.float32 and np.array_equal(md.scale_mat, scale_mats[0])
    want = [scene.load_K_Rt_from_P((w @ s)[:3, :4])[1] for s, w in zip(scale_mats, world_mats)]
    assert all(np.array_equal(p.numpy(), q) for p, q in zip(sd.pose_all, want))
    assert all(np.array_equal(p, scene.load_K_Rt_from_P(w[:3, :4])[1]) for p, w in zip(md.pose_idr, world_mats))
