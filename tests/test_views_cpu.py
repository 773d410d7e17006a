"""svs_hip.views without a GPU: the layout of a view's matrices, the bounds of the launch chunks, the mask rules with each
caller's exception type and name, the evaluation-mask options of the command lines, and the line of seconds."""
import argparse

import numpy as np
import pytest
import torch

from svs_hip import images, views

CPU = torch.device("cpu")


def test_view_matrices_layout_and_shape_error():
    K = np.arange(9, dtype=np.float32).reshape(3, 3) + 100
    E = np.arange(16, dtype=np.float32).reshape(4, 4)
    m = views.view_matrices(K, E)
    assert m.dtype == np.float64 and m.shape == (21,)
    assert m[:9].tolist() == [100 + i for i in range(9)] and m[9:].tolist() == list(range(12))       # the last row of E is left out
    for bad_K, bad_E in ((K[:2], E), (K, E[:3]), (K.reshape(-1), E)):
        with pytest.raises(ValueError, match=r"K \(3,3\) and E \(4,4\)"):
            views.view_matrices(bad_K, bad_E)
    d = views.mats([dict(K=K, E=E), dict(K=2 * K, E=E)], CPU)
    assert d.dtype == torch.float64 and tuple(d.shape) == (2, 21) and d.is_contiguous()
    assert np.array_equal(d[1].numpy(), views.view_matrices(2 * K, E))


@pytest.mark.parametrize("n, want", [(0, []), (1, [(0, 1)]), (16, [(0, 16)]), (17, [(0, 16), (16, 17)]),
                                     (33, [(0, 16), (16, 32), (32, 33)])])
def test_chunks_bounds(n, want):
    assert views.MAX_VIEWS == 16
    vs = [dict(K=np.eye(3) * (i + 1), E=np.eye(4)) for i in range(n)]
    got = list(views.chunks(vs, CPU))
    assert [(at, to) for at, to, _ in got] == want
    for at, to, m in got:
        assert tuple(m.shape) == (to - at, 21) and m[:, 0].tolist() == [float(i + 1) for i in range(at, to)]


def test_device_masks_rules():
    assert views.device_masks(None, 3, 2, 3, CPU, "svs_mesh_paint") is None
    given = [np.array([[0, 2, -1], [0, 0, 255]], np.int16), None, np.array([[0.0, 0.5, -0.0], [np.nan, 1e-30, 0.0]]),
             torch.tensor([[True, False, False], [False, False, True]])]
    out = views.device_masks(given, 4, 2, 3, CPU, "svs_mesh_paint")
    assert out[1] is None and all(m.dtype == torch.uint8 and m.is_contiguous() for m in out if m is not None)
    assert out[0].tolist() == [[0, 1, 1], [0, 0, 1]] and out[2].tolist() == [[0, 1, 0], [1, 1, 0]]
    assert out[3].tolist() == [[1, 0, 0], [0, 0, 1]]


@pytest.mark.parametrize("name, error", [("svs_mesh_vertex_visibility", ValueError), ("svs_mesh_paint", ValueError),
                                         ("svs_tsdf_integrate", AssertionError)])
def test_device_masks_errors_are_the_callers(name, error):
    with pytest.raises(error, match=name + ".*mask"):
        views.device_masks([np.ones((2, 3)), np.ones((3, 2))], 2, 2, 3, CPU, name, error)
    with pytest.raises(error, match=name + ".*1 masks for 2 views"):
        views.device_masks([None], 2, 2, 3, CPU, name, error)


def test_eval_mask_args_come_together(capsys):
    p = argparse.ArgumentParser()
    views.add_eval_mask_args(p, "cut every view by its evaluation mask")
    for argv in (["--data-dir-root", "d"], ["--dataset", "DTU"]):
        with pytest.raises(SystemExit):
            views.check_eval_mask_args(p, p.parse_args(argv))
        assert "--data-dir-root and --dataset come together" in capsys.readouterr().err
    for argv in ([], ["--data-dir-root", "d", "--dataset", "BlendedMVS"]):
        views.check_eval_mask_args(p, p.parse_args(argv))
    with pytest.raises(SystemExit):
        p.parse_args(["--dataset", "other"])


def test_seconds_line_is_the_head_of_phases_summary():
    ph = images.Phases(names=("read", "kernels"))
    ph.s["read"], ph.s["kernels"] = 1.23456, 0.0004
    assert images.seconds_line(ph.s) == "seconds: read 1.235, kernels 0.000"
    assert ph.summary(2.0).split(", total")[0] == images.seconds_line(ph.s)
    assert views.launches_since(dict(a=5, b=2), dict(a=3, b=2)) == dict(a=2, b=0)
