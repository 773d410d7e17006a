"""The claim of csrc/svs_views.h on the GPU: a point lands on the same pixel in the TSDF volume, the visibility test and
the painter, at half-pixel ties, where separate copies of the rule would part first.

One view of 4 x 5 pixels, E the identity, K = [[2,0,.5],[0,2,.5],[0,0,1]]: a point (a/4, b/4, 1) projects to ((a+1)/2,
(b+1)/2), an exact half-integer or integer in float32 and float64.  Six points: two on a tie in x, two on a tie in y, two on
none (for those, rounding half down picks the rule's own pixel, so their second launch repeats the first).  Per point two
launches of each unit, with a mask that is zero at one pixel only: the pixel of floor(x + 0.5), floor(y + 0.5), then the
pixel that rounding half down would pick.  What every one of the six points must do under either mask follows from the
integer arithmetic below, not from the code under test."""
import numpy as np
import pytest
import torch

from svs_hip import lib, meshpaint, meshview, tsdf
from svs_hip import views as svs_views

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 4, 5
ORIGIN = (1, 1)                                              # in quarters: the first point is (0.25, 0.25, 1)
NODES = [(0, 0), (1, 0), (3, 0), (0, 1), (2, 3), (4, 2)]     # (i, j) of the six points in the volume


def test_one_pixel_rule_at_half_pixel_ties():
    quarters = [(ORIGIN[0] + i, ORIGIN[1] + j) for i, j in NODES]
    halves = [(a + 1, b + 1) for a, b in quarters]                                   # the projection in half pixels
    rule = [((u + 1) // 2, (v + 1) // 2) for u, v in halves]                         # floor(x + 0.5): a tie goes up
    down = [(u // 2, v // 2) for u, v in halves]                                     # ceil(x - 0.5): a tie goes down
    assert [u % 2 for u, _ in halves] == [0, 1, 1, 0, 0, 0] and [v % 2 for _, v in halves] == [0, 0, 0, 1, 1, 0]
    assert all(0 <= x < W and 0 <= y < H for x, y in rule + down)

    view = dict(K=np.array([[2, 0, 0.5], [0, 2, 0.5], [0, 0, 1.0]]), E=np.eye(4))
    verts = torch.tensor([[a / 4, b / 4, 1.0] for a, b in quarters], dtype=torch.float32, device=DEV)
    mats = svs_views.mats([view], DEV)
    depth = torch.ones((1, H, W), dtype=torch.float32, device=DEV)
    image = [torch.full((H, W, 3), 200, dtype=torch.uint8, device=DEV)]
    for p in range(len(NODES)):
        for zero in (rule[p], down[p]):
            mask = torch.ones((H, W), dtype=torch.uint8, device=DEV)
            mask[zero[1], zero[0]] = 0
            off_want = [int(r == zero) for r in rule]
            seen_want = [1 - o for o in off_want]
            assert off_want[p] == int(zero == rule[p])                               # hidden by the first mask; by the second only off a tie
            seen = torch.zeros(len(NODES), dtype=torch.int32, device=DEV)
            off = torch.zeros_like(seen)
            lib.check(meshview.visibility_raw(verts, mats, 1, H, W, depth, [mask], 0.01, 0.0, seen, off), "svs_mesh_vertex_visibility")
            assert seen.tolist() == seen_want and off.tolist() == off_want, (p, zero)
            acc = torch.zeros((len(NODES), 4), dtype=torch.float64, device=DEV)
            lib.check(meshpaint.paint_raw(verts, None, mats, 1, H, W, depth, image, [mask], acc), "svs_mesh_paint")
            assert acc[:, 3].tolist() == [float(s) for s in seen_want], (p, zero)
            vol = tsdf.Volume((ORIGIN[0] / 4, ORIGIN[1] / 4, 1.0), (5, 4, 1), 0.25, trunc=1.0, colors=False)
            vol.integrate([dict(K=view["K"], E=view["E"], depth=depth[0], mask=mask)])
            assert [float(vol.weight[i, j, 0]) for i, j in NODES] == [float(s) for s in seen_want], (p, zero)
