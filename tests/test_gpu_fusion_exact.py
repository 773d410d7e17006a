"""Depth fusion on the GPU (csrc/svs_fusion.hip) against the ordered oracle, bit for bit, on every case of tests/fusion_cases.py.

The unit is compiled without fma contraction and holds only IEEE float64 / float32 operations in a stated order;
tests/test_fusion_cases_cpu.py shows that the ordered oracle equals the float64 oracle on the general-camera cases and that no
case outside the manufactured ties has a quantity within rounding of a threshold.  So every element of every output must be
EQUAL (NaN equal to NaN): no fraction of differing pixels, no tolerance.  Every case runs twice: through the C-ABI into
buffers pre-filled with a sentinel (an element the kernel does not write shows), and -- where the case is made of cameras --
through `svs_hip.fusion.fuse_view(..., per_source=True)`, which forms the matrices itself.  The module prints the number of
unequal elements per case and output (profiles/fusion_parity.txt is that table from one MI355X)."""
import os

import numpy as np
import pytest
import torch

import fusion_cases as fc

pytestmark = pytest.mark.gpu
SVS_EINVAL, SVS_ESHAPE = -1, -2
F32 = np.float32
SENT_F, SENT_B = -12345.5, 171
ROWS = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def parity_table():
    yield
    cols = fc.OUTPUTS
    print("\n\nunequal elements against the ordered oracle (C-ABI call / svs_hip.fusion.fuse_view; - = not produced)")
    print(f"{'case':30s} {'n_src':>5s} {'H x W':>9s} " + " ".join(f"{k[:12]:>12s}" for k in cols))
    for name, n_src, hw, abi, prod in ROWS:
        cells = [f"{abi.get(k, '-')}/{'-' if prod is None else prod.get(k, '-')}" for k in cols]
        print(f"{name:30s} {n_src:5d} {hw[0]:4d}x{hw[1]:<4d} " + " ".join(f"{c:>12s}" for c in cells))
    total = sum(v for _, _, _, abi, prod in ROWS for d in (abi, prod or {}) for v in d.values())
    print(f"{len(ROWS)} cases, {total} unequal elements in all")


def _t(a, dev, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


class Buffers:
    """device inputs of one raw case and sentinel-filled outputs for `svs_fuse_view` / `svs_fuse_points`"""

    def __init__(self, raw, dev, sent_f=SENT_F, sent_b=SENT_B):
        self.H, self.W = raw["ref_depth"].shape
        H, W = self.H, self.W
        self.n_src = n = len(raw["src_depths"])
        self.ref, self.confidence = _t(raw["ref_depth"], dev, F32), _t(raw["confidence"], dev, F32)
        self.srcs = [_t(s, dev, F32) for s in raw["src_depths"]]
        self.mats = _t(np.asarray(raw["mats"], np.float64).reshape(n, 68) if n else np.zeros((1, 68)), dev)
        self.pmats = _t(np.asarray(raw["pmats"], np.float64), dev)
        self.img = _t(raw["img"], dev, F32)
        self.extra = _t(raw["extra_mask"], dev, np.uint8)
        self.conf, self.fdist, self.fdiff = float(raw["conf"]), float(raw["filter_dist"]), float(raw["filter_diff"])
        self.thres = int(raw["thres_view"])
        full = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=dev)
        self.out = dict(depth_avg=full((H, W), torch.float64, sent_f), photo_mask=full((H, W), torch.uint8, sent_b),
                        geo_mask=full((H, W), torch.uint8, sent_b), final_mask=full((H, W), torch.uint8, sent_b),
                        src_mask=full((n, H, W), torch.uint8, sent_b), src_depth_reproj=full((n, H, W), torch.float32, sent_f),
                        src_x=full((n, H, W), torch.float32, sent_f), src_y=full((n, H, W), torch.float32, sent_f))
        self.ws = full((H * W,), torch.int32, -7)
        self.xyz, self.rgb = full((H * W, 3), torch.float32, sent_f), full((H * W, 3), torch.uint8, sent_b)
        self.count = full((1,), torch.int32, -7)
        self.sent_f, self.sent_b = sent_f, sent_b

    def view_args(self, **over):
        from svs_hip.ops import _ptr, _ptr_array, _stream
        o = self.out
        a = dict(ref=_ptr(self.ref), confidence=_ptr(self.confidence), srcs=_ptr_array(self.srcs), mats=_ptr(self.mats),
                 n_src=self.n_src, H=self.H, W=self.W, conf=self.conf, fdist=self.fdist, fdiff=self.fdiff, thres=self.thres,
                 extra=_ptr(self.extra), depth_avg=_ptr(o["depth_avg"]), photo_mask=_ptr(o["photo_mask"]),
                 geo_mask=_ptr(o["geo_mask"]), final_mask=_ptr(o["final_mask"]), src_mask=_ptr(o["src_mask"]),
                 src_depth_reproj=_ptr(o["src_depth_reproj"]), src_x=_ptr(o["src_x"]), src_y=_ptr(o["src_y"]), stream=_stream())
        a.update(over)
        return tuple(a.values())

    def point_args(self, **over):
        from svs_hip.ops import _ptr, _stream
        a = dict(depth_avg=_ptr(self.out["depth_avg"]), final_mask=_ptr(self.out["final_mask"]), img=_ptr(self.img),
                 pmats=_ptr(self.pmats), H=self.H, W=self.W, ws=_ptr(self.ws), xyz=_ptr(self.xyz), rgb=_ptr(self.rgb),
                 count=_ptr(self.count), stream=_stream())
        a.update(over)
        return tuple(a.values())

    def untouched(self):
        torch.cuda.synchronize()
        fl = all(bool((self.out[k] == self.sent_f).all()) for k in ("depth_avg", "src_depth_reproj", "src_x", "src_y"))
        by = all(bool((self.out[k] == self.sent_b).all()) for k in ("photo_mask", "geo_mask", "final_mask", "src_mask"))
        pt = bool((self.xyz == self.sent_f).all()) and bool((self.rgb == self.sent_b).all()) and bool((self.ws == -7).all())
        return fl and by and pt and int(self.count.item()) == -7

    def run(self, L):
        """both entries -> numpy outputs; rows of xyz / rgb beyond the count must still hold the sentinel"""
        assert L.svs_fuse_view(*self.view_args()) == 0, L.svs_last_error_string()
        assert L.svs_fuse_points(*self.point_args()) == 0, L.svs_last_error_string()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in self.out.items()}
        n = int(self.count.item())
        assert 0 <= n <= self.H * self.W
        xyz, rgb = self.xyz.cpu().numpy(), self.rgb.cpu().numpy()
        assert (xyz[n:] == F32(self.sent_f)).all() and (rgb[n:] == self.sent_b).all()
        got["xyz"] = xyz[:n]
        if self.img is not None:
            got["rgb"] = rgb[:n]
        return got


def _unequal(got, want):
    return {k: fc.n_unequal(got[k], want[k]) for k in fc.OUTPUTS if k in want}


@pytest.mark.parametrize("name", fc.case_names())
def test_every_output_equals_the_ordered_oracle(dev, name):
    from svs_hip import fusion, lib
    c = fc.case(name)
    want = c["want"]
    abi = _unequal(Buffers(c["raw"], dev).run(lib.load()), want)
    prod = None
    if "ref" in c:
        out = fusion.fuse_view(c["ref"], c["srcs"], per_source=True, **c["kw"])
        prod = _unequal({k: v.cpu().numpy() for k, v in out.items()}, want)
    ROWS.append((name, len(c["raw"]["src_depths"]), c["raw"]["ref_depth"].shape, abi, prod))
    print(f"{name}: C-ABI {abi}; fuse_view {prod}")
    assert set(abi) == set(fc.OUTPUTS) and not any(abi.values()), abi
    assert prod is None or (set(prod) == set(fc.OUTPUTS) and not any(prod.values())), prod


@pytest.mark.parametrize("name", ["remapB-3x257-poison", "nsrc16-257x17", "special-depths", "points-17x241-ragged"])
def test_a_repeat_run_is_bit_identical(dev, name):
    from svs_hip import lib
    raw = fc.case(name)["raw"]
    a = Buffers(raw, dev).run(lib.load())
    b = Buffers(raw, dev, sent_f=777.25, sent_b=90).run(lib.load())          # other sentinels: nothing of them may show
    assert set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_rejected_fuse_view_calls_write_nothing(dev):
    from svs_hip import lib
    from svs_hip.ops import _ptr_array
    L = lib.load()
    raw = fc.case("set25x31-ref0")["raw"]
    two = dict(raw, src_depths=raw["src_depths"] * 2, mats=np.concatenate([raw["mats"], raw["mats"]]))
    b = Buffers(two, dev)

    def rejected(code, **over):
        assert L.svs_fuse_view(*b.view_args(**over)) == code, over
        assert b"svs_fuse_view" in L.svs_last_error_string(), over

    for k in ("ref", "confidence", "srcs", "mats", "depth_avg", "photo_mask", "geo_mask", "final_mask"):
        rejected(SVS_EINVAL, **{k: None})
    rejected(SVS_EINVAL, srcs=_ptr_array([b.srcs[0], None]))
    assert b"source depth 1" in L.svs_last_error_string()
    for n in (-1, 17):
        rejected(SVS_ESHAPE, n_src=n)
    for h, w in ((0, b.W), (b.H, 0), (-3, b.W), (b.H, -1), (0, 0)):
        rejected(SVS_ESHAPE, H=h, W=w)
    # sizes whose product does not fit the int pixel index: refused before any launch
    for h, w in ((46341, 46341), (65536, 65536), (2147483647, 2), (1, 2147483647)):
        rejected(SVS_ESHAPE, H=h, W=w)
        assert b"exceeds" in L.svs_last_error_string()
    for k in ("src_depth_reproj", "src_x", "src_y"):                          # per-source outputs come as a set
        rejected(SVS_EINVAL, **{k: None})
    assert b.untouched()
    want = fc.ordered_fuse_mats(**two)
    got = b.run(L)
    assert not any(_unequal(got, want).values())


def test_rejected_fuse_points_calls_write_nothing(dev):
    from svs_hip import lib
    L = lib.load()
    raw = fc.case("points-3x85-ragged")["raw"]
    b = Buffers(raw, dev)
    assert L.svs_fuse_view(*b.view_args()) == 0
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in b.out.items()}

    def rejected(code, **over):
        assert L.svs_fuse_points(*b.point_args(**over)) == code, over
        assert b"svs_fuse_points" in L.svs_last_error_string(), over

    for k in ("depth_avg", "final_mask", "pmats", "ws", "xyz", "count", "rgb"):   # (rgb: required once an image is given)
        rejected(SVS_EINVAL, **{k: None})
    for h, w in ((0, b.W), (b.H, 0), (-3, b.W), (b.H, -1)):
        rejected(SVS_ESHAPE, H=h, W=w)
    for h, w in ((46341, 46341), (65536, 65536), (2147483647, 2)):
        rejected(SVS_ESHAPE, H=h, W=w)
        assert b"exceeds" in L.svs_last_error_string()
    torch.cuda.synchronize()
    assert bool((b.xyz == SENT_F).all()) and bool((b.rgb == SENT_B).all()) and bool((b.ws == -7).all())
    assert int(b.count.item()) == -7 and all(torch.equal(before[k], b.out[k]) for k in before)
    want = fc.case("points-3x85-ragged")["want"]
    assert not any(_unequal(b.run(L), want).values())
    # without an image no colour buffer is needed, and none is written
    b2 = Buffers(dict(raw, img=None), dev)
    got = b2.run(L)
    assert fc.same(got["xyz"], want["xyz"]) and "rgb" not in got and bool((b2.rgb == SENT_B).all())
