"""Host logic of the train step that needs neither a device nor the library: cutting a padded batch's outputs, the lazy
result mappings, the weight-gradient / unpack job tables as functions of integers.  (The collective policy's two-rank case is
in tests/test_dist_gloo.py.)"""
import pytest
import torch

from svs_hip import lib as _lib
from svs_hip import train
from svs_hip.trainer import _GroupedLosses, _GroupedOutputs, _ValidRays
from volsdf.model.network import cut_rays


def _same(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b)
    return a == b


def _padded_outputs(n_pad=16, S=5):
    g = torch.Generator().manual_seed(0)
    return {"rgb_values": torch.randn(n_pad, 3, generator=g), "weights": torch.randn(n_pad, S, generator=g),
            "xyz_flat": torch.randn(n_pad * S, 3, generator=g),                 # flattened rays x samples
            "grad_theta": torch.randn(2 * n_pad, 3, generator=g),               # two per-ray halves
            "scalar": torch.tensor(2.5), "note": "not a tensor", "odd": torch.randn(n_pad + 3, generator=g)}


@pytest.mark.parametrize("n_valid", [1, 15, 16])
def test_valid_rays_equals_cut_rays(n_valid):
    out = _padded_outputs(16)
    want = cut_rays(out, n_valid, 16)
    got = _ValidRays(out, n_valid, 16)
    assert list(want) == list(got)
    for k in want:
        assert _same(got[k], want[k]), k
    if n_valid < 16:
        assert got["rgb_values"].shape == (n_valid, 3) and got["xyz_flat"].shape == (n_valid * 5, 3)
        assert torch.equal(got["grad_theta"], torch.cat([out["grad_theta"][:n_valid], out["grad_theta"][16:16 + n_valid]]))
        assert got["odd"] is out["odd"] and got["scalar"] is out["scalar"]


def _lazy_cases():
    res = [({"loss": torch.tensor(1.0), "rgb_loss": torch.tensor(0.5), "n": 2},
            {"rgb_values": torch.zeros(3, 3), "weights": torch.ones(3, 4), "tag": "a", "s": torch.tensor(1.0)}),
           ({"loss": torch.tensor(2.0), "rgb_loss": torch.tensor(0.25), "n": 3},
            {"rgb_values": torch.ones(2, 3), "weights": torch.zeros(2, 4), "tag": "a", "s": torch.tensor(1.0)})]
    losses = {"loss": torch.tensor(3.0), "rgb_loss": torch.tensor(0.75), "n": 5}
    outputs = {"rgb_values": torch.cat([torch.zeros(3, 3), torch.ones(2, 3)]), "weights": torch.cat([torch.ones(3, 4), torch.zeros(2, 4)]),
               "tag": "a", "s": torch.tensor(1.0)}
    padded = _padded_outputs(16)
    return [(lambda: _GroupedLosses(res), losses), (lambda: _GroupedOutputs(res), outputs),
            (lambda: _ValidRays(padded, 9, 16), cut_rays(padded, 9, 16))]


@pytest.mark.parametrize("case", range(3))
def test_lazy_results_read_like_the_eager_dict(case):
    """every read of the mapping protocol sees every key, before any key has been made"""
    make, eager = _lazy_cases()[case]
    keys = list(eager)
    assert len(make()) == len(eager)
    assert list(iter(make())) == keys and list(make().keys()) == keys and list(make()) == keys
    lazy = make()
    assert all(k in lazy for k in keys) and "missing" not in lazy
    assert lazy.get("missing", 7) == 7 and lazy.get("missing") is None
    with pytest.raises(KeyError):
        lazy["missing"]
    items = make().items()
    assert [k for k, _ in items] == keys and all(_same(v, eager[k]) for k, v in items)
    assert all(_same(a, b) for a, b in zip(make().values(), eager.values())) and len(make().values()) == len(eager)
    assert all(_same(make().get(k), eager[k]) for k in keys)
    lazy = make()
    assert all(_same(lazy[k], eager[k]) for k in keys) and lazy[keys[0]] is lazy[keys[0]]      # formed once


# ---- job tables: the parent commit's formulas, restated -----------------------------------------------------------------
KBLOCK, KREC, LDW = 128 * 64, 64, 288


def _tiles(n):
    return ((n + 127) // 128) * 4


def _stride(n):
    return _tiles(n) * KBLOCK


def _rec(n, n_blocks, block):
    return n_blocks * _tiles(n) * KBLOCK + block * _tiles(n) * KREC


def _o(base, n_floats):
    return base + 4 * n_floats


# made-up, distinct, 4 KiB-aligned "device addresses"
A = {name: 0x7F0000000000 + i * 0x10000000 for i, name in enumerate(
    ("dWk", "dbk", "absmax", "row0", "zbuf", "feat", "rbuf", "abuf", "ubuf", "pebuf", "hbuf", "gbuf", "feat_bar"))}
WFIELDS = [f for f, _ in _lib.WGradJob._fields_]
UFIELDS = [f for f, _ in _lib.UnpackJob._fields_]


def _ref_wjob(scaled, slot, n_pts, amax, a0, sa0, b0, sb0, a1=None, sa1=0, b1=None, sb1=0, extra=None, sx=0, rec0=None, rec1=None):
    return dict(a0=a0, b0=b0, sa0=sa0, sb0=sb0, a1=a1, b1=b1, sa1=sa1, sb1=sb1, b_extra=extra, s_extra=sx, n_points=n_pts, ldw=LDW,
                dW=_o(A["dWk"], slot * 256 * LDW), db=_o(A["dbk"], slot * 256), absmax=_o(A["absmax"], amax) if scaled else None,
                rec0=rec0 if scaled else None, rec1=rec1 if scaled else None)


def _check_table(got, want, fields):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(fields)
        for f, x in zip(fields, g):
            assert x == w[f], (i, f, x, w[f])
        st = (_lib.WGradJob if fields is WFIELDS else _lib.UnpackJob)(*g)          # what the launch is handed
        assert all(getattr(st, f) == w[f] for f in fields), i


ACC = (A["dWk"], A["dbk"], A["absmax"])


@pytest.mark.parametrize("h2", [True, False], ids=["f16x2", "f32"])
@pytest.mark.parametrize("n_main,n_total", [(1568, 1600), (3104, 3168)], ids=["dtu16x98", "bg32x97"])
def test_foreground_wgrad_tables(n_main, n_total, h2):
    zbuf, feat, rbuf = A["zbuf"], A["feat"], A["rbuf"]
    LSm = _stride(n_main)
    want = [_ref_wjob(h2, 9, n_main, 1, zbuf, KBLOCK, feat, KBLOCK, extra=_o(rbuf, 4 * LSm), sx=1024, rec0=_o(zbuf, _rec(n_main, 5, 0)))]
    for l in range(1, 5):
        want.append(_ref_wjob(h2, 9 + l, n_main, 1, _o(zbuf, l * LSm), KBLOCK, _o(rbuf, (l - 1) * LSm), KBLOCK,
                              rec0=_o(zbuf, _rec(n_main, 5, l))))
    got = train.rgb_wgrad_table(n_main, h2, ACC, zbuf, feat, rbuf)
    _check_table(got, want, WFIELDS)
    assert all((j[14] is None, j[15] is None, j[16] is None) == (not h2, not h2, True) for j in got)

    abuf, ubuf, pebuf, hbuf, gbuf, fbar = (A[k] for k in ("abuf", "ubuf", "pebuf", "hbuf", "gbuf", "feat_bar"))
    LS = _stride(n_total)
    second = lambda l: dict(a1=_o(gbuf, l * LS), sa1=KBLOCK, b1=_o(ubuf, l * LS), sb1=KBLOCK, rec1=_o(ubuf, _rec(n_total, 9, l)))
    want = [_ref_wjob(h2, 0, n_total, 0, abuf, KBLOCK, pebuf, KBLOCK, rec0=_o(abuf, _rec(n_total, 8, 0)), **second(0))]
    for l in range(1, 8):
        want.append(_ref_wjob(h2, l, n_total, 0, _o(abuf, l * LS), KBLOCK, _o(hbuf, (l - 1) * LS), KBLOCK,
                              rec0=_o(abuf, _rec(n_total, 8, l)), **second(l)))
    want.append(_ref_wjob(h2, 8, n_main, 2, fbar, KBLOCK, _o(hbuf, 7 * LS), KBLOCK, rec0=_o(fbar, _rec(n_main, 1, 0))))
    got = train.sdf_wgrad_table(n_total, n_main, h2, ACC, abuf, ubuf, pebuf, hbuf, gbuf, fbar)
    _check_table(got, want, WFIELDS)
    assert all((j[14] is None) == (not h2) and (j[15] is None) == (not h2) for j in got)
    assert [j[16] is None for j in got] == [not h2] * 8 + [True]


@pytest.mark.parametrize("prec", ["f16x2", "f32"])
def test_background_wgrad_table(prec):
    """P = 32 rays x 32 inverse-sphere samples.  The background kernels publish maxima and records at either precision: the
    table does not depend on it (absmax and rec0 are never null here, rec1 always)."""
    P, BGRBUF = 1024, KBLOCK + 1024
    abuf, zbuf, fbar, hbuf, pebuf, rbuf, feat = (A[k] for k in ("abuf", "zbuf", "feat_bar", "hbuf", "pebuf", "rbuf", "feat"))
    LS, Z2, T = _stride(P), 2 * KBLOCK, _tiles(P)
    job = lambda slot, amax, a0, sa0, b0, sb0, rec0, extra=None, sx=0: _ref_wjob(True, slot, P, amax, a0, sa0, b0, sb0, rec0=rec0,
                                                                                  extra=extra, sx=sx)
    want = [job(0, 0, abuf, KBLOCK, pebuf, KBLOCK, _o(abuf, _rec(P, 8, 0)))]
    for l in range(1, 8):
        want.append(job(l, 0, _o(abuf, l * LS), KBLOCK, _o(hbuf, (l - 1) * LS), KBLOCK, _o(abuf, _rec(P, 8, l))))
    want.append(job(8, 2, fbar, KBLOCK, _o(hbuf, 7 * LS), KBLOCK, _o(fbar, _rec(P, 1, 0))))
    zrec = lambda b: _o(zbuf, 2 * T * KBLOCK + b * T * KREC)
    want.append(job(9, 1, zbuf, Z2, feat, KBLOCK, zrec(0), extra=_o(rbuf, KBLOCK), sx=BGRBUF))
    want.append(job(10, 1, _o(zbuf, KBLOCK), Z2, rbuf, BGRBUF, zrec(1)))
    got = train.bg_wgrad_table(P, ACC, abuf, zbuf, fbar, hbuf, pebuf, rbuf, feat)
    _check_table(got, want, WFIELDS)
    assert all(j[14] is not None and j[15] is not None and j[16] is None for j in got)


def _layers(shapes, weight_norm):
    """[(net, l, slot, rows, cols, v, g, gv, gg, gb)] with made-up addresses"""
    out, a = [], 0x7E0000000000
    for net, (base, dims) in enumerate(shapes):
        for l, (rows, cols) in enumerate(dims):
            ptrs = [a + 0x100000 * (5 * len(out) + i) for i in range(5)]
            v, g, gv, gg, gb = ptrs
            out.append((net, l, base + l, rows, cols, v, g if weight_norm else None, gv, gg if weight_norm else None, gb))
    return out


SDF_DIMS = [(256, 39), (256, 256), (256, 256), (217, 256), (256, 256), (256, 256), (256, 256), (256, 256), (257, 256)]
RGB_DIMS = [(256, 271), (256, 256), (256, 256), (256, 256), (3, 256)]
BG_SDF_DIMS = [(256, 84), (256, 256), (256, 256), (172, 256), (256, 256), (256, 256), (256, 256), (256, 256), (257, 256)]
BG_RGB_DIMS = [(128, 283), (3, 128)]


@pytest.mark.parametrize("which", ["finalize", "BgBackward.finalize"])
def test_unpack_tables(which):
    fg = which == "finalize"
    layers = _layers(((0, SDF_DIMS), (9, RGB_DIMS)) if fg else ((0, BG_SDF_DIMS), (9, BG_RGB_DIMS)), weight_norm=fg)
    skip_map, rgb0_map = (1, 2) if fg else (3, 4)
    want = []
    for net, l, slot, rows, cols, v, g, gv, gg, gb in layers:
        is_sdf = net == 0
        want.append(dict(dWk=_o(A["dWk"], slot * 256 * LDW), dbk=_o(A["dbk"], slot * 256), ldw=LDW,
                         map=skip_map if (is_sdf and l == 4) else (rgb0_map if (not is_sdf and l == 0) else 0),
                         rows=rows, cols=cols, row_off=1 if (is_sdf and l == 8) else 0, weight_v=v, weight_g=g,
                         row0=A["row0"] if (is_sdf and l == 8) else None, grad_v=gv, grad_g=gg, grad_b=gb))
    got = train.unpack_table(A["dWk"], A["dbk"], A["row0"], layers, (skip_map, rgb0_map))
    _check_table(got, want, UFIELDS)
    assert len(got) == (14 if fg else 11) and all((j[8] is None) == (not fg) and (j[11] is None) == (not fg) for j in got)


def test_model_layer_shapes_match_the_tables():
    """the shapes the unpack tables above were written for are the models' own"""
    from volsdf.model.network import VolSDFNetwork
    from volsdf.model.network_bg import VolSDFNetworkBG
    from volsdf.utils.conf import bmvs_model_conf, dtu_model_conf
    (sv, sg, _), (rv, rg, _) = VolSDFNetwork(dtu_model_conf()).mlp_params()
    assert [tuple(t.shape) for t in sv] == SDF_DIMS and [tuple(t.shape) for t in rv] == RGB_DIMS and sg and rg
    bg = VolSDFNetworkBG(bmvs_model_conf())
    (bw, _), (rw, _) = bg.bg_params()
    assert [tuple(t.shape) for t in bw] == BG_SDF_DIMS and [tuple(t.shape) for t in rw] == BG_RGB_DIMS
    assert (bg.samples_per_ray(), bg.ray_multiple()) == (97, 32)
    assert (VolSDFNetwork(dtu_model_conf()).samples_per_ray(), VolSDFNetwork(dtu_model_conf()).ray_multiple()) == (98, 16)
