"""The fp16x2 weight-gradient GEMM's index maps (csrc/svs_wgrad.hip, csrc/svs_wgrad_maps.h): which dW entry a (row, column,
point) product lands in, which point a factor is applied to, ragged and multi-item launches, the narrow job, and
deterministic mode.  What random operands at one scale can average away is pinned here with one-hot operands (exact) and
with per-point scales 2^40 apart; the bounds are those of test_wgrad_gemm (test_gpu_backward.py)."""
import ctypes

import numpy as np
import pytest
import torch

import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
ST = 128 * 64          # floats per block slot


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from svs_hip import lib
    return lib.load()


def G(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _launch(L, jobs, precision):
    from svs_hip import lib
    arr = (lib.WGradJob * len(jobs))(*jobs)
    lib.check(L.svs_wgrad_multi(ctypes.cast(arr, ctypes.c_void_p), len(jobs), precision,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


# ---------------------------------------------------------------------------------------------------------------------
# one-hot placement
# ---------------------------------------------------------------------------------------------------------------------
# (row, column, point): a row in each 16-row block of several waves, columns in the first, middle and last 16-column tiles,
# one point from each of the eight point quads
PICKS = [(5, 3, 1), (27, 121, 6), (100, 255, 11), (250, 130, 12), (81, 16, 18), (200, 77, 21), (143, 240, 26), (36, 15, 31)]
VA, VB = 1.5, -2.25     # exact in fp16, and so is everything the kernel forms from them


def _one_hot(L, dev, precision, P, row, col, pt_a, pt_b):
    from svs_hip import lib
    A = np.zeros((P, 256), F32); A[pt_a, row] = VA
    B = np.zeros((P, 256), F32); B[pt_b, col] = VB
    a, rec, _ = synth.rows_to_scaled_block(A, scaled=False, pair=precision == 1)      # unit scales, through the factor path
    b = synth.rows_to_pair_block(B)
    ta, tb, tr = G(a, dev), G(b, dev), G(rec, dev)
    am = torch.tensor([VA], dtype=torch.float32, device=dev)
    dW = torch.zeros(256, 256, device=dev)
    _launch(L, [lib.WGradJob(_ptr(ta), _ptr(tb), ST, ST, None, None, ST, ST, None, 0, P, 256, _ptr(dW), None, _ptr(am),
                             _ptr(tr), None)], precision)
    return dW.cpu().numpy()


@pytest.mark.parametrize("precision", [1, 2])
def test_one_hot_placement(dev, L, precision):
    """A non-zero in one (row, point), B in one (column, same point): dW is that product at (row, column) and 0 elsewhere."""
    cases = [(32, r, c, p) for r, c, p in PICKS] + [(64, 27, 121, 32 + 13)]
    for P, row, col, pt in cases:
        got = _one_hot(L, dev, precision, P, row, col, pt, pt)
        want = np.zeros((256, 256), F32); want[row, col] = VA * VB
        assert np.array_equal(got, want), (P, row, col, pt, np.argwhere(got != 0)[:8].tolist())
    # a point of A never meets another point of B: the neighbour in the quad, the same place in the next quad and in the
    # other read of the fragment
    for pt_b in (7, 10, 14, 22):
        got = _one_hot(L, dev, precision, 32, 27, 121, 6, pt_b)
        assert not got.any(), (pt_b, np.argwhere(got != 0)[:8].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# per-point factors
# ---------------------------------------------------------------------------------------------------------------------
# exponent place of point p: the permutation (11 p + 7) mod 32, written out
PERM = [7, 18, 29, 8, 19, 30, 9, 20, 31, 10, 21, 0, 11, 22, 1, 12, 23, 2, 13, 24, 3, 14, 25, 4, 15, 26, 5, 16, 27, 6, 17, 28]
assert sorted(PERM) == list(range(32))


def _operands(precision, A0, B0, A1, B1, dev):
    """as test_gpu_backward._operands (fp16x2): device blocks, records, and the values the blocks hold"""
    pair = precision == 1
    a0, r0, A0q = synth.rows_to_scaled_block(A0, pair=pair)
    b0 = synth.rows_to_pair_block(B0)
    a1, _, A1q = synth.rows_to_scaled_block(A1, scaled=False, pair=pair)
    b1, r1, B1q = synth.rows_to_scaled_block(B1, pair=pair)
    h = B0.astype(np.float16)
    B0q = h.astype(F32) + ((B0 - h.astype(F32)).astype(np.float16).astype(F32) if pair else 0.0)
    return [G(x, dev) for x in (a0, b0, a1, b1)], (G(r0, dev), G(r1, dev)), (A0q, B0q, A1q, B1q)


@pytest.mark.parametrize("precision", [1, 2])
@pytest.mark.parametrize("P", [32, 33])
def test_per_point_factors(dev, L, P, precision):
    """The scaled operands (A of pair 0, B of pair 1) at a different power of two per point, 2^-30 ... 2^10, in an order
    unrelated to the point index: a factor applied to a neighbouring point is an error of order 1."""
    from svs_hip import lib
    rng = np.random.default_rng(100 + P)
    expo = np.array([round(-30 + 40 * PERM[p % 32] / 31) for p in range(P)], np.float64)
    assert expo.min() == -30 and expo.max() == 10
    scale_a = (2.0 ** expo).astype(F32)[:, None]
    scale_b = (2.0 ** expo[::-1]).astype(F32)[:, None]          # pair 1: the same set of scales, on other points
    A0, B0 = (scale_a * rng.normal(0, 1, (P, 256))).astype(F32), rng.normal(0, 1, (P, 256)).astype(F32)
    A1, B1 = rng.normal(0, 1, (P, 256)).astype(F32), (scale_b * rng.normal(0, 1, (P, 256))).astype(F32)
    absmax = torch.tensor([max(np.abs(A0).max(), np.abs(B1).max())], dtype=torch.float32, device=dev)
    (ta0, tb0, ta1, tb1), (r0, r1), (A0q, B0q, A1q, B1q) = _operands(precision, A0, B0, A1, B1, dev)
    dW = torch.zeros(256, 256, device=dev); db = torch.zeros(256, device=dev)
    _launch(L, [lib.WGradJob(_ptr(ta0), _ptr(tb0), ST, ST, _ptr(ta1), _ptr(tb1), ST, ST, None, 0, P, 256, _ptr(dW), _ptr(db),
                             _ptr(absmax), _ptr(r0), _ptr(r1))], precision)
    ref = A0q.astype(np.float64).T @ B0q + A1q.astype(np.float64).T @ B1q
    e_w, e_b = rel_err(dW.cpu().numpy(), ref), rel_err(db.cpu().numpy(), A0q.astype(np.float64).sum(0))
    print("P %d precision %d  dW %.3g  db %.3g" % (P, precision, e_w, e_b))
    assert e_w < 2e-5
    assert e_b < 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# ragged, multi-item, narrow; deterministic mode
# ---------------------------------------------------------------------------------------------------------------------
P_BIG = 32 * 257 + 5        # more point tiles than workgroups, and a ragged tail

_big_cache = {}


def _big(precision, dev):
    """Operands and float64 references of the big launches, built once per precision and left unchanged."""
    if precision not in _big_cache:
        rng = np.random.default_rng(9)
        P = P_BIG
        A0, B0 = (1e-6 * rng.normal(0, 1, (P, 256))).astype(F32), rng.normal(0, 1, (P, 256)).astype(F32)
        A1, B1 = rng.normal(0, 1, (P, 256)).astype(F32), (1e-6 * rng.normal(0, 1, (P, 256))).astype(F32)
        X = rng.normal(0, 1, (P, 32)).astype(F32); X[:, 16:] = 0
        ts, recs, (A0q, B0q, A1q, B1q) = _operands(precision, A0, B0, A1, B1, dev)
        xt = synth.rows_to_tiles(np.concatenate([X, np.zeros((P, 224), F32)], 1)).reshape(-1, ST)[:, :1024].copy()
        am1 = torch.tensor([np.abs(A0).max()], dtype=torch.float32, device=dev)
        am2 = torch.tensor([max(np.abs(A0).max(), np.abs(B1).max())], dtype=torch.float32, device=dev)
        A64 = A0q.astype(np.float64)
        ref1 = A64.T @ B0q
        _big_cache[precision] = dict(t=ts, rec=recs, x=G(xt, dev), am1=am1, am2=am2, ref1=ref1,
                                     ref2=ref1 + A1q.astype(np.float64).T @ B1q, refx=A64.T @ X[:, :16], refb=A64.sum(0))
    return _big_cache[precision]


def _big_jobs(d, dev):
    """job 0: one pair + the narrow job (16 extra rows, ldw 288) + db; job 1: two pairs + db"""
    from svs_hip import lib
    (ta0, tb0, ta1, tb1), (r0, r1) = d["t"], d["rec"]
    out = [(torch.zeros(256, 288, device=dev), torch.zeros(256, device=dev)) for _ in range(2)]
    jobs = [lib.WGradJob(_ptr(ta0), _ptr(tb0), ST, ST, None, None, ST, ST, _ptr(d["x"]), 1024, P_BIG, 288, _ptr(out[0][0]),
                         _ptr(out[0][1]), _ptr(d["am1"]), _ptr(r0), None),
            lib.WGradJob(_ptr(ta0), _ptr(tb0), ST, ST, _ptr(ta1), _ptr(tb1), ST, ST, None, 0, P_BIG, 288, _ptr(out[1][0]),
                         _ptr(out[1][1]), _ptr(d["am2"]), _ptr(r0), _ptr(r1))]
    return jobs, out


@pytest.mark.parametrize("precision", [1, 2])
def test_ragged_multi_item(dev, L, precision):
    d = _big(precision, dev)
    jobs, out = _big_jobs(d, dev)
    _launch(L, jobs[:1], precision)       # each job with all the workgroups: several items per workgroup
    _launch(L, jobs[1:], precision)
    (dW1, db1), (dW2, db2) = [(w.cpu().numpy(), b.cpu().numpy()) for w, b in out]
    errs = (rel_err(dW1[:, :256], d["ref1"]), rel_err(dW1[:, 256:272], d["refx"]), rel_err(db1, d["refb"]),
            rel_err(dW2[:, :256], d["ref2"]), rel_err(db2, d["refb"]))
    print("precision %d  one pair %.3g  narrow %.3g  db %.3g  two pairs %.3g  db %.3g" % ((precision,) + errs))
    assert max(errs) < 2e-5
    assert not dW1[:, 272:].any()         # the narrow tile's rows 16..31 are zero
    assert not dW2[:, 256:].any()         # no narrow job: nothing beyond column 255


def test_deterministic_mode_repeats(dev, L):
    """The multi-job launch twice into zeroed buffers in deterministic mode: bit-equal."""
    d = _big(1, dev)
    was = L.svs_set_deterministic(1)
    try:
        runs = []
        for _ in range(2):
            jobs, out = _big_jobs(d, dev)
            _launch(L, jobs, 1)
            runs.append([t.cpu().numpy() for pair in out for t in pair])
    finally:
        L.svs_set_deterministic(was)
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    assert rel_err(runs[0][0][:, :256], d["ref1"]) < 2e-5 and rel_err(runs[0][2][:, :256], d["ref2"]) < 2e-5
