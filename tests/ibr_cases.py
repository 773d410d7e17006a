"""TEST INFRASTRUCTURE ONLY -- the inputs of tests/test_gpu_ibr_edges.py and a definition-level reference of the
Laplacian pyramids, built here so that tests/test_ibr_cpu.py can examine exactly the same arrays without a GPU.  numpy only;
torch is imported inside the two C-ABI helpers at the bottom.

  * pyr_down_def / pyr_up_def / blend_def: cv2.pyrDown, cv2.pyrUp and Laplacian_Blending from their definition in float64
    (zero injection, BORDER_REFLECT_101 on the grid the filter runs on, a dense 25-tap sum).  No edge rule is written out:
    ibr_oracle.pyr_up and csrc/svs_ibr.hip both restate the same closed forms, these functions derive them another way.
  * blend_f32: the same blend with every stored array rounded to float32 -- what float32 storage alone costs.
  * BLEND_CASES / blend_case: sizes whose coarsest level is 1x1, 1x2, 2x1, 1x3, 3x1, odd, or crosses a 256-thread block.
  * weights_case: the inputs of svs_ibr_weights written directly (no cameras): map values on every limit of cubic_tap,
    geometric-mask holes on the image border and on the erosion's 16-pixel seams.
"""
import numpy as np

import ibr_oracle as io_

F32 = np.float32
F64 = np.float64
K5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
NUM_LEVELS = io_.NUM_LEVELS


# ---------------------------------------------------------------------------------------------------------------------
# the pyramids from their definition
# ---------------------------------------------------------------------------------------------------------------------
def pyr_down_def(img):
    """cv2.pyrDown: the 5x5 kernel [1 4 6 4 1]^2 / 256 centred on the even rows and columns of the source, the source
    indexed with BORDER_REFLECT_101.  (H,W[,C]) -> ((H+1)//2, (W+1)//2[,C]) float64."""
    img = np.asarray(img, F64)
    H, W = img.shape[:2]
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    out = np.zeros((h2, w2) + img.shape[2:])
    for dy in range(5):
        yy = io_.reflect101(2 * np.arange(h2) - 2 + dy, H)
        for dx in range(5):
            xx = io_.reflect101(2 * np.arange(w2) - 2 + dx, W)
            out += (K5[dy] * K5[dx]) * img[yy][:, xx]
    return out / 256.0


def pyr_up_def(img):
    """cv2.pyrUp: zeros injected to (2h, 2w) (the source at the even rows and columns), then the 5x5 kernel times 4 / 256
    at every pixel of that grid, the grid indexed with BORDER_REFLECT_101.  (h,w[,C]) -> (2h, 2w[,C]) float64."""
    img = np.asarray(img, F64)
    h, w = img.shape[:2]
    z = np.zeros((2 * h, 2 * w) + img.shape[2:])
    z[0::2, 0::2] = img
    out = np.zeros_like(z)
    for dy in range(5):
        yy = io_.reflect101(np.arange(2 * h) - 2 + dy, 2 * h)
        for dx in range(5):
            xx = io_.reflect101(np.arange(2 * w) - 2 + dx, 2 * w)
            out += (K5[dy] * K5[dx]) * z[yy][:, xx]
    return out * (4.0 / 256.0)


def _blend(fill, masks, down, up, store):
    """Laplacian_Blending (simple_ibr.py:112-136) with four levels: fill (n+1,H,W,3), masks (n+1,H,W) -> (H,W,3).
    `store` is applied to every array the computation keeps."""
    fill, masks = np.asarray(fill, F64), np.asarray(masks, F64)
    assert fill.shape == masks.shape + (3,)
    LS = [0.0] * NUM_LEVELS
    for img, m in zip(fill, masks):
        gi, gm = [store(img)], [store(m)]
        for _ in range(NUM_LEVELS - 1):
            gi.append(store(down(gi[-1])))
            gm.append(store(down(gm[-1])))
        for lvl in range(NUM_LEVELS):                   # LS[0] is the coarsest level, as in the reference
            g = NUM_LEVELS - 1 - lvl
            lap = gi[g] if lvl == 0 else store(gi[g] - store(up(gi[g + 1])))
            LS[lvl] = store(LS[lvl] + gm[g][..., None] * lap)
    out = LS[0]
    for lvl in range(1, NUM_LEVELS):
        out = store(store(up(out)) + LS[lvl])
    return store(np.clip(out, 0.0, 1.0))


def blend_def(fill, masks):
    """The blend in float64, built only from pyr_down_def and pyr_up_def."""
    return _blend(fill, masks, pyr_down_def, pyr_up_def, lambda a: a)


def blend_f32(fill, masks):
    """The blend from the oracle's closed forms with every stored array rounded to float32 (-> float64 values that are
    float32 numbers).  |blend_f32 - blend_def| is the yardstick of the GPU bound."""
    return _blend(fill, masks, io_.pyr_down, io_.pyr_up, lambda a: np.asarray(a, F64).astype(F32).astype(F64))


ULP1 = float(np.spacing(F32(1.0)))                       # 1.19e-7


def blend_bound(fill, masks, ref=None):
    """-> (bound, yardstick): 10 x max|blend_f32 - blend_def| on these inputs, at least 4 float32 ulps at 1.0.  The factor
    covers the kernel's float32 arithmetic inside each 25-tap sum and its own, fixed operation order."""
    ref = blend_def(fill, masks) if ref is None else ref
    yard = float(np.abs(blend_f32(fill, masks) - ref).max())
    return max(10.0 * yard, 4 * ULP1), yard


# ---------------------------------------------------------------------------------------------------------------------
# blend cases
# ---------------------------------------------------------------------------------------------------------------------
# (H, W, n_src, kind).  Level 3 is 1x1, 1x2, 2x1 | 1x3, 3x1 (odd levels) | 2x2 | 3x5, 5x3 | 1x33: pyrDown and the level
# kernels cross a 256-thread block with a ragged tail on a one-row coarse level.
BLEND_CASES = (
    (8, 8, 1, "random"), (8, 8, 16, "onehot"), (8, 8, 2, "constant"), (8, 8, 16, "clip"),
    (8, 16, 1, "onehot"), (8, 16, 2, "random"),
    (16, 8, 2, "onehot"), (16, 8, 1, "clip"),
    (8, 24, 1, "random"), (8, 24, 16, "clip"),
    (24, 8, 2, "random"), (24, 8, 16, "onehot"),
    (16, 16, 1, "constant"), (16, 16, 2, "clip"),
    (24, 40, 2, "onehot"), (24, 40, 16, "random"),
    (40, 24, 1, "clip"), (40, 24, 2, "random"),
    (8, 264, 16, "random"), (8, 264, 1, "onehot"), (8, 264, 2, "constant"),
)
CONSTANT = 0.375


def case_id(c):
    return "-".join(str(v) for v in c)


def blend_case(H, W, n_src, kind):
    """-> fill (n_src+1,H,W,3) float32, masks (n_src+1,H,W) float32.
      random    fill uniform in [0, 1], masks uniform and normalised to sum 1 over the entries
      onehot    per pixel one entry has mask 1, the entries in a checkerboard: the largest Laplacian content at every level
      constant  every fill image is 0.375 (a float32 number whose pyramid sums are exact), so the blend is 0.375
      clip      fill in [-0.5, 1.5] and masks with one dominant entry per pixel, so that the final clip acts on a large
                share of the pixels (asserted here on the float64 reference: above 10 %)"""
    rng = np.random.default_rng([H, W, n_src, len(kind)])
    nj = n_src + 1
    fill = rng.uniform(0, 1, (nj, H, W, 3))
    masks = rng.uniform(0, 1, (nj, H, W))
    if kind == "onehot":
        y, x = np.mgrid[0:H, 0:W]
        masks = ((y + x) % nj == np.arange(nj)[:, None, None]).astype(F64)
    elif kind == "constant":
        fill = np.full_like(fill, CONSTANT)
    elif kind == "clip":
        fill = fill * 2.0 - 0.5
        masks = masks ** 12
    else:
        assert kind == "random", kind
    masks = masks / masks.sum(0, keepdims=True)
    fill, masks = fill.astype(F32), masks.astype(F32)
    if kind == "clip":
        ref = blend_def(fill, masks)                        # only the clip produces exactly 0 or 1
        share = float(((ref == 0.0) | (ref == 1.0)).mean())
        assert share > 0.10, (H, W, n_src, share)
    return fill, masks


# ---------------------------------------------------------------------------------------------------------------------
# weights cases
# ---------------------------------------------------------------------------------------------------------------------
WEIGHTS_CASES = ((8, 8, 1), (16, 24, 4), (24, 40, 2), (24, 16, 16), (8, 40, 16))
HIGH_SOURCES_ON = (8, 40, 16)                # the case whose four consistent sources are 12..15, not 0..3
SEAM = 16                                    # the erosion's tile
REF_DIR = np.array([0.0, 0.6, 0.8], F32)


TOL = 1e-5                                   # the unit's bound: float32 kernels against the reference's float64 pyramids
REACH = 32                                   # the pyramid's reach from a flipped threshold (tests/test_gpu_ibr.py)


def dilate(mask, r):
    """Chebyshev dilation of a boolean (H,W) mask by r pixels."""
    m = np.asarray(mask, bool)
    for ax in (0, 1):
        c = np.cumsum(np.pad(m, [(r + 1, r) if a == ax else (0, 0) for a in (0, 1)]).astype(np.int32), axis=ax)
        hi = np.take(c, np.arange(2 * r + 1, c.shape[ax]), axis=ax)
        lo = np.take(c, np.arange(0, c.shape[ax] - 2 * r - 1), axis=ax)
        m = (hi - lo) > 0
    return m


def near_threshold(weights):
    """pixels whose weight of some source lies within 1e-6 of 0.2"""
    return (np.abs(weights[:-1].astype(F64) - 0.2) < 1e-6).any(0)


def tap_mode(mx, my, H, W):
    """cubic_tap's mode per map value in integer arithmetic: 0 wholly outside (or non-finite / beyond int), 1 all sixteen
    taps inside, 2 partly outside."""
    fx, fy = (np.asarray(mx, F32) * F32(32.0)).astype(F32), (np.asarray(my, F32) * F32(32.0)).astype(F32)
    with np.errstate(invalid="ignore"):
        bad = ~((fx > -2.1e9) & (fx < 2.1e9) & (fy > -2.1e9) & (fy < 2.1e9))
    sx = np.clip(np.rint(np.where(bad, 0, fx)).astype(np.int64) >> 5, -32768, 32767) - 1
    sy = np.clip(np.rint(np.where(bad, 0, fy)).astype(np.int64) >> 5, -32768, 32767) - 1
    out = bad | (sx >= W) | (sx + 4 <= 0) | (sy >= H) | (sy + 4 <= 0)
    ins = (sx >= 0) & (sx < W - 3) & (sy >= 0) & (sy < H - 3)
    return np.where(out, 0, np.where(ins, 1, 2))


def limit_values(n):
    """The crafted map values along an axis of length n, by name.  At a whole number the outermost taps have weight 0, so
    -2 and n do not tell a window that is "partly outside" from one "wholly outside"; -1.75 and n + 0.5 do: the last window
    on either side whose single in-image tap has a non-zero weight."""
    v = [("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("+1e12", 1e12), ("-1e12", -1e12), ("+7e7", 7e7),
         ("-7e7", -7e7), ("+40000", 40000.0), ("-40000", -40000.0)]
    v += [(str(x), x) for x in (-0.25, -1.0, -1.75, -2.0, -3.0, -3.5)]
    v += [("n%+g" % d, n + d) for d in (-4.0, -3.5, -3.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0)]
    return v


TIE_EVEN, TIE_ODD = 6, 9                     # (k + 0.5) / 32: x * 32 = k + 0.5 exactly; half-to-even gives 6 and 10


def crafted_entries(H, W):
    """[(name, x or None, y or None)]: None keeps the identity coordinate of the pixel the entry lands on."""
    e = [("x=" + n, v, None) for n, v in limit_values(W)] + [("y=" + n, None, v) for n, v in limit_values(H)]
    # x and y partly outside together, at both corners; the other diagonal too
    e += [("corner00", -0.25, -0.25), ("cornerHW", W - 0.5, H - 0.5), ("corner0W", W - 1.0, -2.0), ("cornerH0", -2.0, H - 1.0)]
    ix, iy = 2, 2                            # an interior sample point: all sixteen taps inside at every size
    e += [("tie", ix + (TIE_EVEN + 0.5) / 32, iy + (TIE_ODD + 0.5) / 32), ("tie'", ix + (TIE_ODD + 0.5) / 32, iy + (TIE_EVEN + 0.5) / 32)]
    e += [("2+1/64", 2 + 1.0 / 64, 2 + 1.0 / 64)]
    for k in range(32):                      # every phase in x and, permuted, in y
        e.append(("phase%d" % k, 1 + k % (W - 3) + k / 32.0, 1 + (3 * k) % (H - 3) + ((7 * k + 3) % 32) / 32.0))
    return e


def hole_positions(H, W):
    """[(name, y, x)]: single-pixel holes of the geometric masks."""
    my, mx = H // 2, W // 2
    h = [("corner", 0, 0), ("corner", 0, W - 1), ("corner", H - 1, 0), ("corner", H - 1, W - 1),
         ("edge", 0, mx), ("edge", H - 1, mx), ("edge", my, 0), ("edge", my, W - 1),
         ("edge+2", 0, 2), ("edge+3", 0, 3), ("edge+2", 2, W - 1), ("edge+3", 3, W - 1)]
    rows = [r for r in (5, H - 3, my) if 0 <= r < H]
    for s in range(SEAM, W, SEAM):           # x seams: both sides, then the halo's last column and one past it
        for i, d in enumerate((-1, 0, 1, -2, -3, 2, 3)):
            if 0 <= s + d < W:
                h.append(("seamx%+d" % d, rows[i % len(rows)], s + d))
    cols = [c for c in (5, W - 3, mx) if 0 <= c < W]
    for s in range(SEAM, H, SEAM):
        for i, d in enumerate((-1, 0, 1, -2, -3, 2, 3)):
            if 0 <= s + d < H:
                h.append(("seamy%+d" % d, s + d, cols[i % len(cols)]))
    return h


_CACHE = {}


def weights_case(H, W, n_src, seed=0):
    """The inputs of svs_ibr_weights, no cameras involved, and the oracle's result on them.  -> dict(imgs, dirs (n,H,W,3),
    ref_dir, pred (H,W,3), geo (n,H,W) uint8, x2d, y2d (n,H,W) float32; on: the consistent sources; holes [(name, source, y,
    x)]; crafted, planted (n,H,W) bool: pixels with a crafted map / inside a planted direction window; crafted_names; mode (n,H,W); n_nan, n_anti; weights, fill, masks: ibr_oracle.weights_stage).

    Directions: every source direction field and the reference direction are one unit vector, so cos_dir is 1 wherever
    the sampled window has weight; a planted all-zero window gives 0/0 -> NaN -> 0, a planted antiparallel one gives -1.
    Geometric masks: at most four sources are on at a pixel (weights about 1/k >= 0.25, well off the 0.2 threshold: five
    would sit a hair under it); the others are 0 everywhere.  Maps: the identity, with crafted_entries() written over a
    block of source 0 and of the last source.  The 8x8 case has one source and 64 pixels: it takes the limits, the corners,
    the ties and 2 + 1/64, leaves the 32 phases and the two off-diagonal corners to the other four cases, and has no hole inside its clean 3x3 corner.
    The case asserts on the oracle's result that no weight is within 1e-6 of the threshold and that no sampled direction
    is a cancellation residue, so the GPU comparison may take every pixel and excuse none."""
    key = (H, W, n_src, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng([H, W, n_src, seed])
    imgs = (rng.integers(0, 256, (n_src, H, W, 3)).astype(F32) / F32(255.0))
    pred = (rng.integers(0, 256, (H, W, 3)).astype(F32) / F32(255.0))
    dirs = np.broadcast_to(REF_DIR, (n_src, H, W, 3)).copy()
    ref_dir = np.broadcast_to(REF_DIR, (H, W, 3)).copy()
    k = min(n_src, 4)
    on = tuple(range(n_src - k, n_src)) if (H, W, n_src) == HIGH_SOURCES_ON else tuple(range(k))
    # planted direction windows, 2x2, on the last two rows (no crafted window straddles their edge symmetrically)
    planted = np.zeros((n_src, H, W), bool)
    planted[on[0], H - 2:H, 1:3] = planted[on[-1], H - 2:H, W - 3:W - 1] = True
    dirs[on[0], H - 2:H, 1:3] = 0.0
    dirs[on[-1], H - 2:H, W - 3:W - 1] = -REF_DIR
    # pixels that keep the identity and their geometric mask.  64 pixels cannot hold the crafted values and a clean 5x5
    # window: the top-left 3x3 stays clean there, which is pixel (0, 0)'s whole in-image neighbourhood -- it survives the
    # erosion exactly when "outside the image takes no part" holds
    tiny = H * W <= 64
    clean = np.zeros((H, W), bool)
    if tiny:
        clean[:3, :3] = True
    else:
        clean[0] = True
    geo = np.zeros((n_src, H, W), np.uint8)
    geo[list(on)] = 1
    holes = []
    for i, (name, y, x) in enumerate(p for p in hole_positions(H, W) if not (tiny and clean[p[1], p[2]])):
        s = on[i % k]
        geo[s, y, x] = 0
        holes.append((name, s, y, x))
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    x2d, y2d = np.tile(xx, (n_src, 1, 1)), np.tile(yy, (n_src, 1, 1))
    crafted = np.zeros((n_src, H, W), bool)
    entries = crafted_entries(H, W)
    slots = np.argwhere(~clean)
    if tiny:
        entries = [e for e in entries if not e[0].startswith("phase") and e[0] not in ("corner0W", "cornerH0")]
    assert len(entries) <= len(slots)
    for s in sorted({0, n_src - 1}):
        for (y, x), (_, vx, vy) in zip(slots, entries):
            crafted[s, y, x] = True
            if vx is not None:
                x2d[s, y, x] = vx
            if vy is not None:
                y2d[s, y, x] = vy
    mode = tap_mode(x2d, y2d, H, W)
    # bookkeeping on the sampled directions: exactly zero (NaN -> 0) or of clear length, never a cancellation residue
    n_nan = n_anti = 0
    for s in range(n_src):
        sd = io_.remap_cubic(dirs[s], x2d[s], y2d[s]).astype(F64)
        nrm = np.linalg.norm(sd, axis=2)
        assert np.all((nrm == 0) | (nrm > 1e-3)), (H, W, n_src, s)
        ident = ~crafted[s]
        n_nan += int(((nrm == 0) & ident).sum())
        n_anti += int((((sd * REF_DIR).sum(2) < 0) & ident).sum())
    w, fill, m = io_.weights_stage(imgs, dirs, ref_dir, pred, geo, x2d, y2d)
    assert np.isfinite(w).all() and np.isfinite(fill).all() and np.isfinite(m).all()
    assert near_threshold(w).sum() == 0
    assert np.abs(w[:-1].astype(F64) - 0.2).min() > 0.04, "a weight is not clearly on one side of the threshold"
    case = dict(imgs=imgs, dirs=dirs, ref_dir=ref_dir, pred=pred, geo=geo, x2d=x2d, y2d=y2d, on=on, holes=holes,
                crafted=crafted, planted=planted, crafted_names=[e[0] for e in entries], mode=mode, n_nan=n_nan, n_anti=n_anti,
                weights=w, fill=fill, masks=m[..., 0])
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[key] = case
    return case


# ---------------------------------------------------------------------------------------------------------------------
# the workspace of csrc/svs_ibr.hip, from its layout comment
# ---------------------------------------------------------------------------------------------------------------------
ALIGN = 256


def _up(b):
    return (b + ALIGN - 1) // ALIGN * ALIGN


def workspace_planes(n_src, H, W):
    """Bytes of the planes the layout comment lists: softmax weights (n+1,H,W) f32, w > 0.2 (n,H,W) u8, for levels 1..3 the
    image planes (n+1,h,w,3) f32 and mask planes (n+1,h,w) f32, the reconstructions of levels 2 and 1 (h,w,3) f32."""
    nj = n_src + 1
    b = nj * H * W * 4 + n_src * H * W
    for lvl in (1, 2, 3):
        b += nj * (H >> lvl) * (W >> lvl) * 16
    for lvl in (1, 2):
        b += (H >> lvl) * (W >> lvl) * 12
    return b


def thr_offset(n_src, H, W):
    """Byte offset of the w > 0.2 plane: it follows the weights, each plane aligned to 256 bytes."""
    return _up((n_src + 1) * H * W * 4)


# ---------------------------------------------------------------------------------------------------------------------
# the two stages through the C-ABI (GPU tests only)
# ---------------------------------------------------------------------------------------------------------------------
def run_weights(L, srcs_img, src_dirs, ref_dir, pred, geo, x2d, y2d, dev, return_thr=False):
    """svs_ibr_weights -> fill (n+1,H,W,3), masks (n+1,H,W); with return_thr also the workspace's w > 0.2 (n,H,W) uint8."""
    import torch
    from svs_hip.ops import _ptr, _ptr_array, _stream
    n, H, W = geo.shape
    t = lambda a, dt=torch.float32: torch.from_numpy(np.array(a, order="C")).to(dev, dt)   # noqa: E731  (a copy: cases are read-only)
    imgs, dirs = [t(a) for a in srcs_img], [t(a) for a in src_dirs]
    rd, pr, g, mx, my = t(ref_dir), t(pred), t(np.asarray(geo, np.uint8), torch.uint8), t(x2d), t(y2d)
    ws = torch.empty(int(L.svs_ibr_workspace_bytes(n, H, W)), dtype=torch.uint8, device=dev)
    fill = torch.empty(n + 1, H, W, 3, device=dev)
    masks = torch.empty(n + 1, H, W, device=dev)
    rc = L.svs_ibr_weights(_ptr_array(imgs), _ptr_array(dirs), _ptr(rd), _ptr(pr), _ptr(g), _ptr(mx), _ptr(my), n, H, W,
                           _ptr(ws), _ptr(fill), _ptr(masks), _stream())
    assert rc == 0
    if return_thr:
        o = thr_offset(n, H, W)
        assert o + n * H * W <= ws.numel()
        return fill.cpu().numpy(), masks.cpu().numpy(), ws[o:o + n * H * W].cpu().numpy().reshape(n, H, W)
    return fill.cpu().numpy(), masks.cpu().numpy()


def run_blend(L, fill, masks, dev):
    """svs_ibr_laplacian_blend -> (H,W,3) float32."""
    import torch
    from svs_hip.ops import _ptr, _stream
    n1, H, W = masks.shape
    f = torch.from_numpy(np.ascontiguousarray(fill, F32)).to(dev)
    m = torch.from_numpy(np.ascontiguousarray(masks, F32)).to(dev)
    ws = torch.empty(int(L.svs_ibr_workspace_bytes(n1 - 1, H, W)), dtype=torch.uint8, device=dev)
    out = torch.empty(H, W, 3, device=dev)
    assert L.svs_ibr_laplacian_blend(_ptr(f), _ptr(m), n1 - 1, H, W, _ptr(ws), _ptr(out), _stream()) == 0
    return out.cpu().numpy()
