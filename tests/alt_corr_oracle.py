"""Host-side reference of the on-the-fly ("alternate") correlation (csrc/alt_corr.hip,
csrc/alt_corr_bwd.hip), independent of the library: numpy on the CPU only.

alt_ref            the forward: sample position x / coord_div in fp32 as the kernels compute it, floor
                   and fraction (x - floor(x), in fp32) from that value, dot products and the four-term
                   blend in fp64.
                   Returns (bins, mag): mag is the same blend over sum_c |f1_c * f2_c| per tap, the
                   quantity every rounding error of the computation is relative to.
alt_ref_levels     all levels in the l*(2r+1)^2 channel order, both coordinate layouts.
alt_bwd_ref        the three gradients as explicit sums (no autograd), with their magnitudes.
f16x3_split        the documented split hi = f16(x), lo = f16(x - hi).
f16x3_restatement  alt_ref's taps from the three kept products hi*hi + lo*hi + hi*lo, summed in fp64.
check              |got - ref| <= bound * mag element by element, NaN exactly where the reference has it.

The coordinate contract (include/raft_hip.h, every kernel form):
  finite coordinate, however large   taps off fmap2 are 0; a window wholly off the map gives bins of
                                     exactly +-0; flow_out = coords - grid in fp32.
  non-finite on either axis          (after the division) every bin of that query at that level NaN.
  backward                           a query with a non-finite coordinate or |coordinate| >= 1e8
                                     contributes nothing; its coords_grad is (0, 0).

Bounds (measured on the CPU against alt_ref by test_alt_corr_oracle_host.py, never
against the kernels), in units of 2^-24 * mag:
  GAMMA32        largest error of a float32 restatement of the documented algorithm
                 (oracle.raft_oracle.alt_corr_forward on float32 inputs, and alt_ref(dtype=float32):
                 the kernels' sequential four-term blend) over the GPU tests' own inputs.
  gamma16x3(s)   the same for f16x3_restatement at map scale s, plus GAMMA32 for the fp32 accumulation.
  GAMMA_BWD      the same for alt_bwd_ref(dtype=float32).
The kernels are held to 4 x these (the margin covers the different summation order: 64-lane
butterflies and MFMA accumulators against einsum)."""
import numpy as np

U24 = 2.0 ** -24
NAN_BITS = 0x7FC00ABC          # the NaN every output is prefilled with (tests compare the bits)
BIG = 1e8                      # the backward's (and the tile kernels' box) "absent query" threshold

# measured by test_alt_corr_oracle_host.py::test_bound_measurement (which asserts they still cover
# the float32 restatements); see DESIGN.md 7.3 for the table
GAMMA32 = 3.5                  # measured 3.33
GAMMA_BWD = 4.25               # measured 4.17
# measured 69.4, 4.38, 1.22, 1.16: the unscaled lo = f16(x - hi) is an f16 subnormal below |x| ~ 2^-3
GAMMA16X3 = {2.0 ** -8: 70.0, 2.0 ** -4: 4.5, 1.0: 1.25, 2.0 ** 6: 1.25}


def bound32():
    return 4 * GAMMA32 * U24


def bound16x3(scale=1.0):
    return 4 * (GAMMA16X3[scale] + GAMMA32) * U24


def bound_bwd():
    return 4 * GAMMA_BWD * U24


# ----------------------------------------------------------------------------- forward


def positions(coords, coord_div):
    """fp32 sample position, its floor (int64, clamped: a huge finite coordinate stays far off any
    map), the fractions position - floor in fp32 as the kernels and the reference kernel subtract them
    (exact except for a position in (-1, 0), where the fraction near 1 rounds to 2^-24: the weight
    1 - fraction of such a query is the documented algorithm's, not its fp64 ideal) and the finite mask;
    coords [..., 2]."""
    f = np.float32
    with np.errstate(all="ignore"):
        p = np.asarray(coords, f) / f(coord_div)
        assert p.dtype == np.float32
        fin = np.isfinite(p[..., 0]) & np.isfinite(p[..., 1])
        ps = np.where(np.isfinite(p), p, f(0))
        fl = np.floor(ps)
        d = (ps - fl).astype(f)
        i = np.clip(fl, -2.0 ** 40, 2.0 ** 40).astype(np.int64)
    return p, i, d, fin


def _taps(f1, f2, b, ix0, iy0, r, dt, absolute=False):
    """s[q, iy, ix] = <f1[b, q], f2[b, y0 + iy, x0 + ix]> (0 off the map), in dt; f1 [B, P, C]."""
    _, H2, W2, _ = f2.shape
    wd = 2 * r + 2
    a = f1[b].astype(dt)
    if absolute:
        a = np.abs(a)
    s = np.zeros((a.shape[0], wd, wd), dt)
    for iy in range(wd):
        h2 = iy0 + iy
        for ix in range(wd):
            w2 = ix0 + ix
            ok = (h2 >= 0) & (h2 < H2) & (w2 >= 0) & (w2 < W2)
            t = f2[b, np.clip(h2, 0, H2 - 1), np.clip(w2, 0, W2 - 1)].astype(dt)
            if absolute:
                t = np.abs(t)
            s[:, iy, ix] = np.where(ok, np.einsum("pc,pc->p", a, t), 0)
    return s


def _blend(s, dx, dy, rd, dt):
    """o[q, oy, ox]: the kernels' sequential four-term blend, in dt."""
    one = dt(1)
    dx, dy = dx.astype(dt)[:, None, None], dy.astype(dt)[:, None, None]
    o = s[:, :rd, :rd] * ((one - dy) * (one - dx))
    o = o + s[:, :rd, 1:] * ((one - dy) * dx)
    o = o + s[:, 1:, :rd] * (dy * (one - dx))
    o = o + s[:, 1:, 1:] * (dy * dx)
    return o


def alt_ref(f1, f2, coords, r, coord_div=1.0, scale_div=1.0, dtype=np.float64, taps=None):
    """f1 [B,H1,W1,C], f2 [B,H2,W2,C], coords [B,N,H1,W1,2] -> (bins, mag), both
    [B,N,(2r+1)^2,H1,W1] (channel oy + (2r+1)*ox).  dtype=np.float32 is the float32 restatement of the
    same algorithm (its mag stays fp64).  taps: a function (f1, f2, b, x0, y0, r) -> s replacing the dot
    products (f16x3_restatement)."""
    B, H1, W1, C = f1.shape
    N = coords.shape[1]
    rd = 2 * r + 1
    P = H1 * W1
    f1p = f1.reshape(B, P, C)
    out = np.zeros((B, N, rd * rd, H1, W1), dtype)
    mag = np.zeros((B, N, rd * rd, H1, W1), np.float64)
    _, i, d, fin = positions(coords, coord_div)
    with np.errstate(all="ignore"):
        for b in range(B):
            for n in range(N):
                x0 = i[b, n, ..., 0].reshape(-1) - r
                y0 = i[b, n, ..., 1].reshape(-1) - r
                dx, dy = d[b, n, ..., 0].reshape(-1), d[b, n, ..., 1].reshape(-1)
                s = (taps(f1p, f2, b, x0, y0, r) if taps else _taps(f1p, f2, b, x0, y0, r, dtype))
                o = _blend(s, dx, dy, rd, dtype) / dtype(np.float32(scale_div))
                m = _blend(_taps(f1p, f2, b, x0, y0, r, np.float64, True), dx, dy, rd, np.float64)
                m = m / np.float64(np.float32(scale_div))
                bad = ~fin[b, n].reshape(-1)
                o[bad] = np.nan
                m[bad] = np.nan
                out[b, n] = o.transpose(2, 1, 0).reshape(rd * rd, H1, W1)   # channel = oy + rd*ox
                mag[b, n] = m.transpose(2, 1, 0).reshape(rd * rd, H1, W1)
    return out, mag


def alt_ref_levels(f1, f2_levels, coords, r, scale_div=1.0, coords_layout=0, dtype=np.float64, taps=None):
    """raft_alt_corr_lookup_levels: coords [B,H1,W1,2] (layout 0) or [B,2,H1,W1] (layout 1), level l
    reads f2_levels[l] at coords / 2^l -> (bins, mag) [B, L*(2r+1)^2, H1, W1]."""
    c = np.asarray(coords, np.float32)
    if coords_layout == 1:
        c = c.transpose(0, 2, 3, 1)
    outs, mags = [], []
    for l, f2 in enumerate(f2_levels):
        o, m = alt_ref(f1, f2, c[:, None], r, float(2 ** l), scale_div, dtype, taps)
        outs.append(o[:, 0])
        mags.append(m[:, 0])
    return np.concatenate(outs, 1), np.concatenate(mags, 1)


def flow_ref(coords):
    """flow_out of the lookups: coords - grid in fp32; coords [B,H1,W1,2]."""
    B, H1, W1, _ = coords.shape
    ys, xs = np.meshgrid(np.arange(H1, dtype=np.float32), np.arange(W1, dtype=np.float32), indexing="ij")
    with np.errstate(all="ignore"):
        return (np.asarray(coords, np.float32) - np.stack([xs, ys], -1)[None]).astype(np.float32)


# ----------------------------------------------------------------------------- f16x3


def f16x3_split(x):
    """(hi, lo) = (f16(x), f16(x - hi)) as am_split_store computes them (unscaled lo, round to nearest,
    f16 subnormals kept)."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def f16x3_restatement(f1, f2, coords, r, coord_div=1.0, scale_div=1.0):
    """alt_ref with every dot product replaced by sum_c (h1 h2 + l1 h2 + h1 l2) in fp64: its distance
    from alt_ref is the split's own error (the dropped l1 l2 and the roundings of hi and lo)."""
    h1, l1 = (v.astype(np.float64) for v in f16x3_split(f1))
    h2, l2 = (v.astype(np.float64) for v in f16x3_split(f2))
    B, H1, W1, C = f1.shape

    def taps(_f1p, _f2, b, x0, y0, rr):
        a, al = h1.reshape(B, -1, C), l1.reshape(B, -1, C)
        return (_taps(a, h2, b, x0, y0, rr, np.float64) + _taps(al, h2, b, x0, y0, rr, np.float64)
                + _taps(a, l2, b, x0, y0, rr, np.float64))

    return alt_ref(f1, f2, coords, r, coord_div, scale_div, np.float64, taps)


# ----------------------------------------------------------------------------- backward


def alt_bwd_ref(f1, f2, coords, gout, r, dtype=np.float64, drop=None):
    """Gradients of the unscaled forward for corr_grad gout [B,N,(2r+1)^2,H1,W1]:
    (f1g, f2g, cg), (|f1g|-, |f2g|-, |cg|-magnitudes): every sum again over absolute values.  A query
    with a non-finite coordinate or |coordinate| >= 1e8 is absent (the contract); drop: a boolean
    [B,N,H1,W1] of further queries to leave out of fmap2_grad (mutation tests).  dtype=np.float32:
    the float32 restatement (magnitudes stay fp64)."""
    B, H1, W1, C = f1.shape
    _, H2, W2, _ = f2.shape
    N = coords.shape[1]
    rd, wd = 2 * r + 1, 2 * r + 2
    P = H1 * W1
    p, i, d, fin = positions(coords, 1.0)
    with np.errstate(all="ignore"):
        present = fin & (np.abs(p[..., 0]) < BIG) & (np.abs(p[..., 1]) < BIG)
    res = []
    for dt, absolute in ((dtype, False), (np.float64, True)):
        a1, a2 = f1.astype(dt).reshape(B, P, C), f2.astype(dt)
        G = gout.astype(dt)
        if absolute:
            a1, a2, G = np.abs(a1), np.abs(a2), np.abs(G)
        f1g = np.zeros((B, P, C), dt)
        f2g = np.zeros((B, H2 * W2, C), dt)
        cg = np.zeros((B, N, H1, W1, 2), dt)
        one = dt(1)
        for b in range(B):
            for n in range(N):
                ok = present[b, n].reshape(-1)
                x0 = i[b, n, ..., 0].reshape(-1) - r
                y0 = i[b, n, ..., 1].reshape(-1) - r
                dx = d[b, n, ..., 0].reshape(-1).astype(dt)[:, None, None]
                dy = d[b, n, ..., 1].reshape(-1).astype(dt)[:, None, None]
                g = G[b, n].reshape(rd, rd, P).transpose(2, 1, 0)            # g[q, oy, ox]
                g = np.where(ok[:, None, None], g, 0)
                # tap gradients, in the order the kernel adds them
                gt = np.zeros((P, wd, wd), dt)
                gt[:, 1:, 1:] += g * (dy * dx)
                gt[:, 1:, :rd] += g * (dy * (one - dx))
                gt[:, :rd, 1:] += g * ((one - dy) * dx)
                gt[:, :rd, :rd] += g * ((one - dy) * (one - dx))
                s = _taps(a1, f2 if not absolute else np.abs(f2), b, x0, y0, r, dt)
                s = np.where(ok[:, None, None], s, 0)
                s00, s01, s10, s11 = s[:, :rd, :rd], s[:, :rd, 1:], s[:, 1:, :rd], s[:, 1:, 1:]
                if absolute:
                    gx = g * ((one - dy) * (s01 + s00) + dy * (s11 + s10))
                    gy = g * ((one - dx) * (s10 + s00) + dx * (s11 + s01))
                else:
                    gx = g * ((one - dy) * (s01 - s00) + dy * (s11 - s10))
                    gy = g * ((one - dx) * (s10 - s00) + dx * (s11 - s01))
                cg[b, n, ..., 0] = gx.transpose(0, 2, 1).reshape(P, -1).sum(1, dtype=dt).reshape(H1, W1)
                cg[b, n, ..., 1] = gy.transpose(0, 2, 1).reshape(P, -1).sum(1, dtype=dt).reshape(H1, W1)
                keep = ok if drop is None else ok & ~drop[b, n].reshape(-1)
                for iy in range(wd):
                    h2 = y0 + iy
                    for ix in range(wd):
                        w2 = x0 + ix
                        inm = ok & (h2 >= 0) & (h2 < H2) & (w2 >= 0) & (w2 < W2)
                        q = np.nonzero(inm)[0]
                        if q.size == 0:
                            continue
                        pix = h2[q] * W2 + w2[q]
                        f1g[b, q] += gt[q, iy, ix, None] * a2[b].reshape(H2 * W2, C)[pix]
                        q2 = np.nonzero(inm & keep)[0]
                        np.add.at(f2g[b], h2[q2] * W2 + w2[q2], gt[q2, iy, ix, None] * a1[b, q2])
        res.append((f1g.reshape(B, H1, W1, C), f2g.reshape(B, H2, W2, C), cg))
    return res[0], res[1]


# ----------------------------------------------------------------------------- comparison


def check(got, ref, mag, bound, what=""):
    """Every element: NaN exactly where ref is NaN, else |got - ref| <= bound * mag (mag 0: got is
    exactly +-0).  Returns the worst |got - ref| / (2^-24 * mag) for the record."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape == mag.shape, (what, got.shape, ref.shape, mag.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern", int(np.isnan(got).sum()), int(nan.sum()))
    err = np.where(nan, 0.0, np.abs(got - np.where(nan, 0.0, ref)))
    lim = np.where(nan, 0.0, bound * mag)
    bad = err > lim
    with np.errstate(all="ignore"):
        ratio = np.where(lim > 0, err / np.where(lim > 0, mag * U24, 1.0), 0.0)
    if bad.any():
        k = np.unravel_index(np.argmax(np.where(bad, err - lim, -1.0)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements beyond {bound / U24:.1f} x 2^-24 x mag; "
                             f"worst at {k}: got {got[k]!r} ref {ref[k]!r} mag {mag[k]!r} "
                             f"(ratio {float(ratio.max()):.2f})")
    return float(ratio.max())


def rejects(got, ref, mag, bound):
    try:
        check(got, ref, mag, bound)
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------- data and coordinate builders


def maps(seed, B, H1, W1, H2, W2, C, scale=1.0):
    rng = np.random.default_rng(seed)
    f1 = (rng.standard_normal((B, H1, W1, C)) * scale).astype(np.float32)
    f2 = (rng.standard_normal((B, H2, W2, C)) * scale).astype(np.float32)
    return f1, f2


def level_maps(seed, B, H2, W2, C, L):
    """independent random levels (reading level l + 1 for level l is an O(1) error); dims halve, >= 1."""
    rng = np.random.default_rng(seed)
    out, h, w = [], H2, W2
    for _ in range(L):
        out.append(rng.standard_normal((B, h, w, C)).astype(np.float32))
        h, w = max(h // 2, 1), max(w // 2, 1)
    return out


def grid(B, N, H1, W1, H2, W2):
    ys, xs = np.meshgrid(np.arange(H1), np.arange(W1), indexing="ij")
    g = np.stack([xs * (W2 / W1), ys * (H2 / H1)], -1).astype(np.float32)
    return np.broadcast_to(g, (B, N, H1, W1, 2)).copy()


def smooth_coords(seed, B, N, H1, W1, H2, W2, spread=1.5):
    rng = np.random.default_rng(seed)
    return (grid(B, N, H1, W1, H2, W2) + rng.normal(0, spread, (B, N, H1, W1, 2))).astype(np.float32)


def tile_boxes(coords, r, coord_div=1.0):
    """The window box (bw, bh) of every 8x8 query tile, from the rule (alt_corr.hip: the union of the
    tile's (2r+2)^2 windows); coords [B,N,H1,W1,2] -> dict (b, n, ty, tx) -> (bw, bh, all_regular)."""
    p, i, _, fin = positions(coords, coord_div)
    with np.errstate(all="ignore"):
        reg = fin & (np.abs(p[..., 0]) < BIG) & (np.abs(p[..., 1]) < BIG)
    B, N, H1, W1, _ = coords.shape
    out = {}
    for b in range(B):
        for n in range(N):
            for ty in range(0, H1, 8):
                for tx in range(0, W1, 8):
                    x = i[b, n, ty:ty + 8, tx:tx + 8, 0]
                    y = i[b, n, ty:ty + 8, tx:tx + 8, 1]
                    out[(b, n, ty // 8, tx // 8)] = (int(x.max() - x.min()) + 2 * r + 2,
                                                     int(y.max() - y.min()) + 2 * r + 2,
                                                     bool(reg[b, n, ty:ty + 8, tx:tx + 8].all()))
    return out


def box_coords(seed, H1, W1, H2, W2, r, bw, bh, edge=False):
    """[1,1,H1,W1,2]: a smooth field whose tile (0, 0) has a window box of exactly bw x bh fmap2 pixels;
    edge: that box lies over the map's right and bottom edges."""
    rng = np.random.default_rng(seed)
    c = (grid(1, 1, H1, W1, H2, W2) + rng.normal(0, 0.7, (1, 1, H1, W1, 2))).astype(np.float32)
    sx, sy = bw - (2 * r + 2), bh - (2 * r + 2)
    assert sx >= 0 and sy >= 0
    x0 = (W2 - sx + 2.3) if edge else 6.3
    y0 = (H2 - sy + 1.6) if edge else 5.6
    jj, ii = np.meshgrid(np.arange(8), np.arange(8))
    c[0, 0, :8, :8, 0] = (x0 + np.round(sx * jj / 7.0))[:H1, :W1]
    c[0, 0, :8, :8, 1] = (y0 + np.round(sy * ii / 7.0))[:H1, :W1]
    got = tile_boxes(c, r)[(0, 0, 0, 0)]
    assert got == (bw, bh, True), (got, bw, bh)
    return c


def levels_fit(coords, r, L, limit):
    """per level: does EVERY tile's box fit (<= limit on both axes, regular coordinates)?  And per
    level the set of tiles that do not."""
    out = []
    for l in range(L):
        boxes = tile_boxes(coords, r, float(2 ** l))
        out.append({k for k, (bw, bh, reg) in boxes.items() if not (reg and bw <= limit and bh <= limit)})
    return out


def mixed_fit_coords(seed, B, H1, W1, H2, W2, r=4, L=4, limit=96):
    """[B,1,H1,W1,2]: a smooth field in which one query of tile (0, 1, 1) (batch 0) lies 200 px away,
    so that tile's box exceeds `limit` at levels 0 and 1 (per-pixel branch) and fits at levels 2 and 3
    (box GEMM); every other tile fits at every level."""
    c = smooth_coords(seed, B, 1, H1, W1, H2, W2, 0.7)
    c[0, 0, 11, 13, 0] += 200.0
    nofit = levels_fit(c, r, L, limit)
    key = (0, 0, 1, 1)
    assert [key in s for s in nofit] == [True, True] + [False] * (L - 2), nofit
    assert all(s <= {key} for s in nofit)
    return c


EDGE_SETS = ("integer", "negative-fraction", "below-integer", "left", "right", "top", "bottom",
             "top-left", "top-right", "bottom-left", "bottom-right", "wholly-off")


def edge_coords(kind, seed, B, N, H1, W1, H2, W2, r):
    """[B,N,H1,W1,2] coordinate sets on the cases the bilinear window arithmetic can get wrong."""
    rng = np.random.default_rng(seed)
    c = smooth_coords(seed, B, N, H1, W1, H2, W2, 1.0)
    eps = np.float32(2.0 ** -20)
    if kind == "integer":                       # dx = dy = 0 exactly
        c = np.round(c)
        assert np.all(c == np.floor(c))
    elif kind == "negative-fraction":           # floor = -1
        c = -rng.uniform(0.01, 0.99, c.shape).astype(np.float32)
        assert np.all(np.floor(c) == -1)
    elif kind == "below-integer":               # k - 2^-20: fraction 1 - 2^-20 (or the nearest fp32)
        k = np.clip(np.round(c), 1, 8).astype(np.float32)
        c = (k - eps).astype(np.float32)
        assert np.all(np.floor(c) == k - 1) and np.all(c - np.floor(c) == np.float32(1) - eps)
    elif kind == "wholly-off":
        c = c + np.float32(H2 + W2 + 4 * r + 40) * rng.choice([-1.0, 1.0], c.shape).astype(np.float32)
        _, i, _, _ = positions(c, 1.0)
        offx = (i[..., 0] + r + 1 < 0) | (i[..., 0] - r >= W2)
        offy = (i[..., 1] + r + 1 < 0) | (i[..., 1] - r >= H2)
        assert np.all(offx & offy)
    else:                                       # windows half off one edge / one corner
        fx = rng.uniform(0.05, 0.95, c.shape[:-1]).astype(np.float32)
        fy = rng.uniform(0.05, 0.95, c.shape[:-1]).astype(np.float32)
        if "left" in kind:
            c[..., 0] = -1.0 + fx - rng.integers(0, r + 1, fx.shape)
        if "right" in kind:
            c[..., 0] = W2 - 1.0 + fx + rng.integers(0, r + 1, fx.shape)
        if "top" in kind:
            c[..., 1] = -1.0 + fy - rng.integers(0, r + 1, fy.shape)
        if "bottom" in kind:
            c[..., 1] = H2 - 1.0 + fy + rng.integers(0, r + 1, fy.shape)
        _, i, _, _ = positions(c, 1.0)
        if "left" in kind:
            assert np.all(i[..., 0] - r < 0) and np.all(i[..., 0] + r + 1 >= 0)
        if "right" in kind:
            assert np.all(i[..., 0] + r + 1 >= W2) and np.all(i[..., 0] - r < W2)
        if "top" in kind:
            assert np.all(i[..., 1] - r < 0) and np.all(i[..., 1] + r + 1 >= 0)
        if "bottom" in kind:
            assert np.all(i[..., 1] + r + 1 >= H2) and np.all(i[..., 1] - r < H2)
    return c.astype(np.float32)


IRREGULAR = (1e8, -1e8, 3e9, -3e9, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan)


def irregular_coords(base, tiles=((0, 0), (1, 2))):
    """base [B,N,H1,W1,2] -> (coords, where): each of IRREGULAR on x only, y only and both, one query
    each, all inside the 8x8 tiles `tiles` (tile row, tile column) of batch 0, set 0; where:
    boolean [B,N,H1,W1] of the changed queries.  Every other tile keeps the base coordinates."""
    c = base.copy()
    where = np.zeros(c.shape[:-1], bool)
    H1, W1 = c.shape[2:4]
    slots = [(ty * 8 + y, tx * 8 + x) for ty, tx in tiles for y in range(8) for x in range(8)
             if ty * 8 + y < H1 and tx * 8 + x < W1]
    need = 3 * len(IRREGULAR)
    assert len(slots) >= need
    slots = slots[::len(slots) // need]
    k = 0
    for v in IRREGULAR:
        for axes in ((0,), (1,), (0, 1)):
            y, x = slots[k]
            for a in axes:
                c[0, 0, y, x, a] = np.float32(v)
            where[0, 0, y, x] = True
            k += 1
    assert int(where.sum()) == 3 * len(IRREGULAR)
    return c, where


def tied_coords(seed, H1, W1, H2, W2, ties=200, neighbours=3):
    """[1,1,H1,W1,2]: `ties` queries whose window origin is the same fmap2 pixel (different
    fractions), `neighbours` more with the origin one pixel off, the rest smooth."""
    rng = np.random.default_rng(seed)
    c = smooth_coords(seed, 1, 1, H1, W1, H2, W2, 1.0)
    flat = c.reshape(-1, 2)
    assert flat.shape[0] >= ties + neighbours
    idx = rng.permutation(flat.shape[0])
    ox, oy = W2 // 2, H2 // 2
    flat[idx[:ties]] = np.stack([ox + rng.uniform(0.01, 0.99, ties), oy + rng.uniform(0.01, 0.99, ties)], -1)
    for j, (ddx, ddy) in enumerate(((1, 0), (0, 1), (-1, -1))[:neighbours]):
        flat[idx[ties + j]] = (ox + ddx + 0.5, oy + ddy + 0.25)
    c = flat.reshape(1, 1, H1, W1, 2).astype(np.float32)
    _, i, _, _ = positions(c, 1.0)
    same = (i[..., 0] == ox) & (i[..., 1] == oy)
    assert int(same.sum()) >= ties
    return c, same


# ----------------------------------------------------------------------------- the kernel forms and their inputs


def kernel_form(C, r, precision):
    """launch_alt's dispatch (alt_corr.hip), restated: which kernel a call reaches with RAFT_ALT_MFMA
    unset."""
    if r > 4:
        return "generic"
    if precision != "fp32" and r == 4 and C % 32 == 0 and C <= 256:
        return "mfma"
    if r == 4 and C % 8 == 0 and C <= 256:
        return "tile"
    return "per-pixel<1>" if C <= 256 else "per-pixel<2>" if C <= 512 else "per-pixel<4>"


def form_bound(C, r, precision):
    return bound16x3(1.0) if kernel_form(C, r, precision) == "mfma" else bound32()


FORMS = [  # (C, r, precision, H1, W1); ids: form_id
    (64, 0, "f16x3", 16, 24), (64, 1, "f16x3", 16, 24), (64, 3, "f16x3", 16, 24), (36, 4, "f16x3", 16, 24),
    (260, 4, "f16x3", 16, 24), (512, 4, "f16x3", 16, 24),
    (516, 4, "f16x3", 16, 24), (1024, 4, "f16x3", 9, 13),
    (64, 4, "fp32", 16, 24), (8, 4, "f16x3", 16, 24), (40, 4, "f16x3", 16, 24), (248, 4, "f16x3", 16, 24),
    (32, 4, "f16x3", 16, 24), (96, 4, "f16x3", 16, 24), (224, 4, "f16x3", 16, 24), (256, 4, "f16x3", 16, 24),
    (64, 5, "f16x3", 16, 24), (64, 8, "f16x3", 16, 24),
    # ragged tiles and a map smaller than one tile, on each kernel
    (64, 3, "f16x3", 13, 19), (40, 4, "f16x3", 13, 19), (64, 4, "f16x3", 13, 19), (64, 5, "f16x3", 13, 19),
    (64, 3, "f16x3", 3, 5), (40, 4, "f16x3", 3, 5), (64, 4, "f16x3", 3, 5), (64, 5, "f16x3", 3, 5),
]
# every kernel (and r = 0, the FP32 route, r = 8) for the coordinate tests
CORE_FORMS = [(64, 3, "f16x3", 16, 24), (260, 4, "f16x3", 16, 24), (516, 4, "f16x3", 16, 24),
              (40, 4, "f16x3", 16, 24), (64, 4, "f16x3", 16, 24), (64, 5, "f16x3", 16, 24),
              (64, 0, "f16x3", 16, 24), (64, 4, "fp32", 16, 24), (64, 8, "f16x3", 16, 24)]


def form_id(form):
    C, r, prec, H1, W1 = form
    return f"{kernel_form(C, r, prec)}-C{C}-r{r}-{prec}-{H1}x{W1}"


def form_inputs(form, B=2, N=2, L=2):
    """(f1 [B,H1,W1,C], f2 levels (independent, L of them, level 0 = H1-2 x W1-1), coords [B,N,H1,W1,2])."""
    C, r, _, H1, W1 = form
    seed = 1000 * C + 10 * r + H1
    H2, W2 = max(H1 - 2, 1), max(W1 - 1, 1)
    f1, _ = maps(seed, B, H1, W1, 1, 1, C)
    return f1, level_maps(seed + 1, B, H2, W2, C, L), smooth_coords(seed + 2, B, N, H1, W1, H2, W2, 1.5)


BWD_CASES = ("tied", "half-left", "half-right", "half-top", "half-bottom", "identical-sets", "1x1", "r0", "C4",
             "C1024", "integer", "irregular")


def bwd_case(name):
    """(f1, f2, coords, corr_grad, r) of the backward tests; "tied": 200 queries share one window origin."""
    B, N, H1, W1, H2, W2, C, r = 1, 1, 16, 24, 12, 20, 32, 2
    if name == "tied":
        C, r = 64, 4
    elif name == "identical-sets":
        N, r = 2, 3
    elif name == "1x1":
        H2 = W2 = 1
    elif name == "r0":
        r = 0
    elif name == "C4":
        C = 4
    elif name == "C1024":
        H1, W1, H2, W2, C, r = 9, 13, 5, 7, 1024, 1
    elif name == "irregular":
        B = 2
    seed = sum(map(ord, name))
    f1, f2 = maps(seed, B, H1, W1, H2, W2, C)
    if name == "tied":
        c = tied_coords(seed, H1, W1, H2, W2)[0]
    elif name.startswith("half-"):
        c = edge_coords(name[5:], seed, B, N, H1, W1, H2, W2, r)
    elif name == "integer":
        c = edge_coords("integer", seed, B, N, H1, W1, H2, W2, r)
    else:
        c = smooth_coords(seed, B, N, H1, W1, H2, W2, 1.5)
    if name == "identical-sets":
        c[:, 1] = c[:, 0]
    if name == "irregular":
        c = irregular_coords(c)[0]
    g = np.random.default_rng(seed + 1).standard_normal((B, N, (2 * r + 1) ** 2, H1, W1)).astype(np.float32)
    return f1, f2, c, g, r
