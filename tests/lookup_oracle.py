"""Host-side reference of the all-pairs correlation lookup (raft_corr_lookup and the kernels that
restate it), independent of the library: numpy / torch on the CPU only.

tile_levels   per-level maps -> the library's pyramid buffer (include/raft_hip.h: 4x4 tiles, levels
              back to back, padding 0), so a lookup is tested on a pyramid the test wrote.
lookup_ref    CorrBlock.__call__ with the sample positions in fp32 exactly as
              oracle.raft_oracle.bilinear_sampler computes them and the four-corner blend in fp64.
off_patch     which (pixel, level) pairs take the kernels' deferred path (lookup_common.hpp:
              axis_entry's OFF_PATCH), restated from the rule, not from the code.  The rule for rows
              is the corrected one: the y-entries used to be tested against the 4-aligned tile range
              like the x-entries, although only the window's own rows are fetched (see axis_entry).
"""
import numpy as np
import torch

SENTINEL = -7.0
U24 = 2.0 ** -24


def level_dims(H, W, L):
    dims, h, w = [], H, W
    for _ in range(L):
        dims.append((h, w))
        h, w = h // 2, w // 2
    return dims


def tile_levels(levels, B, H, W):
    """levels[l]: [B*H*W, h_l, w_l] (numpy or torch, any device) -> the flat fp32 pyramid buffer
    (torch, on the levels' device): per level every query pixel's map in 4x4 tiles, element (y, x) at
    ((y>>2)*TW + (x>>2))*16 + (y&3)*4 + (x&3), zero padded; levels back to back."""
    parts = []
    for lv in levels:
        t = torch.as_tensor(lv)
        n, h, w = t.shape
        assert n == B * H * W
        th, tw = (h + 3) // 4, (w + 3) // 4
        p = torch.zeros(n, th * 4, tw * 4, dtype=torch.float32, device=t.device)
        p[:, :h, :w] = t
        parts.append(p.view(n, th, 4, tw, 4).permute(0, 1, 3, 2, 4).reshape(-1))
    return torch.cat(parts)


def _axis(c, l, r, m):
    """fp32 sampling entries of one axis at level l: c [N] fp32 level-0 coordinate, map size m.
    Returns (fin [N, 2r+1], i int64 floor, t fp32 fraction) as bilinear_sampler + grid_sample do."""
    f = np.float32
    with np.errstate(all="ignore"):
        cen = c.astype(f) / f(2 ** l)
        X = cen[:, None] + np.arange(-r, r + 1, dtype=f)[None]
        g = f(2) * X / f(m - 1) - f(1)
        u = ((g + f(1)) / f(2)) * f(m - 1)
        assert u.dtype == np.float32
        fin = np.isfinite(u)
        us = np.where(fin, u, f(0))
        f0 = np.floor(us)
        t = (us - f0).astype(f)
        i = np.clip(f0, -1e15, 1e15).astype(np.int64)
    return fin, i, t


def lookup_ref(levels, coords, r):
    """levels[l]: [N, h_l, w_l] numpy; coords [N, 2] fp32 (x, y).  Returns (out, cmax), both
    [N, L*(2r+1)^2] fp64, channel lvl*(2r+1)^2 + ix*(2r+1) + iy: the bilinear blend in fp64 of the
    corners at the fp32 positions (zeros off the map, NaN where a position is not finite), and the
    largest |corner| each tap read."""
    coords = np.asarray(coords, np.float32)
    n = coords.shape[0]
    rd = 2 * r + 1
    outs, cms = [], []
    rows = np.arange(n)[:, None, None]
    for l, lv in enumerate(levels):
        lv = np.asarray(lv)
        _, h, w = lv.shape
        fx, xi, xt = _axis(coords[:, 0], l, r, w)
        fy, yi, yt = _axis(coords[:, 1], l, r, h)
        X, Y = xi[:, :, None], yi[:, None, :]           # [N, ix, 1], [N, 1, iy]
        tx, ty = xt.astype(np.float64)[:, :, None], yt.astype(np.float64)[:, None, :]

        def corner(yy, xx):
            ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
            v = lv[rows, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.float64)
            return np.where(ok, v, 0.0)

        c00, c01, c10, c11 = corner(Y, X), corner(Y, X + 1), corner(Y + 1, X), corner(Y + 1, X + 1)
        with np.errstate(invalid="ignore"):
            v = c00 * ((1 - tx) * (1 - ty)) + c01 * (tx * (1 - ty)) + c10 * ((1 - tx) * ty) + c11 * (tx * ty)
            cm = np.maximum(np.maximum(np.abs(c00), np.abs(c01)), np.maximum(np.abs(c10), np.abs(c11)))
        bad = ~(fx[:, :, None] & fy[:, None, :])
        outs.append(np.where(bad, np.nan, v).reshape(n, rd * rd))
        cms.append(cm.reshape(n, rd * rd))
    return np.concatenate(outs, 1), np.concatenate(cms, 1)


def off_patch_taps(coords, dims, r):
    """Per tap [N, L*(2r+1)^2]: the tap takes the kernels' deferred path -- its fp32 floor i or i + 1,
    on either axis, lies outside what the kernel staged for the window floor(c) - r .. floor(c) + r + 1
    (c the level's centroid, floor(c) = floor(x) >> l), and both positions are finite.  Staged
    (lookup_common.hpp, axis_entry): on x the 4-aligned tile range covering the window (whole tile
    columns are loaded); on y the window's own 2r + 2 rows (the other rows of its tiles are not)."""
    coords = np.asarray(coords, np.float32)
    n = coords.shape[0]
    rd = 2 * r + 1
    res = []
    for l, (h, w) in enumerate(dims):
        per_axis = []
        for a, m in ((0, w), (1, h)):
            c = coords[:, a]
            with np.errstate(invalid="ignore"):
                fc = np.clip(np.floor(np.where(np.isfinite(c), c, 0)), -2.0 ** 40, 2.0 ** 40).astype(np.int64) >> l
            if a == 0:
                lo = ((fc - r) >> 2) * 4                 # first column of the first tile
                hi = (((fc + r + 1) >> 2) + 1) * 4       # one past the last tile's last column
            else:
                lo, hi = fc - r, fc + r + 2              # the window's rows
            fin, i, _ = _axis(c, l, r, m)
            off = (i < lo[:, None]) | (i + 1 >= hi[:, None])
            per_axis.append((fin, off))
        (fx, ox), (fy, oy) = per_axis
        fin = fx[:, :, None] & fy[:, None, :]
        res.append(((ox[:, :, None] | oy[:, None, :]) & fin).reshape(n, rd * rd))
    return np.concatenate(res, 1)


def off_patch(coords, dims, r):
    """[N, L] bool: any tap of the (pixel, level) takes the deferred path."""
    t = off_patch_taps(coords, dims, r)
    return t.reshape(t.shape[0], len(dims), -1).any(-1)


# ---------------------------------------------------------------------------------------------
# Coordinate sets of the GPU tests (tests/test_gpu_lookup_forms.py); the host test checks that
# they reach the paths they are meant to reach.
# ---------------------------------------------------------------------------------------------

def grid_xy(B, H, W):
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.broadcast_to(np.stack([xs, ys], -1).astype(np.float32), (B, H, W, 2)).reshape(-1, 2).copy()


def matrix_coords(B, H, W, seed, sigma=3.0):
    """The instantiation matrix's coordinates: grid + N(0, sigma); the last image (the last quarter
    of the rows of a single image) uniform over [-40, W + 40] x [-40, H + 40], so windows hang off
    every edge and lie fully outside."""
    rng = np.random.default_rng(seed)
    g = grid_xy(B, H, W)
    c = (g + rng.normal(0, sigma, g.shape)).astype(np.float32)
    n0 = (B - 1) * H * W if B >= 2 else (3 * H // 4) * W
    c[n0:, 0] = rng.uniform(-40, W + 40, len(c) - n0)
    c[n0:, 1] = rng.uniform(-40, H + 40, len(c) - n0)
    return c


def tap_check(got, ref, cmax, u=0.0, abs_term=0.0):
    """The lookup tests' comparison.  got [N, ntap] fp32 against lookup_ref's (ref, cmax): NaN exactly
    where ref is NaN, elsewhere |got - ref| <= 8 * 2^-24 * cmax + u * |ref| + abs_term.  Returns
    (bad [N, ntap] bool, worst |err| / (2^-24 * cmax) over the taps with cmax > 0)."""
    got = np.asarray(got, np.float64)
    nr, ng = np.isnan(ref), np.isnan(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        bound = 8 * U24 * cmax + u * np.abs(ref) + abs_term
        bad = (nr != ng) | (~nr & ~(err <= bound))
        ratio = np.where(~nr & ~ng & (cmax > 0), err / (U24 * cmax), 0.0)
    return bad, float(ratio.max()) if ratio.size else 0.0


def bound_fraction(got, ref, cmax, u=0.0, abs_term=0.0):
    """Worst |err| / bound of tap_check over the taps with a non-zero bound (for the records)."""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        bound = 8 * U24 * cmax + u * np.abs(ref) + abs_term
        frac = np.where(np.isfinite(got) & np.isfinite(ref) & (bound > 0), np.abs(got - ref) / bound, 0.0)
    return float(frac.max()) if frac.size else 0.0


def describe_bad(bad, got, ref, cmax, rd2):
    """The first failing tap of a tap_check, for the assertion message."""
    p, c = np.argwhere(bad)[0]
    return (f"{int(bad.sum())} taps fail; first: pixel {p} channel {c} (level {c // rd2}, ix*rd+iy {c % rd2}) "
            f"got {got[p, c]!r} ref {ref[p, c]!r} cmax {cmax[p, c]!r}")


def deferred_coords(B, H, W, seed):
    """Section b: every pixel draws one of: the identity grid; grid + an integer shift in [-6, 6]
    per axis; grid + integer shift + one of {+-2^-20, 0.25, 0.5}; an integer position up to 12 px
    off every map edge; on one axis the fp32 number just below a multiple of 8 (the level-3
    centroid c / 8 + offset then rounds up to the next integer, past the patch staged for
    floor(c) >> 3: the one way found to the deferred path on level 3, see
    test_lookup_oracle_host.py).  With B >= 2 the last image is all of the fourth kind."""
    rng = np.random.default_rng(seed)
    n = B * H * W
    g = grid_xy(B, H, W)
    kind = rng.integers(0, 5, n)
    if B >= 2:
        kind[(B - 1) * H * W:] = 3
    shift = rng.integers(-6, 7, (n, 2)).astype(np.float32)
    frac = rng.choice(np.array([2.0 ** -20, -2.0 ** -20, 0.25, 0.5], np.float32), (n, 2))
    edge = np.stack([rng.integers(-12, W + 12, n), rng.integers(-12, H + 12, n)], -1).astype(np.float32)
    c = g.copy()
    c = np.where((kind == 1)[:, None], g + shift, c)
    c = np.where((kind == 2)[:, None], g + shift + frac, c)
    c = np.where((kind == 3)[:, None], edge, c)
    axis = rng.integers(0, 2, n)
    k8 = np.float32(8) * rng.integers(-2, np.where(axis == 0, W, H) // 8 + 3, n).astype(np.float32)
    below = np.nextafter(k8, np.float32(-np.inf))
    for a in (0, 1):
        c[:, a] = np.where((kind == 4) & (axis == a), below, c[:, a])
    return c.astype(np.float32)


# the deferred-path coordinate sets the GPU tests use: (B, H, W) -> seed
DEFERRED_SETS = {(1, 55, 128): 1, (2, 23, 37): 2, (20, 23, 37): 3}


def deferred_set(B, H, W):
    return deferred_coords(B, H, W, DEFERRED_SETS[(B, H, W)])
