"""Host-side reference of the all-pairs correlation build (raft_corr_build, raft_corr_build_prec,
raft_corr_build_ws; CorrBlock.__init__ / CorrBlock.corr, core/corr.py:25-54, 96-127), independent of the
library: numpy only (the tiler is tests/lookup_oracle.py's).

reference   level 0 = <f1[p], f2[q]> / sqrt_c and the floor 2x2 average pools in fp64, and with every level
            a magnitude mag_l: mag_0 = sum_c |f1_c f2_c| / sqrt_c, mag_{l+1} the same pool of mag_l.
restate     the documented arithmetic in float32 (FP32: float32 dot product; F16X3: hi = f16(x),
            lo = f16(x - hi), the sums of hi*hi, lo*hi and hi*lo per 16-channel half-step in float32),
            the float32 division and (((a0+a1)+a2)+a3)/4 in float32.  The bound's coefficient is measured
            from it, never from a kernel.  It also carries the mutations the host test rejects.
tile        levels -> the raw pyramid buffer of include/raft_hip.h (fp64, padding 0); untile its inverse.
units       the work units of raft_corr_build_ws's persistent kernel (a.units in corr_pyramid.hip).
compare     the GPU tests' comparison: |got - ref| <= k * mag element by element, exactly 0 where mag is 0.
"""
import numpy as np

from lookup_oracle import level_dims, tile_levels

U24 = 2.0 ** -24
FLOOR_K = 2 * U24   # one rounding of the division plus one of the pool
MARGIN = 4          # the MFMA's accumulation order against the restatement's
FP32, F16X3 = "fp32", "f16x3"


# ------------------------------------------------------------------------------------ reference


def _pool(x):
    """Floor 2x2 average pool of [N, h, w] in x's dtype, avg_pool2d's window order."""
    h, w = x.shape[1] // 2, x.shape[2] // 2
    a = x[:, 0:2 * h:2, 0:2 * w:2] + x[:, 0:2 * h:2, 1:2 * w:2]
    a = (a + x[:, 1:2 * h:2, 0:2 * w:2]) + x[:, 1:2 * h:2, 1:2 * w:2]
    return a / x.dtype.type(4)


def reference(f1, f2, L, sqrt_c, B, H, W):
    """f1, f2: float32 rows [B*H*W][C].  Returns (levels, mags): per level [B*H*W, h_l, w_l] fp64."""
    P = H * W
    a = np.asarray(f1, np.float64).reshape(B, P, -1)
    b = np.asarray(f2, np.float64).reshape(B, P, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        lv = (np.matmul(a, b.transpose(0, 2, 1)) / np.float64(sqrt_c)).reshape(B * P, H, W)
        mg = (np.matmul(np.abs(a), np.abs(b).transpose(0, 2, 1)) / np.float64(sqrt_c)).reshape(B * P, H, W)
        levels, mags = [lv], [mg]
        for _ in range(L - 1):
            lv, mg = _pool(lv), _pool(mg)
            levels.append(lv)
            mags.append(mg)
    return levels, mags


def split16(x):
    """The unscaled split: hi = f16(x), lo = f16(x - hi), round to nearest even, subnormals kept
    (|x| >= 65520: hi = inf, lo = -inf)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


MUTATIONS = {
    "a": "the lo*hi term dropped in one 16-channel half-step",
    "b": "the last 8 channels of the K tail dropped",
    "c": "fmap1 and fmap2 swapped (the volume transposed)",
    "d": "image b's queries paired with image b+1's targets",
    "e": "a target column shifted by one",
    "f": "the pool window started one pixel late",
    "g": "level l+1 read where level l is meant",
}


def restate(f1, f2, L, sqrt_c, prec, B, H, W, mutation=None):
    """The documented arithmetic in float32: levels [B*H*W, h_l, w_l] float32.  mutation: a key of
    MUTATIONS (a wrong build, for the host test)."""
    f = np.float32
    P = H * W
    a = np.ascontiguousarray(np.asarray(f1, f).reshape(B, P, -1))
    b = np.ascontiguousarray(np.asarray(f2, f).reshape(B, P, -1))
    C = a.shape[2]
    if mutation == "b":
        a, b, C = a[..., :C - 8], b[..., :C - 8], C - 8
    if mutation == "c":
        a, b = b, a
    if mutation == "d":
        b = np.roll(b, -1, axis=0)
    if mutation == "e":
        b = np.roll(b.reshape(B, H, W, C), -1, axis=2).reshape(B, P, C)
    with np.errstate(invalid="ignore", over="ignore"):
        if prec == FP32:
            s = np.matmul(a, b.transpose(0, 2, 1))
        else:
            ah, al = split16(a)
            bh, bl = split16(b)
            hh = np.zeros((B, P, P), f)
            lh = np.zeros((B, P, P), f)
            hl = np.zeros((B, P, P), f)
            for i, c0 in enumerate(range(0, C, 16)):
                sl = slice(c0, min(c0 + 16, C))
                bt_h, bt_l = bh[..., sl].transpose(0, 2, 1), bl[..., sl].transpose(0, 2, 1)
                hh += np.matmul(ah[..., sl], bt_h)
                if not (mutation == "a" and i == 1):
                    lh += np.matmul(al[..., sl], bt_h)
                hl += np.matmul(ah[..., sl], bt_l)
            s = hh + (lh + hl)
        assert s.dtype == f
        lv = (s / f(sqrt_c)).reshape(B * P, H, W)
        levels = [lv]
        for _ in range(L - 1 + (mutation == "g")):
            if mutation == "f":
                h, w = lv.shape[1] // 2, lv.shape[2] // 2
                oy, ox = lv.shape[1] - 2 * h, lv.shape[2] - 2 * w   # 1 on an odd size
                lv = _pool(lv[:, oy:, ox:])
            else:
                lv = _pool(lv)
            levels.append(lv)
    if mutation == "g":
        out = [levels[0]]
        for l in range(1, L):
            z = np.zeros_like(levels[l])
            nxt = levels[l + 1]
            z[:, :nxt.shape[1], :nxt.shape[2]] = nxt
            out.append(z)
        levels = out
    assert all(x.dtype == f for x in levels)
    return levels


# ------------------------------------------------------------------------------------ the raw buffer


def tile(levels, B, H, W):
    """levels[l] [B*H*W, h_l, w_l] -> the raw pyramid buffer by the header's formula, zero padding, fp64
    (float32 levels exactly; fp64 levels as a float32 head + tail through lookup_oracle.tile_levels)."""
    head = [np.asarray(x).astype(np.float32) for x in levels]
    with np.errstate(invalid="ignore"):
        tail = [np.nan_to_num((np.asarray(x, np.float64) - h).astype(np.float32), nan=0.0, posinf=0.0, neginf=0.0)
                for x, h in zip(levels, head)]
    return tile_levels(head, B, H, W).numpy().astype(np.float64) + tile_levels(tail, B, H, W).numpy()


def valid_mask(B, H, W, L):
    """Raw-buffer bool mask: True at the valid elements, False at the tile padding."""
    return tile_levels([np.ones((B * H * W, h, w), np.float32) for h, w in level_dims(H, W, L)], B, H, W).numpy() > 0


def untile(raw, B, H, W, L):
    """The raw buffer's levels as [B*H*W, h_l, w_l] (raw's dtype), bit for bit."""
    raw = np.asarray(raw)
    n, off, out = B * H * W, 0, []
    for h, w in level_dims(H, W, L):
        th, tw = (h + 3) // 4, (w + 3) // 4
        seg = raw[off:off + n * th * tw * 16].reshape(n, th, tw, 4, 4).transpose(0, 1, 3, 2, 4)
        out.append(np.ascontiguousarray(seg.reshape(n, th * 4, tw * 4)[:, :h, :w]))
        off += n * th * tw * 16
    assert off == raw.size
    return out


def pyramid_floats(B, H, W, L):
    return sum(B * H * W * ((h + 3) // 4) * ((w + 3) // 4) * 16 for h, w in level_dims(H, W, L))


def pool_exact(levels):
    """Per level l >= 1: is it bit for bit (((a0+a1)+a2)+a3)/4 of levels[l-1] (float32)?"""
    res = []
    for l in range(1, len(levels)):
        want = _pool(np.asarray(levels[l - 1], np.float32))
        res.append(np.array_equal(want.view(np.uint32), np.ascontiguousarray(levels[l], np.float32).view(np.uint32)))
    return res


def units(B, H, W, nw):
    """a.units of raft_corr_build_ws: images x query tiles (256 queries with 8 waves, 128 with 4) x 16 x 16
    target blocks."""
    tq = {8: 256, 4: 128}[nw]
    return B * -(-(H * W) // tq) * -(-H // 16) * -(-W // 16)


# ------------------------------------------------------------------------------------ the comparison


def measure(levels, ref, mag):
    """Largest |levels - ref| / mag over the elements with mag > 0 (all levels)."""
    worst = 0.0
    for x, r, m in zip(levels, ref, mag):
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.abs(np.asarray(x, np.float64) - r) / m
        q = q[m > 0]
        if q.size:
            worst = max(worst, float(q.max()) if np.isfinite(q).all() else float("inf"))
    return worst


def bound_k(r):
    """The elementwise bound's coefficient from the restatement's largest err / mag."""
    return max(MARGIN * r, FLOOR_K)


def compare(got, ref, mag, k):
    """got, ref, mag: raw buffers (or any equal shapes).  bad = not (|got - ref| <= k * mag): where mag is 0
    (the padding, a zero dot product) the element must be exactly 0; a NaN never passes.  Returns
    (bad, largest |got - ref| / mag over mag > 0)."""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        bad = ~(err <= k * mag)
        q = np.where(mag > 0, err / mag, 0.0)
    worst = float(np.nanmax(q)) if q.size else 0.0
    if np.isnan(q).any():
        worst = float("inf")
    return bad, worst


def describe_bad(bad, got, ref, mag, B, H, W, L):
    """The first failing raw element of a compare, for the assertion message."""
    i = int(np.flatnonzero(bad)[0])
    off = 0
    for l, (h, w) in enumerate(level_dims(H, W, L)):
        s = ((h + 3) // 4) * ((w + 3) // 4) * 16
        if i < off + B * H * W * s:
            p, r = divmod(i - off, s)
            t, e = divmod(r, 16)
            tw = (w + 3) // 4
            y, x = (t // tw) * 4 + e // 4, (t % tw) * 4 + e % 4
            return (f"{int(bad.sum())} elements fail; first: level {l} query {p} (y, x) = ({y}, {x})"
                    f"{' [padding]' if y >= h or x >= w else ''} got {got[i]!r} ref {ref[i]!r} mag {mag[i]!r}")
        off += B * H * W * s
    return f"{int(bad.sum())} elements fail; first raw index {i}"


def target_cells(q, H, W, L):
    """The cells a target pixel q = y * W + x reaches: per level (y_l, x_l), or None from the level on at
    which the floor pool drops it (the last row / column of an odd size)."""
    y, x = divmod(q, W)
    cells, alive = [], True
    for l, (h, w) in enumerate(level_dims(H, W, L)):
        if l:
            y, x = y >> 1, x >> 1
        alive = alive and y < h and x < w
        cells.append((y, x) if alive else None)
    return cells


# ------------------------------------------------------------------------------------ inputs and case tables


def features(B, H, W, C, seed, scale=1.0):
    """N(0, scale^2) float32 rows (f1, f2), each [B*H*W][C]."""
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((2, B * H * W, C)) * scale).astype(np.float32)
    return f[0], f[1]


def sqrt_c32(C):
    return float(np.sqrt(np.float32(C)))


# Tile geometry, C = 64, through every entry: (B, H, W, L)
GEOMETRY = [
    (1, 1, 1, 1),
    (1, 2, 2, 2),
    (1, 3, 5, 1),
    (2, 7, 9, 2),
    (1, 8, 16, 4),
    (1, 9, 17, 4),
    (2, 15, 31, 4),
    (1, 15, 17, 3),    # P = 255
    (1, 16, 16, 5),    # P = 256
    (1, 1, 257, 1),
    (1, 257, 1, 1),
    (1, 17, 33, 5),
    (3, 23, 37, 4),
]
GEOMETRY_C = 64
GEOMETRY_SQRT3 = (2, 7, 9, 2)   # this case divides by 3.0 instead of sqrt(C)

# Channel counts at one shape, ld = C and ld = C + 4
CHANNEL_SHAPE = (2, 9, 17, 3)
CHANNELS = {
    "fp32": [4, 24, 32, 36, 256],
    "prec": [4, 24, 40, 64, 256],
    "ws": [64, 80, 96, 128, 256, 1024],
}
WS_FALLBACK_C = [48, 72, 1040]   # raft_corr_build_ws takes raft_corr_build_prec's kernel (and with FP32 at any C)

# Persistent pipeline: raft_corr_build_ws at (B, 33, 49), C = 64; B from the device's CU count
PIPELINE_HW = (33, 49)
PIPELINE_C = 64
PIPELINE_L = [1, 2, 3, 6]


def pipeline_batches(cus, nw):
    """(B_multi, B_three) for nw waves on a device with cus CUs (work-groups: cus with 8 waves, 2 cus with 4):
    the smallest B with more units than work-groups and not a multiple of them; the smallest B with at
    least 3 units on some work-group (and not a multiple either)."""
    wgs = cus if nw == 8 else 2 * cus
    H, W = PIPELINE_HW
    multi = next(b for b in range(1, 10000) if units(b, H, W, nw) > wgs and units(b, H, W, nw) % wgs)
    three = next(b for b in range(1, 10000) if units(b, H, W, nw) > 2 * wgs and units(b, H, W, nw) % wgs)
    return multi, three


# Magnitude sweep: features x 2^k
SWEEP_SHAPE = (1, 9, 17, 2)
SWEEP_C = 64
SWEEP_K = [12, 8, 4, 0, -2, -3, -4, -6, -8, -12]

# Ragged cases of the switch tests (non-temporal stores, the once-per-process switches)
SWITCH_CASES = [(2, 23, 37, 4), (1, 17, 33, 4)]
SWITCH_C = 64

# Out of range / non-finite: (B, H, W, L); the poisoned pixels: inside, and in the odd size's dropped last row
POISON_SHAPE = (2, 9, 17, 3)
POISON_C = 64
POISON_IMAGE = 1
POISON_INSIDE = 3 * 17 + 6     # (y, x) = (3, 6): cells (3, 6), (1, 3), (0, 1)
POISON_DROPPED = 8 * 17 + 5    # (y, x) = (8, 5): the last row of H = 9, no level-1 cell holds it
POISON_CHANNEL = 5
