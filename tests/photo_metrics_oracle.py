"""raft_photo_metrics' definition (include/raft_hip.h) in numpy fp64, with the error bounds of the fp32 kernel as
functions of the inputs.  Reads only arrays.

    pixel_values(frame1, frame2, flow, patch)  -> the per-pixel values e, h, valid and their fp32 error bounds
    metrics(frame1, frame2, flow, mask, ...)   -> one dict per sample: exact counts, fsum sums, a bound per sum
    totals(records), result(totals)            -> the union of records and PhotoMetrics.result()'s dict

What is exact.  The taps of the warp are taken as the kernel takes them, in fp32: fl = floor(d), t = d - fl (one
fp32 rounding where -1 < d < 0), i0 = j + (int)fl, and `valid` is the integer test on (i0, t).  valid, the mask and
the interior test are therefore the kernel's on every pixel, and so are the counts.  The constants are the fp32
ones the header names (0.81f, 0.1f, 1e-6f, 0.01f and the exponents 0.45f, 0.4f), widened.

What is bounded.  The blend, the grey values, the census terms and the score terms are evaluated in fp64 from
there.  With u = 2^-24 and T = the largest finite |value| of the two frames:

    W2_c      within 10 u T (tests/test_warp_host.py's committed bound of the blend)
    e_c       one more rounding: 10 u T + u |e_c|
    g1        three roundings: 3 u T;  g2: the mean of three W2 (10 u T) and three roundings: 13 u T
    d         g(x + o) - g(x): 2 e_g + u |d|, |d| <= 2 T:  8 u T for image 1, 28 u T for image 2
    c         d / sqrt(0.81 + d^2): |dc/dd| <= 0.81^-0.5 < 1.112 (at d = 0), and four fp32 operations of which the
              square root halves two: 3 u on |c| <= 1
    delta     c1 - c2: the two, and u |delta| <= 2 u:  1.112 * 36 u T + 8 u
    term      delta^2 / (0.1 + delta^2): |df/ddelta| <= 2.054 (at delta^2 = 0.1 / 3), and three fp32 operations
              on a value <= 1:  2.054 err_delta + 3 u
    h         P^2 terms and P^2 - 1 fp32 additions of non-negative partial sums <= h:
              P^2 err_term + (P^2 - 1) u (h + P^2 err_term)

The score functions are monotone in |e| and in h: a term at value t with input bound b moves by at most
max(f(t + b) - f(t), f(t) - f(max(t - b, 0))), evaluated in fp64 per pixel (no Lipschitz constant).  Their fp32
evaluation adds the roundings of the argument (two, damped by the exponent < 1/2: u f) and the device powf's own
error, pow_ulps units in the last place (ulp(f) <= 2 u f): (2 + 2 pow_ulps) u f.  pow_ulps is measured on the
GPU by tests/test_gpu_photo_metrics.py and never taken above POW_ULPS_CAP.  An fp64 sum of n terms in any order
lies within n 2^-53 sum |term| of the correctly rounded sum (math.fsum).

Shared by tests/test_photo_metrics_host.py, tests/test_gpu_photo_metrics.py and tests/golden/make_golden_photo.py."""
import functools
import math

import numpy as np

U = 2.0 ** -24
U53 = 2.0 ** -53
LIMIT = np.float32(2.0 ** 30)
POW_ULPS_CAP = 16
PATCHES = (3, 5, 7)
COUNTS = ("n_mask", "n_census", "n_valid", "n_nonfinite", "pixels")
SUMS = ("l1_sum", "photo_sum", "hamming_sum", "census_sum", "ternary_sum")
C081, C01, C1EM6, C001 = (float(np.float32(v)) for v in (0.81, 0.1, 1e-6, 0.01))
E045, E04 = float(np.float32(0.45)), float(np.float32(0.4))
DC_DD = 1.112       # >= 0.81f ** -0.5 = 1.11111...
DF_DDELTA = 2.054   # >= max |d/ddelta (delta^2 / (0.1 + delta^2))| = 2.05396... at delta^2 = 0.1 / 3


def f_photo(e):
    """(e^2 + 1e-6)^0.45: a photometric_loss term (charbonnier, beta = 255, in 0..255 units); ternary_loss's too."""
    return (np.square(e) + C1EM6) ** E045


def f_census(h):
    """(h + 0.01)^0.4: abs_robust_loss, a census_loss term."""
    return (h + C001) ** E04


f_ternary = f_photo


def as_nchw(frame):
    """A frame, float32 [B,3,H,W] or uint8 [B,H,W,3], as float64 [B,3,H,W]."""
    f = np.asarray(frame)
    if f.dtype == np.uint8:
        assert f.ndim == 4 and f.shape[3] == 3, f.shape
        return np.ascontiguousarray(f.transpose(0, 3, 1, 2)).astype(np.float64)
    assert f.dtype == np.float32 and f.ndim == 4 and f.shape[1] == 3, (f.dtype, f.shape)
    return f.astype(np.float64)


def _axis32(j, d, n):
    """One axis as warp_axis takes it, in fp32: (i0 int64, t float32 widened, inside)."""
    d = d.astype(np.float32)
    fl = np.floor(d)
    t = (d - fl).astype(np.float32)
    i0 = j + fl.astype(np.int64)
    inside = (i0 >= 0) & ((i0 < n - 1) | ((i0 == n - 1) & (t == 0)))
    return i0, t.astype(np.float64), inside


def warp(frame2, flow):
    """raft_warp_frame in zeros mode: the taps in fp32 (exact), the blend in fp64.  frame2 float64 [B,3,H,W], flow
    float32 [B,2,H,W].  Returns (W2 float64 [B,3,H,W], valid bool [B,H,W])."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32
    B, C, H, W = frame2.shape
    assert flow.shape == (B, 2, H, W), (frame2.shape, flow.shape)
    jj = np.broadcast_to(np.arange(W, dtype=np.int64)[None, None, :], (B, H, W))
    ii = np.broadcast_to(np.arange(H, dtype=np.int64)[None, :, None], (B, H, W))
    with np.errstate(invalid="ignore"):
        ok = (np.abs(flow[:, 0]) < LIMIT) & (np.abs(flow[:, 1]) < LIMIT)       # False for NaN and inf
    dx, dy = np.where(ok, flow[:, 0], np.float32(0)), np.where(ok, flow[:, 1], np.float32(0))
    x0, ax, inx = _axis32(jj, dx, W)
    y0, ay, iny = _axis32(ii, dy, H)
    bb = np.arange(B)[:, None, None]
    out = np.zeros((B, C, H, W))
    for c in range(C):
        taps = []
        for yy, xx in ((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)):
            m = ok & (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)    # outside the frame: 0, not read
            taps.append(np.where(m, frame2[bb, c, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0.0))
        v00, v01, v10, v11 = taps
        with np.errstate(invalid="ignore", over="ignore"):
            out[:, c] = (1 - ay) * ((1 - ax) * v00 + ax * v01) + ay * ((1 - ax) * v10 + ax * v11)
    return np.where(ok[:, None], out, 0.0), ok & inx & iny


def soft_hamming(g1, g2, patch):
    """h [B,H,W] of two grey images [B,H,W] in fp64: zero padding, the offsets in row-major order."""
    r = patch // 2
    p1, p2 = (np.pad(g, ((0, 0), (r, r), (r, r))) for g in (g1, g2))
    H, W = g1.shape[1:]
    h = np.zeros_like(g1)
    with np.errstate(invalid="ignore", over="ignore"):
        for dy in range(patch):
            for dx in range(patch):
                d1 = p1[:, dy:dy + H, dx:dx + W] - g1
                d2 = p2[:, dy:dy + H, dx:dx + W] - g2
                delta = d1 / np.sqrt(C081 + d1 * d1) - d2 / np.sqrt(C081 + d2 * d2)
                q = delta * delta
                h = h + q / (C01 + q)
    return h


def frame_scale(frame1, frame2):
    """T: the largest finite |value| of the two frames."""
    vals = np.concatenate([np.abs(as_nchw(f)).ravel() for f in (frame1, frame2)])
    vals = vals[np.isfinite(vals)]
    return float(vals.max()) if vals.size else 0.0


def term_bound(T):
    """The fp32 error bound of one term of h (the module docstring's chain)."""
    err_delta = DC_DD * 36.0 * U * T + 8.0 * U
    return DF_DDELTA * err_delta + 3.0 * U


def pixel_values(frame1, frame2, flow, patch):
    """The definition's per-pixel values in fp64 and their fp32 bounds: a dict with e [B,3,H,W], h [B,H,W], valid
    and interior bool [B,H,W], finite bool [B,H,W], e_bound [B,3,H,W], h_bound [B,H,W], T."""
    assert patch in PATCHES
    i1, i2 = as_nchw(frame1), as_nchw(frame2)
    B, _, H, W = i1.shape
    w2, valid = warp(i2, flow)
    with np.errstate(invalid="ignore", over="ignore"):
        e = i1 - w2
        g1 = (i1[:, 0] + i1[:, 1] + i1[:, 2]) / 3.0
        g2 = (w2[:, 0] + w2[:, 1] + w2[:, 2]) / 3.0
    h = soft_hamming(g1, g2, patch)
    r = patch // 2
    yy, xx = np.mgrid[:H, :W]
    interior = np.broadcast_to((xx >= r) & (xx < W - r) & (yy >= r) & (yy < H - r), (B, H, W))
    T = frame_scale(frame1, frame2)
    n = patch * patch
    tb = term_bound(T)
    with np.errstate(invalid="ignore"):
        h_bound = n * tb + (n - 1) * U * (h + n * tb)
        e_bound = 10.0 * U * T + U * np.abs(e) + 1e-37
    finite = np.isfinite(h) & np.isfinite(e).all(axis=1)
    return {"e": e, "h": h, "valid": valid, "interior": interior, "finite": finite, "e_bound": e_bound,
            "h_bound": h_bound, "T": T}


def mask_pixels(mask, shape):
    """bool [B,H,W]: bool / uint8 nonzero, float32 >= 0.5 (a NaN fails); None: every pixel."""
    if mask is None:
        return np.ones(shape, dtype=bool)
    m = np.asarray(mask).reshape(shape)
    with np.errstate(invalid="ignore"):
        return (m >= np.float32(0.5)) if m.dtype == np.float32 else (m != 0)


def moved(f, t, b):
    """How far the monotone f moves when its argument t >= 0 moves by at most b."""
    return np.maximum(f(t + b) - f(t), f(t) - f(np.maximum(t - b, 0.0)))


def metrics(frame1, frame2, flow, mask=None, patch=7, outgoing=True, pow_ulps=POW_ULPS_CAP):
    """One dict per sample: COUNTS as ints; SUMS as floats (math.fsum of the fp64 terms); "bound_<sum>", the
    largest distance of the kernel's sum from it; "census_map" and "census_map_bound" float64 [H,W]."""
    assert 0 <= pow_ulps <= POW_ULPS_CAP, pow_ulps       # the cap is a condition: a broken pow cannot hide behind it
    v = pixel_values(frame1, frame2, flow, patch)
    B, H, W = v["h"].shape
    m = mask_pixels(mask, (B, H, W))
    if outgoing:
        m = m & v["valid"]
    fp32 = (2.0 + 2.0 * pow_ulps) * U
    out = []
    for b in range(B):
        cnt = m[b] & v["finite"][b]
        cen = cnt & v["interior"][b]
        e, eb = np.abs(v["e"][b][:, cnt]), v["e_bound"][b][:, cnt]        # [3, n]
        h, hb = v["h"][b][cen], v["h_bound"][b][cen]
        terms = {"l1_sum": (e, eb), "photo_sum": (f_photo(e), moved(f_photo, e, eb) + fp32 * f_photo(e)),
                 "hamming_sum": (h, hb), "census_sum": (f_census(h), moved(f_census, h, hb) + fp32 * f_census(h)),
                 "ternary_sum": (f_ternary(h), moved(f_ternary, h, hb) + fp32 * f_ternary(h))}
        rec = {"n_mask": int(m[b].sum()), "n_census": int((m[b] & v["interior"][b]).sum()),
               "n_valid": int(v["valid"][b].sum()), "n_nonfinite": int((m[b] & ~v["finite"][b]).sum()),
               "pixels": H * W, "census_map": v["h"][b], "census_map_bound": v["h_bound"][b]}
        for k, (t, tb) in terms.items():
            rec[k] = math.fsum(t.ravel())
            rec["bound_" + k] = math.fsum(tb.ravel()) + t.size * U53 * math.fsum(np.abs(t).ravel())
        out.append(rec)
    return out


def totals(records):
    """The union of per-sample records: COUNTS summed, SUMS and their bounds by fsum, "images" = samples with
    n_census > 0, "image_census_mean_sum" = fsum of census_sum / n_census over them (and its bound)."""
    t = {k: sum(r[k] for r in records) for k in COUNTS}
    for k in SUMS:
        t[k] = math.fsum(r[k] for r in records)
        t["bound_" + k] = math.fsum(r["bound_" + k] for r in records) + len(records) * U53 * abs(t[k])
    with_census = [r for r in records if r["n_census"] > 0]
    t["images"] = len(with_census)
    means = [r["census_sum"] / r["n_census"] for r in with_census]
    t["image_census_mean_sum"] = math.fsum(means)
    t["bound_image_census_mean_sum"] = (math.fsum(r["bound_census_sum"] / r["n_census"] for r in with_census) +
                                        2 * (len(means) + 1) * U53 * math.fsum(means))
    return t


def result(t):
    """PhotoMetrics.result()'s dict from totals t (the arithmetic restated, not imported)."""
    nan = float("nan")
    tainted = t["n_nonfinite"] > 0

    def mean(a, n):
        return nan if tainted or n <= 0 else a / n

    px = t["pixels"]
    return {"census": nan if tainted or px <= 0 else t["census_sum"] / (t["n_census"] + 1e-6),
            "ternary": mean(t["ternary_sum"], px), "photo": mean(t["photo_sum"], 3 * px),
            "l1": mean(t["l1_sum"], 3 * t["n_mask"]), "hamming": mean(t["hamming_sum"], t["n_census"]),
            "census_image_mean": mean(t["image_census_mean_sum"], t["images"]),
            "valid_share": t["n_valid"] / px if px > 0 else nan, "pixels": px, "images": t["images"],
            "nonfinite": t["n_nonfinite"]}


# ----------------------------------------------------------------------------- the seeded cases


@functools.lru_cache(maxsize=None)
def photo_case(B, H, W, seed=5, sigma=2.5):
    """(frame1, frame2 float32 [B,3,H,W] with integer values in 0..255, flow float32 [B,2,H,W], mask float32
    [B,H,W] of 0 / 1 with about 85 % ones): a smooth image plus noise; frame 2 is frame 1 moved by about a pixel
    plus fresh noise; the flow is smooth (about 1 px) plus Gaussian noise of `sigma` px, so that a share of the
    targets leaves the frame.  uint8_frames() gives the uint8 case's frames.  The arrays are shared: read only."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    y, x = np.mgrid[:H, :W].astype(np.float64)
    f1 = np.empty((B, 3, H, W))
    for b in range(B):
        for c in range(3):
            k, ph = rng.uniform(0.5, 3.0, size=2), rng.uniform(0, 2 * np.pi, size=2)
            f1[b, c] = 127.5 + 90.0 * np.sin(2 * np.pi * k[0] * x / max(W, 2) + ph[0]) * np.cos(
                2 * np.pi * k[1] * y / max(H, 2) + ph[1])
    f1 = f1 + rng.uniform(-30, 30, size=f1.shape)
    f2 = np.roll(f1, (1, -1), axis=(2, 3)) + rng.uniform(-6, 6, size=f1.shape)
    flow = np.empty((B, 2, H, W))
    flow[:, 0] = -1.0 + 0.3 * np.sin(2 * np.pi * y / max(H, 2))
    flow[:, 1] = 1.0 + 0.3 * np.cos(2 * np.pi * x / max(W, 2))
    flow = flow + rng.standard_normal(flow.shape) * sigma
    mask = (rng.uniform(size=(B, H, W)) < 0.85).astype(np.float32)
    out = (np.clip(np.rint(f1), 0, 255).astype(np.float32), np.clip(np.rint(f2), 0, 255).astype(np.float32),
           flow.astype(np.float32), mask)
    for a in out:
        a.setflags(write=False)
    return out


def uint8_frame(frame):
    """The uint8 [B,H,W,3] version of an integer-valued float frame [B,3,H,W]."""
    return np.ascontiguousarray(np.asarray(frame).astype(np.uint8).transpose(0, 2, 3, 1))
