"""raft_flow_metrics' definition (include/raft_hip.h) in numpy: every per-pixel operation in fp32, rounded to
nearest and unfused (numpy's float32 +, -, *, / and sqrt are IEEE operations), counts as Python integers and
sums with math.fsum, which returns the correctly rounded sum.  Reads only arrays.

    metrics(flow, flow_gt, valid=None, gt_limit=None) -> dict per sample list, see below
    totals(records)                                   -> the union of records, with images / image_mean_sum

Shared by tests/test_flow_metrics_host.py and tests/test_gpu_flow_metrics.py."""
import math

import numpy as np

COUNTS = ("n", "n_nonfinite", "n_lt1", "n_lt3", "n_lt5", "n_outlier", "n_s0_10", "n_s10_40", "n_s40")
SUMS = ("epe_sum", "epe_sum_s0_10", "epe_sum_s10_40", "epe_sum_s40")
CANONICAL_NAN = np.uint32(0x7FC00000)     # the NaN an epe_map holds


def pixel_values(flow, flow_gt):
    """(epe, mag, ratio), float32 arrays [B,H,W]: the definition's per-pixel values at every pixel."""
    f = np.asarray(flow)
    g = np.asarray(flow_gt)
    assert f.dtype == np.float32 and g.dtype == np.float32 and f.shape == g.shape and f.shape[1] == 2
    with np.errstate(all="ignore"):
        du, dv = f[:, 0] - g[:, 0], f[:, 1] - g[:, 1]
        epe = np.sqrt(du * du + dv * dv)
        mag = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
        ratio = epe / mag
    assert epe.dtype == mag.dtype == ratio.dtype == np.float32
    return epe, mag, ratio


def valid_pixels(flow_gt, valid=None, gt_limit=None):
    """bool [B,H,W]: the mask says so (bool / uint8: nonzero; float32: >= 0.5, a NaN fails) and, with gt_limit,
    |gu| < gt_limit and |gv| < gt_limit (a NaN fails)."""
    g = np.asarray(flow_gt)
    B, _, H, W = g.shape
    ok = np.ones((B, H, W), dtype=bool)
    if valid is not None:
        v = np.asarray(valid).reshape(B, H, W)
        with np.errstate(invalid="ignore"):
            ok &= (v >= np.float32(0.5)) if v.dtype == np.float32 else (v != 0)
    if gt_limit is not None:
        lim = np.float32(gt_limit)
        with np.errstate(invalid="ignore"):
            ok &= (np.abs(g[:, 0]) < lim) & (np.abs(g[:, 1]) < lim)
    return ok


def metrics(flow, flow_gt, valid=None, gt_limit=None):
    """One dict per sample: the COUNTS as ints, the SUMS as floats (math.fsum of the fp32 epe values, widened),
    "abs_sum" and "abs_sum_<class>" (fsum of |epe| over the same pixels: the error bound's scale), and
    "epe_map" float32 [H,W] (epe at valid pixels, the canonical NaN at invalid ones and for a NaN epe)."""
    epe, mag, ratio = pixel_values(flow, flow_gt)
    ok = valid_pixels(flow_gt, valid, gt_limit)
    out = []
    for b in range(epe.shape[0]):
        e, m, r, v = epe[b], mag[b], ratio[b], ok[b]
        with np.errstate(invalid="ignore"):
            fin = v & (np.abs(e) < np.float32(np.inf))
            cls = (fin & (m < np.float32(10)), fin & (m >= np.float32(10)) & (m < np.float32(40)),
                   fin & (m >= np.float32(40)))
            rec = {"n": int(v.sum()), "n_nonfinite": int((v & ~fin).sum()),
                   "n_lt1": int((fin & (e < np.float32(1))).sum()), "n_lt3": int((fin & (e < np.float32(3))).sum()),
                   "n_lt5": int((fin & (e < np.float32(5))).sum()),
                   "n_outlier": int((fin & (e > np.float32(3)) & (r > np.float32(0.05))).sum()),
                   "n_s0_10": int(cls[0].sum()), "n_s10_40": int(cls[1].sum()), "n_s40": int(cls[2].sum())}
        for name, sel in zip(SUMS, (fin,) + cls):
            vals = e[sel].astype(np.float64)
            rec[name] = math.fsum(vals)
            rec["abs_" + name[4:]] = math.fsum(np.abs(vals))
        emap = np.where(v, e, np.float32(np.nan)).astype(np.float32)
        bits = emap.view(np.uint32).copy()
        bits[np.isnan(emap)] = CANONICAL_NAN
        rec["epe_map"] = bits.view(np.float32)
        out.append(rec)
    return out


def totals(records):
    """The union of per-sample records: COUNTS summed, SUMS (and abs sums) by fsum, "images" = samples with
    n > 0, "image_mean_sum" = fsum of epe_sum / n over them."""
    t = {k: sum(r[k] for r in records) for k in COUNTS}
    for k in SUMS:
        t[k] = math.fsum(r[k] for r in records)
        t["abs_" + k[4:]] = math.fsum(r["abs_" + k[4:]] for r in records)
    with_pixels = [r for r in records if r["n"] > 0]
    t["images"] = len(with_pixels)
    t["image_mean_sum"] = math.fsum(r["epe_sum"] / r["n"] for r in with_pixels)
    return t


def result(t):
    """FlowMetrics.result()'s dict from totals t."""
    nan = float("nan")
    tainted = t["n_nonfinite"] > 0

    def ratio(a, n, scale=1.0):
        return scale * a / n if n > 0 else nan

    def mean(a, n):
        return nan if tainted else ratio(a, n)

    n = t["n"]
    return {"epe": mean(t["epe_sum"], n), "1px": ratio(t["n_lt1"], n), "3px": ratio(t["n_lt3"], n),
            "5px": ratio(t["n_lt5"], n), "f1": nan if tainted else ratio(t["n_outlier"], n, 100.0),
            "epe_image_mean": mean(t["image_mean_sum"], t["images"]),
            "s0-10": mean(t["epe_sum_s0_10"], t["n_s0_10"]), "s10-40": mean(t["epe_sum_s10_40"], t["n_s10_40"]),
            "s40+": mean(t["epe_sum_s40"], t["n_s40"]), "pixels": n, "images": t["images"],
            "nonfinite": t["n_nonfinite"]}


def threshold_pixels():
    """Hand-made pixels around every threshold of the definition, as (flow, flow_gt, valid) with flow and
    flow_gt float32 [1,2,1,N] and valid float32 [1,1,N], and the expected record as a dict of COUNTS
    (derived by hand below, not by metrics()).  gt_limit = 1000 is part of the case."""
    f32, nxt = np.float32, np.nextafter
    up = lambda x: nxt(f32(x), f32(np.inf))       # noqa: E731
    dn = lambda x: nxt(f32(x), f32(-np.inf))      # noqa: E731
    px = []   # (u, v, gu, gv, mask, counted-in)

    def add(u, v, gu, gv, mask=1.0, **k):
        px.append((f32(u), f32(v), f32(gu), f32(gv), f32(mask), k))

    # epe exactly 1, 3, 5 (differences (0,1), (0,3), (3,4)) and one ulp either side; ground truth (100, 0):
    # mag = 100, class s40; ratio = epe / 100 (outlier needs epe > 3 and ratio > 0.05: epe > 5 here).
    add(100, 1, 100, 0, lt3=1, lt5=1, s40=1)                    # epe == 1: not < 1
    add(100, dn(1), 100, 0, lt1=1, lt3=1, lt5=1, s40=1)
    add(100, up(1), 100, 0, lt3=1, lt5=1, s40=1)
    add(100, 3, 100, 0, lt5=1, s40=1)                           # epe == 3: not < 3, not > 3
    add(100, dn(3), 100, 0, lt3=1, lt5=1, s40=1)
    add(100, up(3), 100, 0, lt5=1, s40=1)                       # epe > 3 but ratio 0.03: no outlier
    add(103, 4, 100, 0, s40=1)                          # epe == 5: not < 5; ratio = fl(5 / 100) == fl(0.05): not >
    add(100, dn(5), 100, 0, lt5=1, s40=1)
    add(100, up(5), 100, 0, s40=1, outlier=1)                   # ratio = fl(5.0000005 / 100) > fl(0.05)
    # mag exactly 10 and 40 (ground truth (6,8) and (24,32)), and one ulp below (ground truth (x, 0) has
    # mag = sqrt(x * x) = |x| exactly); prediction == ground truth
    add(6, 8, 6, 8, lt1=1, lt3=1, lt5=1, s10_40=1)
    add(dn(10), 0, dn(10), 0, lt1=1, lt3=1, lt5=1, s0_10=1)
    add(24, 32, 24, 32, lt1=1, lt3=1, lt5=1, s40=1)
    add(dn(40), 0, dn(40), 0, lt1=1, lt3=1, lt5=1, s10_40=1)
    # mag == 0: ratio = epe / 0 = inf (epe > 0) -> outlier when epe > 3; 0 / 0 = NaN -> no outlier
    add(0, 4, 0, 0, lt5=1, s0_10=1, outlier=1)
    add(0, 0, 0, 0, lt1=1, lt3=1, lt5=1, s0_10=1)
    # a ratio one ulp either side of 0.05: epe = 4 exactly (difference (0, 4)); mag = 80 gives 4 / 80, which
    # rounds to fl(0.05): not > 0.05.  mag one ulp below / above 80 moves the quotient by 1.08 ulp of 0.05.
    add(80, 4, 80, 0, lt5=1, s40=1)
    add(dn(80), 4, dn(80), 0, lt5=1, s40=1, outlier=1)
    add(up(80), 4, up(80), 0, lt5=1, s40=1)
    # mask 0.5 against the float just below it
    add(1, 1, 1, 1, mask=0.5, lt1=1, lt3=1, lt5=1, s0_10=1)
    add(1, 1, 1, 1, mask=dn(0.5), invalid=1)
    # ground truth +-1000 against the float just below 1000 (gt_limit = 1000)
    add(0, 0, 1000, 0, invalid=1)
    add(0, 0, 0, -1000, invalid=1)
    add(dn(1000), 0, dn(1000), 0, lt1=1, lt3=1, lt5=1, s40=1)
    add(0, -dn(1000), 0, -dn(1000), lt1=1, lt3=1, lt5=1, s40=1)
    # NaN and +-inf: in the prediction (valid, not finite), in the ground truth (fails gt_limit), in the mask
    add(np.nan, 0, 1, 1, nonfinite=1)
    add(0, np.inf, 1, 1, nonfinite=1)
    add(-np.inf, 0, 1, 1, nonfinite=1)
    add(0, 0, np.nan, 1, invalid=1)
    add(0, 0, 1, np.inf, invalid=1)
    add(0, 0, -np.inf, 1, invalid=1)
    add(1, 1, 1, 1, mask=np.nan, invalid=1)
    add(1, 1, 1, 1, mask=np.inf, lt1=1, lt3=1, lt5=1, s0_10=1)  # inf >= 0.5
    add(1, 1, 1, 1, mask=-np.inf, invalid=1)
    arr = np.array([p[:5] for p in px], dtype=np.float32)
    N = len(px)
    flow = np.ascontiguousarray(arr[:, 0:2].T.reshape(1, 2, 1, N))
    gt = np.ascontiguousarray(arr[:, 2:4].T.reshape(1, 2, 1, N))
    mask = np.ascontiguousarray(arr[:, 4].reshape(1, 1, N))
    want = {k: 0 for k in COUNTS}
    for p in px:
        k = p[5]
        if k.get("invalid"):
            continue
        want["n"] += 1
        want["n_nonfinite"] += k.get("nonfinite", 0)
        for name in ("lt1", "lt3", "lt5", "outlier", "s0_10", "s10_40", "s40"):
            want["n_" + name] += k.get(name, 0)
    return flow, gt, mask, want
