"""The flow-metrics additions that need no GPU: the numpy oracle (tests/flow_metrics_oracle.py) on hand-made pixels
around every threshold and against the reference's torch arithmetic (evaluate.py's validate_* lines) on random
fields; argument validation of utils.flow_errors and utils.FlowMetrics; the new C-ABI entries' argument errors,
symbols and sources.

tests/test_gpu_flow_metrics.py imports the random cases (metrics_case) and the threshold pixels."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import flow_metrics_oracle as FM
from raft_optical_flow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS_EPE = (1.0, 3.0, 5.0)
THRESHOLD_RATIO = 0.05


@functools.lru_cache(maxsize=None)
def metrics_case(B, H, W, seed=0):
    """(flow, flow_gt, valid) float32: ground truth of magnitude up to ~70 px (all three speed classes), a
    prediction off by up to ~8 px (both sides of 1, 3 and 5 px and of the 5 % ratio), |difference| >= 2^-40 so
    that no square underflows; valid float32 [B,H,W] in {0, 0.25, 0.5, 0.75, 1}."""
    rng = np.random.default_rng(1000 * seed + 31 * H + W)
    gt = (rng.uniform(-1.0, 1.0, size=(B, 2, H, W)) * rng.choice([2.0, 20.0, 50.0], size=(B, 1, H, W))).astype(
        np.float32)
    err = rng.standard_normal((B, 2, H, W)) * rng.choice([0.3, 2.0, 4.0], size=(B, 1, H, W))
    flow = (gt + err).astype(np.float32)
    d = np.abs(flow - gt)
    assert d.min() >= 2.0 ** -40 and max(np.abs(flow).max(), np.abs(gt).max()) <= 2.0 ** 40
    valid = rng.choice(np.array([0, 0.25, 0.5, 0.75, 1], dtype=np.float32), size=(B, H, W))
    for a in (flow, gt, valid):
        a.setflags(write=False)
    return flow, gt, valid


# ----------------------------------------------------------------------------- the oracle


def test_oracle_threshold_pixels():
    """Every hand-derived count of the threshold pixels, and the values the derivations rest on."""
    flow, gt, mask, want = FM.threshold_pixels()
    (rec,) = FM.metrics(flow, gt, mask, gt_limit=1000.0)
    assert {k: rec[k] for k in FM.COUNTS} == want
    epe, mag, ratio = (a.reshape(-1) for a in FM.pixel_values(flow, gt))
    f32 = np.float32
    up = lambda x: np.nextafter(f32(x), f32(np.inf))      # noqa: E731
    dn = lambda x: np.nextafter(f32(x), f32(-np.inf))     # noqa: E731
    assert list(epe[:9]) == [1, dn(1), up(1), 3, dn(3), up(3), 5, dn(5), up(5)]
    assert ratio[6] == f32(0.05) and ratio[8] == up(0.05) and ratio[7] == dn(0.05)
    assert list(mag[9:13]) == [10, dn(10), 40, dn(40)]
    assert mag[13] == 0 and np.isinf(ratio[13]) and np.isnan(ratio[14])
    assert list(ratio[15:18]) == [f32(0.05), up(0.05), dn(0.05)] and list(epe[15:18]) == [4, 4, 4]
    # the finite valid pixels' sum is exact here (fsum), and the map holds NaN exactly at the invalid pixels
    ok = FM.valid_pixels(gt, mask, 1000.0).reshape(-1)
    fin = ok & np.isfinite(epe)
    assert rec["epe_sum"] == math.fsum(epe[fin].astype(np.float64))
    m = rec["epe_map"].reshape(-1)
    assert np.array_equal(np.isnan(m), ~ok | np.isnan(epe))
    assert np.all(m.view(np.uint32)[np.isnan(m)] == FM.CANONICAL_NAN)
    assert np.array_equal(m[ok & ~np.isnan(epe)], epe[ok & ~np.isnan(epe)])
    # without the limit the +-1000 pixels count, and non-finite ground truth is a non-finite epe
    (rec2,) = FM.metrics(flow, gt, mask)
    assert rec2["n"] == rec["n"] + 5 and rec2["n_nonfinite"] == rec["n_nonfinite"] + 3
    # speed classes partition the finite valid pixels
    for r in (rec, rec2):
        assert r["n_s0_10"] + r["n_s10_40"] + r["n_s40"] == r["n"] - r["n_nonfinite"]
        assert math.isclose(r["epe_sum_s0_10"] + r["epe_sum_s10_40"] + r["epe_sum_s40"], r["epe_sum"], rel_tol=1e-15)


def test_oracle_mask_dtypes_and_shapes():
    flow, gt, valid = metrics_case(2, 7, 9)
    want = FM.metrics(flow, gt, valid)
    as_bool = valid >= 0.5
    for v in (as_bool, as_bool.astype(np.uint8) * 7, as_bool.reshape(2, 1, 7, 9), valid.reshape(2, 1, 7, 9)):
        got = FM.metrics(flow, gt, v)
        assert [{k: r[k] for k in FM.COUNTS + FM.SUMS} for r in got] == \
               [{k: r[k] for k in FM.COUNTS + FM.SUMS} for r in want]
    assert FM.metrics(flow, gt)[0]["n"] == 63 and 0 < want[0]["n"] < 63


def test_oracle_sqrt_and_divide_are_correctly_rounded():
    """numpy's float32 sqrt and divide against the fp64 operation rounded to fp32 (53 >= 2 * 24 + 2 bits: the
    double rounding is innocuous for sqrt and for the quotient of two fp32 values)."""
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 100, size=200000).astype(np.float32)
    y = rng.uniform(0.01, 100, size=200000).astype(np.float32)
    assert np.array_equal(np.sqrt(x), np.sqrt(x.astype(np.float64)).astype(np.float32))
    assert np.array_equal(x / y, (x.astype(np.float64) / y.astype(np.float64)).astype(np.float32))


def reference_counts(flow, gt, valid):
    """evaluate.py's arithmetic in torch on the host, per sample: (epe, out, val) as numpy arrays [H*W]."""
    res = []
    for b in range(flow.shape[0]):
        f, g = torch.from_numpy(flow[b].copy()), torch.from_numpy(gt[b].copy())
        epe = torch.sum((f - g) ** 2, dim=0).sqrt()                     # evaluate.py:115 / :148
        mag = torch.sum(g ** 2, dim=0).sqrt()                           # :149
        epe, mag = epe.view(-1), mag.view(-1)
        val = torch.from_numpy(valid[b].copy()).view(-1) >= 0.5         # :153
        out = ((epe > 3.0) & ((epe / mag) > 0.05)).float()              # :155
        res.append((epe.numpy(), out.numpy(), val.numpy()))
    return res


def near_threshold(flow, gt, ulps=2):
    """bool [B,H,W]: the oracle's fp32 epe lies within `ulps` ulp of 1, 3 or 5, or its ratio of 0.05."""
    epe, _, ratio = FM.pixel_values(flow, gt)
    near = np.zeros(epe.shape, dtype=bool)
    for vals, ts in ((epe, THRESHOLDS_EPE), (ratio, (THRESHOLD_RATIO,))):
        for t in ts:
            t = np.float32(t)
            near |= np.abs(vals.astype(np.float64) - float(t)) <= ulps * float(np.spacing(t))
    return near


@pytest.mark.parametrize("shape,seed", [((2, 120, 200), 0), ((1, 436, 344), 1)])
def test_oracle_matches_reference_torch_arithmetic(shape, seed):
    """Every count the reference forms, from its own torch lines, equals the oracle's after leaving out the pixels
    within 2 ulp of a threshold (torch's vectorised sqrt is not correctly rounded); the seeds are chosen so that
    no pixel is left out.  The mean EPE agrees to the fp32 ulp per pixel that sqrt may differ by."""
    flow, gt, valid = metrics_case(*shape, seed=seed)
    near = near_threshold(flow, gt)
    assert near.mean() == 0.0                                     # the left-out share
    keep = ~near
    ref = reference_counts(flow, gt, valid)
    for b, (epe, out, val) in enumerate(ref):
        k = keep[b].reshape(-1)
        with_mask = FM.metrics(flow[b:b + 1] * 1, gt[b:b + 1] * 1, np.where(keep[b], valid[b], 0)[None])[0]
        no_mask = FM.metrics(flow[b:b + 1] * 1, gt[b:b + 1] * 1, keep[b][None])[0]
        # validate_sintel: all pixels; np.mean(epe_all < k) * N
        assert no_mask["n"] == int(k.sum())
        for name, t in zip(("n_lt1", "n_lt3", "n_lt5"), THRESHOLDS_EPE):
            assert no_mask[name] == int((epe[k] < t).sum()), name
        # validate_kitti: out[val]
        assert with_mask["n"] == int((val & k).sum())
        assert with_mask["n_outlier"] == int(out[val & k].sum())
        assert 0 < with_mask["n_outlier"] < with_mask["n"]
        mean_ref = float(epe[val & k].mean(dtype=np.float64))
        mean = with_mask["epe_sum"] / with_mask["n"]
        assert abs(mean - mean_ref) <= float(np.spacing(np.float32(epe.max())))


def test_totals_and_result():
    flow, gt, valid = metrics_case(2, 7, 9)
    empty = np.zeros((1, 7, 9), dtype=np.float32)
    recs = FM.metrics(flow, gt, valid) + FM.metrics(flow[:1] * 1, gt[:1] * 1, empty)
    t = FM.totals(recs)
    assert t["images"] == 2 and t["n"] == recs[0]["n"] + recs[1]["n"] and recs[2]["n"] == 0
    r = FM.result(t)
    assert r["pixels"] == t["n"] and r["images"] == 2 and r["nonfinite"] == 0
    assert r["epe_image_mean"] == (recs[0]["epe_sum"] / recs[0]["n"] + recs[1]["epe_sum"] / recs[1]["n"]) / 2
    assert r["f1"] == 100.0 * t["n_outlier"] / t["n"] and r["1px"] == t["n_lt1"] / t["n"]
    bad = flow.copy()
    bad[0, 0, 0, 0] = np.inf
    r = FM.result(FM.totals(FM.metrics(bad, gt)))
    assert r["nonfinite"] == 1 and all(math.isnan(r[k]) for k in ("epe", "f1", "epe_image_mean", "s0-10", "s40+"))
    assert r["1px"] == FM.totals(FM.metrics(bad, gt))["n_lt1"] / 126
    assert math.isnan(FM.result(FM.totals([]))["epe"])


# ----------------------------------------------------------------------------- argument checks


def test_flow_errors_argument_checks():
    from raft_optical_flow_amd.utils import FlowErrors, flow_errors
    assert FlowErrors._fields == FM.COUNTS + FM.SUMS + ("epe_map",)
    fl, gt = torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8)
    with pytest.raises(RuntimeError, match="ROCm GPU only"):       # CPU tensors: there is no CPU path
        flow_errors(fl, gt)
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        flow_errors(fl, gt, valid=torch.ones(1, 8, 8, dtype=torch.bool), gt_limit=1000)
    with pytest.raises(TypeError, match="flow must be a tensor"):
        flow_errors(fl.numpy(), gt)
    with pytest.raises(TypeError, match="flow_gt must be a tensor"):
        flow_errors(fl, gt.numpy())
    with pytest.raises(TypeError, match="flow must be float32"):
        flow_errors(fl.double(), gt)
    with pytest.raises(TypeError, match="flow_gt must be float32"):
        flow_errors(fl, gt.half())
    for bad in (torch.zeros(2, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 0, 8)):
        with pytest.raises(ValueError, match=r"\[B, 2, H, W\]"):
            flow_errors(bad, gt)
    for bad in (torch.zeros(1, 2, 8, 9), torch.zeros(2, 2, 8, 8), torch.zeros(2, 8, 8)):
        with pytest.raises(ValueError, match="differ in shape"):
            flow_errors(fl, bad)
    with pytest.raises(TypeError, match="valid must be a tensor"):
        flow_errors(fl, gt, valid=np.ones((1, 8, 8), dtype=bool))
    for dt in (torch.float64, torch.int32, torch.float16):
        with pytest.raises(TypeError, match="bool, uint8 or float32"):
            flow_errors(fl, gt, valid=torch.ones(1, 8, 8, dtype=dt))
    for shape in ((8, 8), (1, 8, 9), (1, 2, 8, 8), (2, 8, 8), (1, 1, 1, 8, 8)):
        with pytest.raises(ValueError, match="valid must be"):
            flow_errors(fl, gt, valid=torch.ones(*shape))
    for bad in ("1000", True, [1000.0]):
        with pytest.raises(TypeError, match="gt_limit must be a number"):
            flow_errors(fl, gt, gt_limit=bad)
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gt_limit must be positive"):
            flow_errors(fl, gt, gt_limit=bad)


def test_flow_metrics_argument_checks():
    from raft_optical_flow_amd.utils import FlowMetrics
    with pytest.raises(ValueError, match="gt_limit must be positive"):
        FlowMetrics(gt_limit=0.0)
    with pytest.raises(TypeError, match="gt_limit must be a number"):
        FlowMetrics(gt_limit="1000")
    m = FlowMetrics(gt_limit=1000)
    assert m.gt_limit == 1000.0 and FlowMetrics().gt_limit == 0.0
    fl, gt = torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8)
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        m.update(fl, gt)
    with pytest.raises(TypeError, match="flow must be float32"):
        m.update(fl.double(), gt)
    with pytest.raises(ValueError, match="differ in shape"):
        m.update(fl, torch.zeros(1, 2, 8, 9))
    with pytest.raises(TypeError, match="bool, uint8 or float32"):
        m.update(fl, gt, torch.ones(1, 8, 8, dtype=torch.int64))
    # nothing accumulated: every mean over nothing is NaN, the counts are 0; reset() is harmless
    m.reset()
    r = m.result()
    assert set(r) == {"epe", "1px", "3px", "5px", "f1", "epe_image_mean", "s0-10", "s10-40", "s40+", "pixels",
                      "images", "nonfinite"}
    assert r["pixels"] == r["images"] == r["nonfinite"] == 0
    assert all(math.isnan(r[k]) for k in ("epe", "1px", "3px", "5px", "f1", "epe_image_mean", "s0-10", "s40+"))


FAKE = 1 << 20  # 16-byte aligned stand-in pointers: an argument error returns before any launch


def test_metrics_symbols_and_argument_errors():
    lib = _lib.load()
    for name in ("raft_flow_metrics_ws_bytes", "raft_flow_metrics"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.raft_hip_abi_version() == 19 and _lib.ABI_VERSION == 19   # additive entries
    assert (_lib.MASK_U8, _lib.MASK_F32) == (0, 1)
    assert _lib.FM_COUNTS == FM.COUNTS and _lib.FM_SUMS == FM.SUMS
    P, G = _lib.FM_BLOCK_PIXELS, _lib.FM_MAX_BLOCKS
    rec = _lib.FM_SLOTS * 8
    ws = lib.raft_flow_metrics_ws_bytes
    assert ws(1, 1, 1) == rec and ws(1, 1, P) == rec and ws(1, 1, P + 1) == 2 * rec
    assert ws(3, G, P) == 3 * G * rec and ws(3, G, P + 1) == 3 * G * rec          # the cap: larger samples wrap
    assert ws(2, 37, 53) == 2 * 2 * rec
    assert ws(0, 8, 8) == 0 and ws(1, -1, 8) == 0 and ws(1 << 10, 1 << 10, 1 << 10) == 0
    err = lib.raft_hip_last_error
    p = [FAKE * k for k in range(1, 8)]

    def call(**kw):
        a = dict(flow=p[0], fsb=128, fsc=64, fp=8, gt=p[1], gsb=128, gsc=64, gp=8, valid=p[2], tag=_lib.MASK_F32,
                 vsb=64, vp=8, B=1, H=8, W=8, limit=0.0, record=p[3], totals=p[4], emap=p[5], ws=p[6])
        a.update(kw)
        return lib.raft_flow_metrics(*a.values(), None)

    for k in ("flow", "gt", "record", "ws"):
        assert call(**{k: None}) == -1 and b"null pointer" in err()
    big = {"B": 1 << 10, "H": 1 << 10, "W": 1 << 10, "fp": 1 << 10, "gp": 1 << 10, "vp": 1 << 10}
    for kw in ({"B": 0}, {"H": -1}, {"W": 0}, big):
        assert call(**kw) == -1 and b"bad size" in err()
    for tag in (2, -1):
        assert call(tag=tag) == -1 and b"unknown mask dtype" in err()
    for lim in (float("nan"), float("inf")):
        assert call(limit=lim) == -1 and b"gt_limit" in err()
    for kw in ({"fp": 7}, {"gp": 7}, {"fsb": -1}, {"fsc": -1}, {"gsb": -1}, {"gsc": -64}):
        assert call(**kw) == -1 and b"bad strides" in err()
    for kw in ({"vp": 7}, {"vsb": -1}):
        assert call(**kw) == -1 and b"bad mask strides" in err()
    for kw in ({"flow": p[0] + 2}, {"gt": p[1] + 1}, {"valid": p[2] + 2}, {"emap": p[5] + 2}, {"record": p[3] + 4},
               {"totals": p[4] + 4}, {"ws": p[6] + 2}):
        assert call(**kw) == -1 and b"misaligned" in err()
    for kw in ({"record": p[0]}, {"record": p[1]}, {"record": p[2]}, {"totals": p[0]}, {"totals": p[3]},
               {"emap": p[1]}, {"emap": p[3]}, {"ws": p[2]}, {"ws": p[3]}, {"ws": p[4]}, {"ws": p[5]}):
        assert call(**kw) == -1 and b"aliases" in err()
    # an absent mask: its tag and strides are not read, and a byte mask needs no alignment
    # (the alias check is the last one: reaching it shows that the earlier ones passed)
    assert call(valid=None, tag=9, vsb=-1, vp=0, ws=p[3]) == -1 and b"aliases" in err()
    assert call(valid=p[2] + 1, tag=_lib.MASK_U8, ws=p[3]) == -1 and b"aliases" in err()
    assert call(totals=None, emap=None, limit=-5.0, ws=p[3]) == -1 and b"aliases" in err()


def test_sources_mention_the_new_file_and_entries():
    with open(os.path.join(ROOT, "raft_optical_flow_amd", "csrc", "Makefile")) as fh:
        srcs = next(ln for ln in fh if ln.startswith("SRCS :="))
    assert "flow_metrics.hip" in srcs.split()                    # built, and hashed with the rest
    with open(os.path.join(ROOT, "include", "raft_hip.h")) as fh:
        hdr = fh.read()
    for name in ("raft_flow_metrics(", "raft_flow_metrics_ws_bytes(", "#define RAFT_HIP_ABI_VERSION 19",
                 "#define RAFT_FLOW_METRICS_SLOTS 16", f"#define RAFT_FLOW_METRICS_BLOCK_PIXELS {_lib.FM_BLOCK_PIXELS}",
                 f"#define RAFT_FLOW_METRICS_MAX_BLOCKS {_lib.FM_MAX_BLOCKS}", "#define RAFT_MASK_U8 0",
                 "#define RAFT_MASK_F32 1"):
        assert name in hdr, name
    slots = [n.upper() for n in FM.COUNTS + FM.SUMS] + ["IMAGES", "IMAGE_MEAN_SUM", "RESERVED"]
    for i, n in enumerate(slots):
        assert f"#define RAFT_FM_{n} {i}\n" in hdr, n
    assert (_lib.FM_IMAGES, _lib.FM_IMAGE_MEAN_SUM, _lib.FM_RESERVED) == (13, 14, 15)
    with open(os.path.join(ROOT, "raft_optical_flow_amd", "csrc", "flow_metrics.hip")) as fh:
        src = fh.read()
    assert 'extern "C" int raft_flow_metrics(' in src and 'extern "C" size_t raft_flow_metrics_ws_bytes(' in src
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.replace("no atomics", "")
    from raft_optical_flow_amd.utils import utils as U_
    for word in ("flow_errors", "FlowMetrics", "validate_chairs", "validate_sintel", "validate_kitti"):
        assert word in U_.__doc__, word
