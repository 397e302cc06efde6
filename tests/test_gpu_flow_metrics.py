"""raft_flow_metrics, utils.flow_errors and utils.FlowMetrics on the GPU, against tests/flow_metrics_oracle.py.

Counts equal the oracle's exactly.  An fp64 sum of n fp32 terms lies within n * 2^-53 * sum |epe| of the
correctly rounded sum (math.fsum), whatever the order of the additions.  epe_map equals the oracle's bit for
bit.  Every output and workspace buffer the kernel tests hand to the C entry is prefilled with 0xFF bytes (NaN as
float32 and as float64, -1 as int64); running totals are the exception: the call adds into them.  The inputs keep
|flow - flow_gt| in [2^-40, 2^40], so no square underflows."""
import argparse
import functools
import math

import numpy as np
import pytest
import torch

import flow_metrics_oracle as FM
import test_flow_metrics_host as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
U53 = 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)      # (a copy: the shared cases are read-only)


def nan_bytes(shape, dtype):
    """A device buffer of 0xFF bytes."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(0xFF)
    return t


def launch(flow, gt, valid=None, gt_limit=None, epe_map=True, totals=None):
    """raft_flow_metrics on device tensors of any strides, every output prefilled with NaN bytes: returns
    (records as a list of dicts, epe_map numpy [B,H,W] or None, raw record int64 numpy [B,16])."""
    from raft_optical_flow_amd import _lib as L
    B, _, H, W = flow.shape
    assert flow.stride(3) == 1 and gt.stride(3) == 1
    vp, tag, vsb, vpitch = None, 0, 0, 0
    if valid is not None:
        v = valid.reshape(B, H, W) if valid.dim() == 4 else valid
        tag = L.MASK_F32 if v.dtype == torch.float32 else L.MASK_U8
        vp, vsb, vpitch = v.data_ptr(), v.stride(0), v.stride(1)
    record = nan_bytes((B, L.FM_SLOTS), torch.int64)
    ws = nan_bytes((L.load().raft_flow_metrics_ws_bytes(B, H, W) // 8,), torch.int64)
    emap = nan_bytes((B, 1, H, W), torch.float32) if epe_map else None
    L.call("raft_flow_metrics", flow.data_ptr(), flow.stride(0), flow.stride(1), flow.stride(2), gt.data_ptr(),
           gt.stride(0), gt.stride(1), gt.stride(2), vp, tag, vsb, vpitch, B, H, W,
           0.0 if gt_limit is None else float(gt_limit), record.data_ptr(),
           None if totals is None else totals.data_ptr(), None if emap is None else emap.data_ptr(), ws.data_ptr(),
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw = record.cpu().numpy()
    return [unpack(r) for r in raw], (emap[:, 0].cpu().numpy() if epe_map else None), raw


def unpack(row):
    """One record (int64 [16]) as a dict: the counts, the sums, images, image_mean_sum, reserved."""
    row = np.ascontiguousarray(row, dtype=np.int64)
    f = row.view(np.float64)
    d = {k: int(row[i]) for i, k in enumerate(FM.COUNTS)}
    d.update({k: float(f[len(FM.COUNTS) + i]) for i, k in enumerate(FM.SUMS)})
    d.update(images=int(row[13]), image_mean_sum=float(f[14]), reserved=int(row[15]))
    return d


TERMS = {"epe_sum": None, "epe_sum_s0_10": "n_s0_10", "epe_sum_s10_40": "n_s10_40", "epe_sum_s40": "n_s40"}


def check_record(got, want, what=""):
    """Counts exactly; every sum within n * 2^-53 * sum |epe| of the fsum value (n the sum's number of terms)."""
    for k in FM.COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k, cnt in TERMS.items():
        n = want["n"] - want["n_nonfinite"] if cnt is None else want[cnt]
        bound = n * U53 * want["abs_" + k[4:]]
        assert abs(got[k] - want[k]) <= bound, (what, k, got[k], want[k], bound)
    assert got["reserved"] == 0, what


def check_sample_records(recs, wants, what=""):
    for b, (g, w) in enumerate(zip(recs, wants)):
        check_record(g, w, f"{what} sample {b}")
        assert g["images"] == 0 and g["image_mean_sum"] == 0.0     # totals only


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


def check_map(emap, wants):
    for b, w in enumerate(wants):
        assert same_bits(emap[b], w["epe_map"]), b


def P():
    from raft_optical_flow_amd import _lib as L
    return L.FM_BLOCK_PIXELS


def G():
    from raft_optical_flow_amd import _lib as L
    return L.FM_MAX_BLOCKS


# ----------------------------------------------------------------------------- shapes


SHAPES = [(1, 1, 1),        # one pixel
          (1, 3, 5),        # the scalar tail, rows shorter than two groups
          (2, 7, 9),        # odd width: groups wrap rows; two samples
          (1, 8, 12),       # fully aligned: every group takes the 16-byte loads
          (3, 16, 20)]


@pytest.mark.parametrize("shape", SHAPES)
def test_small_shapes(shape):
    flow, gt, valid = R.metrics_case(*shape)
    for v in (None, valid):
        want = FM.metrics(flow, gt, v)
        recs, emap, _ = launch(dev(flow), dev(gt), None if v is None else dev(v))
        check_sample_records(recs, want, f"{shape}")
        check_map(emap, want)
    assert all(w["n"] == shape[1] * shape[2] for w in FM.metrics(flow, gt))


def test_block_sizes_and_grid_wrap():
    """Exactly P pixels (one full work-group), P + 1 (a second work-group with one pixel), and more than G * P
    (the grid's cap: the grid-stride loop wraps), P and G being the kernel's constants."""
    from raft_optical_flow_amd import _lib as L
    p, g = P(), G()
    assert (p, g) == (1024, 256)
    rec = L.FM_SLOTS * 8
    for shape in ((1, 32, 32), (1, 25, 41), (1, 513, 512)):
        B, H, W = shape
        n = H * W
        flow, gt, valid = R.metrics_case(*shape)
        want = FM.metrics(flow, gt, valid)
        recs, emap, _ = launch(dev(flow), dev(gt), dev(valid))
        check_sample_records(recs, want, f"{shape}")
        check_map(emap, want)
        assert L.load().raft_flow_metrics_ws_bytes(B, H, W) == min(-(-n // p), g) * rec
    assert 32 * 32 == p and 25 * 41 == p + 1 and 513 * 512 > g * p


@pytest.mark.parametrize("shape, partials", [((2, 513, 512), 256),   # the finalize stages one sample per pass
                                             ((17, 3, 5), 1)])        # 16 samples per pass, then one alone
def test_finalize_passes_with_totals(shape, partials):
    """The finalize kernel's passes over the samples, with running totals: the records against the oracle, each
    sample's record equal to that of the sample scored alone, and the totals equal to the records added in sample
    order (the counts as integers, the sums in fp64, bit for bit)."""
    from raft_optical_flow_amd import _lib as L
    B, H, W = shape
    assert L.load().raft_flow_metrics_ws_bytes(1, H, W) == partials * L.FM_SLOTS * 8 and partials <= G()
    flow, gt, valid = R.metrics_case(*shape)
    want = FM.metrics(flow, gt, valid)
    args = (dev(flow), dev(gt), dev(valid))
    totals = torch.zeros(L.FM_SLOTS, dtype=torch.int64, device=DEV)
    recs, emap, raw = launch(*args, totals=totals)
    check_sample_records(recs, want, f"{shape}")
    check_map(emap, want)
    for b in range(B):
        assert np.array_equal(launch(*(a[b:b + 1] for a in args), epe_map=False)[2][0], raw[b]), b
    tot = totals.cpu().numpy()
    nc, ns = len(FM.COUNTS), len(FM.SUMS)
    assert np.array_equal(tot[:nc], raw[:, :nc].sum(axis=0))                      # the counts: the records' sum
    acc = np.zeros(ns)
    for r in raw:                                                                 # the sums: added in sample order
        acc = acc + r[nc:nc + ns].view(np.float64)
    assert np.array_equal(tot[nc:nc + ns].view(np.float64), acc)
    assert all(w["n"] > 0 for w in want) and unpack(tot)["images"] == B and unpack(tot)["reserved"] == 0


def test_unpadded_view_with_odd_offset():
    """InputPadder.unpad's view of a padded flow, rows at an odd left offset, over a contiguous ground truth: the
    operands' alignments differ, nothing is copied, nothing outside the crop is read (the pad is NaN)."""
    flow, gt, valid = R.metrics_case(2, 13, 19)
    padded = torch.full((2, 2, 16, 24), float("nan"), device=DEV)
    view = padded[..., 2:15, 3:22]
    view.copy_(dev(flow))
    assert not view.is_contiguous() and view.data_ptr() % 16 != 0
    want = FM.metrics(flow, gt, valid)
    recs, emap, _ = launch(view, dev(gt), dev(valid))
    check_sample_records(recs, want)
    check_map(emap, want)
    assert all(w["n_nonfinite"] == 0 for w in want)
    # the same through the public call, with a strided float mask and a strided ground truth as well
    from raft_optical_flow_amd.utils import flow_errors
    gpad = torch.zeros(2, 2, 13, 32, device=DEV)
    gview = gpad[..., 4:23]
    gview.copy_(dev(gt))
    vpad = torch.zeros(2, 13, 21, device=DEV)
    vview = vpad[..., 1:20]
    vview.copy_(dev(valid))
    e = flow_errors(view, gview, vview, epe_map=True)
    torch.cuda.synchronize()
    for b, w in enumerate(want):
        check_record(unpack_errors(e, b), w)
    check_map(e.epe_map[:, 0].cpu().numpy(), want)


def unpack_errors(e, b):
    d = {k: int(getattr(e, k)[b]) for k in FM.COUNTS}
    d.update({k: float(getattr(e, k)[b]) for k in FM.SUMS})
    d["reserved"] = 0
    return d


# ----------------------------------------------------------------------------- the definition's rules


def test_threshold_pixels():
    """The hand-made pixels of the host test: the counts derived there by hand."""
    flow, gt, mask, want = FM.threshold_pixels()
    (orc,) = FM.metrics(flow, gt, mask, gt_limit=1000.0)
    recs, emap, _ = launch(dev(flow), dev(gt), dev(mask), gt_limit=1000.0)
    assert {k: recs[0][k] for k in FM.COUNTS} == want
    check_record(recs[0], orc)
    check_map(emap, [orc])
    # a lone pixel per launch takes the scalar path; the row of N pixels above the vector path where aligned
    N = flow.shape[3]
    cnt = {k: 0 for k in FM.COUNTS}
    f1, g1 = (np.ascontiguousarray(a[0, :, 0, :].T).reshape(N, 2, 1, 1) for a in (flow, gt))
    recs, _, _ = launch(dev(f1), dev(g1), dev(mask.reshape(N, 1, 1)), gt_limit=1000.0, epe_map=False)   # N of 1 x 1
    for r in recs:
        for k in FM.COUNTS:
            cnt[k] += r[k]
    assert cnt == want


def test_mask_dtypes_and_shapes():
    flow, gt, valid = R.metrics_case(2, 7, 9)
    want = FM.metrics(flow, gt, valid)
    as_bool = valid >= 0.5
    first = None
    for v in (dev(valid), dev(as_bool), dev(as_bool.astype(np.uint8) * 7), dev(valid).reshape(2, 1, 7, 9),
              dev(as_bool).reshape(2, 1, 7, 9), dev(as_bool.astype(np.uint8)).reshape(2, 1, 7, 9)):
        recs, emap, raw = launch(dev(flow), dev(gt), v)
        check_sample_records(recs, want, f"{v.dtype} {tuple(v.shape)}")
        check_map(emap, want)
        first = raw if first is None else first
        assert np.array_equal(raw, first)                          # the same pixels: the same bits
    # a byte mask at an odd address, rows of an aligned width (12): byte loads, the same result
    flow, gt, valid = R.metrics_case(1, 8, 12)
    want = FM.metrics(flow, gt, valid)
    buf = torch.zeros(8 * 12 + 1, dtype=torch.uint8, device=DEV)
    odd = buf[1:].view(1, 8, 12)
    odd.copy_(dev(valid >= 0.5))
    recs, emap, raw = launch(dev(flow), dev(gt), odd)
    check_sample_records(recs, want)
    assert np.array_equal(raw, launch(dev(flow), dev(gt), dev(valid))[2])


def test_gt_limit():
    flow, gt, valid = R.metrics_case(2, 16, 20)
    gt = gt.copy()
    gt[0, 0, 3, 4:9] = [1000.0, -1000.0, np.nextafter(np.float32(1000), np.float32(0)), 2000.0, np.nan]
    gt[1, 1, 0, 0:3] = [np.inf, -np.inf, np.float32(-999.99994)]
    for lim in (1000.0, 30.0):
        want = FM.metrics(flow, gt, valid, gt_limit=lim)
        recs, emap, _ = launch(dev(flow), dev(gt), dev(valid), gt_limit=lim)
        check_sample_records(recs, want, f"limit {lim}")
        check_map(emap, want)
        assert all(w["n_nonfinite"] == 0 for w in want)
    assert FM.metrics(flow, gt, None, gt_limit=1000.0)[0]["n"] == 16 * 20 - 4
    assert FM.metrics(flow, gt, None, gt_limit=30.0)[0]["n"] < 16 * 20 - 4


def test_nonfinite_rule():
    """A valid pixel whose epe is not finite counts in n and n_nonfinite only; an invalid one counts nowhere."""
    flow, gt, valid = R.metrics_case(1, 16, 20)
    flow, gt, valid = flow.copy(), gt.copy(), valid.copy()
    valid[0, 0, :8] = 1.0
    valid[0, 1, :4] = [0.0, 0.25, 1.0, 1.0]
    flow[0, 0, 0, 0:4] = [np.nan, np.inf, -np.inf, 3e38]       # (3e38)^2 overflows: epe = inf
    gt[0, 1, 0, 4:6] = [np.nan, np.inf]
    flow[0, 1, 1, 0:2] = [np.nan, np.inf]                       # masked out: counted nowhere
    flow[0, 0, 1, 2], gt[0, 0, 1, 2] = np.inf, np.inf           # inf - inf = NaN
    want = FM.metrics(flow, gt, valid)
    assert want[0]["n_nonfinite"] == 7
    recs, emap, _ = launch(dev(flow), dev(gt), dev(valid))
    check_sample_records(recs, want)
    check_map(emap, want)
    assert math.isfinite(recs[0]["epe_sum"]) and recs[0]["n_lt5"] > 0
    # FlowMetrics: the means are NaN, the shares stay counts over n
    from raft_optical_flow_amd.utils import FlowMetrics
    r = FlowMetrics().update(dev(flow), dev(gt), dev(valid)).result()
    assert r["nonfinite"] == 7 and r["pixels"] == want[0]["n"]
    assert all(math.isnan(r[k]) for k in ("epe", "f1", "epe_image_mean", "s0-10", "s10-40", "s40+"))
    assert r["1px"] == want[0]["n_lt1"] / want[0]["n"] and r["5px"] == want[0]["n_lt5"] / want[0]["n"]


# ----------------------------------------------------------------------------- reproducibility


def test_sample_alone_equals_sample_in_batch_and_runs_repeat():
    flow, gt, valid = R.metrics_case(3, 37, 53)
    args = (dev(flow), dev(gt), dev(valid))
    _, emap, raw = launch(*args)
    _, emap2, raw2 = launch(*args)
    assert np.array_equal(raw, raw2) and same_bits(emap, emap2)                   # two runs
    for b in range(3):
        _, e1, r1 = launch(*(a[b:b + 1] for a in args))
        assert np.array_equal(r1[0], raw[b]) and same_bits(e1[0], emap[b]), b      # alone / in the batch
    order = [2, 0, 1]
    _, _, rp = launch(*(a[order].contiguous() for a in args))
    assert np.array_equal(rp, raw[order])                                         # at another batch index
    # above the grid's cap as well
    flow, gt, valid = R.metrics_case(1, 513, 512)
    args = (dev(flow), dev(gt), dev(valid))
    assert np.array_equal(launch(*args, epe_map=False)[2], launch(*args, epe_map=False)[2])


def test_flow_errors_returns_device_tensors():
    from raft_optical_flow_amd.utils import FlowErrors, flow_errors
    flow, gt, valid = R.metrics_case(2, 7, 9)
    want = FM.metrics(flow, gt, valid, gt_limit=45.0)
    e = flow_errors(dev(flow), dev(gt), dev(valid >= 0.5).reshape(2, 1, 7, 9), gt_limit=45.0, epe_map=True)
    assert isinstance(e, FlowErrors)
    for k in FM.COUNTS:
        t = getattr(e, k)
        assert t.is_cuda and t.dtype == torch.int64 and tuple(t.shape) == (2,), k
    for k in FM.SUMS:
        t = getattr(e, k)
        assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (2,), k
    assert e.epe_map.dtype == torch.float32 and tuple(e.epe_map.shape) == (2, 1, 7, 9)
    for b, w in enumerate(want):
        check_record(unpack_errors(e, b), w)
    check_map(e.epe_map[:, 0].cpu().numpy(), want)
    assert flow_errors(dev(flow), dev(gt)).epe_map is None
    _, _, raw = launch(dev(flow), dev(gt), dev(valid), gt_limit=45.0)
    assert [int(x) for x in e.n_outlier] == [int(r[5]) for r in raw]
    assert np.array_equal(e.epe_sum.cpu().numpy().view(np.int64), raw[:, 9])      # the entry's bits


# ----------------------------------------------------------------------------- FlowMetrics


def test_flow_metrics_accumulates_over_batches():
    """Three batches of different shapes, one sample without a valid pixel: the totals equal the oracle on the
    union, epe_image_mean is the mean of the per-image means, images skips the empty sample, reset() clears."""
    from raft_optical_flow_amd.utils import FlowMetrics
    cases = [R.metrics_case(2, 7, 9), R.metrics_case(1, 25, 41), R.metrics_case(3, 16, 20)]
    empty = np.zeros((3, 16, 20), dtype=np.float32)
    empty[0], empty[2] = cases[2][2][0], cases[2][2][2]
    cases[2] = (cases[2][0], cases[2][1], empty)
    m = FlowMetrics()
    recs = []
    for k, (flow, gt, valid) in enumerate(cases):
        v = dev(valid) if k != 1 else dev(valid >= 0.5)
        assert m.update(dev(flow), dev(gt), v) is m
        recs += FM.metrics(flow, gt, valid)
    assert recs[4]["n"] == 0
    t = FM.totals(recs)
    want = FM.result(t)
    got = m.result()
    tot = unpack(m._totals.cpu().numpy())
    check_record(tot, t, "totals")
    assert tot["images"] == t["images"] == 5 and got["images"] == 5
    means = [r["epe_sum"] / r["n"] for r in recs if r["n"] > 0]
    # each image's sum within n 2^-53 sum|epe|, its quotient and the running sum one rounding each
    bound = sum((r["n"] + 2) * U53 * r["abs_sum"] / r["n"] for r in recs if r["n"] > 0) + 5 * U53 * sum(means)
    assert abs(tot["image_mean_sum"] - math.fsum(means)) <= bound
    assert abs(got["epe_image_mean"] - math.fsum(means) / 5) <= bound / 5 + U53 * max(means)
    for k in ("pixels", "nonfinite", "1px", "3px", "5px", "f1"):
        assert got[k] == want[k], k
    n = t["n"]
    assert abs(got["epe"] - want["epe"]) <= n * U53 * t["abs_sum"] / n + U53 * want["epe"]
    for k, c in (("s0-10", "s0_10"), ("s10-40", "s10_40"), ("s40+", "s40")):
        assert abs(got[k] - want[k]) <= (t["n_" + c] + 1) * U53 * t["abs_sum_" + c] / t["n_" + c], k
    m.reset()
    r = m.result()
    assert r["pixels"] == r["images"] == 0 and math.isnan(r["epe"])
    flow, gt, valid = cases[0]
    again = m.update(dev(flow), dev(gt), dev(valid)).result()
    alone = FlowMetrics().update(dev(flow), dev(gt), dev(valid)).result()
    assert again == alone and again["images"] == 2


# ----------------------------------------------------------------------------- end to end


@functools.lru_cache(maxsize=None)
def small_model():
    from raft_optical_flow_amd import RAFT
    wts = load_golden("raft_small_weights.npz")
    m = RAFT(argparse.Namespace(small=True, mixed_precision=False, alternate_corr=False))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in wts.items()})
    return m.to(DEV).eval()


def test_end_to_end_small_model_against_the_reference_sequence():
    """raft-small at 64x96, 2 iterations, on a 61x93 pair through InputPadder: FlowMetrics on the unpadded view
    against evaluate.py's own lines on the host copy (torch on the CPU, numpy lists, means at the end)."""
    from raft_optical_flow_amd import InputPadder
    from raft_optical_flow_amd.init import smooth_images
    from raft_optical_flow_amd.utils import FlowMetrics
    H, W = 61, 93
    i1, i2 = smooth_images(1, H, W, seed=11)
    rng = np.random.default_rng(3)
    m = small_model()
    padder = InputPadder(i1.shape)
    p1, p2 = padder.pad(i1.to(DEV), i2.to(DEV))
    assert tuple(p1.shape[-2:]) == (64, 96)
    with torch.no_grad():
        _, flow_pr = m(p1, p2, iters=2, test_mode=True)
    view = padder.unpad(flow_pr)
    assert tuple(view.shape) == (1, 2, H, W) and not view.is_contiguous()
    flow_host = padder.unpad(flow_pr[0]).cpu()                              # evaluate.py:113 / :146
    # ground truth around the prediction, so that the errors straddle 1, 3 and 5 px and the 5 % ratio
    gt_np = (flow_host.numpy() + rng.standard_normal((2, H, W)) * rng.choice([0.4, 2.5, 5.0], size=(1, H, W))).astype(
        np.float32)
    valid_np = rng.choice(np.array([0.0, 1.0], dtype=np.float32), size=(H, W), p=[0.2, 0.8])
    flow_gt, valid_gt = torch.from_numpy(gt_np), torch.from_numpy(valid_np)
    near = R.near_threshold(flow_host.numpy()[None], gt_np[None])[0]
    keep = torch.from_numpy(~near)

    epe = torch.sum((flow_host - flow_gt) ** 2, dim=0).sqrt()               # :148
    mag = torch.sum(flow_gt ** 2, dim=0).sqrt()                             # :149
    epe, mag = epe.view(-1), mag.view(-1)
    val = (valid_gt.view(-1) >= 0.5) & keep.view(-1)                        # :153, less the pixels left out
    out = ((epe > 3.0) & ((epe / mag) > 0.05)).float()                      # :155
    epe_all = epe[val].numpy()
    ref = {"n": int(val.sum()), "1px": float(np.mean(epe_all < 1)), "3px": float(np.mean(epe_all < 3)),
           "5px": float(np.mean(epe_all < 5)), "f1": 100 * float(np.mean(out[val].numpy(), dtype=np.float64)),
           "epe": float(np.mean(epe_all, dtype=np.float64))}

    got = FlowMetrics().update(view, flow_gt[None].to(DEV), (valid_gt.bool() & keep)[None].to(DEV)).result()
    n = ref["n"]
    assert got["pixels"] == n and got["nonfinite"] == 0 and got["images"] == 1 and n > 0.7 * H * W * 0.8
    for k in ("1px", "3px", "5px"):
        assert round(got[k] * n) == round(ref[k] * n) and abs(got[k] - ref[k]) < 1e-6, k
    assert round(got["f1"] * n / 100) == round(ref["f1"] * n / 100)
    assert 0.05 < got["1px"] < got["3px"] < got["5px"] < 0.95 and 1 < got["f1"] < 99
    # the fp64 bound on the sum, plus one fp32 ulp per pixel for torch's square root, over n
    bound = n * U53 * ref["epe"] + float(np.spacing(np.float32(epe_all.max())))
    assert abs(got["epe"] - ref["epe"]) <= bound, (got["epe"], ref["epe"], bound)
    assert got["epe_image_mean"] == got["epe"]
