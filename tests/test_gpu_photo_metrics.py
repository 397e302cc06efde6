"""raft_photo_metrics, utils.photo_errors and utils.PhotoMetrics on the GPU, against tests/photo_metrics_oracle.py.

Counts equal the oracle's exactly.  census_map and the sums lie within the bounds the oracle derives from the
inputs (its docstring has the chain); the one constant that is measured, the device powf's error, is measured
here (test_powf_error_measured), doubled, and refused above 16 ulps.  The structure of the computation is held
to the bits, without a tolerance: scoring (frame 1, frame 2, flow) equals scoring (frame 1, warp_frame(frame 2,
flow), zero flow).  Every output and workspace buffer the kernel tests hand to the C entry is prefilled with 0xFF
bytes (NaN as float32 and as float64, -1 as int64); running totals are the exception: the call adds into them.
The shapes come from the tile and cap constants of raft_optical_flow_amd._lib."""
import functools
import math

import numpy as np
import pytest
import torch

import photo_metrics_oracle as O
import test_photo_metrics_host as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


def L():
    from raft_optical_flow_amd import _lib
    return _lib


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)      # (a copy: the shared cases are read-only)


def nan_bytes(shape, dtype):
    """A device buffer of 0xFF bytes."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(0xFF)
    return t


def entry_args(f1, f2, flow, mask, patch, outgoing, record, totals, cmap, ws):
    """raft_photo_metrics' argument list for device tensors of any strides (unit element stride)."""
    lib = L()
    B, _, H, W = flow.shape
    assert flow.stride(3) == 1
    if f1.dtype == torch.uint8:
        assert f1.is_contiguous() and f2.is_contiguous()
        tag, s1, s2 = lib.FRAME_U8_NHWC, (0, 0, 0), (0, 0, 0)
    else:
        assert f1.stride(3) == 1 and f2.stride(3) == 1
        tag, s1, s2 = lib.FRAME_F32_NCHW, f1.stride()[:3], f2.stride()[:3]
    mp, mtag, msb, mpitch = None, 0, 0, 0
    if mask is not None:
        m = mask.reshape(B, H, W) if mask.dim() == 4 else mask
        mtag = lib.MASK_F32 if m.dtype == torch.float32 else lib.MASK_U8
        mp, msb, mpitch = m.data_ptr(), m.stride(0), m.stride(1)
    return (f1.data_ptr(), *s1, f2.data_ptr(), *s2, tag, flow.data_ptr(), *flow.stride()[:3], mp, mtag, msb, mpitch,
            B, H, W, patch, lib.PM_OUTGOING if outgoing else 0, record.data_ptr(),
            None if totals is None else totals.data_ptr(), None if cmap is None else cmap.data_ptr(), ws.data_ptr())


def launch(f1, f2, flow, mask=None, patch=7, outgoing=True, census_map=True, totals=None):
    """raft_photo_metrics with every output prefilled with NaN bytes: (records as a list of dicts, census_map
    numpy [B,H,W] or None, the raw records int64 numpy [B,16])."""
    lib = L()
    B, _, H, W = flow.shape
    record = nan_bytes((B, lib.PM_SLOTS), torch.int64)
    ws = nan_bytes((lib.load().raft_photo_metrics_ws_bytes(B, H, W, patch) // 8,), torch.int64)
    cmap = nan_bytes((B, 1, H, W), torch.float32) if census_map else None
    lib.call("raft_photo_metrics", *entry_args(f1, f2, flow, mask, patch, outgoing, record, totals, cmap, ws),
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw = record.cpu().numpy()
    return [unpack(r) for r in raw], (cmap[:, 0].cpu().numpy() if census_map else None), raw


def unpack(row):
    """One record (int64 [16]) as a dict: the counts, the sums, images, image_census_mean_sum, reserved."""
    row = np.ascontiguousarray(row, dtype=np.int64)
    f = row.view(np.float64)
    d = {k: int(row[i]) for i, k in enumerate(O.COUNTS)}
    d.update({k: float(f[len(O.COUNTS) + i]) for i, k in enumerate(O.SUMS)})
    d.update(images=int(row[10]), image_census_mean_sum=float(f[11]), reserved=[int(v) for v in row[12:]])
    return d


def check_record(got, want, what=""):
    """Counts exactly; every sum within the oracle's bound."""
    for k in O.COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in O.SUMS:
        assert abs(got[k] - want[k]) <= want["bound_" + k], (what, k, got[k], want[k], want["bound_" + k])
    assert got["reserved"] == [0, 0, 0, 0], what


def check_sample_records(recs, wants, what=""):
    for b, (g, w) in enumerate(zip(recs, wants)):
        check_record(g, w, f"{what} sample {b}")
        assert g["images"] == 0 and g["image_census_mean_sum"] == 0.0     # totals only


def check_map(cmap, wants, what=""):
    for b, w in enumerate(wants):
        h, hb = w["census_map"], w["census_map_bound"]
        fin = np.isfinite(h)
        assert np.array_equal(np.isfinite(cmap[b]), fin), (what, b)
        assert np.all(np.abs(cmap[b][fin] - h[fin]) <= hb[fin]), (what, b, np.abs(cmap[b][fin] - h[fin]).max())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


def frames(f1, f2, u8):
    return (dev(O.uint8_frame(f1)), dev(O.uint8_frame(f2))) if u8 else (dev(f1), dev(f2))


def oracle(f1, f2, flow, mask=None, patch=7, outgoing=True):
    return O.metrics(f1, f2, flow, mask, patch=patch, outgoing=outgoing, pow_ulps=pow_ulps())


def compare(shape, patch, u8=False, with_mask=True, outgoing=True):
    f1, f2, flow, mask = O.photo_case(*shape)
    m = mask if with_mask else None
    want = oracle(f1, f2, flow, m, patch, outgoing)
    recs, cmap, raw = launch(*frames(f1, f2, u8), dev(flow), None if m is None else dev(m), patch, outgoing)
    check_sample_records(recs, want, f"{shape} P={patch} u8={u8}")
    check_map(cmap, want, f"{shape} P={patch} u8={u8}")
    return want, raw, cmap


# ----------------------------------------------------------------------------- the measured constant


@functools.lru_cache(maxsize=None)
def measured_powf_ulps():
    """The device powf's largest error, in units in the last place of the fp32 result, over the arguments the
    kernel forms: B samples of 7 x 7 pixels at patch 7 have one interior pixel each, and the mask selects it
    alone, so that every sum of a record is one term (photo_sum: three, two of them the constant powf(1e-6f,
    0.45f), which sample 0, identical frames, gives on its own).  The flow is zero: W2 is frame 2 exactly, the
    residual of channel 0 is fl(I1 - I2), and h is read from census_map, so each powf argument is known to the
    bit and its result is compared with fp64 pow.  Residuals span 1e-4 .. 255 (and 0), h spans 0 .. 46."""
    B, S = 2048, 7
    rng = np.random.default_rng(11)
    f1 = rng.integers(0, 256, size=(B, 3, S, S)).astype(np.float32)
    amp = 10.0 ** rng.uniform(-3, 2.3, size=(B, 1, 1, 1))            # small to large census differences
    f2 = (f1 + amp * rng.standard_normal((B, 3, S, S))).astype(np.float32)
    f1[1:33], f2[1:33] = 255.0, f2[1:33] - f1[1:33]                   # opposite census signs: h near its maximum
    f1[1:33, 1:, 3, 3] = 128.0
    f2[:, 1:, 3, 3] = f1[:, 1:, 3, 3]                                 # e_1 = e_2 = 0 at the scored pixel
    res = (10.0 ** rng.uniform(-4, np.log10(255.0), size=B)).astype(np.float32)
    f2[:, 0, 3, 3] = np.float32(300.0)
    f1[:, 0, 3, 3] = f2[:, 0, 3, 3] - res * rng.choice([-1, 1], size=B).astype(np.float32)
    f1[0], f2[0] = 7.0, 7.0                                           # sample 0: identical frames
    mask = np.zeros((B, S, S), dtype=np.uint8)
    mask[:, 3, 3] = 1
    flow = np.zeros((B, 2, S, S), dtype=np.float32)
    recs, cmap, _ = launch(dev(f1), dev(f2), dev(flow), dev(mask), patch=7)
    assert all(r["n_mask"] == 1 and r["n_census"] == 1 and r["n_nonfinite"] == 0 for r in recs)
    f32 = np.float32
    k = recs[0]["ternary_sum"]                                        # powf(1e-6f, 0.45f)
    assert recs[0]["photo_sum"] == 3 * k and cmap[0, 3, 3] == 0.0
    e = (f1[:, 0, 3, 3] - f2[:, 0, 3, 3]).astype(f32)
    h = cmap[:, 3, 3].astype(f32)
    args = {"photo": ((e * e).astype(f32) + f32(1e-6)).astype(f32), "census": (h + f32(0.01)).astype(f32),
            "ternary": ((h * h).astype(f32) + f32(1e-6)).astype(f32)}
    got = {"photo": np.array([r["photo_sum"] for r in recs]) - 2 * k,
           "census": np.array([r["census_sum"] for r in recs]), "ternary": np.array([r["ternary_sum"] for r in recs])}
    expo = {"photo": O.E045, "census": O.E04, "ternary": O.E045}
    worst = 0.0
    for name in ("photo", "census", "ternary"):
        truth = args[name].astype(np.float64) ** expo[name]
        assert np.array_equal(got[name], got[name].astype(f32).astype(np.float64)), name   # fp32 values, one term
        ulps = np.abs(got[name] - truth) / np.spacing(truth.astype(f32)).astype(np.float64)
        print(f"device powf, {name} terms: arguments {args[name].min():.3g} .. {args[name].max():.3g}, "
              f"max error {ulps.max():.3f} ulp")
        worst = max(worst, float(ulps.max()))
    assert h.max() > 45 and h[1:].min() < 0.05 and np.abs(e).max() > 200
    return worst


def pow_ulps():
    """Twice the measured figure (the arguments outside the tests are not sampled); above the cap the oracle
    refuses it."""
    return 2.0 * measured_powf_ulps()


def test_powf_error_measured():
    worst = measured_powf_ulps()
    print(f"device powf: max error {worst:.3f} ulp over the kernel's three terms; the bounds use {2 * worst:.3f}")
    assert 2.0 * worst <= O.POW_ULPS_CAP, worst


# ----------------------------------------------------------------------------- structure, to the bits


@pytest.mark.parametrize("patch", [3, 5, 7])
def test_structure_equals_scoring_the_warped_frame(patch):
    """Scoring (f1, f2, flow) with a float mask v equals scoring (f1, warp_frame(f2, flow), zero flow) with the mask
    v & valid and outgoing off: in every slot but n_valid, and in the census map, bit for bit.  n_valid equals
    warp_frame's valid count."""
    from raft_optical_flow_amd.utils import photo_errors, warp_frame
    th, tw = L().PM_TILE_H, L().PM_TILE_W
    f1, f2, flow, mask = (dev(a) for a in O.photo_case(2, th + 3, tw + 5))
    a = photo_errors(f1, f2, flow, mask=mask, patch=patch, census_map=True)
    warped, valid = warp_frame(f2, flow)
    both = ((mask >= 0.5) & valid[:, 0]).float()
    b = photo_errors(f1, warped, torch.zeros_like(flow), mask=both, patch=patch, outgoing=False, census_map=True)
    for k in a._fields:
        if k == "n_valid":
            assert torch.equal(a.n_valid, valid.sum(dim=(1, 2, 3)))
            assert torch.equal(b.n_valid, torch.full_like(b.n_valid, (th + 3) * (tw + 5)))
        elif k == "census_map":
            assert same_bits(a.census_map.cpu().numpy(), b.census_map.cpu().numpy())
        else:
            ta, tb = getattr(a, k), getattr(b, k)
            assert torch.equal(ta.view(torch.int64), tb.view(torch.int64)), k
    assert 0 < int(a.n_valid[0]) < (th + 3) * (tw + 5) and int(a.n_census[0]) > 0 and int(a.n_nonfinite.sum()) == 0


# ----------------------------------------------------------------------------- against the oracle: shapes


def shapes():
    th, tw, cap = L().PM_TILE_H, L().PM_TILE_W, L().PM_MAX_BLOCKS
    return {"one pixel": (1, 1, 1), "no interior at patch 7": (1, 5, 9), "one tile": (1, th, tw),
            "a tile, a row and a column more": (1, th + 1, tw + 1), "odd width": (2, 19, 23),
            "the golden's": (2, 37, 53), "more tiles than the cap": (1, th * cap + 1, 3)}


@pytest.mark.parametrize("name", ["one pixel", "no interior at patch 7", "one tile", "a tile, a row and a column more",
                                  "odd width", "the golden's", "more tiles than the cap"])
def test_shapes_against_oracle(name):
    lib = L()
    shape = shapes()[name]
    B, H, W = shape
    want, raw, cmap = compare(shape, 7)
    compare(shape, 7, with_mask=False)
    tiles = -(-H // lib.PM_TILE_H) * -(-W // lib.PM_TILE_W)
    assert lib.load().raft_photo_metrics_ws_bytes(B, H, W, 7) == B * min(tiles, lib.PM_MAX_BLOCKS) * lib.PM_SLOTS * 8
    if name == "more tiles than the cap":
        assert tiles == lib.PM_MAX_BLOCKS + 1 and want[0]["n_census"] == 0
        assert compare(shape, 3)[0][0]["n_census"] > 0                # ... with interior pixels in every tile
        assert compare((1, 3, lib.PM_TILE_W * lib.PM_MAX_BLOCKS + 1), 3)[0][0]["n_census"] > 0   # ... and along x
    if name in ("one pixel", "no interior at patch 7"):
        assert all(w["n_census"] == 0 for w in want) and np.isfinite(cmap).all()
        assert all(r[8] == 0 and r[7] == 0 for r in raw)               # +0.0: nothing was added
    if name in ("odd width", "the golden's"):
        for w in want:
            assert w["n_nonfinite"] == 0 and w["n_census"] > 0 and 0.5 < w["n_valid"] / w["pixels"] < 0.95


def test_finalize_carries_sums_across_staging_runs_with_totals():
    """Two samples of 257 tiles each, more than the finalize kernel stages at a time (256): each sample is staged
    in two runs with its sums carried across.  The records against the oracle, each equal to that of the sample
    scored alone, and the totals equal to the records added in sample order, bit for bit."""
    lib = L()
    shape = (2, lib.PM_TILE_H * 256 + 1, 3)
    B, H, W = shape
    tiles = -(-H // lib.PM_TILE_H) * -(-W // lib.PM_TILE_W)
    assert tiles == 257 and lib.load().raft_photo_metrics_ws_bytes(1, H, W, 3) == tiles * lib.PM_SLOTS * 8
    f1, f2, flow, mask = O.photo_case(*shape)
    want = oracle(f1, f2, flow, mask, 3)
    args = (dev(f1), dev(f2), dev(flow), dev(mask))
    totals = torch.zeros(lib.PM_SLOTS, dtype=torch.int64, device=DEV)
    recs, cmap, raw = launch(*args, patch=3, totals=totals)
    check_sample_records(recs, want, f"{shape}")
    check_map(cmap, want, f"{shape}")
    assert all(w["n_census"] > 0 for w in want)
    for b in range(B):
        assert np.array_equal(launch(*(a[b:b + 1] for a in args), patch=3, census_map=False)[2][0], raw[b]), b
    tot = totals.cpu().numpy()
    nc, ns = len(O.COUNTS), len(O.SUMS)
    assert np.array_equal(tot[:nc], raw[:, :nc].sum(axis=0))                      # the counts: the records' sum
    acc = np.zeros(ns)
    for r in raw:                                                                 # the sums: added in sample order
        acc = acc + r[nc:nc + ns].view(np.float64)
    assert np.array_equal(tot[nc:nc + ns].view(np.float64), acc)
    assert unpack(tot)["images"] == B and unpack(tot)["reserved"] == [0, 0, 0, 0]


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("patch", [3, 5, 7])
def test_patches_and_frame_dtypes(patch, u8):
    th, tw = L().PM_TILE_H, L().PM_TILE_W
    for shape in ((2, 19, 23), (1, th + 1, tw + 1)):
        want, _, _ = compare(shape, patch, u8=u8)
        r = patch // 2
        assert want[0]["n_census"] <= (shape[1] - 2 * r) * (shape[2] - 2 * r)
    if u8:   # integer-valued frames: the uint8 and the float32 forms give the same bits
        f1, f2, flow, mask = O.photo_case(2, 19, 23)
        a = launch(*frames(f1, f2, True), dev(flow), dev(mask), patch)
        b = launch(*frames(f1, f2, False), dev(flow), dev(mask), patch)
        assert np.array_equal(a[2], b[2]) and same_bits(a[1], b[1])


def test_hand_made_pixels():
    """The host test's hand-made cases: h written down by hand, within the oracle's bound of the kernel's map."""
    for name, make in sorted(R.HAND_CASES.items()):
        (f1, f2, flow), h = make()
        (want,) = oracle(f1, f2, flow, patch=3)
        recs, cmap, _ = launch(dev(f1), dev(f2), dev(flow), patch=3)
        check_sample_records(recs, [want], name)
        assert np.all(np.abs(cmap[0] - h) <= want["census_map_bound"] + 1e-12), name
    (f1, f2, flow), _ = R.case_identical()
    recs, cmap, _ = launch(dev(f1), dev(f2), dev(flow), patch=3)
    n = recs[0]["n_census"]
    assert np.all(cmap == 0) and recs[0]["l1_sum"] == 0 and recs[0]["hamming_sum"] == 0
    assert abs(recs[0]["census_sum"] - n * R.K_CENSUS) <= n * (2 + 2 * pow_ulps()) * O.U * R.K_CENSUS
    assert abs(recs[0]["ternary_sum"] - n * R.K_PHOTO) <= n * (2 + 2 * pow_ulps()) * O.U * R.K_PHOTO


def test_owner_revealing_frame():
    """Frame 1's grey value encodes (y, x) with differences of the census transform's own scale; frame 2 is 0.
    A wrong neighbour offset or a wrong halo column changes h by O(1): with the first column of the second tile
    replaced by its neighbour, the oracle's own h moves by more than 0.05 on most rows of the column before it,
    while the bound is below 2e-3."""
    th, tw = L().PM_TILE_H, L().PM_TILE_W
    H, W = 2 * th + 3, 2 * tw + 5
    y, x = np.mgrid[:H, :W]
    g = (0.25 * ((7 * y + 3 * x) % 11) + 0.0625 * ((y * W + x) % 7)).astype(np.float32)
    f1, f2 = R.grey(g), R.grey(np.zeros((H, W)))
    flow = np.zeros((1, 2, H, W), dtype=np.float32)
    for patch in (3, 7):
        (want,) = oracle(f1, f2, flow, patch=patch)
        recs, cmap, _ = launch(dev(f1), dev(f2), dev(flow), patch=patch)
        check_sample_records(recs, [want], f"P={patch}")
        check_map(cmap, [want])
        assert want["census_map_bound"].max() < 2e-3
        bad = g.copy()
        bad[:, tw] = g[:, tw + 1]
        off = O.pixel_values(R.grey(bad), f2, flow, patch)["h"][0]
        assert np.median(np.abs(off - want["census_map"])[:, tw - 1]) > 0.05


# ----------------------------------------------------------------------------- views, masks, options


def test_strided_crops_at_an_odd_offset():
    """Frames, flow and mask as crops of larger NaN-filled tensors at an odd offset (InputPadder.unpad's view):
    nothing is copied by the entry, nothing outside the crop is read."""
    from raft_optical_flow_amd.utils import photo_errors
    f1, f2, flow, mask = O.photo_case(2, 19, 23)
    want = oracle(f1, f2, flow, mask, 5)

    def crop(a, c):
        big = torch.full((2, c, 19 + 5, 23 + 9), float("nan"), device=DEV)
        view = big[..., 2:21, 3:26]
        view.copy_(dev(a).reshape(2, c, 19, 23))
        assert not view.is_contiguous() and view.data_ptr() % 16 != 0
        return view

    v1, v2, vf, vm = crop(f1, 3), crop(f2, 3), crop(flow, 2), crop(mask, 1)
    recs, cmap, raw = launch(v1, v2, vf, vm[:, 0], patch=5)
    check_sample_records(recs, want)
    check_map(cmap, want)
    assert all(w["n_nonfinite"] == 0 for w in want)
    assert np.array_equal(raw, launch(dev(f1), dev(f2), dev(flow), dev(mask), patch=5)[2])   # the same bits
    e = photo_errors(v1, v2, vf, mask=vm, patch=5, census_map=True)
    assert np.array_equal(torch.stack([getattr(e, k).view(torch.int64) for k in O.COUNTS + O.SUMS], 1).cpu().numpy(),
                          raw[:, :10])
    assert same_bits(e.census_map[:, 0].cpu().numpy(), cmap)


def test_mask_dtypes_and_outgoing():
    f1, f2, flow, mask = O.photo_case(2, 19, 23)
    want = oracle(f1, f2, flow, mask, 7)
    as_bool = mask >= 0.5
    first = None
    for v in (dev(mask), dev(as_bool), dev(as_bool.astype(np.uint8) * 7), dev(mask).reshape(2, 1, 19, 23),
              dev(as_bool).reshape(2, 1, 19, 23)):
        recs, cmap, raw = launch(dev(f1), dev(f2), dev(flow), v)
        check_sample_records(recs, want, f"{v.dtype} {tuple(v.shape)}")
        first = raw if first is None else first
        assert np.array_equal(raw, first)                          # the same pixels: the same bits
    nanmask = np.array(mask)
    nanmask[:, 4, 5] = np.nan                                     # a NaN mask value fails
    recs, _, _ = launch(dev(f1), dev(f2), dev(flow), dev(nanmask))
    check_sample_records(recs, oracle(f1, f2, flow, nanmask, 7))
    for m in (None, mask):
        want0 = oracle(f1, f2, flow, m, 7, outgoing=False)
        recs, cmap, _ = launch(dev(f1), dev(f2), dev(flow), None if m is None else dev(m), outgoing=False)
        check_sample_records(recs, want0, "outgoing=False")
        check_map(cmap, want0)
    assert want0[0]["n_mask"] > want[0]["n_mask"] and want0[0]["n_valid"] == want[0]["n_valid"]


def test_flows_that_leave_the_frame_and_bad_flows():
    """Flows far out of the frame, and NaN / inf / 2^30 flows: those pixels are invalid (W2 = 0), nothing else is
    disturbed, and with outgoing set no pixel is non-finite."""
    f1, f2, flow, mask = O.photo_case(2, 19, 23)
    far = np.array(flow)
    far[0, 0, :, :6] += 500.0
    far[0, 1, 10:, :] -= 1e6
    far[1, 0, 3, 4], far[1, 1, 5, 6], far[1, 0, 7, 8], far[1, 1, 9, 10] = np.nan, np.inf, -np.inf, 2.0 ** 30
    far[1, 0, 11, 12] = -2.0 ** 30
    far[1, 0, 13, 14] = np.nextafter(np.float32(2.0 ** 30), np.float32(0))     # just below the limit: not rejected
    for outgoing in (True, False):
        want = oracle(f1, f2, far, mask, 7, outgoing)
        recs, cmap, _ = launch(dev(f1), dev(f2), dev(far), dev(mask), outgoing=outgoing)
        check_sample_records(recs, want, f"outgoing={outgoing}")
        check_map(cmap, want)
        assert all(w["n_nonfinite"] == 0 for w in want)
    # nothing else is disturbed: away from the bad pixels' patches the map keeps the bits of the clean run
    clean = np.array(far)
    clean[1] = flow[1]
    a = launch(dev(f1), dev(f2), dev(far), dev(mask))[1][1]
    b = launch(dev(f1), dev(f2), dev(clean), dev(mask))[1][1]
    near = np.zeros((19, 23), dtype=bool)
    for y, x in ((3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14)):
        near[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] = True
    assert same_bits(a[~near], b[~near]) and not same_bits(a[near], b[near])


def test_nan_frame_value_taints_its_patch_and_its_taps():
    """A NaN in frame 1 taints the P x P pixels whose patch holds it; a NaN in frame 2 the pixels whose taps read
    it and their patches.  Those pixels count in n_nonfinite and in no sum; the sums stay finite."""
    f1, f2, flow, mask = O.photo_case(1, 19, 23)
    z = np.zeros_like(flow)
    g1 = np.array(f1)
    g1[0, 1, 9, 11] = np.nan
    (want,) = oracle(g1, f2, z, None, 5)
    recs, cmap, _ = launch(dev(g1), dev(f2), dev(z), patch=5)
    check_sample_records(recs, [want])
    check_map(cmap, [want])
    assert recs[0]["n_nonfinite"] == 25 and np.isnan(cmap[0]).sum() == 25 and np.isnan(cmap[0, 7:12, 9:14]).all()
    assert all(math.isfinite(recs[0][k]) for k in O.SUMS)
    g2 = np.array(f2)
    g2[0, 0, 9, 11] = np.nan
    (want,) = oracle(f1, g2, flow, None, 3)
    recs, cmap, _ = launch(dev(f1), dev(g2), dev(flow), patch=3)
    check_sample_records(recs, [want])
    check_map(cmap, [want])
    assert want["n_nonfinite"] > 0 and all(math.isfinite(recs[0][k]) for k in O.SUMS)
    u1, u2 = frames(f1, f2, True)                                  # (uint8 frames hold no NaN: the same call is clean)
    assert launch(u1, u2, dev(flow), patch=3)[0][0]["n_nonfinite"] == 0


# ----------------------------------------------------------------------------- reproducibility


def test_samples_swapped_runs_repeat_and_graph_replay():
    lib = L()
    th, tw = lib.PM_TILE_H, lib.PM_TILE_W
    f1, f2, flow, mask = (dev(a) for a in O.photo_case(2, th + 5, 2 * tw + 3))
    _, cmap, raw = launch(f1, f2, flow, mask)
    _, cmap2, raw2 = launch(f1, f2, flow, mask)
    assert np.array_equal(raw, raw2) and same_bits(cmap, cmap2)                    # two runs
    swap = [1, 0]
    _, cmap_s, raw_s = launch(*(a[swap].contiguous() for a in (f1, f2, flow, mask)))
    assert np.array_equal(raw_s, raw[swap]) and same_bits(cmap_s, cmap[swap])       # at the other batch index
    for b in range(2):
        _, c1, r1 = launch(*(a[b:b + 1] for a in (f1, f2, flow, mask)))
        assert np.array_equal(r1[0], raw[b]) and same_bits(c1[0], cmap[b]), b       # alone / in the batch
    # captured in and replayed from a graph, into buffers refilled with NaN bytes in between
    B, _, H, W = flow.shape
    record, cm = nan_bytes((B, lib.PM_SLOTS), torch.int64), nan_bytes((B, 1, H, W), torch.float32)
    ws = nan_bytes((lib.load().raft_photo_metrics_ws_bytes(B, H, W, 7) // 8,), torch.int64)
    args = entry_args(f1, f2, flow, mask, 7, True, record, None, cm, ws)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lib.call("raft_photo_metrics", *args, torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        for t in (record, cm, ws):
            t.view(torch.uint8).fill_(0xFF)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(record.cpu().numpy(), raw) and same_bits(cm[:, 0].cpu().numpy(), cmap)
    # above the cap as well (the strided tile loop)
    big = tuple(dev(a) for a in O.photo_case(1, th * lib.PM_MAX_BLOCKS + 1, 3))
    assert np.array_equal(launch(*big, patch=3)[2], launch(*big, patch=3)[2])


# ----------------------------------------------------------------------------- the public calls


def test_photo_errors_returns_device_tensors():
    from raft_optical_flow_amd.utils import PhotoErrors, photo_errors
    f1, f2, flow, mask = O.photo_case(2, 19, 23)
    want = oracle(f1, f2, flow, mask, 3)
    e = photo_errors(dev(f1), dev(f2), dev(flow), mask=dev(mask >= 0.5).reshape(2, 1, 19, 23), patch=3,
                     census_map=True)
    assert isinstance(e, PhotoErrors)
    for k in O.COUNTS:
        t = getattr(e, k)
        assert t.is_cuda and t.dtype == torch.int64 and tuple(t.shape) == (2,), k
    for k in O.SUMS:
        t = getattr(e, k)
        assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (2,), k
    assert e.census_map.dtype == torch.float32 and tuple(e.census_map.shape) == (2, 1, 19, 23)
    for b, w in enumerate(want):
        got = {k: int(getattr(e, k)[b]) for k in O.COUNTS}
        got.update({k: float(getattr(e, k)[b]) for k in O.SUMS})
        got["reserved"] = [0, 0, 0, 0]
        check_record(got, w)
    check_map(e.census_map[:, 0].cpu().numpy(), want)
    assert photo_errors(dev(f1), dev(f2), dev(flow)).census_map is None
    u = photo_errors(*frames(f1, f2, True), dev(flow), mask=dev(mask), patch=3)
    assert torch.equal(u.census_sum.view(torch.int64), e.census_sum.view(torch.int64))


def test_photo_metrics_accumulates_over_batches():
    """Two updates of different shapes, one sample without an interior pixel: the totals equal the sum of the
    records, images included; result() equals the oracle's dict within the bounds; reset() clears."""
    from raft_optical_flow_amd.utils import PhotoMetrics
    cases = [O.photo_case(2, 19, 23), O.photo_case(1, 5, 9), O.photo_case(2, 37, 53)]
    m = PhotoMetrics(patch=7)
    recs, raws = [], []
    for k, (f1, f2, flow, mask) in enumerate(cases):
        fr = frames(f1, f2, k == 2)
        assert m.update(*fr, dev(flow), mask=dev(mask)) is m
        recs += oracle(f1, f2, flow, mask, 7)
        raws.append(launch(*fr, dev(flow), dev(mask))[2])
    assert recs[2]["n_census"] == 0
    t = O.totals(recs)
    tot_raw = m._totals.cpu().numpy()
    tot = unpack(tot_raw)
    raw = np.concatenate(raws)
    assert np.array_equal(tot_raw[:5], raw[:, :5].sum(axis=0))                   # the counts: the records' sum
    acc = np.zeros(5)
    for r in raw:                                                               # the sums: added in sample order
        acc = acc + r[5:10].view(np.float64)
    assert np.array_equal(tot_raw[5:10].view(np.float64), acc)
    check_record(tot, t, "totals")
    assert tot["images"] == t["images"] == 4
    assert abs(tot["image_census_mean_sum"] - t["image_census_mean_sum"]) <= t["bound_image_census_mean_sum"]
    want, got = O.result(t), m.result()
    for k in ("pixels", "images", "nonfinite", "valid_share"):
        assert got[k] == want[k], k
    rel = 4 * O.U53
    for k, s, n in (("census", "census_sum", t["n_census"] + 1e-6), ("ternary", "ternary_sum", t["pixels"]),
                    ("photo", "photo_sum", 3 * t["pixels"]), ("l1", "l1_sum", 3 * t["n_mask"]),
                    ("hamming", "hamming_sum", t["n_census"])):
        assert abs(got[k] - want[k]) <= t["bound_" + s] / n + rel * abs(want[k]), k
    assert abs(got["census_image_mean"] - want["census_image_mean"]) <= (
        t["bound_image_census_mean_sum"] / 4 + rel * want["census_image_mean"])
    m.reset()
    r = m.result()
    assert r["pixels"] == r["images"] == 0 and math.isnan(r["census"])
    f1, f2, flow, mask = cases[0]
    again = m.update(dev(f1), dev(f2), dev(flow), mask=dev(mask)).result()
    alone = PhotoMetrics().update(dev(f1), dev(f2), dev(flow), mask=dev(mask)).result()
    assert again == alone and again["images"] == 2
    # a NaN frame value: the means are NaN, the counts stay
    g1 = np.array(f1)
    g1[0, 0, 9, 11] = np.nan
    r = PhotoMetrics(patch=3).update(dev(g1), dev(f2), dev(np.zeros_like(flow))).result()
    assert r["nonfinite"] == 9 and math.isnan(r["census"]) and math.isnan(r["photo"]) and r["valid_share"] == 1.0
