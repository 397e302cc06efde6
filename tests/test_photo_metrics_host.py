"""The label-free scoring additions that need no GPU: tests/photo_metrics_oracle.py (the fp64 restatement of
raft_photo_metrics, include/raft_hip.h) pinned on hand-made pixels and against the reference's ternary_loss,
census_loss and photometric_loss (tests/golden/photo_reference.npz); PhotoMetrics.result()'s arithmetic from
hand-written totals; the argument checks of photo_errors / PhotoMetrics on CPU tensors; the new C entries'
argument errors; the sources.

tests/test_gpu_photo_metrics.py imports the hand-made cases."""
import math
import os

import numpy as np
import pytest
import torch

import photo_metrics_oracle as O
from raft_optical_flow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "photo_reference.npz")
K_CENSUS = O.C001 ** O.E04        # a census term at h = 0: 0.01f ^ 0.4f
K_PHOTO = O.C1EM6 ** O.E045       # a photometric or ternary term at 0: 1e-6f ^ 0.45f


def term(v):
    """One offset's term of h where one image's grey difference is v (or -v) and the other's is 0."""
    s2 = v * v / (O.C081 + v * v)
    return s2 / (O.C01 + s2)


def grey(a):
    """A grey float32 frame [1,3,H,W] from [H,W] values."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float32)[None, None], (1, 3) + np.shape(a)))


# ----------------------------------------------------------------------------- hand-made cases: (inputs, h by hand)


def case_identical(H=9, W=11):
    """Identical frames, zero flow: every residual and every census difference is 0."""
    f1, _, _, _ = O.photo_case(1, H, W)
    return (f1, f1, np.zeros((1, 2, H, W), dtype=np.float32)), np.zeros((H, W))


def case_constant_shift(H=6, W=9, c=40.0, patch=3):
    """A constant frame against itself under the flow (2, 0): W2 = c where x + 2 <= W - 1, else 0 (and not valid).
    g1 is constant, so inside the frame d1 = 0; g2 steps from c to 0 between columns W-3 and W-2.  Patch 3: a
    pixel in column W-3 sees the three zeros of column W-2 (d2 = -c); one in column W-2 is itself 0 and sees the
    three c of column W-3 (d2 = +c); beyond the frame both images read the padding: image 1 gives d1 = -c there,
    image 2 gives d2 = -c where g2 = c and 0 where g2 = 0.  By hand, per pixel: the number of offsets at which
    exactly one of (c1, c2) is 0 -- every such term is term(c); where both are -c or both 0 the term is 0."""
    assert patch == 3
    f = grey(np.full((H, W), c))
    flow = np.zeros((1, 2, H, W), dtype=np.float32)
    flow[:, 0] = 2.0
    g1 = np.full((H, W), c)
    g2 = np.where(np.arange(W)[None, :] <= W - 3, c, 0.0) * np.ones((H, 1))
    h = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            n = 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    inside = 0 <= yy < H and 0 <= xx < W
                    d1 = (g1[yy, xx] if inside else 0.0) - g1[y, x]
                    d2 = (g2[yy, xx] if inside else 0.0) - g2[y, x]
                    assert d1 in (0.0, -c) and d2 in (0.0, -c, c)
                    n += (d1 == 0.0) != (d2 == 0.0)
                    assert not (d1 != 0 and d2 == c)      # -c against +c never occurs: 2 c would need its own term
            h[y, x] = n * term(c)
    return (f, f, flow), h


def case_bright_pixel(H=7, W=8, y0=3, x0=4, v=2.0, patch=3):
    """Frame 1 is 0 but for one pixel of grey value v; frame 2 is 0; zero flow.  At the bright pixel the eight
    neighbours differ by -v: h = 8 term(v); each of the eight neighbours sees it at one offset: h = term(v)."""
    a = np.zeros((H, W))
    a[y0, x0] = v
    h = np.zeros((H, W))
    h[y0 - 1:y0 + 2, x0 - 1:x0 + 2] = term(v)
    h[y0, x0] = 8 * term(v)
    return (grey(a), grey(np.zeros((H, W))), np.zeros((1, 2, H, W), dtype=np.float32)), h


def case_corner_padding(H=5, W=6, c=1.5, patch=3):
    """A constant frame against a zero frame, zero flow: image 1 differs from its zero padding only.  Patch 3:
    a corner pixel has 5 offsets outside the frame, another border pixel 3, an interior pixel none."""
    h = np.zeros((H, W))
    h[0, :] = h[-1, :] = h[:, 0] = h[:, -1] = 3 * term(c)
    h[0, 0] = h[0, -1] = h[-1, 0] = h[-1, -1] = 5 * term(c)
    return (grey(np.full((H, W), c)), grey(np.zeros((H, W))), np.zeros((1, 2, H, W), dtype=np.float32)), h


HAND_CASES = {"identical": case_identical, "constant_shift": case_constant_shift, "bright_pixel": case_bright_pixel,
              "corner_padding": case_corner_padding}


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_oracle_on_hand_made_pixels(name):
    (f1, f2, flow), h = HAND_CASES[name]()
    v = O.pixel_values(f1, f2, flow, 3)
    assert np.abs(v["h"][0] - h).max() <= 1e-13 * max(1.0, h.max())
    assert v["finite"].all()


def test_identical_frames_sums():
    """h = 0 and e = 0 everywhere: census_sum = n 0.01^0.4, ternary_sum = n 1e-6^0.45, photo_sum = 3 n_mask
    1e-6^0.45, for every patch; the interior shrinks with the patch."""
    (f1, f2, flow), _ = case_identical(9, 11)
    for patch, n_int in ((3, 7 * 9), (5, 5 * 7), (7, 3 * 5)):
        (r,) = O.metrics(f1, f2, flow, patch=patch)
        assert (r["n_mask"], r["n_census"], r["n_valid"], r["n_nonfinite"], r["pixels"]) == (99, n_int, 99, 0, 99)
        assert r["l1_sum"] == 0.0 and r["hamming_sum"] == 0.0
        assert abs(r["census_sum"] - n_int * K_CENSUS) <= 1e-12 and abs(r["ternary_sum"] - n_int * K_PHOTO) <= 1e-12
        assert abs(r["photo_sum"] - 3 * 99 * K_PHOTO) <= 1e-12
    assert abs(K_CENSUS - 0.01 ** 0.4) < 1e-8 and abs(K_PHOTO - 1e-6 ** 0.45) < 1e-8


def test_constant_shift_counts_and_sums():
    """The flow (2, 0) pushes the last two columns out: they are not valid and, with outgoing, not counted.
    Interior and counted: 1 <= x <= W-3 on rows 1 .. H-2; of those only column W-3 has h != 0 (3 term(c))."""
    (f1, f2, flow), h = case_constant_shift()
    H, W = h.shape
    (r,) = O.metrics(f1, f2, flow, patch=3)
    assert r["n_valid"] == H * (W - 2) and r["n_mask"] == H * (W - 2) and r["n_census"] == (H - 2) * (W - 3)
    assert r["l1_sum"] == 0.0                                        # where counted, W2 == frame 1
    t = term(40.0)
    assert abs(r["hamming_sum"] - (H - 2) * 3 * t) <= 1e-12
    want = (H - 2) * ((W - 4) * K_CENSUS + (3 * t + O.C001) ** O.E04)
    assert abs(r["census_sum"] - want) <= 1e-12
    (r0,) = O.metrics(f1, f2, flow, patch=3, outgoing=False)          # the two columns count: |e| = c there
    assert r0["n_mask"] == H * W and r0["n_census"] == (H - 2) * (W - 2) and r0["n_valid"] == r["n_valid"]
    assert abs(r0["l1_sum"] - 3 * 2 * H * 40.0) <= 1e-9


def test_mask_and_nonfinite_rules():
    f1, f2, flow, mask = O.photo_case(1, 12, 14)
    base = O.metrics(f1, f2, flow, mask, patch=5)[0]
    for m in (mask >= 0.5, (mask >= 0.5).astype(np.uint8) * 9, mask.reshape(1, 1, 12, 14)):
        assert O.metrics(f1, f2, flow, m, patch=5)[0]["n_mask"] == base["n_mask"]
    nanmask = np.array(mask)
    nanmask[0, 0, 0] = np.nan
    assert not O.mask_pixels(nanmask, (1, 12, 14))[0, 0, 0]
    # a NaN in frame 1 taints the pixels whose patch holds it; a bad flow makes its own pixel invalid only
    g1 = np.array(f1)
    g1[0, 1, 6, 7] = np.nan
    z = np.zeros_like(flow)
    (r,) = O.metrics(g1, f2, z, patch=5)
    assert r["n_nonfinite"] == 25 and r["n_mask"] == 12 * 14
    bad = np.array(z)
    bad[0, 0, 3, 3], bad[0, 1, 4, 4], bad[0, 0, 5, 5] = np.nan, np.inf, 2.0 ** 30
    (r,) = O.metrics(f1, f2, bad, patch=5)
    assert r["n_nonfinite"] == 0 and r["n_valid"] == 12 * 14 - 3 == r["n_mask"]
    (r,) = O.metrics(f1, f2, bad, patch=5, outgoing=False)
    assert r["n_nonfinite"] == 0 and r["n_mask"] == 12 * 14


def test_oracle_case_properties():
    """The cases the GPU test compares on: no non-finite pixel, interior pixels, a valid share in (0.5, 0.95)."""
    for shape in ((2, 37, 53), (2, 19, 23)):
        f1, f2, flow, mask = O.photo_case(*shape)
        for r in O.metrics(f1, f2, flow, mask, patch=7):
            share = r["n_valid"] / r["pixels"]
            print(f"{shape}: valid share {share:.3f}, n_census {r['n_census']}")
            assert r["n_nonfinite"] == 0 and r["n_census"] > 0 and 0.5 < share < 0.95
    with pytest.raises(AssertionError):
        O.metrics(f1, f2, flow, mask, pow_ulps=O.POW_ULPS_CAP + 1)    # the cap is a condition


def test_bound_constants():
    d = np.linspace(-50, 50, 2_000_001)
    c = d / np.sqrt(O.C081 + d * d)
    assert np.abs(np.diff(c) / np.diff(d)).max() <= O.DC_DD and O.C081 ** -0.5 <= O.DC_DD < 1.113
    x = np.linspace(-2.2, 2.2, 2_000_001)
    f = x * x / (O.C01 + x * x)
    assert 2.05 < np.abs(np.diff(f) / np.diff(x)).max() <= O.DF_DDELTA
    assert O.term_bound(255.0) < 2e-3                                  # fp32 rounding, not slack


# ----------------------------------------------------------------------------- the reference's outputs


def test_golden_fixture_matches_oracle():
    """tests/golden/photo_reference.npz (make_golden_photo.py): the seeded case and what the reference's
    ternary_loss, census_loss and photometric_loss return for it in fp32.  The reference adds N fp32 terms:
    its sum lies within (N + 64) 2^-24 relative of the exact one in the worst case, N = B H W (times 3 for the
    photometric loss); the measured distances, stored beside the values, are of the order of 1e-7."""
    g = np.load(GOLDEN)
    f1, f2, flow, mask = (g[k] for k in ("frame1", "frame2", "flow", "mask"))
    case = O.photo_case(2, 37, 53)
    for a, b in zip((f1, f2, flow, mask), case):
        assert a.dtype == np.float32 and np.array_equal(a, b)        # the fixture IS the seeded case
    assert bool(g["outgoing_equals_valid"])
    n = 2 * 37 * 53
    want = {}
    for patch in (3, 7):
        r = O.result(O.totals(O.metrics(f1, f2, flow, mask, patch=patch)))
        want[f"census_p{patch}"], want[f"ternary_p{patch}"], want["photo"] = r["census"], r["ternary"], r["photo"]
    for k, terms in (("ternary_p3", n), ("census_p7", n), ("census_p3", n), ("photo", 3 * n)):
        ref, stored = float(g[k]), float(g["ref_dist_" + k])
        dist = abs(ref - want[k]) / abs(want[k])
        print(f"{k}: reference {ref:.9g}, oracle {want[k]:.9g}, distance {dist:.3e} (stored {stored:.3e})")
        assert dist <= (terms + 64) * 2.0 ** -24
        assert abs(dist - stored) <= 1e-12 and stored <= 1e-6


# ----------------------------------------------------------------------------- result()


def _totals(**kw):
    cnt = [0] * _lib.PM_SLOTS
    sums = [0.0] * _lib.PM_SLOTS
    for i, k in enumerate(_lib.PM_COUNTS):
        cnt[i] = kw.get(k, 0)
    for i, k in enumerate(_lib.PM_SUMS):
        sums[len(_lib.PM_COUNTS) + i] = kw.get(k, 0.0)
    cnt[_lib.PM_IMAGES] = kw.get("images", 0)
    sums[_lib.PM_IMAGE_CENSUS_MEAN_SUM] = kw.get("image_census_mean_sum", 0.0)
    return cnt, sums


def test_result_arithmetic_from_hand_written_totals():
    from raft_optical_flow_amd.utils import PhotoMetrics
    from raft_optical_flow_amd.utils.utils import photo_result
    assert _lib.PM_COUNTS == O.COUNTS and _lib.PM_SUMS == O.SUMS and _lib.PM_SLOTS == 16
    assert (_lib.PM_IMAGES, _lib.PM_IMAGE_CENSUS_MEAN_SUM, _lib.PM_RESERVED) == (10, 11, 12)
    kw = dict(n_mask=80, n_census=50, n_valid=90, n_nonfinite=0, pixels=100, l1_sum=480.0, photo_sum=600.0,
              hamming_sum=125.0, census_sum=75.0, ternary_sum=40.0, images=2, image_census_mean_sum=3.5)
    r = photo_result(*_totals(**kw))
    assert r == {"census": 75.0 / (50 + 1e-6), "ternary": 0.4, "photo": 2.0, "l1": 2.0, "hamming": 2.5,
                 "census_image_mean": 1.75, "valid_share": 0.9, "pixels": 100, "images": 2, "nonfinite": 0}
    assert r == O.result(kw)
    # through the class: the totals as the device keeps them (int64 slots, the sums by their bits)
    cnt, sums = _totals(**kw)
    raw = torch.tensor(cnt, dtype=torch.int64)
    raw.view(torch.float64)[5:10] = torch.tensor(sums[5:10], dtype=torch.float64)
    raw.view(torch.float64)[11] = 3.5
    m = PhotoMetrics(patch=5, outgoing=False)
    m._totals = raw
    assert m.result() == r and (m.patch, m.outgoing) == (5, False)
    # no interior pixel: census follows the reference's formula (0 / 1e-6 = 0), the means over nothing are NaN
    r = photo_result(*_totals(n_mask=45, n_valid=45, pixels=45, l1_sum=90.0, photo_sum=27.0))
    assert r["census"] == 0.0 and math.isnan(r["hamming"]) and math.isnan(r["census_image_mean"])
    assert r["ternary"] == 0.0 and r["photo"] == 0.2 and r["l1"] == 90.0 / 135 and r["images"] == 0
    none = {k: 0 for k in kw}
    none.update(n_mask=45, n_valid=45, pixels=45, l1_sum=90.0, photo_sum=27.0)
    assert r == _nan_equal(O.result(none), r)
    # nothing scored at all, and before the first update: every mean is NaN
    for r in (photo_result(*_totals()), PhotoMetrics().result()):
        assert all(math.isnan(r[k]) for k in ("census", "ternary", "photo", "l1", "hamming", "census_image_mean",
                                              "valid_share"))
        assert (r["pixels"], r["images"], r["nonfinite"]) == (0, 0, 0)
    # a mask that leaves nothing: pixels > 0, no scored pixel
    r = photo_result(*_totals(n_valid=70, pixels=100))
    assert math.isnan(r["l1"]) and math.isnan(r["hamming"]) and r["photo"] == 0.0 and r["valid_share"] == 0.7
    # a non-finite pixel taints the means; the counts and valid_share stay
    r = photo_result(*_totals(**dict(kw, n_nonfinite=3)))
    assert all(math.isnan(r[k]) for k in ("census", "ternary", "photo", "l1", "hamming", "census_image_mean"))
    assert r["valid_share"] == 0.9 and r["nonfinite"] == 3 and r["pixels"] == 100 and r["images"] == 2


def _nan_equal(a, b):
    """a, with every NaN replaced by b's value where that is a NaN too (so that == compares the rest)."""
    return {k: (b[k] if isinstance(v, float) and math.isnan(v) and math.isnan(b[k]) else v) for k, v in a.items()}


def test_metrics_reset_without_totals():
    from raft_optical_flow_amd.utils import PhotoMetrics
    m = PhotoMetrics()
    m.reset()
    assert m.result()["pixels"] == 0
    m._totals = torch.ones(16, dtype=torch.int64)
    m.reset()
    assert m.result()["pixels"] == 0 and m.result()["images"] == 0


# ----------------------------------------------------------------------------- argument validation


def test_photo_errors_argument_checks():
    from raft_optical_flow_amd.utils import PhotoMetrics, photo_errors
    fr, fl = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8)
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for fn in (photo_errors, PhotoMetrics().update):
        for f in (fr, u8):
            with pytest.raises(RuntimeError, match="ROCm GPU only"):  # CPU tensors: there is no CPU path
                fn(f, f, fl)
        with pytest.raises(RuntimeError, match="ROCm GPU only"):
            fn(fr, fr, fl, torch.ones(1, 8, 8, dtype=torch.bool))
        for args in ((fr.numpy(), fr, fl), (fr, None, fl), (fr, fr, fl.numpy())):
            with pytest.raises(TypeError, match="tensor"):
                fn(*args)
        with pytest.raises(TypeError, match="float32"):
            fn(fr, fr, fl.double())
        with pytest.raises(TypeError, match="float32 .* or uint8"):
            fn(fr.half(), fr.half(), fl)
        with pytest.raises(TypeError, match="differ in dtype"):
            fn(fr, u8, fl)
        for bad in (torch.zeros(2, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 0, 8)):
            with pytest.raises(ValueError, match=r"\[B, 2, H, W\]"):
                fn(fr, fr, bad)
        for bad in (torch.zeros(3, 8, 8), torch.zeros(1, 3, 8, 9), torch.zeros(2, 3, 8, 8), torch.zeros(1, 1, 8, 8),
                    torch.zeros(1, 8, 8, 3)):
            with pytest.raises(ValueError, match="frame1"):
                fn(bad, fr, fl)
            with pytest.raises(ValueError, match="frame2"):
                fn(fr, bad, fl)
        with pytest.raises(ValueError, match="frame1"):
            fn(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), u8, fl)
        with pytest.raises(TypeError, match="mask must be a tensor"):
            fn(fr, fr, fl, np.ones((1, 8, 8)))
        with pytest.raises(TypeError, match="bool, uint8 or float32"):
            fn(fr, fr, fl, torch.ones(1, 8, 8, dtype=torch.float64))
        for bad in (torch.ones(8, 8), torch.ones(1, 8, 9), torch.ones(1, 2, 8, 8), torch.ones(2, 8, 8)):
            with pytest.raises(ValueError, match="mask must be"):
                fn(fr, fr, fl, bad)
    for bad in (4, 9, 1, 0, -3):
        with pytest.raises(ValueError, match="patch must be 3, 5 or 7"):
            photo_errors(fr, fr, fl, patch=bad)
        with pytest.raises(ValueError, match="patch must be 3, 5 or 7"):
            PhotoMetrics(patch=bad)
    for bad in (7.0, "7", True, None):
        with pytest.raises(TypeError, match="patch must be an int"):
            photo_errors(fr, fr, fl, patch=bad)
        with pytest.raises(TypeError, match="patch must be an int"):
            PhotoMetrics(patch=bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError, match="outgoing must be a bool"):
            photo_errors(fr, fr, fl, outgoing=bad)
        with pytest.raises(TypeError, match="outgoing must be a bool"):
            PhotoMetrics(outgoing=bad)


FAKE = 1 << 20  # 16-byte aligned stand-in pointers: an argument error returns before any launch


def test_photo_symbols_and_argument_errors():
    lib = _lib.load()
    for name in ("raft_photo_metrics", "raft_photo_metrics_ws_bytes"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.raft_hip_abi_version() == 19 and _lib.ABI_VERSION == 19   # additive entries
    th, tw, cap, rec = _lib.PM_TILE_H, _lib.PM_TILE_W, _lib.PM_MAX_BLOCKS, _lib.PM_SLOTS * 8
    assert (th, tw, cap, _lib.PM_OUTGOING) == (16, 64, 512, 1)
    ws = lib.raft_photo_metrics_ws_bytes
    assert ws(1, 1, 1, 3) == rec and ws(3, th, tw, 7) == 3 * rec and ws(1, th + 1, tw + 1, 5) == 4 * rec
    assert ws(2, th * cap, 1, 7) == 2 * cap * rec and ws(2, th * cap + 1, 1, 7) == 2 * cap * rec
    assert ws(1, 436, 1024, 7) == 28 * 16 * rec
    for bad in ((0, 8, 8, 7), (1, -1, 8, 7), (1, 8, 0, 7), (1 << 10, 1 << 10, 1 << 10, 7), (1, 8, 8, 4), (1, 8, 8, 9),
                (1, 8, 8, 1)):
        assert ws(*bad) == 0, bad
    err = lib.raft_hip_last_error
    p = [FAKE * k for k in range(1, 9)]
    F32, U8 = _lib.FRAME_F32_NCHW, _lib.FRAME_U8_NHWC

    def call(**kw):
        a = dict(f1=p[0], s1b=192, s1c=64, s1p=8, f2=p[1], s2b=192, s2c=64, s2p=8, tag=F32, flow=p[2], fsb=128,
                 fsc=64, fp=8, mask=p[3], mtag=_lib.MASK_U8, msb=64, mp=8, B=1, H=8, W=8, patch=7, flags=1,
                 record=p[4], totals=p[5], cmap=p[6], ws=p[7])
        a.update(kw)
        return lib.raft_photo_metrics(*a.values(), None)

    for k in ("f1", "f2", "flow", "record", "ws"):
        assert call(**{k: None}) == -1 and b"null pointer" in err()
    for patch in (1, 4, 9, 0):
        assert call(patch=patch) == -1 and b"patch must be" in err()
    for kw in ({"B": 0}, {"H": -1}, {"W": 0}, {"B": 1 << 10, "H": 1 << 10, "W": 1 << 10}):
        assert call(**kw) == -1 and b"bad size" in err()
    assert call(tag=2) == -1 and b"unknown frame dtype" in err()
    assert call(mtag=2) == -1 and b"unknown mask dtype" in err()
    for flags in (2, 3, -1):
        assert call(flags=flags) == -1 and b"unknown flags" in err()
    for kw in ({"fp": 7}, {"fsb": -1}, {"fsc": -1}):
        assert call(**kw) == -1 and b"bad strides" in err()
    for kw in ({"s1p": 7}, {"s2p": 7}, {"s1b": -1}, {"s2c": -8}):
        assert call(**kw) == -1 and b"bad frame strides" in err()
    for kw in ({"mp": 7}, {"msb": -1}):
        assert call(**kw) == -1 and b"bad mask strides" in err()
    for kw in ({"f1": p[0] + 2}, {"f2": p[1] + 1}, {"flow": p[2] + 2}, {"cmap": p[6] + 1}, {"record": p[4] + 4},
               {"totals": p[5] + 4}, {"ws": p[7] + 4}, {"mtag": _lib.MASK_F32, "mask": p[3] + 2}):
        assert call(**kw) == -1 and b"misaligned" in err()
    for kw in ({"record": p[0]}, {"ws": p[1]}, {"totals": p[2]}, {"cmap": p[3]}, {"ws": p[4]}, {"cmap": p[5]},
               {"totals": p[4]}):
        assert call(**kw) == -1 and b"aliases" in err()
    # uint8 frames are dense: their strides are not read and they need no alignment; a byte mask needs none
    # (the alias check is the last one: reaching it shows that the earlier ones passed)
    assert call(tag=U8, f1=p[0] + 1, f2=p[1] + 3, s1p=0, s2b=-1, mask=p[3] + 1, ws=p[4]) == -1 and b"aliases" in err()


def test_sources_mention_the_new_file_and_entries():
    with open(os.path.join(ROOT, "raft_optical_flow_amd", "csrc", "Makefile")) as fh:
        srcs = next(ln for ln in fh if ln.startswith("SRCS :="))
    assert "photo_metrics.hip" in srcs.split()                   # built, and hashed with the rest
    with open(os.path.join(ROOT, "include", "raft_hip.h")) as fh:
        hdr = fh.read()
    for name in ("raft_photo_metrics(", "raft_photo_metrics_ws_bytes(", "#define RAFT_PHOTO_METRICS_TILE_H 16",
                 "#define RAFT_PHOTO_METRICS_TILE_W 64", "#define RAFT_PHOTO_METRICS_MAX_BLOCKS 512",
                 "#define RAFT_HIP_ABI_VERSION 19"):
        assert name in hdr, name
    csrc = os.path.join(ROOT, "raft_optical_flow_amd", "csrc")
    with open(os.path.join(csrc, "photo_metrics.hip")) as fh:
        src = fh.read()
    assert 'extern "C" int raft_photo_metrics(' in src and "#pragma clang fp contract(off)" in src
    assert '#include "warp_common.hpp"' in src
    with open(os.path.join(csrc, "flow_warp.hip")) as fh:         # one copy of the warp arithmetic
        assert '#include "warp_common.hpp"' in fh.read()
    from raft_optical_flow_amd.utils import utils as U_
    for word in ("photo_errors", "PhotoMetrics", "census_loss", "ternary_loss", "photometric_loss"):
        assert word in U_.__doc__, word
    assert "stream.push" in U_.photo_errors.__doc__ and "~out.occ_fw" in U_.photo_errors.__doc__
