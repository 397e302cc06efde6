"""The frame-warp additions that need no GPU: fp64 restatements of raft_warp_frame and raft_splat_density
(include/raft_hip.h) with their fp32 error bounds, pinned against torch's grid_sample in float64 and against the
reference's image_warp / IFNET_m.warp outputs (tests/golden/warp_reference.npz); the random cases the kernel test
uses and their caps; argument validation of warp_frame, splat_density and stream(warp=...); the new C-ABI
entries' argument errors.

tests/test_gpu_warp.py imports the restatements (warp_reference, density_reference), the bounds and the cases."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

from raft_optical_flow_amd import _lib

U = 2.0 ** -24                    # fp32 unit roundoff (round to nearest)
LIMIT = 2.0 ** 30                 # a displacement of this magnitude (or a non-finite one) is rejected
SHAPES = [(1, 5, 7), (2, 37, 53), (1, 16, 260)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "warp_reference.npz")


# ----------------------------------------------------------------------------- the restatements


def _axis(j, d, n, border):
    """One axis in fp64: (i0, t, inside).  fl = floor(d), t = d - fl, i0 = j + fl; inside: j + d in [0, n-1],
    tested without forming the sum; border mode clamps (i0, t) afterwards."""
    fl = np.floor(d)
    t = d - fl
    i0 = (j + fl).astype(np.int64)
    inside = (i0 >= 0) & ((i0 < n - 1) | ((i0 == n - 1) & (t == 0)))
    if border:
        lo, hi = i0 < 0, i0 >= n - 1
        t = np.where(lo | hi, 0.0, t)
        i0 = np.where(lo, 0, np.where(hi, n - 1, i0))
    return i0, t, inside


def warp_reference(frame, flow, border=False):
    """raft_warp_frame in fp64.  frame [B,C,H,W], flow [B,2,H,W] (values taken as given and widened).  Returns a
    dict: value [B,C,H,W]; valid [B,H,W] bool; T [B,C,H,W], the largest |tap| that was read; bound [B,C,H,W] =
    10 u T + 1e-37, the fp32 error bound of the kernel's blend (derivation: tests/test_bidi_host.py's bound_err,
    `blend`: every tap passes through two products and two sums with two weights in error by <= u each; taps
    outside the frame are exact zeros); margin [B,H,W], the distance of x + flow(x) to the frame's edge (0 on it,
    inf for rejected displacements)."""
    frame = np.asarray(frame, dtype=np.float64)
    flow = np.asarray(flow, dtype=np.float64)
    B, C, H, W = frame.shape
    assert flow.shape == (B, 2, H, W), (frame.shape, flow.shape)
    jj = np.broadcast_to(np.arange(W, dtype=np.float64)[None, None, :], (B, H, W))
    ii = np.broadcast_to(np.arange(H, dtype=np.float64)[None, :, None], (B, H, W))
    with np.errstate(invalid="ignore"):
        ok = (np.abs(flow[:, 0]) < LIMIT) & (np.abs(flow[:, 1]) < LIMIT)       # False for NaN and inf
    dx, dy = np.where(ok, flow[:, 0], 0.0), np.where(ok, flow[:, 1], 0.0)
    x0, ax, inx = _axis(jj, dx, W, border)
    y0, ay, iny = _axis(ii, dy, H, border)
    bb = np.arange(B)[:, None, None]
    value = np.zeros((B, C, H, W))
    T = np.zeros((B, C, H, W))
    for c in range(C):
        taps = []
        for yy, xx in ((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)):
            m = ok & (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)    # outside the crop: 0, not read
            taps.append(np.where(m, frame[bb, c, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0.0))
        v00, v01, v10, v11 = taps
        with np.errstate(invalid="ignore", over="ignore"):
            value[:, c] = (1 - ay) * ((1 - ax) * v00 + ax * v01) + ay * ((1 - ax) * v10 + ax * v11)
            T[:, c] = np.nan_to_num(np.max(np.abs(taps), axis=0), nan=np.inf)
    value = np.where(ok[:, None], value, 0.0)
    valid = ok & inx & iny
    px, py = jj + dx, ii + dy      # (fp64: exact for every fp32 flow of the cases used here)
    margin = np.minimum(np.minimum(np.abs(px), np.abs(px - (W - 1))), np.minimum(np.abs(py), np.abs(py - (H - 1))))
    margin = np.where(ok, margin, np.inf)
    return {"value": value, "valid": valid, "T": T, "bound": 10.0 * U * T + 1e-37, "margin": margin}


def density_reference(flow):
    """raft_splat_density in fp64.  flow [B,2,H,W].  Returns (density [B,H,W], n [B,H,W], bound [B,H,W]): n is the
    number of taps added to the pixel (four per contributing source, zero weights included).  Per tap the fp32
    weight carries 3 roundings (<= 3 u absolute: the weights are <= 1) and the fixed-point truncation <= 2^-32;
    the conversion of the sum rounds once more: bound = n (3 u + 2^-32) + u density."""
    flow = np.asarray(flow, dtype=np.float64)
    B, _, H, W = flow.shape
    den = np.zeros((B, H, W))
    n = np.zeros((B, H, W), dtype=np.int64)
    jj = np.broadcast_to(np.arange(W, dtype=np.float64)[None, None, :], (B, H, W))
    ii = np.broadcast_to(np.arange(H, dtype=np.float64)[None, :, None], (B, H, W))
    with np.errstate(invalid="ignore"):
        ok = (np.abs(flow[:, 0]) < LIMIT) & (np.abs(flow[:, 1]) < LIMIT)
    dx, dy = np.where(ok, flow[:, 0], 0.0), np.where(ok, flow[:, 1], 0.0)
    flx, fly = np.floor(dx), np.floor(dy)
    ax, ay = dx - flx, dy - fly
    x0, y0 = (jj + flx).astype(np.int64), (ii + fly).astype(np.int64)
    ok &= (x0 >= 0) & (x0 <= W - 1) & (y0 >= 0) & (y0 <= H - 1)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    bb = np.broadcast_to(np.arange(B)[:, None, None], (B, H, W))
    for yy, xx, wt in ((y0, x0, (1 - ax) * (1 - ay)), (y0, x1, ax * (1 - ay)), (y1, x0, (1 - ax) * ay),
                       (y1, x1, ax * ay)):
        np.add.at(den, (bb[ok], yy[ok], xx[ok]), wt[ok])
        np.add.at(n, (bb[ok], yy[ok], xx[ok]), 1)
    return den, n, n * (3.0 * U + 2.0 ** -32) + U * den


# ----------------------------------------------------------------------------- the random cases


@functools.lru_cache(maxsize=None)
def warp_case(B, H, W, C=3, seed=7):
    """(frame [B,C,H,W] float32 in 0..255, flow [B,2,H,W] float32): a smooth image plus noise, a smooth flow of
    up to about 9 px (a quarter of the frame where that is less) with per-pixel noise added on image 1 (the last
    image of a batch of one is left smooth).  rint() of the frame is the uint8 case's frame."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    y, x = np.mgrid[:H, :W].astype(np.float64)
    frame = np.empty((B, C, H, W))
    for b in range(B):
        for c in range(C):
            k = rng.uniform(0.5, 3.0, size=2)
            ph = rng.uniform(0, 2 * np.pi, size=2)
            frame[b, c] = 127.5 + 90.0 * np.sin(2 * np.pi * k[0] * x / W + ph[0]) * np.cos(
                2 * np.pi * k[1] * y / H + ph[1])
    frame = np.clip(frame + rng.uniform(-30, 30, size=frame.shape), 0.0, 255.0)
    ampx, ampy = min(9.0, W / 4.0), min(9.0, H / 4.0)
    flow = np.empty((B, 2, H, W))
    for b in range(B):
        ph = rng.uniform(0, 2 * np.pi, size=4)
        flow[b, 0] = ampx * np.sin(2 * np.pi * 0.8 * x / W + ph[0]) * np.cos(2 * np.pi * 0.6 * y / H + ph[1])
        flow[b, 1] = ampy * np.cos(2 * np.pi * 0.7 * x / W + ph[2]) * np.sin(2 * np.pi * 0.9 * y / H + ph[3])
    if B > 1:
        flow[1] += rng.standard_normal((2, H, W)) * 1.5
    return frame.astype(np.float32), flow.astype(np.float32)


def u8_frame(frame):
    """The uint8 [B,H,W,3] version of a float frame [B,3,H,W] in 0..255."""
    return np.ascontiguousarray(np.rint(frame).astype(np.uint8).transpose(0, 2, 3, 1))


def half_margin(value):
    """Distance of each value, clamped to 0..255, to the nearest half-integer: where it exceeds the error bound,
    rint(fp32 result) equals rint(fp64 value)."""
    v = np.clip(value, 0.0, 255.0)
    return np.abs(v - np.floor(v) - 0.5)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("border", [False, True])
def test_random_case_caps(shape, border):
    """The uint8 comparison leaves out the pixels whose fp64 value lies within the fp32 bound of a half-integer:
    on the fp64 reference alone they are at most 1 % of the frame.  On the 2 x 37 x 53 case the valid share lies
    strictly between 0.5 and 0.95, so the kernel's in-frame and out-of-frame branches both run."""
    frame, flow = warp_case(*shape)
    for fr in (frame, np.rint(frame)):
        d = warp_reference(fr, flow, border)
        close = half_margin(d["value"]) <= d["bound"]
        share = close.any(axis=1).mean()
        print(f"{shape} border={border}: half-integer share {share:.2e}, valid share {d['valid'].mean():.3f}, "
              f"max bound {d['bound'].max():.2e}")
        assert share <= 0.01, share
        assert float(d["bound"].max()) <= 10 * U * 255.0 + 1e-30      # the bound is fp32 rounding, not slack
    if shape == SHAPES[1]:
        assert 0.5 < d["valid"].mean() < 0.95, d["valid"].mean()
    _, n, bound = density_reference(flow)
    assert float(bound.max()) < 1e-4 and n.max() >= 4


# ----------------------------------------------------------------------------- vs grid_sample (float64)


@pytest.mark.parametrize("border", [False, True])
def test_restatement_matches_grid_sample(border):
    """The definition is grid_sample(align_corners=True) with padding_mode zeros / border: float64 on both sides
    and the normalised grid built in float64, so only the grid's own round trip separates them."""
    frame, flow = warp_case(2, 37, 53)
    B, C, H, W = frame.shape
    d = warp_reference(frame, flow, border)
    f64 = flow.astype(np.float64)
    px = np.arange(W)[None, None, :] + f64[:, 0]
    py = np.arange(H)[None, :, None] + f64[:, 1]
    grid = torch.from_numpy(np.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], -1))
    g = torch.nn.functional.grid_sample(torch.from_numpy(frame.astype(np.float64)), grid, mode="bilinear",
                                        padding_mode="border" if border else "zeros", align_corners=True).numpy()
    # a position within 1e-9 of an integer may fall on the other side of it after the round trip: the taps
    # differ there, the value does not (bilinear interpolation is continuous), so no pixel is left out
    rel = np.abs(g - d["value"]).max() / 255.0
    print(f"border={border}: max |restatement - grid_sample| / 255 = {rel:.2e}")
    assert rel <= 1e-9
    assert 0.5 < d["valid"].mean() < 0.95


def test_restatement_edge_rules():
    """Zero flow returns the frame; a whole-pixel shift shifts it, with zeros (or the replicated edge) in the
    band and valid False there; positions in (-1, 0) keep their partial weight in zeros mode and clamp in border
    mode; a target exactly on the last column reads nothing beyond it (NaN there would show); non-finite and
    huge displacements give 0 and invalid in both modes."""
    rng = np.random.default_rng(3)
    fr = rng.uniform(0, 255, size=(1, 2, 6, 9))
    z = np.zeros((1, 2, 6, 9))
    for border in (False, True):
        d = warp_reference(fr, z, border)
        assert np.array_equal(d["value"], fr) and d["valid"].all()
    f = z.copy()
    f[:, 0], f[:, 1] = 2, -1
    band = (np.arange(9)[None, :] > 6) | (np.arange(6)[:, None] < 1)
    d = warp_reference(fr, f, False)
    want = np.zeros_like(fr)
    want[..., 1:, :7] = fr[..., :5, 2:]
    assert np.array_equal(d["value"], want) and np.array_equal(d["valid"][0], ~band)
    d = warp_reference(fr, f, True)
    want = fr[..., np.clip(np.arange(6) - 1, 0, 5), :][..., np.clip(np.arange(9) + 2, 0, 8)]
    assert np.array_equal(d["value"], want) and np.array_equal(d["valid"][0], ~band)
    f = z.copy()
    f[:, 0] = -np.arange(9)[None, :] - 0.25          # every pixel targets x = -0.25
    d = warp_reference(fr, f, False)
    assert np.allclose(d["value"], 0.75 * fr[..., :1], rtol=1e-15) and not d["valid"].any()
    d = warp_reference(fr, f, True)
    assert np.array_equal(d["value"], np.broadcast_to(fr[..., :1], fr.shape)) and not d["valid"].any()
    f = z.copy()
    f[:, 0] = 8 - np.arange(9)[None, :]              # every pixel targets column W-1 exactly
    nan_beyond = np.concatenate([fr, np.full((1, 2, 6, 1), np.nan)], axis=3)[..., :9]
    d = warp_reference(nan_beyond, f, False)
    assert np.array_equal(d["value"], np.broadcast_to(fr[..., 8:], fr.shape)) and d["valid"].all()
    for bad in (np.nan, np.inf, -np.inf, 3e38, 2.0 ** 30, -2.0 ** 30):
        f = z.copy()
        f[0, 0, 2, 3] = bad
        f[0, 1, 4, 5] = bad
        for border in (False, True):
            d = warp_reference(fr, f, border)
            assert not d["valid"][0, 2, 3] and not d["valid"][0, 4, 5]
            assert np.all(d["value"][0, :, 2, 3] == 0) and np.all(d["value"][0, :, 4, 5] == 0)
            assert d["valid"].sum() == 6 * 9 - 2
    f = z.copy()
    f[0, 0, 0, 0] = np.nextafter(np.float32(2.0 ** 30), np.float32(0))      # just below the limit: not rejected
    assert warp_reference(fr, f, True)["value"][0, 0, 0, 0] == fr[0, 0, 0, 8]


def test_density_restatement_analytic():
    """No reference density is stored (the reference's indexed `+=` keeps one write per pixel, not the sum), so
    the restatement is pinned analytically: zero flow gives ones; a whole-pixel shift gives exactly 1 on the
    shifted interior and 0 in the band; every source onto one pixel gives H W; a fractional target in the last
    column puts both weights on the edge pixel."""
    H, W = 6, 9
    z = np.zeros((1, 2, H, W))
    den, n, bound = density_reference(z)
    assert np.all(den == 1) and n.sum() == 4 * H * W and np.all(n[0, 1:-1, 1:-1] == 4)
    f = z.copy()
    f[:, 0], f[:, 1] = 2, -1
    den, _, _ = density_reference(f)
    want = np.zeros((H, W))
    want[:H - 1, 2:] = 1
    assert np.array_equal(den[0], want)
    f = z.copy()
    f[0, 0] = 3 - np.arange(W)[None, :]
    f[0, 1] = 2 - np.arange(H)[:, None]
    den, _, _ = density_reference(f)
    assert den[0, 2, 3] == H * W and den.sum() == H * W
    f = z.copy()
    f[0, 0, :, W - 1] = 0.25          # x0 = W-1, ax = 0.25: x1 clamps to W-1
    f[0, 1, H - 1, :] = 0.5           # likewise in y
    den, _, _ = density_reference(f)
    assert np.all(den == 1)
    f[0, 0, 0, 0] = np.nan
    f[0, 1, 1, 1] = -np.inf
    f[0, 0, 2, 2] = 2.0 ** 30
    den, _, _ = density_reference(f)
    assert den[0, 0, 0] == 0 and den[0, 1, 1] == 0 and den[0, 2, 2] == 0 and den.sum() == H * W - 3


# ----------------------------------------------------------------------------- the reference's outputs


def test_golden_fixture_matches_restatement():
    """tests/golden/warp_reference.npz (make_golden_warp.py): seeded inputs and what the reference's image_warp
    and IFNET_m.warp return for them, in fp32 through grid_sample's normalised grid.  Each output's distance to
    the fp64 restatement was stored with it; the restatement here reproduces those distances, and they are the
    size the fp32 grid round trip explains (~1e-3 on values in 0..255), not a difference of definition."""
    g = np.load(GOLDEN)
    frame, flow = g["frame"], g["flow"]
    assert frame.shape == (2, 3, 37, 53) and flow.shape == (2, 2, 37, 53)
    assert frame.dtype == np.float32 and flow.dtype == np.float32
    assert 0 <= frame.min() and frame.max() <= 255 and 5 < np.abs(flow[0]).max() < 10
    c_frame, c_flow = warp_case(2, 37, 53)
    assert np.array_equal(frame, c_frame) and np.array_equal(flow, c_flow)   # the fixture IS the random case
    for name, border in (("zeros", False), ("border", True)):
        d = warp_reference(frame, flow, border)
        dist = float(np.abs(g["warp_" + name].astype(np.float64) - d["value"]).max())
        stored = float(g["ref_dist_" + name])
        print(f"{name}: reference's distance to fp64 {dist:.3e} (stored {stored:.3e})")
        assert abs(dist - stored) <= 1e-9 * stored
        assert 1e-5 < stored < 5e-3


# ----------------------------------------------------------------------------- argument validation


def _model():
    from raft_optical_flow_amd import RAFT
    return RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False)).eval()


def test_stream_warp_argument_checks():
    from raft_optical_flow_amd import (BidirectionalFlow, BidirectionalFlowViz, BidirectionalFlowVizWarp,
                                       BidirectionalFlowWarp, FlowStream, FlowVizWarp, FlowWarp)
    m = _model()
    assert m.stream().warp is None                                # the default: no warp
    for mode in ("zeros", "border"):
        s = m.stream(iters=2, warp=mode)
        assert isinstance(s, FlowStream) and s.warp == mode
        assert m.stream(bidirectional=True, visualize="rgb", warp=mode).warp == mode
    for bad in ("reflection", "ZEROS", True, 1, ""):
        with pytest.raises(ValueError, match="warp must be"):
            m.stream(warp=bad)
    assert FlowWarp._fields == ("flow_low", "flow_up", "warped", "valid")
    assert FlowVizWarp._fields == ("flow_low", "flow_up", "rgb", "warped", "valid")
    tail = ("warped_fw", "warped_bw", "valid_fw", "valid_bw")
    assert BidirectionalFlowWarp._fields == BidirectionalFlow._fields + tail
    assert BidirectionalFlowVizWarp._fields == BidirectionalFlowViz._fields + tail
    s = m.stream(warp="zeros")
    with pytest.raises(ValueError, match="a frame is"):           # the frame checks come before any device work
        s.push(torch.zeros(3, 16, 16))
    s.close()
    with pytest.raises(RuntimeError, match="close"):
        s.push(torch.zeros(1, 3, 16, 16))


def test_warp_frame_argument_checks():
    from raft_optical_flow_amd.utils import warp_frame
    fr, fl = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8)
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for f in (fr, u8):
        with pytest.raises(RuntimeError, match="ROCm GPU only"):  # CPU tensors: there is no CPU path
            warp_frame(f, fl)
    with pytest.raises(TypeError, match="tensor"):
        warp_frame(fr.numpy(), fl)
    with pytest.raises(TypeError, match="tensor"):
        warp_frame(fr, fl.numpy())
    with pytest.raises(TypeError, match="float32"):
        warp_frame(fr, fl.double())
    with pytest.raises(TypeError, match="float32 .* or uint8"):
        warp_frame(fr.half(), fl)
    for bad in (torch.zeros(2, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 0, 8)):
        with pytest.raises(ValueError, match=r"\[B, 2, H, W\]"):
            warp_frame(fr, bad)
    for bad in (torch.zeros(3, 8, 8), torch.zeros(1, 3, 8, 9), torch.zeros(2, 3, 8, 8),
                torch.zeros(1, 8, 8, 4, dtype=torch.uint8), torch.zeros(1, 3, 8, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="frame"):
            warp_frame(bad, fl)
    with pytest.raises(ValueError, match="padding"):
        warp_frame(fr, fl, padding="reflection")
    with pytest.raises(TypeError, match="out_dtype"):
        warp_frame(fr, fl, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="3 channels"):
        warp_frame(torch.zeros(1, 5, 8, 8), fl, out_dtype=torch.uint8)


def test_splat_density_argument_checks():
    from raft_optical_flow_amd.utils import splat_density
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        splat_density(torch.zeros(1, 2, 8, 8))
    with pytest.raises(TypeError, match="tensor"):
        splat_density(np.zeros((1, 2, 8, 8), dtype=np.float32))
    with pytest.raises(TypeError, match="float32"):
        splat_density(torch.zeros(1, 2, 8, 8, dtype=torch.float64))
    for bad in (torch.zeros(2, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 0)):
        with pytest.raises(ValueError, match=r"\[B, 2, H, W\]"):
            splat_density(bad)


FAKE = 1 << 20  # 16-byte aligned stand-in pointers: an argument error returns before any launch


def test_warp_symbols_and_argument_errors():
    lib = _lib.load()
    for name in ("raft_warp_frame", "raft_splat_ws_bytes", "raft_splat_density"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.raft_hip_abi_version() == 19 and _lib.ABI_VERSION == 19   # additive entries
    assert _lib.WARP_BORDER == 1
    err = lib.raft_hip_last_error
    p = [FAKE * k for k in range(1, 6)]
    F32, U8 = _lib.FRAME_F32_NCHW, _lib.FRAME_U8_NHWC

    def warp(**kw):
        a = dict(flow=p[0], fsb=128, fsc=64, fp=8, frame=p[1], tag=F32, isb=192, isc=64, ip=8, top=0, left=0, B=1,
                 C=3, H=8, W=8, flags=0, out=p[2], otag=F32, valid=p[3])
        a.update(kw)
        return lib.raft_warp_frame(*a.values(), None)

    for k in ("flow", "frame", "out", "valid"):
        assert warp(**{k: None}) == -1 and b"null pointer" in err()
    for kw in ({"B": 0}, {"H": -1}, {"W": 0}, {"B": 1 << 10, "H": 1 << 10, "W": 1 << 10, "fp": 1 << 10, "ip": 1 << 10}):
        assert warp(**kw) == -1 and b"bad size" in err()
    assert warp(tag=2) == -1 and b"unknown frame dtype" in err()
    assert warp(otag=-1) == -1 and b"unknown output dtype" in err()
    for flags in (2, 4, -1):
        assert warp(flags=flags) == -1 and b"unknown flags" in err()
    assert warp(C=0) == -1 and b"bad channel count" in err()
    for kw in ({"tag": U8, "C": 4}, {"otag": U8, "C": 1}, {"tag": U8, "otag": U8, "C": 5}):
        assert warp(**kw) == -1 and b"3 channels" in err()
    for kw in ({"top": -1}, {"left": -2}):
        assert warp(**kw) == -1 and b"negative crop" in err()
    for kw in ({"fp": 7}, {"left": 1}, {"fsb": -1}, {"fsc": -1}):
        assert warp(**kw) == -1 and b"bad strides" in err()
    for kw in ({"ip": 7}, {"isb": -1}, {"isc": -8}):
        assert warp(**kw) == -1 and b"bad frame strides" in err()
    for kw in ({"flow": p[0] + 2}, {"frame": p[1] + 1}, {"out": p[2] + 4}, {"valid": p[3] + 1},
               {"otag": U8, "out": p[2] + 2}):
        assert warp(**kw) == -1 and b"misaligned" in err()
    for kw in ({"out": p[0]}, {"out": p[1]}, {"valid": p[2]}, {"valid": p[0]}, {"valid": p[1]}):
        assert warp(**kw) == -1 and b"aliases" in err()
    # a uint8 frame is dense: its strides are not read, and it needs no alignment
    # (the alias check is the last one: reaching it shows that the earlier ones passed)
    assert warp(tag=U8, frame=p[1] + 1, isb=-1, ip=0, valid=p[2]) == -1 and b"aliases" in err()

    assert lib.raft_splat_ws_bytes(2, 37, 53) == 2 * 37 * 53 * 8
    assert lib.raft_splat_ws_bytes(0, 8, 8) == 0 and lib.raft_splat_ws_bytes(1 << 10, 1 << 10, 1 << 10) == 0

    def splat(**kw):
        a = dict(flow=p[0], sb=128, sc=64, pitch=8, top=0, left=0, B=1, H=8, W=8, ws=p[1], den=p[2])
        a.update(kw)
        return lib.raft_splat_density(*a.values(), None)

    for k in ("flow", "ws", "den"):
        assert splat(**{k: None}) == -1 and b"null pointer" in err()
    for kw in ({"B": 0}, {"H": 0}, {"W": -3}, {"B": 1 << 10, "H": 1 << 10, "W": 1 << 10, "pitch": 1 << 10}):
        assert splat(**kw) == -1 and b"bad size" in err()
    assert splat(top=-1) == -1 and b"negative crop" in err()
    for kw in ({"pitch": 7}, {"left": 1}, {"sb": -1}, {"sc": -1}):
        assert splat(**kw) == -1 and b"bad strides" in err()
    for kw in ({"flow": p[0] + 1}, {"ws": p[1] + 4}, {"den": p[2] + 2}):
        assert splat(**kw) == -1 and b"misaligned" in err()
    for kw in ({"den": p[0]}, {"den": p[1]}, {"ws": p[0]}):
        assert splat(**kw) == -1 and b"aliases" in err()


def test_sources_mention_the_new_file_and_entries():
    with open(os.path.join(ROOT, "raft_optical_flow_amd", "csrc", "Makefile")) as fh:
        srcs = next(ln for ln in fh if ln.startswith("SRCS :="))
    assert "flow_warp.hip" in srcs.split()                       # built, and hashed with the rest
    with open(os.path.join(ROOT, "include", "raft_hip.h")) as fh:
        hdr = fh.read()
    for name in ("raft_warp_frame(", "raft_splat_density(", "raft_splat_ws_bytes(", "#define RAFT_WARP_BORDER 1",
                 "#define RAFT_HIP_ABI_VERSION 19"):
        assert name in hdr, name
    with open(os.path.join(ROOT, "raft_optical_flow_amd", "csrc", "flow_warp.hip")) as fh:
        src = fh.read()
    assert 'extern "C" int raft_warp_frame(' in src and 'extern "C" int raft_splat_density(' in src
    from raft_optical_flow_amd.utils import utils as U_
    for word in ("warp_frame", "splat_density", "image_warp", "backward_warp_op", "IFNET_m.warp"):
        assert word in U_.__doc__, word
