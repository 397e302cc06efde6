"""The flow colour-wheel visualisation on the GPU: raft_flow_to_rgb, utils.flow_viz and RAFT.stream(visualize=...).

Bound (set from the number formats, not from what the kernel gives): the kernel computes in fp32 what the
reference computes in fp32 / fp64 and the oracle (tests/flow_viz_oracle.py) in fp64.  The colour is a continuous
function of the flow but for floor(255 * col), so a rounding difference can move a byte by one level where
255 * col lies within ~1e-5 of an integer.  Every byte must be within 1 level, and at most 1e-3 of a case's
pixels may differ at all; a wrong wheel index, channel order, normalisation or branch moves most of the image.
(The reference stands at 0 differing pixels against the fp64 oracle on the fixtures: test_flow_viz_host.py.)

The fixtures hold no pixel ON a discontinuity of the colour in exact arithmetic (radius exactly 1; outside the
unit disc, a direction at an exact multiple of 45 degrees, where 255 * col is an integer such as
0.75 * (0.75 * 215 + 0.25 * 235) = 165): there floor() is decided by the last rounding of whichever arithmetic
evaluates it, fp64 included (tests/golden/make_golden_viz.py).

Observed on an MI355X (differing pixels / pixels, largest difference in levels):
  every golden case (3 x 37 x 53 fields, 64 x 64 chart, clip_flow, bgr, flow_uv_to_colors)   0, 0 levels
  non-finite pixels, fixed rad_max = 2, clip with infinities, both crops, the Python forms    0, 0 levels
  1 x 61 x 93 and 2 x 33 x 64 against the oracle                         1 / 5673 and 1 / 4224, 1 level
  every other shape, the stream's rgb against the oracle (2 x 60 x 76)                         0, 0 levels
  demo.py's sequence at 440 x 1024 against the oracle                             7 / 450560, 1 level
"""
import argparse
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import flow_viz_oracle as O
from conftest import GOLDEN, REPO, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


@functools.lru_cache(maxsize=None)
def gold():
    return load_golden("flow_viz.npz")


def close(got, want, what):
    """The bound of the module docstring; prints the figures before it asserts."""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape, got.dtype)
    worst, frac = O.compare(got, want)
    npx = want.size // 3
    print(f"flow_viz {what}: {round(frac * npx)} / {npx} pixels differ, max {worst} level(s)")
    assert worst <= 1 and frac <= 1e-3, (what, worst, frac)


def kernel(flow, H=None, W=None, top=0, left=0, rad_max=None, clip=None, bgr=False, unit=False, frame=None):
    """raft_flow_to_rgb through the C-ABI on a contiguous GPU buffer [B,2,Hb,Wb] (frame [B,3,Hb,Wb]), the image
    being the H x W crop at (top, left).  The output buffer is longer than the image and canary-filled: the
    bytes past the end must stay untouched.  Returns uint8 [B,Hout,W,3]."""
    from raft_optical_flow_amd import _lib as L
    B, _, Hb, Wb = flow.shape
    H, W = H or Hb, W or Wb
    assert flow.is_contiguous() and flow.is_cuda and (frame is None or frame.is_contiguous())
    Hout = 2 * H if frame is not None else H
    n = B * Hout * W * 3
    out = torch.full((n + 64,), CANARY, dtype=torch.uint8, device=flow.device)
    flags = (L.VIZ_BGR if bgr else 0) | (L.VIZ_UNIT if unit else 0) | (L.VIZ_CLIP if clip is not None else 0)
    own = rad_max is None and not unit
    nws = L.load().raft_flow_viz_ws_bytes(B, H, W) // 4
    ws = torch.full((nws + 16,), 1e30, device=flow.device)   # stale and huge: every slot must be written first
    L.call("raft_flow_to_rgb", flow.data_ptr(), 2 * Hb * Wb, Hb * Wb, Wb, top, left, B, H, W, clip or 0.0,
           rad_max or 0.0, flags, frame.data_ptr() if frame is not None else None, 3 * Hb * Wb, Hb * Wb, Wb,
           ws.data_ptr() if own else None, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (out[n:] == CANARY).all(), "bytes past the output's end were written"
    assert (ws[nws:] == 1e30).all(), "floats past the workspace's end were written"
    return out[:n].view(B, Hout, W, 3)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------
# the kernel against the reference's goldens and the fp64 oracle
# ---------------------------------------------------------------------------------------------

def test_kernel_against_reference_goldens():
    g = gold()
    close(kernel(dev(g["flows"])), g["img_flows"], "golden flows 3x37x53")
    close(kernel(dev(g["chart"][None])), g["img_chart"][None], "golden chart 64x64")
    close(kernel(dev(g["flows"][1:2]), clip=3.0), g["img_clip3"][None], "golden clip_flow=3")
    close(kernel(dev(g["flows"][:1]), bgr=True), g["img_bgr"][None], "golden bgr")
    close(kernel(dev(g["uv"][None]), unit=True), g["img_uv"][None], "golden flow_uv_to_colors")
    # and the oracle on the same inputs (it equals the goldens byte for byte: test_flow_viz_host.py)
    close(kernel(dev(g["flows"])), O.flow_to_rgb(g["flows"]), "oracle flows 3x37x53")


def test_kernel_cases_the_reference_cannot_define():
    g = gold()
    f = g["flows"][:2].copy()
    big = float(np.sqrt((f[0].astype(np.float64) ** 2).sum(0)).max())
    f[0, :, 3, 4] = (np.nan, 1.0)
    f[0, :, 5, 6] = (1.0, np.inf)
    f[0, :, 7, 8] = (-np.inf, np.nan)
    f[0, :, 9, 10] = (np.inf, 100 * big)
    f[0, :, 36, 52] = (np.nan, np.nan)
    got = kernel(dev(f))
    for y, x in ((3, 4), (5, 6), (7, 8), (9, 10), (36, 52)):
        assert (got[0, y, x] == 0).all(), (y, x)            # exactly black
    close(got, O.flow_to_rgb(f), "non-finite pixels")       # and they did not move the maximum
    assert (kernel(torch.zeros(2, 2, 9, 11, device=DEV)) == 255).all()                     # all-zero flow
    assert (kernel(torch.full((1, 2, 9, 11), float("nan"), device=DEV)) == 0).all()        # all non-finite
    mixed = torch.zeros(2, 2, 9, 11, device=DEV)
    mixed[0] = float("inf")
    got = kernel(mixed)
    assert (got[0] == 0).all() and (got[1] == 255).all()
    # a fixed rad_max below the field: the 3/4-brightness branch on most pixels
    f = g["flows"][:2]
    want = O.flow_to_rgb(f, rad_max=2.0)
    assert (np.sqrt((f.astype(np.float64) ** 2).sum(1)) > 2.0).mean() > 0.5
    close(kernel(dev(f), rad_max=2.0), want, "fixed rad_max=2 (0.75 branch)")
    # clip with infinities: +inf becomes clip_flow, -inf becomes 0, NaN stays black
    f = g["flows"][:1].copy()
    f[0, :, 1, 1] = (np.inf, -np.inf)
    f[0, :, 2, 2] = (np.nan, 0.0)
    got = kernel(dev(f), clip=3.0)
    close(got, O.flow_to_rgb(f, clip_flow=3.0), "clip_flow with infinities")
    assert (got[0, 2, 2] == 0).all() and not (got[0, 1, 1] == 0).all()


# ---------------------------------------------------------------------------------------------
# shapes where the kernel can go wrong
# ---------------------------------------------------------------------------------------------

def field(B, H, W, seed, scale=4.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, 2, H, W)) * scale).astype(np.float32)


@pytest.mark.parametrize("B,H,W", [(1, 5, 7), (1, 61, 93), (1, 2, 1), (1, 2, 3), (1, 2, 4), (1, 2, 5), (3, 2, 5),
                                   (2, 33, 64)])
def test_kernel_shapes(B, H, W):
    """Smaller than a vector or a work-group; more than one work-group with an odd width (rows wrap inside a
    thread's four pixels); W in {1, 3, 4, 5} at H = 2 for the head and tail of the packed stores; images that
    share a thread's four pixels; W % 4 == 0 (the 16-byte loads) with more than one work-group per image."""
    f = field(B, H, W, seed=H * W)
    f[1:] *= 7.0
    close(kernel(dev(f)), O.flow_to_rgb(f), f"{B}x{H}x{W}")
    close(kernel(dev(f), rad_max=3.0, bgr=True), O.flow_to_rgb(f, rad_max=3.0, bgr=True), f"{B}x{H}x{W} fixed bgr")


def test_kernel_crop_of_padded_buffer():
    """2 x 37 x 53 as the crop (top=3, left=5) of a 48 x 64 buffer: odd offset, pitch != W, two images whose
    maxima differ by 10 x, and a surrounding filled with huge values and NaNs that must not be read."""
    g = gold()
    f = g["flows"][:2].copy()
    f[1] *= 10.0
    buf = np.full((2, 2, 48, 64), 1e30, np.float32)
    buf[:, :, ::2, ::3] = np.nan
    buf[:, :, 3:40, 5:58] = f
    fr = np.random.default_rng(5).integers(0, 256, (2, 3, 37, 53)).astype(np.float32)
    fbuf = np.full((2, 3, 48, 64), np.nan, np.float32)
    fbuf[:, :, 3:40, 5:58] = fr
    want = O.flow_to_rgb(f)
    m = O.rad_max_of(f)
    assert 5 < m[1] / m[0] < 20
    got = kernel(dev(buf), 37, 53, top=3, left=5)
    close(got, want, "crop (3,5) of 48x64")
    assert torch.equal(got, kernel(dev(f)))          # bit for bit what the dense call gives
    st = kernel(dev(buf), 37, 53, top=3, left=5, frame=dev(fbuf))
    assert torch.equal(st[:, :37], dev(fr.astype(np.uint8)).permute(0, 2, 3, 1)) and torch.equal(st[:, 37:], got)
    # an aligned crop of the same buffer takes the 16-byte loads: (top=2, left=4), 40 x 56
    b2 = field(2, 48, 64, seed=11)
    close(kernel(dev(b2), 40, 56, top=2, left=4), O.flow_to_rgb(b2[:, :, 2:42, 4:60]), "aligned crop (2,4) 40x56")


def test_kernel_graph_replay_is_bit_identical():
    """Both launches captured once and replayed on new inputs (a larger, then a smaller maximum): no state
    survives between replays, so each equals the eager call on the same input bit for bit."""
    from raft_optical_flow_amd import _lib as L
    B, H, W = 2, 37, 53
    fs = [dev(field(B, H, W, seed=s, scale=sc)) for s, sc in ((1, 4.0), (2, 40.0), (3, 0.5))]
    buf = fs[0].clone()
    out = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(L.load().raft_flow_viz_ws_bytes(B, H, W) // 4, device=DEV)

    def call():
        L.call("raft_flow_to_rgb", buf.data_ptr(), 2 * H * W, H * W, W, 0, 0, B, H, W, 0.0, 0.0, 0, None, 0, 0, 0,
               ws.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)

    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for f in fs[1:] + fs[:1] + fs[1:2]:
        buf.copy_(f)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, kernel(f))


# ---------------------------------------------------------------------------------------------
# stacking
# ---------------------------------------------------------------------------------------------

def test_stacking():
    f = field(2, 9, 13, seed=1)
    fr = np.random.default_rng(2).integers(0, 256, (2, 3, 9, 13)).astype(np.float32)
    fr[0, :, 0, :8] = np.array([0.0, 255.0, 255.6, -3.0, np.nan, 0.5, 1.5, 254.5], np.float32)
    fr[1, 1, 2, 3] = 1e9
    fr[1, 2, 2, 3] = -np.inf
    plain = kernel(dev(f))
    st = kernel(dev(f), frame=dev(fr))
    assert st.shape == (2, 18, 13, 3)
    assert torch.equal(st[:, 9:], plain)                                   # bottom: the unstacked call, bit for bit
    want = O.frame_bytes(fr)
    assert np.array_equal(want[0, 0, :8, 0], [0, 255, 255, 0, 0, 0, 2, 254])   # saturation, NaN, ties to even
    assert want[1, 2, 3, 1] == 255 and want[1, 2, 3, 2] == 0
    assert np.array_equal(st[:, :9].cpu().numpy(), want)                   # top: the frame's bytes exactly
    sb = kernel(dev(f), frame=dev(fr), bgr=True)
    assert torch.equal(sb, st.flip(-1))                                    # BGR reverses frame rows and colours


# ---------------------------------------------------------------------------------------------
# the Python forms
# ---------------------------------------------------------------------------------------------

def test_flow_to_image_forms():
    from raft_optical_flow_amd.utils import flow_viz as V
    g = gold()
    hwc = np.ascontiguousarray(g["flows"][1].transpose(1, 2, 0))
    a = V.flow_to_image(hwc)
    assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape == (37, 53, 3)
    close(a, g["img_flows"][1], "flow_to_image numpy")
    b = V.flow_to_image(torch.from_numpy(hwc))
    c = V.flow_to_image(torch.from_numpy(hwc).to(DEV))
    assert torch.is_tensor(b) and not b.is_cuda and c.is_cuda and b.dtype == c.dtype == torch.uint8
    assert np.array_equal(a, b.numpy()) and np.array_equal(a, c.cpu().numpy())
    assert np.array_equal(V.flow_to_image(hwc.astype(np.float64)), a)      # converted to float32 first
    close(V.flow_to_image(hwc, clip_flow=3.0), g["img_clip3"], "flow_to_image clip_flow")
    assert (V.flow_to_image(hwc, clip_flow=0.0) == 255).all()              # the reference: everything clipped to 0
    assert np.array_equal(V.flow_to_image(hwc, convert_to_bgr=True), a[..., ::-1])
    uv = g["uv"]
    d = V.flow_uv_to_colors(uv[0], uv[1])
    close(d, g["img_uv"], "flow_uv_to_colors numpy")
    assert np.array_equal(V.flow_uv_to_colors(uv[0], uv[1], convert_to_bgr=True), d[..., ::-1])
    assert np.array_equal(V.flow_uv_to_colors(torch.from_numpy(uv[0]).to(DEV), torch.from_numpy(uv[1]).to(DEV)
                                              ).cpu().numpy(), d)


def test_flow_to_rgb_strided_crop_and_bgr():
    from raft_optical_flow_amd.utils.flow_viz import flow_to_rgb
    up = dev(field(2, 48, 64, seed=9))
    up[1] *= 10
    frame = dev(np.random.default_rng(4).integers(0, 256, (2, 3, 48, 64)).astype(np.float32))
    crop = up[..., 3:-8, 5:-6]
    fcrop = frame[..., 3:-8, 5:-6]
    assert not crop.is_contiguous() and crop.shape == (2, 2, 37, 53)
    a = flow_to_rgb(crop)
    assert a.shape == (2, 37, 53, 3) and a.dtype == torch.uint8 and a.is_cuda
    assert torch.equal(a, flow_to_rgb(crop.contiguous()))
    close(a, O.flow_to_rgb(crop.cpu().numpy()), "flow_to_rgb strided crop")
    assert torch.equal(flow_to_rgb(crop, bgr=True), a.flip(-1))
    s = flow_to_rgb(crop, rad_max=5.0, frame=fcrop)
    assert torch.equal(s, flow_to_rgb(crop.contiguous(), rad_max=5.0, frame=fcrop.contiguous()))
    assert torch.equal(s[:, 37:], flow_to_rgb(crop, rad_max=5.0))
    assert torch.equal(s[:, :37], fcrop.permute(0, 2, 3, 1).to(torch.uint8))
    close(flow_to_rgb(crop, clip_flow=3.0), O.flow_to_rgb(crop.cpu().numpy(), clip_flow=3.0), "flow_to_rgb clip_flow")
    # one image of a batch (a batch stride that is not 2 * H * W) and a channel-swapped view (copied once)
    assert torch.equal(flow_to_rgb(up[1:]), flow_to_rgb(up)[1:])
    close(flow_to_rgb(up.flip(1)), O.flow_to_rgb(up.cpu().numpy()[:, ::-1]), "flow_to_rgb flipped channels")


# ---------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def small_model():
    from raft_optical_flow_amd import RAFT
    w = load_golden("raft_small_weights.npz")
    m = RAFT(argparse.Namespace(small=True, mixed_precision=False, alternate_corr=False))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return m.to(DEV).eval()


VH, VW = 60, 76


@functools.lru_cache(maxsize=None)
def video():
    """3 frames, uint8 [2,60,76,3]: 60 x 76 is padded to 64 x 80 (top 2, left 2).  The smallest frame of this
    kind the model takes: the 4-level correlation pyramid needs 8 x 8 at 1/8 resolution (36 x 52, padded to
    40 x 56, leaves 5 x 7 and an empty fourth level, which the reference rejects as well)."""
    from raft_optical_flow_amd.init import smooth_images
    fr = [smooth_images(2, VH, VW, seed=3, shift=(3.0 * k, -2.0 * k))[1] for k in range(3)]
    return tuple(f.permute(0, 2, 3, 1).contiguous().to(torch.uint8).to(DEV) for f in fr)


SEQ = (0, 1, 2, 1)   # the frames pushed: pair k is (frame SEQ[k], frame SEQ[k + 1])


def run_stream(graph, **kw):
    """Push SEQ; with the graph, the first pair runs eagerly, the second captures and replays, the third replays
    again.  Returns the three results and the plan's kernel names."""
    m = small_model()
    m.hip_graph = graph
    try:
        with m.stream(iters=3, **kw) as s:
            outs = [s.push(video()[i]) for i in SEQ]
            names = s.plan.kernel_names()
    finally:
        m.hip_graph = True
    torch.cuda.synchronize()
    assert outs[0] is None
    return outs[1:], names


def as_frame(u8):
    return u8.permute(0, 3, 1, 2).float()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_stream_rgb_equals_flow_to_rgb(graph):
    """rgb is flow_to_rgb(flow_up) of the same step, bit for bit: eager, and through the graph across two
    replays."""
    from raft_optical_flow_amd import FlowViz
    from raft_optical_flow_amd.utils.flow_viz import flow_to_rgb
    v = video()
    plain, names0 = run_stream(graph)
    outs, names = run_stream(graph, visualize="rgb")
    assert names == names0 + ["raft_flow_to_rgb"]
    for o, p in zip(outs, plain):
        assert isinstance(o, FlowViz) and isinstance(p, tuple) and not isinstance(p, FlowViz) and len(p) == 2
        assert torch.equal(o.flow_low, p[0]) and torch.equal(o.flow_up, p[1])   # the flow itself did not move
        assert o.rgb.shape == (2, VH, VW, 3) and o.rgb.dtype == torch.uint8
        assert torch.equal(o.rgb, flow_to_rgb(o.flow_up))
    assert not torch.equal(outs[0].rgb, outs[1].rgb)
    close(outs[1].rgb, O.flow_to_rgb(outs[1].flow_up.cpu().numpy()), "stream rgb vs oracle")
    # fixed scale, BGR and stacking: image1 of pair k is frame SEQ[k]
    outs, names = run_stream(graph, visualize="bgr", viz_rad_max=4.0, viz_stack=True)
    assert names == names0 + ["raft_flow_to_rgb"]
    for k, o in enumerate(outs):
        assert o.rgb.shape == (2, 2 * VH, VW, 3)
        assert torch.equal(o.rgb, flow_to_rgb(o.flow_up, rad_max=4.0, bgr=True, frame=as_frame(v[SEQ[k]])))
        assert torch.equal(o.rgb[:, :VH], v[SEQ[k]].flip(-1))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_stream_bidirectional_rgb(graph):
    from raft_optical_flow_amd import BidirectionalFlow, BidirectionalFlowViz
    from raft_optical_flow_amd.utils.flow_viz import flow_to_rgb
    v = video()
    plain, names0 = run_stream(graph, bidirectional=True)
    outs, names = run_stream(graph, bidirectional=True, visualize="rgb")
    assert names == names0 + ["raft_flow_to_rgb"] * 2
    assert BidirectionalFlowViz._fields == BidirectionalFlow._fields + ("rgb_fw", "rgb_bw")
    for o, p in zip(outs, plain):
        assert isinstance(o, BidirectionalFlowViz) and isinstance(p, BidirectionalFlow)
        assert all(torch.equal(a, b) for a, b in zip(o[:8], p))
        assert torch.equal(o.rgb_fw, flow_to_rgb(o.up_fw))
        assert torch.equal(o.rgb_bw, flow_to_rgb(o.up_bw))       # normalised by its own maximum
    # (were rgb_bw normalised by the forward maximum it would differ: the two maxima are not equal)
    o = outs[1]
    assert not np.array_equal(O.rad_max_of(o.up_fw.cpu().numpy()), O.rad_max_of(o.up_bw.cpu().numpy()))
    outs, _ = run_stream(graph, bidirectional=True, visualize="rgb", viz_rad_max=4.0, viz_stack=True)
    for k, o in enumerate(outs):
        assert torch.equal(o.rgb_fw, flow_to_rgb(o.up_fw, rad_max=4.0, frame=as_frame(v[SEQ[k]])))
        assert torch.equal(o.rgb_bw, flow_to_rgb(o.up_bw, rad_max=4.0, frame=as_frame(v[SEQ[k + 1]])))


def test_stream_default_is_unchanged_and_release():
    m = small_model()
    with m.stream(iters=3) as s0, m.stream(iters=3, visualize=None, viz_rad_max=None, viz_stack=False) as s1, \
            m.stream(iters=3, visualize="rgb") as s2:
        for f in video()[:2]:
            a, b, c = s0.push(f), s1.push(f), s2.push(f)
        assert type(a) is tuple and len(a) == 2 and type(b) is tuple and torch.equal(a[1], b[1])
        n0, n1 = s0.plan.kernel_names(), s1.plan.kernel_names()
        assert n0 == n1 and "raft_flow_to_rgb" not in n0
        assert n0[:2] == ["raft_stream_carry", "raft_ingest_frame"]
        assert s0.plan.rgb is None and s2.plan.rgb[0].shape == (2, VH, VW, 3)
        pl = s2.plan
    assert pl.rgb is None and pl.launches == []     # release() dropped the new buffers


@pytest.mark.parametrize("bidi", [False, True], ids=["uni", "bidi"])
def test_stream_range_guard_recolours_exact_flow(bidi):
    """fnet's head scaled so |fmap| > 2^15 (as test_gpu_stream.py's guard test): the step is flagged and re-run
    in exact fp32, and the image returned is that of the exact flow, not of the flagged step's."""
    import warnings
    from raft_optical_flow_amd import RAFT
    from raft_optical_flow_amd.utils.flow_viz import flow_to_rgb
    m = RAFT(argparse.Namespace(small=True, mixed_precision=False, alternate_corr=False))
    m.load_state_dict(small_model().state_dict())
    m.to(DEV).eval()
    with torch.no_grad():
        m.fnet.conv2.weight.mul_(20000.0)
        m.fnet.conv2.bias.mul_(20000.0)
    v = video()
    with torch.no_grad(), m.stream(iters=3, bidirectional=bidi, visualize="rgb", viz_stack=True) as s:
        assert s.plan is None and s.push(v[0]) is None
        assert m.range_guard == "fallback" and s.plan.guarded
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            o = s.push(v[1])
        assert len([x for x in w if "range guard" in str(x.message)]) == 1
        flagged = [t.clone() for t in s.plan.rgb]
    if bidi:
        assert torch.equal(o.rgb_fw, flow_to_rgb(o.up_fw, frame=as_frame(v[0])))
        assert torch.equal(o.rgb_bw, flow_to_rgb(o.up_bw, frame=as_frame(v[1])))
        assert not torch.equal(o.rgb_fw, flagged[0])
    else:
        assert torch.equal(o.rgb, flow_to_rgb(o.flow_up, frame=as_frame(v[0])))
        assert not torch.equal(o.rgb, flagged[0])


# ---------------------------------------------------------------------------------------------
# demo.py's call sequence through compat/
# ---------------------------------------------------------------------------------------------

DEMO = r'''
import sys
sys.path.append('core')
import argparse, io, json, os
import numpy as np
import torch
from PIL import Image
from raft import RAFT
from utils import flow_viz
from utils.utils import InputPadder
DEVICE = 'cuda'
g = np.load(os.path.join(os.environ['RAFT_GOLDEN'], 'raft_small_demo_0016_0017_i12.npz'))
w = np.load(os.path.join(os.environ['RAFT_GOLDEN'], 'raft_small_weights.npz'))
ckpt = os.path.join(os.environ['RAFT_TMP'], 'raft-small.pth')
torch.save({'module.' + k: torch.from_numpy(w[k]) for k in w.files}, ckpt)
def load_image(key):
    img = np.array(Image.open(io.BytesIO(g[key].tobytes()))).astype(np.uint8)
    img = torch.from_numpy(img).permute(2, 0, 1).float()
    return img[None].to(DEVICE)
def viz(img, flo):
    img = img[0].permute(1,2,0).cpu().numpy()
    flo = flo[0].permute(1,2,0).cpu().numpy()
    # map flow to rgb image
    flo = flow_viz.flow_to_image(flo)
    img_flo = np.concatenate([img, flo], axis=0)
    return img_flo
args = argparse.Namespace(model=ckpt, small=True, mixed_precision=False, alternate_corr=False)
model = torch.nn.DataParallel(RAFT(args))
model.load_state_dict(torch.load(args.model))
model = model.module
model.to(DEVICE)
model.eval()
with torch.no_grad():
    image1 = load_image('png1')
    image2 = load_image('png2')
    padder = InputPadder(image1.shape)
    image1, image2 = padder.pad(image1, image2)
    flow_low, flow_up = model(image1, image2, iters=20, test_mode=True)
    img_flo = viz(image1, flow_up)
np.savez(os.path.join(os.environ['RAFT_TMP'], 'demo_viz.npz'), img_flo=img_flo, flow_up=flow_up.cpu().numpy(),
         image1=image1.cpu().numpy())
print(json.dumps({'shape': list(img_flo.shape), 'dtype': str(img_flo.dtype)}))
'''


def test_demo_sequence_with_flow_viz(tmp_path):
    out = subprocess.run([sys.executable, "-c", DEMO], cwd=os.path.join(REPO, "compat"), capture_output=True,
                         text=True, timeout=200, env=dict(os.environ, RAFT_TMP=str(tmp_path), RAFT_GOLDEN=GOLDEN))
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    z = np.load(os.path.join(tmp_path, "demo_viz.npz"))
    up, img = z["flow_up"], z["img_flo"]
    H, W = up.shape[2:]
    assert r["shape"] == [2 * H, W, 3] and (H, W) == (440, 1024)
    assert np.array_equal(img[:H], z["image1"][0].transpose(1, 2, 0))     # demo.py stacks the float frame
    flo = img[H:]
    assert np.array_equal(flo, flo.astype(np.uint8))
    close(flo.astype(np.uint8)[None], O.flow_to_rgb(up), "demo.py sequence 440x1024")
