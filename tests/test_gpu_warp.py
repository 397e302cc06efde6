"""utils.warp_frame, utils.splat_density and RAFT.stream(warp=...) on the GPU.

The kernel tests hold raft_warp_frame and raft_splat_density to the fp64 restatements of their definitions in
test_warp_host.py (warp_reference, density_reference), within the fp32 bounds derived there, and to the
reference's own outputs (tests/golden/warp_reference.npz) within the reference's measured distance to fp64 plus
that bound.  The stream tests use test_gpu_stream.py's conventions and helpers (seeded weights, smooth_images
frames f0..f3, 128x192 and 123x181, ITERS = 4): what push returns is utils.warp_frame of the same step, bit for
bit, and the flow itself does not move."""
import itertools
import warnings

import numpy as np
import pytest
import torch

import test_gpu_stream as S
import test_warp_host as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ITERS = S.ITERS
MODES = ("zeros", "border")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(DEV)


def warp(frame, flow, padding="zeros", out_dtype=None):
    """utils.warp_frame -> (warped as numpy [B,C,H,W] whatever the layout, valid [B,H,W])."""
    from raft_optical_flow_amd.utils import warp_frame
    out, valid = warp_frame(frame, flow, padding=padding, out_dtype=out_dtype)
    torch.cuda.synchronize()
    B, H, W = flow.shape[0], flow.shape[2], flow.shape[3]
    want = out_dtype or frame.dtype
    assert out.dtype == want and valid.dtype == torch.bool and tuple(valid.shape) == (B, 1, H, W)
    if want == torch.uint8:
        assert tuple(out.shape) == (B, H, W, 3)
        out = out.permute(0, 3, 1, 2)
    else:
        assert tuple(out.shape) == (B, frame.shape[3] if frame.dtype == torch.uint8 else frame.shape[1], H, W)
    return out.cpu().numpy(), valid[:, 0].cpu().numpy()


def density(flow):
    from raft_optical_flow_amd.utils import splat_density
    out = splat_density(flow)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (flow.shape[0], 1) + tuple(flow.shape[2:])
    return out[:, 0].cpu().numpy()


def int_frame(B, C, H, W, seed=0):
    """Small-integer frame (0..63): halves and quarters of its values are exact in fp32."""
    rng = np.random.default_rng(seed + 100 * H + W + C)
    return rng.integers(0, 64, size=(B, C, H, W)).astype(np.float32)


def to_u8(frame):
    """float [B,3,H,W] -> uint8 [B,H,W,3] on the device."""
    return dev(R.u8_frame(frame), np.uint8)


def band(B, H, W, dx, dy):
    x, y = np.arange(W)[None, None, :], np.arange(H)[None, :, None]
    return np.broadcast_to((x + dx < 0) | (x + dx > W - 1) | (y + dy < 0) | (y + dy > H - 1), (B, H, W))


# ----------------------------------------------------------------------------- exact cases


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("C", [1, 3, 5])
def test_zero_flow_returns_the_frame(shape, C):
    B, H, W = shape
    fr = int_frame(B, C, H, W)
    z = torch.zeros(B, 2, H, W, device=DEV)
    for mode in MODES:
        out, valid = warp(dev(fr), z, mode)
        assert np.array_equal(out, fr) and valid.all()
    if C == 3:
        for mode, od in itertools.product(MODES, (None, torch.float32)):
            out, valid = warp(to_u8(fr), z, mode, od)
            assert np.array_equal(out, fr) and valid.all()
        out, _ = warp(dev(fr), z, "zeros", torch.uint8)
        assert np.array_equal(out, fr)


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("shift", [(2, 0), (0, -1), (-3, 2)])
def test_whole_pixel_shifts(shape, shift):
    """A whole-pixel shift: the shifted frame, zeros (or the replicated edge) in the band, valid = not the band."""
    B, H, W = shape
    sx, sy = shift
    fr = int_frame(B, 3, H, W)
    fl = torch.zeros(B, 2, H, W, device=DEV)
    fl[:, 0], fl[:, 1] = sx, sy
    bd = band(B, H, W, sx, sy)
    xs, ys = np.arange(W) + sx, np.arange(H) + sy
    clamped = fr[:, :, np.clip(ys, 0, H - 1), :][:, :, :, np.clip(xs, 0, W - 1)]
    want = {"zeros": np.where(bd[:, None], 0.0, clamped), "border": clamped}
    for mode in MODES:
        for frame, od in ((dev(fr), None), (to_u8(fr), None), (to_u8(fr), torch.float32), (dev(fr), torch.uint8)):
            out, valid = warp(frame, fl, mode, od)
            assert np.array_equal(out, want[mode]), (mode, frame.dtype, od)
            assert np.array_equal(valid, ~bd)
    assert int((~warp(dev(fr), fl)[1])[0, H // 2].sum()) == min(abs(sx), W)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_half_pixel_shifts_are_exact(shape):
    """Flow (0.5, -0.5) on a small-integer image: weights 1/2 and 1/4, every operation exact, so the fp32 result
    equals the fp64 one; the uint8 result is its rint (ties to even: quarters of integers do hit .5)."""
    B, H, W = shape
    fr = int_frame(B, 3, H, W)
    fl = torch.zeros(B, 2, H, W, device=DEV)
    fl[:, 0], fl[:, 1] = 0.5, -0.5
    for mode in MODES:
        d = R.warp_reference(fr, fl.cpu().numpy(), mode == "border")
        for frame in (dev(fr), to_u8(fr)):
            out, valid = warp(frame, fl, mode, torch.float32)
            assert np.array_equal(out.astype(np.float64), d["value"]) and np.array_equal(valid, d["valid"])
            out, _ = warp(frame, fl, mode, torch.uint8)
            assert np.array_equal(out.astype(np.float64), np.rint(d["value"]))
    assert (np.abs(d["value"] - np.floor(d["value"]) - 0.5) == 0).any()      # ties are exercised


def test_targets_on_the_last_column_and_row_read_no_neighbour():
    """Targets exactly on column W-1 / row H-1 are valid and take the edge value alone.  Flow and frame are crops
    at odd offsets of NaN-prefilled buffers: a tap beyond the crop would put a NaN in the output."""
    B, C, H, W = 1, 3, 6, 7
    fbuf = torch.full((B, 2, H + 3, W + 4), float("nan"), device=DEV)
    ibuf = torch.full((B, C, H + 3, W + 4), float("nan"), device=DEV)
    fl, fr = fbuf[:, :, 1:1 + H, 3:3 + W], ibuf[:, :, 1:1 + H, 3:3 + W]
    img = int_frame(B, C, H, W)
    fr.copy_(dev(img))
    x = torch.arange(W, device=DEV, dtype=torch.float32)[None, :].expand(H, W)
    y = torch.arange(H, device=DEV, dtype=torch.float32)[:, None].expand(H, W)
    fl[0, 0] = (W - 1) - x                            # every pixel targets column W-1 ...
    fl[0, 1] = torch.where(y < H - 1, 0.5, 0.0)       # ... half-way between two rows (its own on the last)
    fl[0, :, :, 2] = torch.stack([torch.full((H,), 1.5, device=DEV), (H - 1) - y[:, 0]])   # column 2: row H-1
    f = fl.cpu().numpy()
    for mode in MODES:
        d = R.warp_reference(img, f, mode == "border")
        assert d["valid"].all()
        out, valid = warp(fr, fl, mode)
        assert not np.isnan(out).any() and valid.all()
        assert np.array_equal(out.astype(np.float64), d["value"])
        out8, _ = warp(fr, fl, mode, torch.uint8)
        assert np.array_equal(out8.astype(np.float64), np.rint(d["value"]))
    # zeros mode one step further: the outside taps are not read either (they contribute 0, not NaN * 0)
    fl[0, 0] += 0.5
    fl[0, 1, H - 1] += 0.25
    for mode in MODES:
        out, valid = warp(fr, fl, mode)
        d = R.warp_reference(img, fl.cpu().numpy(), mode == "border")
        assert not np.isnan(out).any() and np.array_equal(out.astype(np.float64), d["value"])
        assert np.array_equal(valid, d["valid"]) and not valid[0, :, 0].any()


def test_zeros_keeps_partial_weights_border_clamps():
    """Positions in (-1, 0) and (W-1, W): zeros mode blends the inside tap with its weight, border mode clamps."""
    B, C, H, W = 1, 1, 4, 8
    img = int_frame(B, C, H, W) + 1.0
    fl = torch.zeros(B, 2, H, W, device=DEV)
    x = torch.arange(W, device=DEV, dtype=torch.float32)
    fl[0, 0, :2] = -x - 0.25                # rows 0, 1: x = -0.25
    fl[0, 0, 2:] = (W - 1) - x + 0.75       # rows 2, 3: x = W - 1 + 0.75
    out, valid = warp(dev(img), fl, "zeros")
    assert not valid.any()
    assert np.array_equal(out[0, 0, :2], np.broadcast_to(0.75 * img[0, 0, :2, :1], (2, W)))
    assert np.array_equal(out[0, 0, 2:], np.broadcast_to(0.25 * img[0, 0, 2:, -1:], (2, W)))
    out, valid = warp(dev(img), fl, "border")
    assert not valid.any()
    assert np.array_equal(out[0, 0, :2], np.broadcast_to(img[0, 0, :2, :1], (2, W)))
    assert np.array_equal(out[0, 0, 2:], np.broadcast_to(img[0, 0, 2:, -1:], (2, W)))
    fl2 = torch.zeros(B, 2, H, W, device=DEV)
    fl2[0, 1] = -torch.arange(H, device=DEV, dtype=torch.float32)[:, None] - 0.5     # y = -0.5
    out, _ = warp(dev(img), fl2, "zeros")
    assert np.array_equal(out[0, 0], np.broadcast_to(0.5 * img[0, 0, :1], (H, W)))
    out, _ = warp(dev(img), fl2, "border")
    assert np.array_equal(out[0, 0], np.broadcast_to(img[0, 0, :1], (H, W)))


@pytest.mark.parametrize("mode", MODES)
def test_non_finite_and_huge_flow(mode):
    """NaN, +-inf, 3e38 and +-2^30 components: output 0 and valid False in both modes; every other pixel is as
    the restatement says."""
    B, H, W = 2, 37, 53
    frame, flow = R.warp_case(B, H, W)
    flow = flow.copy()
    bad = [np.nan, np.inf, -np.inf, 3e38, -3e38, 2.0 ** 30, -2.0 ** 30]
    rng = np.random.default_rng(4)
    spots = []
    for k, v in enumerate(bad * 3):
        b, c, y, x = rng.integers(B), k % 2, rng.integers(H), rng.integers(W)
        flow[b, c, y, x] = v
        spots.append((b, y, x))
    d = R.warp_reference(frame, flow, mode == "border")
    for frame_t, od in ((dev(frame), None), (to_u8(frame), None), (dev(frame), torch.uint8)):
        out, valid = warp(frame_t, dev(flow), mode, od)
        for b, y, x in spots:
            assert np.all(out[b, :, y, x] == 0) and not valid[b, y, x]
        assert not np.isnan(out.astype(np.float64)).any()
    out, valid = warp(dev(frame), dev(flow), mode)
    assert np.all(np.abs(out.astype(np.float64) - d["value"]) <= d["bound"])
    assert np.array_equal(valid[d["margin"] != 0], d["valid"][d["margin"] != 0])
    assert len(set(spots)) > 15 and not d["valid"][tuple(zip(*spots))].any()


# ----------------------------------------------------------------------------- the random case


def check_random(shape, C, mode, in_u8, out_u8):
    B, H, W = shape
    frame, flow = R.warp_case(B, H, W, C)
    src = np.rint(frame) if in_u8 else frame
    d = R.warp_reference(src, flow, mode == "border")
    frame_t = to_u8(frame) if in_u8 else dev(frame)
    out, valid = warp(frame_t, dev(flow), mode, torch.uint8 if out_u8 else torch.float32)
    edge = d["margin"] != 0
    assert np.array_equal(valid[edge], d["valid"][edge])
    if not out_u8:
        ratio = float(np.max(np.abs(out.astype(np.float64) - d["value"]) / d["bound"]))
        print(f"{shape} C={C} {mode} {'u8' if in_u8 else 'f32'}->f32: worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0, ratio
        return ratio
    want = np.rint(np.clip(d["value"], 0.0, 255.0))
    safe = R.half_margin(d["value"]) > d["bound"]
    left_out = float((~safe).any(axis=1).mean())
    print(f"{shape} {mode} {'u8' if in_u8 else 'f32'}->u8: share within the bound of a half-integer {left_out:.2e}")
    assert left_out <= 0.01
    assert np.array_equal(out[safe].astype(np.float64), want[safe])
    assert np.all(np.abs(out.astype(np.float64) - want) <= 1.0)
    return 0.0


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_random_case_every_layout(shape, mode):
    """f32 output within the derived bound of fp64, elementwise; uint8 output equal to rint(fp64) wherever the
    margin to a half-integer exceeds the bound and within +-1 elsewhere; valid equal off the frame's edge."""
    for in_u8, out_u8 in itertools.product((False, True), (False, True)):
        check_random(shape, 3, mode, in_u8, out_u8)
    for C in (1, 5):
        check_random(shape, C, mode, False, False)


@pytest.mark.parametrize("name,mode", [("zeros", "zeros"), ("border", "border")])
def test_reference_fixture(name, mode):
    """|kernel - reference| <= the reference's own measured distance to fp64 + the kernel's derived bound:
    image_warp (zeros) and IFNET_m.warp (border) on the stored inputs."""
    g = np.load(R.GOLDEN)
    frame, flow = g["frame"], g["flow"]
    d = R.warp_reference(frame, flow, mode == "border")
    out, _ = warp(dev(frame), dev(flow), mode)
    diff = np.abs(out.astype(np.float64) - g["warp_" + name].astype(np.float64))
    allow = float(g["ref_dist_" + name]) + d["bound"]
    print(f"{name}: max |kernel - reference| = {diff.max():.3e} (reference's distance to fp64 "
          f"{float(g['ref_dist_' + name]):.3e}); max |kernel - fp64| = "
          f"{np.abs(out.astype(np.float64) - d['value']).max():.3e}")
    assert np.all(diff <= allow)


def test_strided_inputs_equal_dense_copies():
    """A channel-sliced frame, a flow cropped at (top, left) = (1, 3) and a transposed view (copied once) give
    what their dense copies give."""
    from raft_optical_flow_amd.utils import splat_density, warp_frame
    B, H, W = 2, 37, 53
    frame, flow = R.warp_case(B, H, W, 5)
    big = torch.full((B, 7, H, W), 7.0, device=DEV)
    big[:, 1:6] = dev(frame)
    fr = big[:, 1:6:2]                                  # channels 0, 2, 4 of the frame: a channel stride of 2 planes
    fbuf = torch.full((B, 2, H + 2, W + 5), float("nan"), device=DEV)
    fl = fbuf[:, :, 1:1 + H, 3:3 + W]
    fl.copy_(dev(flow))
    assert not fr.is_contiguous() and not fl.is_contiguous()
    frT = dev(frame[:, ::2].transpose(0, 1, 3, 2)).transpose(2, 3)      # unit stride along H, not W
    flT = dev(flow.transpose(0, 1, 3, 2)).transpose(2, 3)
    assert frT.stride(3) != 1 and torch.equal(frT, fr)
    for mode in MODES:
        want = warp_frame(fr.contiguous(), fl.contiguous(), padding=mode)
        for a, b in ((fr, fl), (frT, flT), (fr, flT)):
            got = warp_frame(a, b, padding=mode)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    want = splat_density(fl.contiguous())
    assert torch.equal(splat_density(fl), want) and torch.equal(splat_density(flT), want)


# ----------------------------------------------------------------------------- density


@pytest.mark.parametrize("shape", R.SHAPES)
def test_density_exact_cases(shape):
    """Zero flow: all ones.  Whole-pixel shifts: exactly 1 where a source lands, 0 in the band.  Every source
    onto one pixel: exactly H W there.  Fractional targets on the last column / row: the clamp puts both weights
    on the edge pixel.  Non-finite sources contribute nothing."""
    B, H, W = shape
    z = torch.zeros(B, 2, H, W, device=DEV)
    assert np.all(density(z) == 1.0)
    for sx, sy in ((2, 0), (0, -1), (-3, 2)):
        fl = z.clone()
        fl[:, 0], fl[:, 1] = sx, sy
        got = density(fl)
        assert np.array_equal(got, (~band(B, H, W, -sx, -sy)).astype(np.float32))
        assert np.array_equal(got.astype(np.float64), R.density_reference(fl.cpu().numpy())[0])
    x = torch.arange(W, device=DEV, dtype=torch.float32)[None, :]
    y = torch.arange(H, device=DEV, dtype=torch.float32)[:, None]
    fl = z.clone()
    fl[:, 0], fl[:, 1] = (W // 2) - x, (H // 3) - y
    got = density(fl)
    assert np.all(got[:, H // 3, W // 2] == H * W) and got.sum() == B * H * W
    fl = z.clone()
    fl[:, 0, :, W - 1] = 0.25
    fl[:, 1, H - 1, :] = 0.5
    assert np.all(density(fl) == 1.0)
    fl = z.clone()
    fl[0, 0, 0, 0] = float("nan")
    fl[0, 1, H - 1, W - 1] = float("-inf")
    fl[0, 0, H // 2, W // 2] = 3e38
    fl[0, 1, 1, 1] = 2.0 ** 30
    got = density(fl)
    want = np.ones((B, H, W), dtype=np.float32)
    for yy, xx in ((0, 0), (H - 1, W - 1), (H // 2, W // 2), (1, 1)):
        want[0, yy, xx] = 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_density_random_case_and_reproducibility(shape):
    """Within n (3 u + 2^-32) + u density of the fp64 sum, elementwise; two runs on the same input are bitwise
    equal (integer accumulation: no dependence on the order the adds arrive in)."""
    from raft_optical_flow_amd.utils import splat_density
    _, flow = R.warp_case(*shape)
    den, n, bound = R.density_reference(flow)
    fl = dev(flow)
    a, b = splat_density(fl), splat_density(fl)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    got = a[:, 0].cpu().numpy().astype(np.float64)
    ratio = float(np.max(np.abs(got - den) / np.maximum(bound, 1e-300)))
    print(f"{shape}: density worst error / bound = {ratio:.3f}, max density {den.max():.2f}, max taps {n.max()}")
    assert np.all(np.abs(got - den) <= bound)
    assert np.all(got[n == 0] == 0)
    if shape != R.SHAPES[0]:
        assert den.max() > 1.5 and (den < 0.5).any()        # pile-ups and holes both occur


# ----------------------------------------------------------------------------- streams


def seq(H, W, u8):
    f = S.frames(1, H, W)
    if u8:
        return [x.permute(0, 2, 3, 1).contiguous().to(torch.uint8).to(DEV) for x in f]
    return [x.to(DEV) for x in f]


def run(m, frames_, graph=True, **kw):
    """Push the frames through a fresh stream; with the graph the first pair runs eagerly, the second captures
    and replays, the third replays again.  Returns (results per pair, the plan's kernel names)."""
    m.hip_graph = graph
    try:
        with torch.no_grad(), m.stream(iters=ITERS, **kw) as s:
            outs = [s.push(f) for f in frames_]
            names = s.plan.kernel_names()
    finally:
        m.hip_graph = True
    torch.cuda.synchronize()
    assert outs[0] is None
    return outs[1:], names


@pytest.fixture(scope="module")
def model():
    return S.make_model()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("hw,u8", [((128, 192), False), ((123, 181), True), ((123, 181), False)],
                         ids=["128x192-f32", "123x181-u8", "123x181-f32"])
def test_stream_warp_equals_warp_frame(model, graph, hw, u8):
    """warped / valid of push are utils.warp_frame(current frame, flow_up, padding) of the same step, bit for bit;
    the flows equal those of the same stream opened without warp; the launch list grew by one raft_warp_frame."""
    from raft_optical_flow_amd import FlowWarp
    from raft_optical_flow_amd.utils import warp_frame
    fr = seq(*hw, u8)
    plain, names0 = run(model, fr, graph)
    assert "raft_warp_frame" not in names0
    for mode in MODES:
        outs, names = run(model, fr, graph, warp=mode)
        assert names == names0 + ["raft_warp_frame"]
        for k, (o, p) in enumerate(zip(outs, plain)):
            assert isinstance(o, FlowWarp) and type(p) is tuple and len(p) == 2
            assert torch.equal(o.flow_low, p[0]) and torch.equal(o.flow_up, p[1])
            want, wvalid = warp_frame(fr[k + 1], o.flow_up, padding=mode)
            assert o.warped.dtype == fr[0].dtype and o.warped.shape == fr[0].shape
            assert o.valid.dtype == torch.bool and tuple(o.valid.shape) == (1, 1) + hw
            assert torch.equal(o.warped, want) and torch.equal(o.valid, wvalid)
        assert not torch.equal(outs[0].warped, outs[1].warped)
        assert 0 < float(outs[1].valid.float().mean()) <= 1


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("hw,u8", [((128, 192), False), ((123, 181), True)], ids=["128x192-f32", "123x181-u8"])
def test_stream_bidirectional_warp(model, graph, hw, u8):
    """Both directions: warped_fw is the current frame by up_fw, warped_bw the previous frame by up_bw."""
    from raft_optical_flow_amd import BidirectionalFlow, BidirectionalFlowWarp
    from raft_optical_flow_amd.utils import warp_frame
    fr = seq(*hw, u8)[:3]
    plain, names0 = run(model, fr, graph, bidirectional=True)
    outs, names = run(model, fr, graph, bidirectional=True, warp="zeros")
    assert names == names0 + ["raft_warp_frame"] * 2
    for k, (o, p) in enumerate(zip(outs, plain)):
        assert isinstance(o, BidirectionalFlowWarp) and isinstance(p, BidirectionalFlow)
        assert all(torch.equal(a, b) for a, b in zip(o[:8], p))
        for got, gvalid, frame, up in ((o.warped_fw, o.valid_fw, fr[k + 1], o.up_fw),
                                       (o.warped_bw, o.valid_bw, fr[k], o.up_bw)):
            want, wvalid = warp_frame(frame, up, padding="zeros")
            assert got.dtype == fr[0].dtype and torch.equal(got, want) and torch.equal(gvalid, wvalid)
    outs, _ = run(model, fr[:2], graph, bidirectional=True, warp="border")
    o = outs[0]
    assert torch.equal(o.warped_bw, warp_frame(fr[0], o.up_bw, padding="border")[0])


def test_stream_warp_with_visualize_and_default_unchanged(model):
    """With visualize the new fields follow rgb; without warp the stream is what it was; release() drops the
    new buffers."""
    from raft_optical_flow_amd import BidirectionalFlowVizWarp, FlowVizWarp
    from raft_optical_flow_amd.utils import warp_frame
    from raft_optical_flow_amd.utils.flow_viz import flow_to_rgb
    fr = seq(123, 181, True)[:2]
    (plain,), names0 = run(model, fr)
    (same,), names1 = run(model, fr, warp=None)
    assert names0 == names1 and type(same) is tuple and S.equal(plain, same)
    (o,), names = run(model, fr, visualize="rgb", warp="border")
    assert names == names0 + ["raft_flow_to_rgb", "raft_warp_frame"]
    assert isinstance(o, FlowVizWarp) and torch.equal(o.rgb, flow_to_rgb(o.flow_up))
    want, wvalid = warp_frame(fr[1], o.flow_up, padding="border")
    assert torch.equal(o.warped, want) and torch.equal(o.valid, wvalid) and torch.equal(o.flow_up, plain[1])
    (o,), names = run(model, fr, bidirectional=True, visualize="rgb", warp="zeros")
    assert isinstance(o, BidirectionalFlowVizWarp) and names[-4:] == ["raft_flow_to_rgb"] * 2 + ["raft_warp_frame"] * 2
    assert torch.equal(o.warped_fw, warp_frame(fr[1], o.up_fw)[0])
    with torch.no_grad(), model.stream(iters=ITERS, warp="zeros") as s:
        s.push(fr[0])
        s.push(fr[1])
        pl = s.plan
        assert pl.warped[0].shape == fr[0].shape and pl.warp_valid[0].dtype == torch.uint8
    assert pl.warped is None and pl.warp_valid is None and pl.launches == []


def test_stream_warp_survives_reset_and_weight_change():
    from raft_optical_flow_amd.utils import warp_frame
    fr = seq(128, 192, False)
    m = S.make_model()
    with torch.no_grad(), m.stream(iters=ITERS, warp="zeros") as s:
        assert s.push(fr[0]) is None
        first = s.push(fr[1])
        s.reset()
        assert s.push(fr[1]) is None
        after = s.push(fr[2])
        m.update_block.gru.convz1.weight.mul_(1.5)         # the plan is rebuilt under the stream
        got = s.push(fr[3])
    for o, cur in ((first, fr[1]), (after, fr[2]), (got, fr[3])):
        want, wvalid = warp_frame(cur, o.flow_up)
        assert torch.equal(o.warped, want) and torch.equal(o.valid, wvalid)
    fresh, _ = run(m, fr[2:4], warp="zeros")               # built after the edit
    assert all(torch.equal(a, b) for a, b in zip(got, fresh[0]))


@pytest.mark.parametrize("bidi", [False, True], ids=["uni", "bidi"])
def test_stream_range_guard_warps_by_the_exact_flow(bidi):
    """fnet's head scaled so |fmap| > 2^15 (test_gpu_stream.py's guard test): the step is flagged and re-run in
    exact fp32, and the warp returned is that of the exact flow, not of the flagged step's."""
    from raft_optical_flow_amd.utils import warp_frame
    m = S.make_model()
    with torch.no_grad():
        m.fnet.conv2.weight.mul_(20000.0)
        m.fnet.conv2.bias.mul_(20000.0)
    fr = seq(123, 181, True)
    with torch.no_grad(), m.stream(iters=ITERS, bidirectional=bidi, warp="border") as s:
        assert s.push(fr[0]) is None
        assert m.range_guard == "fallback" and s.plan.guarded
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            o = s.push(fr[1])
        assert len([x for x in w if "range guard" in str(x.message)]) == 1
        flagged = [t.clone() for t in s.plan.warped]
    if bidi:
        for got, gvalid, frame, up in ((o.warped_fw, o.valid_fw, fr[1], o.up_fw),
                                       (o.warped_bw, o.valid_bw, fr[0], o.up_bw)):
            want, wvalid = warp_frame(frame, up, padding="border")
            assert got.dtype == torch.uint8 and torch.equal(got, want) and torch.equal(gvalid, wvalid)
        assert not torch.equal(o.warped_fw, flagged[0])
    else:
        want, wvalid = warp_frame(fr[1], o.flow_up, padding="border")
        assert o.warped.dtype == torch.uint8 and torch.equal(o.warped, want) and torch.equal(o.valid, wvalid)
        assert not torch.equal(o.warped, flagged[0])
