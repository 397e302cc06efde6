"""utils.resize_frame, utils.resize_flow and utils.InputScaler on the GPU.

The kernel tests hold raft_resize to the fp64 definition of tests/resize_oracle.py within the fp32 bounds derived
there (bilinear: eight roundings on the path of an output, ((1 + 4u)^2 - 1) T, 1.2e-4 on 0..255; area: one per
summed term and the division; a flow multiplier: two more), and to the reference's own InputScaler outputs
(tests/golden/resize_reference.npz) within the reference's recorded distance to fp64 plus that bound.  Exact
cases (identity, 2x of integers, constant flows), non-finite taps and strided inputs are bitwise.
"""
import functools

import numpy as np
import pytest
import torch

import resize_oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = [("bilinear", False), ("bilinear", True), ("area", False)]
MODE_IDS = ["bilinear", "bilinear-align", "area"]
# beyond the table of tests/resize_oracle.py: a row whose (2 d + 1) S passes 2^31 (the 64-bit coordinates, along x
# and along y; the second also has more rows than one pass of the grid takes), and an output row wider than the
# 1024 samples a work-group covers
EXTRA = [((1, 1, 40000), (1, 70001)), ((1, 40000, 2), (70001, 1)), ((1, 2, 300), (3, 1100))]
SHAPES = O.SHAPES + EXTRA
GUARD = 64   # elements kept behind a destination: they must stay as they were


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(DEV)


def raw_resize(src, size, mode="bilinear", align=False, out_u8=False, mul=(1.0, 1.0)):
    """raft_resize itself into a prefilled destination (float32: NaN; uint8: 0xA5) with a guard behind it.
    src: float32 [B,C,H,W] or uint8 [B,H,W,3] on the device.  Returns numpy [B,C,h,w] whatever the layout."""
    from raft_optical_flow_amd import _lib as L
    in_u8 = src.dtype == torch.uint8
    b, c, hs, ws = (src.shape[0], 3, src.shape[1], src.shape[2]) if in_u8 else src.shape
    h, w = size
    n = b * c * h * w
    if out_u8:
        buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    else:
        buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    strides = (0, 0, 0) if in_u8 else (src.stride(0), src.stride(1), src.stride(2))
    L.call("raft_resize", src.data_ptr(), L.FRAME_U8_NHWC if in_u8 else L.FRAME_F32_NCHW, *strides, 0, 0, b, c, hs, ws,
           buf.data_ptr(), L.FRAME_U8_NHWC if out_u8 else L.FRAME_F32_NCHW, h, w,
           L.RESIZE_AREA if mode == "area" else L.RESIZE_BILINEAR, L.RESIZE_ALIGN_CORNERS if align else 0,
           float(mul[0]), float(mul[1]), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    guard = host[n:]
    assert (guard == 0xA5).all() if out_u8 else np.isnan(guard).all(), "the guard behind the destination was written"
    out = host[:n]
    return O.nchw(out.reshape(b, h, w, 3)) if out_u8 else out.reshape(b, c, h, w)


def tolerance(mode, T, src_hw, size, mul=1.0, flow=False):
    if mode == "area":
        return O.tol_area(T, O.max_box(src_hw, size), mul, flow)
    return O.tol_bilinear(T, mul, flow)


def check_f32(got, ref, tol, what):
    assert not np.isnan(got).any(), f"{what}: an output element was not written"
    dist = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: max |kernel - fp64| = {dist:.3e} (bound {tol:.3e})")
    assert dist <= tol, what


def check_u8(got, ref, tol, what):
    """The rounded oracle, but where the oracle lies within tol of a tie: there the byte may differ by 1."""
    want = O.to_u8(ref)
    c = np.clip(ref, 0.0, 255.0)
    near_tie = np.abs(np.abs(c - np.floor(c)) - 0.5) <= tol
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{what}: {int((diff != 0).sum())} bytes differ, {int(near_tie.sum())} outputs lie within {tol:.1e} of a tie")
    assert (diff[~near_tie] == 0).all() and (diff <= 1).all(), what


# ----------------------------------------------------------------------------- random cases


@functools.lru_cache(maxsize=None)
def case(src, size, mode, align):
    """One seeded source per shape, its uint8 version, and their fp64 resizes: computed once, read only."""
    b, hs, ws = src
    v = O.seeded_frame(b, 5, hs, ws, seed=hs * 131 + ws)
    u8 = np.rint(v[:, :3]).astype(np.uint8)
    ref, ref_u8 = O.resize_ref(v, size, mode, align), O.resize_ref(u8, size, mode, align)
    for a in (v, u8, ref, ref_u8):
        a.setflags(write=False)
    return v, u8, ref, ref_u8


@pytest.mark.parametrize("mode,align", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("src,size", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{d[0]}x{d[1]}" for s, d in SHAPES])
def test_random_case_every_layout(src, size, mode, align):
    v, u8, ref, ref_u8 = case(src, size, mode, align)
    tol = tolerance(mode, 255.0, src[1:], size)
    for C in (1, 3, 5):
        got = raw_resize(dev(v[:, :C]), size, mode, align)
        check_f32(got, ref[:, :C], tol, f"float32 C={C} -> float32")
    check_u8(raw_resize(dev(v[:, :3]), size, mode, align, out_u8=True), ref[:, :3], tol, "float32 -> uint8")
    u8_dev = dev(O.nhwc(u8), np.uint8)
    check_f32(raw_resize(u8_dev, size, mode, align), ref_u8, tol, "uint8 -> float32")
    check_u8(raw_resize(u8_dev, size, mode, align, out_u8=True), ref_u8, tol, "uint8 -> uint8")


@pytest.mark.parametrize("mode,align", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("src,size", O.SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{d[0]}x{d[1]}" for s, d in O.SHAPES])
def test_flow_multipliers(src, size, mode, align):
    """resize_flow: channel 0 times w / W, channel 1 times h / H, each ratio rounded to fp32 once."""
    from raft_optical_flow_amd.utils import resize_flow, resize_frame
    b, hs, ws = src
    fl = O.seeded_flow(b, hs, ws, seed=hs + ws)
    m0, m1 = O.flow_muls((hs, ws), size)
    ref = O.resize_ref(fl, size, mode, align, m0, m1)
    got = resize_flow(dev(fl), size, mode, align)
    assert got.dtype == torch.float32 and tuple(got.shape) == (b, 2) + tuple(size)
    got = got.cpu().numpy()
    for c, m in ((0, m0), (1, m1)):
        check_f32(got[:, c], ref[:, c], tolerance(mode, 20.0, (hs, ws), size, m, True), f"flow channel {c} (x {m:.4f})")
    plain = resize_frame(dev(fl), size, mode, align).cpu().numpy()       # the same launch without the multipliers
    assert np.array_equal(got[:, 0], plain[:, 0] * np.float32(m0)) and np.array_equal(got[:, 1], plain[:, 1] * np.float32(m1))
    raw = raw_resize(dev(fl), size, mode, align, mul=(m0, m1))
    assert np.array_equal(raw, got)


def test_resize_frame_layouts_and_dtypes():
    from raft_optical_flow_amd.utils import resize_frame
    v, u8, ref, ref_u8 = case((2, 37, 53), (19, 27), "bilinear", False)
    f32, u8d = dev(v[:, :3]), dev(O.nhwc(u8), np.uint8)
    a = resize_frame(f32, (19, 27))
    assert a.dtype == torch.float32 and tuple(a.shape) == (2, 3, 19, 27)
    assert np.array_equal(a.cpu().numpy(), raw_resize(f32, (19, 27)))
    b = resize_frame(u8d, (19, 27))
    assert b.dtype == torch.uint8 and tuple(b.shape) == (2, 19, 27, 3)
    assert np.array_equal(O.nchw(b.cpu().numpy()), raw_resize(u8d, (19, 27), out_u8=True))
    c = resize_frame(u8d, (19, 27), out_dtype=torch.float32)
    assert c.dtype == torch.float32 and np.array_equal(c.cpu().numpy(), raw_resize(u8d, (19, 27)))
    d = resize_frame(f32, (19, 27), out_dtype=torch.uint8)
    assert d.dtype == torch.uint8 and np.array_equal(O.nchw(d.cpu().numpy()), raw_resize(f32, (19, 27), out_u8=True))
    five = resize_frame(dev(v), [19, 27], mode="area")
    assert tuple(five.shape) == (2, 5, 19, 27)


# ----------------------------------------------------------------------------- bitwise cases


@pytest.mark.parametrize("align", [False, True])
def test_identity_returns_the_input(align):
    from raft_optical_flow_amd.utils import resize_flow, resize_frame
    v = dev(O.seeded_frame(2, 5, 5, 7, seed=4))
    assert torch.equal(resize_frame(v, (5, 7), align_corners=align), v)
    u8 = dev(np.random.default_rng(5).integers(0, 256, size=(2, 5, 7, 3)), np.uint8)
    assert torch.equal(resize_frame(u8, (5, 7), align_corners=align), u8)
    fl = dev(O.seeded_flow(2, 5, 7))
    assert torch.equal(resize_flow(fl, (5, 7), align_corners=align), fl)       # both multipliers are 1.0
    if not align:
        assert torch.equal(resize_frame(v, (5, 7), mode="area"), v)


@pytest.mark.parametrize("hw", [(64, 96), (6, 10), (2, 2)])
def test_half_size_of_integers_is_the_block_mean(hw):
    """2x down, align_corners=False: every weight is exactly 1/2, so integer frames give the exact mean of each
    2 x 2 block, and bilinear equals area bit for bit."""
    from raft_optical_flow_amd.utils import resize_frame
    H, W = hw
    v = np.random.default_rng(H + W).integers(0, 256, size=(1, 3, H, W)).astype(np.float32)
    want = v.reshape(1, 3, H // 2, 2, W // 2, 2).sum(axis=(3, 5)) / np.float32(4)          # exact in fp32
    bil = resize_frame(dev(v), (H // 2, W // 2))
    area = resize_frame(dev(v), (H // 2, W // 2), mode="area")
    assert np.array_equal(bil.cpu().numpy(), want) and torch.equal(bil, area)
    u8 = dev(O.nhwc(v), np.uint8)
    assert np.array_equal(O.nchw(resize_frame(u8, (H // 2, W // 2)).cpu().numpy()), O.to_u8(want.astype(np.float64)))


@pytest.mark.parametrize("mode", ["bilinear", "area"])
def test_constant_flow_doubles_at_twice_the_size(mode):
    """align_corners=False at 2x: the weights are quarters (up) and halves (down), so a constant stays exact and
    the multiplier 2.0 (0.5 on the way back) is all that happens to it."""
    from raft_optical_flow_amd.utils import resize_flow
    align = False
    fl = torch.empty(2, 2, 17, 23, device=DEV)
    fl[:, 0], fl[:, 1] = 3.0, -7.0
    up = resize_flow(fl, (34, 46), mode, align)
    assert torch.equal(up[:, 0], torch.full_like(up[:, 0], 6.0)) and torch.equal(up[:, 1], torch.full_like(up[:, 1], -14.0))
    down = resize_flow(up, (17, 23), mode, align)
    assert torch.equal(down, fl)


# ----------------------------------------------------------------------------- non-finite input


@pytest.mark.parametrize("size", [(19, 27), (74, 106), (37, 53)], ids=["down", "up", "identity"])
@pytest.mark.parametrize("mode,align", MODES, ids=MODE_IDS)
def test_non_finite_taps_spread_as_the_formula_says(mode, align, size):
    """A NaN and an Inf in the source reach exactly the outputs whose taps include them, weight 0 or not."""
    v = O.seeded_frame(1, 2, 37, 53, seed=9).copy()
    nan_at, inf_at = (11, 20), (30, 41)
    v[0, 0, nan_at[0], nan_at[1]] = np.nan
    v[0, 1, inf_at[0], inf_at[1]] = np.inf
    ref = O.resize_ref(v, size, mode, align)
    got = raw_resize(dev(v), size, mode, align)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref))
    assert not np.isneginf(got).any()
    fin = np.isfinite(ref)
    assert float(np.abs(got[fin] - ref[fin]).max()) <= tolerance(mode, 255.0, (37, 53), size)
    # the same set from the taps themselves
    if mode == "area":
        ylo, yhi = O.box_coords(size[0], 37)
        xlo, xhi = O.box_coords(size[1], 53)
        rows = lambda y: np.array([a <= y < b for a, b in zip(ylo, yhi)])            # noqa: E731
        cols = lambda x: np.array([a <= x < b for a, b in zip(xlo, xhi)])            # noqa: E731
    else:
        y0, y1, _, _ = O.lin_coords(size[0], 37, align)
        x0, x1, _, _ = O.lin_coords(size[1], 53, align)
        rows = lambda y: (np.array(y0) == y) | (np.array(y1) == y)                   # noqa: E731
        cols = lambda x: (np.array(x0) == x) | (np.array(x1) == x)                   # noqa: E731
    for c, (y, x) in ((0, nan_at), (1, inf_at)):
        touched = rows(y)[:, None] & cols(x)[None, :]
        assert touched.any() and np.array_equal(~np.isfinite(got[0, c]), touched)


# ----------------------------------------------------------------------------- strides


@pytest.mark.parametrize("mode,align", MODES, ids=MODE_IDS)
def test_strided_inputs_equal_dense_copies(mode, align):
    from raft_optical_flow_amd import InputPadder
    from raft_optical_flow_amd.utils import resize_flow, resize_frame
    big = dev(O.seeded_frame(2, 4, 50, 70, seed=2))
    crop = big[:, 1:4, 6:43, 9:62]                                  # a 2 x 3 x 37 x 53 crop, every stride its own
    assert not crop.is_contiguous()
    for size in ((19, 27), (40, 56)):
        assert torch.equal(resize_frame(crop, size, mode, align), resize_frame(crop.contiguous(), size, mode, align))
        assert torch.equal(resize_frame(crop, size, mode, align, out_dtype=torch.uint8),
                           resize_frame(crop.contiguous(), size, mode, align, out_dtype=torch.uint8))
    padder = InputPadder((2, 2, 37, 53))
    padded = padder.pad(dev(O.seeded_flow(2, 37, 53)))[0]           # [2,2,40,56]: a padded flow_up
    view = padder.unpad(padded)
    assert tuple(view.shape) == (2, 2, 37, 53) and not view.is_contiguous()
    assert torch.equal(resize_flow(view, (74, 106), mode, align), resize_flow(view.contiguous(), (74, 106), mode, align))


# ----------------------------------------------------------------------------- the reference's outputs


FIXTURE_KEYS = [(n, w, t) for n in ("s19x27", "s40x56") for w, t in (("frame", "fill"), ("flow", "fill"), ("flow", "unfill"))]


@pytest.mark.parametrize("name,what,tag", FIXTURE_KEYS, ids=["-".join(k) for k in FIXTURE_KEYS])
def test_reference_fixture(name, what, tag):
    """The kernel, and InputScaler.fill / unfill, lie within (the reference's recorded distance to fp64 + the
    derived fp32 bound) of what the reference's InputScaler returned."""
    from raft_optical_flow_amd.utils import InputScaler, resize_flow, resize_frame
    g = load_golden("resize_reference.npz")
    size = tuple(int(v) for v in g[name + "_size"])
    flow = what == "flow"
    key = f"{name}_{what}_{tag}"
    src = g[what] if tag == "fill" else g[f"{name}_{what}_fill"]
    tgt = size if tag == "fill" else (37, 53)
    want, stored = g[key].astype(np.float64), float(g["ref_dist_" + key])
    T = float(np.abs(src).max())
    tols = [tolerance("bilinear", T, src.shape[-2:], tgt, m, True) for m in O.flow_muls(src.shape[-2:], tgt)] if flow \
        else [tolerance("bilinear", T, src.shape[-2:], tgt)] * 3
    scaler = InputScaler((2, 3, 37, 53), stride=8) if name == "s40x56" else InputScaler((37, 53), size=size)
    assert (scaler.tgt_height, scaler.tgt_width) == size
    outs = {"kernel": (resize_flow if flow else resize_frame)(dev(src), tgt),
            "InputScaler": getattr(scaler, tag)(dev(src), is_flow=flow),
            "InputScaler, CPU tensor, 5 dims": getattr(scaler, tag)(torch.from_numpy(src)[None], is_flow=flow)[0]}
    assert outs["InputScaler, CPU tensor, 5 dims"].device.type == "cpu"
    for who, got in outs.items():
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape
        for c in range(got.shape[1]):
            dist = float(np.abs(got[:, c] - want[:, c]).max())
            print(f"{key} channel {c}, {who}: max |ours - reference| = {dist:.3e} (bound {stored:.3e} + {tols[c]:.3e})")
            assert dist <= stored + tols[c]
    assert np.array_equal(outs["kernel"].cpu().numpy(), outs["InputScaler"].cpu().numpy())


def test_input_scaler_round_trip_and_modes():
    from raft_optical_flow_amd.utils import InputScaler, resize_frame
    v = O.seeded_frame(2, 3, 37, 53, seed=6)
    for mode, align in MODES:
        sc = InputScaler(v.shape, scale_factor=0.5, interpolation_mode=mode, interpolation_align_corners=align)
        small = sc.fill(dev(v))
        assert tuple(small.shape) == (2, 3, 18, 26)
        assert torch.equal(small, resize_frame(dev(v), (18, 26), mode, align))
        back = sc.unfill(small)
        assert torch.equal(back, resize_frame(small, (37, 53), mode, align))
        ref = O.resize_ref(small.cpu().numpy(), (37, 53), mode, align)
        check_f32(back.cpu().numpy(), ref, tolerance(mode, 255.0, (18, 26), (37, 53)), f"unfill of a frame, {mode}")
    half = InputScaler(v.shape, size=(19, 27)).fill(dev(v).double())          # another float dtype comes back as it came
    assert half.dtype == torch.float64 and tuple(half.shape) == (2, 3, 19, 27)
