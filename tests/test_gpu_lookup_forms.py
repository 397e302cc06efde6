"""The all-pairs lookups' instantiations, layouts and rare paths against tests/lookup_oracle.py.

Every test runs a lookup on a pyramid the test wrote itself (lookup_oracle.tile_levels: INDEPENDENT
random levels, so reading another level, another corner or another channel order is an O(1) error)
and compares every tap with lookup_oracle.lookup_ref: the reference's fp32 sample positions, the
four-corner blend in fp64.

Bound of a plain lookup tap (lookup_oracle.tap_check): |got - ref| <= 8 * 2^-24 * cmax, cmax the
largest |corner| the tap read, NaN exactly where the reference has NaN.  1 - t, the weight product and
the value product are one rounding each, plus three additions: <= 6 * 2^-24 * cmax to first order; 8
covers the kernels' fused multiply-add form and the deferred / generic paths' four-product form.
The fused kernel's taps (recovered through a signed selection weight, see _fused_taps) add
u * |ref| + 2^-24 for the rounding of the tap to the conv's operand type: u = 2^-20 (f16x3: the split
drops at most 2^-22 relative), 2^-11 (f16), 2^-8 (bf16); 2^-24 absolute for f16's subnormal range.
Measured worst ratios |err| / (2^-24 * cmax) per kernel form: DESIGN.md.

Every written buffer lies inside a sentinel with guard rows; columns past ntap of a wider row,
columns 2.. of a flow row and the guards must come back untouched.  flow_out is compared bit for
bit with coords - grid in fp32.

Kernel forms (corr_pyramid.hip raft_corr_lookup's dispatch): radius 1..4 run
corr_lookup_kernel<R, LMAX>, LMAX = 4 for <= 4 levels, else 6; R = 4 with <= 4 levels and at most
16384 query pixels its scalar-interval window form (SCAL), more pixels the VALU form; any other
radius corr_lookup_generic_kernel."""
import functools

import numpy as np
import pytest
import torch

import lookup_oracle as LO
from test_gpu_lookup_conv import pack_lookup_conv_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = LO.SENTINEL
G = 4  # guard rows


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()
    yield
    for cached in (_pyramid, _coords, _ref):  # the shared pyramids and references: not kept for later modules
        cached.cache_clear()
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- shared data (never modified)


@functools.lru_cache(maxsize=None)
def _pyramid(B, H, W, L):
    """(pyramid buffer on the device, the levels on the host) of independent N(0, 1) levels, generated
    on the device from a seed.  The first L' levels are the pyramid of a lookup with L' < L levels."""
    from raft_optical_flow_amd import kernels as K
    gd = torch.Generator(device=DEV).manual_seed(1000 * B + 10 * H + W)
    levels = [torch.randn(B * H * W, h, w, generator=gd, device=DEV) for h, w in LO.level_dims(H, W, L)]
    pyr = LO.tile_levels(levels, B, H, W)
    assert pyr.numel() == K.pyramid_floats(B, H, W, L)
    return pyr, [lv.cpu().numpy() for lv in levels]


@functools.lru_cache(maxsize=None)
def _coords(kind, B, H, W):
    if kind == "matrix":
        return LO.matrix_coords(B, H, W, seed=7)
    if kind == "deferred":
        return LO.deferred_set(B, H, W)
    assert kind == "far"
    rng = np.random.default_rng(9)
    return (LO.grid_xy(B, H, W) + rng.normal(0, 40.0, (B * H * W, 2))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _ref(kind, B, H, W, Lmax, L, r):
    _, levels = _pyramid(B, H, W, Lmax)
    return LO.lookup_ref(levels[:L], _coords(kind, B, H, W), r)


def _form(B, H, W, L, r):
    if r < 1 or r > 4:
        return "generic"
    if L > 4:
        return f"R{r}-LMAX6"
    return f"R{r}-LMAX4-" + ("scalar" if r == 4 and B * H * W <= 16384 else "valu")


def _buf(rows, ld):
    whole = torch.full((rows + 2 * G, ld), SENT, device=DEV)
    return whole, whole[G:G + rows]


def _guards_ok(whole, rows, used):
    return bool((whole[:G] == SENT).all() and (whole[G + rows:] == SENT).all() and (whole[G:G + rows, used:] == SENT).all())


def _lookup(pyr, B, H, W, L, r, coords, cl=0, ol=0, pad=0, flow_ld=0, flag=None):
    """raft_corr_lookup with coords layout cl, out layout ol, out_ld = ntap + pad, flow rows of flow_ld
    floats (0: no flow_out); returns (taps [N, ntap], flow [N, 2] or None) on the host, after checking
    that nothing but the taps / the two flow columns was written."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    N, P = B * H * W, H * W
    ntap = L * (2 * r + 1) ** 2
    c = torch.from_numpy(coords).to(DEV)
    if cl == 1:
        c = c.view(B, P, 2).permute(0, 2, 1).contiguous()
    if ol == 0:
        whole, out = _buf(N, ntap + pad)
    else:
        whole = torch.full((B * ntap * P + 2 * G * 64,), SENT, device=DEV)
        out = whole[G * 64:G * 64 + B * ntap * P]
    fwhole, flow = _buf(N, flow_ld) if flow_ld else (None, None)
    _lib.call("raft_corr_lookup", pyr.data_ptr(), B, H, W, L, r, c.data_ptr(), cl, out.data_ptr(), ntap + pad, ol,
              flow.data_ptr() if flow_ld else None, flow_ld, flag.data_ptr() if flag is not None else None,
              K.stream_handle())
    torch.cuda.synchronize()
    if ol == 0:
        assert _guards_ok(whole, N, ntap), "wrote past the taps of a row or into the guard rows"
        taps = out[:, :ntap]
    else:
        assert bool((whole[:G * 64] == SENT).all() and (whole[-G * 64:] == SENT).all())
        taps = out.view(B, ntap, P).permute(0, 2, 1).reshape(N, ntap)
    if flow_ld:
        assert _guards_ok(fwhole, N, 2), "wrote past the two flow columns or into the guard rows"
    return taps.cpu().numpy(), (flow[:, :2].cpu().numpy() if flow_ld else None)


def _flow_ref(coords, B, H, W):
    with np.errstate(invalid="ignore"):
        return coords - LO.grid_xy(B, H, W)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _assert_taps(got, ref, cmax, r, what, u=0.0, abs_term=0.0, only=None):
    bad, ratio = LO.tap_check(got, ref, cmax, u, abs_term)
    if only is not None:
        assert not (bad & only).any(), f"{what}, deferred taps only: " + LO.describe_bad(bad & only, got, ref, cmax,
                                                                                        (2 * r + 1) ** 2)
    assert not bad.any(), f"{what}: " + LO.describe_bad(bad, got, ref, cmax, (2 * r + 1) ** 2)
    print(f"LOOKUP-RATIO {what}: worst |err| / (2^-24 cmax) = {ratio:.3f}, worst |err| / bound = "
          f"{LO.bound_fraction(got, ref, cmax, u, abs_term):.3f}")
    return ratio


# ----------------------------------------------------------------------------- a. the instantiation matrix

S, M, V = (2, 17, 21, 4), (1, 64, 72, 6), (47, 17, 21, 4)   # (B, H, W, Lmax): ragged at every level; 6 levels; > 16384 px
# (shape, L, r, coords layout, out layout, out_ld - ntap, flow_ld)
MATRIX = (
    [(S, 4, r, 0, 0, 0, 0) for r in (1, 2, 3, 4)] +
    [(S, L, r, 0, 0, 0, 0) for L in (1, 2, 3) for r in (4, 2)] +
    [(M, L, r, 0, 0, 0, 0) for L in (5, 6) for r in (1, 2, 3, 4)] +
    [(S, 1, 0, 0, 0, 0, 0), (S, 4, 0, 0, 0, 0, 0), (S, 4, 5, 0, 0, 0, 0), (S, 1, 7, 0, 0, 0, 0), (S, 4, 7, 0, 0, 0, 0),
     (M, 6, 0, 0, 0, 0, 0), (M, 6, 5, 0, 0, 0, 0), (M, 6, 7, 0, 0, 0, 0)] +
    # layouts, leading dimensions and flow_out on R = 4 / L = 4 and a generic radius; ntap = 243 at an
    # aligned out_ld (L = 3, r = 4: the row store without 16-B vectors); R = 1 at 6 levels
    [(S, 4, r, cl, ol, pad, fl) for r in (4, 5)
     for cl, ol, pad, fl in ((1, 1, 0, 2), (1, 0, 4, 4), (0, 0, 1, 2), (0, 1, 0, 4), (0, 0, 0, 4))] +
    [(S, 3, 4, 0, 0, 1, 4), (S, 3, 4, 1, 0, 5, 2), (M, 6, 1, 1, 1, 0, 2), (M, 5, 4, 0, 0, 4, 4)] +
    # the VALU window form of R = 4 (more than 16384 query pixels), NHWC as the forward and NCHW
    [(V, 4, 4, 0, 0, 0, 4), (V, 4, 4, 1, 1, 0, 0)]
)


def _mid(c):
    (B, H, W, _), L, r, cl, ol, pad, fl = c
    return f"{B}x{H}x{W}-L{L}-r{r}-{_form(B, H, W, L, r)}-c{cl}o{ol}-ld+{pad}-flow{fl}"


@pytest.mark.parametrize("case", MATRIX, ids=_mid)
def test_instantiation_matrix(case):
    """One launch per case on a small map: every (R, LMAX) instantiation raft_corr_lookup dispatches,
    level counts 1..6 (levels past L are duplicates of the last in the kernel's arguments), the generic
    kernel at r = 0, 5, 7, both coords / out layouts, out_ld in {ntap, ntap + 4, ntap + 1}, flow rows of
    2 and 4 floats.  Coordinates: grid + N(0, 3), one image (a quarter of a single image) uniform over
    [-40, size + 40]: windows hang off every edge and lie fully outside."""
    (B, H, W, Lmax), L, r, cl, ol, pad, fl = case
    pyr, _ = _pyramid(B, H, W, Lmax)
    coords = _coords("matrix", B, H, W)
    ref, cmax = _ref("matrix", B, H, W, Lmax, L, r)
    got, flow = _lookup(pyr, B, H, W, L, r, coords, cl, ol, pad, fl)
    _assert_taps(got, ref, cmax, r, _mid(case))
    if fl:
        assert _same(flow, _flow_ref(coords, B, H, W))


# ----------------------------------------------------------------------------- c. the fused kernel's taps


def _fused_taps(pyr, B, H, W, coords, prec, flags=None):
    """raft_corr_lookup_conv never writes its correlation rows: recover them with a convc1 weight that is
    a signed selection -- output channel j = +tap[k0 + j], channel 128 + j = -tap[k0 + j], zero bias, so
    relu(v) - relu(-v) = v exactly -- in three launches, k0 = 0, 128, 196.  Returns (taps [N, 324],
    flow [N, 2], the three flags of the last launch)."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    N, ntap = B * H * W, 324
    rng = np.random.default_rng(3)
    wf = (rng.standard_normal((128, 2, 7, 7)) * 0.1).astype(np.float32)
    bf = np.zeros(128, np.float32)
    c = torch.from_numpy(coords).to(DEV)
    taps = np.zeros((N, ntap), np.float32)
    for k0 in (0, 128, 196):
        wc = np.zeros((256, ntap), np.float32)
        j = np.arange(128)
        wc[j, k0 + j] = 1.0
        wc[128 + j, k0 + j] = -1.0
        pc, frag, pf, ffrag = pack_lookup_conv_weights(wc, np.zeros(256, np.float32), wf, bf, prec)
        c1w, c1 = _buf(N, 260)
        f1w, f1 = _buf(N, 132)
        fww, flow = _buf(N, 4)
        fl = torch.zeros(3, dtype=torch.int32, device=DEV) if flags is None else flags
        fp = fl.data_ptr()
        _lib.call("raft_corr_lookup_conv", pyr.data_ptr(), B, H, W, 4, 4, c.data_ptr(), flow.data_ptr(), 4, fp,
                  _lib.PRECISIONS[prec], frag.data_ptr(), pc.bias.data_ptr(), 256, c1.data_ptr(), 260, fp + 4,
                  ffrag.data_ptr(), pf.bias.data_ptr(), 128, 7, f1.data_ptr(), 132, fp + 8, K.stream_handle())
        torch.cuda.synchronize()
        assert _guards_ok(c1w, N, 256) and _guards_ok(f1w, N, 128) and _guards_ok(fww, N, 2)
        o = c1.cpu().numpy()
        assert (np.isnan(o[:, :256]) | (o[:, :256] >= 0)).all()
        taps[:, k0:k0 + 128] = o[:, :128] - o[:, 128:256]
    return taps, flow[:, :2].cpu().numpy(), fl.cpu().tolist()


U_PREC = {"f16x3": 2.0 ** -20, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}


def _check_fused(kind, B, H, W, prec):
    pyr, _ = _pyramid(B, H, W, 4)
    coords = _coords(kind, B, H, W)
    ref, cmax = _ref(kind, B, H, W, 4, 4, 4)
    assert not np.isnan(ref).any()      # (a NaN tap would spread over its whole convc1 row)
    taps, flow, flags = _fused_taps(pyr, B, H, W, coords, prec)
    only = LO.off_patch_taps(coords, LO.level_dims(H, W, 4), 4) if kind == "deferred" else None
    _assert_taps(taps, ref, cmax, 4, f"lookup_conv-{prec}-{kind}-{B}x{H}x{W}", U_PREC[prec], 2.0 ** -24, only)
    assert _same(flow, _flow_ref(coords, B, H, W))
    assert flags[0] == 0


@pytest.mark.parametrize("kind,B,H,W", [("deferred", 1, 55, 128), ("matrix", 2, 17, 21), ("far", 1, 19, 35)])
@pytest.mark.parametrize("prec", ["f16x3", "f16", "bf16"])
def test_fused_taps_vs_oracle(kind, B, H, W, prec):
    """raft_corr_lookup_conv's own taps against the oracle (until now only against raft_corr_lookup, the
    same lookup code): config 2's grid with the deferred-path coordinates, a ragged small map with windows
    off every edge, and coordinates N(0, 40) far off the map."""
    _check_fused(kind, B, H, W, prec)


# ----------------------------------------------------------------------------- b. the deferred path


@pytest.mark.parametrize("B,H,W,r", [(1, 55, 128, 4), (2, 23, 37, 1), (2, 23, 37, 2), (2, 23, 37, 3), (20, 23, 37, 4)])
def test_deferred_path_lookup(B, H, W, r):
    """corr_lookup_kernel's two copies of the deferred branch (a tap whose floor the fp32 round trip moved
    off the staged patch: four corners from global memory): the scalar-interval form (55x128, r = 4), the
    VALU form at R = 1, 2, 3 and at R = 4 (17020 pixels).  The coordinate sets (lookup_oracle.deferred_coords)
    reach the branch on every level: test_lookup_oracle_host.py checks the counts.  The bound is asserted
    over exactly the deferred taps first, so a failure names the path."""
    pyr, _ = _pyramid(B, H, W, 4)
    coords = _coords("deferred", B, H, W)
    only = LO.off_patch_taps(coords, LO.level_dims(H, W, 4), r)
    assert only.any()
    ref, cmax = _ref("deferred", B, H, W, 4, 4, r)
    got, flow = _lookup(pyr, B, H, W, 4, r, coords, flow_ld=4)
    _assert_taps(got, ref, cmax, r, f"deferred-{B}x{H}x{W}-r{r}-{_form(B, H, W, 4, r)}", only=only)
    assert _same(flow, _flow_ref(coords, B, H, W))


@pytest.mark.parametrize("B,H,W", [(1, 55, 128), (2, 23, 37)])
def test_deferred_path_fused(B, H, W):
    """lookup_conv.hip's copy of the deferred branch, on the same coordinates (taps recovered as in
    test_fused_taps_vs_oracle)."""
    _check_fused("deferred", B, H, W, "f16x3")


# ----------------------------------------------------------------------------- d. range flags

FB, FH, FW = 2, 17, 21
FLAG_VALUES = {"40000": (40000.0, 1), "32768": (32768.0, 0), "nan": (float("nan"), 0), "none": (None, 0)}


def _flag_pyramid(value):
    """Levels of N(0, 0.01) in which one element is `value`: (1, 1) of the last pixel's level-3 map (2x2),
    which the last pixel's centre tap at coordinates (8, 8) samples with weight 1 (8 / 8 + 0 = 1 on a
    2-px axis: 2 * 1 / 1 - 1 = 1, back to exactly 1).  The reference confirms it below."""
    rng = np.random.default_rng(4)
    levels = [(rng.standard_normal((FB * FH * FW, h, w)) * 0.01).astype(np.float32)
              for h, w in LO.level_dims(FH, FW, 4)]
    if value is not None:
        levels[3][-1, 1, 1] = value
    coords = (LO.grid_xy(FB, FH, FW) + rng.uniform(-2, 2, (FB * FH * FW, 2))).astype(np.float32)
    coords[-1] = (8.0, 8.0)
    return LO.tile_levels(levels, FB, FH, FW).to(DEV), levels, coords


def _flag_expect(levels, coords, r, value):
    ref, cmax = LO.lookup_ref(levels, coords, r)
    rd = 2 * r + 1
    ci = 3 * rd * rd + r * rd + r
    if value is not None:
        assert ref[-1, ci] == value or (np.isnan(value) and np.isnan(ref[-1, ci]))
    rest = np.abs(ref)
    rest[-1, ci] = 0
    assert np.nanmax(rest) < 1.0          # the one element is the only large tap
    with np.errstate(invalid="ignore"):
        return ref, cmax, int(bool((np.abs(ref) > 32768.0).any()))


@pytest.mark.parametrize("vid", list(FLAG_VALUES))
@pytest.mark.parametrize("r", [4, 3, 5], ids=["R4-scalar", "R3-valu", "r5-generic"])
def test_lookup_range_flag(r, vid):
    """raft_corr_lookup's flag in its three kernels: raised by a tap of 40000, not by exactly 32768 (the
    rule is "exceeds"), not by NaN, not without a large tap; a flag already 1 stays 1."""
    value, want = FLAG_VALUES[vid]
    pyr, levels, coords = _flag_pyramid(value)
    ref, cmax, expect = _flag_expect(levels, coords, r, value)
    assert expect == want
    for preset in (0, 1):
        flag = torch.full((3,), -5, dtype=torch.int32, device=DEV)
        flag[1] = preset
        got, _ = _lookup(pyr, FB, FH, FW, 4, r, coords, flag=flag[1:])
        assert flag.cpu().tolist() == [-5, max(want, preset), -5]
        _assert_taps(got, ref, cmax, r, f"flag-r{r}-{vid}")


@pytest.mark.parametrize("vid", list(FLAG_VALUES))
def test_lookup_convf1_lookup_flag(vid):
    """The lookup flag of raft_corr_lookup_convf1 (its convf1 flag: test_lookup_convf1_range_guard)."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    value, want = FLAG_VALUES[vid]
    pyr, levels, coords = _flag_pyramid(value)
    N, ntap, n = FB * FH * FW, 324, 32
    wv = torch.zeros(n // 32, 49, 2, 32, device=DEV)
    bias = torch.zeros(n, device=DEV)
    c = torch.from_numpy(coords).to(DEV)
    for preset in (0, 1):
        flags = torch.tensor([preset, 0], dtype=torch.int32, device=DEV)
        whole, out = _buf(N, ntap)
        f1w, f1 = _buf(N, n)
        _lib.call("raft_corr_lookup_convf1", pyr.data_ptr(), FB, FH, FW, 4, 4, c.data_ptr(), 0, out.data_ptr(), ntap, 0,
                  None, 0, flags.data_ptr(), wv.data_ptr(), bias.data_ptr(), n, 7, _lib.PREC_F16X3, f1.data_ptr(), n,
                  flags.data_ptr() + 4, K.stream_handle())
        torch.cuda.synchronize()
        assert flags.cpu().tolist() == [max(want, preset), 0]
        assert _guards_ok(whole, N, ntap) and _guards_ok(f1w, N, n)


@pytest.mark.parametrize("vid", list(FLAG_VALUES))
def test_lookup_conv_lookup_flag(vid):
    """raft_corr_lookup_conv's first flag (the lookup's taps, the split convc1 input) with the 40000,
    exactly-32768, NaN and no-large-tap pyramids; the selection weights pass the tap through, so c1's
    own flag (outputs above the limit) follows it where the tap is selected (k0 = 196 covers level 3)."""
    value, want = FLAG_VALUES[vid]
    pyr, levels, coords = _flag_pyramid(value)
    for preset in (0, 1):
        flags = torch.tensor([preset, 0, 0], dtype=torch.int32, device=DEV)
        _, _, got = _fused_taps(pyr, FB, FH, FW, coords, "f16x3", flags=flags)
        assert got == [max(want, preset), want, 0]


def _alt_case(entry, C, r, far, level):
    """fmaps of small values whose one dot product is value * scale_div: fmap1's pixel p0 is e_0 * a,
    fmap2's pixel q0 of `level` is e_0 * b (+ small values elsewhere), p0's coordinate is q0 * 2^level
    exactly, so its centre tap is the dot product with weight 1."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    B, H1, W1 = 1, 16, 24
    sd = 8.0
    L = level + 1 if entry == "levels" else 1
    dims = LO.level_dims(H1, W1, L)
    p0y, p0x = 9, 12                  # tile (1, 1) of the 8x8 query tiles
    q0y, q0x = 3, 5

    def run(value):
        rng = np.random.default_rng(6)
        f1 = (rng.standard_normal((B, H1, W1, C)) * 1e-3).astype(np.float32)
        f2s = [(rng.standard_normal((B, h, w, C)) * 1e-3).astype(np.float32) for h, w in dims]
        f1[0, p0y, p0x] = 0
        if value is not None:
            a = 200.0 if value == 40000.0 else 128.0
            f1[0, p0y, p0x, 0] = a
            f2s[level][0, q0y, q0x, 0] = np.float32(value / a * sd) if np.isfinite(value) else value
        coords = (LO.grid_xy(B, H1, W1) + rng.uniform(-0.9, 0.9, (H1 * W1, 2))).astype(np.float32).reshape(B, H1, W1, 2)
        coords[0, p0y, p0x] = (q0x * 2 ** level, q0y * 2 ** level)
        if far:
            coords[0, p0y + 2, p0x + 1] = (40.5, -7.25)   # this tile's window box does not fit: per pixel
        N, rd2 = B * H1 * W1, (2 * r + 1) ** 2
        out = []
        for preset in (0, 1):
            flag = torch.tensor([-5, preset, -5], dtype=torch.int32, device=DEV)
            whole, o = _buf(N, L * rd2 + 3)
            t1 = torch.from_numpy(f1).to(DEV)
            t2 = [torch.from_numpy(f).to(DEV) for f in f2s]
            ct = torch.from_numpy(coords).to(DEV)
            if entry == "levels":
                ptrs, hs, ws = K.alt_levels_args([(t, h, w) for t, (h, w) in zip(t2, dims)])
                _lib.call("raft_alt_corr_lookup_levels_prec", t1.data_ptr(), ptrs, hs, ws, L, ct.data_ptr(), 0,
                          o.data_ptr(), L * rd2 + 3, B, H1, W1, C, r, sd, None, 0, flag.data_ptr() + 4,
                          _lib.PREC_F16X3, K.stream_handle())
            else:
                _lib.call("raft_alt_corr_lookup_nhwc_prec", t1.data_ptr(), t2[0].data_ptr(), ct.data_ptr(), 0, 1.0,
                          o.data_ptr(), rd2 + 3, B, H1, W1, H1, W1, C, r, sd, None, 0, flag.data_ptr() + 4,
                          _lib.PREC_F16X3, K.stream_handle())
            torch.cuda.synchronize()
            assert _guards_ok(whole, N, L * rd2)
            got = o[p0y * W1 + p0x, level * rd2 + r * (2 * r + 1) + r].item()
            rest = o[:, :L * rd2].clone()
            rest[p0y * W1 + p0x, level * rd2 + r * (2 * r + 1) + r] = 0
            if value is None or np.isfinite(value):
                assert float(rest.abs().max()) < 100.0      # nothing else is large
            out.append((flag.cpu().tolist(), got))
        return out

    return run


ALT_SITES = [  # id names the flag site of alt_corr.hip the case reaches (launch_alt's dispatch)
    ("nhwc-C40-r4:tile-kernel-alt_bin_store", "nhwc", 40, 4, False, 0),
    ("nhwc-C64-r4:mfma-box-gemm", "nhwc", 64, 4, False, 0),
    ("nhwc-C40-r4-far-coordinate:tile-kernel-per-pixel-alt_pixel", "nhwc", 40, 4, True, 0),
    ("nhwc-C64-r3:per-pixel-kernel-alt_pixel", "nhwc", 64, 3, False, 0),
    ("nhwc-C64-r5:generic-radius-kernel", "nhwc", 64, 5, False, 0),
    ("levels-C64-r4-level1:mfma-box-gemm-all-levels", "levels", 64, 4, False, 1),
    ("levels-C40-r4-level1:tile-kernel-per-level-launches", "levels", 40, 4, False, 1),
]


@pytest.mark.parametrize("vid", list(FLAG_VALUES))
@pytest.mark.parametrize("site", ALT_SITES, ids=[s[0] for s in ALT_SITES])
def test_alt_lookup_range_flag(site, vid):
    """The range flag of raft_alt_corr_lookup_nhwc_prec / _levels_prec at each of its sites: one dot
    product of exactly 40000 * scale_div raises it, exactly 32768 * scale_div and NaN do not, a preset 1
    stays.  (alt_corr.hip's fifth site, the MFMA kernel's [B][N][RD^2][H][W] branch, is reached only by
    raft_alt_corr_forward_prec, which passes no flag.)"""
    _, entry, C, r, far, level = site
    value, want = FLAG_VALUES[vid]
    for preset, (flags, got) in zip((0, 1), _alt_case(entry, C, r, far, level)(value)):
        if value is not None:
            assert got == value or (np.isnan(value) and np.isnan(got)), got
        assert flags == [-5, max(want, preset), -5]


# ----------------------------------------------------------------------------- e. pyramid padding

BUILDS = [  # (id, entry, C): the kernel the entry reaches at 23x37 (corr_pyramid.hip's dispatch)
    ("raft_corr_build-C24:corr_build_kernel-fp32", "build", 24),
    # f16x3 takes corr_build2_kernel (the RAFT_CORR_BUILD_BIG path, the default, at every shape); the
    # RAFT_CORR_BUILD_BIG=0 kernel is chosen once per process from the environment: not reachable here
    ("raft_corr_build_prec-f16x3-C40:corr_build2_kernel", "prec", 40),
    ("raft_corr_build_ws-f16x3-C64:corr_build4_kernel-256x256", "ws", 64),
]


@pytest.mark.parametrize("bid,entry,C", BUILDS, ids=[b[0] for b in BUILDS])
def test_build_writes_zero_padding(bid, entry, C):
    """The lookups read ragged tiles whole and rely on the pyramid's padding being 0.  Each build entry on
    a NaN-prefilled buffer, 23x37, B = 2, 4 levels (ragged at every level: 23x37, 11x18, 5x9, 2x4): every
    padding element of every level, indexed in the raw buffer by the header's formula, is +0.0 or -0.0,
    and the valid elements equal raft_corr_pyramid_level's row-major copy."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    B, H, W, L = 2, 23, 37, 4
    N = B * H * W
    g = torch.Generator().manual_seed(C)
    f1 = torch.randn(N, C, generator=g).to(DEV)
    f2 = torch.randn(N, C, generator=g).to(DEV)
    pyr = torch.full((K.pyramid_floats(B, H, W, L),), float("nan"), device=DEV)
    s = K.stream_handle()
    if entry == "build":
        _lib.call("raft_corr_build", f1.data_ptr(), f2.data_ptr(), C, B, H, W, C, L, K.sqrt_c(C), pyr.data_ptr(), s)
    elif entry == "prec":
        _lib.call("raft_corr_build_prec", f1.data_ptr(), f2.data_ptr(), C, B, H, W, C, L, K.sqrt_c(C), _lib.PREC_F16X3,
                  pyr.data_ptr(), s)
    else:
        nbytes = int(_lib.load().raft_corr_build_ws_bytes_prec(B, H, W, C, _lib.PREC_F16X3))
        assert nbytes > 0, "this shape does not take the 256 x 256 kernel"
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.call("raft_corr_build_ws", f1.data_ptr(), f2.data_ptr(), C, B, H, W, C, L, K.sqrt_c(C), _lib.PREC_F16X3,
                  pyr.data_ptr(), ws.data_ptr(), nbytes, s)
    off = 0
    for l, (h, w) in enumerate(LO.level_dims(H, W, L)):
        th, tw = -(-h // 4), -(-w // 4)
        S = th * tw * 16
        y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        idx = torch.from_numpy((((y >> 2) * tw + (x >> 2)) * 16 + (y & 3) * 4 + (x & 3)).ravel()).to(DEV)
        region = pyr[off:off + N * S].view(N, S)
        copy = torch.empty(N, h * w, device=DEV)
        _lib.call("raft_corr_pyramid_level", pyr.data_ptr(), B, H, W, L, l, copy.data_ptr(), s)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(copy).all()) and float(copy.abs().max()) > 0
        assert torch.equal(region[:, idx], copy), f"level {l}: valid elements differ from raft_corr_pyramid_level"
        pad = torch.ones(S, dtype=torch.bool, device=DEV)
        pad[idx] = False
        assert int(pad.sum()) == S - h * w > 0
        assert bool((region[:, pad] == 0).all()), f"level {l}: padding is not zero"
        off += N * S
    assert off == pyr.numel()


# ----------------------------------------------------------------------------- f. huge and non-finite coordinates

HUGE = [1e6, -1e6, 3e9, -3e9, 3e38, -3e38, float("inf"), float("-inf"), float("nan")]


def _huge_coords():
    """The matrix coordinates of 2x17x21 (with in-range values at the special pixels: `base`) and the same
    with 18 pixels set, one axis at a time, to the HUGE values (`huge`); `special` their indices."""
    B, H, W = 2, 17, 21
    base = _coords("matrix", B, H, W).copy()
    rng = np.random.default_rng(12)
    special = np.sort(rng.choice(B * H * W, 2 * len(HUGE), replace=False))
    base[special] = LO.grid_xy(B, H, W)[special] + 0.25
    huge = base.copy()
    for k, p in enumerate(special):
        huge[p, k % 2] = np.float32(HUGE[k // 2])
    return base, huge, special


def _check_huge(got_base, got_huge, ref_huge, cmax, special, r, what, u=0.0, abs_term=0.0, rows_nan=False):
    others = np.ones(len(got_base), bool)
    others[special] = False
    assert _same(got_base[others], got_huge[others]), f"{what}: a huge coordinate changed another pixel's taps"
    for k, p in enumerate(special):
        v = HUGE[k // 2]
        if rows_nan and np.isnan(ref_huge[p]).any():
            continue    # the fused kernel: a NaN tap makes the pixel's whole convc1 row NaN, and its relu (fmaxf) 0
        if not np.isfinite(v):
            assert np.isnan(got_huge[p]).all(), (what, v)
        elif abs(v) < 1e38:
            assert (got_huge[p] == 0).all(), (what, v)
        # +-3e38: 2 X overflows on level 0 (NaN taps), X / 2^l does not on the others (0): as the reference
        bad, _ = LO.tap_check(got_huge[p:p + 1], ref_huge[p:p + 1], cmax[p:p + 1], u, abs_term)
        assert not bad.any(), (what, v, int(bad.sum()))


@pytest.mark.parametrize("B2,r", [(2, 4), (2, 3), (2, 5), (47, 4)],
                         ids=["R4-scalar", "R3-valu", "r5-generic", "R4-valu-16779px"])
def test_huge_and_non_finite_coordinates_lookup(B2, r):
    """Coordinates of 1e6, 3e9 (past the int range), 3e38, inf and NaN, either sign, one axis at a time:
    every other pixel's row is bit-equal to a run where those pixels hold in-range coordinates; a pixel
    with a far finite coordinate has all-zero taps; one with a non-finite coordinate all-NaN taps (+-3e38:
    NaN on level 0, where 2 X overflows, 0 on the others -- the reference's arithmetic, lookup_ref);
    flow_out = coords - grid in fp32.  (R4-valu: the same pixels in the first two of 47 images.)

    Why no address can escape (read before this test was first run):
    - Window origins.  floor(c) is clamped to +-2^30 before the conversion (lookup_common.hpp
      floor_origin), so origin - R, + 2R + 2 and the differences of the clipped row / column intervals do
      not wrap.  Unclamped they did: a row coordinate that converts to INT_MIN / INT_MAX (-3e9, -inf, 3e9,
      inf) made y0 + 2R + 2 wrap, the scalar-interval form's row count max(rhi - rlo, 0) came out as
      2R + 2 again, and its lanes fetched from a window base about 2^29 tile rows off the pyramid
      (corr_lookup_kernel<4, 4, *, true>, and lookup_conv_kernel's 64-bit-base path; its 32-bit-offset
      path fetched wrapped, in-buffer offsets).  Found by reading, fixed with the clamp, then run.
    - corr_lookup_kernel, both window forms: a lane fetches only if unsigned compares put its row inside
      [max(y0, 0), min(y0 + WD, 4 th)) and its tile column inside [max(txo, 0), min(txo + ntx, tw)) (SCAL), or
      (unsigned)ty < th and (unsigned)tx < tw (VALU); every other lane passes offset 0x80000000 to a raw
      buffer whose num_records is below it: no access.
    - The taps: axis_entry's (int)floorf(u) saturates (v_cvt_i32_f32), i - origin is then far outside
      [0, extent) (origin within +-2^30 + R), so the tap is OFF_PATCH; a non-finite u is NAN_POS and
      never indexes.  The LDS patch is indexed only with 0 <= i - origin < extent.
    - The deferred at(y, x) of corr_lookup_kernel and lookup_conv_kernel, and the generic kernel's, load
      only if (unsigned)y < h and (unsigned)x < w; i + 1 wrapping to INT_MIN fails that compare."""
    H, W, L = 17, 21, 4
    base, huge, special = _huge_coords()
    if B2 > 2:
        extra = _coords("matrix", B2, H, W)[len(base):]
        base, huge = np.concatenate([base, extra]), np.concatenate([huge, extra])
    pyr, levels = _pyramid(B2, H, W, L)
    ref, cmax = LO.lookup_ref([lv[:2 * H * W] for lv in levels], huge[:2 * H * W], r)
    got_b, _ = _lookup(pyr, B2, H, W, L, r, base, flow_ld=2)
    got_h, flow = _lookup(pyr, B2, H, W, L, r, huge, flow_ld=2)
    n = 2 * H * W
    assert _same(got_b[n:], got_h[n:])
    _check_huge(got_b[:n], got_h[:n], ref, cmax, special, r, _form(B2, H, W, L, r))
    assert _same(flow, _flow_ref(huge, B2, H, W))


def test_huge_and_non_finite_coordinates_fused():
    """The same pixels through raft_corr_lookup_conv (lookup_conv_kernel; the argument above covers its
    window table and its deferred branch).  Its taps come back through convc1 and its relu: a pixel with a
    NaN tap has an all-NaN convc1 row, which fmaxf(., 0) stores as 0, so those pixels' taps are not
    observable here; the far finite pixels' taps are 0 and every other pixel's recovered taps are
    bit-equal between the two runs."""
    B, H, W = 2, 17, 21
    base, huge, special = _huge_coords()
    pyr, levels = _pyramid(B, H, W, 4)
    ref, cmax = LO.lookup_ref(levels, huge, 4)
    got_b, _, _ = _fused_taps(pyr, B, H, W, base, "f16x3")
    got_h, flow, _ = _fused_taps(pyr, B, H, W, huge, "f16x3")
    _check_huge(got_b, got_h, ref, cmax, special, 4, "lookup_conv", U_PREC["f16x3"], 2.0 ** -24, rows_nan=True)
    assert _same(flow, _flow_ref(huge, B, H, W))
