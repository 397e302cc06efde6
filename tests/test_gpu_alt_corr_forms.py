"""The on-the-fly ("alternate") correlation kernels on every form against tests/alt_corr_oracle.py.

Every case runs an entry of include/raft_hip.h on outputs prefilled with one NaN bit pattern inside
guard floats, with sentinel columns (out_ld = L*(2r+1)^2 + 3, flow_ld = 5): guards and sentinel
columns must come back bit for bit, every documented element must be written, and every element is
compared with alt_corr_oracle.alt_ref (fp32 sample positions, dot products and the blend in fp64):
|got - ref| <= bound * mag, mag the same blend over sum_c |f1_c f2_c| per tap, NaN exactly where the
reference has NaN.  No element is left out.

bound (alt_corr_oracle.py; measured on the CPU against alt_ref, never against the
kernels): 4 x GAMMA32 x 2^-24 for the exact-fp32 kernels, 4 x (gamma16x3(scale) + GAMMA32) x 2^-24 for
the MFMA box GEMM, 4 x GAMMA_BWD x 2^-24 for the backward.

Kernel forms (alt_corr.hip launch_alt's dispatch, restated by alt_corr_oracle.kernel_form): r > 4 the
generic kernel; r = 4, C % 32 == 0, C <= 256 and a precision other than FP32 the MFMA box GEMM (window
box <= 96 x 96 per 8x8 query tile, else per pixel); r = 4, C % 8 == 0, C <= 256 the VALU tile kernel
(box <= 28 x 28, else per pixel); anything else alt_corr_kernel<1|2|4> by C <= 256 / <= 512 / above.

The worst measured ratio |err| / (2^-24 mag) of each case is printed (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import alt_corr_oracle as A
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64  # guard floats on either side of every output


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()
    yield
    for cached in (_form_inputs, _form_ref):
        cached.cache_clear()
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- buffers and runners


def _nanbuf(n):
    """n floats of the prefill NaN between two guards: (whole int32 view, the n floats)."""
    whole = torch.full((n + 2 * GUARD,), A.NAN_BITS, dtype=torch.int32, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(torch.float32)


def _untouched(t):
    return bool((t == A.NAN_BITS).all())


def _guards_ok(whole):
    return _untouched(whole[:GUARD]) and _untouched(whole[-GUARD:])


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _prec(name):
    from raft_optical_flow_amd import _lib
    return _lib.PRECISIONS[name]


def _forward(f1, f2, coords, r, scale_div, prec=None):
    """raft_alt_corr_forward (prec None) / raft_alt_corr_forward_prec: coords [B,N,H1,W1,2] ->
    [B,N,(2r+1)^2,H1,W1]; guards checked, every element written."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    B, H1, W1, C = f1.shape
    _, H2, W2, _ = f2.shape
    N = coords.shape[1]
    rd2 = (2 * r + 1) ** 2
    whole, out = _nanbuf(B * N * rd2 * H1 * W1)
    t1, t2, ct = _t(f1), _t(f2), _t(coords)
    if prec is None:
        _lib.call("raft_alt_corr_forward", t1.data_ptr(), t2.data_ptr(), ct.data_ptr(), out.data_ptr(), B, H1, W1,
                  H2, W2, C, N, r, scale_div, K.stream_handle())
    else:
        _lib.call("raft_alt_corr_forward_prec", t1.data_ptr(), t2.data_ptr(), ct.data_ptr(), out.data_ptr(), B, H1,
                  W1, H2, W2, C, N, r, scale_div, _prec(prec), K.stream_handle())
    torch.cuda.synchronize()
    assert _guards_ok(whole)
    assert not bool((out.view(torch.int32) == A.NAN_BITS).any()), "an element was not written"
    return out.cpu().numpy().reshape(B, N, rd2, H1, W1)


def _lookup(f1, f2s, coords, r, scale_div, prec, cl=0, coord_div=None, flow=True):
    """raft_alt_corr_lookup_nhwc_prec (coord_div given: one level, f2s[0]) / raft_alt_corr_lookup_levels_prec
    (coord_div None: every level of f2s): coords [B,H1,W1,2], passed in layout cl -> (bins
    [B, L*(2r+1)^2, H1, W1], flow [B,H1,W1,2] or None, the raw rows for bit comparisons)."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    B, H1, W1, C = f1.shape
    L = len(f2s)
    rd2 = (2 * r + 1) ** 2
    ld, fld, rows = L * rd2 + 3, 5, B * H1 * W1
    whole, out = _nanbuf(rows * ld)
    fwhole, fl = _nanbuf(rows * fld)
    t1, t2 = _t(f1), [_t(f) for f in f2s]
    ct = _t(coords if cl == 0 else coords.transpose(0, 3, 1, 2))
    fp = fl.data_ptr() if flow else None
    if coord_div is None:
        ptrs, hs, ws = K.alt_levels_args([(t, f.shape[1], f.shape[2]) for t, f in zip(t2, f2s)])
        _lib.call("raft_alt_corr_lookup_levels_prec", t1.data_ptr(), ptrs, hs, ws, L, ct.data_ptr(), cl,
                  out.data_ptr(), ld, B, H1, W1, C, r, scale_div, fp, fld, None, _prec(prec), K.stream_handle())
    else:
        assert L == 1
        _lib.call("raft_alt_corr_lookup_nhwc_prec", t1.data_ptr(), t2[0].data_ptr(), ct.data_ptr(), cl, coord_div,
                  out.data_ptr(), ld, B, H1, W1, f2s[0].shape[1], f2s[0].shape[2], C, r, scale_div, fp, fld, None,
                  _prec(prec), K.stream_handle())
    torch.cuda.synchronize()
    assert _guards_ok(whole) and _guards_ok(fwhole)
    o = out.view(torch.int32).reshape(rows, ld)
    assert _untouched(o[:, L * rd2:]), "sentinel columns of the output rows"
    assert not bool((o[:, :L * rd2] == A.NAN_BITS).any()), "an output element was not written"
    f = fl.view(torch.int32).reshape(rows, fld)
    assert _untouched(f[:, 2:] if flow else f), "sentinel columns of the flow rows"
    raw = out.reshape(rows, ld)[:, :L * rd2].cpu().numpy()
    got = raw.reshape(B, H1, W1, L * rd2).transpose(0, 3, 1, 2)
    gflow = None
    if flow:
        assert not bool((f[:, :2] == A.NAN_BITS).any()), "a flow element was not written"
        gflow = fl.reshape(rows, fld)[:, :2].cpu().numpy().reshape(B, H1, W1, 2)
    return got, gflow, raw


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _flow_ok(gflow, coords):
    want = A.flow_ref(coords)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(gflow), nan) and _same_bits(np.where(nan, 0, gflow), np.where(nan, 0, want))


def _note(what, ratio):
    print(f"ALT {what}: worst |err| / (2^-24 mag) = {ratio:.2f}")


# ----------------------------------------------------------------------------- a. the form matrix


@functools.lru_cache(maxsize=None)
def _form_inputs(form):
    return A.form_inputs(form)


@functools.lru_cache(maxsize=None)
def _form_ref(form, l, div, sd):
    """alt_ref of the form's inputs on level map l at coord_div div (shared, never modified)."""
    f1, f2s, c = _form_inputs(form)
    return A.alt_ref(f1, f2s[l], c, form[1], div, sd)


@pytest.mark.parametrize("entry", ["forward", "forward_prec", "nhwc", "levels"])
@pytest.mark.parametrize("form", A.FORMS, ids=A.form_id)
def test_form_matrix(form, entry):
    """Every kernel form through every entry: raft_alt_corr_forward (always exact fp32) and _forward_prec
    with N = 1 and 2 ([B][N][RD^2][H1][W1]; on the MFMA forms this is the kernel's layout-0 branch that
    no other test reaches), _lookup_nhwc_prec and _lookup_levels_prec with both coordinate layouts, B = 2,
    flow_out checked bit for bit."""
    C, r, prec, H1, W1 = form
    f1, f2s, c = _form_inputs(form)
    sd = 8.0
    rd2 = (2 * r + 1) ** 2
    worst = 0.0
    if entry in ("forward", "forward_prec"):
        p = None if entry == "forward" else prec
        bound = A.bound32() if p is None else A.form_bound(C, r, prec)
        ref, mag = _form_ref(form, 0, 1.0, sd)
        for N in (1, 2):
            got = _forward(f1, f2s[0], c[:, :N], r, sd, p)
            worst = max(worst, A.check(got, ref[:, :N], mag[:, :N], bound, f"{entry} N={N}"))
    elif entry == "nhwc":
        bound = A.form_bound(C, r, prec)
        for cl, l, div in ((0, 0, 1.0), (1, 1, 2.0)):
            ref, mag = _form_ref(form, l, div, sd)
            got, gflow, _ = _lookup(f1, f2s[l:l + 1], c[:, 0], r, sd, prec, cl, div)
            worst = max(worst, A.check(got, ref[:, 0], mag[:, 0], bound, f"nhwc layout {cl} coord_div {div}"))
            assert _flow_ok(gflow, c[:, 0])
    else:
        bound = A.form_bound(C, r, prec)
        refs = [_form_ref(form, l, float(2 ** l), sd) for l in range(2)]
        ref = np.concatenate([x[0][:, 0] for x in refs], 1)
        mag = np.concatenate([x[1][:, 0] for x in refs], 1)
        for cl in (0, 1):
            got, gflow, _ = _lookup(f1, f2s, c[:, 0], r, sd, prec, cl)
            assert got.shape[1] == 2 * rd2
            worst = max(worst, A.check(got, ref, mag, bound, f"levels layout {cl}"))
            assert _flow_ok(gflow, c[:, 0])
    _note(f"{A.form_id(form)} {entry}", worst)


# ----------------------------------------------------------------------------- b. box geometry

MFMA_BW = [10, 12, 13, 16, 17, 19, 20, 24, 25, 32, 33, 48, 49, 96]   # 96 / bw box rows per band changes at each
BOXES = ([("tile", 40, bw, bh) for bw, bh in ((28, 28), (29, 28), (28, 29))]
         + [("mfma", 64, bw, bh) for bw in MFMA_BW for bh in (10, 96)]
         + [("mfma", 64, 97, 10), ("mfma", 64, 10, 97)])


@pytest.mark.parametrize("edge", [False, True], ids=["inside", "over-right-bottom-edge"])
@pytest.mark.parametrize("box", BOXES, ids=[f"{k}-C{C}-box{bw}x{bh}" for k, C, bw, bh in BOXES])
def test_box_geometry(box, edge):
    """Tile (0, 0) gets a window box of exactly bw x bh fmap2 pixels (alt_corr_oracle.box_coords asserts
    it): the tile kernel's 28 / 29 limit on each axis separately, the MFMA kernel at every bw where its
    box rows per band (96 / bw) change, narrow-and-tall (many bands) and wide-and-short (one band)
    boxes, and boxes that fail on one axis only (per-pixel path)."""
    kind, C, bw, bh = box
    r, H1, W1, H2, W2 = 4, 16, 24, 112, 112
    assert A.kernel_form(C, r, "f16x3") == kind
    f1, f2 = A.maps(bw * 100 + bh, 1, H1, W1, H2, W2, C)
    c = A.box_coords(bw + 7 * bh + edge, H1, W1, H2, W2, r, bw, bh, edge)
    ref, mag = A.alt_ref(f1, f2, c, r, 1.0, 8.0)
    got, gflow, _ = _lookup(f1, [f2], c[:, 0], r, 8.0, "f16x3", 0, 1.0)
    _note(f"box {kind} {bw}x{bh} edge={edge}", A.check(got, ref[:, 0], mag[:, 0], A.form_bound(C, r, "f16x3")))
    assert _flow_ok(gflow, c[:, 0])


# ----------------------------------------------------------------------------- c. levels


def _per_level(f1, f2s, c, r, sd, prec):
    raws, flow = [], None
    for l, f2 in enumerate(f2s):
        _, gf, raw = _lookup(f1, [f2], c, r, sd, prec, 0, float(2 ** l), flow=(l == 0))
        raws.append(raw)
        flow = gf if l == 0 else flow
    return np.concatenate(raws, 1), flow


@pytest.mark.parametrize("C", [64, 40], ids=["mfma-C64-one-launch", "tile-C40-per-level-launches"])
@pytest.mark.parametrize("L", [1, 4, 6])
def test_levels(L, C):
    """raft_alt_corr_lookup_levels_prec with 1, 4 and AM_MAXL = 6 levels: within bound of alt_ref_levels
    and bit-identical to the per-level calls."""
    r, B, H1, W1 = 4, 2, 16, 24
    f1, _ = A.maps(L + C, B, H1, W1, 1, 1, C)
    f2s = A.level_maps(L + C + 1, B, 32, 48, C, L)
    c = A.smooth_coords(L, B, 1, H1, W1, 32, 48, 2.0)[:, 0]
    ref, mag = A.alt_ref_levels(f1, f2s, c, r, 8.0)
    got, gflow, raw = _lookup(f1, f2s, c, r, 8.0, "f16x3")
    _note(f"levels L={L} C={C}", A.check(got, ref, mag, A.form_bound(C, r, "f16x3")))
    per, pflow = _per_level(f1, f2s, c, r, 8.0, "f16x3")
    assert _same_bits(raw, per) and _same_bits(gflow, pflow)


def test_levels_rejects_seven():
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    B, H1, W1, C, r, L = 1, 8, 8, 32, 4, 7
    t1 = torch.zeros(B * H1 * W1, C, device=DEV)
    t2 = [(torch.zeros(B * 64, C, device=DEV), 8, 8) for _ in range(L)]
    ct = torch.zeros(B * H1 * W1, 2, device=DEV)
    whole, out = _nanbuf(B * H1 * W1 * L * 81)
    ptrs, hs, ws = K.alt_levels_args(t2)
    rc = _lib.load().raft_alt_corr_lookup_levels_prec(t1.data_ptr(), ptrs, hs, ws, L, ct.data_ptr(), 0, out.data_ptr(),
                                                      L * 81, B, H1, W1, C, r, 1.0, None, 0, None, _prec("f16x3"),
                                                      K.stream_handle())
    torch.cuda.synchronize()
    assert rc == -1     # RAFT_E_INVALID
    assert _untouched(whole)


def test_levels_mixed_fit():
    """One query 200 px away: its tile's box does not fit at levels 0 and 1 (per-pixel branch; the next
    level's setup and first band load follow it) and fits at levels 2 and 3 (box GEMM); the builder
    asserts which levels fit."""
    r, B, H1, W1, C, L = 4, 2, 16, 24, 64, 4
    f1, _ = A.maps(77, B, H1, W1, 1, 1, C)
    f2s = A.level_maps(78, B, 24, 240, C, L)
    c = A.mixed_fit_coords(3, B, H1, W1, 24, 240)[:, 0]
    ref, mag = A.alt_ref_levels(f1, f2s, c, r, 8.0)
    got, gflow, raw = _lookup(f1, f2s, c, r, 8.0, "f16x3")
    _note("levels mixed fit", A.check(got, ref, mag, A.bound16x3()))
    assert _flow_ok(gflow, c)
    per, pflow = _per_level(f1, f2s, c, r, 8.0, "f16x3")
    assert _same_bits(raw, per) and _same_bits(gflow, pflow)


# ----------------------------------------------------------------------------- d. coordinates


@pytest.mark.parametrize("map2", [(14, 23), (1, 1), (2, 3)], ids=lambda m: f"fmap2-{m[0]}x{m[1]}")
@pytest.mark.parametrize("form", A.CORE_FORMS, ids=A.form_id)
def test_coordinate_sets(form, map2):
    """Exact integers (dx = 0), negative fractions (floor = -1), k - 2^-20, windows half off each edge
    and each corner and wholly off the map, on every kernel, also with an fmap2 smaller than the
    window; a window wholly off the map gives exactly 0 (mag = 0 there)."""
    C, r, prec, H1, W1 = form
    H2, W2 = map2
    B = 2
    f1, f2 = A.maps(C + r + H2, B, H1, W1, H2, W2, C)
    worst = 0.0
    for k, kind in enumerate(A.EDGE_SETS):
        c = A.edge_coords(kind, 31 * k + H2, B, 1, H1, W1, H2, W2, r)
        ref, mag = A.alt_ref(f1, f2, c, r, 1.0, 8.0)
        if kind == "wholly-off":
            assert not mag.any()
        got, gflow, _ = _lookup(f1, [f2], c[:, 0], r, 8.0, prec, k % 2, 1.0)
        worst = max(worst, A.check(got, ref[:, 0], mag[:, 0], A.form_bound(C, r, prec), kind))
        assert _flow_ok(gflow, c[:, 0]), kind
        if A.kernel_form(C, r, prec) == "mfma":     # ... and the [B][N][RD^2][H1][W1] branch
            gotf = _forward(f1, f2, c, r, 8.0, prec)
            worst = max(worst, A.check(gotf, ref, mag, A.form_bound(C, r, prec), kind + " forward_prec"))
    _note(f"coordinate sets {A.form_id(form)} fmap2 {H2}x{W2}", worst)


@pytest.mark.parametrize("entry", ["nhwc", "levels", "forward_prec"])
@pytest.mark.parametrize("form", A.CORE_FORMS, ids=A.form_id)
def test_irregular_coordinates(form, entry):
    """The coordinate contract of include/raft_hip.h: one query each with +-1e8, +-3e9, +-3.4e38, +-inf
    and NaN on x only, y only and both.  Finite: every bin exactly 0; non-finite: every bin NaN;
    flow_out = coords - grid in fp32; every query of the other 8x8 tiles bit-identical to the run with
    ordinary coordinates; the queries of the same tiles within the bound."""
    C, r, prec, H1, W1 = form
    B, H2, W2, sd = 2, 14, 23, 8.0
    f1, _ = A.maps(C + r, B, H1, W1, 1, 1, C)
    f2s = A.level_maps(C + r + 1, B, H2, W2, C, 2)
    base = A.smooth_coords(C, B, 1, H1, W1, H2, W2, 1.5)
    c, where = A.irregular_coords(base)
    bound = A.form_bound(C, r, prec)
    tiles = np.zeros((B, H1, W1), bool)
    for ty, tx in ((0, 0), (1, 2)):
        tiles[0, ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True
    if entry == "forward_prec":
        ref, mag = A.alt_ref(f1, f2s[0], c, r, 1.0, sd)
        got = _forward(f1, f2s[0], c, r, sd, prec)
        got0 = _forward(f1, f2s[0], base, r, sd, prec)
        worst = A.check(got, ref, mag, bound)
        assert _same_bits(got[:, 0].transpose(0, 2, 3, 1)[~tiles], got0[:, 0].transpose(0, 2, 3, 1)[~tiles])
        ref, got = ref[:, 0], got[:, 0]
    else:
        lv = f2s if entry == "levels" else f2s[:1]
        div = None if entry == "levels" else 1.0
        ref, mag = A.alt_ref_levels(f1, lv, c[:, 0], r, sd)
        got, gflow, _ = _lookup(f1, lv, c[:, 0], r, sd, prec, 0, div)
        got0, gflow0, _ = _lookup(f1, lv, base[:, 0], r, sd, prec, 0, div)
        worst = A.check(got, ref, mag, bound)
        assert _flow_ok(gflow, c[:, 0])
        assert _same_bits(got.transpose(0, 2, 3, 1)[~tiles], got0.transpose(0, 2, 3, 1)[~tiles])
    # the contract, spelled out on the reference-independent side: level 0 of every special query
    rd2 = (2 * r + 1) ** 2
    g0 = got.transpose(0, 2, 3, 1)[where[:, 0]][:, :rd2]
    fin = np.isfinite(c[:, 0][where[:, 0]]).all(-1)
    assert np.isnan(g0[~fin]).all() and (g0[fin] == 0).all()
    _note(f"irregular {A.form_id(form)} {entry}", worst)


@pytest.mark.parametrize("form", A.CORE_FORMS, ids=A.form_id)
def test_coord_div_3(form):
    """coord_div = 3 (not a power of two): the bins are those of coords / 3 in fp32, flow_out is
    coords - grid exactly (not (coords / 3) * 3 - grid)."""
    C, r, prec, H1, W1 = form
    f1, f2s, c = _form_inputs(form)
    c3 = (c[:, :1] * np.float32(2.9173)).astype(np.float32)
    assert np.mean((c3 / np.float32(3)) * np.float32(3) != c3) > 0.1     # the product does not give c3 back
    ref, mag = A.alt_ref(f1, f2s[0], c3, r, 3.0, 8.0)
    for cl in (0, 1):
        got, gflow, _ = _lookup(f1, f2s[:1], c3[:, 0], r, 8.0, prec, cl, 3.0)
        A.check(got, ref[:, 0], mag[:, 0], A.form_bound(C, r, prec))
        assert _flow_ok(gflow, c3[:, 0])


# ----------------------------------------------------------------------------- e. the split's magnitude range


@pytest.mark.parametrize("scale", list(A.GAMMA16X3), ids=lambda s: f"scale-2^{int(np.log2(s))}")
def test_f16x3_magnitude_sweep(scale):
    """The MFMA box GEMM on the golden feature maps scaled by 2^-8 .. 2^6: within 4 x (the f16x3
    restatement's own error at that scale + the fp32 accumulation term).  The split's lo = f16(x - hi) is
    unscaled, so below |x| ~ 2^-3 it is an f16 subnormal and the error relative to mag grows as the maps
    shrink (DESIGN.md 7.3 has the curve)."""
    g = load_golden("lookup_b2c64_16x20.npz")
    f1 = np.ascontiguousarray(g["fmap1"].transpose(0, 2, 3, 1)) * np.float32(scale)
    f2 = np.ascontiguousarray(g["fmap2"].transpose(0, 2, 3, 1)) * np.float32(scale)
    c = A.smooth_coords(9, 2, 1, 16, 20, 16, 20, 1.5)
    ref, mag = A.alt_ref(f1, f2, c, 4, 1.0, 8.0)
    got, _, _ = _lookup(f1, [f2], c[:, 0], 4, 8.0, "f16x3", 0, 1.0)
    _note(f"f16x3 box GEMM at map scale {scale}", A.check(got, ref[:, 0], mag[:, 0], A.bound16x3(scale)))
    # the exact-fp32 route of the same call stays at the fp32 bound at every scale
    got, _, _ = _lookup(f1, [f2], c[:, 0], 4, 8.0, "fp32", 0, 1.0)
    _note(f"fp32 tile kernel at map scale {scale}", A.check(got, ref[:, 0], mag[:, 0], A.bound32()))


# ----------------------------------------------------------------------------- f. the backward


def _backward(f1, f2, c, g, r):
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    B, H1, W1, C = f1.shape
    _, H2, W2, _ = f2.shape
    N = c.shape[1]
    nws = int(_lib.load().raft_alt_corr_backward_workspace_floats(B, H1, W1, H2, W2, C, N, r))
    assert nws > 0
    w1, o1 = _nanbuf(f1.size)
    w2, o2 = _nanbuf(f2.size)
    wc, oc = _nanbuf(c.size)
    ws = torch.full((nws + 64,), A.NAN_BITS, dtype=torch.int32, device=DEV)
    t = [_t(x) for x in (f1, f2, c, g)]
    _lib.call("raft_alt_corr_backward", *(x.data_ptr() for x in t), o1.data_ptr(), o2.data_ptr(), oc.data_ptr(),
              B, H1, W1, H2, W2, C, N, r, ws.data_ptr(), nws, K.stream_handle())
    torch.cuda.synchronize()
    assert _guards_ok(w1) and _guards_ok(w2) and _guards_ok(wc)
    assert _untouched(ws[nws:]), "the 64 floats past the workspace"
    for o in (o1, o2, oc):
        assert not bool((o.view(torch.int32) == A.NAN_BITS).any()), "a gradient element was not written"
    return (o1.cpu().numpy().reshape(f1.shape), o2.cpu().numpy().reshape(f2.shape),
            oc.cpu().numpy().reshape(c.shape))


@pytest.mark.parametrize("name", A.BWD_CASES)
def test_backward(name):
    """raft_alt_corr_backward against alt_corr_oracle.alt_bwd_ref (explicit fp64 sums; a query with a
    non-finite coordinate or |coordinate| >= 1e8 is absent and has coords_grad (0, 0)): 200 queries
    sharing one window origin, windows half off each edge, two identical coordinate sets, a 1x1 fmap2,
    r = 0, C = 4 and 1024, exact integers, irregular coordinates.  Bit-identical run to run."""
    f1, f2, c, g, r = A.bwd_case(name)
    ref, mags = A.alt_bwd_ref(f1, f2, c, g, r)
    got = _backward(f1, f2, c, g, r)
    worst = max(A.check(x, y, m, A.bound_bwd(), f"{name} {what}")
                for x, y, m, what in zip(got, ref, mags, ("fmap1_grad", "fmap2_grad", "coords_grad")))
    if name == "irregular":
        _, where = A.irregular_coords(c)
        assert (got[2][where] == 0).all()
    if name in ("tied", "irregular"):
        again = _backward(f1, f2, c, g, r)
        assert all(_same_bits(x, y) for x, y in zip(got, again))
    _note(f"backward {name}", worst)
