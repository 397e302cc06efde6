"""raft_corr_lookup_conv with 16 waves per work-group and two query pixels per wave (lookup_conv.hip):
wave w of a 2x16 tile owns pixels 2w and 2w + 1 (waves 8-15 the tile's second row), outputs 16w .. 16w + 15
of convc1 and, waves 0-7, of convf1.

Every launch runs on a pyramid the test wrote (lookup_oracle.tile_levels) inside sentinel buffers with
guard rows.  convc1 / convf1 are checked as tests/test_gpu_lookup_conv.py checks them: against an fp64
conv of the plain lookup's rows (raft_corr_lookup) and of flow = coords - grid, operands rounded to the
conv precision's operand type in the one-product modes, at TOL[prec] x max(1, max|ref|); the flow rows
equal the plain lookup's bit for bit.

Map sizes.  The entry point takes a query grid whose four pyramid levels are all non-empty, so 8x8 is the
smallest map it accepts, and from 16x16 on no level is one pixel wide (a 1-px axis has no finite sample
position: every tap of that level is NaN, core/utils/utils.py bilinear_sampler).  The maps 3x17 (B=2),
2x16 and 1x1 are therefore refused by the launch, before and after this kernel: test_maps_below_the_pyramid
asserts the refusal and that nothing is written.  What those maps were chosen for is tested at the
smallest maps that launch:
  17x17, B=2   odd height: the last tile row's second row is off the map, its waves 8-15 hold no pixel;
               ragged width: in the last tile column only wave 0's first pixel is valid
  16x16        whole tiles only
  8x8          the smallest map: half a tile wide, level 3 one pixel (NaN taps: rows of relu(NaN) = 0)
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lookup_oracle as LO
from test_gpu_lookup_conv import TOL, pack_lookup_conv_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = LO.SENTINEL
G = 4          # guard rows
NTAP = 324
PRECS = ["f16x3", "bf16", "f16"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()
    yield
    for cached in (_pyramid, _weights, _plain):
        cached.cache_clear()
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- shared data (never modified)


@functools.lru_cache(maxsize=None)
def _pyramid(B, H, W, positive=False, plant=None):
    """Independent N(0, 1) levels (|.| + 1 with `positive`); plant = (pixel, value): that pixel's whole
    level-3 map holds `value`."""
    rng = np.random.default_rng(100 * B + 10 * H + W)
    levels = [rng.standard_normal((B * H * W, h, w)).astype(np.float32) for h, w in LO.level_dims(H, W, 4)]
    if positive:
        levels = [np.abs(lv) + 1 for lv in levels]
    if plant is not None:
        levels[3][plant[0]] = plant[1]
    return LO.tile_levels(levels, B, H, W).to(DEV)


def _rand_weights(seed=5):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((256, NTAP)) * 0.05).astype(np.float32), (rng.standard_normal(256) * 0.1).astype(np.float32),
            (rng.standard_normal((128, 2, 7, 7)) * 0.1).astype(np.float32), (rng.standard_normal(128) * 0.1).astype(np.float32))


C0 = 0 * 81 + 4 * 9 + 4    # level 0's centre tap


def _owner_weights():
    """convc1 row n = n + 1 on the centre tap of level 0, convf1 row n = n + 1 on the centre tap of the x
    flow, zero elsewhere and zero bias: output n of a pixel is (n + 1) x one operand."""
    wc = np.zeros((256, NTAP), np.float32)
    wc[:, C0] = np.arange(1, 257)
    wf = np.zeros((128, 2, 7, 7), np.float32)
    wf[:, 0, 3, 3] = np.arange(1, 129)
    return wc, np.zeros(256, np.float32), wf, np.zeros(128, np.float32)


def _one_weights(which):
    """Zero weights but one of 60000 (exact in f16 and bf16) on the same taps as _owner_weights."""
    wc, bc, wf, bf = np.zeros((256, NTAP), np.float32), np.zeros(256, np.float32), np.zeros((128, 2, 7, 7), np.float32), \
        np.zeros(128, np.float32)
    if which == "c1":
        wc[5, C0] = 61440.0
    if which == "f1":
        wf[7, 0, 3, 3] = 61440.0
    return wc, bc, wf, bf


@functools.lru_cache(maxsize=None)
def _weights(kind, prec):
    w = {"rand": _rand_weights, "owner": _owner_weights, "zero": lambda: _one_weights(None),
         "c1big": lambda: _one_weights("c1"), "f1big": lambda: _one_weights("f1")}[kind]()
    return w, pack_lookup_conv_weights(*w, prec)


def _buf(rows, ld):
    whole = torch.full((rows + 2 * G, ld), SENT, device=DEV)
    return whole, whole[G:G + rows]


def _guards_ok(whole, rows, used):
    return bool((whole[:G] == SENT).all() and (whole[G + rows:] == SENT).all() and (whole[G:G + rows, used:] == SENT).all())


class Out:
    pass


def _alloc(N):
    o = Out()
    o.c1w, o.c1 = _buf(N, 260)
    o.f1w, o.f1 = _buf(N, 132)
    o.flw, o.flow = _buf(N, 4)
    o.flags = torch.zeros(3, dtype=torch.int32, device=DEV)
    return o


def _launch(o, pyr, B, H, W, c, packed, prec):
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    pc, frag, pf, ffrag = packed
    fp = o.flags.data_ptr()
    _lib.call("raft_corr_lookup_conv", pyr.data_ptr(), B, H, W, 4, 4, c.data_ptr(), o.flow.data_ptr(), 4, fp,
              _lib.PRECISIONS[prec], frag.data_ptr(), pc.bias.data_ptr(), 256, o.c1.data_ptr(), 260, fp + 4,
              ffrag.data_ptr(), pf.bias.data_ptr(), 128, 7, o.f1.data_ptr(), 132, fp + 8, K.stream_handle())


def _fused(pyr, B, H, W, coords, wkind, prec):
    N = B * H * W
    o = _alloc(N)
    c = torch.from_numpy(coords).to(DEV)
    _launch(o, pyr, B, H, W, c, _weights(wkind, prec)[1], prec)
    torch.cuda.synchronize()
    # nothing past n channels of a row, past the two flow columns, or outside the rows of the map's pixels
    assert _guards_ok(o.c1w, N, 256) and _guards_ok(o.f1w, N, 128) and _guards_ok(o.flw, N, 2)
    o.flags = o.flags.cpu().tolist()
    return o


@functools.lru_cache(maxsize=None)
def _plain(B, H, W, positive, ckey):
    """raft_corr_lookup's rows and flow for the coordinate set `ckey` (the unfused path)."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    N = B * H * W
    c = torch.from_numpy(_coords(ckey, B, H, W)).to(DEV)
    corr = torch.empty(N, NTAP, device=DEV)
    flow = torch.full((N, 4), SENT, device=DEV)
    _lib.call("raft_corr_lookup", _pyramid(B, H, W, positive).data_ptr(), B, H, W, 4, 4, c.data_ptr(), 0, corr.data_ptr(),
              NTAP, 0, flow.data_ptr(), 4, None, K.stream_handle())
    torch.cuda.synchronize()
    return corr.cpu(), flow.cpu().numpy()


def _refs(corr, coords, B, H, W, weights, prec):
    """The fp64 references of tests/test_gpu_lookup_conv.py: relu(conv) of the plain lookup's rows and of
    flow = coords - grid (zero padded), operands rounded in the one-product modes."""
    wc, bc, wf, bf = weights
    rnd = {"f16": torch.float16, "bf16": torch.bfloat16}.get(prec)
    cin, wref = corr.double(), torch.from_numpy(wc).double()
    if rnd is not None:
        cin, wref = cin.to(rnd).double(), wref.to(rnd).double()
    ref = torch.relu(cin @ wref.T + torch.from_numpy(bc).double())
    with np.errstate(invalid="ignore"):
        fl = (coords - LO.grid_xy(B, H, W)).reshape(B, H, W, 2)
    flow, wfr = torch.from_numpy(fl).permute(0, 3, 1, 2).double(), torch.from_numpy(wf).double()
    if rnd is not None:
        flow, wfr = flow.to(rnd).double(), wfr.to(rnd).double()
    fref = torch.relu(F.conv2d(flow, wfr, torch.from_numpy(bf).double(), padding=3)).permute(0, 2, 3, 1).reshape(-1, 128)
    return ref, fref


def _close(got, ref, prec, rows=None):
    got = got.cpu().double()
    if rows is not None:
        got, ref = got[rows], ref[rows]
    scale, err = float(ref.abs().max()), float((got - ref).abs().max())
    print(f"WAVES {prec}: err {err:.3e} scale {scale:.3e} bound {TOL[prec] * max(1.0, scale):.3e}")
    assert err <= TOL[prec] * max(1.0, scale), (err, scale)


# ----------------------------------------------------------------------------- coordinates


def _coords(ckey, B, H, W):
    g = LO.grid_xy(B, H, W)
    rng = np.random.default_rng(17)
    if ckey == "rand":
        return (g + rng.normal(0, 3.0, g.shape)).astype(np.float32)
    if ckey == "posflow":     # flows in [0.6, 0.9]: convf1's centre operand and level 0's centre tap are positive
        return (g + rng.uniform(0.6, 0.9, g.shape)).astype(np.float32)
    assert ckey == "cases"
    return _case_coords(B, H, W)[0]


KINDS = ["common", "common", "offpatch", "common", "common", "far+", "integer", "ulp", "far-", "common", "common", "nan",
         "offpatch", "offpatch", "ulp", "integer"]


def _case_coords(B, H, W):
    """Pixel x of a row takes KINDS[x % 16], so that the pair of a wave (2w, 2w + 1) is in turn
    common | common, off-patch | common, common | far, integer | one ulp beside, far | common, common | NaN,
    off-patch | off-patch, ulp | integer:
      common    grid + U(-2, 2)
      offpatch  on y the fp32 number just below a multiple of 8: the level-3 centroid c / 8 + offset rounds up
                past the rows staged for floor(c) >> 3 (lookup_oracle.deferred_coords' fifth kind)
      far+-     +-1e6 on both axes: every window off every map
      integer   grid + an integer shift; ulp: the fp32 neighbour of such an integer position
      nan       x = NaN: every tap NaN"""
    rng = np.random.default_rng(23)
    g = LO.grid_xy(B, H, W)
    c = (g + rng.uniform(-2, 2, g.shape)).astype(np.float32)
    kind = np.array([KINDS[int(x) % 16] for x in g[:, 0]])
    shift = rng.integers(-3, 4, g.shape).astype(np.float32)
    k8 = np.float32(8) * rng.integers(0, H // 8 + 1, len(g)).astype(np.float32)
    c[kind == "offpatch", 1] = np.nextafter(k8, np.float32(-np.inf))[kind == "offpatch"]
    c[kind == "far+"] = 1e6
    c[kind == "far-"] = -1e6
    c[kind == "integer"] = (g + shift)[kind == "integer"]
    side = np.where(rng.integers(0, 2, g.shape) == 1, np.float32(np.inf), np.float32(-np.inf))
    c[kind == "ulp"] = np.nextafter(g + shift, side)[kind == "ulp"]
    c[kind == "nan", 0] = np.nan
    return c.astype(np.float32), kind


# ----------------------------------------------------------------------------- maps


@pytest.mark.parametrize("B,H,W", [(2, 17, 17), (1, 16, 16)], ids=["2x17x17-odd-ragged", "16x16-whole-tiles"])
@pytest.mark.parametrize("prec", PRECS)
def test_maps(B, H, W, prec):
    pyr = _pyramid(B, H, W, False)
    coords = _coords("rand", B, H, W)
    corr, flow = _plain(B, H, W, False, "rand")
    o = _fused(pyr, B, H, W, coords, "rand", prec)
    ref, fref = _refs(corr, coords, B, H, W, _weights("rand", prec)[0], prec)
    _close(o.c1[:, :256], ref, prec)
    _close(o.f1[:, :128], fref, prec)
    assert np.array_equal(o.flow[:, :2].cpu().numpy(), flow[:, :2])
    assert o.flags == [0, 0, 0]


def test_smallest_map():
    """8x8: half a tile wide; level 3 is one pixel, so every pixel has NaN taps, an all-NaN convc1 row and
    relu (fmaxf) stores 0; convf1 and the flow rows as everywhere."""
    B, H, W, prec = 1, 8, 8, "f16x3"
    coords = _coords("rand", B, H, W)
    o = _fused(_pyramid(B, H, W, False), B, H, W, coords, "rand", prec)
    assert bool((o.c1[:, :256] == 0).all())
    _, fref = _refs(torch.zeros(B * H * W, NTAP), coords, B, H, W, _weights("rand", prec)[0], prec)
    _close(o.f1[:, :128], fref, prec)
    assert np.array_equal(o.flow[:, :2].cpu().numpy(), coords - LO.grid_xy(B, H, W))
    assert o.flags[0] == 0


@pytest.mark.parametrize("B,H,W", [(2, 3, 17), (1, 2, 16), (1, 1, 1)])
def test_maps_below_the_pyramid(B, H, W):
    """Maps with an empty pyramid level: the launch is refused (it was before this kernel) and writes nothing."""
    from raft_optical_flow_amd import _lib
    N = B * H * W
    o = _alloc(N)
    pyr = torch.zeros(64 * N * 16, device=DEV)
    c = torch.from_numpy(LO.grid_xy(B, H, W)).to(DEV)
    with pytest.raises(_lib.RaftHipError, match="level is empty"):
        _launch(o, pyr, B, H, W, c, _weights("rand", "f16x3")[1], "f16x3")
    torch.cuda.synchronize()
    assert _guards_ok(o.c1w, N, 0) and _guards_ok(o.f1w, N, 0) and _guards_ok(o.flw, N, 0)
    assert o.flags.cpu().tolist() == [0, 0, 0]


# ----------------------------------------------------------------------------- the two pixels of a wave on different paths


@pytest.mark.parametrize("prec", PRECS)
def test_coords_cases(prec):
    """16x32 (two tiles a row, every wave of every tile): the pairs of _case_coords.  convc1 rows against
    the reference built from the plain lookup's rows; a pixel with a NaN tap has an all-NaN row, stored as
    relu (fmaxf) = 0, and must not touch its partner's.  The far pixels' taps are all zero: their rows are
    relu(bias).  convf1 does not depend on a pixel's lookup path (test_maps, test_owner_weights check it;
    here +-1e6 flows overflow f16 operands), so only its guards are checked.  Flow rows bit for bit."""
    B, H, W = 1, 16, 32
    coords, kind = _case_coords(B, H, W)
    dims = LO.level_dims(H, W, 4)
    off = LO.off_patch(coords, dims, 4).any(1)
    assert off[kind == "offpatch"].all() and not off[kind == "common"].any()   # the pairs are what they claim
    corr, flow = _plain(B, H, W, False, "cases")
    nanrow = torch.isnan(corr).any(1).numpy()
    assert (nanrow == (kind == "nan")).all()
    far = (kind == "far+") | (kind == "far-")
    assert bool((corr[torch.from_numpy(far)] == 0).all())
    o = _fused(_pyramid(B, H, W, False), B, H, W, coords, "rand", prec)
    w = _weights("rand", prec)[0]
    ref, _ = _refs(torch.nan_to_num(corr), coords, B, H, W, w, prec)
    _close(o.c1[:, :256], ref, prec, rows=torch.from_numpy(~nanrow))
    assert bool((o.c1[torch.from_numpy(nanrow).to(DEV), :256] == 0).all())
    assert np.array_equal(o.flow[:, :2].cpu().numpy(), flow[:, :2], equal_nan=True)
    assert o.flags[:2] == [0, 0]


# ----------------------------------------------------------------------------- which wave and lane owns which output

# One non-zero product per output: hi(w) * hi(x) is exact in fp32 (11 + 11 or 8 + 8 significand bits), so the
# one-product modes reproduce the fp64 product of the rounded operands to the fp32 rounding of the result,
# 2^-24 relative; f16x3 adds w * lo, the split dropping at most 2^-22 of x (test_gpu_lookup_forms.py: u = 2^-20).
U_OWNER = {"f16x3": 2.0 ** -20, "f16": 2.0 ** -23, "bf16": 2.0 ** -23}


@pytest.mark.parametrize("prec", PRECS)
def test_owner_weights(prec):
    """Output n = (n + 1) x one operand (positive: a pyramid of |N(0, 1)| + 1, flows in [0.6, 0.9]): every
    output, channel by channel, within U_OWNER of its own reference value, and output n / output 0 rounds to
    n + 1 -- a wrong wave-to-column or lane-to-weight-unit mapping is another integer."""
    B, H, W = 1, 17, 17
    coords = _coords("posflow", B, H, W)
    corr, _ = _plain(B, H, W, True, "posflow")
    o = _fused(_pyramid(B, H, W, True), B, H, W, coords, "owner", prec)
    ref, fref = _refs(corr, coords, B, H, W, _weights("owner", prec)[0], prec)
    for got, r, n in ((o.c1[:, :256], ref, 256), (o.f1[:, :128], fref, 128)):
        got = got.cpu().double()
        assert float(r[:, 0].min()) > 0.005    # (a border pixel's centre tap: >= 0.1 x 0.1 x 1)
        ratio = got / got[:, :1]
        assert torch.equal(torch.round(ratio), torch.arange(1, n + 1).double().expand_as(ratio)), "an output is another's"
        assert bool(((got - r).abs() <= U_OWNER[prec] * r.abs()).all()), float(((got - r).abs() / r.abs()).max())
    assert o.flags == [0, 0, 0]


# ----------------------------------------------------------------------------- range flags


@pytest.mark.parametrize("prec", PRECS)
def test_range_flags(prec):
    """16x32.  flag 0: a level-3 map of 40000 under pixel (1, 19) -- the second pixel of wave 9 of its
    tile -- gives that pixel taps above 2^15 (and nothing else does); flag 1 / flag 2: one convc1 / convf1
    weight of 61440 on an operand >= 0.6 (flows in [0.6, 0.9]; interior taps >= 1); all three stay 0 otherwise."""
    B, H, W = 1, 16, 32
    px = 1 * W + 19
    assert (px % W) % 16 == 3 and (16 * 1 + 3) // 2 == 9 and (16 * 1 + 3) % 2 == 1
    coords = _coords("posflow", B, H, W)
    plain = _pyramid(B, H, W, True)
    assert _fused(plain, B, H, W, coords, "zero", prec).flags == [0, 0, 0]
    assert _fused(_pyramid(B, H, W, True, (px, 40000.0)), B, H, W, coords, "zero", prec).flags == [1, 0, 0]
    assert _fused(plain, B, H, W, coords, "c1big", prec).flags == [0, 1, 0]
    assert _fused(plain, B, H, W, coords, "f1big", prec).flags == [0, 0, 1]


# ----------------------------------------------------------------------------- determinism


@pytest.mark.parametrize("prec", PRECS)
def test_determinism_and_graph_replay(prec):
    """Two launches, and a captured launch replayed, give the bits of the first."""
    B, H, W = 2, 17, 17
    N = B * H * W
    pyr, packed = _pyramid(B, H, W, False), _weights("rand", prec)[1]
    c = torch.from_numpy(_coords("rand", B, H, W)).to(DEV)
    a, b, g_ = _alloc(N), _alloc(N), _alloc(N)
    _launch(a, pyr, B, H, W, c, packed, prec)
    _launch(b, pyr, B, H, W, c, packed, prec)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(g_, pyr, B, H, W, c, packed, prec)
    torch.cuda.synchronize()
    for whole in (g_.c1w, g_.f1w, g_.flw):
        whole.fill_(SENT)
    graph.replay()
    torch.cuda.synchronize()
    for x in (b, g_):
        assert torch.equal(a.c1w, x.c1w) and torch.equal(a.f1w, x.f1w) and torch.equal(a.flw, x.flw)
        assert x.flags.cpu().tolist() == [0, 0, 0]
