"""Caller-side HIP kernels against the reference's own outputs (tests/golden/caller_utils.npz,
written by tests/golden/make_golden.py from core/utils/utils.py): replicate padding (exact),
forward_interpolate (exact: the same nearest source), bilinear_sampler (1e-6) + its mask,
and the batched .flo writer.  Below those, the same kernels through their C entries at the edges the goldens
do not reach (tests/elementwise_oracle.py is the reference), and raft_stream_carry's two kernels."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_input_padder_gpu_matches_reference():
    from raft_optical_flow_amd import InputPadder
    g = load_golden("caller_utils.npz")
    x = torch.from_numpy(g["pad_in"]).to(DEV)
    for mode, key in (("sintel", "pad_sintel"), ("kitti", "pad_kitti")):
        p = InputPadder(x.shape, mode=mode)
        y, = p.pad(x)
        assert y.is_cuda and np.array_equal(y.cpu().numpy(), g[key])
        assert torch.equal(p.unpad(y), x)


def test_input_padder_cpu_tensor_round_trips_through_gpu():
    from raft_optical_flow_amd import InputPadder
    g = load_golden("caller_utils.npz")
    x = torch.from_numpy(g["pad_in"])
    y, = InputPadder(x.shape).pad(x)
    assert not y.is_cuda and np.array_equal(y.numpy(), g["pad_sintel"])


@pytest.mark.parametrize("name", ["fi_smooth", "fi_leaving", "fi_zero"])
def test_forward_interpolate_matches_reference(name):
    from raft_optical_flow_amd.utils.utils import forward_interpolate
    g = load_golden("caller_utils.npz")
    f = torch.from_numpy(g[name + "_in"]).to(DEV)
    out = forward_interpolate(f)
    assert out.is_cuda and out.shape == f.shape
    assert np.array_equal(out.cpu().numpy(), g[name + "_out"])
    # batched form
    out2 = forward_interpolate(torch.stack([f, f]))
    assert torch.equal(out2[1], out)


def test_bilinear_sampler_matches_reference():
    from raft_optical_flow_amd.utils.utils import bilinear_sampler
    g = load_golden("caller_utils.npz")
    out, m = bilinear_sampler(torch.from_numpy(g["bs_img"]).to(DEV), torch.from_numpy(g["bs_coords"]).to(DEV),
                              mask=True)
    assert float(np.abs(out.cpu().numpy() - g["bs_out"]).max()) < 1e-6
    assert np.array_equal(m.cpu().numpy(), g["bs_mask"])


def test_write_flo_batch(tmp_path):
    from raft_optical_flow_amd import io as rio
    flows = torch.randn(3, 2, 9, 13, device=DEV)
    paths = [str(tmp_path / f"f{i}.flo") for i in range(3)]
    rio.write_flo_batch(paths, flows)
    for i in range(3):
        assert np.array_equal(rio.readFlow(paths[i]), flows[i].permute(1, 2, 0).cpu().numpy())


# ----------------------------------------------------------------------------- the C entries, directly
#
# Below, every kernel is launched through its C entry on sentinel-filled buffers and held to
# tests/elementwise_oracle.py (fp64, or the reference's own operator where the result is exact).

SENT = -7.0


def _call(name, *args):
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    # tensors are passed as they are and stay referenced until the launch has finished
    _lib.call(name, *[a.data_ptr() if torch.is_tensor(a) else a for a in args], K.stream_handle())
    torch.cuda.synchronize()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _take(buf, n):
    host = buf.cpu().numpy()
    assert np.all(host[n:] == SENT), "wrote past the output"
    return host[:n]


@pytest.mark.parametrize("case", [
    (7, 4, 5, 0, 0, 3, 0),    # one side only
    (3, 3, 3, 2, 0, 0, 0),    # one side only, the other axis
    (7, 4, 5, 1, 2, 3, 4),    # all four different, NC = 7
    (2, 1, 2, 3, 5, 5, 3),    # pads larger than the image (H = 1, W = 2, pads 3 / 5)
    (7, 4, 5, 0, 0, 0, 0),    # zero pads: a copy
], ids=lambda c: "NC%d-%dx%d-t%db%dl%dr%d" % c)
def test_pad_replicate_is_np_pad_edge(case):
    """raft_pad_replicate, exact against np.pad(mode='edge')."""
    nc, h, w, top, bottom, left, right = case
    x = np.random.default_rng(nc + h).normal(size=(nc, h, w)).astype(np.float32)
    want = np.pad(x, ((0, 0), (top, bottom), (left, right)), mode="edge")
    out = torch.full((want.size + 16,), SENT, device=DEV)
    _call("raft_pad_replicate", _dev(x), out.data_ptr(), nc, h, w, top, bottom, left, right)
    assert np.array_equal(_take(out, want.size).reshape(want.shape), want)


def _axis_values(size):
    """Coordinates along one axis of `size` pixels: every integer, the borders -1, 0, size-1, size and their
    neighbours one ulp to either side, far outside, NaN and +-Inf."""
    f = np.float32
    v = [f(i) for i in range(size)]
    for e in (-1.0, 0.0, float(size - 1), float(size)):
        v += [f(e), np.nextafter(f(e), f(-1e9)), np.nextafter(f(e), f(1e9))]
    v += [f(0.37), f(size - 1.25), f(1e6), f(-1e6), f(np.nan), f(np.inf), f(-np.inf)]
    return np.asarray(v, np.float32)


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("hw", [(6, 9), (6, 1)], ids=lambda s: "%dx%d" % s)
def test_bilinear_sample_edges(hw, C):
    """raft_bilinear_sample on exact-integer, border (-1, 0, S-1, S and one ulp around each), far (+-1e6), NaN and
    +-Inf coordinates; Ho x Wo differs from H x W; N = 2 (image 1 samples random positions); W == 1 divides by
    zero like the reference (NaN everywhere).  Reference: F.grid_sample(align_corners=True, zeros) on the CPU
    with the reference's normalisation: in float32 for the NaN pattern and the mask (both must be equal), in
    float64 for the values, within max(4 * E_ref, 8 * 2^-24 * max|img|), E_ref the float32 CPU result's own error
    against float64.  Seen on an MI355X (profiles/elementwise_gpu_tests.log), 6 x 9: C = 1: E_ref 1.1e-6, bound
    4.5e-6, kernel 6.1e-7; C = 5: E_ref 1.0e-6, bound 4.1e-6, kernel 6.6e-7."""
    import elementwise_oracle as EO
    H, W = hw
    r = np.random.default_rng(H * W + C)
    img = r.normal(size=(2, C, H, W)).astype(np.float32)
    xs, ys = _axis_values(W), _axis_values(H)
    Ho, Wo = len(ys), len(xs)
    coords = np.empty((2, Ho, Wo, 2), np.float32)
    coords[0, ..., 0], coords[0, ..., 1] = xs[None, :], ys[:, None]
    coords[1, ..., 0] = r.uniform(-2, W + 1, size=(Ho, Wo))
    coords[1, ..., 1] = r.uniform(-2, H + 1, size=(Ho, Wo))
    out = torch.full((2 * C * Ho * Wo + 16,), SENT, device=DEV)
    mask = torch.full((2 * Ho * Wo + 16,), SENT, device=DEV)
    _call("raft_bilinear_sample", _dev(img), _dev(coords), out.data_ptr(), mask.data_ptr(), 2, C,
          H, W, Ho, Wo)
    got = _take(out, 2 * C * Ho * Wo).reshape(2, C, Ho, Wo)
    gm = _take(mask, 2 * Ho * Wo).reshape(2, Ho, Wo, 1)
    ref32, m32 = EO.bilinear_sampler(img, coords, torch.float32)
    ref64, _ = EO.bilinear_sampler(img, coords, torch.float64)
    bad = ~np.isfinite(coords).all(-1)
    assert np.isnan(ref32[np.broadcast_to(bad[:, None], ref32.shape)]).all()   # NaN / Inf coordinate -> NaN
    assert np.array_equal(np.isnan(got), np.isnan(ref32))
    assert np.array_equal(gm, m32)
    if W == 1:
        assert np.isnan(got).all()
        return
    assert np.array_equal(np.isnan(ref64), np.isnan(ref32))
    bound, e_ref = EO.measured_bound(ref32, ref64, 8 * EO.U * np.abs(img).max())
    ok = ~np.isnan(ref64)
    err = float(np.abs(got.astype(np.float64) - ref64)[ok].max())
    print(f"bilinear_sample {hw} C={C}: E_ref {e_ref:.3e} bound {bound:.3e} gpu err {err:.3e}; mask ones {int(gm.sum())}")
    assert err <= bound
    # integer coordinates read the pixel itself (2 y / (H - 1) rounds, so to the bound, not to the bit); the mask
    # is 0 on the border (g == +-1) and 1 strictly inside
    assert np.abs(got[0][:, :H, :W] - img[0]).max() <= bound
    assert np.array_equal(gm[0, :H, :W, 0], ((xs[None, :W] > 0) & (xs[None, :W] < W - 1) & (ys[:H, None] > 0)
                                             & (ys[:H, None] < H - 1)).astype(np.float32))
    # without a mask pointer the output is the same
    out2 = torch.full_like(out, SENT)
    _call("raft_bilinear_sample", _dev(img), _dev(coords), out2.data_ptr(), None, 2, C, H, W, Ho,
          Wo)
    assert np.array_equal(_take(out2, got.size), got.reshape(-1), equal_nan=True)


def _forward_interpolate(flow):
    """raft_forward_interpolate on flow [B, 2, H, W] (numpy float32) through the C entry."""
    b, _, h, w = flow.shape
    out = torch.full((flow.size + 16,), SENT, device=DEV)
    _call("raft_forward_interpolate", _dev(flow), out.data_ptr(), b, h, w)
    return _take(out, flow.size).reshape(flow.shape)


def _continuous(seed, h, w):
    r = np.random.default_rng(seed)
    f = (r.normal(size=(2, h, w)) * 3).astype(np.float32)
    if h == 1:
        f[1] = r.uniform(0.1, 0.9, size=(h, w))   # a one-row frame: only 0 < y + dy < 1 lands inside
    return f


@pytest.mark.parametrize("hw", [(13, 17), (16, 16), (1, 257), (24, 40)], ids=lambda s: "%dx%d" % s)
def test_forward_interpolate_continuous_flows(hw):
    """H*W below, at and one past the 256-target work-group, and 24 x 40; B = 2 with different flows.  On a
    continuous random flow no target has two sources at exactly the smallest distance (asserted on the fp64
    brute force), so every output is bit-equal to the reference's scipy result and to the brute force."""
    import elementwise_oracle as EO
    from oracle import raft_oracle as O
    flows = np.stack([_continuous(1, *hw), _continuous(2, *hw)])
    got = _forward_interpolate(flows)
    for i in range(2):
        dmin, members, _ = EO.nearest_sources(flows[i])
        assert np.isfinite(dmin).all() and (members.sum(1) == 1).all()
        assert np.array_equal(got[i], O.forward_interpolate(flows[i]))
        assert np.array_equal(got[i], EO.forward_interpolate_lowest(flows[i]))


def test_forward_interpolate_no_source_one_source_and_nonfinite():
    import elementwise_oracle as EO
    h, w = 9, 14
    away = np.full((2, h, w), 100.0, np.float32)            # every source leaves the frame: all zeros
    one = away.copy()
    one[:, 4, 9] = (0.25, -1.5)                              # one valid source only: its flow everywhere
    holes = _continuous(3, h, w)                             # NaN / Inf at some sources: never chosen
    holes[0, 2, 3] = np.nan
    holes[1, 5, 5] = np.nan
    holes[:, 7, 1] = (np.inf, 0.0)
    holes[:, 0, 13] = (0.0, -np.inf)
    got = _forward_interpolate(np.stack([away, one, holes]))
    assert np.array_equal(got[0], np.zeros_like(away))
    assert np.array_equal(got[1], np.broadcast_to(np.float32([0.25, -1.5])[:, None, None], (2, h, w)))
    dmin, members, _ = EO.nearest_sources(holes)
    assert (members.sum(1) == 1).all() and np.isfinite(dmin).all()
    want = EO.forward_interpolate_lowest(holes)              # the brute force, those sources excluded
    assert np.isfinite(want).all()
    assert np.array_equal(got[2], want)


@pytest.mark.parametrize("hw", [(13, 17), (24, 40)], ids=lambda s: "%dx%d" % s)
def test_forward_interpolate_ties_take_the_lowest_source_index(hw):
    """An integer-valued flow: about half the targets have several sources at exactly the smallest distance.
    Where there is no tie the output is bit-equal to the reference (scipy); where there is one, it is the flow of
    the lowest source index of the minimum set (include/raft_hip.h), whereas scipy's cKDTree picks an
    implementation-defined member.  The allowance is a condition, not a tolerance: only tied targets may deviate."""
    import elementwise_oracle as EO
    from oracle import raft_oracle as O
    h, w = hw
    flow = np.random.default_rng(h).integers(-3, 4, size=(2, h, w)).astype(np.float32)
    got = _forward_interpolate(flow[None])[0].reshape(2, -1)
    _, members, lowest = EO.nearest_sources(flow)
    tied = members.sum(1) > 1
    assert (lowest >= 0).all() and tied.any() and (~tied).any()
    ref = O.forward_interpolate(flow).reshape(2, -1)
    assert np.array_equal(got[:, ~tied], ref[:, ~tied])
    assert np.array_equal(got, flow.reshape(2, -1)[:, lowest])
    deviates = (got != ref).any(0)
    assert not deviates[~tied].any()
    print(f"forward_interpolate {hw}: {int(tied.sum())} of {tied.size} targets tied; differs from scipy on "
          f"{int(deviates.sum())}, all of them tied")


@pytest.mark.parametrize("form", ["vector", "scalar-length", "scalar-offset"])
def test_stream_carry_vector_and_scalar(form):
    """raft_stream_carry copies three segments exactly and writes nothing behind any of them.  How each kernel is
    forced: vector (float4) needs every length % 4 == 0 and every pointer 16-byte aligned; a segment length that
    is no multiple of 4 ('scalar-length') or one pointer offset by 4 bytes ('scalar-offset') takes the scalar
    kernel."""
    lens = (1001, 8, 12) if form == "scalar-length" else (1000, 8, 12)
    off = 1 if form == "scalar-offset" else 0
    r = np.random.default_rng(0)
    src = [_dev(r.normal(size=n + 4).astype(np.float32)) for n in lens]
    dst = [torch.full((n + 20,), SENT, device=DEV) for n in lens]
    ptr = lambda t, k: t.data_ptr() + (4 * off if k == 1 else 0)
    args = []
    for k in range(3):
        args += [ptr(src[k], k), ptr(dst[k], k), lens[k]]
    _call("raft_stream_carry", *args)
    for k in range(3):
        o = off if k == 1 else 0
        host = dst[k].cpu().numpy()
        assert np.array_equal(host[o:o + lens[k]], src[k].cpu().numpy()[o:o + lens[k]]), k
        assert np.all(host[:o] == SENT) and np.all(host[o + lens[k]:] == SENT), k
