"""RAFT.stream(bidirectional=True) / engine.BidiStreamPlan and utils.fb_consistency on the GPU.

The kernel tests hold raft_fb_consistency to the fp64 restatement of its definition in test_bidi_host.py
(fb_reference), within the fp32 rounding bound derived there.  The stream tests use test_gpu_stream.py's
conventions and helpers (seeded weights, smooth_images frames f0..f3, 128x192 and 123x181, ITERS = 4): what push
returns is what model(cat[prev, cur], cat[cur, prev]) returns, with every frame encoded once."""
import functools
import warnings

import numpy as np
import pytest
import torch

import test_bidi_host as R
import test_gpu_stream as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
ITERS = S.ITERS
FIELDS = ("low_fw", "up_fw", "low_bw", "up_bw", "occ_fw", "occ_bw", "err_fw", "err_bw")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


def fb(fw, bw, **kw):
    from raft_optical_flow_amd.utils import fb_consistency
    out = fb_consistency(fw, bw, **kw)
    torch.cuda.synchronize()
    assert [o.dtype for o in out] == [torch.bool, torch.bool, torch.float32, torch.float32]
    assert all(tuple(o.shape) == (fw.shape[0], 1) + tuple(fw.shape[2:]) for o in out)
    return [o[:, 0].cpu().numpy() for o in out]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def check_against_reference(got, fw, bw, cap=0.01):
    """err within the fp32 bound of the fp64 value; occ equal wherever the fp64 margin exceeds the bound; the
    pixels left out at most `cap` of the frame.  Returns the worst err ratio to its bound."""
    occ_fw, occ_bw, err_fw, err_bw = got
    worst = 0.0
    for d, occ, err in zip(R.fb_reference(fw, bw), (occ_fw, occ_bw), (err_fw, err_bw)):
        ins = d["inside"]
        assert np.all(np.isposinf(err[~ins])) and np.all(occ[~ins])
        assert np.all(np.isfinite(err[ins]))
        diff = np.abs(err.astype(np.float64)[ins] - d["err"][ins])
        ratio = float(np.max(diff / d["bound_err"][ins])) if ins.any() else 0.0
        worst = max(worst, ratio)
        assert ratio <= 1.0, ratio
        safe = ins & (np.abs(d["err"] - d["thr"]) > d["bound"])
        assert (ins & ~safe).sum() <= cap * ins.size
        assert np.array_equal(occ[safe], d["occ"][safe])
    return worst


# ----------------------------------------------------------------------------- the kernel


@pytest.mark.parametrize("shape", R.SHAPES)
def test_fb_zero_flows(shape):
    B, H, W = shape
    z = torch.zeros(B, 2, H, W, device=DEV)
    occ_fw, occ_bw, err_fw, err_bw = fb(z, z)
    assert not occ_fw.any() and not occ_bw.any()
    assert np.all(err_fw == 0) and np.all(err_bw == 0)


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("shift", [(2, 0), (0, -1), (-3, 2)])
def test_fb_integer_shifts(shape, shift):
    """bw = -fw, a whole-pixel shift: err is exactly 0 inside and the occluded band has the shift's width on
    the side each flow points to."""
    B, H, W = shape
    sx, sy = shift
    fw = torch.zeros(B, 2, H, W, device=DEV)
    fw[:, 0], fw[:, 1] = sx, sy
    occ_fw, occ_bw, err_fw, err_bw = fb(fw, -fw)
    x, y = np.arange(W)[None, None, :], np.arange(H)[None, :, None]

    def band(dx, dy):
        return np.broadcast_to((x + dx < 0) | (x + dx > W - 1) | (y + dy < 0) | (y + dy > H - 1), (B, H, W))
    assert np.array_equal(occ_fw, band(sx, sy)) and np.array_equal(occ_bw, band(-sx, -sy))
    for occ, err in ((occ_fw, err_fw), (occ_bw, err_bw)):
        assert np.all(err[~occ] == 0) and np.all(np.isposinf(err[occ]))
    assert int(occ_fw[0, H // 2].sum()) == min(abs(sx), W) and int(occ_fw[0, :, W // 2].sum()) == min(abs(sy), H)


def test_fb_targets_on_the_last_column_and_row_read_no_neighbour():
    """A target exactly on column W-1 or row H-1 is in the frame and takes the corner's value.  The flows are
    crops of buffers that hold NaN everywhere else, so a tap beyond the frame (one element further along the
    row, or one row down) would turn err into NaN.  Small integers and halves: every operation is exact."""
    B, H, W = 1, 6, 7
    big = [torch.full((B, 2, H + 2, W + 3), float("nan"), device=DEV) for _ in range(2)]
    fw, bw = (t[:, :, :H, :W] for t in big)
    x = torch.arange(W, device=DEV, dtype=torch.float32)[None, :].expand(H, W)
    y = torch.arange(H, device=DEV, dtype=torch.float32)[:, None].expand(H, W)
    fw[0, 0] = (W - 1) - x                 # every pixel of fw targets column W-1 ...
    fw[0, 1] = torch.where(y < H - 1, 0.5, 0.0)   # ... half-way between two rows (its own row on the last)
    bw[0, 0] = 0.0
    bw[0, 1] = (H - 1) - y                 # every pixel of bw targets row H-1, in its own column ...
    bw[0, 0, :, 3] = 2.5                   # ... but column 3: half-way between columns 5 and 6,
    bw[0, 0, :, W - 1] = -1.0 - (y[:, 0] % 4)   # and the last column: 1..4 columns to the left (the value fw samples)
    got = fb(fw, bw)
    f, b = fw.cpu().numpy(), bw.cpu().numpy()
    for d, occ, err in zip(R.fb_reference(f, b), got[:2], got[2:]):
        assert d["inside"].all() and np.all(np.isfinite(err))
        assert np.array_equal(err.astype(np.float64), d["err"]) and np.array_equal(occ, d["occ"])
    # the corner value itself: fw at (y, x) samples bw's x component on column W-1, rows y and y+1
    last, inner = b[0, :, :, -1:], np.arange(H)[:, None] < H - 1
    gx = np.where(inner, 0.5 * (last[0] + np.roll(last[0], -1, 0)), last[0])
    gy = np.where(inner, 0.5 * (last[1] + np.roll(last[1], -1, 0)), last[1])
    assert np.array_equal(got[2][0], (f[0, 0] + gx) ** 2 + (f[0, 1] + gy) ** 2)


def test_fb_non_finite_flows_are_occluded():
    B, H, W = 1, 9, 12
    fw0, bw0 = R.random_case(1, 37, 53)
    fw, bw = fw0[:, :, :H, :W].copy() * 0.2, bw0[:, :, :H, :W].copy() * 0.2
    fw[0, 0, 2, 3] = np.nan
    fw[0, 1, 4, 5] = np.inf
    fw[0, 0, 6, 7] = -np.inf
    fw[0, 1, 1, 1] = 3e38
    bw[0, 1, 5, 5] = np.nan
    bw[0, 0, 7, 2] = np.inf
    occ_fw, occ_bw, err_fw, err_bw = fb(dev(fw), dev(bw))
    for (yy, xx) in ((2, 3), (4, 5), (6, 7), (1, 1)):
        assert occ_fw[0, yy, xx] and np.isposinf(err_fw[0, yy, xx])
    assert occ_bw[0, 5, 5] and occ_bw[0, 7, 2] and np.isposinf(err_bw[0, 5, 5])
    dfw, dbw = R.fb_reference(fw, bw)
    # a fw pixel whose target taps a non-finite bw value (with weight > 0) is occluded; every other pixel is
    # what the reference says
    with np.errstate(invalid="ignore"):
        hit = ~np.isfinite(dfw["err"]) & dfw["inside"]
    assert np.all(occ_fw[hit])
    with np.errstate(invalid="ignore"):
        fine = np.isfinite(dfw["err"]) & (np.abs(dfw["err"] - dfw["thr"]) > dfw["bound"])
    assert np.array_equal(occ_fw[fine], dfw["occ"][fine])
    assert np.all(occ_fw[~dfw["inside"]]) and np.all(occ_bw[~dbw["inside"]])


@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 16, 260)])
def test_fb_pitched_and_non_contiguous_inputs(shape):
    """A crop of a larger tensor (pitch != width, odd offsets: every alignment of the 16-byte path and its scalar
    tail), a channel-last view (element stride != 1: copied once) and an expanded batch give the plain result."""
    B, H, W = shape
    fw, bw = R.random_case(*shape)
    plain = fb(dev(fw), dev(bw))
    for oy, ox, extra in ((1, 1, 2), (0, 4, 4), (3, 2, 1), (2, 3, 5)):
        bigs = [torch.full((B, 2, H + oy + 2, W + ox + extra), 1e6, device=DEV) for _ in range(2)]
        for t, a in zip(bigs, (fw, bw)):
            t[:, :, oy:oy + H, ox:ox + W] = dev(a)
        got = fb(bigs[0][:, :, oy:oy + H, ox:ox + W], bigs[1][:, :, oy:oy + H, ox:ox + W])
        assert all(np.array_equal(g, p) for g, p in zip(got, plain)), (oy, ox, extra)
    nhwc = [dev(a).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for a in (fw, bw)]
    assert not nhwc[0].is_contiguous()
    assert all(np.array_equal(g, p) for g, p in zip(fb(*nhwc), plain))
    one = fb(dev(fw[:1]).expand(3, -1, -1, -1), dev(bw[:1]).expand(3, -1, -1, -1))
    for g, p in zip(one, plain):
        assert all(np.array_equal(g[i], p[0]) for i in range(3))


@pytest.mark.parametrize("shape", R.SHAPES)
def test_fb_random_case_against_fp64(shape):
    """|err - err_fp64| <= 2^-24 (30 T sqrt(E) + 4 E) (T the largest tap, E the exact err: the derivation is
    test_bidi_host.bound_err's docstring), occ equal to the fp64 mask wherever the fp64 margin exceeds the bound
    of err and threshold together, and at most 1 % of the frame left out."""
    fw, bw = R.random_case(*shape)
    worst = check_against_reference(fb(dev(fw), dev(bw), alpha=0.01, beta=0.5), fw, bw)
    print(f"{shape}: worst |err - fp64| / bound = {worst:.3f}")


def test_fb_other_constants():
    fw, bw = R.random_case(2, 37, 53)
    got = fb(dev(fw), dev(bw), alpha=0.05, beta=2.0)
    a = float(np.float32(0.05))
    for d, occ in zip(R.fb_reference(fw, bw, a, 2.0), got[:2]):
        safe = d["inside"] & (np.abs(d["err"] - d["thr"]) > 10 * d["bound"])
        assert np.array_equal(occ[safe], d["occ"][safe])
    assert not np.array_equal(got[0], fb(dev(fw), dev(bw))[0])


# ----------------------------------------------------------------------------- the stream


def run_bidi(m, seq, iters=ITERS, warm=False, to=lambda x: x.to(DEV), **kw):
    outs, inits = [], []
    with torch.no_grad(), m.stream(iters=iters, warm_start=warm, bidirectional=True, **kw) as s:
        for i, f in enumerate(seq):
            o = s.push(to(f))
            assert (o is None) == (i == 0)
            if o is not None:
                assert o._fields == FIELDS
                outs.append(o)
                inits.append(s.last_flow_init)
    torch.cuda.synchronize()
    return outs, inits


def pairwise(m, a, b, iters=ITERS, flow_init=None, mode="sintel"):
    """The batched pairwise call the stream must equal: model(cat[pad a, pad b], cat[pad b, pad a]) + unpad ->
    (low_fw, up_fw, low_bw, up_bw)."""
    pa, p = S.pad_cpu(a, mode)
    pb, _ = S.pad_cpu(b, mode)
    n = a.shape[0]
    with torch.no_grad():
        low, up = m(torch.cat([pa, pb]).to(DEV), torch.cat([pb, pa]).to(DEV), iters=iters, flow_init=flow_init,
                    test_mode=True)
    up = S.unpad(up, p)
    return low[:n], up[:n], low[n:], up[n:]


def flows_err(o, ref):
    return max(S.maxabs(x, y) for x, y in zip(o[:4], ref))


@functools.lru_cache(maxsize=None)
def oracle_pair_bw(H, W, k, small=False, alternate=False, iters=ITERS):
    """The numpy oracle on the padded frames (f_k+1, f_k): the backward direction of pair k."""
    from oracle import raft_oracle as O
    f = S.frames(1, H, W)
    a, p = S.pad_cpu(f[k + 1])
    b, _ = S.pad_cpu(f[k])
    par = {n: v.numpy() for n, v in S.weights(small).items()}
    low, up = O.raft_forward(par, a.numpy(), b.numpy(), iters=iters, small=small, alternate_corr=alternate)
    return low, S.unpad(up, p)


@pytest.fixture(scope="module")
def model():
    return S.make_model()


@pytest.fixture(scope="module")
def cold(model):
    """The cold bidirectional stream over f0..f3 at 128x192 (hipGraph replay from the second pair on)."""
    return run_bidi(model, S.frames(1, 128, 192))[0]


def test_each_step_matches_the_oracle_in_both_directions(cold):
    assert len(cold) == 3
    for k, o in enumerate(cold):
        assert tuple(o.low_fw.shape) == tuple(o.low_bw.shape) == (1, 2, 16, 24)
        assert tuple(o.up_fw.shape) == tuple(o.up_bw.shape) == (1, 2, 128, 192)
        assert tuple(o.occ_fw.shape) == tuple(o.err_bw.shape) == (1, 1, 128, 192)
        assert o.occ_fw.dtype == o.occ_bw.dtype == torch.bool and o.err_fw.dtype == torch.float32
        rf, rb = S.oracle_pair(128, 192, k), oracle_pair_bw(128, 192, k)
        e = (S.maxabs(o.low_fw, rf[0]), S.maxabs(o.up_fw, rf[1]), S.maxabs(o.low_bw, rb[0]), S.maxabs(o.up_bw, rb[1]))
        print(f"pair {k}: bidi stream vs oracle max-abs low_fw {e[0]:.3e} up_fw {e[1]:.3e} low_bw {e[2]:.3e} "
              f"up_bw {e[3]:.3e}")
        assert max(e) <= 1e-3, (k, e)


def test_each_step_matches_the_batched_pairwise_call(model, cold):
    f = S.frames(1, 128, 192)
    worst = max(flows_err(o, pairwise(model, f[k], f[k + 1])) for k, o in enumerate(cold))
    print(f"bidi stream vs batched pairwise max-abs {worst:.3e}")
    assert worst < 1e-4, worst


def test_forward_half_is_the_one_directional_stream(model, cold):
    uni = S.run_stream(model, S.frames(1, 128, 192))[0]
    worst = max(max(S.maxabs(o.low_fw, u[0]), S.maxabs(o.up_fw, u[1])) for o, u in zip(cold, uni))
    print(f"bidi forward half vs one-directional stream max-abs {worst:.3e}")
    assert worst < 1e-4, worst


def test_carry_is_lossless(model, cold):
    """All eight fields, bit for bit: a carried context (the GRU's initial hidden state in particular) that went
    stale or was overwritten by the loop would differ from a freshly primed one."""
    f = S.frames(1, 128, 192)
    (fresh12,) = run_bidi(model, f[1:3])[0]
    assert S.equal(cold[1], fresh12)
    (fresh23,) = run_bidi(model, f[2:4])[0]
    assert S.equal(cold[2], fresh23)
    with torch.no_grad(), model.stream(iters=ITERS, bidirectional=True) as s:
        assert s.push(f[0].to(DEV)) is None
        first = s.push(f[1].to(DEV))
        s.reset()
        assert s.push(f[1].to(DEV)) is None
        after = s.push(f[2].to(DEV))
        again = s.push(f[3].to(DEV))
    assert S.equal(first, cold[0]) and S.equal(after, cold[1]) and S.equal(again, cold[2])
    assert not torch.equal(cold[1].low_bw, cold[2].low_bw)


def test_graph_equals_eager(cold):
    m = S.make_model()
    m.hip_graph = False
    eager = run_bidi(m, S.frames(1, 128, 192))[0]
    for a, b in zip(cold, eager):
        assert S.equal(a, b)


@pytest.mark.parametrize("mode", ["sintel", "kitti"])
def test_masks_are_the_op_on_the_returned_flows(model, mode):
    """123x181 (pads [1,2,2,3] / [1,2,0,5]), uint8 frames: the step's masks and residuals, computed in place on
    the padded buffer, equal fb_consistency of the unpadded flows it returns, bit for bit; the flows equal the
    batched pairwise call.  (Seeded weights give two flows of a few pixels that do not agree: the published
    constants call nearly every pixel occluded.  The second mode therefore runs alpha = 0 and beta = the median
    residual of pair 0 under the default constants, which splits pair 0 in half by construction and makes the
    mask a plain threshold of the returned residual.)"""
    from raft_optical_flow_amd.utils import fb_consistency
    f = S.frames(1, 123, 181)
    u8 = [x.permute(0, 2, 3, 1).contiguous().to(torch.uint8) for x in f[:3]]
    consts = {}
    if mode != "sintel":
        e0 = run_bidi(model, u8[:2], pad_mode=mode)[0][0].err_fw
        consts = {"fb_alpha": 0.0, "fb_beta": float(e0[e0.isfinite()].median())}
    outs, _ = run_bidi(model, u8, pad_mode=mode, **consts)
    for k, o in enumerate(outs):
        assert tuple(o.low_fw.shape) == (1, 2, 16, 23) and tuple(o.up_bw.shape) == (1, 2, 123, 181)
        assert tuple(o.occ_fw.shape) == tuple(o.err_bw.shape) == (1, 1, 123, 181)
        want = fb_consistency(o.up_fw, o.up_bw, **{n[3:]: v for n, v in consts.items()})
        assert S.equal((o.occ_fw, o.occ_bw, o.err_fw, o.err_bw), want)
        assert flows_err(o, pairwise(model, f[k], f[k + 1], mode=mode)) < 1e-4
        frac = (float(o.occ_fw.float().mean()), float(o.occ_bw.float().mean()))
        finite = float(o.err_fw.isfinite().float().mean())
        print(f"{mode} pair {k}: occluded fw {frac[0]:.3f} bw {frac[1]:.3f}, finite err {finite:.3f}")
        assert finite > 0.5                                        # most targets stay in the frame
        if consts:
            for occ, err in ((o.occ_fw, o.err_fw), (o.occ_bw, o.err_bw)):
                assert torch.equal(occ, (err > consts["fb_beta"]) | ~err.isfinite())
            assert k > 0 or 0.4 < frac[0] < 0.6, frac
    if mode == "sintel":
        rf, rb = S.oracle_pair(123, 181, 0), oracle_pair_bw(123, 181, 0)
        e = max(S.maxabs(outs[0].low_fw, rf[0]), S.maxabs(outs[0].up_fw, rf[1]), S.maxabs(outs[0].low_bw, rb[0]),
                S.maxabs(outs[0].up_bw, rb[1]))
        assert e <= 1e-3, e


def test_warm_start(model, cold):
    from oracle import raft_oracle as O
    f = S.frames(1, 128, 192)
    outs, inits = run_bidi(model, f, warm=True)
    assert S.equal(outs[0], cold[0])                       # zero flow interpolates to zero
    assert tuple(inits[0].shape) == (2, 2, 16, 24) and float(inits[0].abs().max()) == 0.0
    for k in (1, 2):
        init = inits[k]
        # each direction from its own direction's flow of the step before; the forward half first
        assert np.array_equal(init[0].cpu().numpy(), O.forward_interpolate(outs[k - 1].low_fw[0].cpu().numpy()))
        assert np.array_equal(init[1].cpu().numpy(), O.forward_interpolate(outs[k - 1].low_bw[0].cpu().numpy()))
        e = flows_err(outs[k], pairwise(model, f[k], f[k + 1], flow_init=init))
        print(f"warm pair {k}: bidi stream vs batched pairwise with that flow_init max-abs {e:.3e}")
        assert e < 1e-4, (k, e)
    assert not torch.equal(outs[1].low_fw, cold[1].low_fw) and not torch.equal(outs[1].low_bw, cold[1].low_bw)


def test_lockstep_batch(model):
    f2 = S.frames(2, 128, 192)
    both, _ = run_bidi(model, f2[:3], to=lambda x: x)
    for slot in range(2):
        own, _ = run_bidi(model, [x[slot:slot + 1] for x in f2[:3]])
        for k in range(2):
            e = max(S.maxabs(getattr(both[k], n)[slot:slot + 1], getattr(own[k], n)) for n in FIELDS[:4])
            print(f"slot {slot} pair {k}: B=2 vs B=1 max-abs {e:.3e}")
            assert e < 1e-4, (slot, k, e)
            assert tuple(both[k].occ_bw.shape) == (2, 1, 128, 192)
    assert S.maxabs(both[0].low_bw[0], both[0].low_bw[1]) > 1e-2


def test_weights_change_mid_stream():
    f = S.frames(1, 128, 192)
    m = S.make_model()
    with torch.no_grad(), m.stream(iters=ITERS, bidirectional=True) as s:
        s.push(f[0].to(DEV))
        s.push(f[1].to(DEV))
        m.update_block.gru.convz1.weight.mul_(1.5)
        m.cnet.conv2.weight.mul_(1.25)             # the carried context is stale too
        got = s.push(f[2].to(DEV))
        then = s.push(f[3].to(DEV))
    fresh, _ = run_bidi(m, f[1:4])                 # built after the edit
    assert S.equal(got, fresh[0]) and S.equal(then, fresh[1])
    unchanged, _ = run_bidi(S.make_model(), f[1:3])
    assert not torch.equal(got.low_bw, unchanged[0].low_bw)


def test_range_guard():
    """fnet's head scaled so |fmap| > 65504, as test_gpu_stream.test_range_guard: every step is flagged, warns
    once and returns the exact-f32 re-run of BOTH directions, with the masks recomputed from those flows."""
    from raft_optical_flow_amd.utils import fb_consistency
    f = S.frames(1, 128, 192)
    m = S.make_model()
    ref = S.make_model(precision="fp32")
    for mm in (m, ref):
        with torch.no_grad():
            mm.fnet.conv2.weight.mul_(20000.0)
            mm.fnet.conv2.bias.mul_(20000.0)
    with torch.no_grad(), m.stream(iters=ITERS, warm_start=True, bidirectional=True) as s:
        assert s.push(f[0].to(DEV)) is None
        for k in (1, 2):
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                o = s.push(f[k].to(DEV))
            assert len([x for x in w if "range guard" in str(x.message)]) == 1
            want = pairwise(ref, f[k - 1], f[k], flow_init=s.last_flow_init)
            assert S.equal(o[:4], want)
            assert S.equal(o[4:], fb_consistency(o.up_fw, o.up_bw))
    m.range_guard = "raise"
    with torch.no_grad(), m.stream(iters=ITERS, bidirectional=True) as s:
        s.push(f[0].to(DEV))
        with pytest.raises(FloatingPointError):
            s.push(f[1].to(DEV))


def test_step_launch_list(model):
    """Both directions at the encoder cost of one: no more fnet / cnet launches than the one-directional step
    (every launch ahead of the refinement but the correlation build), one consistency launch closing the step."""
    from raft_optical_flow_amd.engine import BidiStreamPlan, StreamPlan
    device = torch.device(DEV, torch.cuda.current_device())
    pk = model.packed(device)
    uni = StreamPlan(pk, 1, 123, 181, 2, warm_start=True, device=device)
    bi = BidiStreamPlan(pk, 1, 123, 181, 2, warm_start=True, device=device)
    nu, nb = uni.kernel_names(), bi.kernel_names()
    head = lambda n: n[:n.index("raft_init_coords")]  # noqa: E731
    for name in ("raft_conv2d", "raft_instnorm_apply", "raft_instnorm_merge_fused", "raft_instnorm_stats"):
        assert head(nb).count(name) <= head(nu).count(name), name
    assert head(nu).count("raft_conv2d") > 20          # (the trunks are what is being counted)
    assert nb.count("raft_fb_consistency") == 1 and nb[-1] == "raft_fb_consistency"
    assert nb[:2] == ["raft_stream_carry_n", "raft_ingest_frame"] and nb.count("raft_ingest_frame") == 1
    assert nb.count("raft_stream_carry_n") == 2 and nb.count("raft_forward_interpolate") == 1
    assert "raft_stream_carry" not in nb and "raft_prep_images" not in nb
    # the refinement is the shared helper's, launch for launch
    tail = lambda n: n[n.index("raft_init_coords"):n.index("raft_flow_from_coords") + 1]  # noqa: E731
    assert tail(nb) == tail(nu)
    assert nu[:2] == ["raft_stream_carry", "raft_ingest_frame"] and "raft_fb_consistency" not in nu
    uni.release()
    bi.release()


@pytest.mark.parametrize("variant", ["small", "alternate", "fp32"])
def test_variants_match_the_batched_pairwise_call(variant):
    m = S.make_model(small=variant == "small", alternate=variant == "alternate",
                     precision="fp32" if variant == "fp32" else None)
    f = S.frames(1, 128, 192)
    iters = 2 if variant == "alternate" else ITERS
    outs, _ = run_bidi(m, f[:3], iters=iters)
    for k, o in enumerate(outs):
        e = flows_err(o, pairwise(m, f[k], f[k + 1], iters=iters))
        print(f"{variant} pair {k}: bidi stream vs batched pairwise max-abs {e:.3e}")
        assert e < 1e-4, (variant, k, e)


def test_lifecycle_and_errors():
    f = S.frames(1, 128, 192)
    m = S.make_model()
    s = m.stream(iters=ITERS, bidirectional=True)
    with torch.no_grad():
        s.push(f[0].to(DEV))
        assert s.push(f[1].to(DEV)) is not None
        with pytest.raises(ValueError, match=r"\(1, 3, 128, 192\).*\(1, 3, 120, 192\)"):
            s.push(f[0][:, :, :120].contiguous().to(DEV))
        with pytest.raises(ValueError, match="uint8"):
            s.push(torch.zeros(1, 128, 192, 3, dtype=torch.uint8, device=DEV))
        assert s.push(f[2].to(DEV)) is not None       # the stream survives a refused frame
    s.close()
    s.close()
    with pytest.raises(RuntimeError, match="close"):
        s.push(f[0].to(DEV))
