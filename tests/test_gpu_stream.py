"""RAFT.stream / engine.StreamPlan on the GPU: every frame of a video is encoded once, and what push()
returns is what RAFT.forward returns for (previous frame, this frame).

One 4-frame sequence f0..f3 = smooth_images(..., shift=(3k, -2k))[1], k = 0..3, seeded weights, iters <= 4:
the inputs the parity tests and smoke() hold to 1e-3 against the numpy oracle without tripping the range guard.
The oracle results are computed once per pair and shared."""
import argparse
import functools
import gc
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ITERS = 4
SEED = 3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


def maxabs(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))


def equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def weights(small=False):
    from raft_optical_flow_amd import RAFT
    from raft_optical_flow_amd.init import seeded_state_dict
    m = RAFT(argparse.Namespace(small=small, mixed_precision=False, alternate_corr=False))
    return seeded_state_dict(m, 0)


def make_model(small=False, alternate=False, precision=None):
    from raft_optical_flow_amd import RAFT
    m = RAFT(argparse.Namespace(small=small, mixed_precision=False, alternate_corr=alternate))
    m.conv_precision = precision
    m.load_state_dict(weights(small))
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def frames(B, H, W):
    """f0..f3, float32 [B,3,H,W] on the CPU (integer values 0..255)."""
    from raft_optical_flow_amd.init import smooth_images
    return tuple(smooth_images(B, H, W, seed=SEED, shift=(3.0 * k, -2.0 * k))[1] for k in range(4))


def pad_cpu(x, mode="sintel"):
    """InputPadder.pad on the CPU (torch's own replicate padding)."""
    from raft_optical_flow_amd import InputPadder
    p = InputPadder(x.shape, mode)._pad
    return torch.nn.functional.pad(x, p, mode="replicate"), p


def unpad(x, p):
    h, w = x.shape[-2:]
    return x[..., p[2]:h - p[3], p[0]:w - p[1]]


@functools.lru_cache(maxsize=None)
def oracle_pair(H, W, k, small=False, alternate=False, iters=ITERS):
    """The numpy oracle on the padded frames (f_k, f_k+1), cold start; flow_up unpadded."""
    from oracle import raft_oracle as O
    f = frames(1, H, W)
    a, p = pad_cpu(f[k])
    b, _ = pad_cpu(f[k + 1])
    par = {n: v.numpy() for n, v in weights(small).items()}
    low, up = O.raft_forward(par, a.numpy(), b.numpy(), iters=iters, small=small, alternate_corr=alternate)
    return low, unpad(up, p)


def run_stream(m, seq, iters=ITERS, warm=False, to=lambda x: x.to(DEV), **kw):
    """Push a sequence through a fresh stream: [(flow_low, flow_up)] per pair and last_flow_init per pair."""
    outs, inits = [], []
    with torch.no_grad(), m.stream(iters=iters, warm_start=warm, **kw) as s:
        for i, f in enumerate(seq):
            o = s.push(to(f))
            assert (o is None) == (i == 0)
            if o is not None:
                outs.append(o)
                inits.append(s.last_flow_init)
    torch.cuda.synchronize()
    return outs, inits


@pytest.fixture(scope="module")
def model():
    return make_model()


@pytest.fixture(scope="module")
def cold(model):
    """The cold stream over f0..f3 at 128x192 (f16x3, hipGraph replay from the second pair on)."""
    return run_stream(model, frames(1, 128, 192))[0]


# ----------------------------------------------------------------------------- 1. ingest


@pytest.mark.parametrize("hw", [(123, 181), (128, 192)])
@pytest.mark.parametrize("mode", ["sintel", "kitti"])
@pytest.mark.parametrize("B", [1, 2])
def test_ingest_is_exact(hw, mode, B):
    """raft_ingest_frame == InputPadder.pad + 2 * (x / 255) - 1, bit for bit, from float NCHW and uint8 NHWC."""
    from raft_optical_flow_amd import InputPadder
    from raft_optical_flow_amd.utils import ingest_frame
    H, W = hw
    g = torch.Generator().manual_seed(H * 1000 + W + B)
    u8 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    x = u8.permute(0, 3, 1, 2).float().contiguous()
    padded_ref, p = pad_cpu(x, mode)
    if hw == (123, 181):
        assert p == ([1, 2, 2, 3] if mode == "sintel" else [1, 2, 0, 5])
    else:
        assert p == [0, 0, 0, 0]
    rows_ref = (2 * (padded_ref / 255.0) - 1.0).permute(0, 2, 3, 1).reshape(-1, 3)
    (pad_gpu,) = InputPadder(x.shape, mode).pad(x.to(DEV))
    assert torch.equal(pad_gpu.cpu(), padded_ref)
    for frame in (x.to(DEV), u8.to(DEV), u8):
        rows, padded, pad = ingest_frame(frame, mode)
        assert pad == InputPadder(x.shape, mode)._pad == p
        assert rows.is_cuda and padded.is_cuda and rows.dtype == padded.dtype == torch.float32
        assert tuple(padded.shape) == tuple(padded_ref.shape) and tuple(rows.shape) == tuple(rows_ref.shape)
        assert torch.equal(padded.cpu(), padded_ref)
        assert torch.equal(padded, pad_gpu)
        assert torch.equal(rows.cpu(), rows_ref)


# ----------------------------------------------------------------------------- 2-5. the steps


def test_each_step_matches_the_oracle(cold):
    assert len(cold) == 3
    for k, (low, up) in enumerate(cold):
        rlow, rup = oracle_pair(128, 192, k)
        assert tuple(low.shape) == (1, 2, 16, 24) and tuple(up.shape) == (1, 2, 128, 192)
        e = (maxabs(low, rlow), maxabs(up, rup))
        print(f"pair {k}: stream vs oracle max-abs low {e[0]:.3e} up {e[1]:.3e}")
        assert e[0] <= 1e-3 and e[1] <= 1e-3, (k, e)


def test_each_step_matches_the_pairwise_path(model, cold):
    """fnet over one image may tile differently from fnet over two: the bound is the one
    test_gpu_configs.py uses for that cause, not bit-equality."""
    f = frames(1, 128, 192)
    worst = 0.0
    for k, (low, up) in enumerate(cold):
        with torch.no_grad():
            plow, pup = model(f[k].to(DEV), f[k + 1].to(DEV), iters=ITERS, test_mode=True)
        e = max(maxabs(low, plow), maxabs(up, pup))
        print(f"pair {k}: stream vs pairwise max-abs {e:.3e}")
        worst = max(worst, e)
    assert worst < 1e-4, worst


def test_state_carry_is_lossless(model, cold):
    f = frames(1, 128, 192)
    (fresh12,) = run_stream(model, f[1:3])[0]          # a fresh stream fed f1, f2
    assert equal(cold[1], fresh12)
    (fresh23,) = run_stream(model, f[2:4])[0]          # both roles of the carry: pair (f2, f3)
    assert equal(cold[2], fresh23)
    with torch.no_grad(), model.stream(iters=ITERS) as s:
        assert s.push(f[0].to(DEV)) is None
        first = s.push(f[1].to(DEV))
        s.reset()                                      # a sequence boundary in the middle of a stream
        assert s.push(f[1].to(DEV)) is None
        after = s.push(f[2].to(DEV))
        again = s.push(f[3].to(DEV))
    assert equal(first, cold[0]) and equal(after, cold[1]) and equal(again, cold[2])


def test_graph_equals_eager(cold):
    m = make_model()
    m.hip_graph = False
    eager = run_stream(m, frames(1, 128, 192))[0]
    for a, b in zip(cold, eager):
        assert equal(a, b)


# ----------------------------------------------------------------------------- 6. warm start


def test_warm_start(model, cold):
    from oracle import raft_oracle as O
    f = frames(1, 128, 192)
    outs, inits = run_stream(model, f, warm=True)
    # zero flow interpolates to zero and coords0 + 0 == coords0: the first warm pair is the cold one
    assert equal(outs[0], cold[0])
    assert float(inits[0].abs().max()) == 0.0
    par = {n: v.numpy() for n, v in weights().items()}
    for k in (1, 2):
        init = inits[k].cpu().numpy()
        want = O.forward_interpolate(outs[k - 1][0][0].cpu().numpy())
        assert np.array_equal(init[0], want)
        a, b = pad_cpu(f[k])[0], pad_cpu(f[k + 1])[0]
        rlow, rup = O.raft_forward(par, a.numpy(), b.numpy(), iters=ITERS, flow_init=init)
        e = (maxabs(outs[k][0], rlow), maxabs(outs[k][1], rup))
        print(f"warm pair {k}: stream vs oracle max-abs low {e[0]:.3e} up {e[1]:.3e}")
        assert e[0] <= 1e-3 and e[1] <= 1e-3, (k, e)
    assert not torch.equal(outs[1][0], cold[1][0])


# ----------------------------------------------------------------------------- shapes, precisions, variants


def test_odd_size_uint8_frames_both_pad_modes(model):
    """123x181 (pads [1,2,2,3]), frames delivered as uint8 NHWC; flow_up comes back at the frame's size."""
    f = frames(1, 123, 181)
    u8 = [x.permute(0, 2, 3, 1).contiguous().to(torch.uint8) for x in f[:3]]
    outs, _ = run_stream(model, u8)
    for k, (low, up) in enumerate(outs):
        assert tuple(low.shape) == (1, 2, 16, 23) and tuple(up.shape) == (1, 2, 123, 181)
        rlow, rup = oracle_pair(123, 181, k)
        e = (maxabs(low, rlow), maxabs(up, rup))
        print(f"123x181 pair {k}: stream vs oracle max-abs low {e[0]:.3e} up {e[1]:.3e}")
        assert e[0] <= 1e-3 and e[1] <= 1e-3, (k, e)
        a, p = pad_cpu(f[k])
        b, _ = pad_cpu(f[k + 1])
        with torch.no_grad():
            plow, pup = model(a.to(DEV), b.to(DEV), iters=ITERS, test_mode=True)
        assert max(maxabs(low, plow), maxabs(up, unpad(pup, p))) < 1e-4
    # the bottom-pad rule (any other mode), float frames: equals the pairwise path on InputPadder's padding
    (o,), _ = run_stream(model, f[:2], pad_mode="kitti")
    a, p = pad_cpu(f[0], "kitti")
    b, _ = pad_cpu(f[1], "kitti")
    assert p == [1, 2, 0, 5]
    with torch.no_grad():
        plow, pup = model(a.to(DEV), b.to(DEV), iters=ITERS, test_mode=True)
    assert max(maxabs(o[0], plow), maxabs(o[1], unpad(pup, p))) < 1e-4


def test_fp32_precision():
    m = make_model(precision="fp32")
    outs, _ = run_stream(m, frames(1, 128, 192))
    for k, (low, up) in enumerate(outs):
        rlow, rup = oracle_pair(128, 192, k)
        assert maxabs(low, rlow) <= 1e-3 and maxabs(up, rup) <= 1e-3


def test_raft_small():
    m = make_model(small=True)
    outs, _ = run_stream(m, frames(1, 128, 192)[:3])
    for k, (low, up) in enumerate(outs):
        rlow, rup = oracle_pair(128, 192, k, small=True)
        assert maxabs(low, rlow) <= 1e-3 and maxabs(up, rup) <= 1e-3
    with torch.no_grad():
        plow, pup = m(frames(1, 128, 192)[1].to(DEV), frames(1, 128, 192)[2].to(DEV), iters=ITERS, test_mode=True)
    assert max(maxabs(outs[1][0], plow), maxabs(outs[1][1], pup)) < 1e-4


def test_alternate_corr():
    m = make_model(alternate=True)
    outs, _ = run_stream(m, frames(1, 128, 192)[:3], iters=2)
    for k, (low, up) in enumerate(outs):
        rlow, rup = oracle_pair(128, 192, k, alternate=True, iters=2)
        assert maxabs(low, rlow) <= 1e-3 and maxabs(up, rup) <= 1e-3


# ----------------------------------------------------------------------------- 7. lockstep batch


def test_lockstep_batch(model):
    """B = 2 is two independent streams in lockstep (frames handed over as CPU tensors: the stream stages them)."""
    f2 = frames(2, 128, 192)
    both, _ = run_stream(model, f2[:3], to=lambda x: x)
    for slot in range(2):
        own, _ = run_stream(model, [x[slot:slot + 1] for x in f2[:3]])
        for k in range(2):
            e = max(maxabs(both[k][0][slot:slot + 1], own[k][0]), maxabs(both[k][1][slot:slot + 1], own[k][1]))
            print(f"slot {slot} pair {k}: B=2 vs B=1 max-abs {e:.3e}")
            assert e < 1e-4, (slot, k, e)
    assert maxabs(both[0][0][0], both[0][0][1]) > 1e-2  # the two sequences really differ


# ----------------------------------------------------------------------------- 8. range guard


def test_range_guard():
    """fnet's head scaled so |fmap| > 65504 (as test_f16x3_range_guard_falls_back_to_fp32): every step is
    flagged, warns once and returns the exact-f32 result; the next warm start begins from the corrected flow."""
    from oracle import raft_oracle as O
    f = frames(1, 128, 192)
    m = make_model()
    ref = make_model(precision="fp32")
    for mm in (m, ref):
        with torch.no_grad():
            mm.fnet.conv2.weight.mul_(20000.0)
            mm.fnet.conv2.bias.mul_(20000.0)
    rout, rinit = run_stream(ref, f[:3], warm=True)
    assert m.range_guard == "fallback"
    with torch.no_grad(), m.stream(iters=ITERS, warm_start=True) as s:
        assert s.push(f[0].to(DEV)) is None
        outs = []
        for k in (1, 2):
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                outs.append(s.push(f[k].to(DEV)))
            assert len([x for x in w if "range guard" in str(x.message)]) == 1
            e = (maxabs(outs[-1][0], rout[k - 1][0]), maxabs(outs[-1][1], rout[k - 1][1]))
            print(f"guarded pair {k - 1}: stream fallback vs fp32 stream max-abs low {e[0]:.3e} up {e[1]:.3e}")
            assert e == (0.0, 0.0), e
        want = O.forward_interpolate(outs[0][0][0].cpu().numpy())
        assert np.array_equal(s.last_flow_init[0].cpu().numpy(), want)
    m.range_guard = "raise"
    with torch.no_grad(), m.stream(iters=ITERS) as s:
        s.push(f[0].to(DEV))
        with pytest.raises(FloatingPointError):
            s.push(f[1].to(DEV))


# ----------------------------------------------------------------------------- 9. weights change mid-stream


def test_weights_change_mid_stream():
    f = frames(1, 128, 192)
    m = make_model()
    with torch.no_grad(), m.stream(iters=ITERS) as s:
        s.push(f[0].to(DEV))
        before = s.push(f[1].to(DEV))
        m.update_block.gru.convz1.weight.mul_(1.5)
        got = s.push(f[2].to(DEV))
        then = s.push(f[3].to(DEV))
    fresh, _ = run_stream(m, f[1:4])  # built after the edit
    assert equal(got, fresh[0]) and equal(then, fresh[1])
    unchanged, _ = run_stream(make_model(), f[1:3])
    assert not torch.equal(got[0], unchanged[0][0])  # the edit matters


# ----------------------------------------------------------------------------- 10. lifecycle and errors


def test_lifecycle_and_errors():
    f = frames(1, 128, 192)
    m = make_model()
    run_stream(m, f[:3])   # packs the weights and their lazily made forms: they belong to the model
    n_plans = len(m._plans)
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    s = m.stream(iters=ITERS)
    with torch.no_grad():
        s.push(f[0].to(DEV))
        o1 = s.push(f[1].to(DEV))
        o2 = s.push(f[2].to(DEV))      # replays the captured graph
        with pytest.raises(ValueError, match=r"\(1, 3, 128, 192\).*\(1, 3, 120, 192\)"):
            s.push(f[0][:, :, :120].contiguous().to(DEV))
        with pytest.raises(ValueError, match="uint8"):
            s.push(torch.zeros(1, 128, 192, 3, dtype=torch.uint8, device=DEV))
    assert len(m._plans) == n_plans
    m.release_plans()                   # not the stream's plan
    with torch.no_grad():
        assert s.push(f[3].to(DEV)) is not None
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - base
    assert held > (1 << 20), held       # the plan's buffers are visible to this measure
    s.close()
    s.close()                           # idempotent
    with pytest.raises(RuntimeError, match="close"):
        s.push(f[0].to(DEV))
    del o1, o2
    gc.collect()
    torch.cuda.synchronize()
    left = torch.cuda.memory_allocated() - base
    # Nothing of the plan may survive close().  The allowance is 64 KiB: the caching allocator rounds every
    # tensor to 512 B, so a handful of few-byte tensors torch itself may keep (a graph's generator state) fit
    # in it many times over, while the smallest buffer of the plan that matters, one 16x24 feature map
    # (384 rows x 256 floats = 384 KiB), does not.
    print(f"stream plan held {held} B, {left} B left after close()")
    assert left <= 64 * 1024, left
    m.train()
    with pytest.raises(NotImplementedError, match="inference path"):
        m.stream()


def test_step_launch_list(model):
    """The stream's kernels are the plan's own: one ingest, one carry, fnet over ONE image per step."""
    from raft_optical_flow_amd.engine import StreamPlan
    pk = model.packed(torch.device(DEV, torch.cuda.current_device()))
    sp = StreamPlan(pk, 1, 123, 181, 2, warm_start=True, device=torch.device(DEV, torch.cuda.current_device()))
    names = sp.kernel_names()
    assert names[:2] == ["raft_stream_carry", "raft_ingest_frame"]
    assert names.count("raft_forward_interpolate") == 1 and "raft_prep_images" not in names
    assert names[-1] == "raft_flow_from_coords" and (sp.Hp, sp.Wp) == (128, 184)
    rp = model.plan(1, 128, 184, 2, True, True)
    # the refinement is the shared helper's: launch for launch the pairwise plan's
    tail = lambda n: n[n.index("raft_init_coords"):]  # noqa: E731
    assert tail(names) == tail(rp.kernel_names())
    sp.release()
    model.release_plans()
