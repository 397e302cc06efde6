"""The video-stream additions that need no GPU: the new C-ABI entries are exported and prototyped, report
argument errors before any launch, and FlowStream checks its arguments on the host."""
import argparse
import ctypes

import pytest

from raft_optical_flow_amd import _lib

FAKE = 1 << 20  # 16-byte aligned stand-in pointers: an argument error returns before any launch


def test_stream_symbols_are_exported_and_prototyped():
    lib = _lib.load()
    for name in ("raft_ingest_frame", "raft_stream_carry", "raft_frame_pad"):
        assert name in _lib.EXPORTED
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.raft_hip_abi_version() == 19  # additive entries: the ABI version did not move
    assert (_lib.FRAME_F32_NCHW, _lib.FRAME_U8_NHWC) == (0, 1)


def _err(lib):
    return lib.raft_hip_last_error()


def test_ingest_frame_argument_errors():
    lib = _lib.load()
    a, b, c = FAKE, 2 * FAKE, 3 * FAKE
    for args in ((None, 0, 1, 8, 8, 1, b, c), (a, 0, 1, 8, 8, 1, None, c), (a, 0, 1, 8, 8, 1, b, None)):
        assert lib.raft_ingest_frame(*args, None) == -1 and b"null pointer" in _err(lib)
    for h, w, bb in ((0, 8, 1), (-3, 8, 1), (8, 0, 1), (8, 8, 0)):
        assert lib.raft_ingest_frame(a, 0, bb, h, w, 1, b, c, None) == -1 and b"bad size" in _err(lib)
    for tag in (2, -1, 100):
        assert lib.raft_ingest_frame(a, tag, 1, 8, 8, 1, b, c, None) == -1 and b"unknown dtype tag" in _err(lib)
    for args in ((a, 0, 1, 8, 8, 1, a, c), (a, 1, 1, 8, 8, 0, b, a), (a, 0, 1, 8, 8, 1, b, b)):
        assert lib.raft_ingest_frame(*args, None) == -1 and b"in-place" in _err(lib)


def test_stream_carry_argument_errors():
    lib = _lib.load()
    p = [FAKE * k for k in range(1, 7)]
    ok = [p[0], p[1], 64, p[2], p[3], 64, p[4], p[5], 64]
    for i in (0, 1, 3, 4, 6, 7):
        bad = list(ok)
        bad[i] = None
        assert lib.raft_stream_carry(*bad, None) == -1 and b"null pointer" in _err(lib)
    for i in (2, 5, 8):
        bad = list(ok)
        bad[i] = 0
        assert lib.raft_stream_carry(*bad, None) == -1 and b"bad size" in _err(lib)
    for i in (0, 3, 6):
        bad = list(ok)
        bad[i + 1] = bad[i]
        assert lib.raft_stream_carry(*bad, None) == -1 and b"in-place" in _err(lib)


@pytest.mark.parametrize("hw", [(123, 181), (128, 192), (436, 1024), (1, 1), (375, 1242), (8, 7)])
def test_frame_pad_is_input_padders_rule(hw):
    from raft_optical_flow_amd import InputPadder
    from raft_optical_flow_amd.engine import frame_pad
    for mode, centred in (("sintel", True), ("kitti", False)):
        assert frame_pad(hw[0], hw[1], centred) == InputPadder(hw, mode)._pad
    assert frame_pad(123, 181, True) == [1, 2, 2, 3]  # asymmetric on both axes
    out = [ctypes.c_int(-7) for _ in range(4)]
    _lib.load().raft_frame_pad(123, 181, 0, ctypes.byref(out[0]), None, None, ctypes.byref(out[3]))
    assert (out[0].value, out[1].value, out[3].value) == (1, -7, 5)  # NULL outputs are skipped


def _model():
    from raft_optical_flow_amd import RAFT
    return RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False)).eval()


def test_flow_stream_host_side_argument_checks():
    import torch

    from raft_optical_flow_amd import FlowStream, InputPadder
    m = _model()
    for bad in (0, -1):
        with pytest.raises(ValueError, match="iters"):
            m.stream(iters=bad)
    s = m.stream(iters=1, pad_mode="no-such-mode")  # falls to the bottom-pad rule, as InputPadder does
    assert isinstance(s, FlowStream)
    assert s.pad(123, 181) == InputPadder((123, 181), "no-such-mode")._pad == [1, 2, 0, 5]
    assert m.stream().pad(123, 181) == InputPadder((123, 181))._pad == [1, 2, 2, 3]
    assert s.last_flow_init is None
    # a frame is float32 [B,3,H,W] or uint8 [B,H,W,3]: anything else is refused before any device work
    for frame in (torch.zeros(1, 3, 16, 16, dtype=torch.float64), torch.zeros(3, 16, 16),
                  torch.zeros(1, 16, 16, 3), torch.zeros(1, 3, 16, 16, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="a frame is"):
            s.push(frame)
    s.close()
    with pytest.raises(RuntimeError, match="close"):
        s.push(torch.zeros(1, 3, 16, 16))
    m.train()
    with pytest.raises(NotImplementedError, match="inference path"):
        m.stream()
    m.eval()
    replica = m._replicate_for_data_parallel()
    with pytest.raises(RuntimeError, match="replica"):
        replica.stream()
