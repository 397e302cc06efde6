"""Runners of the correlation builds for tests/test_gpu_corr_build_forms.py: every operand and output in a
NaN-prefilled allocation.  Run as a script (python corr_build_gpu.py OUT.npz) it is the fresh child process
of the once-per-process switches: it builds corr_build_oracle.SWITCH_CASES with raft_corr_build_ws and
raft_corr_build_prec (F16X3) under whatever RAFT_CB4_L2 / RAFT_CORR_BUILD_BIG its environment holds and
writes the raw pyramids to OUT.npz."""
import contextlib
import os
import sys

import numpy as np
import torch

import corr_build_oracle as CB

DEV = "cuda"
GUARD = 64                 # guard floats on either side of the pyramid and the workspace
NAN_BITS = 0x7FC0BEEF      # the prefill: one NaN bit pattern no kernel produces
PAD_ROWS = 3               # NaN rows before and after each fmap
ENTRIES = ("fp32", "prec", "ws8", "ws4")
SWITCHES = ("RAFT_CORR_NT", "RAFT_CB4_W4", "RAFT_CB_ORDER", "RAFT_CORR_BUILD4")   # read per call


def prec_of(entry):
    return CB.FP32 if entry == "fp32" else CB.F16X3


@contextlib.contextmanager
def switches(**kv):
    """The per-call switches set to kv (all others unset) for the duration."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _nanbuf(n):
    whole = torch.full((n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def _untouched(t):
    return bool((t == NAN_BITS).all())


def _operand(rows, ld):
    """rows [n][C] -> its device rows [n][ld] inside a NaN-filled allocation: PAD_ROWS rows of NaN before
    and after, NaN in the ld - C columns."""
    n, C = rows.shape
    whole = torch.full(((n + 2 * PAD_ROWS) * ld,), float("nan"), device=DEV)
    view = whole[PAD_ROWS * ld:(PAD_ROWS + n) * ld].view(n, ld)
    view[:, :C] = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
    return whole, view


def build(entry, f1, f2, B, H, W, L, sqrt_c, ld=None, env=None, ws_prec=None, ws_kernel=True, accessor=False):
    """One build on NaN-prefilled buffers -> the raw pyramid (numpy float32), or (raw, levels) with the levels
    raft_corr_pyramid_level returns.  entry: fp32 (raft_corr_build), prec (raft_corr_build_prec, F16X3), ws8 /
    ws4 (raft_corr_build_ws, default / RAFT_CB4_W4=1; precision ws_prec or F16X3; ws_kernel: the call is
    expected to take the 256 x 256 kernel, i.e. raft_corr_build_ws_bytes_prec > 0, else == 0 and the workspace
    must come back untouched).  Asserts: guards intact, every float of the pyramid written."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    lib = _lib.load()
    C = f1.shape[1]
    ld = C if ld is None else ld
    n = K.pyramid_floats(B, H, W, L)
    assert n == CB.pyramid_floats(B, H, W, L)
    keep1, t1 = _operand(f1, ld)
    keep2, t2 = _operand(f2, ld)
    whole, pyr = _nanbuf(n)
    env = dict(env or {})
    if entry == "ws4":
        env["RAFT_CB4_W4"] = "1"
    ws_whole = ws = None
    with switches(**env):
        if entry == "fp32":
            _lib.call("raft_corr_build", t1.data_ptr(), t2.data_ptr(), ld, B, H, W, C, L, sqrt_c, pyr.data_ptr(),
                      K.stream_handle())
        elif entry == "prec":
            _lib.call("raft_corr_build_prec", t1.data_ptr(), t2.data_ptr(), ld, B, H, W, C, L, sqrt_c, _lib.PREC_F16X3,
                      pyr.data_ptr(), K.stream_handle())
        else:
            prec = _lib.PREC_F16X3 if ws_prec is None else ws_prec
            need = int(lib.raft_corr_build_ws_bytes_prec(B, H, W, C, prec))
            wsb = int(lib.raft_corr_build_ws_bytes(B, H, W, C))
            assert (need == wsb and need > 0) if ws_kernel else need == 0, (need, wsb)
            ws_whole, ws = _nanbuf((wsb + 3) // 4)
            _lib.call("raft_corr_build_ws", t1.data_ptr(), t2.data_ptr(), ld, B, H, W, C, L, sqrt_c, prec,
                      pyr.data_ptr(), ws.data_ptr(), wsb, K.stream_handle())
        torch.cuda.synchronize()
    assert _untouched(whole[:GUARD]) and _untouched(whole[-GUARD:]), "the pyramid's guards"
    if ws_whole is not None:
        assert _untouched(ws_whole[:GUARD]) and _untouched(ws_whole[-GUARD:]), "the workspace's guards"
        assert ws_kernel or _untouched(ws), "a fallback wrote the workspace"
    assert not bool((pyr == NAN_BITS).any()), "a pyramid element was not written"
    raw = pyr.view(torch.float32).cpu().numpy()
    if not accessor:
        return raw
    levels = []
    fpyr = pyr.view(torch.float32)
    for l, (h, w) in enumerate(CB.level_dims(H, W, L)):
        lw, out = _nanbuf(B * H * W * h * w)
        _lib.call("raft_corr_pyramid_level", fpyr.data_ptr(), B, H, W, L, l, out.data_ptr(), K.stream_handle())
        torch.cuda.synchronize()
        assert _untouched(lw[:GUARD]) and _untouched(lw[-GUARD:])
        levels.append(out.view(torch.float32).cpu().numpy().reshape(B * H * W, h, w))
    return raw, levels


def switch_case_inputs(i):
    B, H, W, L = CB.SWITCH_CASES[i]
    f1, f2 = CB.features(B, H, W, CB.SWITCH_C, seed=900 + i)
    return (B, H, W, L), f1, f2, CB.sqrt_c32(CB.SWITCH_C)


def main(out):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = {}
    for i in range(len(CB.SWITCH_CASES)):
        (B, H, W, L), f1, f2, sc = switch_case_inputs(i)
        for entry in ("ws8", "ws4", "prec"):
            res[f"{entry}_{i}"] = build(entry, f1, f2, B, H, W, L, sc)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
