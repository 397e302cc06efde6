"""The resize's definition, its arguments and its reference fixture, without a GPU.

tests/resize_oracle.py restates raft_resize's definition (include/raft_hip.h) in numpy fp64 with exact integer
source coordinates.  Here it is pinned to torch.nn.functional.interpolate on float64 CPU tensors (1e-9 max|v|:
fp64 rounding and torch's fp64 coordinate put the difference near 1e-11 at these sizes, four orders below
anything fp32 can show), its coordinates' properties are checked with exact integers, the recorded outputs of the
reference's InputScaler (tests/golden/resize_reference.npz) are held to their own recorded distance, and the
argument checks of utils.resize_frame / resize_flow / InputScaler and of the C entry are exercised: all of them
raise before a device is touched.
"""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_oracle as O
from raft_optical_flow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_reference.npz")


# ----------------------------------------------------------------------------- the oracle against torch fp64


@pytest.mark.parametrize("mode,align", [("bilinear", False), ("bilinear", True), ("area", False)])
@pytest.mark.parametrize("src,size", O.SHAPES)
def test_oracle_matches_torch_fp64(src, size, mode, align):
    b, hs, ws = src
    v = O.seeded_frame(b, 3, hs, ws, seed=hs * 131 + ws).astype(np.float64)
    kw = {} if mode == "area" else {"align_corners": align}
    want = F.interpolate(torch.from_numpy(v), size=size, mode=mode, **kw).numpy()
    got = O.resize_ref(v, size, mode, align)
    dist = float(np.abs(got - want).max())
    print(f"{src} -> {size} {mode} align={align}: max |oracle - torch fp64| = {dist:.3e}")
    assert got.shape == want.shape
    assert dist <= 1e-9 * float(np.abs(v).max())


def test_oracle_flow_multipliers_and_u8_rounding():
    fl = O.seeded_flow(1, 17, 23).astype(np.float64)
    m0, m1 = O.flow_muls((17, 23), (40, 56))
    assert m0 == float(np.float32(56 / 23)) and m1 == float(np.float32(40 / 17))
    plain, scaled = O.resize_ref(fl, (40, 56)), O.resize_ref(fl, (40, 56), "bilinear", False, m0, m1)
    assert np.array_equal(scaled[:, 0], plain[:, 0] * m0) and np.array_equal(scaled[:, 1], plain[:, 1] * m1)
    three = O.resize_ref(np.ones((1, 3, 4, 4)), (2, 2), "area", False, 2.0, 3.0)   # the third channel is not scaled
    assert np.array_equal(three[0, :, 0, 0], [2.0, 3.0, 1.0])
    v = np.array([-3.0, 0.5, 1.5, 2.5, 254.5, 255.5, 300.0, np.nan, np.inf, -np.inf, 0.49999, 127.50001])
    assert O.to_u8(v).tolist() == [0, 0, 2, 2, 254, 255, 255, 0, 255, 0, 0, 128]   # ties to even, saturated


# ----------------------------------------------------------------------------- coordinate properties


def test_identity_has_zero_weights():
    for n in (1, 2, 7, 53, 1920, 32768):
        for align in (False, True):
            i0, i1, rem, den = O.lin_coords(n, n, align)
            assert i0 == list(range(n)) and rem == [0] * n
            assert i1 == [min(k + 1, n - 1) for k in range(n)]


def test_align_corners_hits_samples_when_divisible():
    for S, D in ((2, 5), (5, 9), (5, 13), (9, 5), (33, 9), (4, 1), (1, 4)):
        assert S == 1 or D == 1 or (D - 1) % (S - 1) == 0 or (S - 1) % (D - 1) == 0
        i0, i1, rem, den = O.lin_coords(D, S, True)
        if D > 1 and S > 1 and (S - 1) % (D - 1) == 0:             # a downscale by an integer step
            assert rem == [0] * D and i0 == [d * (S - 1) // (D - 1) for d in range(D)]
        if D > 1 and S > 1 and (D - 1) % (S - 1) == 0:             # every source sample is hit exactly
            k = (D - 1) // (S - 1)
            assert [i0[d] for d in range(0, D, k)] == list(range(S)) and all(rem[d] == 0 for d in range(0, D, k))
        assert i0[0] == 0 and rem[0] == 0                          # the corners align
        assert D == 1 or S == 1 or (i0[-1] == S - 1 and rem[-1] == 0)


@pytest.mark.parametrize("S,D", [(32768, 32767), (32767, 32768), (32768, 1), (3, 32768), (32749, 19997),
                                 (1080, 544), (1920, 960), (1920, 1277)])
def test_index_arithmetic_is_exact(S, D):
    """i0 + rem / den is the position torch defines, as an exact fraction, at sizes up to 2^15."""
    for align in (False, True):
        i0, i1, rem, den = O.lin_coords(D, S, align)
        for d in sorted({0, 1, D // 3, D // 2, D - 2, D - 1} & set(range(D))):
            if align:
                pos = Fraction(d * (S - 1), D - 1) if D > 1 else Fraction(0)
            else:
                pos = max(Fraction(S, D) * (Fraction(d) + Fraction(1, 2)) - Fraction(1, 2), Fraction(0))
            assert Fraction(i0[d]) + Fraction(rem[d], den) == pos
            assert 0 <= i0[d] <= i1[d] <= S - 1 and i1[d] - i0[d] == (1 if i0[d] < S - 1 else 0)
            assert 0 <= rem[d] < den


def test_area_boxes_tile_the_source():
    for S, D in ((37, 19), (53, 27), (8, 1), (1, 5), (17, 40), (96, 48), (1080, 544)):
        lo, hi = O.box_coords(D, S)
        assert lo[0] == 0 and hi[-1] == S and all(0 <= a < b <= S for a, b in zip(lo, hi))
        assert all(lo[d + 1] <= hi[d] for d in range(D - 1))       # no gap
        if S % D == 0:
            assert all(b - a == S // D for a, b in zip(lo, hi))    # a plain average pool


# ----------------------------------------------------------------------------- the reference's outputs


def test_golden_fixture_matches_oracle():
    """tests/golden/resize_reference.npz (make_golden_resize.py): the seeded case and what the reference's
    InputScaler.fill / unfill return for it in fp32.  Each output's distance to the fp64 definition was stored
    with it; the oracle reproduces those distances, and they are the size F.interpolate's fp32 coordinate
    explains (below 1e-2 on these values), not a difference of definition."""
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 200_000
    frame, flow = g["frame"], g["flow"]
    c_frame, c_flow = O.golden_case()
    assert frame.dtype == np.float32 and np.array_equal(frame, c_frame) and np.array_equal(flow, c_flow)
    assert tuple(g["s19x27_size"]) == (19, 27) and tuple(g["s40x56_size"]) == (40, 56)
    assert tuple(g["stride8_size"]) == (40, 56)                    # stride 8 of 37 x 53: stored once, as (40, 56)
    n = 0
    for name, size in (("s19x27", (19, 27)), ("s40x56", (40, 56))):
        for what, x, tags in (("frame", frame, ("fill",)), ("flow", flow, ("fill", "unfill"))):
            for tag in tags:
                key = f"{name}_{what}_{tag}"
                src = x if tag == "fill" else g[f"{name}_{what}_fill"]
                tgt = size if tag == "fill" else (37, 53)
                m = O.flow_muls(src.shape[-2:], tgt) if what == "flow" else (1.0, 1.0)
                ref = O.resize_ref(src, tgt, "bilinear", False, *m)
                dist = float(np.abs(g[key].astype(np.float64) - ref).max())
                stored = float(g["ref_dist_" + key])
                print(f"{key}: reference's distance to fp64 {dist:.3e} (stored {stored:.3e})")
                assert g[key].dtype == np.float32 and g[key].shape == ref.shape
                assert abs(dist - stored) <= 1e-9 * stored
                assert 1e-6 < stored < 1e-2
                n += 1
    assert n == 6


# ----------------------------------------------------------------------------- InputScaler


def test_input_scaler_size_arithmetic():
    from raft_optical_flow_amd.utils import InputScaler
    s = InputScaler((2, 3, 37, 53), stride=8)
    assert (s.orig_height, s.orig_width, s.tgt_height, s.tgt_width) == (37, 53, 40, 56)
    s = InputScaler((40, 56), stride=8)                            # already a multiple: unchanged
    assert (s.tgt_height, s.tgt_width) == (40, 56)
    s = InputScaler((1080, 1920), stride=64)
    assert (s.tgt_height, s.tgt_width) == (1088, 1920)
    s = InputScaler((1, 3, 1080, 1920), size=(544, 960))
    assert (s.tgt_height, s.tgt_width) == (544, 960)
    s = InputScaler(torch.Size((1, 3, 37, 53)), scale_factor=0.5)  # truncation, not rounding
    assert (s.tgt_height, s.tgt_width) == (18, 26)
    s = InputScaler((123, 181), scale_factor=0.5)
    assert (s.tgt_height, s.tgt_width) == (61, 90)
    s = InputScaler((37, 53), scale_factor=1.5)
    assert (s.tgt_height, s.tgt_width) == (55, 79)
    s = InputScaler((37, 53))                                      # the defaults: the same size
    assert (s.tgt_height, s.tgt_width) == (37, 53)
    assert s.interpolation_mode == "bilinear" and s.interpolation_align_corners is False
    s = InputScaler((37, 53), size=(19, 27), interpolation_mode="area")
    assert s.interpolation_mode == "area"
    assert InputScaler((37, 53), size=(19, 27), interpolation_align_corners=True).interpolation_align_corners is True


def test_input_scaler_argument_errors():
    from raft_optical_flow_amd.utils import InputScaler
    with pytest.raises(ValueError, match="stride OR size"):
        InputScaler((37, 53), stride=8, size=(40, 56))
    for mode in ("nearest", "bicubic", "BILINEAR", None):
        with pytest.raises(NotImplementedError, match="bilinear"):
            InputScaler((37, 53), interpolation_mode=mode)
    with pytest.raises(ValueError, match="align_corners"):
        InputScaler((37, 53), interpolation_mode="area", interpolation_align_corners=True)
    with pytest.raises(TypeError, match="align_corners"):
        InputScaler((37, 53), interpolation_align_corners=1)
    for bad in (0, -8):
        with pytest.raises(ValueError, match="stride"):
            InputScaler((37, 53), stride=bad)
    with pytest.raises(TypeError, match="stride"):
        InputScaler((37, 53), stride=8.0)
    for bad in ((0, 5), (5, -1)):
        with pytest.raises(ValueError, match="positive"):
            InputScaler((37, 53), size=bad)
    for bad in ((5,), (1, 2, 3), (2.5, 3), 7, "ab"):
        with pytest.raises(TypeError, match="size"):
            InputScaler((37, 53), size=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 0.01):
        with pytest.raises(ValueError, match="scale_factor"):
            InputScaler((37, 53), scale_factor=bad)
    with pytest.raises(TypeError, match="scale_factor"):
        InputScaler((37, 53), scale_factor="0.5")
    with pytest.raises(ValueError, match="orig_shape"):
        InputScaler((37,))
    s = InputScaler((8, 8), size=(4, 4))
    with pytest.raises(TypeError, match="tensor"):
        s.fill(np.zeros((1, 3, 8, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="C, H, W"):
        s.fill(torch.zeros(8, 8))
    with pytest.raises(ValueError, match="floating-point"):
        s.fill(torch.zeros(1, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="2 channels"):
        s.unfill(torch.zeros(1, 1, 4, 4), is_flow=True)


# ----------------------------------------------------------------------------- resize_frame / resize_flow


def test_resize_argument_checks():
    from raft_optical_flow_amd.utils import resize_flow, resize_frame
    fr, fl = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8)
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for f in (fr, u8):
        with pytest.raises(RuntimeError, match="ROCm GPU only"):   # CPU tensors: there is no CPU path
            resize_frame(f, (4, 4))
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        resize_flow(fl, (4, 4))
    with pytest.raises(TypeError, match="tensor"):
        resize_frame(fr.numpy(), (4, 4))
    with pytest.raises(TypeError, match="tensor"):
        resize_flow(fl.numpy(), (4, 4))
    with pytest.raises(TypeError, match="float32 .* or uint8"):
        resize_frame(fr.half(), (4, 4))
    with pytest.raises(TypeError, match="float32"):
        resize_flow(fl.double(), (4, 4))
    for bad in (torch.zeros(3, 8, 8), torch.zeros(1, 3, 0, 8), torch.zeros(1, 8, 8, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="frame"):
            resize_frame(bad, (4, 4))
    for bad in (torch.zeros(2, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 0, 8)):
        with pytest.raises(ValueError, match=r"\[B, 2, H, W\]"):
            resize_flow(bad, (4, 4))
    for fn, x in ((resize_frame, fr), (resize_flow, fl)):
        for bad in ((4,), 4, (4.0, 4), (True, 4)):
            with pytest.raises(TypeError, match="size"):
                fn(x, bad)
        with pytest.raises(ValueError, match="positive"):
            fn(x, (0, 4))
        for mode in ("nearest", "bicubic", "linear"):
            with pytest.raises(NotImplementedError, match="bilinear"):
                fn(x, (4, 4), mode=mode)
        with pytest.raises(ValueError, match="align_corners"):
            fn(x, (4, 4), mode="area", align_corners=True)
        with pytest.raises(TypeError, match="align_corners"):
            fn(x, (4, 4), align_corners=None)
    with pytest.raises(TypeError, match="out_dtype"):
        resize_frame(fr, (4, 4), out_dtype=torch.float16)
    with pytest.raises(ValueError, match="3 channels"):
        resize_frame(torch.zeros(1, 5, 8, 8), (4, 4), out_dtype=torch.uint8)


# ----------------------------------------------------------------------------- the C entry


FAKE = 1 << 20  # 16-byte aligned stand-in pointers: an argument error returns before any launch


def test_resize_symbol_and_argument_errors():
    lib = _lib.load()
    assert "raft_resize" in _lib.EXPORTED and hasattr(lib, "raft_resize")
    assert lib.raft_hip_abi_version() == 19 and _lib.ABI_VERSION == 19   # an additive entry
    assert (_lib.RESIZE_BILINEAR, _lib.RESIZE_AREA, _lib.RESIZE_ALIGN_CORNERS) == (0, 1, 1)
    err = lib.raft_hip_last_error
    F32, U8 = _lib.FRAME_F32_NCHW, _lib.FRAME_U8_NHWC

    def resize(**kw):
        a = dict(src=FAKE, stag=F32, sb=192, sc=64, pitch=8, top=0, left=0, B=1, C=3, Hs=8, Ws=8, dst=2 * FAKE, dtag=F32,
                 Hd=4, Wd=4, mode=0, flags=0, mul0=1.0, mul1=1.0)
        a.update(kw)
        return lib.raft_resize(*a.values(), None)

    for k in ("src", "dst"):
        assert resize(**{k: None}) == -1 and b"null pointer" in err()
    assert resize(stag=2) == -1 and b"unknown source dtype" in err()
    assert resize(dtag=-1) == -1 and b"unknown destination dtype" in err()
    for mode in (2, -1, 7):
        assert resize(mode=mode) == -1 and b"unknown mode" in err()
    for flags in (2, 4, -1):
        assert resize(flags=flags) == -1 and b"unknown flags" in err()
    assert resize(mode=1, flags=1) == -1 and b"bilinear option" in err()
    for kw in ({"B": 0}, {"C": 0}, {"Hs": -1}, {"Ws": 0}, {"Hd": 0}, {"Wd": -4}):
        assert resize(**kw) == -1 and b"bad size" in err()
    for kw in ({"B": 1 << 10, "Hs": 1 << 10, "Ws": 1 << 10, "pitch": 1 << 10}, {"Hd": 1 << 15, "Wd": 1 << 15},
               {"B": 1 << 20, "C": 1 << 20}, {"C": 1 << 16, "Hd": 1 << 16, "Wd": 1 << 16}):
        assert resize(**kw) == -1 and b"below 2^30" in err()
    for kw in ({"stag": U8, "C": 4}, {"dtag": U8, "C": 1}, {"stag": U8, "dtag": U8, "C": 5}):
        assert resize(**kw) == -1 and b"3 channels" in err()
    for kw in ({"top": -1}, {"left": -2}):
        assert resize(**kw) == -1 and b"negative crop" in err()
    for kw in ({"pitch": 7}, {"left": 1}, {"sb": -1}, {"sc": -1}):
        assert resize(**kw) == -1 and b"bad source strides" in err()
    for kw in ({"src": FAKE + 2}, {"dst": 2 * FAKE + 1}):
        assert resize(**kw) == -1 and b"misaligned" in err()
    assert resize(dst=FAKE) == -1 and b"aliases" in err()
    # a uint8 source is dense: its strides are not read, and neither uint8 side needs alignment
    # (the alias check is the last one: reaching it shows that the earlier ones passed)
    assert resize(stag=U8, dtag=U8, src=FAKE + 1, dst=FAKE + 1, sb=-1, pitch=0) == -1 and b"aliases" in err()


def test_sources_mention_the_new_file_and_entry():
    with open(os.path.join(ROOT, "raft_optical_flow_amd", "csrc", "Makefile")) as fh:
        srcs = next(ln for ln in fh if ln.startswith("SRCS :="))
    assert "resize.hip" in srcs.split()                            # built, and hashed with the rest
    with open(os.path.join(ROOT, "include", "raft_hip.h")) as fh:
        hdr = fh.read()
    for name in ("int raft_resize(", "#define RAFT_RESIZE_BILINEAR 0", "#define RAFT_RESIZE_AREA 1",
                 "#define RAFT_RESIZE_ALIGN_CORNERS 1", "#define RAFT_HIP_ABI_VERSION 19"):
        assert name in hdr, name
    with open(os.path.join(ROOT, "raft_optical_flow_amd", "csrc", "resize.hip")) as fh:
        src = fh.read()
    assert 'extern "C" int raft_resize(' in src and "fp contract(off)" in src
    from raft_optical_flow_amd.utils import utils as U_
    for name in ("resize_frame", "resize_flow", "InputScaler"):
        assert name in U_.__doc__ and hasattr(U_, name)
