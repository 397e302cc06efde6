"""Host-side checks of the flow colour-wheel visualisation (no GPU).

The fp64 restatement of the header's definition (tests/flow_viz_oracle.py) is held to the reference's recorded
bytes (tests/golden/flow_viz.npz, written by tests/golden/make_golden_viz.py): the GPU tests then hold the kernel
to both.  The rest is plumbing that must work before any GPU call: the wheel, the signature table, option
validation, the compat import layout."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import flow_viz_oracle as O
from conftest import REPO, load_golden

from raft_optical_flow_amd import _lib


@pytest.fixture(scope="module")
def gold():
    return load_golden("flow_viz.npz")


def test_oracle_equals_reference_goldens(gold):
    """Byte for byte: the reference computes these fields partly in fp32, the restatement wholly in fp64, and at
    37 x 53 and 64 x 64 no byte falls on the other side of a floor()."""
    f = gold["flows"]
    assert f.shape == (3, 2, 37, 53) and f.dtype == np.float32
    for k in range(3):
        assert np.array_equal(O.flow_to_image(f[k].transpose(1, 2, 0)), gold["img_flows"][k]), k
    assert np.array_equal(O.flow_to_rgb(f), gold["img_flows"])   # the batched form: per-image maxima
    assert np.array_equal(O.flow_to_image(gold["chart"].transpose(1, 2, 0)), gold["img_chart"])
    assert np.array_equal(O.flow_to_image(f[1].transpose(1, 2, 0), clip_flow=3.0), gold["img_clip3"])
    assert np.array_equal(O.flow_to_image(f[0].transpose(1, 2, 0), convert_to_bgr=True), gold["img_bgr"])
    assert np.array_equal(gold["img_bgr"][..., ::-1], gold["img_flows"][0])
    uv = gold["uv"]
    assert np.sqrt((uv.astype(np.float64) ** 2).sum(0)).max() > 1
    assert np.array_equal(O.flow_to_rgb(uv[None], unit=True)[0], gold["img_uv"])


def test_chart_covers_the_wheel(gold):
    """The chart fixture reaches all 55 wheel entries, both axes and the zero vector (white)."""
    c = gold["chart"].astype(np.float64)
    fk = (np.arctan2(-c[1], -c[0]) / np.pi + 1) / 2 * 54
    k0 = np.clip(np.floor(fk), 0, 54).astype(int).ravel()
    assert set(k0) == set(range(54))   # (k0 = 54 needs the angle +pi exactly: v = -0.0)
    assert set(k0) | set((k0 + 1) % 55) == set(range(55))
    assert tuple(gold["img_chart"][32, 32]) == (255, 255, 255)


def test_oracle_own_rules():
    """What the reference leaves undefined or lacks: non-finite pixels, fixed rad_max, stacking."""
    f = np.zeros((2, 2, 4, 6), np.float32)
    f[0, 0] = 3.0
    f[0, :, 1, 2] = (np.nan, 1.0)
    f[0, :, 2, 3] = (1e30, np.inf)
    f[1] = np.nan
    assert np.array_equal(O.rad_max_of(f), [3.0, 0.0])
    img = O.flow_to_rgb(f)
    assert (img[0, 1, 2] == 0).all() and (img[0, 2, 3] == 0).all() and (img[1] == 0).all()
    assert np.array_equal(img[0, 0, 0], O.flow_to_rgb(np.array([3.0, 0.0], np.float32).reshape(1, 2, 1, 1))[0, 0, 0])
    assert (O.flow_to_rgb(np.zeros((1, 2, 3, 3), np.float32)) == 255).all()
    # a fixed rad_max below the field: the 3/4-brightness branch; leftward flow is wheel[27] = (0, 209, 255)
    dim = O.flow_to_rgb(np.array([-4.0, 0.0], np.float32).reshape(1, 2, 1, 1), rad_max=2.0)
    assert tuple(dim[0, 0, 0]) == (0, int(np.floor(255 * (209 / 255 * 0.75))), 191)
    fr = np.array([0.0, 17.0, 255.0, 255.6, -3.0, np.nan, 0.5, 1.5], np.float32)
    frame = np.broadcast_to(fr, (1, 3, 1, 8))
    st = O.flow_to_rgb(np.zeros((1, 2, 1, 8), np.float32), frame=frame)
    assert st.shape == (1, 2, 8, 3)
    assert np.array_equal(st[0, 0, :, 0], [0, 17, 255, 255, 0, 0, 0, 2]) and (st[0, 1] == 255).all()
    assert np.array_equal(O.flow_to_rgb(f, bgr=True), img[..., ::-1])


def test_make_colorwheel_equals_golden(gold):
    from raft_optical_flow_amd.utils.flow_viz import make_colorwheel
    w = make_colorwheel()
    assert w.shape == (55, 3) and w.dtype == np.float64
    assert np.array_equal(w, gold["wheel"]) and np.array_equal(O.wheel(), gold["wheel"])


def test_signature_table_and_header():
    for name in ("raft_flow_viz_ws_bytes", "raft_flow_to_rgb"):
        assert name in _lib.EXPORTED
    hdr = open(os.path.join(REPO, "include", "raft_hip.h")).read()
    assert "size_t raft_flow_viz_ws_bytes(int B, int H, int W);" in hdr
    assert "int raft_flow_to_rgb(const float* flow, long batch_stride, long chan_stride, long pitch," in hdr
    assert "#define RAFT_HIP_ABI_VERSION 19" in hdr
    for flag, val in (("RAFT_VIZ_BGR", _lib.VIZ_BGR), ("RAFT_VIZ_UNIT", _lib.VIZ_UNIT), ("RAFT_VIZ_CLIP", _lib.VIZ_CLIP)):
        assert f"#define {flag} {val} " in hdr
    assert len(_lib._PROTOS["raft_flow_to_rgb"][1]) == 19   # the header's 18 arguments and the stream
    mk = open(os.path.join(REPO, "raft_optical_flow_amd", "csrc", "Makefile")).read()
    assert "flow_viz.hip" in next(ln for ln in mk.splitlines() if ln.startswith("SRCS :="))   # hashed with the rest


FAKE = 1 << 20  # aligned stand-in pointers: an argument error returns before any launch


def test_argument_errors():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libraft_hip.so is not built")
    lib = _lib.load()
    assert lib.raft_hip_abi_version() == 19   # additive entries: the ABI version did not move
    err = lib.raft_hip_last_error
    assert lib.raft_flow_viz_ws_bytes(1, 5, 7) == 4 and lib.raft_flow_viz_ws_bytes(2, 436, 1024) == 2 * 256 * 4
    assert lib.raft_flow_viz_ws_bytes(0, 5, 7) == 0 and lib.raft_flow_viz_ws_bytes(1 << 10, 1 << 10, 1 << 10) == 0

    def viz(**kw):
        a = dict(flow=FAKE, sb=128, sc=64, pitch=8, top=0, left=0, B=1, H=8, W=8, clip=0.0, fixed=0.0, flags=0,
                 frame=None, fsb=192, fsc=64, fpitch=8, ws=2 * FAKE, out=3 * FAKE)
        a.update(kw)
        return lib.raft_flow_to_rgb(*a.values(), None)

    for k in ("flow", "out"):
        assert viz(**{k: None}) == -1 and b"null pointer" in err()
    assert viz(ws=None) == -1 and b"null workspace" in err()
    for kw in ({"B": 0}, {"H": -1}, {"W": 0}, {"B": 1 << 10, "H": 1 << 10, "W": 1 << 10, "pitch": 1 << 10}):
        assert viz(**kw) == -1 and b"bad size" in err()
    assert viz(left=-1) == -1 and b"negative crop" in err()
    for kw in ({"pitch": 7}, {"left": 1}, {"sb": -1}):
        assert viz(**kw) == -1 and b"bad strides" in err()
    assert viz(frame=4 * FAKE, fpitch=7) == -1 and b"bad frame strides" in err()
    for bad in (-1.0, float("nan"), float("inf")):
        assert viz(fixed=bad) == -1 and b"fixed_rad_max" in err()
    for bad in (-1.0, float("nan")):
        assert viz(clip=bad, flags=_lib.VIZ_CLIP) == -1 and b"clip_flow" in err()
    assert viz(flags=8) == -1 and b"unknown flags" in err()
    assert viz(out=3 * FAKE + 2) == -1 and b"misaligned" in err()
    for kw in ({"out": FAKE}, {"out": 2 * FAKE}, {"frame": 3 * FAKE}, {"ws": FAKE}):
        assert viz(**kw) == -1 and b"aliases" in err()


class _NoGpuModel:
    """Stands where a model would: stream() must reject its options before it looks at the model."""
    training = False

    def __getattr__(self, name):
        raise AssertionError(f"the model was touched ({name}) before the options were checked")


def test_stream_option_validation_before_any_gpu_call():
    from raft_optical_flow_amd.raft import RAFT, FlowStream
    for bad in ("RGB", "hsv", 1, True):
        with pytest.raises(ValueError, match="visualize must be"):
            FlowStream(_NoGpuModel(), visualize=bad)
    for bad in (0, -1.0, float("nan"), float("inf"), "3"):
        with pytest.raises(ValueError, match="viz_rad_max"):
            FlowStream(_NoGpuModel(), visualize="rgb", viz_rad_max=bad)
    with pytest.raises(TypeError, match="viz_stack"):
        FlowStream(_NoGpuModel(), visualize="rgb", viz_stack=1)
    # through RAFT.stream, on a CPU model: the same errors, and valid options open a stream without a GPU
    import argparse
    m = RAFT(argparse.Namespace(small=True, mixed_precision=False, alternate_corr=False)).eval()
    with pytest.raises(ValueError, match="visualize must be"):
        m.stream(visualize="gray")
    with pytest.raises(ValueError, match="viz_rad_max"):
        m.stream(visualize="bgr", viz_rad_max=0.0)
    s = m.stream(visualize="bgr", viz_rad_max=12, viz_stack=True)
    assert (s.visualize, s.viz_rad_max, s.viz_stack) == ("bgr", 12.0, True)
    d = m.stream()
    assert (d.visualize, d.viz_rad_max, d.viz_stack) == (None, None, False)


def test_flow_to_image_assertions_before_any_gpu_call():
    from raft_optical_flow_amd.utils.flow_viz import flow_to_image, flow_to_rgb
    with pytest.raises(AssertionError, match="input flow must have three dimensions"):
        flow_to_image(np.zeros((4, 4), np.float32))
    with pytest.raises(AssertionError, match=r"input flow must have shape \[H,W,2\]"):
        flow_to_image(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(AssertionError, match=r"input flow must have shape \[H,W,2\]"):
        flow_to_image(torch.zeros(2, 4, 4))
    a = torch.zeros(1, 2, 8, 8)
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        flow_to_rgb(a)
    with pytest.raises(TypeError, match="float32"):
        flow_to_rgb(a.double())
    with pytest.raises(ValueError, match=r"\[B, 2, H, W\]"):
        flow_to_rgb(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="differ in size"):
        flow_to_rgb(a, frame=torch.zeros(1, 3, 8, 9))
    with pytest.raises(ValueError, match="viz_rad_max"):
        flow_to_rgb(a, rad_max=-2.0)


def test_compat_shim_imports_under_demo_layout():
    """demo.py's own lines: cwd = the directory that holds core/, sys.path.append('core'), from utils import
    flow_viz."""
    code = ("import sys\nsys.path.append('core')\nfrom utils import flow_viz\n"
            "w = flow_viz.make_colorwheel()\nassert w.shape == (55, 3)\n"
            "assert callable(flow_viz.flow_to_image) and callable(flow_viz.flow_uv_to_colors)\n"
            "import raft_optical_flow_amd.utils.flow_viz as V\nassert flow_viz.flow_to_image is V.flow_to_image\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(REPO, "compat"), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
