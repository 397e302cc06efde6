"""The layout and state kernels on their own: raft_nchw_to_nhwc, raft_nhwc_to_nchw, raft_avgpool2_nhwc,
raft_prep_images, raft_init_coords and raft_flow_from_coords against include/raft_hip.h's definitions (fp64 where
the formula rounds, tests/elementwise_oracle.py).

Every output buffer is pre-filled with -7.0: the padding columns of ld > C rows and a tail behind the last row
must still hold it after the launch."""
import numpy as np
import pytest
import torch

import elementwise_oracle as EO
from oracle import raft_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0
TAIL = 16
SHAPES = [(2, 5, 7), (3, 1, 9), (1, 4, 1)]
ids = lambda s: "B%d-%dx%d" % s


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


def call(name, *args):
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    # tensors are passed as they are and stay referenced until the launch has finished
    _lib.call(name, *[a.data_ptr() if torch.is_tensor(a) else a for a in args], K.stream_handle())
    torch.cuda.synchronize()


def sentinel(n):
    return torch.full((n + TAIL,), SENT, device=DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def take(buf, n):
    """The first n floats of a sentinel buffer as numpy; the tail must be untouched."""
    host = buf.cpu().numpy()
    assert np.all(host[n:] == SENT), "wrote past the output"
    return host[:n]


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("C", [1, 2, 3, 5, 64])
def test_nchw_nhwc_round_trip(C, shape):
    """NCHW -> rows [B*H*W][ld] equals the permute exactly for ld in {C, C + 3}, the padding columns keep the
    sentinel, and rows -> NCHW gives the input back."""
    B, H, W = shape
    n = B * H * W
    x = np.random.default_rng(C * 100 + W).normal(size=(B, C, H, W)).astype(np.float32)
    want = x.transpose(0, 2, 3, 1).reshape(n, C)
    xd = dev(x)
    for ld in (C, C + 3):
        rows = sentinel(n * ld)
        call("raft_nchw_to_nhwc", xd.data_ptr(), rows.data_ptr(), ld, B, C, H, W)
        got = take(rows, n * ld).reshape(n, ld)
        assert np.array_equal(got[:, :C], want), ld
        assert np.all(got[:, C:] == SENT), ld
        back = sentinel(n * C)
        call("raft_nhwc_to_nchw", rows.data_ptr(), ld, back.data_ptr(), B, C, H, W)
        assert np.array_equal(take(back, n * C).reshape(B, C, H, W), x), ld


@pytest.mark.parametrize("hw", [(2, 2), (5, 7), (6, 9), (3, 2)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("C", [1, 5, 64])
def test_avgpool2_nhwc(C, hw):
    """Bit-equal to (((a + b) + c) + d) / 4 in fp32 (the 2 x 2 window in row-major order), within
    3 * 2^-24 * max|x| of F.avg_pool2d's definition in fp64; odd sizes floor; B = 2."""
    B, (H, W) = 2, hw
    Ho, Wo = H // 2, W // 2
    x = (np.random.default_rng(C + H).normal(size=(B, H, W, C)) * 3 + 1).astype(np.float32)
    out = sentinel(B * Ho * Wo * C)
    call("raft_avgpool2_nhwc", dev(x), out.data_ptr(), B, H, W, C)
    got = take(out, B * Ho * Wo * C).reshape(B, Ho, Wo, C)
    assert np.array_equal(got, EO.avg_pool2_rows_fp32(x))
    ref = EO.avg_pool2(x.transpose(0, 3, 1, 2)).transpose(0, 2, 3, 1)
    assert np.abs(got - ref).max() <= 3 * EO.U * np.abs(x).max()


@pytest.mark.parametrize("shape", [(2, 5, 7), (2, 1, 9), (2, 4, 1)], ids=ids)
def test_init_coords_and_flow_from_coords(shape):
    """coords rows [B*H*W][2] = coords_grid (+ flow_init), flow = coords - coords_grid: one fp32 add / subtract
    each, so bit-equal to the numpy expression; B = 2 with a different flow per image."""
    B, H, W = shape
    n = B * H * W
    grid = O.coords_grid(B, H, W)
    as_rows = lambda a: a.transpose(0, 2, 3, 1).reshape(n, 2)
    flow = (np.random.default_rng(H + W).normal(size=(B, 2, H, W)) * 7).astype(np.float32)
    assert not np.array_equal(flow[0], flow[1])
    # without flow_init: the grid itself
    c0 = sentinel(n * 2)
    call("raft_init_coords", c0.data_ptr(), None, B, H, W)
    assert np.array_equal(take(c0, n * 2).reshape(n, 2), as_rows(grid))
    # with flow_init
    c1 = sentinel(n * 2)
    call("raft_init_coords", c1.data_ptr(), dev(flow), B, H, W)
    want = (grid + flow).astype(np.float32)
    assert np.array_equal(take(c1, n * 2).reshape(n, 2), as_rows(want))
    # and back: (grid + flow) - grid in fp32 (not always flow itself)
    f = sentinel(n * 2)
    call("raft_flow_from_coords", c1.data_ptr(), f.data_ptr(), B, H, W)
    assert np.array_equal(take(f, n * 2).reshape(B, 2, H, W), want - grid)
    # arbitrary coords, not produced by init_coords
    cr = (np.random.default_rng(1).normal(size=(n, 2)) * 30).astype(np.float32)
    f2 = sentinel(n * 2)
    call("raft_flow_from_coords", dev(cr), f2.data_ptr(), B, H, W)
    assert np.array_equal(take(f2, n * 2).reshape(B, 2, H, W), cr.reshape(B, H, W, 2).transpose(0, 3, 1, 2) - grid)


@pytest.mark.parametrize("hw", [(5, 7), (1, 9), (4, 1)], ids=lambda s: "%dx%d" % s)
def test_prep_images(hw):
    """rows [2B*H*W][3] = 2 * (x / 255) - 1, image1's batch then image2's, within 3 * 2^-24 of fp64 (three
    rounded operations on values of magnitude <= 1); B = 2, the inputs include 0, 255 and non-integers."""
    B, (H, W) = 2, hw
    r = np.random.default_rng(H)
    a = r.uniform(0, 255, size=(B, 3, H, W)).astype(np.float32)
    b = r.uniform(0, 255, size=(B, 3, H, W)).astype(np.float32)
    a.reshape(-1)[:4] = (0.0, 255.0, 127.5, 128.0)
    b.reshape(-1)[-3:] = (255.0, 0.0, 0.25)
    n = 2 * B * H * W * 3
    out = sentinel(n)
    call("raft_prep_images", dev(a), dev(b), out.data_ptr(), B, H, W)
    got = take(out, n).reshape(-1, 3)
    ref = EO.prep_images(a, b)
    assert np.abs(got - ref).max() <= 3 * EO.U
    assert got.min() >= -1.0 and got.max() <= 1.0
    # image1's batch first, image2's second (the two differ far beyond the bound)
    half = B * H * W
    assert np.abs(ref[:half] - ref[half:]).max() > 0.1
    assert got[0, 0] == -1.0 and got[1, 0] == 1.0          # x = 0 and x = 255 are exact
