"""raft_convex_upsample and raft_upflow8 against fp64 (tests/elementwise_oracle.py).

Both kernels take coords (grid + flow) as NHWC rows [B*H*W][2] and subtract the grid themselves; the reference's
flow is float32(coords - grid), computed the same way, and everything after that is fp64.  Output buffers are
pre-filled with -7.0 and carry a tail that must keep it; the mask's padding columns (mask_ld = 580) hold NaN, so
a read past column 576 poisons the output.

Measured tolerances: E_ref is the error of the reference's own fp32 arithmetic (oracle.raft_oracle on float32
inputs) against the same function on float64 inputs, for the very inputs of the case; the kernel may differ from
fp64 by 4 * E_ref, not less than 16 * 2^-24 * max|ref| (device expf and division round differently from numpy's by
a few ulp per tap, over 9 taps)."""
import numpy as np
import pytest
import torch

import elementwise_oracle as EO
from oracle import raft_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0
CONVEX_SHAPES = [(2, 5, 7), (1, 1, 1), (1, 1, 9), (3, 6, 1)]
UPFLOW_SHAPES = [(2, 5, 7), (1, 1, 1), (1, 1, 7), (1, 5, 1), (1, 30, 240)]
ids = lambda s: "B%d-%dx%d" % s


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


def coords_of(flow):
    """flow NCHW float32 -> (coords NCHW float32 = grid + flow, the same as NHWC rows [B*H*W, 2])."""
    b, _, h, w = flow.shape
    c = (O.coords_grid(b, h, w) + flow.astype(np.float32)).astype(np.float32)
    return c, np.ascontiguousarray(c.transpose(0, 2, 3, 1).reshape(-1, 2))


def rough_flow(shape, seed):
    b, h, w = shape
    return (np.random.default_rng(seed).normal(size=(b, 2, h, w)) * 10).astype(np.float32)


def smooth_flow(shape):
    b, h, w = shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    u = 6 * np.sin(2 * np.pi * (xs / max(w, 2) + ys / max(h, 2))) + 0.05 * xs
    v = -4 * np.cos(np.pi * xs / max(w, 2)) + 0.1 * ys
    f = np.stack([np.stack([u, v]) * (1 + 0.5 * i) for i in range(b)])
    return f.astype(np.float32)


def run_kernel(entry, crows, shape, mask_rows=None):
    """Launch raft_convex_upsample / raft_upflow8; returns flow_up [B, 2, 8H, 8W] as numpy after checking the
    sentinel behind it."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    b, h, w = shape
    n = b * 2 * 64 * h * w
    cd = torch.from_numpy(crows).to(DEV)
    out = torch.full((n + 64,), SENT, device=DEV)
    if entry == "raft_convex_upsample":
        md = torch.from_numpy(mask_rows).to(DEV)
        _lib.call(entry, cd.data_ptr(), md.data_ptr(), mask_rows.shape[1], out.data_ptr(), b, h, w, K.stream_handle())
    else:
        _lib.call(entry, cd.data_ptr(), out.data_ptr(), b, h, w, K.stream_handle())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.all(host[n:] == SENT), "wrote past the output"
    return host[:n].reshape(b, 2, 8 * h, 8 * w)


def mask_rows_of(mask, ld):
    """mask [B, 576, H, W] -> rows [B*H*W][ld], NaN past column 576."""
    b, _, h, w = mask.shape
    rows = np.full((b * h * w, ld), np.nan, np.float32)
    rows[:, :576] = mask.transpose(0, 2, 3, 1).reshape(-1, 576)
    return rows


def random_logits(shape, seed):
    """Logits ~ N(0, 10), like a trained model's (they span tens), with three planted sub-pixels:
    all nine logits -100; one logit +88 among zeros (expf overflows without the max-subtraction); one at -80."""
    b, h, w = shape
    m = (np.random.default_rng(seed).normal(size=(b, 9, 8, 8, h, w)) * 10).astype(np.float32)
    m[0, :, 1, 2, 0, 0] = -100.0
    m[b - 1, :, 3, 4, h - 1, w - 1] = 0.0
    m[b - 1, 5, 3, 4, h - 1, w - 1] = 88.0
    m[0, 7, 5, 6, h // 2, w // 2] = -80.0
    return m.reshape(b, 576, h, w)


def distinct_logits(shape):
    """One distinct value per (k, a, b), the same at every pixel: an a / b transposition or a wrong k stride
    changes every weight."""
    b, h, w = shape
    idx = np.arange(576)
    vals = ((idx * 7919) % 577) / 577.0 * 8.0 - 4.0
    assert len(np.unique(vals)) == 576
    return np.broadcast_to(vals.astype(np.float32)[None, :, None, None], (b, 576, h, w)).copy()


@pytest.mark.parametrize("mask_ld", [576, 580])
@pytest.mark.parametrize("kind", ["random", "distinct"])
@pytest.mark.parametrize("shape", CONVEX_SHAPES, ids=ids)
def test_convex_upsample_vs_fp64(shape, kind, mask_ld):
    """Within max(4 * E_ref, 16 * 2^-24 * max|ref|) of the fp64 reference.

    Seen on an MI355X (profiles/elementwise_gpu_tests.log; the test prints all three for every case):
      (2, 5, 7) random    E_ref 3.6e-5  max|ref| 176  bound 1.7e-4  kernel 2.7e-5
      (2, 5, 7) distinct  E_ref 2.4e-5  max|ref| 126  bound 1.2e-4  kernel 2.0e-5
      (1, 1, 1) random    E_ref 6.0e-6  max|ref| 109  bound 1.0e-4  kernel 6.0e-6   (the floor decides)
      (1, 1, 9) random    E_ref 2.5e-5  max|ref| 160  bound 1.5e-4  kernel 2.5e-5
      (3, 6, 1) random    E_ref 2.5e-5  max|ref| 222  bound 2.1e-4  kernel 2.5e-5
    the same for mask_ld 576 and 580; in no case is the kernel further from fp64 than the reference's float32."""
    b, h, w = shape
    flow = rough_flow(shape, seed=h * 10 + w)
    c, crows = coords_of(flow)
    f32 = EO.flow_of_coords(c)
    mask = random_logits(shape, seed=b + w) if kind == "random" else distinct_logits(shape)
    ref = EO.upsample_flow(f32, mask)
    bound, e_ref = EO.measured_bound(EO.upsample_flow(f32, mask, np.float32), ref, 16 * EO.U * np.abs(ref).max())
    got = run_kernel("raft_convex_upsample", crows, shape, mask_rows_of(mask, mask_ld))
    assert np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    print(f"convex {shape} {kind} ld={mask_ld}: E_ref {e_ref:.3e} max|ref| {np.abs(ref).max():.1f} bound {bound:.3e} "
          f"gpu err {err:.3e}")
    assert err <= bound


@pytest.mark.parametrize("shape", CONVEX_SHAPES, ids=ids)
def test_convex_upsample_one_hot(shape):
    """Logit k at +60 and the rest 0, for every sub-pixel: the output is 8 * flow of neighbour
    (h + k / 3 - 1, w + k % 3 - 1), 0 where that is off the map, to 9 * e^-60 * max|8 flow| plus one fp32
    rounding: pins k -> (ky, kx) and the zero padding."""
    b, h, w = shape
    flow = rough_flow(shape, seed=3)
    c, crows = coords_of(flow)
    f8 = 8.0 * EO.flow_of_coords(c).astype(np.float64)
    big = np.abs(f8).max()
    tol = 9 * np.exp(-60.0) * big + EO.U * big
    pad = np.pad(f8, ((0, 0), (0, 0), (1, 1), (1, 1)))
    for k in range(9):
        m = np.zeros((b, 9, 64, h, w), np.float32)
        m[:, k] = 60.0
        got = run_kernel("raft_convex_upsample", crows, shape, mask_rows_of(m.reshape(b, 576, h, w), 576))
        nb = pad[:, :, k // 3:k // 3 + h, k % 3:k % 3 + w]              # flow at (h + k/3 - 1, w + k%3 - 1)
        want = np.repeat(np.repeat(nb, 8, axis=2), 8, axis=3)
        assert np.abs(got - want).max() <= tol, k


@pytest.mark.parametrize("field", ["rough", "smooth"])
@pytest.mark.parametrize("shape", UPFLOW_SHAPES, ids=ids)
def test_upflow8(shape, field):
    """(a) against oracle.raft_oracle.upflow8 on float32, the kernel's own arithmetic: 8 * 2^-24 * max|ref|;
    (b) against fp64 (8 * F.interpolate on doubles): max(4 * E_ref, 16 * 2^-24 * max|ref|), E_ref the float32
    oracle's own error against fp64, because the rounding of sx * X decides which source column is read: E_ref is
    3.8e-3 at 30 x 240 on the rough field and 0 at 1 x 1, so no fixed bound serves.
    Seen on an MI355X (profiles/elementwise_gpu_tests.log): (a) 0 at every shape, the kernel is the float32
    oracle bit for bit (its interpolation is compiled without fma contraction; contracted, lx = fma(sx, X, -x0)
    took the unrounded product and (a) read 4.0e-4 against 1.4e-4 at 30 x 240 rough); (b) therefore E_ref itself:
    6.3e-5 at (2, 5, 7) rough, 3.6e-3 at 30 x 240 rough (bound 1.5e-2), 3.1e-5 at 30 x 240 smooth, 0 at 1 x 1."""
    flow = rough_flow(shape, seed=11) if field == "rough" else smooth_flow(shape)
    c, crows = coords_of(flow)
    f32 = EO.flow_of_coords(c)
    ref32 = O.upflow8(f32)
    ref64 = EO.upflow8(f32)
    big = float(np.abs(ref64).max())
    bound, e_ref = EO.measured_bound(ref32, ref64, 16 * EO.U * big)
    got = run_kernel("raft_upflow8", crows, shape)
    err32 = float(np.abs(got.astype(np.float64) - ref32).max())
    err64 = float(np.abs(got - ref64).max())
    print(f"upflow8 {shape} {field}: max|ref| {big:.1f}; vs fp32 oracle {err32:.3e} (bound {8 * EO.U * big:.3e}); "
          f"E_ref {e_ref:.3e}, vs fp64 {err64:.3e} (bound {bound:.3e})")
    assert err32 <= 8 * EO.U * big
    assert err64 <= bound
