"""The bidirectional-stream additions that need no GPU: an fp64 restatement of the forward-backward check
(include/raft_hip.h), pinned against torch's grid_sample where the two definitions coincide; the random case
the kernel test uses and its margin cap; argument validation of stream(bidirectional=...) and fb_consistency;
the new C-ABI entries' argument errors.

tests/test_gpu_bidi.py imports the restatement (fb_reference), the fp32 error bound and the cases from here."""
import argparse
import ctypes
import functools

import numpy as np
import pytest
import torch

from raft_optical_flow_amd import _lib

ALPHA = float(np.float32(0.01))   # the ABI takes floats: the reference uses the constants the kernel sees
BETA = 0.5
U = 2.0 ** -24                    # fp32 unit roundoff (round to nearest)
SHAPES = [(1, 5, 7), (2, 37, 53), (1, 16, 260)]


# ----------------------------------------------------------------------------- the restatement


def fb_direction(F, G, alpha=ALPHA, beta=BETA):
    """One direction of the check in fp64.  F, G: [B,2,H,W] arrays (their values are taken as given and
    widened).  Returns a dict of [B,H,W] arrays: err, occ, thr, inside, bound (below)."""
    F = np.asarray(F, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64)
    B, _, H, W = F.shape
    jj = np.arange(W, dtype=np.float64)[None, None, :]
    ii = np.arange(H, dtype=np.float64)[None, :, None]
    fx, fy = F[:, 0], F[:, 1]
    with np.errstate(invalid="ignore"):
        # x + F(x) in [0, W-1] x [0, H-1], compared without forming the sum (exact for any F)
        inside = (np.isfinite(fx) & np.isfinite(fy) & (fx >= -jj) & (fx <= (W - 1) - jj)
                  & (fy >= -ii) & (fy <= (H - 1) - ii))
    fxs, fys = np.where(inside, fx, 0.0), np.where(inside, fy, 0.0)
    flx, fly = np.floor(fxs), np.floor(fys)
    ax, ay = fxs - flx, fys - fly
    x0 = (jj + flx).astype(np.int64)
    y0 = (ii + fly).astype(np.int64)
    x1ok, y1ok = x0 + 1 <= W - 1, y0 + 1 <= H - 1
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    bb = np.arange(B)[:, None, None]
    g = []
    tmax = np.zeros(fx.shape)
    for c in range(2):
        Gc = G[:, c]
        # a +1 corner outside the frame has weight 0 and is not read
        v00 = Gc[bb, y0, x0]
        v01 = np.where(x1ok, Gc[bb, y0, x1], 0.0)
        v10 = np.where(y1ok, Gc[bb, y1, x0], 0.0)
        v11 = np.where(x1ok & y1ok, Gc[bb, y1, x1], 0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            g.append((1 - ay) * ((1 - ax) * v00 + ax * v01) + ay * ((1 - ax) * v10 + ax * v11))
            tmax = np.maximum(tmax, np.nan_to_num(np.max(np.abs([v00, v01, v10, v11]), axis=0), nan=np.inf))
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = fxs + g[0], fys + g[1]
        err = sx * sx + sy * sy
        n2 = (fxs * fxs + fys * fys) + (g[0] * g[0] + g[1] * g[1])
        thr = alpha * n2 + beta
        occ = ~((err <= thr) & (err < np.inf))
        # fp32 error bound of the kernel's err and threshold together (derivation: error_bound's docstring)
        bound = error_bound(tmax, err, n2, thr)
    err = np.where(inside, err, np.inf)
    occ = np.where(inside, occ, True)
    return {"err": err, "occ": occ, "thr": thr, "inside": inside, "bound": bound, "bound_err": bound_err(tmax, err)}


def bound_err(T, E):
    """|err_fp32 - err_fp64| <= U * (30 T sqrt(E) + 4 E), T = the largest |tap| of G, E = the exact err.

    The kernel rounds once per operation (no contraction); u = 2^-24.
      weights: t = d - floor(d) is exact except for d in (-1, 0), where 1 + d rounds once: |dt| <= u/2;
               1 - t rounds once more: |d(1-t)| <= u.
      blend:   g = wy0 (wx0 v00 + ax v01) + ay (wx0 v10 + ax v11): every tap passes through two products and
               two sums (4 roundings) with two weights in error by <= u each (absolute, weights <= 1); the
               weights sum to 1, so |dg| <= (4 + 2 + 2) u T, taken as 10 u T for the second-order terms.
      s = F + g: |ds| <= 10 u T + u |s| per component.
      err = sx^2 + sy^2: 2 |s| |ds| per square + one rounding per square + one for the sum:
               |derr| <= 2 (|sx| + |sy|) 10 u T + 2 u E + u E + u E <= 28.3 u T sqrt(E) + 4 u E
               (|sx| + |sy| <= sqrt(2 E)), taken as 30 u T sqrt(E) + 4 u E.
    This is a few ulps of the largest intermediate: T sqrt(E) <= |F|^2 + |g|^2 up to a constant."""
    with np.errstate(invalid="ignore", over="ignore"):
        return U * (30.0 * T * np.sqrt(E) + 4.0 * E) + 1e-37


def error_bound(T, E, N, thr):
    """bound_err plus the threshold's own fp32 error: thr = alpha (|F|^2 + |g|^2) + beta with N = |F|^2 + |g|^2:
    |g|^2 inherits 2 |g| |dg| <= 2 sqrt(2 N) 10 u T <= 30 u T sqrt(N), the squares and sums round 4 u N in
    all, the product and the final sum one rounding of thr each: alpha u (30 T sqrt(N) + 4 N) + 2 u thr."""
    with np.errstate(invalid="ignore", over="ignore"):
        return bound_err(T, E) + ALPHA * U * (30.0 * T * np.sqrt(N) + 4.0 * N) + 2.0 * U * thr


def fb_reference(fw, bw, alpha=ALPHA, beta=BETA):
    """(direction fw, direction bw) of the check in fp64."""
    return fb_direction(fw, bw, alpha, beta), fb_direction(bw, fw, alpha, beta)


# ----------------------------------------------------------------------------- the random smooth case


def _field(rng, B, comps):
    """A smooth analytic flow field: per image a sum of `comps` low-frequency sinusoids; returns a function
    (x, y arrays [B,H,W]) -> [B,2,H,W] float64."""
    k = rng.uniform(0.5, 2.0, size=(B, 2, comps, 2))     # cycles over the frame, per axis
    ph = rng.uniform(0, 2 * np.pi, size=(B, 2, comps))
    am = rng.uniform(0.3, 1.0, size=(B, 2, comps)) / comps

    def f(x, y, H, W, amp):
        out = np.zeros((B, 2) + x.shape[1:])
        for c in range(2):
            for m in range(comps):
                arg = (2 * np.pi * (k[:, c, m, 0, None, None] * x / W + k[:, c, m, 1, None, None] * y / H)
                       + ph[:, c, m, None, None])
                out[:, c] += am[:, c, m, None, None] * np.sin(arg)
            out[:, c] *= amp[c]
        return out
    return f


@functools.lru_cache(maxsize=None)
def random_case(B, H, W, seed=11):
    """fw smooth with magnitudes up to about 40 px (a quarter of the frame where that is less), bw = -fw warped
    back to the second frame (first order: bw(q) = -fw(q - fw(q))) plus per-pixel noise whose amplitude is
    drawn per pixel from {0, 0.02, 0.3, 1, 4} px: consistent, borderline and occluded pixels side by side."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    f = _field(rng, B, 3)
    amp = (min(40.0, W / 4.0), min(40.0, H / 4.0))
    x = np.broadcast_to(np.arange(W, dtype=np.float64)[None, None, :], (B, H, W))
    y = np.broadcast_to(np.arange(H, dtype=np.float64)[None, :, None], (B, H, W))
    fw = f(x, y, H, W, amp)
    back = f(x, y, H, W, amp)
    bw = -f(x - back[:, 0], y - back[:, 1], H, W, amp)
    level = rng.choice([0.0, 0.02, 0.3, 1.0, 4.0], size=(B, 1, H, W))
    bw = bw + level * rng.standard_normal((B, 2, H, W))
    return fw.astype(np.float32), bw.astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES)
def test_random_case_is_usable(shape):
    """The kernel test leaves out the pixels whose fp64 margin |err - threshold| is within the fp32 bound: on
    the fp64 reference alone they are at most 1 % of the frame, and the case exercises both outcomes."""
    fw, bw = random_case(*shape)
    assert float(np.abs(fw).max()) <= 41.0 and (shape != SHAPES[2] or float(np.abs(fw).max()) > 20.0)
    for d in fb_reference(fw, bw):
        ins = d["inside"]
        with np.errstate(invalid="ignore"):
            close = ins & (np.abs(d["err"] - d["thr"]) <= d["bound"])
        assert close.sum() <= 0.01 * ins.size, (shape, int(close.sum()))
        assert np.all(d["occ"][~ins]) and np.all(np.isinf(d["err"][~ins]))
        if shape != SHAPES[0]:
            occ_in = d["occ"][ins]
            assert 0.05 < occ_in.mean() < 0.95, occ_in.mean()      # occluded and consistent pixels inside
            assert 0.02 < (~ins).mean() < 0.9                       # and pixels that leave the frame
        assert float(d["bound"][ins].max()) < 1e-2                  # the bound is fp32 rounding, not slack


# ----------------------------------------------------------------------------- vs grid_sample


def test_restatement_matches_grid_sample_on_interior_targets():
    """On targets strictly inside the frame (every corner in it) the definition is grid_sample's bilinear with
    align_corners=True: pixel coordinates map to the normalised grid as 2 p / (S - 1) - 1."""
    B, H, W = 2, 19, 23
    rng = np.random.default_rng(5)
    fw = rng.uniform(-6, 6, size=(B, 2, H, W))
    bw = rng.uniform(-6, 6, size=(B, 2, H, W))
    d = fb_direction(fw, bw)
    jj = np.arange(W)[None, None, :]
    ii = np.arange(H)[None, :, None]
    px, py = jj + fw[:, 0], ii + fw[:, 1]
    interior = (px > 0) & (px < W - 1) & (py > 0) & (py < H - 1)
    assert 0.2 < interior.mean() < 0.95
    grid = torch.from_numpy(np.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], -1))
    g = torch.nn.functional.grid_sample(torch.from_numpy(bw), grid, mode="bilinear", padding_mode="zeros",
                                        align_corners=True).numpy()
    err = (fw[:, 0] + g[:, 0]) ** 2 + (fw[:, 1] + g[:, 1]) ** 2
    thr = ALPHA * ((fw ** 2).sum(1) + (g ** 2).sum(1)) + BETA
    assert np.all(d["inside"][interior])
    assert np.max(np.abs(err - d["err"])[interior]) < 1e-9     # fp64 both: normalise / unnormalise rounding only
    safe = interior & (np.abs(err - thr) > 1e-9)
    assert np.array_equal((err > thr)[safe], d["occ"][safe])


def test_restatement_edge_rules():
    """Zero flows: err 0, nothing occluded.  An integer shift with bw = -fw: err exactly 0 inside, the occluded
    band is the shift's width on the side the flow points to.  A target exactly on the last column / row is in
    the frame and takes the corner's value, whatever lies beyond (NaN here would show a read)."""
    z = np.zeros((1, 2, 5, 7))
    for d in fb_reference(z, z):
        assert not d["occ"].any() and np.all(d["err"] == 0)
    fw = np.zeros((1, 2, 6, 9))
    fw[:, 0] = 2
    fw[:, 1] = -1
    dfw, dbw = fb_reference(fw, -fw)
    assert np.array_equal(dfw["occ"][0], (np.arange(9)[None, :] > 6) | (np.arange(6)[:, None] < 1))
    assert np.array_equal(dbw["occ"][0], (np.arange(9)[None, :] < 2) | (np.arange(6)[:, None] > 4))
    assert np.all(dfw["err"][~dfw["occ"]] == 0) and np.all(np.isinf(dfw["err"][dfw["occ"]]))
    F = np.zeros((1, 2, 4, 5))
    F[0, 0] = 4 - np.arange(5)[None, :]        # every pixel targets column W-1
    G = np.arange(40, dtype=np.float64).reshape(1, 2, 4, 5)
    d = fb_direction(F, G)
    assert d["inside"].all()
    want = (F[0, 0] + G[0, 0, :, 4:5]) ** 2 + G[0, 1, :, 4:5] ** 2
    assert np.array_equal(d["err"][0], want)
    bad = fw.copy()
    bad[0, 0, 2, 3] = np.nan
    bad[0, 1, 1, 1] = np.inf
    d = fb_direction(bad, -fw)
    assert d["occ"][0, 2, 3] and d["occ"][0, 1, 1]


# ----------------------------------------------------------------------------- argument validation


def _model():
    from raft_optical_flow_amd import RAFT
    return RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False)).eval()


def test_stream_bidirectional_argument_checks():
    from raft_optical_flow_amd import BidirectionalFlow, FlowStream
    m = _model()
    s = m.stream(iters=2, bidirectional=True, fb_alpha=0.02, fb_beta=1)
    assert isinstance(s, FlowStream) and s.bidirectional and (s.fb_alpha, s.fb_beta) == (0.02, 1.0)
    assert not m.stream().bidirectional                       # the default is the one-directional stream
    assert BidirectionalFlow._fields == ("low_fw", "up_fw", "low_bw", "up_bw", "occ_fw", "occ_bw", "err_fw", "err_bw")
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="bidirectional"):
            m.stream(bidirectional=bad)
    for kw in ({"fb_alpha": -0.1}, {"fb_beta": float("nan")}, {"fb_alpha": float("inf")}):
        with pytest.raises(ValueError, match="finite and not negative"):
            m.stream(bidirectional=True, **kw)
    with pytest.raises(TypeError, match="must be a number"):
        m.stream(bidirectional=True, fb_beta="0.5")
    # the frame checks are the one-directional stream's, before any device work
    with pytest.raises(ValueError, match="a frame is"):
        s.push(torch.zeros(3, 16, 16))
    s.close()
    with pytest.raises(RuntimeError, match="close"):
        s.push(torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match="iters"):
        m.stream(iters=0, bidirectional=True)


def test_fb_consistency_argument_checks():
    from raft_optical_flow_amd.utils import fb_consistency
    a = torch.zeros(1, 2, 8, 8)
    with pytest.raises(RuntimeError, match="ROCm GPU only"):       # CPU tensors: there is no CPU path
        fb_consistency(a, a)
    with pytest.raises(TypeError, match="float32"):
        fb_consistency(a.double(), a)
    with pytest.raises(TypeError, match="float32"):
        fb_consistency(a, a.half())
    with pytest.raises(TypeError, match="tensor"):
        fb_consistency(a.numpy(), a)
    for bad in (torch.zeros(2, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 0, 8)):
        with pytest.raises(ValueError, match=r"\[B, 2, H, W\]"):
            fb_consistency(bad, bad)
    with pytest.raises(ValueError, match="differ in shape"):
        fb_consistency(a, torch.zeros(1, 2, 8, 9))
    with pytest.raises(ValueError, match="finite and not negative"):
        fb_consistency(a, a, alpha=-1.0)


FAKE = 1 << 20  # 16-byte aligned stand-in pointers: an argument error returns before any launch


def test_bidi_symbols_and_argument_errors():
    lib = _lib.load()
    for name in ("raft_fb_consistency", "raft_stream_carry_n"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.raft_hip_abi_version() == 19   # additive entries: the ABI version did not move
    err = lib.raft_hip_last_error
    p = [FAKE * k for k in range(1, 7)]

    def fb(**kw):
        a = dict(fw=p[0], fsb=128, fsc=64, fp=8, bw=p[1], bsb=128, bsc=64, bp=8, top=0, left=0, B=1, H=8, W=8,
                 alpha=0.01, beta=0.5, o0=p[2], o1=p[3], e0=p[4], e1=p[5])
        a.update(kw)
        return lib.raft_fb_consistency(*a.values(), None)

    for k in ("fw", "bw", "o0", "o1", "e0", "e1"):
        assert fb(**{k: None}) == -1 and b"null pointer" in err()
    for kw in ({"B": 0}, {"H": -1}, {"W": 0}, {"B": 1 << 10, "H": 1 << 10, "W": 1 << 10, "fp": 1 << 10, "bp": 1 << 10}):
        assert fb(**kw) == -1 and b"bad size" in err()
    assert fb(top=-1) == -1 and b"negative crop" in err()
    for kw in ({"fp": 7}, {"bp": 7}, {"left": 1}, {"fsb": -1}):
        assert fb(**kw) == -1 and b"bad strides" in err()
    for kw in ({"alpha": -1.0}, {"beta": float("nan")}, {"alpha": float("inf")}):
        assert fb(**kw) == -1 and b"finite and not negative" in err()
    for kw in ({"fw": p[0] + 2}, {"e0": p[4] + 4}, {"o1": p[3] + 1}):
        assert fb(**kw) == -1 and b"misaligned" in err()
    assert fb(o1=p[2]) == -1 and b"share an output" in err()

    def carry(segs, n=None):
        arr = (_lib.Copy2D * max(len(segs), 1))()
        for a, s in zip(arr, segs):
            a.src, a.src_ld, a.dst, a.dst_ld, a.rows, a.cols = s
        return lib.raft_stream_carry_n(arr, len(segs) if n is None else n, None)

    ok = (p[0], 64, p[1], 64, 4, 64)
    assert lib.raft_stream_carry_n(None, 1, None) == -1 and b"null pointer" in err()
    assert carry([ok], n=0) == -1 and b"segments" in err()
    assert carry([ok] * 9) == -1 and b"segments" in err()
    assert carry([(None,) + ok[1:]]) == -1 and b"null pointer in segment 0" in err()
    for bad in ((p[0], 32, p[1], 64, 4, 64), (p[0], 64, p[1], 64, 0, 64), (p[0], 64, p[1], 8, 4, 64)):
        assert carry([ok, bad]) == -1 and b"bad size in segment 1" in err()
    assert carry([(p[0], 64, p[0], 64, 4, 64)]) == -1 and b"in-place" in err()
    assert ctypes.sizeof(_lib.Copy2D) == 48 and _lib.CARRY_MAX_SEGS == 8
