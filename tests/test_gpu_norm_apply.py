"""raft_instnorm_apply, raft_norm_apply_affine and raft_groupnorm_stats against fp64 (tests/elementwise_oracle.py).

The applies run at B = 2 with (HW, C) = (77, 64) and (300, 96): relu_mode x residual form x the three leading
dimensions, each in {C, C + 4}.  Inputs carry a per-channel offset of up to 50 standard deviations, so a slip in
`x - mean` shows; the statistics are random per (image, channel) and the kernel and the reference read the same
fp32 values.  Every output buffer is pre-filled with -7.0 and everything outside the C written columns of the
B*HW written rows must still hold it.

How each kernel of raft_instnorm_apply is forced (the entry picks by alignment):
  vector (instnorm_apply4_kernel)   C % 4 == 0, every ld % 4 == 0, every pointer 16-byte aligned;
  scalar (instnorm_apply_kernel)    (a) ld = C + 1,  (b) x offset by 4 bytes with C % 4 == 0,  (c) C = 6.
Forms (a) and (b) read the vector run's data and (c) its first 6 channels; all three must agree with the vector
run bit for bit (the same fp32 expressions per element).

Tolerance of the applies (derived, per element): OPS * 2^-24 * mag * 2, where mag is the largest magnitude of
any intermediate on that element's path (the oracle returns it) and OPS counts the rounded fp32 operations of the
longest path: normalise (subtract, multiply), scale by gamma, shift by beta = 4, the residual's own four, the
final add: 9 for raft_norm_apply_affine; raft_instnorm_apply has no scale / shift: 2 + 2 + 1 = 5.  relu rounds
nothing.  The factor 2 allows for fma contraction (at most one more rounding per contracted pair)."""
import itertools

import numpy as np
import pytest
import torch

import elementwise_oracle as EO

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0
OPS_APPLY = 5
OPS_AFFINE = 9
SHAPES = [(2, 77, 64), (2, 300, 96)]   # B, HW (ragged against 256 / more than one block), C


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


def dev_rows(vals, ld, off=0):
    """vals: device [N, C] -> (flat buffer filled with SENT, byte pointer to rows [N][ld] `off` floats into it)."""
    n, c = vals.shape
    flat = torch.full((off + n * ld + 5,), SENT, device=DEV)
    flat[off:off + n * ld].view(n, ld)[:, :c] = vals
    return flat, flat.data_ptr() + 4 * off


def read_rows(flat, n, c, ld, off=0):
    """The [N, C] written block as numpy, after asserting that nothing else in the buffer changed."""
    host = flat.cpu().numpy()
    block = host[off:off + n * ld].reshape(n, ld)
    vals = block[:, :c].copy()
    block[:, :c] = SENT
    assert np.all(host == SENT), "the kernel wrote outside its C columns / B*HW rows"
    return vals


def make_case(B, HW, C, seed):
    """x, resid [B*HW, C] float32 with per-channel offsets up to 50 sd; stats / resid stats [B, C, 2] random per
    (image, channel); gamma / beta / resid gamma / resid beta [C]."""
    r = np.random.default_rng(seed)

    def field():
        sd = r.uniform(0.5, 4.0, size=C)
        off = r.uniform(-50, 50, size=C) * sd
        x = (r.normal(size=(B, HW, C)) * sd + off).astype(np.float32)
        mean = off + r.normal(size=(B, C)) * sd * 0.3
        rstd = r.uniform(0.5, 2.0, size=(B, C)) / sd
        return x, np.stack([mean, rstd], -1).astype(np.float32)

    x, st = field()
    res, rst = field()
    aff = [r.normal(size=C).astype(np.float32) * s for s in (1.5, 2.0, 1.5, 2.0)]
    return x, st, res, rst, aff


def launch(entry, B, HW, C, xd, st, rd, rst, mode, ld, rld, old, xoff=0, aff=(None,) * 4):
    """One launch of `entry`; xd / rd device [B*HW, C] (rd None: no residual), st / rst device stats (rst None:
    raw residual), aff = device (gamma, beta, resid_gamma, resid_beta) for the affine entry.  Returns the output
    block [B*HW, C] as numpy."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    n = B * HW
    xbuf, xp = dev_rows(xd, ld, xoff)
    rbuf, rp = dev_rows(rd, rld) if rd is not None else (None, None)
    out = torch.full((n * old + 5,), SENT, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    if entry == "raft_instnorm_apply":
        _lib.call(entry, xp, ld, p(st), rp, rld, p(rst), mode, out.data_ptr(), old, B, HW, C, K.stream_handle())
    else:
        g, b, rg, rb = aff
        _lib.call(entry, xp, ld, p(st), p(g), p(b), rp, rld, p(rst), p(rg), p(rb), mode, out.data_ptr(), old, B, HW,
                  C, K.stream_handle())
    torch.cuda.synchronize()
    return read_rows(out, n, C, old)


def check(got, ref, mag, ops, what):
    tol = ops * EO.U * mag * 2
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > tol
    assert not bad.any(), (what, float(err.max()), float((err / np.maximum(tol, 1e-300)).max()), int(bad.sum()))


def ld_grid(C, resid):
    """(ld, resid_ld, out_ld), each in {C, C + 4}; resid_ld only matters with a residual."""
    opts = (C, C + 4)
    return [(a, b, c) for a in opts for b in (opts if resid != "none" else (C,)) for c in opts]


@pytest.mark.parametrize("resid", ["none", "raw", "stats"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-HW%d-C%d" % s)
def test_instnorm_apply_vector_and_scalar(shape, mode, resid):
    """Both kernels of raft_instnorm_apply over the whole (ld, resid_ld, out_ld) grid, against fp64 within
    5 * 2^-24 * mag * 2 per element, and against each other bit for bit."""
    B, HW, C = shape
    n = B * HW
    x, st, res, rst, _ = make_case(B, HW, C, seed=HW + mode)
    kw = {} if resid == "none" else dict(resid=res) if resid == "raw" else dict(resid=res, resid_stats=rst)
    ref, mag = EO.norm_apply(x, st, mode, **kw)
    ref, mag = ref.reshape(n, C), mag.reshape(n, C)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    xd, std = t(x.reshape(n, C)), t(st)
    rd = t(res.reshape(n, C)) if resid != "none" else None
    rstd = t(rst) if resid == "stats" else None
    # form (c): the first 6 channels as a tensor of their own (C = 6: no quads)
    x6, st6 = xd[:, :6].contiguous(), std[:, :6].contiguous()
    r6 = rd[:, :6].contiguous() if rd is not None else None
    rst6 = rstd[:, :6].contiguous() if rstd is not None else None
    run = lambda *a, **k: launch("raft_instnorm_apply", *a, **k)
    for ld, rld, old in ld_grid(C, resid):
        what = (ld, rld, old)
        vec = run(B, HW, C, xd, std, rd, rstd, mode, ld, rld, old)                   # vector kernel
        check(vec, ref, mag, OPS_APPLY, ("vector",) + what)
        s_ld = run(B, HW, C, xd, std, rd, rstd, mode, C + 1, rld, old)               # scalar (a): ld = C + 1
        s_off = run(B, HW, C, xd, std, rd, rstd, mode, ld, rld, old, xoff=1)         # scalar (b): x + 4 bytes
        s_c6 = run(B, HW, 6, x6, st6, r6, rst6, mode, ld - C + 6, rld - C + 6, old - C + 6)   # scalar (c): C = 6
        for name, got in (("ld=C+1", s_ld), ("x+4B", s_off)):
            check(got, ref, mag, OPS_APPLY, (name,) + what)
            assert np.array_equal(got, vec), (name,) + what
        check(s_c6, ref[:, :6], mag[:, :6], OPS_APPLY, ("C=6",) + what)
        assert np.array_equal(s_c6, vec[:, :6]), ("C=6",) + what


@pytest.mark.parametrize("resid", ["none", "raw", "stats"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-HW%d-C%d" % s)
def test_norm_apply_affine(shape, mode, resid):
    """raft_norm_apply_affine over the same grid, with gamma / beta each present or absent (and the residual's
    pair too where the residual is normalised), against fp64 within 9 * 2^-24 * mag * 2 per element; with no
    affine at all it equals raft_instnorm_apply bit for bit."""
    B, HW, C = shape
    n = B * HW
    x, st, res, rst, aff = make_case(B, HW, C, seed=100 + HW + mode)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    xd, std = t(x.reshape(n, C)), t(st)
    rd = t(res.reshape(n, C)) if resid != "none" else None
    rstd = t(rst) if resid == "stats" else None
    affd = [t(a) for a in aff]
    on_off = list(itertools.product((False, True), repeat=2))
    for g_on, b_on in on_off:
        for rg_on, rb_on in (on_off if resid == "stats" else [(False, False)]):
            use = (g_on, b_on, rg_on, rb_on)
            kw = dict(gamma=aff[0] if g_on else None, beta=aff[1] if b_on else None)
            if resid != "none":
                kw["resid"] = res
            if resid == "stats":
                kw.update(resid_stats=rst, resid_gamma=aff[2] if rg_on else None, resid_beta=aff[3] if rb_on else None)
            ref, mag = EO.norm_apply(x, st, mode, **kw)
            ref, mag = ref.reshape(n, C), mag.reshape(n, C)
            dev_aff = tuple(a if on else None for a, on in zip(affd, use))
            for ld, rld, old in ld_grid(C, resid):
                got = launch("raft_norm_apply_affine", B, HW, C, xd, std, rd, rstd, mode, ld, rld, old, aff=dev_aff)
                check(got, ref, mag, OPS_AFFINE, (use, ld, rld, old))
                if not any(use):
                    plain = launch("raft_instnorm_apply", B, HW, C, xd, std, rd, rstd, mode, ld, rld, old)
                    assert np.array_equal(got, plain), (ld, rld, old)


def test_norm_apply_affine_ignores_resid_affine_without_resid_stats():
    """include/raft_hip.h: the residual is scaled 'likewise' only where it is normalised; a raw residual is added
    as it is, whatever resid_gamma / resid_beta hold."""
    B, HW, C = 2, 77, 64
    x, st, res, _, aff = make_case(B, HW, C, seed=5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ref, mag = EO.norm_apply(x, st, 2, resid=res, gamma=aff[0], beta=aff[1])
    got = launch("raft_norm_apply_affine", B, HW, C, t(x.reshape(-1, C)), t(st), t(res.reshape(-1, C)), None, 2, C, C,
                 C, aff=tuple(t(a) for a in aff))
    check(got, ref.reshape(-1, C), mag.reshape(-1, C), OPS_AFFINE, "raw residual")


@pytest.mark.parametrize("ld", [6, 8, 11])
def test_instnorm_stats_fits_its_workspace(ld):
    """raft_instnorm_workspace_floats is what raft_instnorm_stats needs: on a workspace of exactly that many
    floats nothing behind it is written, and the statistics (C = 6 / ld = 8 with C = 8: the scalar and the vector
    partial kernel) match fp64 at test_instnorm_stats_vs_fp64's bounds.  Bad sizes give 0."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    lib = _lib.load()
    B, HW, C = 2, 300, 8 if ld == 8 else 6
    nws = lib.raft_instnorm_workspace_floats(B, HW, C)
    assert nws > 0 and lib.raft_instnorm_workspace_floats(0, HW, C) == 0 and lib.raft_instnorm_workspace_floats(B, HW, 0) == 0
    x = (np.random.default_rng(ld).normal(size=(B, HW, C)) * 3 + np.linspace(-40, 40, C)).astype(np.float32)
    xbuf, xp = dev_rows(torch.from_numpy(x.reshape(B * HW, C)).to(DEV), ld)
    ws = torch.full((nws + 64,), SENT, device=DEV)
    st = torch.full((B * C * 2 + 4,), SENT, device=DEV)
    _lib.call("raft_instnorm_stats", xp, ld, B, HW, C, 1e-5, st.data_ptr(), ws.data_ptr(), K.stream_handle())
    torch.cuda.synchronize()
    assert bool((ws[nws:] == SENT).all()) and bool((st[B * C * 2:] == SENT).all())
    got = st[:B * C * 2].cpu().numpy().astype(np.float64).reshape(B, C, 2)
    mean, rstd = EO.groupnorm_stats(x, C)
    assert np.abs(got[..., 0] - mean).max() < 1e-5 * max(1.0, float(np.abs(mean).max()))
    assert np.abs((got[..., 1] - rstd) / rstd).max() < 1e-5


@pytest.mark.parametrize("per_group", [8, 12, 1])
def test_groupnorm_stats_vs_fp64(per_group):
    """raft_groupnorm_stats at C / G in {8, 12, 1}, HW = 77, ld > C, B = 2, one group per image sitting 1e3
    standard deviations from zero: mean to 1e-5 * max(1, |mean|), rstd to 1e-5 relative (the bounds of
    test_instnorm_stats_vs_fp64), every channel carrying its group's pair."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    B, HW, C, ld = 2, 77, 96, 96 + 5
    G = C // per_group
    r = np.random.default_rng(per_group)
    sd = np.repeat(r.uniform(0.5, 2.0, size=(B, G)), per_group, axis=1)
    off = np.repeat(r.uniform(-5, 5, size=(B, G)), per_group, axis=1) * sd
    off[0, :per_group] = 1e3 * sd[0, 0]                    # image 0, group 0
    off[1, C - per_group:] = -1e3 * sd[1, C - 1]           # image 1, last group
    x = (r.normal(size=(B, HW, C)) * sd[:, None] + off[:, None] + r.normal(size=C) * 0.2).astype(np.float32)
    xbuf, xp = dev_rows(torch.from_numpy(x.reshape(B * HW, C)).to(DEV), ld)
    st = torch.full((B * C * 2 + 4,), SENT, device=DEV)
    _lib.call("raft_groupnorm_stats", xp, ld, B, HW, C, G, 1e-5, st.data_ptr(), K.stream_handle())
    torch.cuda.synchronize()
    host = st.cpu().numpy().astype(np.float64)
    assert np.all(host[B * C * 2:] == SENT)
    got = host[:B * C * 2].reshape(B, C, 2)
    mean, rstd = EO.groupnorm_stats(x, G)
    assert np.abs(mean).max() > 400
    e_mean = float(np.abs(got[..., 0] - mean).max())
    e_rstd = float(np.abs((got[..., 1] - rstd) / rstd).max())
    print(f"groupnorm C/G={per_group}: mean err {e_mean:.3e} (|mean| max {np.abs(mean).max():.1f}), rstd rel {e_rstd:.3e}")
    assert e_mean < 1e-5 * max(1.0, float(np.abs(mean).max()))
    assert e_rstd < 1e-5
    # one pair per group, repeated over its channels
    gg = got.reshape(B, G, per_group, 2)
    assert np.array_equal(gg, np.broadcast_to(gg[:, :, :1], gg.shape))
