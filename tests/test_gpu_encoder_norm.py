"""The InstanceNorm encoders' conv path on every kernel form, at kernel level, against fp64.

An InstanceNorm encoder is never normalised by a pass over its activations: the conv that produces a raw output
also writes per-wave (count, mean, M2) partials (raft_conv2d_params.stats_part), one of three merges turns them into
{mean, rstd}, and the next 3x3 conv applies relu((x - mean) * rstd) in its loaders (in_norm).  All of it runs in
instantiations that exist only for these convs (conv_halo_kernel<ENC = true>, the GEMM kernel's per-image M tiling,
the stem's statistics call).  For every entry of conv_forms.ENC_TABLE (form, slots and in_norm_ok asserted before
each launch) in f16x3, bf16 and f16, with the operands laid out as the engine lays them out except that the output
is a column sub-view of a wider sentinel-filled buffer with guard rows, stats_ld = N + 4, stats_part starts as NaN
with guard slots around it, and the data carries the conditions of encoder_norm_data (images on scales x1 / x20, a
constant channel, a channel whose bias is 30 deviations, input offsets of both signs):

(a) the output against torch fp64 conv2d(act(instance_norm(x))) (the plain conv without in_norm), {mean, rstd} fed
    as the fp64 statistics rounded to float32; per image, CONV_TOL[prec] x max(1, max |ref|); sentinels untouched;
(b) the partials slot by slot over the footprints include/raft_hip.h documents: count exactly, mean and M2 against
    fp64 over the same pixels of the kernel's own output (elementwise_oracle.partials_mismatch states the float32
    bounds), empty slots (0, 0, 0), nothing outside [slot][n < N] changed from NaN;
(c) raft_instnorm_merge, _merge_ws and _merge_fused on those partials against the fp64 statistics of the kernel's
    own output, at 4 x the measured error of the float32 restatement of the documented algorithm
    (elementwise_oracle.ENC_STATS_MEASURED); _fused == _ws bit for bit, counters left zero over two
    calls, every merge bit-identical run to run; the constant channel gives its bias and 1 / sqrt(eps).

test_synthetic_merges runs the three merges on hand-made partials.  tests/test_encoder_norm_host.py shows on the
CPU that the comparisons used here reject wrong references."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import conv_forms as CF
import elementwise_oracle as EO
import encoder_norm_data as ED
from test_gpu_parity import CONV_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.0     # sentinel of unwritten columns / guard rows
G = 4           # guard rows above and below every buffer
GS = 2          # guard slots before and after the partials
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    lib = _lib.load()
    assert (lib.raft_conv2d_set_halo_ks(0), lib.raft_conv2d_set_halo_loaders(0)) == (2, 8)   # the table's defaults
    yield
    for cached in (_dev_data, _packed):
        cached.cache_clear()
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- data (shared, never modified)


@functools.lru_cache(maxsize=None)
def _dev_data(key, variant):
    d = ED.case_data(key, variant)
    B, H, W, cin = key[:4]
    return dict(xrows=ED.rows_of(d["x"]).reshape(B * H * W, cin).contiguous().to(DEV),
                ref=ED.rows_of(d["ref"]).contiguous().to(DEV),
                in_stats=None if d["in_stats"] is None else d["in_stats"].to(DEV))


@functools.lru_cache(maxsize=None)
def _packed(key, variant, prec):
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    d = ED.case_data(key, variant)
    pc = K.pack_conv(d["w"], d["b"], key[7], d["pad"], device=DEV)
    pc.precision = _lib.PRECISIONS[prec]
    return pc


def _buf(rows, ld, fill=SENT):
    whole = torch.full((rows + 2 * G, ld), fill, device=DEV)
    return whole, whole[G:G + rows]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- one launch


def _run(c, variant="std", form=None, stats=True):
    """Launches the entry's conv with its features set (form asserted first) and returns its buffers."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    lib = _lib.load()
    key = ED.key_of(c)
    d, dd = ED.case_data(key, variant), _dev_data(key, variant)
    n, ho, wo = c.n, d["ho"], d["wo"]
    assert (ho, wo) == CF.out_hw(c)
    npix, rows_in = c.B * ho * wo, c.B * c.H * c.W
    xw, X = _buf(rows_in, c.cin if c.cin % 4 else c.cin + 8)
    X[:, :c.cin] = dd["xrows"]
    x_before = xw.clone()
    ow, O = _buf(npix, n + 12)
    out = K.Rows(O, 4, n)
    pc = _packed(key, variant, c.prec)
    assert (pc.bias is None) == (variant == "nobias")
    p = K.conv_params(pc, K.Rows(X, 0, c.cin), c.B, c.H, c.W, out)
    ld_s = n + 4
    partw = part = None
    if stats and c.stats:
        partw = torch.full(((c.B * max(c.slots, 1) + 2 * GS) * ld_s * 4,), NAN, device=DEV)
        part = partw[GS * ld_s * 4:(GS + c.B * max(c.slots, 1)) * ld_s * 4]
        p.stats_part, p.stats_ld = part.data_ptr(), ld_s
    if c.in_norm:
        p.in_norm, p.in_norm_relu = dd["in_stats"].data_ptr(), int(d["relu"])
    if c.stats and c.slots == 0 and stats:     # RAFT-small's stem: the launch rejects stats_part
        return dict(rc=lib.raft_conv2d(ctypes.byref(p), K.stream_handle()))
    got_form = _lib.conv_form(p).astuple()
    assert got_form == (form or c.form), (c.name, got_form, form or c.form)
    assert lib.raft_conv2d_stats_slots(ctypes.byref(p)) == c.slots, c.name
    assert lib.raft_conv2d_in_norm_ok(ctypes.byref(p)) == c.in_norm_ok, c.name
    K.conv_launch(p)(K.stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(xw, x_before), (c.name, "the input changed")
    inner = ow[G:-G, 4:4 + n]
    rest = ow.clone()
    rest[G:-G, 4:4 + n] = SENT
    assert bool((rest == SENT).all()), (c.name, "wrote outside its rows / columns")
    return dict(y=inner.reshape(c.B, ho * wo, n).contiguous(), ow=ow, partw=partw, part=part, ld_s=ld_s, ho=ho, wo=wo,
                ref=dd["ref"], d=d)


# ----------------------------------------------------------------------------- the merges


def _merge_all(part, slots, B, C, ld, eps=EO.STATS_EPS):
    """The three merges, twice each, on part ([B][slots][ld][4] floats on the device).  Asserts run-to-run
    bit-identity, _fused == _ws bit for bit and the counters left zero; returns {name: stats [B, C, 2]}."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    lib = _lib.load()
    s = K.stream_handle()
    nws = int(lib.raft_instnorm_merge_ws_floats(slots, B, C))
    ncnt = int(lib.raft_instnorm_merge_counters(B, C))
    assert nws > 0 and ncnt > 0
    counters = torch.zeros(ncnt, dtype=torch.int32, device=DEV)
    got = {"merge": [], "ws": [], "fused": []}
    for _ in range(2):
        st = torch.full((B * C * 2,), NAN, device=DEV)
        _lib.call("raft_instnorm_merge", part.data_ptr(), slots, B, C, ld, eps, st.data_ptr(), s)
        got["merge"].append(st)
        ws = torch.full((nws,), NAN, device=DEV)   # (every double of it is written before it is read)
        st = torch.full((B * C * 2,), NAN, device=DEV)
        _lib.call("raft_instnorm_merge_ws", part.data_ptr(), slots, B, C, ld, eps, ws.data_ptr(), st.data_ptr(), s)
        got["ws"].append(st)
        ws = torch.full((nws,), NAN, device=DEV)
        st = torch.full((B * C * 2,), NAN, device=DEV)
        _lib.call("raft_instnorm_merge_fused", part.data_ptr(), slots, B, C, ld, eps, ws.data_ptr(), counters.data_ptr(),
                  st.data_ptr(), s)
        torch.cuda.synchronize()
        got["fused"].append(st)
        assert int(counters.abs().sum()) == 0, "raft_instnorm_merge_fused left a counter set"
    for name, (a, b) in got.items():
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(_bits(a), _bits(b)), (name, "not bit-identical run to run")
    assert torch.equal(_bits(got["ws"][0]), _bits(got["fused"][0])), "_merge_fused differs from _merge_ws"
    return {name: v[0].view(B, C, 2) for name, v in got.items()}


# ----------------------------------------------------------------------------- every table entry


def _check_entry(c, variant):
    r = _run(c, variant)
    y, n, B = r["y"], c.n, c.B
    # (a) the output
    bad, worst = EO.conv_mismatch(y, r["ref"], CONV_TOL[c.prec])
    line = f"ENCERR case={c.name} variant={variant} out_err/bound={worst:.3e}"
    if not c.slots:
        print(line)
        assert bad == 0, (c.name, worst)
        return
    # (b) the partials, slot by slot
    pv = r["part"].view(B, c.slots, r["ld_s"], 4)
    edge = GS * r["ld_s"] * 4
    assert bool(torch.isnan(r["partw"][:edge]).all()) and bool(torch.isnan(r["partw"][-edge:]).all()), "guard slots"
    assert bool(torch.isnan(pv[:, :, n:]).all()), (c.name, "wrote columns >= N of the partials")
    assert bool(torch.isfinite(pv[:, :, :n]).all()), (c.name, "a partial (or its fourth float) was not written")
    got_part = tuple(pv[:, :, :n, k] for k in range(3))
    ids, slots = EO.stats_slot_ids(*ED.footprint_of(c), r["ho"], r["wo"], device=DEV)
    assert slots == c.slots
    ref_part = EO.slot_partials(y, ids, slots)
    empty = ref_part[0] == 0
    assert int(empty[0, :, 0].sum()) == slots - len(set(ids.tolist()))
    assert bool((got_part[0][empty] == 0).all() and (got_part[1][empty] == 0).all() and (got_part[2][empty] == 0).all())
    report = []
    nbad = EO.partials_mismatch(got_part, ref_part, y, report, blocks=2 if ED.footprint_of(c) == ("halo", 16) else 1)
    # (c) the merges
    m64, r64 = EO.instnorm_stats_fp64(y)
    vmax = y.abs().amax(1)
    merged = _merge_all(r["part"], slots, B, n, r["ld_s"])
    worst_m = worst_r = 0.0
    sbad = 0
    for name, st in merged.items():
        b_, em, er = EO.stats_mismatch(st[..., 0], st[..., 1], m64, r64, vmax)
        sbad += b_
        worst_m, worst_r = max(worst_m, em), max(worst_r, er)
    bm, br = EO.enc_stats_bounds()
    print(f"{line} part_bad={nbad} E_mean={worst_m:.3e} (bound {bm:.3e}) E_rstd={worst_r:.3e} (bound {br:.3e})")
    assert bad == 0, (c.name, worst)
    assert nbad == 0, (c.name, nbad, report)
    assert sbad == 0, (c.name, worst_m, worst_r)
    # the constant channel: its bias and 1 / sqrt(eps) to float32 rounding (a sum of <= 64 equal values: 64 u)
    k = n - 2
    want = ED.CONST_BIAS if r["d"]["b"] is not None else 0.0
    assert bool((y[:, :, k] == float(np.float32(want))).all())
    rs_eps = 1.0 / float(np.float32(EO.STATS_EPS)) ** 0.5
    for st in merged.values():
        assert float((st[:, k, 0].double() - float(np.float32(want))).abs().max()) <= 64 * EO.U * want
        assert float((st[:, k, 1].double() / rs_eps - 1).abs().max()) < 2.0 ** -22


EXTRA = ([(f"e32-8-{p}", v) for p in CF.ENC_PRECS for v in ("nobias", "norelu")]
         + [("g2-16to16-f16x3", "nobias"), ("stem-64-f16x3", "nobias"), ("big-96-f16x3", "nobias"),
            ("e64-64-f16x3", "norelu"), ("e1-32to8-bf16", "nobias")])
MATRIX = [(c.name, "std") for c in CF.ENC_TABLE if c.slots > 0] + EXTRA


@pytest.mark.parametrize("name,variant", MATRIX, ids=[f"{n}-{v}" for n, v in MATRIX])
def test_encoder_conv_on_form(name, variant):
    _check_entry(CF.ENC_BY_NAME[name], variant)


@pytest.mark.parametrize("prec", CF.ENC_PRECS)
def test_small_stem_rejects_stats_part(prec):
    """RAFT-small's 32-output stem runs on the GEMM kernel's gather mode and has no statistics slots (the engine
    takes raft_instnorm_stats for it): raft_conv2d rejects stats_part without launching, and the bare conv holds
    the fp64 bound."""
    c = CF.ENC_BY_NAME[f"stem-32-{prec}"]
    assert _run(c)["rc"] == -1   # RAFT_E_INVALID
    r = _run(c, stats=False)
    bad, worst = EO.conv_mismatch(r["y"], r["ref"], CONV_TOL[prec])
    print(f"ENCERR case={c.name} variant=std out_err/bound={worst:.3e}")
    assert bad == 0, worst


EIGHT = [c.name for c in CF.ENC_TABLE if c.form[0] == CF.HALO and c.form[4] == 8]


@pytest.mark.parametrize("name", EIGHT)
def test_eight_loaders_equal_four(monkeypatch, name):
    """The 8-loader rows at 4 loaders: the same output and the same partials bit for bit.  The encoders' loader
    count has a switch of its own, RAFT_HALO_NL8_ENC=0, read at every launch (raft_conv2d_set_halo_loaders moves
    the update block's convs only: asserted here, the form stays at 8 under it)."""
    from raft_optical_flow_amd import _lib
    lib = _lib.load()
    c = CF.ENC_BY_NAME[name]
    monkeypatch.delenv("RAFT_HALO_NL8_ENC", raising=False)
    a = _run(c)
    assert lib.raft_conv2d_set_halo_loaders(4) == 8
    try:
        assert _lib.conv_form(CF.host_params(c)).astuple() == c.form
    finally:
        lib.raft_conv2d_set_halo_loaders(8)
    monkeypatch.setenv("RAFT_HALO_NL8_ENC", "0")
    b = _run(c, form=c.form[:4] + (4,) + c.form[5:])
    assert torch.equal(_bits(a["ow"]), _bits(b["ow"]))
    assert torch.equal(_bits(a["partw"]), _bits(b["partw"]))


# ----------------------------------------------------------------------------- synthetic merges


def _synthetic(slots, C, cond, seed):
    """Hand-made partials [B = 3][slots][C + 4][4] (float32, CPU): counts 1 .. 32, means around a per-channel base
    in [-5, 5], M2 = count x a variance in (0, 2); the padding columns and every fourth float NaN.  cond:
    "sprinkled" (a third of the slots but slot 0 hold no pixel: (0, 0, 0)), "slot0_only" (only slot 0 holds pixels),
    "slot0_far" (sprinkled, and slot 0 is one pixel 100 within-slot deviations away), "all_equal" (sprinkled, every
    mean equal and every M2 zero)."""
    B = 3
    g = torch.Generator().manual_seed(seed)
    base = torch.linspace(-5, 5, C)[None, None, :]
    cnt = torch.randint(1, 33, (B, slots, C), generator=g).float()
    mean = base + torch.randn(B, slots, C, generator=g)
    m2 = cnt * 2 * torch.rand(B, slots, C, generator=g)
    if cond == "all_equal":
        mean, m2 = base.expand(B, slots, C).clone(), torch.zeros(B, slots, C)
    if cond == "slot0_far":
        cnt[:, 0], mean[:, 0], m2[:, 0] = 1.0, base[:, 0] + 100.0, 0.0
    hole = torch.rand(B, slots, 1, generator=g) < (1.0 if cond == "slot0_only" else 1.0 / 3)
    hole[:, 0] = False
    hole = hole.expand(B, slots, C)
    cnt[hole], mean[hole], m2[hole] = 0.0, 0.0, 0.0
    part = torch.full((B, slots, C + 4, 4), NAN)
    part[:, :, :C, 0], part[:, :, :C, 1], part[:, :, :C, 2] = cnt, mean, m2
    return part, (cnt, mean, m2)


@pytest.mark.parametrize("C", [8, 64, 96, 300])
@pytest.mark.parametrize("slots", [1, 2, 63, 64, 65, 128, 129, 2049])
def test_synthetic_merges(slots, C):
    """The three merges on hand-made (count, mean, M2) partials (B = 3, stats_ld = C + 4 with NaN padding, slot
    counts around the 64-slot level-1 group and the 8 x 16-group level-2 stride, C below, at and off the 64-channel
    group), against the pooled statistics by definition in fp64 (elementwise_oracle.pooled_stats).

    Bound, from fp64 rounding of the documented sums (eps64 = 2^-53, S = slots, K = slot 0's mean, d_i = m_i - K):
      mean:  u |mean| for the float32 result + (S + 8) eps64 (max |d_i| + |K|) for S additions of terms <= c_i |d_i|
             over n, and K + s1 / n (Chan's running mean moves by at most max |d_i| per step: the same bound);
      var:   4 (S + 8) eps64 s2 / n, s2 = sum M2_i + c_i d_i^2 >= s1^2 / n (Cauchy-Schwarz): S additions of
             non-negative terms, twice (s2 and s1, whose relative error doubles in s1^2), and the difference;
             Chan's M2 is a sum of non-negative terms below s2;
      rstd:  u for the float32 result + half the relative error of var + eps.
    Each merge is within the bound of the reference, any two within twice the bound of each other, and _merge_ws
    equals _merge_fused bit for bit.  Slot 0 always holds pixels (the merges' documented precondition)."""
    B, eps64 = 3, 2.0 ** -53
    eps = float(np.float32(EO.STATS_EPS))
    for i, cond in enumerate(("sprinkled", "slot0_only", "slot0_far", "all_equal")):
        part, (cnt, mean, m2) = _synthetic(slots, C, cond, 1000 * slots + 10 * C + i)
        assert bool((cnt[:, 0] > 0).all())
        n, mu, q = EO.pooled_stats(cnt, mean, m2)
        var = q / n
        rstd = 1.0 / torch.sqrt(var + eps)
        d = (mean.double() - mean[:, :1].double()) * (cnt > 0)
        s2 = (m2.double() + cnt.double() * d * d).sum(1)
        b_mean = EO.U * (1 + 1e-6) * mu.abs() + (slots + 8) * eps64 * (d.abs().amax(1) + mean[:, 0].double().abs())
        b_rstd = EO.U * (1 + 1e-6) + 0.5 * 4 * (slots + 8) * eps64 * (s2 / n) / (var + eps)
        got = _merge_all(part.to(DEV), slots, B, C, C + 4)
        st = {k: v.cpu().double() for k, v in got.items()}
        for name, v in st.items():
            em = ((v[..., 0] - mu).abs() / b_mean).max()
            er = (((v[..., 1] - rstd) / rstd).abs() / b_rstd).max()
            assert float(em) <= 1.0 and float(er) <= 1.0, (cond, name, float(em), float(er))
        for a, b in (("merge", "ws"), ("merge", "fused")):
            assert bool(((st[a][..., 0] - st[b][..., 0]).abs() <= 2 * b_mean).all()), (cond, a, b)
            assert bool((((st[a][..., 1] - st[b][..., 1]) / rstd).abs() <= 2 * b_rstd).all()), (cond, a, b)
