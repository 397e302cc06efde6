"""Host side of the encoder InstanceNorm conv tests (no device): conv_forms.ENC_TABLE pinned through the library's
host queries, the float32 restatement of the documented statistics algorithm held to fp64 (its measured error
sets the GPU bounds: elementwise_oracle.ENC_STATS_MEASURED), and the GPU tests' comparisons shown to
reject wrong references."""
import ctypes

import pytest
import torch

import conv_forms as CF
import elementwise_oracle as EO
import encoder_norm_data as ED
from raft_optical_flow_amd import _lib
from test_gpu_parity import CONV_TOL

SHAPES = sorted({c.name.rsplit("-", 1)[0] for c in CF.ENC_TABLE if c.slots > 0})


def _entry(shape):
    return CF.ENC_BY_NAME[shape + "-f16x3"]


def test_enc_table_host_side():
    """raft_conv2d_form with the features set (halo_pick depends on them), raft_conv2d_stats_slots and
    raft_conv2d_in_norm_ok of every ENC_TABLE entry, on 256 CUs; the slot count agrees with the documented
    footprints (elementwise_oracle.stats_slot_ids); the table reaches every form the encoders' convs take."""
    lib = _lib.load()
    assert (lib.raft_conv2d_set_halo_ks(0), lib.raft_conv2d_set_halo_loaders(0)) == (2, 8)
    for c in CF.ENC_TABLE:
        p = CF.host_params(c)
        bare = CF.host_params(c, features=False)
        assert bool(p.stats_part) == (c.stats and c.slots > 0) and bool(p.in_norm) == c.in_norm
        f = _lib.conv_form(p).astuple()
        assert f == c.form, (c.name, f, c.form)
        for q in (p, bare):
            assert lib.raft_conv2d_stats_slots(ctypes.byref(q)) == c.slots, c.name
            assert lib.raft_conv2d_in_norm_ok(ctypes.byref(q)) == c.in_norm_ok, c.name
        assert lib.raft_conv2d_halo_tile_rows(ctypes.byref(p)) == (f[1] if f[0] == CF.HALO else 0)
        ho, wo = CF.out_hw(c)
        if c.slots:
            ids, slots = EO.stats_slot_ids(*ED.footprint_of(c), ho, wo)
            assert slots == c.slots and int(ids.max()) < slots and int(ids[0]) == 0, c.name
        if c.in_norm:
            assert c.in_norm_ok == 1
    # RAFT-small's stem: no slots, and the launch's argument check rejects stats_part (and leaves the form alone)
    small = CF.host_params(CF.ENC_BY_NAME["stem-32-f16x3"])
    small.stats_part, small.stats_ld = 1 << 20, 36
    f = _lib.ConvForm(kernel=-5)
    assert lib.raft_conv2d_form(ctypes.byref(small), ctypes.byref(f)) == -1 and f.kernel == -5
    # just past the in0_c <= 256 edge the launch rejects in_norm
    wide = CF.host_params(CF.ENC_BY_NAME["e32-288to64-f16x3"])
    wide.in_norm, wide.in_norm_relu = 1 << 20, 1
    assert lib.raft_conv2d_form(ctypes.byref(wide), ctypes.byref(f)) == -1
    # the forms the table must reach
    forms = {c.form for c in CF.ENC_TABLE if c.slots > 0}
    halo = {(f[1], f[2]) for f in forms if f[0] == CF.HALO}
    assert halo == {(8, 32), (8, 64), (16, 64)}
    assert {f[4] for f in forms if f[0] == CF.HALO} == {4, 8}
    assert {c.form[3] for c in CF.ENC_TABLE if c.form[0] == CF.HALO and c.kh == 1} == {1, 2, 3}
    assert {f[6] for f in forms if f[0] == CF.GEMM} == {1, 2} and any(f[0] == CF.STEM for f in forms)
    # the 3 x 5 image on 8-row tiles: 4 slots of which 2 hold no pixel
    ids, slots = EO.stats_slot_ids("halo", 8, 3, 5)
    assert slots == 4 and sorted(set(ids.tolist())) == [0, 1]


def test_statistics_definitions_agree():
    """The oracle's own pieces: fp64 slot partials pooled by definition, and merged by Chan's formula, are the
    plain fp64 statistics of the data (1e-12), on ragged halo, 16-row and GEMM footprints with empty slots."""
    g = torch.Generator().manual_seed(5)
    for kind, th, ho, wo in (("halo", 8, 19, 27), ("halo", 16, 21, 33), ("gemm", 0, 10, 14), ("stem", 8, 3, 5)):
        y = torch.randn(2, ho * wo, 5, generator=g, dtype=torch.float64) * 3 + 7
        ids, slots = EO.stats_slot_ids(kind, th, ho, wo)
        part = EO.slot_partials(y, ids, slots)
        assert float(part[0][0, :, 0].sum()) == ho * wo
        m64, r64 = EO.instnorm_stats_fp64(y)
        for merge in (EO.pooled_stats, EO.chan_merge):
            m, r = EO.mean_rstd(*merge(*part))
            assert float((m - m64).abs().max()) < 1e-12 and float((r / r64 - 1).abs().max()) < 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_restated_statistics_against_fp64(shape):
    """The documented algorithm in float32 (per slot an fp32 sum, the mean, M2 about that mean; Chan's merge in
    fp64; float32 results) against fp64, on the float32 rounding of every table shape's fp64 output and every data
    condition (encoder_norm_data): E_mean relative to the channel's max |v| in its image, E_rstd relative.  The
    largest values over all shapes are ENC_STATS_MEASURED; the GPU bound is 4 x that (the kernel sums a wave's 32
    values in another order), and the restatement itself must sit inside the bound with that margin."""
    c = _entry(shape)
    variants = ["std", "nobias"] + (["norelu"] if c.in_norm else [])
    ids, slots = EO.stats_slot_ids(*ED.footprint_of(c), *CF.out_hw(c))
    for variant in variants:
        d = ED.case_data(ED.key_of(c), variant)
        y32 = ED.rows_of(d["ref"]).float()
        mean, rstd = EO.instnorm_stats_restated(y32, ids, slots)
        em, er = EO.stats_errors(mean, rstd, y32)
        print(f"RESTATED shape={shape} variant={variant} E_mean={float(em.max()):.3e} E_rstd={float(er.max()):.3e}")
        assert float(em.max()) <= EO.ENC_STATS_MEASURED["mean"] and float(er.max()) <= EO.ENC_STATS_MEASURED["rstd"]
        bad, _, _ = EO.stats_mismatch(mean, rstd, *EO.instnorm_stats_fp64(y32), y32.abs().amax(1))
        assert bad == 0
        # the constant channel: its bias and 1 / sqrt(eps) to float32 rounding
        k = c.n - 2
        want = ED.CONST_BIAS if d["b"] is not None else 0.0
        assert float((mean[:, k].double() - float(torch.tensor(want).float())).abs().max()) <= 32 * EO.U * want
        assert float((rstd[:, k].double() * float(torch.tensor(EO.STATS_EPS).float()) ** 0.5 - 1).abs().max()) < 2 ** -22
        # the float32 partials pass the slot comparison against the fp64 ones
        assert EO.partials_mismatch(EO.slot_partials(y32, ids, slots, torch.float32), EO.slot_partials(y32, ids, slots),
                                    y32) == 0


@pytest.mark.parametrize("shape", ["big-96", "big-128"])
def test_two_block_slots_against_fp64(shape):
    """The 16-row tiles' slots as the header documents them (two 32-pixel blocks, float32 partials each, combined
    by Chan's formula in float32) sit inside partials_mismatch's two-block bound.  (The one-block bound lacks the
    first-order term of d^2's error and is missed at big-96 by the 30-deviation channel on an 8-pixel ragged
    slot, by 7.5e-6 of M2: measured here and on the GPU.)"""
    c = _entry(shape)
    ho, wo = CF.out_hw(c)
    ids, slots = EO.stats_slot_ids("halo", 16, ho, wo)
    y32 = ED.rows_of(ED.case_data(ED.key_of(c))["ref"]).float()
    block = 2 * ids + ((torch.arange(ho * wo) // wo) % 4) // 2      # rows 4w, 4w + 1 | 4w + 2, 4w + 3 of wave w
    cnt, mean, m2 = EO.slot_partials(y32, block, 2 * slots, torch.float32)
    (a0, a1, a2), (b0, b1, b2) = [[t[:, k::2] for t in (cnt, mean, m2)] for k in (0, 1)]
    n = a0 + b0
    d = b1 - a1
    both = (a0 > 0) & (b0 > 0)
    f = n.clamp_min(1)
    got = (n, torch.where(both, a1 + d * (b0 / f), torch.where(a0 > 0, a1, b1)),
           torch.where(both, a2 + b2 + d * d * (a0 * b0 / f), torch.where(a0 > 0, a2, b2)))
    ref = EO.slot_partials(y32, ids, slots)
    assert EO.partials_mismatch(got, ref, y32, blocks=2) == 0
    if shape == "big-96":
        assert EO.partials_mismatch(got, ref, y32) > 0


@pytest.mark.parametrize("shape", ["e32-8", "big-96", "g2-16to16", "stem-64"])
def test_statistics_comparisons_reject_mutated_references(shape):
    """A stand-in for a correct kernel (the fp64 output rounded to float32, its float32 partials, the restated
    merge) passes the slot-by-slot and the merged comparisons, and each of these references fails them: one
    slot's pixels dropped; one out-of-image pixel of a ragged tile counted (its value: the bias, a conv of
    padding); image b's statistics read for image b + 1."""
    c = _entry(shape)
    d = ED.case_data(ED.key_of(c))
    ho, wo = CF.out_hw(c)
    ids, slots = EO.stats_slot_ids(*ED.footprint_of(c), ho, wo)
    y32 = ED.rows_of(d["ref"]).float()
    vmax = y32.abs().amax(1)
    got_part = EO.slot_partials(y32, ids, slots, torch.float32)
    got = EO.instnorm_stats_restated(y32, ids, slots)
    ref_part = EO.slot_partials(y32, ids, slots)
    assert EO.partials_mismatch(got_part, ref_part, y32) == 0
    assert EO.stats_mismatch(*got, *EO.mean_rstd(*EO.pooled_stats(*ref_part)), vmax)[0] == 0
    # (1) the pixels of one slot dropped: the slot is empty in the reference
    s = int(ids[len(ids) // 2])
    keep = ids != s
    ids1 = ids[keep]
    drop = EO.slot_partials(y32[:, keep], ids1, slots)
    assert int(drop[0][0, s, 0]) == 0
    assert EO.partials_mismatch(got_part, drop, y32) >= c.n
    assert EO.stats_mismatch(*got, *EO.mean_rstd(*EO.pooled_stats(*drop)), vmax)[0] > 0.5 * c.B * c.n
    # (2) one pixel outside the image counted in the last (ragged) slot that holds pixels
    last = int(ids.max())
    extra = torch.zeros(c.B, 1, c.n) + d["b"][None, None, :]
    more = EO.slot_partials(torch.cat([y32, extra], 1), torch.cat([ids, torch.tensor([last])]), slots)
    assert EO.partials_mismatch(got_part, more, y32) >= c.n
    assert EO.stats_mismatch(*got, *EO.mean_rstd(*EO.pooled_stats(*more)), vmax)[0] > 0.5 * c.B * c.n
    # (3) the other image's statistics
    assert c.B >= 2
    rolled = [torch.roll(t, 1, 0) for t in ref_part]
    assert EO.partials_mismatch(got_part, rolled, y32) > 0.5 * c.B * c.n * len(set(ids.tolist()))
    assert EO.stats_mismatch(*got, *[torch.roll(t, 1, 0) for t in EO.instnorm_stats_fp64(y32)], vmax)[0] > 0.5 * c.B * c.n


@pytest.mark.parametrize("prec", CF.ENC_PRECS)
@pytest.mark.parametrize("shape", ["e32-8", "e32-24"])
def test_in_norm_comparison_rejects_mutated_references(shape, prec):
    """The output comparison (per image, CONV_TOL[prec] x max(1, max |ref|)) at each precision's bound: the
    reference rounded to float32 passes; a reference without the relu, with the zero padding normalised like a
    pixel, or with the previous image's {mean, rstd}, fails."""
    c = _entry(shape)
    d = ED.case_data(ED.key_of(c))
    got = d["ref"].float()
    assert EO.conv_mismatch(got, d["ref"], CONV_TOL[prec])[0] == 0
    for mutate in ("no_relu", "pad_normalised", "next_image"):
        bad = EO.enc_conv_ref(d["x"], d["w"], d["b"], c.stride, d["pad"], d["in_stats"], d["relu"], mutate)
        assert EO.conv_mismatch(got, bad, CONV_TOL[prec])[0] == c.B, (mutate, prec)
