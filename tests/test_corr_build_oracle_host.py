"""Host checks of tests/corr_build_oracle.py, the reference the GPU tests of the correlation builds
(tests/test_gpu_corr_build_forms.py) compare with: it agrees with the project's oracles, its tiler is the
header's formula, the case tables have the properties the GPU cases rely on, the comparison at the GPU
tests' bound rejects seven wrong builds, and the magnitude figures of the unscaled f16 split that
include/raft_hip.h and DESIGN.md 7.4 quote."""
import numpy as np
import pytest
import torch

import corr_build_oracle as CB
from lookup_oracle import level_dims

U = CB.U24


def _nchw(rows, B, H, W):
    return np.ascontiguousarray(rows.reshape(B, H, W, -1).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (2, 5, 7, 12), (1, 33, 37, 8), (3, 9, 11, 36)])
def test_reference_is_the_oracles_pyramid(B, H, W, C):
    """reference == oracle.raft_oracle.corr_pyramid in fp64 and oracle.torch_cpu.corr_pyramid to float32
    rounding (elementwise against mag), odd sizes, every L in 1..6 the shape allows."""
    from oracle import raft_oracle as O
    from oracle import torch_cpu as T
    f1, f2 = CB.features(B, H, W, C, seed=H * W + C)
    for L in range(1, 7):
        if min(H, W) >> (L - 1) < 1:
            continue
        ref, mag = CB.reference(f1, f2, L, np.sqrt(np.float64(C)), B, H, W)
        assert [x.shape[1:] for x in ref] == level_dims(H, W, L)
        want = O.corr_pyramid(_nchw(f1, B, H, W).astype(np.float64), _nchw(f2, B, H, W).astype(np.float64), L)
        got32 = T.corr_pyramid(torch.from_numpy(_nchw(f1, B, H, W)), torch.from_numpy(_nchw(f2, B, H, W)), L)
        for l in range(L):
            assert np.abs(ref[l] - want[l].reshape(ref[l].shape)).max() <= 1e-12 * max(1.0, np.abs(ref[l]).max())
            assert (mag[l] >= np.abs(ref[l]) * (1 - 1e-12)).all()
            err = np.abs(got32[l].numpy().reshape(ref[l].shape).astype(np.float64) - ref[l])
            assert (err <= (C + 4) * U * mag[l]).all()   # a float32 dot product of C terms, division, pools


def test_restatements_follow_the_reference():
    """The float32 restatements stay within sqrt(C) x 2^-24 mag of fp64 at unit scale (C roundings of
    partial sums of random sign, each at most 2^-24 mag: a random walk)."""
    for C in (64, 256):
        B, H, W, L = 2, 9, 17, 3
        f1, f2 = CB.features(B, H, W, C, seed=C)
        ref, mag = CB.reference(f1, f2, L, CB.sqrt_c32(C), B, H, W)
        for prec in (CB.FP32, CB.F16X3):
            r = CB.measure(CB.restate(f1, f2, L, CB.sqrt_c32(C), prec, B, H, W), ref, mag)
            assert 0 < r < np.sqrt(C) * U, (C, prec, r / U)


@pytest.mark.parametrize("B,H,W,L", [(1, 1, 1, 1), (2, 3, 5, 2), (1, 9, 17, 4), (2, 8, 16, 4), (1, 33, 49, 6)])
def test_tile_is_the_headers_formula_and_round_trips(B, H, W, L):
    """tile places element (y, x) of query p at off_l + p * S_l + ((y>>2) TW_l + (x>>2)) 16 + (y&3) 4 + (x&3)
    (include/raft_hip.h), every other float is 0, untile inverts it bit for bit, valid_mask marks exactly
    the placed elements."""
    rng = np.random.default_rng(B * H + W)
    levels = [rng.standard_normal((B * H * W, h, w)) + 3.0 for h, w in level_dims(H, W, L)]   # fp64, never 0
    raw = CB.tile(levels, B, H, W)
    assert raw.dtype == np.float64 and raw.size == CB.pyramid_floats(B, H, W, L)
    want = np.zeros_like(raw)
    off = 0
    for lv in levels:
        n, h, w = lv.shape
        th, tw = -(-h // 4), -(-w // 4)
        S = th * tw * 16
        p, y, x = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing="ij")
        want[off + p * S + ((y >> 2) * tw + (x >> 2)) * 16 + (y & 3) * 4 + (x & 3)] = lv
        off += n * S
    assert np.abs(raw - want).max() <= 2.0 ** -45 * 8 and np.array_equal(raw == 0, want == 0)
    mask = CB.valid_mask(B, H, W, L)
    assert np.array_equal(mask, want != 0) and (raw[~mask] == 0).all()
    back = CB.untile(raw.astype(np.float32), B, H, W, L)
    for b, lv in zip(back, levels):
        assert np.array_equal(b, lv.astype(np.float32))
    assert all(CB.pool_exact(CB.restate(*CB.features(B, H, W, 8, 1), L, 2.0, CB.FP32, B, H, W)))


def test_units_restates_the_launch():
    assert CB.units(1, 55, 128, 8) == 896           # config 2's map: 28 query tiles x 32 target tiles
    assert CB.units(3, 9, 70, 8) == 45 and CB.units(2, 37, 53, 8) == 192 and CB.units(2, 37, 53, 4) == 384
    assert CB.units(1, 33, 49, 8) == 84 and CB.units(1, 33, 49, 4) == 156
    assert CB.units(1, 16, 16, 8) == 1 and CB.units(1, 16, 17, 8) == 4 and CB.units(1, 17, 16, 4) == 6


def test_geometry_table_properties():
    """What the tile-geometry cases are there for, asserted: the residues of H and W against the 8 x 8,
    8 x 16 and 16 x 16 target blocks, of P against the 64, 128 and 256 query tiles, single pixels, ragged
    and 1-px levels, pools that drop a row or column, every level count up to 5."""
    G = CB.GEOMETRY
    assert len(set(G)) == 13 and CB.GEOMETRY_SQRT3 in G
    P = {g: g[1] * g[2] for g in G}
    # query tiles: fewer than one tile, exactly 256, one short of it, one past it, multiples and non-multiples
    assert P[(1, 1, 1, 1)] == 1 and P[(1, 15, 17, 3)] == 255 and P[(1, 16, 16, 5)] == 256
    assert P[(1, 1, 257, 1)] == 257 and P[(1, 257, 1, 1)] == 257
    assert P[(1, 8, 16, 4)] == 128 and P[(1, 8, 16, 4)] % 64 == 0
    assert P[(2, 7, 9, 2)] == 63 and P[(1, 3, 5, 1)] < 64
    for m in (64, 128, 256):
        assert any(p % m == 0 for p in P.values()) and any(p % m not in (0, 1) and p > m for p in P.values()), m
    # target blocks: aligned to 8 / 16, one past, one short, odd
    for m in (8, 16):
        for a in (1, 2):
            res = {g[a] % m for g in G}
            assert {0, 1, m - 1} <= res, (m, a, res)
    assert any(g[1] > 16 and g[2] > 16 for g in G)                 # more than one 16 x 16 block both ways
    assert any(g[1] == 1 and g[2] > 256 for g in G) and any(g[2] == 1 and g[1] > 256 for g in G)
    assert any(g[0] > 1 for g in G) and any(g[0] == 3 for g in G)
    assert {g[3] for g in G} == {1, 2, 3, 4, 5}
    dims = {g: level_dims(g[1], g[2], g[3]) for g in G}
    assert dims[(1, 16, 16, 5)][-1] == (1, 1) and dims[(1, 8, 16, 4)][-1] == (1, 2) and dims[(1, 17, 33, 5)][-1] == (1, 2)
    assert dims[(1, 2, 2, 2)] == [(2, 2), (1, 1)]
    assert all(min(h, w) >= 1 for d in dims.values() for h, w in d)
    ragged = {g: [l for l, (h, w) in enumerate(d) if h % 4 or w % 4] for g, d in dims.items()}
    assert ragged[(1, 8, 16, 4)] == [2, 3] and ragged[(1, 16, 16, 5)] == [3, 4]     # aligned levels 0 and 1
    assert ragged[(3, 23, 37, 4)] == [0, 1, 2, 3] and ragged[(1, 9, 17, 4)] == [0, 2, 3]
    drops = {g: [l for l, (h, w) in enumerate(d[:-1]) if h % 2 or w % 2] for g, d in dims.items()}
    assert drops[(1, 9, 17, 4)] == [0] and drops[(2, 15, 31, 4)] == [0, 1, 2] and drops[(1, 8, 16, 4)] == []
    # a level-1 / level-2 tile row the level above only half fills (H = 9: level-0 tile rows 0..2, level 1 has 4 rows)
    assert dims[(1, 9, 17, 4)][1] == (4, 8) and dims[(1, 17, 33, 5)][2] == (4, 8)
    # every case: one unit or several, all below the work-group counts (a work-group takes one unit)
    un = {g: CB.units(g[0], g[1], g[2], 8) for g in G}
    assert un[(1, 16, 16, 5)] == 1 and un[(1, 1, 257, 1)] == 34 and un[(3, 23, 37, 4)] == 72
    assert max(un.values()) < 256 and max(CB.units(g[0], g[1], g[2], 4) for g in G) < 512


def test_channel_table_properties():
    """K tails of the 32-channel step (fp32, prec), half-step counts of the workspace build and the three
    ways out of it (C < 64, C % 16, C > 1024)."""
    B, H, W, L = CB.CHANNEL_SHAPE
    assert B == 2 and H % 8 == 1 and W % 16 == 1 and L == 3 and level_dims(H, W, L) == [(9, 17), (4, 8), (2, 4)]
    for key in ("fp32", "prec"):
        cs = CB.CHANNELS[key]
        assert all(c % 4 == 0 for c in cs)
        assert any(c < 32 for c in cs) and any(c % 32 == 0 for c in cs) and any(c > 32 and c % 32 for c in cs)
        assert any(c % 32 % 16 in (4, 8) for c in cs) and 256 in cs
    assert 40 in CB.CHANNELS["prec"] and 36 in CB.CHANNELS["fp32"] and 24 in CB.CHANNELS["prec"]
    ws = CB.CHANNELS["ws"]
    assert all(c % 16 == 0 and 64 <= c <= 1024 for c in ws) and min(ws) == 64 and max(ws) == 1024
    assert {c // 16 for c in ws} == {4, 5, 6, 8, 16, 64}       # odd and even half-step counts, 3 stages ahead
    fb = CB.WS_FALLBACK_C
    assert any(c < 64 and c % 16 == 0 for c in fb) and any(c % 16 and c > 64 for c in fb)
    assert any(c > 1024 and c % 16 == 0 for c in fb) and all(c % 4 == 0 for c in fb)


@pytest.mark.parametrize("cus", [256, 304, 120, 64])
def test_pipeline_table_properties(cus):
    """The persistent-pipeline cases: 84 / 156 units per image; the batch sizes give more units than
    work-groups, not a multiple of them, and at least 3 units on a work-group, on any CU count; on 256 CUs
    they are the issue's B = 4 (336 of 256, 624 of 512) and B = 7 (588 of 256, 1092 of 512)."""
    H, W = CB.PIPELINE_HW
    assert CB.units(1, H, W, 8) == 84 and CB.units(1, H, W, 4) == 156
    assert H % 16 == 1 and W % 16 == 1 and (H * W) % 128 not in (0, 1)
    assert level_dims(H, W, 6)[-1] == (1, 1) and CB.PIPELINE_L == [1, 2, 3, 6] and CB.PIPELINE_C // 16 == 4
    for nw in (8, 4):
        wgs = cus if nw == 8 else 2 * cus
        multi, three = CB.pipeline_batches(cus, nw)
        um, u3 = CB.units(multi, H, W, nw), CB.units(three, H, W, nw)
        assert um > wgs and um % wgs and u3 >= 2 * wgs + 1 and u3 % wgs and -(-u3 // wgs) >= 3
    if cus == 256:
        assert CB.pipeline_batches(256, 8) == (4, 7) and CB.pipeline_batches(256, 4) == (4, 7)
        assert [CB.units(b, H, W, nw) for b, nw in ((4, 8), (4, 4), (7, 8), (7, 4))] == [336, 624, 588, 1092]


def test_other_table_properties():
    B, H, W, L = CB.SWEEP_SHAPE
    assert (B, L) == (1, 2) and H % 2 and W % 2 and CB.SWEEP_K == [12, 8, 4, 0, -2, -3, -4, -6, -8, -12]
    for (b, h, w, l) in CB.SWITCH_CASES:
        assert h % 16 and w % 16 and h % 8 and w % 8 and l == 4 and (h * w) % 128
        assert CB.units(b, h, w, 8) > 1
    B, H, W, L = CB.POISON_SHAPE
    assert B == 2 and CB.POISON_IMAGE == 1 and H % 2 == 1
    assert CB.target_cells(CB.POISON_INSIDE, H, W, L) == [(3, 6), (1, 3), (0, 1)]
    assert CB.target_cells(CB.POISON_DROPPED, H, W, L) == [(8, 5), None, None]
    assert CB.target_cells(0, 9, 17, 3) == [(0, 0), (0, 0), (0, 0)]
    assert CB.target_cells(16, 9, 17, 3) == [(0, 16), None, None]


# ------------------------------------------------------------------------------------ mutations


def _mutation_case(C):
    B, H, W, L = CB.CHANNEL_SHAPE
    f1, f2 = CB.features(B, H, W, C, seed=100 + C)
    sc = CB.sqrt_c32(C)
    ref, mag = CB.reference(f1, f2, L, sc, B, H, W)
    return (B, H, W, L), f1, f2, sc, CB.tile(ref, B, H, W), CB.tile(mag, B, H, W), ref, mag


@pytest.mark.parametrize("mutation,prec", [(m, p) for m in sorted(CB.MUTATIONS) for p in (CB.F16X3, CB.FP32)
                                           if (m, p) != ("a", CB.FP32)])   # the fp32 product has no lo*hi term
def test_comparison_rejects_wrong_builds(mutation, prec):
    """Each mutation of the restatement breaks the bound the GPU tests use, k = max(4 r, 2 x 2^-24) with r the
    unmutated restatement's largest err / mag on the same case, in at least one element; the unmutated
    restatement passes.  (2, 9, 17, 3): two images, odd sizes, C = 64 (C = 40 for the K tail)."""
    C = 40 if mutation == "b" else 64
    (B, H, W, L), f1, f2, sc, tref, tmag, ref, mag = _mutation_case(C)
    good = CB.restate(f1, f2, L, sc, prec, B, H, W)
    k = CB.bound_k(CB.measure(good, ref, mag))
    assert k < 4 * np.sqrt(C) * U
    bad, _ = CB.compare(CB.tile(good, B, H, W), tref, tmag, k)
    assert not bad.any()
    wrong = CB.restate(f1, f2, L, sc, prec, B, H, W, mutation=mutation)
    bad, worst = CB.compare(CB.tile(wrong, B, H, W), tref, tmag, k)
    print(f"mutation {mutation} ({CB.MUTATIONS[mutation]}), {prec}: {int(bad.sum())} of {bad.size} elements fail, "
          f"worst {worst / U:.3g} x 2^-24 mag against k = {k / U:.3g}")
    assert bad.any()
    if mutation == "g":
        lv = CB.untile(bad, B, H, W, L)
        assert not lv[0].any() and lv[1].any() and lv[2].any()


def test_comparison_rejects_nonzero_padding_and_nan():
    (B, H, W, L), f1, f2, sc, tref, tmag, ref, mag = _mutation_case(64)
    good = CB.tile(CB.restate(f1, f2, L, sc, CB.F16X3, B, H, W), B, H, W)
    pad = np.flatnonzero(~CB.valid_mask(B, H, W, L))
    for v in (1e-30, np.nan, -0.0):
        x = good.copy()
        x[pad[7]] = v
        bad, _ = CB.compare(x, tref, tmag, 8 * U)
        assert bad.sum() == (0 if v == 0 else 1)
    x = good.copy()
    x[np.flatnonzero(CB.valid_mask(B, H, W, L))[11]] = np.nan
    bad, worst = CB.compare(x, tref, tmag, 8 * U)
    assert bad.sum() == 1 and worst == float("inf")
    assert "level 0 query 0" in CB.describe_bad(bad, x, tref, tmag, B, H, W, L)


# ------------------------------------------------------------------------------------ the magnitude sweep


def _sweep(C, shape, prec):
    B, H, W, L = shape
    out = {}
    for k in CB.SWEEP_K:
        f1, f2 = CB.features(B, H, W, C, seed=7, scale=2.0 ** k)
        sc = CB.sqrt_c32(C)
        ref, mag = CB.reference(f1, f2, L, sc, B, H, W)
        out[k] = CB.measure(CB.restate(f1, f2, L, sc, prec, B, H, W), ref, mag) / U
    return out


@pytest.mark.parametrize("C", [64, 256])
def test_magnitude_sweep_of_the_split(C):
    """The restatement's largest err / mag for N(0, s^2) features, s = 2^k: the figures include/raft_hip.h and
    DESIGN.md 7.4 quote (printed).  While lo = f16(x - hi) is a normal f16 (s >= 2^-3 or so) the error is a
    fraction of 2^-24 mag whatever s; below, lo lies in the f16 subnormals (step 2^-24): each operand carries
    an absolute error of up to 2^-25, a product one of ~2^-25 s, against a product size of s^2, so err / mag
    grows as 1 / s: x16 per four octaves (asserted within a factor 2)."""
    f16 = _sweep(C, CB.SWEEP_SHAPE, CB.F16X3)
    f32 = _sweep(C, CB.SWEEP_SHAPE, CB.FP32)
    print(f"C = {C}, {CB.SWEEP_SHAPE}: largest err / (2^-24 mag) of the restatement")
    for k in CB.SWEEP_K:
        print(f"  s = 2^{k:<4d} f16x3 {f16[k]:9.3f}   fp32 {f32[k]:6.3f}")
    # the figures quoted in include/raft_hip.h and DESIGN.md 7.4 (a BLAS with another summation order may move
    # the unit-scale figures a little: held within a factor 1.5)
    quoted = {64: {0: 2.24, -3: 3.45, -4: 6.37, -6: 25.3, -8: 107.8, -12: 1378.0},
              256: {0: 1.32, -3: 1.74, -4: 2.76, -6: 11.0, -8: 44.6, -12: 732.0}}[C]
    for k, v in quoted.items():
        assert v / 1.5 <= f16[k] <= v * 1.5, (k, f16[k], v)
    assert {64: 4.29, 256: 3.66}[C] / 1.5 <= f32[0] <= {64: 4.29, 256: 3.66}[C] * 1.5
    for k in (12, 8, 4, 0):
        assert f16[k] < np.sqrt(C) / 2 and abs(f16[k] / f16[0] - 1) < 0.01, (k, f16[k])
    assert f16[-2] < 2 * f16[0] and f16[-3] < 2 * f16[0]
    for k in (-4, -8):
        assert 8 <= f16[k - 4] / f16[k] <= 32, (k, f16[k - 4], f16[k])
    assert f16[-4] > 1.5 * f16[0] and f16[-6] > 2 * f16[-4] and f16[-12] > 100
    assert max(f32.values()) < np.sqrt(C) and max(f32.values()) / min(f32.values()) < 1.5   # fp32: the same at every s


def test_split_out_of_range():
    """|x| >= 65520 rounds to hi = inf, lo = x - inf = -inf: every element that involves it is NaN in the
    restatement (inf - inf, or inf x 0); 65504, the largest f16, and anything that rounds to it, splits fine."""
    hi, lo = CB.split16(np.array([65504.0, 65519.0, 65520.0, 1e5, -1e5], np.float32))
    assert hi[0] == 65504 and lo[0] == 0 and hi[1] == 65504 and lo[1] == 15
    assert np.isinf(hi[2:]).all() and np.isinf(lo[2:]).all() and (np.sign(hi[2:]) == -np.sign(lo[2:])).all()
    B, H, W, L = 1, 3, 5, 2
    f1, f2 = CB.features(B, H, W, 16, seed=3)
    f1[4, 2] = 1e5
    lv = CB.restate(f1, f2, L, 4.0, CB.F16X3, B, H, W)
    assert np.isnan(lv[0][4]).all() and np.isnan(lv[1][4]).all()
    assert np.isfinite(np.delete(lv[0], 4, axis=0)).all() and np.isfinite(np.delete(lv[1], 4, axis=0)).all()
    assert np.isfinite(CB.restate(f1, f2, L, 4.0, CB.FP32, B, H, W)[0]).all()
