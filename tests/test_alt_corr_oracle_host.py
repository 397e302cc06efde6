"""tests/alt_corr_oracle.py against the project's oracles, its builders' promises, the comparison's
power to reject wrong references at every bound in use, and the measurement of those bounds (host
only: no GPU, no library)."""
import numpy as np
import pytest
import torch

import alt_corr_oracle as A
from conftest import load_golden
from oracle import raft_oracle as O
from oracle import torch_cpu as T

BOUNDS = [A.bound32(), A.bound_bwd()] + [A.bound16x3(s) for s in A.GAMMA16X3]


def _case(seed=1, B=2, N=2, H1=9, W1=11, H2=7, W2=10, C=32):
    """Ordinary coordinates: x - floor(x) is exact in fp32 (no coordinate inside (-1, 0), where the
    kernels' fp32 fraction rounds), so alt_ref and the fp64 oracles compute the same weights."""
    f1, f2 = A.maps(seed, B, H1, W1, H2, W2, C)
    c = A.smooth_coords(seed + 1, B, N, H1, W1, H2, W2, 2.0)
    c[(c > -1) & (c < 0)] -= np.float32(1.0)
    assert np.array_equal((c - np.floor(c)).astype(np.float64), c.astype(np.float64) - np.floor(c))
    return f1, f2, c


@pytest.mark.parametrize("r", [0, 2, 4])
def test_alt_ref_equals_the_oracles(r):
    f1, f2, c = _case()
    ref, mag = A.alt_ref(f1, f2, c, r)
    d = [x.astype(np.float64) for x in (f1, f2, c)]
    assert np.abs(ref - O.alt_corr_forward(*d, r)).max() < 1e-12
    got = T.alt_corr_forward(*(torch.tensor(x) for x in d), r).numpy()
    assert np.abs(ref - got).max() < 1e-12
    assert np.all(mag >= np.abs(ref) - 1e-12)
    # coord_div and scale_div: the position is coords / coord_div in fp32
    ref2, _ = A.alt_ref(f1, f2, c, r, coord_div=2.0, scale_div=8.0)
    assert np.abs(ref2 * 8.0 - O.alt_corr_forward(d[0], d[1], (c / np.float32(2)).astype(np.float64), r)).max() < 1e-12


def test_alt_ref_levels_order_and_layouts():
    f1, _, c = _case(N=1)
    c = np.abs(c)                                   # ordinary at every level (c / 2^l >= 0)
    f2s = A.level_maps(5, 2, 7, 10, 32, 3)
    ref, _ = A.alt_ref_levels(f1, f2s, c[:, 0], 2, scale_div=4.0)
    ref1, _ = A.alt_ref_levels(f1, f2s, c[:, 0].transpose(0, 3, 1, 2), 2, scale_div=4.0, coords_layout=1)
    assert np.array_equal(ref, ref1)
    for l, f2 in enumerate(f2s):
        want = O.alt_corr_forward(f1.astype(np.float64), f2.astype(np.float64),
                                  (c / np.float32(2 ** l)).astype(np.float64), 2)[:, 0] / 4.0
        assert np.abs(ref[:, 25 * l:25 * (l + 1)] - want).max() < 1e-12


def test_contract_for_huge_and_non_finite_coordinates():
    f1, f2, c = _case(N=1, H1=16, W1=24)
    ci, where = A.irregular_coords(c)
    ref, mag = A.alt_ref(f1, f2, ci, 2)
    base, _ = A.alt_ref(f1, f2, c, 2)
    w = where[:, :, None].repeat(25, 2)
    assert np.array_equal(ref[~w], base[~w])
    nonfin = ~np.isfinite(ci).all(-1)
    assert np.all(np.isnan(ref[nonfin[:, :, None].repeat(25, 2)]))
    fin_special = (where & ~nonfin)[:, :, None].repeat(25, 2)
    assert np.all(ref[fin_special] == 0) and np.all(mag[fin_special] == 0)
    # the backward: those queries are absent
    g = np.random.default_rng(0).standard_normal(ref.shape).astype(np.float32)
    (f1g, f2g, cg), _ = A.alt_bwd_ref(f1, f2, ci, g, 2)
    cz = c.copy()
    cz[where] = 1e6  # wholly off the map: contributes nothing either
    (f1z, f2z, cgz), _ = A.alt_bwd_ref(f1, f2, cz, g, 2)
    assert np.array_equal(f1g, f1z) and np.array_equal(f2g, f2z)
    assert np.all(cg[where] == 0) and np.array_equal(cg[~where], cgz[~where])


@pytest.mark.parametrize("r", [0, 1, 3])
def test_alt_bwd_ref_equals_autograd(r):
    f1, f2, c = _case(H1=6, W1=7, H2=5, W2=6, C=8)
    g = np.random.default_rng(3).standard_normal((2, 2, (2 * r + 1) ** 2, 6, 7))
    (f1g, f2g, cg), (m1, m2, mc) = A.alt_bwd_ref(f1, f2, c, g, r)
    a, b, cc = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (f1, f2, c))
    (T.alt_corr_forward(a, b, cc, r) * torch.tensor(g)).sum().backward()
    for got, ref, m in ((f1g, a.grad, m1), (f2g, b.grad, m2), (cg, cc.grad, mc)):
        assert np.abs(got - ref.numpy()).max() < 1e-11
        assert np.all(m >= np.abs(got) - 1e-11)


def test_builders_hold_their_promises():
    for bw, bh in [(10, 10), (13, 96), (96, 10), (97, 10), (10, 97), (28, 29), (49, 10)]:
        for edge in (False, True):
            c = A.box_coords(bw + bh, 16, 24, 112, 112, 4, bw, bh, edge)
            assert A.tile_boxes(c, 4)[(0, 0, 0, 0)][:2] == (bw, bh)
    with pytest.raises(AssertionError):
        A.box_coords(1, 16, 24, 112, 112, 4, 9, 10)      # narrower than one window
    c = A.mixed_fit_coords(3, 2, 16, 24, 24, 240)
    nofit = A.levels_fit(c, 4, 4, 96)
    assert [len(s) for s in nofit] == [1, 1, 0, 0]
    assert all(len(s) == 0 for s in A.levels_fit(A.smooth_coords(3, 2, 1, 16, 24, 24, 240, 0.7), 4, 4, 96))
    for kind in A.EDGE_SETS:
        for H2, W2 in ((14, 23), (1, 1), (2, 3)):
            assert A.edge_coords(kind, 7, 2, 1, 16, 24, H2, W2, 4).shape == (2, 1, 16, 24, 2)
    c, same = A.tied_coords(5, 16, 24, 12, 20)
    assert int(same.sum()) >= 200
    ci, where = A.irregular_coords(A.smooth_coords(1, 2, 1, 16, 24, 14, 23))
    assert int(where.sum()) == 27 and not where[1].any()
    tiles = {(y // 8, x // 8) for _, _, y, x in zip(*np.nonzero(where))}
    assert tiles == {(0, 0), (1, 2)}
    assert A.kernel_form(64, 4, "f16x3") == "mfma" and A.kernel_form(64, 4, "fp32") == "tile"
    assert A.kernel_form(36, 4, "f16x3") == "per-pixel<1>" and A.kernel_form(516, 4, "f16x3") == "per-pixel<4>"
    assert A.kernel_form(64, 5, "fp32") == "generic" and A.kernel_form(288, 4, "f16x3") == "per-pixel<2>"


# ----------------------------------------------------------------------------- mutations


def _mutation_case():
    r = 2
    rd = 2 * r + 1
    f1, _, c = _case(N=1)
    c[0, 0, 0, 0] = (3.0 + 0.01, 2.0 + 0.5)        # a tap of weight <= 0.02: dx = 0.01
    f2s = A.level_maps(5, 2, 7, 10, 32, 2)
    ref, mag = A.alt_ref_levels(f1, f2s, c[:, 0], r, scale_div=4.0)
    return r, rd, f1, f2s, c, ref, mag


FWD_MUTATIONS = ["ix-iy-swapped", "dx-dy-swapped", "origin-off-by-one", "next-level", "scale-twice",
                 "small-tap-dropped"]


@pytest.mark.parametrize("mut", FWD_MUTATIONS)
def test_forward_mutations_are_rejected(mut):
    r, rd, f1, f2s, c, ref, mag = _mutation_case()
    B, H1, W1 = 2, 9, 11
    if mut == "ix-iy-swapped":
        bad = ref.reshape(B, 2, rd, rd, H1, W1).transpose(0, 1, 3, 2, 4, 5).reshape(ref.shape)
    elif mut == "dx-dy-swapped":
        # (the blend with the fractions exchanged: feed the reference transposed maps and coordinates)
        def swapped(f2, div):
            _, i, d, _ = A.positions(c[:, 0], div)
            out = np.zeros((B, rd * rd, H1, W1))
            for b in range(B):
                x0, y0 = i[b, ..., 0].reshape(-1) - r, i[b, ..., 1].reshape(-1) - r
                s = A._taps(f1.reshape(B, -1, 32), f2, b, x0, y0, r, np.float64)
                o = A._blend(s, d[b, ..., 1].reshape(-1), d[b, ..., 0].reshape(-1), rd, np.float64) / 4.0
                out[b] = o.transpose(2, 1, 0).reshape(rd * rd, H1, W1)
            return out
        bad = np.concatenate([swapped(f2, float(2 ** l)) for l, f2 in enumerate(f2s)], 1)
    elif mut == "origin-off-by-one":
        bad, _ = A.alt_ref_levels(f1, f2s, c[:, 0] + np.float32(1.0), r, scale_div=4.0)
    elif mut == "next-level":
        bad, _ = A.alt_ref_levels(f1, [f2s[1], f2s[1]], c[:, 0], r, scale_div=4.0)
    elif mut == "scale-twice":
        bad = ref / 4.0
    else:
        # the query at (0, 0, 0, 0): bin (oy, ox) loses its s01 tap, whose weight is (1 - dy) dx = 0.005
        _, i, d, _ = A.positions(c[:, 0], 1.0)
        x0, y0 = i[0, ..., 0].reshape(-1) - r, i[0, ..., 1].reshape(-1) - r
        s = A._taps(f1.reshape(B, -1, 32), f2s[0], 0, x0, y0, r, np.float64)
        w = (1.0 - float(d[0, 0, 0, 1])) * float(d[0, 0, 0, 0])
        assert 0 < w <= 0.02
        bad = ref.copy()
        oy, ox = 1, 2
        bad[0, oy + rd * ox, 0, 0] -= s[0, oy, ox + 1] * w / 4.0
    assert not np.array_equal(bad, ref)
    for bound in BOUNDS:
        assert A.rejects(bad, ref, mag, bound), (mut, bound)
        A.check(ref, ref, mag, bound)
        A.check(ref.astype(np.float32), ref, mag, bound)      # ... and a correctly rounded result passes


def test_backward_mutations_are_rejected():
    H1, W1, H2, W2, C, r = 16, 24, 12, 20, 8, 2
    f1, f2 = A.maps(2, 1, H1, W1, H2, W2, C)
    c, same = A.tied_coords(5, H1, W1, H2, W2)
    g = np.random.default_rng(1).standard_normal((1, 1, 25, H1, W1)).astype(np.float32)
    (f1g, f2g, cg), (m1, m2, mc) = A.alt_bwd_ref(f1, f2, c, g, r)
    drop = np.zeros_like(same)
    drop[tuple(np.argwhere(same)[17])] = True         # one of the 200 tied queries
    (_, f2bad, _), _ = A.alt_bwd_ref(f1, f2, c, g, r, drop=drop)
    cbad = cg[..., ::-1]
    for bound in BOUNDS:
        assert A.rejects(f2bad, f2g, m2, bound)
        assert A.rejects(cbad, cg, mc, bound)
        A.check(f2g.astype(np.float32), f2g, m2, bound)
        A.check(cg.astype(np.float32), cg, mc, bound)


# ----------------------------------------------------------------------------- the bounds


def _ratio(got, ref, mag):
    ok = ~np.isnan(ref) & (mag > 0)
    return float((np.abs(got.astype(np.float64) - ref)[ok] / (A.U24 * mag[ok])).max())


def test_bound_measurement(capsys):
    """GAMMA32, GAMMA16X3 and GAMMA_BWD (alt_corr_oracle.py) cover the float32 / f16x3
    restatements on the GPU tests' own inputs; the figures are printed (pytest -s)."""
    g32 = 0.0
    for form in A.FORMS:
        C, r, _, H1, W1 = form
        f1, f2s, c = A.form_inputs(form)
        ref, mag = A.alt_ref(f1, f2s[0], c, r, scale_div=8.0)
        a = _ratio(A.alt_ref(f1, f2s[0], c, r, scale_div=8.0, dtype=np.float32)[0], ref, mag)
        b = _ratio(O.alt_corr_forward(f1, f2s[0], c, r) / np.float32(8.0), ref, mag)
        g32 = max(g32, a, b)
    for form in (A.CORE_FORMS[0], A.CORE_FORMS[4]):      # ... and the coordinate sets on the smallest fmap2
        C, r, _, H1, W1 = form
        f1, f2 = A.maps(C + r + 2, 2, H1, W1, 2, 3, C)
        for k, kind in enumerate(A.EDGE_SETS):
            c = A.edge_coords(kind, 31 * k + 2, 2, 1, H1, W1, 2, 3, r)
            ref, mag = A.alt_ref(f1, f2, c, r, scale_div=8.0)
            if mag.any():
                g32 = max(g32, _ratio(A.alt_ref(f1, f2, c, r, scale_div=8.0, dtype=np.float32)[0], ref, mag))
    gold = load_golden("lookup_b2c64_16x20.npz")
    m1 = np.ascontiguousarray(gold["fmap1"].transpose(0, 2, 3, 1))
    m2 = np.ascontiguousarray(gold["fmap2"].transpose(0, 2, 3, 1))
    c = A.smooth_coords(9, 2, 1, 16, 20, 16, 20, 1.5)
    g16 = {}
    for s in A.GAMMA16X3:
        a1, a2 = (m1 * np.float32(s)), (m2 * np.float32(s))
        ref, mag = A.alt_ref(a1, a2, c, 4, scale_div=8.0)
        g16[s] = _ratio(A.f16x3_restatement(a1, a2, c, 4, scale_div=8.0)[0], ref, mag)
    gb = 0.0
    for name in A.BWD_CASES:
        f1, f2, cc, g, r = A.bwd_case(name)
        ref, mags = A.alt_bwd_ref(f1, f2, cc, g, r)
        got, _ = A.alt_bwd_ref(f1, f2, cc, g, r, dtype=np.float32)
        gb = max(gb, max(_ratio(x, y, m) for x, y, m in zip(got, ref, mags)))
    with capsys.disabled():
        print(f"\nGAMMA32 measured {g32:.2f} (recorded {A.GAMMA32}); GAMMA_BWD measured {gb:.2f} "
              f"(recorded {A.GAMMA_BWD}); f16x3 restatement by map scale: "
              + ", ".join(f"2^{int(np.log2(s))}: {v:.2f} (recorded {A.GAMMA16X3[s]})" for s, v in g16.items()))
    assert g32 <= A.GAMMA32 and gb <= A.GAMMA_BWD
    assert all(g16[s] <= A.GAMMA16X3[s] for s in g16)
