"""Host checks of tests/lookup_oracle.py, the reference the GPU lookup tests
(test_gpu_lookup_forms.py) compare against: lookup_ref against the fp32 oracle and against
torch's grid_sample, tile_levels against an untiling written here, the comparison against
hand-mutated references, and the input conditions of the deferred-path tests -- the coordinate
sets those tests use reach the path on the levels they claim, so they cannot pass vacuously."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lookup_oracle as LO
from oracle import raft_oracle as O


def _pooled(B, H, W, C, L, seed):
    rng = np.random.default_rng(seed)
    f1 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    f2 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    pyr = O.corr_pyramid(f1, f2, L)                       # [B*H*W, 1, h_l, w_l]
    return pyr, [p[:, 0] for p in pyr]


@pytest.mark.parametrize("B,H,W,L,r", [(2, 9, 13, 4, 3), (1, 12, 17, 3, 4), (2, 8, 8, 4, 1)])
def test_lookup_ref_equals_fp32_oracle(B, H, W, L, r):
    """lookup_ref (fp32 positions, fp64 blend) against oracle.corr_lookup (all fp32) on a pooled
    pyramid, within the GPU tests' bound; 9x13 and 8x8 have a 1-px last level (NaN taps)."""
    pyr, levels = _pooled(B, H, W, 16, L, seed=H)
    coords = LO.matrix_coords(B, H, W, seed=W, sigma=2.0)
    ref, cmax = LO.lookup_ref(levels, coords, r)
    cn = coords.reshape(B, H, W, 2).transpose(0, 3, 1, 2)
    got = O.corr_lookup(pyr, cn, r).transpose(0, 2, 3, 1).reshape(B * H * W, -1)
    assert got.dtype == np.float32
    bad, ratio = LO.tap_check(got, ref, cmax)
    assert not bad.any(), LO.describe_bad(bad, got, ref, cmax, (2 * r + 1) ** 2)
    assert np.isnan(ref).any() == (min(H, W) >> (L - 1) == 1)
    assert ratio > 0  # the two are not the same arithmetic: the comparison is not vacuous


def test_lookup_ref_equals_grid_sample():
    """One small case against the reference's real operator: core/utils/utils.py's
    bilinear_sampler = F.grid_sample(align_corners=True) of 2x/(W-1)-1, in fp32 on the CPU."""
    B, H, W, L, r = 1, 10, 14, 3, 2
    _, levels = _pooled(B, H, W, 8, L, seed=3)
    coords = LO.matrix_coords(B, H, W, seed=4, sigma=2.0)
    ref, cmax = LO.lookup_ref(levels, coords, r)
    n, rd = B * H * W, 2 * r + 1
    d = torch.linspace(-r, r, rd)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), -1).view(1, rd, rd, 2)   # core/corr.py:41-44
    outs = []
    for l, lv in enumerate(levels):
        h, w = lv.shape[1:]
        c = torch.from_numpy(coords).view(n, 1, 1, 2) / 2 ** l + delta
        xg = 2 * c[..., 0] / (w - 1) - 1
        yg = 2 * c[..., 1] / (h - 1) - 1
        s = F.grid_sample(torch.from_numpy(lv)[:, None], torch.stack([xg, yg], -1), align_corners=True)
        outs.append(s.view(n, rd * rd))
    got = torch.cat(outs, 1).numpy()
    bad, _ = LO.tap_check(got, ref, cmax)
    assert not bad.any(), LO.describe_bad(bad, got, ref, cmax, rd * rd)


def test_tile_levels_round_trip():
    """tile_levels against the header's formula applied element by element, every other float 0."""
    B, H, W, L = 1, 3, 2, 3
    H2, W2 = 11, 6                              # the maps need not be the query grid's size here
    rng = np.random.default_rng(0)
    dims = LO.level_dims(H2, W2, L)
    levels = [rng.standard_normal((B * H * W, h, w)).astype(np.float32) + 3.0 for h, w in dims]
    buf = LO.tile_levels(levels, B, H, W).numpy()
    seen = np.zeros(buf.shape, bool)
    off = 0
    for lv, (h, w) in zip(levels, dims):
        th, tw = -(-h // 4), -(-w // 4)
        S = th * tw * 16
        for p in range(B * H * W):
            for y in range(h):
                for x in range(w):
                    i = off + p * S + ((y >> 2) * tw + (x >> 2)) * 16 + (y & 3) * 4 + (x & 3)
                    assert buf[i] == lv[p, y, x] and not seen[i]
                    seen[i] = True
        off += B * H * W * S
    assert off == buf.size and (buf[~seen] == 0).all() and (~seen).any()


def _mutants(levels, coords, r):
    rd2 = (2 * r + 1) ** 2
    L = len(levels)
    ref, cmax = LO.lookup_ref(levels, coords, r)
    shifted = LO.lookup_ref([np.roll(lv, 1, axis=2) for lv in levels], coords, r)[0]      # one corner column over
    swapped = ref.reshape(-1, L, 2 * r + 1, 2 * r + 1).transpose(0, 1, 3, 2).reshape(ref.shape)  # ix <-> iy
    nextlvl = np.roll(ref.reshape(-1, L, rd2), -1, axis=1).reshape(ref.shape)              # reads level l + 1
    return ref, cmax, {"corner": shifted, "ix_iy": swapped, "level": nextlvl}


@pytest.mark.parametrize("u,abs_term", [(0.0, 0.0), (2.0 ** -20, 2.0 ** -24), (2.0 ** -11, 2.0 ** -24),
                                       (2.0 ** -8, 2.0 ** -24)], ids=["plain", "f16x3", "f16", "bf16"])
def test_comparison_rejects_mutated_references(u, abs_term):
    """The GPU tests' comparison at each of their bounds (the plain lookup's and the fused kernel's
    three precisions): a stand-in for a correct kernel (the reference rounded to fp32) passes, and a
    reference with one corner column shifted, ix / iy swapped in the channel order, or level l + 1
    read for level l fails -- on independent random levels each is an O(1) error on the taps on the map."""
    B, H, W, L, r = 2, 17, 21, 4, 4
    rng = np.random.default_rng(1)
    levels = [rng.standard_normal((B * H * W, h, w)).astype(np.float32) for h, w in LO.level_dims(H, W, L)]
    coords = LO.matrix_coords(B, H, W, seed=2)
    ref, cmax, muts = _mutants(levels, coords, r)
    got = ref.astype(np.float32)
    assert not LO.tap_check(got, ref, cmax, u, abs_term)[0].any()
    for name, m in muts.items():
        bad = LO.tap_check(got, m, cmax, u, abs_term)[0]
        assert bad.mean() > 0.1, (name, bad.mean())  # (half the taps of this set lie off the map: 0 either way)
    # and restricted to the deferred taps alone (section b's separate assertion)
    dcoords = LO.deferred_coords(B, H, W, seed=5)
    ref, cmax, muts = _mutants(levels, dcoords, r)
    off = LO.off_patch_taps(dcoords, LO.level_dims(H, W, L), r)
    assert off.sum() > 50
    for name, m in muts.items():
        bad = LO.tap_check(ref.astype(np.float32), m, cmax, u, abs_term)[0]
        assert bad[off].any(), name


def test_deferred_path_input_conditions():
    """Every coordinate set of the deferred-path GPU tests reaches the path: off_patch counts
    >= 64 pixels on each of levels 0, 1, 2 at 55x128 (r = 4) and >= 16 on each of levels 0, 1 at
    23x37 (every radius run there), and >= 16 on level 3 in every set.  The identity grid alone
    (a forward's first iteration) gives 1118 / 1040 / 256 / 128 at 55x128: 362 / 290 / 128 / 0 of
    them through the x axis or a row outside the window's tile rows, the rest through a row inside
    those tile rows but outside the window's own 2r + 2 fetched rows (lookup_common.hpp)."""
    dims = LO.level_dims(55, 128, 4)
    ident = LO.off_patch(LO.grid_xy(1, 55, 128), dims, 4).sum(0)
    assert list(ident) == [1118, 1040, 256, 128]
    n = LO.off_patch(LO.deferred_set(1, 55, 128), dims, 4).sum(0)
    assert (n[:3] >= 64).all() and n[3] >= 16, n
    dims = LO.level_dims(23, 37, 4)
    assert list(LO.off_patch(LO.grid_xy(1, 23, 37), dims, 4).sum(0)) == [186, 131, 0, 0]
    for B, radii in ((2, (1, 2, 3, 4)), (20, (4,))):
        c = LO.deferred_set(B, 23, 37)
        for r in radii:
            n = LO.off_patch(c, dims, r).sum(0)
            assert (n[:2] >= 16).all() and n[3] >= 16, (B, r, n)


def test_level3_deferred_path_exists():
    """Level 3, searched over every integer in [-80, size + 80] on either axis, r = 1..4, the same
    + 2^-20, and the fp32 number just below each integer.  On x no integer (+ 2^-20) reaches the
    deferred path at these sizes; on y one does at 55x128 (a level-3 row the round trip moves out of
    the window's rows) and none at 23x37, whose level 3 is 2 rows (H - 1 = 1: the round trip is exact).
    The number just below a multiple of 8 reaches it on both axes at both sizes: c / 8 + offset
    rounds up to the next integer while the window was staged for floor(c) >> 3.  deferred_coords
    therefore draws such coordinates (its fifth kind)."""
    for H, W in ((55, 128), (23, 37)):
        dims = LO.level_dims(H, W, 4)
        for r in (1, 2, 3, 4):
            for a, size in ((0, W), (1, H)):
                v = np.arange(-80, size + 80, dtype=np.float32)
                c = np.full((len(v), 2), 3.0, np.float32)
                for eps in (0.0, 2.0 ** -20):
                    c[:, a] = v + np.float32(eps)
                    hit = LO.off_patch(c, dims, r)[:, 3]
                    assert hit.any() == (a == 1 and H == 55), (H, W, r, a, eps)
                c[:, a] = np.nextafter(v, np.float32(-np.inf))
                hit = LO.off_patch(c, dims, r)[:, 3]
                assert hit.any() and (v[hit] % 8 == 0).all()


def test_off_patch_matches_its_definition_on_a_known_case():
    """x = 4 at r = 4, W = 128: tap offset -4 samples X = 0 exactly (on the patch, origin 0);
    x = 8: X = 4, where the round trip through 2 X / 127 - 1 comes back just below 4: the floor
    drops to 3, left of the patch origin 4.  y = 5 at H = 55: the window's rows are 1 .. 10 and
    offset -4 samples Y = 1, which comes back as 0.9999994: row 0, inside the window's tile rows
    but not one of its rows."""
    dims = LO.level_dims(55, 128, 1)
    c = np.array([[4.0, 20.5], [8.0, 20.5]], np.float32)
    fin, i, t = LO._axis(c[:, 0], 0, 4, 128)
    assert i[0, 0] == 0 and t[0, 0] == 0
    got = LO.off_patch(c, dims, 4)[:, 0]
    assert i[1, 0] == 3 and bool(got[1]) and not got[0]
    c = np.array([[20.5, 5.0]], np.float32)
    fin, i, t = LO._axis(c[:, 1], 0, 4, 55)
    assert i[0, 0] == 0 and t[0, 0] == np.float32(1 - 10 * 2.0 ** -24)
    assert LO.off_patch(c, dims, 4)[0, 0]
