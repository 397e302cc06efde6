"""Every all-pairs correlation build form (corr_pyramid.hip: corr_build_kernel<false> / <true>,
corr_build2_kernel, corr_split4_kernel + corr_build4_kernel<L1, L2, NW>, pool2_tiled_kernel, untile_kernel)
through raft_corr_build, raft_corr_build_prec (F16X3) and raft_corr_build_ws (F16X3, 8 and 4 waves) against
tests/corr_build_oracle.py, element by element.

Every case: the pyramid and the workspace prefilled with one NaN bit pattern between guards, the fmaps inside
NaN-filled allocations (NaN rows before and after, NaN in the ld - C columns).  The whole raw buffer is
compared with tile(reference): |got - ref| <= k mag per element, mag = sum_c |f1_c f2_c| / sqrt_c pooled like
the levels, exactly 0 where mag is 0 (all the padding), no NaN left, nothing excluded.  k = max(4 r, 2 x 2^-24),
r the largest err / mag of the float32 restatement of the documented arithmetic on the same case, measured here
on the host (never from a kernel); 4 covers the MFMA's accumulation order, 2 x 2^-24 is one rounding of the
division plus one of the pool.  raft_corr_pyramid_level of every level is bit-identical to the raw buffer's
valid elements, and every level l >= 1 is bit for bit (((a0+a1)+a2)+a3)/4 of the kernel's own level l - 1.

Each case prints k and the kernel's largest err / mag (pytest -s; profiles/corr_build_gpu_tests.log,
DESIGN.md 7.4)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import corr_build_gpu as G
import corr_build_oracle as CB

pytestmark = pytest.mark.gpu
U = CB.U24
ENTRIES = G.ENTRIES


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()
    yield
    _case.cache_clear()
    torch.cuda.empty_cache()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ----------------------------------------------------------------------------- references, computed once


class Case:
    """One input set and its fp64 reference; the tiled reference per level and the restatement's err / mag per
    level and precision are computed on first use and kept (a level's segment of the raw buffer does not
    depend on how many levels follow)."""

    def __init__(self, B, H, W, L, f1, f2, sqrt_c):
        self.shape, self.f1, self.f2, self.sqrt_c = (B, H, W, L), f1, f2, sqrt_c
        self.ref, self.mag = CB.reference(f1, f2, L, sqrt_c, B, H, W)
        self._tiles, self._r = {}, {}

    def tiles(self, L):
        B, H, W, _ = self.shape
        for l in range(L):
            if l not in self._tiles:
                self._tiles[l] = (CB.tile([self.ref[l]], B, H, W), CB.tile([self.mag[l]], B, H, W))
        return (np.concatenate([self._tiles[l][0] for l in range(L)]),
                np.concatenate([self._tiles[l][1] for l in range(L)]))

    def k(self, prec, L):
        B, H, W, Lmax = self.shape
        if prec not in self._r:
            lv = CB.restate(self.f1, self.f2, Lmax, self.sqrt_c, prec, B, H, W)
            self._r[prec] = [CB.measure([lv[l]], [self.ref[l]], [self.mag[l]]) for l in range(Lmax)]
        return CB.bound_k(max(self._r[prec][:L]))


@functools.lru_cache(maxsize=3)
def _case(B, H, W, C, L, seed, kexp=0, sqrt_c=None):
    f1, f2 = CB.features(B, H, W, C, seed, 2.0 ** kexp)
    return Case(B, H, W, L, f1, f2, CB.sqrt_c32(C) if sqrt_c is None else sqrt_c)


def _verify(tag, entry, case, raw, levels=None, L=None, poisoned=None):
    """The checks of every case (module docstring).  poisoned: a raw-buffer mask of the elements a non-finite
    or out-of-range feature reaches, exempt here (their test checks them)."""
    B, H, W, Lmax = case.shape
    L = Lmax if L is None else L
    k = case.k(G.prec_of(entry), L)
    tref, tmag = case.tiles(L)
    assert raw.shape == tref.shape
    bad, worst = CB.compare(raw if poisoned is None else np.where(poisoned, tref, raw), tref, tmag, k)
    print(f"CBLOG {tag} entry={entry} shape={B}x{H}x{W} C={case.f1.shape[1]} L={L} k={k / U:.3f} "
          f"kernel={worst / U:.3f}")
    assert not bad.any(), CB.describe_bad(bad, raw, tref, tmag, B, H, W, L)
    assert not np.isnan(raw[~poisoned] if poisoned is not None else raw).any()
    own = CB.untile(raw, B, H, W, L)
    if levels is not None:
        assert len(levels) == L and all(_same_bits(a, b) for a, b in zip(levels, own)), "raft_corr_pyramid_level"
    if poisoned is None:
        assert all(CB.pool_exact(own)), CB.pool_exact(own)
    return worst


def _run(tag, entry, case, ld=None, env=None, L=None, **kw):
    B, H, W, Lmax = case.shape
    L = Lmax if L is None else L
    raw, levels = G.build(entry, case.f1, case.f2, B, H, W, L, case.sqrt_c, ld=ld, env=env, accessor=True, **kw)
    _verify(tag, entry, case, raw, levels, L)
    return raw


# ----------------------------------------------------------------------------- tile geometry


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("B,H,W,L", CB.GEOMETRY)
def test_tile_geometry(B, H, W, L, entry):
    """Every entry at every shape of corr_build_oracle.GEOMETRY (C = 64; what each shape is there for:
    test_corr_build_oracle_host.py); one shape divides by 3.0, which a reciprocal multiply misses by more
    than the floor of the bound."""
    sc = 3.0 if (B, H, W, L) == CB.GEOMETRY_SQRT3 else None
    _run("geometry", entry, _case(B, H, W, CB.GEOMETRY_C, L, seed=H * 1000 + W, sqrt_c=sc))


# ----------------------------------------------------------------------------- channel counts


_CHANNEL_CASES = ([("fp32", c) for c in CB.CHANNELS["fp32"]] + [("prec", c) for c in CB.CHANNELS["prec"]] +
                  [(e, c) for c in CB.CHANNELS["ws"] for e in ("ws8", "ws4")])


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("entry,C", _CHANNEL_CASES)
def test_channel_counts(entry, C, pad):
    """K tails of the 32-channel step (C % 32 != 0, zero-filled by a select), half-step counts 4 .. 64 of the
    workspace build, ld = C and ld = C + 4 with NaN in the unused columns (never read)."""
    B, H, W, L = CB.CHANNEL_SHAPE
    _run("channels", entry, _case(B, H, W, C, L, seed=C), ld=C + pad)


@pytest.mark.parametrize("entry", ["ws8", "ws4"])
@pytest.mark.parametrize("C,fp32", [(c, False) for c in CB.WS_FALLBACK_C] + [(64, True)])
def test_ws_fallbacks_are_the_plain_build(C, fp32, entry):
    """raft_corr_build_ws outside its kernel's shapes (C < 64, C % 16 != 0, C > 1024, FP32) is
    raft_corr_build_prec bit for bit, raft_corr_build_ws_bytes_prec is 0, the workspace stays untouched."""
    from raft_optical_flow_amd import _lib
    B, H, W, L = CB.CHANNEL_SHAPE
    case = _case(B, H, W, C, L, seed=C)
    plain = "fp32" if fp32 else "prec"
    want = _run("fallback", plain, case, ld=C + 4)
    got = G.build(entry, case.f1, case.f2, B, H, W, L, case.sqrt_c, ld=C + 4, ws_kernel=False,
                  ws_prec=_lib.PREC_FP32 if fp32 else None)
    assert _same_bits(got, want)


# ----------------------------------------------------------------------------- the persistent pipeline


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _per_image(raws, B, H, W, L):
    """B one-image raw buffers -> the raw buffer of the batch (levels back to back, images within a level)."""
    out, off = [], 0
    for h, w in CB.level_dims(H, W, L):
        n = H * W * ((h + 3) // 4) * ((w + 3) // 4) * 16
        out += [r[off:off + n] for r in raws]
        off += n
    return np.concatenate(out)


@pytest.mark.parametrize("which,nw,L", [(wh, nw, L) for wh in ("multi", "three") for nw in (8, 4)
                                       for L in CB.PIPELINE_L])
def test_persistent_pipeline(which, nw, L):
    """corr_build4_kernel<L1, L2, NW> with work-groups that take several units (the since / wait_vm<NDMA *
    (AHEAD - 1) + NSTORE> accounting; NSTORE 32, 40, 44 by level count): B from the device's CU count so that
    units > work-groups, not a multiple of them ("multi"), and >= 3 units on some work-group ("three").
    Against fp64, and bit-identical to the same images built one at a time (the same unit arithmetic on
    another unit-to-work-group assignment: a DMA landing in a stage still being read shows as a difference)."""
    H, W = CB.PIPELINE_HW
    cus = _cus()
    wgs = cus if nw == 8 else 2 * cus
    B = CB.pipeline_batches(cus, nw)[which == "three"]
    un = CB.units(B, H, W, nw)
    assert un > wgs and un % wgs != 0 and CB.units(1, H, W, nw) < wgs
    if which == "three":
        assert -(-un // wgs) >= 3
    entry = f"ws{nw}"
    case = _case(B, H, W, CB.PIPELINE_C, max(CB.PIPELINE_L), seed=B)
    raw = _run(f"pipeline-{which}({un}/{wgs})", entry, case, L=L)
    P = H * W
    singles = [G.build(entry, case.f1[b * P:(b + 1) * P], case.f2[b * P:(b + 1) * P], 1, H, W, L, case.sqrt_c)
               for b in range(B)]
    assert _same_bits(raw, _per_image(singles, B, H, W, L))


# ----------------------------------------------------------------------------- switches read per call


@pytest.mark.parametrize("entry", ["prec", "ws8", "ws4"])
@pytest.mark.parametrize("shape", ["multi-unit", "ragged"])
def test_nontemporal_stores_bit_identical(shape, entry):
    """RAFT_CORR_NT=1 (on by default only past 512 MiB of level 0) writes the bytes RAFT_CORR_NT=0 writes."""
    if shape == "ragged":
        B, H, W, L = CB.SWITCH_CASES[0]
        case = _case(B, H, W, CB.SWITCH_C, L, seed=900)
    else:
        H, W = CB.PIPELINE_HW
        B, L = CB.pipeline_batches(_cus(), 4 if entry == "ws4" else 8)[0], 3
        case = _case(B, H, W, CB.PIPELINE_C, max(CB.PIPELINE_L), seed=B)
    on = _run(f"nt-{shape}", entry, case, env={"RAFT_CORR_NT": "1"}, L=L)
    off = G.build(entry, case.f1, case.f2, B, H, W, L, case.sqrt_c, env={"RAFT_CORR_NT": "0"})
    assert _same_bits(on, off)


# ----------------------------------------------------------------------------- switches read once per process


def test_once_per_process_switches():
    """RAFT_CB4_L2=0 (level 2 by pool2_tiled_kernel from level 1 instead of the build's registers) and
    RAFT_CORR_BUILD_BIG=0 (corr_build_kernel<true>, f16x3 on 64 x 64 tiles) in one fresh child process
    (corr_build_gpu.py), which writes its raw pyramids to a file: the CB4_L2=0 pyramids are this process's
    default builds bit for bit; the 64 x 64 f16x3 pyramids hold the elementwise bound against fp64 with zero
    padding (their sums acc + (acc2 + acc3) are ordered differently from corr_build2's)."""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "child.npz")
        env = dict(os.environ, RAFT_CB4_L2="0", RAFT_CORR_BUILD_BIG="0")
        for k in G.SWITCHES:
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                         "corr_build_gpu.py"), out],
                           env=env, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with np.load(out) as z:
            child = {k: z[k] for k in z.files}
    for i in range(len(CB.SWITCH_CASES)):
        (B, H, W, L), f1, f2, sc = G.switch_case_inputs(i)
        case = Case(B, H, W, L, f1, f2, sc)
        for entry in ("ws8", "ws4"):
            mine = _run(f"cb4-l2-default-{i}", entry, case)
            assert _same_bits(child[f"{entry}_{i}"], mine), (entry, i)
        _verify(f"build-big-0-{i}", "prec", case, child[f"prec_{i}"])


# ----------------------------------------------------------------------------- magnitudes


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kexp", CB.SWEEP_K)
def test_magnitude_sweep(kexp, entry):
    """Features x 2^kexp: F16X3 follows the restatement at every scale under the same rule (its k grows as
    1 / s below 2^-3: lo in the f16 subnormals), FP32 stays at its own k throughout."""
    B, H, W, L = CB.SWEEP_SHAPE
    _run(f"sweep-2^{kexp}", entry, _case(B, H, W, CB.SWEEP_C, L, seed=7, kexp=kexp))


def _poison_case(side, where, value):
    """(case with the value, case with 0 in its place, raw-buffer mask of what the value may reach, the mask's
    valid elements): CB.POISON_SHAPE, channel POISON_CHANNEL of one row of image POISON_IMAGE."""
    B, H, W, L = CB.POISON_SHAPE
    P = H * W
    px = CB.POISON_INSIDE if where == "inside" else CB.POISON_DROPPED
    row = CB.POISON_IMAGE * P + px
    f1, f2 = CB.features(B, H, W, CB.POISON_C, seed=41)
    z1, z2 = f1.copy(), f2.copy()
    (f1 if side == "query" else f2)[row, CB.POISON_CHANNEL] = value
    (z1 if side == "query" else z2)[row, CB.POISON_CHANNEL] = 0.0
    ind = []
    for l, (h, w) in enumerate(CB.level_dims(H, W, L)):
        m = np.zeros((B * P, h + (-h) % 4, w + (-w) % 4), np.float32)   # whole tiles: padding addressable
        if side == "query":
            m[row] = 1
        else:
            cell = CB.target_cells(px, H, W, L)[l]
            if cell is not None:
                m[CB.POISON_IMAGE * P:(CB.POISON_IMAGE + 1) * P, cell[0], cell[1]] = 1
        ind.append(m)
    reach = np.concatenate([CB.tile([m], B, H, W) for m in ind]) > 0
    sc = CB.sqrt_c32(CB.POISON_C)
    return (B, H, W, L), (f1, f2), Case(B, H, W, L, z1, z2, sc), reach, reach & CB.valid_mask(B, H, W, L)


def _check_poison(tag, entry, side, where, value, nan_only=False):
    (B, H, W, L), (f1, f2), zcase, reach, hit = _poison_case(side, where, value)
    zero = _run(f"{tag}-zeroed", entry, zcase)
    got = G.build(entry, f1, f2, B, H, W, L, zcase.sqrt_c)
    # everything the value cannot reach: bit for bit the build with 0 in its place (padding included)
    assert _same_bits(got[~reach], zero[~reach]), f"{int((got[~reach] != zero[~reach]).sum())} floats differ"
    # every valid element it reaches: non-finite (NaN where the rule says NaN)
    assert hit.any() and (np.isnan(got[hit]).all() if nan_only else not np.isfinite(got[hit]).any())
    if side == "query":
        # its maps' padding: unspecified at level 0, exactly 0 deeper
        n0 = B * H * W * ((H + 3) // 4) * ((W + 3) // 4) * 16
        pad = reach & ~hit
        pad[:n0] = False
        assert (got[pad] == 0).all()
    else:
        assert (reach == hit).all()    # a target never reaches padding
        levels = CB.untile(hit, B, H, W, L)
        want = [c is not None for c in CB.target_cells(CB.POISON_INSIDE if where == "inside" else CB.POISON_DROPPED,
                                                       H, W, L)]
        assert [bool(x.any()) for x in levels] == want


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("side", ["query", "target"])
def test_out_of_range(side, entry):
    """One feature of 1e5.  FP32: finite, within the bound.  F16X3 (|fmap| >= 65520: hi = inf, lo = -inf):
    NaN in exactly the elements a non-finite feature would reach, everything else bit for bit the build with
    0 in its place."""
    if entry == "fp32":
        (B, H, W, L), (f1, f2), zcase, _, _ = _poison_case(side, "inside", 1e5)
        raw = _run(f"range-{side}", entry, Case(B, H, W, L, f1, f2, zcase.sqrt_c))
        assert np.isfinite(raw).all()
    else:
        _check_poison(f"range-{side}", entry, side, "inside", 1e5, nan_only=True)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "pinf", "ninf"])
@pytest.mark.parametrize("side,where", [("query", "inside"), ("target", "inside"), ("target", "dropped")])
def test_non_finite_features(side, where, value, entry):
    """A NaN / +Inf / -Inf in one channel of one fmap1 row changes only that query's maps (all its valid
    elements non-finite, deeper-level padding still 0); in one fmap2 row it makes non-finite exactly the
    level-0 element q of every query of that image and the pooled cells that contain it (none for a pixel in
    the last row that the floor pool drops) and never touches padding.  Every other float of the buffer is
    bit-identical to the build with that feature set to 0, which holds the fp64 bound."""
    _check_poison(f"nonfinite-{side}-{where}", entry, side, where, value)
