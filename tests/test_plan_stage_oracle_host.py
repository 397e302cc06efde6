"""tests/plan_stage_oracle.py (torch fp64, one function per plan stage) pinned on the CPU.

* The stages chained for 3 iterations reproduce oracle.raft_oracle.raft_forward (numpy, float32: the
  restatement pinned to the reference's own goldens by tests/test_oracle_golden.py), RAFT-full and RAFT-small,
  all-pairs and alternate, seeded weights: flow_low and flow_up.  The difference is the float32 round-off of
  that oracle.  Measured on the CPU (flow_low / flow_up, against raft_forward in float32):

      full  all-pairs 1.98e-06 / 5.19e-06      full  alternate 1.98e-06 / 4.79e-06
      small all-pairs 1.64e-06 / 1.28e-05      small alternate 1.34e-06 / 1.05e-05

  The bounds are 4 x the measured maxima 1.98e-06 and 1.28e-05: FLOW_LOW_TOL = 7.92e-06, FLOW_UP_TOL =
  5.12e-05.  The frame pair is 128 x 136 (a 16 x 17 feature map), not 64 x 96: an 8 x 12 map pools to a 1 x 1
  fourth level, whose all-pairs lookup is NaN in the reference (core/utils/utils.py:60-61 divides by H - 1),
  and AlternateCorrBlock cannot pool it four times at all; 16 x 17 is the smallest ragged map on which both
  are defined, and the one the GPU stage test uses.  raft_forward in float64 on the same inputs is held to
  1e-9 besides, which pins the restatement itself rather than float32's round-off.
* update_step equals the update block's own conv layers (the nn.Conv2d of raft_optical_flow_amd.update's module
  tree, which compat/core/update.py re-exports, in .double(), composed as core/update.py composes them) and
  oracle.raft_oracle's float64 update blocks to 1e-12 relative.  (The modules' own forward runs on the HIP
  path only, so it cannot be the float64 reference; their layers can.)
* update_step reproduces the reference's recorded update-block outputs (tests/golden/update_*_16x24.npz,
  float32) to the 1e-4 those goldens are held to elsewhere.
"""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plan_stage_oracle as PSO
from conftest import load_golden
from oracle import raft_oracle as O
from raft_optical_flow_amd import RAFT
from raft_optical_flow_amd.init import seeded_images, seeded_state_dict

FLOW_LOW_TOL = 4 * 1.98e-6
FLOW_UP_TOL = 4 * 1.28e-5


def _model(small):
    m = RAFT(argparse.Namespace(small=small, mixed_precision=False, alternate_corr=False)).eval()
    sd = seeded_state_dict(m, 0)
    m.load_state_dict(sd)
    return m, sd


def _maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
@pytest.mark.parametrize("alternate", [False, True], ids=["allpairs", "alt"])
def test_chained_stages_reproduce_raft_forward(small, alternate):
    _, sd = _model(small)
    H, W = 128, 136
    i1, i2 = seeded_images(1, H, W)
    low, ups = PSO.forward(sd, i1, i2, 3, small, alternate)
    npsd = {k: v.numpy() for k, v in sd.items()}
    ref_low, ref_up = O.raft_forward(npsd, i1.numpy(), i2.numpy(), iters=3, small=small, alternate_corr=alternate)
    assert np.isfinite(ref_up).all()
    e_low, e_up = _maxabs(low, ref_low), _maxabs(ups[-1], ref_up)
    print(f"\nsmall={small} alt={alternate}: flow_low {e_low:.3g}  flow_up {e_up:.3g}  (vs float32 raft_forward)")
    assert e_low < FLOW_LOW_TOL and e_up < FLOW_UP_TOL, (e_low, e_up)
    r64_low, r64_up = O.raft_forward(npsd, i1.numpy(), i2.numpy(), iters=3, small=small, alternate_corr=alternate,
                                     dtype=np.float64)
    e_low, e_up = _maxabs(low, r64_low), _maxabs(ups[-1], r64_up)
    print(f"   flow_low {e_low:.3g}  flow_up {e_up:.3g}  (vs float64 raft_forward)")
    assert e_low < 1e-9 and e_up < 1e-9, (e_low, e_up)


def test_train_mode_list_and_flow_init():
    """Every iteration's flow_up and a non-zero flow_init (core/raft.py:208-211), against raft_forward in float64."""
    _, sd = _model(False)
    i1, i2 = seeded_images(1, 128, 136)
    g = torch.Generator().manual_seed(3)
    init = torch.randn(1, 2, 16, 17, generator=g) * 2
    _, ups = PSO.forward(sd, i1, i2, 2, False, flow_init=init)
    npsd = {k: v.numpy() for k, v in sd.items()}
    ref = O.raft_forward(npsd, i1.numpy(), i2.numpy(), iters=2, flow_init=init.numpy(), test_mode=False,
                         dtype=np.float64)
    assert len(ref) == len(ups) == 2
    for a, b in zip(ups, ref):
        assert _maxabs(a, b) < 1e-9


def _rel(a, b):
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


def _inputs(small, h=11, w=13, b=2):
    hd, cd, r = PSO.dims(small)
    g = torch.Generator().manual_seed(5)
    net = torch.tanh(torch.randn(b, hd, h, w, generator=g, dtype=torch.float64))
    inp = torch.relu(torch.randn(b, cd, h, w, generator=g, dtype=torch.float64))
    corr = torch.randn(b, 4 * (2 * r + 1) ** 2, h, w, generator=g, dtype=torch.float64)
    flow = torch.randn(b, 2, h, w, generator=g, dtype=torch.float64) * 3
    return net, inp, corr, flow


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
def test_update_step_equals_the_modules_layers_in_double(small):
    m, sd = _model(small)
    ub = m.update_block.double()
    net, inp, corr, flow = _inputs(small)
    e, gru, fh = ub.encoder, ub.gru, ub.flow_head
    with torch.no_grad():
        # core/update.py composed of the module tree's own layers
        cor = F.relu(e.convc1(corr))
        if not small:
            cor = F.relu(e.convc2(cor))
        flo = F.relu(e.convf2(F.relu(e.convf1(flow))))
        motion = torch.cat([F.relu(e.conv(torch.cat([cor, flo], 1))), flow], 1)
        x = torch.cat([inp, motion], 1)
        h = net
        steps = [(gru.convz, gru.convr, gru.convq)] if small else [(gru.convz1, gru.convr1, gru.convq1),
                                                                    (gru.convz2, gru.convr2, gru.convq2)]
        for cz, cr, cq in steps:
            hx = torch.cat([h, x], 1)
            z, r = torch.sigmoid(cz(hx)), torch.sigmoid(cr(hx))
            rh = r * h
            q = torch.tanh(cq(torch.cat([rh, x], 1)))
            h = (1 - z) * h + z * q
        delta = fh.conv2(F.relu(fh.conv1(h)))
        mask = None if small else 0.25 * ub.mask(h)
    p = PSO.params(sd)
    net2, delta2, mask2, det = PSO.update_step(net, inp, corr, flow, p, small, detail=True)
    assert _rel(net2, h) < 1e-12 and _rel(delta2, delta) < 1e-12
    assert _rel(det["out"], motion) < 1e-12 and _rel(det["z"], z) < 1e-12 and _rel(det["rh"], rh) < 1e-12
    if small:
        assert mask2 is None
    else:
        assert _rel(mask2, mask) < 1e-12
    # the numpy oracle's float64 blocks, written independently
    npsd = {k: v.numpy().astype(np.float64) for k, v in sd.items() if v.dtype.is_floating_point}
    blk = O.small_update_block if small else O.basic_update_block
    n3, m3, d3 = blk(net.numpy(), inp.numpy(), corr.numpy(), flow.numpy(), npsd)
    assert _rel(net2, torch.from_numpy(n3)) < 1e-12 and _rel(delta2, torch.from_numpy(d3)) < 1e-12
    if not small:
        assert _rel(mask2, torch.from_numpy(m3)) < 1e-12


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
def test_gru_context_plus_dynamic_part_is_the_whole_conv(small):
    """gru_context is the `inp` columns of each GRU conv with its bias: adding the conv of the remaining columns
    over [h | motion | flow] gives the whole conv of cat[h, inp, motion, flow]."""
    _, sd = _model(small)
    p = PSO.params(sd)
    hd, cd, _ = PSO.dims(small)
    net, inp, corr, flow = _inputs(small)
    me = PSO.motion_encoder(flow, corr, p, small)
    hx = torch.cat([net, inp, me["out"]], 1)
    dyn = torch.cat([net, me["out"]], 1)
    for ctx, (zk, rk, qk, pad) in zip(PSO.gru_context(inp, p, small), PSO.gru_steps(small)):
        for i, k in enumerate((zk, rk, qk)):
            w = p[k + ".weight"]
            rest = F.conv2d(dyn, torch.cat([w[:, :hd], w[:, hd + cd:]], 1), None, 1, pad)
            whole = F.conv2d(hx, w, p[k + ".bias"], 1, pad)
            assert _rel(ctx[:, i * hd:(i + 1) * hd] + rest, whole) < 1e-12


@pytest.mark.parametrize("small", [False, True], ids=["full", "small"])
def test_update_step_reproduces_the_reference_goldens(small):
    g = load_golden("update_small_16x24.npz" if small else "update_full_16x24.npz")
    wts = {k[len("w."):]: v for k, v in g.items() if k.startswith("w.")}
    if not wts:
        _, sd = _model(small)
        wts = {k: v for k, v in sd.items() if k.startswith("update_block.")}
    p = PSO.params({k if k.startswith("update_block.") else "update_block." + k: v for k, v in wts.items()})
    t = lambda a: torch.from_numpy(np.asarray(a)).double()   # noqa: E731
    net, delta, mask = PSO.update_step(t(g["net"]), t(g["inp"]), t(g["corr"]), t(g["flow"]), p, small)
    assert _maxabs(net, g["net_out"]) < 1e-4 and _maxabs(delta, g["delta_out"]) < 1e-4
    if not small:
        assert _maxabs(mask, g["mask_out"]) < 1e-4


def test_lookup_marks_one_pixel_levels_nan_like_raft_oracle():
    rng = np.random.default_rng(2)
    f1 = rng.standard_normal((1, 16, 9, 17))
    f2 = rng.standard_normal((1, 16, 9, 17))
    coords = O.coords_grid(1, 9, 17, np.float64) + rng.uniform(-6, 6, (1, 2, 9, 17))
    ref = O.corr_lookup(O.corr_pyramid(f1, f2, 4), coords, 4)
    got = PSO.lookup(PSO.corr_pyramid(torch.from_numpy(f1), torch.from_numpy(f2)), torch.from_numpy(coords), 4).numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.isnan(got[:, 243:]).all() and np.isfinite(got[:, :243]).all()
    assert _maxabs(got[:, :243], ref[:, :243]) < 1e-12
