"""Every stage of the engine's plans against fp64, under every plan-time switch.

A RaftPlan is built directly (PackedRaft of a seeded model, images from init.seeded_images) and run in slices
with K.run: the launches before the loop, then each iteration, then raft_flow_from_coords.  After each slice the
plan's own buffers are read and each stage is held to tests/plan_stage_oracle.py (torch fp64 restatements of the
reference's operations on the model's own state_dict: no packing, no permutation) EVALUATED ON THE PLAN'S OWN
INPUT TO THAT STAGE, so no error compounds from stage to stage:

  prep          the prep rows                                   <- the images
  fnet          plan.fmap, both frames                          <- the GPU prep rows
  cnet          the h and inp columns of ub.hx                  <- the GPU prep rows
  ctx           each ub.ctx[i] = z | r | q, biases included     <- GPU inp, the raw convz / convr / convq weights
  corr          every pyramid level / pooled fmap2 level        <- GPU fmap
  lookup        ub.corr where a launch writes it, the flow slot <- GPU pyramid (alternate: GPU fmap), GPU coords
  cor1, flo1    convc1 / convf1 outputs                         <- GPU corr where written, else the fp64 lookup
  update        motion, z and r*h of the last half-step, new h, <- GPU h, inp, the fp64 lookup of the GPU coords
                coords, mask
  up            flow_up, flow_low                               <- GPU coords and mask

Before the first iteration ub.coords is overwritten with the grid + a seeded flow of up to 6 px, with some
queries sent off the map altogether, and the h columns with a seeded tanh state (the oracle gets the same), so
the update stage is not dominated by zero flow.  ub.fh is prefilled with a sentinel: an iteration without a mask
(the fh1-only branch) must leave its mask half alone; the pad and inp columns of ub.hx must not change in the loop.

Shapes.  The all-pairs sampler is undefined on a level one pixel high (the reference divides by H - 1 = 0 and
returns NaN; the kernels reproduce the NaN, and the conv epilogues' fmaxf then drops it where torch's relu keeps
it).  B=2, 72 x 136 (a 9 x 17 map: levels 9x17, 4x8, 2x4, 1x2) is therefore checked through the lookup (NaN
exactly where the oracle has it) and convf1; the update and upsampling stages are checked on B=2, 128 x 136
(16 x 17: levels 16x17, 8x8, 4x4, 2x2), the smallest ragged map whose four levels are all defined.  The alternate
path runs B=1, 128 x 136.

Bounds, all relative to max(1, max|ref|) of the compared tensor:
  * single-conv stages (prep, ctx, cor1, flo1): test_gpu_parity.CONV_TOL[prec];
  * corr levels and the all-pairs lookup 1e-5, the alternate lookup 1e-4 (test_gpu_parity / test_gpu_lookup_conv);
    the flow slot, flow_low and flow_up (fp32 elementwise kernels, exp for the softmax) 1e-5;
  * multi-conv stages (fnet, cnet, update): 4 x the default plans' worst measured error over all cases, rounded up
    to one digit, and never above (convs in the stage) x CONV_TOL[prec].  MEASURED / MULTI below and DESIGN.md 7.5:

                          fp32      f16x3     f16       bf16
      fnet    measured    1.53e-6   1.37e-6   1.84e-3   1.41e-2
              bound       7e-6      6e-6      8e-3      6e-2
      cnet    measured    5.61e-6   4.44e-6   5.49e-3   4.62e-2
              bound       3e-5      2e-5      3e-2      2e-1
      update  measured    1.26e-6   1.20e-6   9.43e-4   6.75e-3
              bound       6e-6      5e-6      4e-3      3e-2
      cap (15 x CONV_TOL) 1.5e-3    1.5e-3    7.5e-2    4.5e-1   (RAFT-small's update: 9 x)

Planted errors, each found at the stage that owns it with every earlier stage passing (full f16x3, all-pairs and
alternate): icols / mcols swapped in PackedUpdate -> ctx (relative error 1.6), then update; bctx dropped -> ctx
(1.2e-2), then update; alpha = 1.0 for mask2 -> update's mask alone (0.28); the K.JOIN after the context branch
omitted -> check c (the capture refuses the unjoined side stream; the sliced run synchronises between slices
and cannot see it).

Switches (tools/plan_signature.py::SWITCHES, imported).  For each setting a fresh plan is built under
monkeypatch.setenv, never through the model's plan cache; its canonical launch text must differ from the default
plan's, or, where the switch cannot act on that network, equal it (nothing more to run then).  Then
  a. every stage bound above holds for the switched plan (full f16x3, small f16x3, full fp32);
  b. bit-equality with the default plan's buffers, by what the switch changes (BIT_EQUAL):
     - RAFT_CTX_SIDE=0, RAFT_CTX_ORDER=early|mix, RAFT_FLOW_SIDE=0 (RAFT-small; RAFT-full with RAFT_CONV_PAIR=0)
       only move launches between streams or reorder independent ones: every buffer;
     - RAFT_MERGE_FUSED=0: raft_instnorm_merge_fused runs raft_instnorm_merge_ws's two levels in the same order
       (csrc/misc.hip), so the statistics and everything after them: every buffer;
     - RAFT_EPI_STATS=0, RAFT_IN_NORM=0 change how the InstanceNorm statistics are computed or applied, which
       only the feature network has (cnet: BatchNorm folded / none): prep, cnet and ctx bit-equal, the rest
       to the bounds;
     - RAFT_CONV_PAIR=0, RAFT_FUSE_CONVF1=0, RAFT_FUSE_CONVC1=0 change which kernel computes convf1 / convc1
       (and, for the pair, the tile a conv runs on): everything before the loop and the flow slot (one fp32
       subtraction in every lookup kernel) bit-equal, the rest to the bounds;
  c. plan.run() eager, then plan.replay() twice: flow_low, flow_up, the new h and coords bit-equal, which runs
     each fork / join layout under capture (one pass: a determinism check, not a race hunt).
"""
import argparse
import functools
import importlib.util
import os

import pytest
import torch

import plan_stage_oracle as PSO
from conftest import REPO
from test_gpu_parity import CONV_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda"

_spec = importlib.util.spec_from_file_location("plan_signature", os.path.join(REPO, "tools", "plan_signature.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

FULL_SHAPE = (2, 128, 136)
DEGENERATE_SHAPE = (2, 72, 136)
ALT_SHAPE = (1, 128, 136)

# convs in a multi-conv stage (the cap of its bound)
N_CONVS = {("fnet", False): 16, ("cnet", False): 16, ("update", False): 15,
           ("fnet", True): 22, ("cnet", True): 22, ("update", True): 9}
# worst measured relative error of the default plans over every case of test_default_plan_stages,
# test_both_mask_settings and test_train_mode_every_iteration_upsamples (MI355X; f16 / bf16: RAFT-full only)
MEASURED = {
    "fp32": {"fnet": 1.53e-6, "cnet": 5.61e-6, "update": 1.26e-6},
    "f16x3": {"fnet": 1.37e-6, "cnet": 4.44e-6, "update": 1.20e-6},
    "f16": {"fnet": 1.84e-3, "cnet": 5.49e-3, "update": 9.43e-4},
    "bf16": {"fnet": 1.41e-2, "cnet": 4.62e-2, "update": 6.75e-3},
}
# 4 x MEASURED, rounded up to one digit (the caps, N_CONVS x CONV_TOL, are 15 to 500 times larger)
MULTI = {
    "fp32": {"fnet": 7e-6, "cnet": 3e-5, "update": 6e-6},
    "f16x3": {"fnet": 6e-6, "cnet": 2e-5, "update": 5e-6},
    "f16": {"fnet": 8e-3, "cnet": 3e-2, "update": 4e-3},
    "bf16": {"fnet": 6e-2, "cnet": 2e-1, "update": 3e-2},
}
ELEMENTWISE_TOL = 1e-5
LOOKUP_TOL = {False: 1e-5, True: 1e-4}   # all-pairs, alternate

LOOKUPS = ("raft_corr_lookup", "raft_corr_lookup_convf1", "raft_corr_lookup_conv", "raft_alt_corr_lookup_levels_prec")
CORR_WRITERS = ("raft_corr_lookup", "raft_corr_lookup_convf1", "raft_alt_corr_lookup_levels_prec")

PRE_LOOP = ("prep", "fnet", "cnet", "ctx", "corr")
ALL_STAGES = PRE_LOOP + ("flow", "lookup", "update", "up")
BIT_EQUAL = {
    ("RAFT_CTX_SIDE", "0"): ALL_STAGES, ("RAFT_CTX_ORDER", "early"): ALL_STAGES, ("RAFT_CTX_ORDER", "mix"): ALL_STAGES,
    ("RAFT_FLOW_SIDE", "0"): ALL_STAGES, ("RAFT_MERGE_FUSED", "0"): ALL_STAGES,
    ("RAFT_EPI_STATS", "0"): ("prep", "cnet", "ctx"), ("RAFT_IN_NORM", "0"): ("prep", "cnet", "ctx"),
    ("RAFT_CONV_PAIR", "0"): PRE_LOOP + ("flow",), ("RAFT_FUSE_CONVF1", "0"): PRE_LOOP + ("flow",),
    ("RAFT_FUSE_CONVC1", "0"): PRE_LOOP + ("flow",),
}
assert set(BIT_EQUAL) == set(S.SWITCHES)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_optical_flow_amd import _lib
    _lib.load()


@pytest.fixture
def default_env(monkeypatch):
    for name in {n for n, _ in S.SWITCHES}:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


# ---------------------------------------------------------------------------- building and running plans


@functools.lru_cache(maxsize=None)
def _model(small):
    from raft_optical_flow_amd import RAFT
    from raft_optical_flow_amd.init import seeded_state_dict
    m = RAFT(argparse.Namespace(small=small, mixed_precision=False, alternate_corr=False))
    sd = seeded_state_dict(m, 0)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), PSO.params(sd)


@functools.lru_cache(maxsize=None)
def _packed(small, prec):
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import engine as E
    with torch.no_grad():
        return E.PackedRaft(_model(small)[0], DEV, _lib.PRECISIONS[prec])


def build_plan(small, prec, shape, iters=1, test_mode=True, alternate=False):
    from raft_optical_flow_amd import engine as E
    B, H, W = shape
    return E.RaftPlan(_packed(small, prec), B, H, W, iters, test_mode=test_mode, alternate=alternate, device=DEV)


def plan_text(plan):
    return S.signature(plan.launches, plan)[0]


def _nchw(t, off, c, b, h, w):
    """Columns [off, off + c) of a rows buffer [b*h*w, ld] -> NCHW on the CPU (fp32, the device's bits)."""
    return t[: b * h * w, off:off + c].reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous().cpu()


def _rows(x):
    b, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(b * h * w, c).contiguous()


@functools.lru_cache(maxsize=None)
def seeded_state(b, h, w, hd):
    """(coords, h): the grid + U(-6, 6) px flow with every 37th query sent 3 maps away, and a tanh state."""
    g = torch.Generator().manual_seed(1234 + b * 1000 + h * 31 + w)
    flow = torch.rand(b, 2, h, w, generator=g) * 12 - 6
    far = torch.zeros(b * h * w, dtype=torch.bool)
    far[5::37] = True
    far = far.view(b, 1, h, w)
    sign = torch.where(torch.rand(b, 2, h, w, generator=g) < 0.5, -1.0, 1.0)
    flow = torch.where(far, sign * 3.0 * max(h, w) + flow, flow)
    coords = PSO.coords_grid(b, h, w).float() + flow
    return coords, torch.tanh(torch.randn(b, hd, h, w, generator=g))


def execute(plan):
    """Run the plan in slices; -> {name: CPU tensor} of every compared buffer (the plan's own bits), the
    per-iteration ones under 'it<i>.<name>'."""
    from raft_optical_flow_amd import _lib
    from raft_optical_flow_amd import kernels as K
    from raft_optical_flow_amd.init import seeded_images
    pk, ub, L = plan.pk, plan.ub, plan.launches
    pu = pk.update
    B, H, W, h, w = plan.B, plan.H, plan.W, plan.h, plan.w
    hd, cd = pu.hdim, pu.cdim
    i1, i2 = seeded_images(B, H, W)
    plan.set_inputs(i1.to(DEV), i2.to(DEV))
    side = torch.cuda.Stream(device=DEV)
    snap = {"img1": i1, "img2": i2}
    torch.cuda.synchronize()
    K.run(L[:plan.loop_start], side)
    torch.cuda.synchronize()
    snap["prep"] = _nchw(plan.arena.bufs[0], 0, 3, 2 * B, H, W)
    snap["fmap"] = _nchw(plan.fmap, 0, pk.fdim, 2 * B, h, w)
    snap["h0"] = _nchw(ub.hx, 0, hd, B, h, w)
    snap["inp"] = _nchw(ub.hx, pu.inp_off, cd, B, h, w)
    for i, c in enumerate(ub.ctx):
        snap[f"ctx{i}"] = _nchw(c, 0, 3 * hd, B, h, w)
    if not plan.alternate:
        for lvl, (lh, lw) in enumerate(K.pyramid_dims(h, w, pk.levels)):
            out = torch.empty(B * h * w, lh, lw, device=DEV)
            _lib.call("raft_corr_pyramid_level", plan.pyramid.data_ptr(), B, h, w, pk.levels, lvl, out.data_ptr(),
                      K.stream_handle())
            snap[f"pyr{lvl}"] = out.cpu()
    else:
        for lvl, (t, lh, lw) in enumerate(plan.f2levels):
            snap[f"f2lvl{lvl}"] = _nchw(t, 0, pk.fdim, B, lh, lw)
    coords, hstate = seeded_state(B, h, w, hd)
    ub.coords.copy_(_rows(coords))
    ub.hx[:, :hd].copy_(_rows(hstate))
    ub.fh.fill_(-7.0)
    starts = [i for i in range(plan.loop_start, plan.loop_end)
              if isinstance(L[i], K.Launch) and L[i].name in LOOKUPS]
    assert len(starts) == plan.iters and starts[0] == plan.loop_start, starts
    for it, (a, b) in enumerate(zip(starts, starts[1:] + [plan.loop_end])):
        torch.cuda.synchronize()
        p = f"it{it}."
        snap[p + "coords_in"] = _nchw(ub.coords, 0, 2, B, h, w)
        snap[p + "hx_in"] = ub.hx.cpu()
        names = {l.name for l in L[a:b] if isinstance(l, K.Launch)}
        K.run(L[a:b], side)
        torch.cuda.synchronize()
        snap[p + "hx"] = ub.hx.cpu()
        if names & set(CORR_WRITERS):
            snap[p + "corr"] = _nchw(ub.corr, 0, ub.corr.shape[1], B, h, w)
        if ub.cor1 is not None:
            snap[p + "cor1"] = _nchw(ub.cor1, 0, ub.cor1.shape[1], B, h, w)
        snap[p + "flo1"] = _nchw(ub.flo1, 0, ub.flo1.shape[1], B, h, w)
        snap[p + "z"] = _nchw(ub.z, 0, hd, B, h, w)
        snap[p + "rh"] = _nchw(ub.rh, 0, hd, B, h, w)
        snap[p + "coords"] = _nchw(ub.coords, 0, 2, B, h, w)
        snap[p + "fh"] = ub.fh.cpu()
        if "raft_convex_upsample" in names:
            snap[p + "mask"] = _nchw(ub.mask, 0, 576, B, h, w)
        if names & {"raft_convex_upsample", "raft_upflow8"}:
            snap[p + "flow_up"] = plan.flow_up[-1 if plan.test_mode else it].cpu()
    K.run(L[plan.loop_end:], side)
    torch.cuda.synchronize()
    snap["flow_low"] = plan.flow_low.cpu()
    return snap


# ---------------------------------------------------------------------------- the stage checks


def rel_err(got, ref):
    """max |got - ref| / max(1, max|ref|) over the finite entries; NaN exactly where the reference has it."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), "NaN pattern differs from the oracle's"
    ok = ~nan
    if not bool(ok.any()):
        return 0.0
    scale = max(1.0, float(ref[ok].abs().max()))
    return float((got[ok] - ref[ok]).abs().max()) / scale


def stage_errors(snap, small, prec, alternate, iters):
    """{(stage, name): relative error} of every compared buffer, each against the oracle on the plan's own input
    to its stage; asserts the structural properties (untouched columns, sentinel) on the way."""
    p = _model(small)[1]
    hd, cd, r = PSO.dims(small)
    mc = 80 if small else 126
    B = snap["h0"].shape[0]
    h, w = snap["h0"].shape[-2:]
    E = {}
    d = lambda t: t.double()   # noqa: E731
    E["prep", "prep"] = rel_err(snap["prep"], torch.cat([PSO.prep(snap["img1"]), PSO.prep(snap["img2"])], 0))
    prep = d(snap["prep"])
    E["fnet", "fmap"] = rel_err(snap["fmap"], PSO.encoder(prep, p, "fnet", small))
    net, inp = PSO.context_split(PSO.encoder(prep[:B], p, "cnet", small), small)
    E["cnet", "h"] = rel_err(snap["h0"], net)
    E["cnet", "inp"] = rel_err(snap["inp"], inp)
    for i, ref in enumerate(PSO.gru_context(d(snap["inp"]), p, small)):
        E["ctx", f"ctx{i}"] = rel_err(snap[f"ctx{i}"], ref)
    f1, f2 = d(snap["fmap"][:B]), d(snap["fmap"][B:])
    if not alternate:
        for lvl, ref in enumerate(PSO.corr_pyramid(f1, f2)):
            E["corr", f"pyr{lvl}"] = rel_err(snap[f"pyr{lvl}"], ref[:, 0])
        pyr = [d(snap[f"pyr{lvl}"])[:, None] for lvl in range(4)]
        degenerate = min(pyr[-1].shape[-2:]) < 2
        look = lambda c: PSO.lookup(pyr, c, r)   # noqa: E731
    else:
        ref = f2
        for lvl in range(4):
            E["corr", f"f2lvl{lvl}"] = rel_err(snap[f"f2lvl{lvl}"], ref)
            ref = torch.nn.functional.avg_pool2d(ref, 2, stride=2) if lvl < 3 else ref
        degenerate = False
        look = lambda c: PSO.alt_lookup(f1, f2, c, r)   # noqa: E731
    grid = PSO.coords_grid(B, h, w)
    inp_off = hd + mc + 2 + (2 if small else 0)
    for it in range(iters):
        q = f"it{it}."
        t = (lambda s: s) if iters == 1 else (lambda s, it=it: f"{s}@{it}")
        hx_in, hx = snap[q + "hx_in"], snap[q + "hx"]
        # the pad and inp columns of HX are not the loop's to write
        assert torch.equal(hx[:, hd + mc + 2:].view(torch.int32), hx_in[:, hd + mc + 2:].view(torch.int32))
        assert bool((hx[:, hd + mc + 2:inp_off] == 0).all())
        coords_in = d(snap[q + "coords_in"])
        h_in = d(_nchw(hx_in, 0, hd, B, h, w))
        flow = coords_in - grid
        E["flow", t("flow")] = rel_err(_nchw(hx, hd + mc, 2, B, h, w), flow)
        corr = look(coords_in)
        if q + "corr" in snap:
            E["lookup", t("corr")] = rel_err(snap[q + "corr"], corr)
        me_in = d(snap[q + "corr"]) if q + "corr" in snap else corr
        # convf1 reads the flow slot the lookup launch wrote (bit-equal to coords - grid up to fp32 rounding)
        E["flo1", t("flo1")] = rel_err(snap[q + "flo1"], torch.relu(PSO.conv(
            d(_nchw(hx, hd + mc, 2, B, h, w)), p, "update_block.encoder.convf1", 1, 3)))
        if degenerate:
            continue   # a NaN level: the update step is undefined (module docstring)
        if not small:
            E["cor1", t("cor1")] = rel_err(snap[q + "cor1"], torch.relu(PSO.conv(
                me_in, p, "update_block.encoder.convc1", 1, 0)))
        net2, delta, mask, det = PSO.update_step(h_in, d(snap["inp"]), corr, flow, p, small, detail=True)
        E["update", t("motion")] = rel_err(_nchw(hx, hd, mc, B, h, w), det["motion"])
        E["update", t("z")] = rel_err(snap[q + "z"], det["z"])
        E["update", t("rh")] = rel_err(snap[q + "rh"], det["rh"])
        E["update", t("h")] = rel_err(_nchw(hx, 0, hd, B, h, w), net2)
        E["update", t("coords")] = rel_err(snap[q + "coords"], coords_in + delta)
        if small:
            pass
        elif q + "mask" in snap:
            E["update", t("mask")] = rel_err(snap[q + "mask"], mask)
        else:   # the fh1-only branch leaves the mask half of FH alone
            assert bool((snap[q + "fh"][:, 256:] == -7.0).all())
            assert bool((snap[q + "fh"][:, :256] != -7.0).all())
        if q + "flow_up" in snap:
            fl = d(snap[q + "coords"]) - grid
            up = PSO.upflow8(fl) if small else PSO.convex_upsample(fl, d(snap[q + "mask"]))
            E["up", t("flow_up")] = rel_err(snap[q + "flow_up"], up)
    if not degenerate:
        E["up", "flow_low"] = rel_err(snap["flow_low"], d(snap[f"it{iters - 1}.coords"]) - grid)
    return E


def bound(stage, small, prec, alternate):
    if stage in ("prep", "ctx", "cor1", "flo1"):
        return CONV_TOL[prec]
    if stage == "corr":
        return 1e-5
    if stage == "lookup":
        return LOOKUP_TOL[alternate]
    if stage in ("flow", "up"):
        return ELEMENTWISE_TOL
    b = MULTI[prec][stage]
    assert b <= N_CONVS[stage, small] * CONV_TOL[prec], (stage, b)
    return b


def hold(E, small, prec, alternate, label):
    print(f"\n== {label}")
    worst = {}
    for (stage, name), e in E.items():
        worst[stage] = max(worst.get(stage, 0.0), e)
        print(f"   {stage:7s} {name:12s} {e:.3g}   (bound {bound(stage, small, prec, alternate):.1g})")
    print("   STAGE_MAX " + label + " " + " ".join(f"{s}={e:.3g}" for s, e in worst.items()))
    bad = {k: (e, bound(k[0], small, prec, alternate)) for k, e in E.items()
           if not e <= bound(k[0], small, prec, alternate)}
    assert not bad, f"{label}: stages over their bounds (error, bound): {bad}"


def stage_of(key):
    """The stage a snapshot entry belongs to (for the bit-equality groups)."""
    k = key.split(".")[-1]
    if key in ("img1", "img2") or k in ("coords_in", "hx_in"):
        return None   # the test's own inputs
    if k == "prep":
        return "prep"
    if k == "fmap":
        return "fnet"
    if k in ("h0", "inp"):
        return "cnet"
    if k.startswith("ctx"):
        return "ctx"
    if k.startswith("pyr") or k.startswith("f2lvl"):
        return "corr"
    if k in ("corr", "cor1", "flo1"):
        return "lookup"
    if k in ("flow_up", "flow_low"):
        return "up"
    return "update"   # hx, z, rh, coords, fh, mask


def assert_bit_equal(snap, base, stages, small, label):
    hd, mc = (96, 80) if small else (128, 126)
    same = []
    for key, t in snap.items():
        st = stage_of(key)
        if key.endswith(".hx") and "flow" in stages:
            assert torch.equal(t[:, hd + mc:hd + mc + 2].view(torch.int32),
                               base[key][:, hd + mc:hd + mc + 2].view(torch.int32)), f"{label}: flow slot of {key}"
        if st is None or st not in stages or key not in base:
            continue   # (a buffer only one of the two plans writes, e.g. ub.corr, has no counterpart)
        assert torch.equal(t.view(torch.int32), base[key].view(torch.int32)), f"{label}: {key} is not bit-equal"
        same.append(key)
    print(f"   BIT_EQUAL {label}: {len(same)} buffers of stages {','.join(stages)}")


_DEFAULT = {}


def default_run(small, prec, shape, iters=1, test_mode=True, alternate=False):
    """(launch text, snapshot, stage errors) of the default plan of a configuration, computed once."""
    key = (small, prec, shape, iters, test_mode, alternate)
    if key not in _DEFAULT:
        plan = build_plan(small, prec, shape, iters, test_mode, alternate)
        try:
            text, snap = plan_text(plan), execute(plan)
        finally:
            plan.release()
        _DEFAULT[key] = (text, snap, stage_errors(snap, small, prec, alternate, iters))
    return _DEFAULT[key]


# ---------------------------------------------------------------------------- 2. the default plans, stage by stage


CASES = ([("full", prec, shape, False) for prec in ("fp32", "f16x3", "f16", "bf16")
          for shape in (DEGENERATE_SHAPE, FULL_SHAPE)]
         + [("small", prec, shape, False) for prec in ("fp32", "f16x3") for shape in (DEGENERATE_SHAPE, FULL_SHAPE)]
         + [("full", prec, ALT_SHAPE, True) for prec in ("fp32", "f16x3")])


def _id(c):
    net, prec, (b, hh, ww), alt = c
    return f"{net}-{'alt' if alt else 'allpairs'}-{prec}-b{b}x{hh}x{ww}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_default_plan_stages(default_env, case):
    net, prec, shape, alt = case
    small = net == "small"
    _, _, E = default_run(small, prec, shape, alternate=alt)
    hold(E, small, prec, alt, _id(case))


def test_both_mask_settings(default_env):
    """iters=2, test_mode: iteration 0 takes the fh1-only branch (no mask, no upsampling; the mask half of FH
    keeps its sentinel), iteration 1 the merged fh1 | mask GEMM.  Both update stages to the bounds."""
    _, snap, E = default_run(False, "f16x3", FULL_SHAPE, iters=2)
    assert "it0.mask" not in snap and "it0.flow_up" not in snap and "it1.mask" in snap and "it1.flow_up" in snap
    assert ("update", "h@0") in E and ("update", "mask@1") in E and ("update", "mask@0") not in E
    hold(E, False, "f16x3", False, "full-allpairs-f16x3-iters2-test")


@pytest.mark.parametrize("net", ["full", "small"])
def test_train_mode_every_iteration_upsamples(default_env, net):
    """test_mode=False, iters=2: both flow_up entries (and both masks) against the oracle."""
    small = net == "small"
    _, snap, E = default_run(small, "f16x3", FULL_SHAPE, iters=2, test_mode=False)
    assert ("up", "flow_up@0") in E and ("up", "flow_up@1") in E
    assert not torch.equal(snap["it0.flow_up"], snap["it1.flow_up"])
    hold(E, small, "f16x3", False, f"{net}-allpairs-f16x3-iters2-train")


# ---------------------------------------------------------------------------- 3. every plan-time switch, run


SWITCH_CONFIGS = [("full", "f16x3"), ("small", "f16x3"), ("full", "fp32")]


def _switched(monkeypatch, env, small, prec, label, base_env=()):
    """Build the plan under `env` (on top of base_env), compare its text with the default's (built under
    base_env alone); -> (plan or None where the texts are equal, the default's (text, snap, errors))."""
    for k, v in base_env:
        monkeypatch.setenv(k, v)
    if base_env:
        plan = build_plan(small, prec, FULL_SHAPE)
        try:
            text, snap = plan_text(plan), execute(plan)
        finally:
            plan.release()
        base = (text, snap, None)
    else:
        base = default_run(small, prec, FULL_SHAPE)
    for k, v in env:
        monkeypatch.setenv(k, v)
    plan = build_plan(small, prec, FULL_SHAPE)
    if plan_text(plan) == base[0]:
        plan.release()
        print(f"\n   SWITCH {label}: plan EQUAL to the default's")
        return None, base
    print(f"\n   SWITCH {label}: plan differs from the default's")
    return plan, base


def _eager_and_replays(plan, label):
    from raft_optical_flow_amd.init import seeded_images
    pu, ub = plan.pk.update, plan.ub
    i1, i2 = seeded_images(plan.B, plan.H, plan.W)
    plan.set_inputs(i1.to(DEV), i2.to(DEV))

    def outs():
        torch.cuda.synchronize()
        return [plan.flow_low.cpu(), plan.flow_up[0].cpu(), ub.hx[:, :pu.hdim].cpu(), ub.coords.cpu()]

    plan.run()
    eager = outs()
    assert all(bool(torch.isfinite(t).all()) for t in eager)
    for i in range(2):
        plan.replay()
        for name, a, b in zip(("flow_low", "flow_up", "h", "coords"), eager, outs()):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{label}: replay {i}: {name} != eager"


# the switches that can act on each network / precision (the others must leave the launch list alone)
def _acts(name, small, prec):
    if name in ("RAFT_CONV_PAIR", "RAFT_FUSE_CONVF1"):
        return not small
    if name == "RAFT_FUSE_CONVC1":
        return not small and prec != "fp32"
    if name == "RAFT_FLOW_SIDE":
        return small
    if name == "RAFT_IN_NORM":   # raft_conv2d_in_norm_ok: the halo kernel's 3x3 convs, which fp32 convs do not run on
        return prec != "fp32"
    return True


@pytest.mark.parametrize("config", SWITCH_CONFIGS, ids=lambda c: "-".join(c))
@pytest.mark.parametrize("switch", S.SWITCHES, ids=lambda s: "=".join(s))
def test_switched_plan(default_env, switch, config):
    net, prec = config
    small = net == "small"
    label = f"{net}-{prec}-{switch[0]}={switch[1]}"
    plan, (_, base_snap, _) = _switched(default_env, [switch], small, prec, label)
    assert (plan is not None) == _acts(switch[0], small, prec), f"{label}: the switch did not take effect as expected"
    if plan is None:
        return   # the same launch list as the default plan, which test_default_plan_stages runs
    try:
        snap = execute(plan)
        hold(stage_errors(snap, small, prec, False, 1), small, prec, False, label)          # a
        assert_bit_equal(snap, base_snap, BIT_EQUAL[switch], small, label)                   # b
        _eager_and_replays(plan, label)                                                      # c
    finally:
        plan.release()


def test_flow_side_on_full_without_the_pair(default_env):
    """RAFT_FLOW_SIDE acts on RAFT-full only with RAFT_CONV_PAIR=0: the flow branch on the side stream or not,
    every buffer bit-equal."""
    label = "full-f16x3-RAFT_CONV_PAIR=0-RAFT_FLOW_SIDE=0"
    plan, (_, base_snap, _) = _switched(default_env, [("RAFT_FLOW_SIDE", "0")], False, "f16x3", label,
                                        base_env=[("RAFT_CONV_PAIR", "0")])
    assert plan is not None, "RAFT_FLOW_SIDE=0 did not change the RAFT_CONV_PAIR=0 plan"
    try:
        snap = execute(plan)
        hold(stage_errors(snap, False, "f16x3", False, 1), False, "f16x3", False, label)
        assert_bit_equal(snap, base_snap, ALL_STAGES, False, label)
        _eager_and_replays(plan, label)
    finally:
        plan.release()


@pytest.mark.parametrize("config", SWITCH_CONFIGS, ids=lambda c: "-".join(c))
def test_default_plan_eager_and_replays(default_env, config):
    net, prec = config
    plan = build_plan(net == "small", prec, FULL_SHAPE)
    try:
        _eager_and_replays(plan, f"{net}-{prec}-default")
    finally:
        plan.release()
