"""RAFT — drop-in for core/raft.py (inference on MI355X).

`RAFT(args)` builds the same module tree as the reference (`core/raft.py:37-78`:
fnet / cnet / update_block with identical parameter names, so reference
checkpoints — including DataParallel `module.` ones via the caller's wrapper —
load unchanged) and `forward(image1, image2, iters=12, flow_init=None,
upsample=True, test_mode=False)` keeps the reference's contract
(`core/raft.py:145-251`): NCHW float images in [0, 255] with H, W multiples of
8 on the model's device; returns `(flow_low, flow_up)` in test_mode, else the
list of `iters` upsampled flows.

Execution is an engine.RaftPlan: every kernel is hand-written HIP (encoders,
correlation build + pyramid, window lookup, update block, upsampling), the
launch list is fixed per input shape.  The first forward of a shape runs the
launch list eagerly; from the second one on the whole forward (including the
32-iteration loop) is captured once and replays as one hipGraph, so unchanged
callers (demo.py, evaluate.py) get graph replay without setting anything
(`args.hip_graph = False`, `model.hip_graph = False` or RAFT_HIP_GRAPH=0 keep
eager launches).  Plans live in a small LRU (RAFT_MAX_PLANS, default 2): a
plan pins its correlation pyramid (275 MB at 440x1024) and buffers, so
evaluate.py's many KITTI sizes do not accumulate device memory.

Video: `model.stream(iters, warm_start, pad_mode)` returns a FlowStream (below): `push(frame)`
gives the flow of (previous frame, this frame) and encodes every frame once (engine.StreamPlan).
With `bidirectional=True` it also gives the flow of (this frame, previous frame) and the
forward-backward occlusion masks of the two, still at one fnet and one cnet pass per frame
(engine.BidiStreamPlan).

f16x3 range guard: the default fp32-accurate split arithmetic holds only while every
conv input stays below 65504 in magnitude (include/raft_hip.h).  The convs and lookups
whose outputs feed split convs raise a device flag above 2^15.  `model.range_guard`
(env RAFT_RANGE_GUARD) chooses what happens then:
  "fallback" (default)  forward() waits for its flag (one host sync per forward) and, when it
                        is raised, warns and returns the result of a re-run on exact f32 MFMA:
                        what forward() returns is always the exact-range result ("sync" is
                        the same mode);
  "deferred"            opt-in, for callers that queue forwards back to back: the flag is
                        copied to pinned host memory behind the forward and read once that
                        copy has completed (at a later forward() call, at
                        model.check_range_guard(), which waits, or at interpreter exit).  A
                        raised flag warns and re-runs that forward on exact f32 MFMA INTO the
                        tensors it returned; values read from them before that point were
                        the inexact ones (the warning says so);
  "raise"               as "fallback", but raises FloatingPointError;
  "off"                 no device checks at all.
"""
from __future__ import annotations

import atexit
import os
import warnings
import weakref
from collections import OrderedDict, deque, namedtuple

import threading

import torch
import torch.nn as nn

from . import kernels as K
from .engine import BidiStreamPlan, PackedRaft, RaftPlan, StreamPlan, frame_layout, frame_pad
from .extractor import BasicEncoder, SmallEncoder
from .update import BasicUpdateBlock, SmallUpdateBlock
from .utils.flow_viz import check_viz_options, flow_to_rgb
from .utils.utils import check_fb_params, check_warp_option, coords_grid, fb_consistency, warp_frame

# module attribute kept for API parity with core/raft.py:11-22 (callers monkeypatch it);
# the HIP path never autocasts: its arithmetic is RAFT.conv_precision
autocast = torch.amp.autocast

# default conv arithmetic of an fp32 model (include/raft_hip.h, RAFT_PREC_*):
# "f16x3" = fp32-accurate split-f16 MFMA, "fp32" = f32 MFMA
DEFAULT_PRECISION = "f16x3"

_CACHE_LOCK = threading.Lock()  # creation of per-device cache entries (DataParallel threads)


class RAFT(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        if args.small:
            self.hidden_dim = hdim = 96
            self.context_dim = cdim = 64
            args.corr_levels = 4
            args.corr_radius = 3
        else:
            self.hidden_dim = hdim = 128
            self.context_dim = cdim = 128
            args.corr_levels = 4
            args.corr_radius = 4
        if "dropout" not in self.args:
            self.args.dropout = 0
        if "alternate_corr" not in self.args:
            self.args.alternate_corr = False
        if "mixed_precision" not in self.args:
            self.args.mixed_precision = False
        if args.small:
            self.fnet = SmallEncoder(output_dim=128, norm_fn="instance", dropout=args.dropout)
            self.cnet = SmallEncoder(output_dim=hdim + cdim, norm_fn="none", dropout=args.dropout)
            self.update_block = SmallUpdateBlock(self.args, hidden_dim=hdim)
        else:
            self.fnet = BasicEncoder(output_dim=256, norm_fn="instance", dropout=args.dropout)
            self.cnet = BasicEncoder(output_dim=hdim + cdim, norm_fn="batch", dropout=args.dropout)
            self.update_block = BasicUpdateBlock(self.args, hidden_dim=hdim)
        # execution state (not part of state_dict)
        self.hip_graph = bool(getattr(args, "hip_graph", os.environ.get("RAFT_HIP_GRAPH", "1") != "0"))
        self.max_plans = int(os.environ.get("RAFT_MAX_PLANS", "2"))
        self.range_guard = os.environ.get("RAFT_RANGE_GUARD", "fallback")
        # conv arithmetic: "fp32" | "f16x3" | "f16"; args.mixed_precision (the
        # reference's fp16 autocast, core/raft.py:156) selects "f16"
        self.conv_precision = getattr(args, "conv_precision", None)
        # packed weights and plans per device: {str(device): {"packed": {precision: (weights key,
        # PackedRaft)}, "plans": OrderedDict}}; nn.DataParallel replicas share their source's
        # (_replicate_for_data_parallel), each replica touching only its own device's entry
        self._caches = {}
        self._pending = deque()     # deferred range-guard checks ("deferred"), oldest first

    def _replicate_for_data_parallel(self):
        """nn.DataParallel (the reference's multi-GPU API, train.py:172, evaluate.py:179) re-replicates
        the module on every forward by shallow-copying __dict__.  A replica keeps the per-device caches
        of its SOURCE module (so packing and graph capture happen once per device, not per forward;
        the weights key is the source's, whose values every replica copies) and a range-guard queue of
        its own; replicas on different devices never touch the same cache entry."""
        replica = super()._replicate_for_data_parallel()
        replica.__dict__["_dp_source"] = self.__dict__.get("_dp_source") or self
        replica.__dict__["_pending"] = deque()
        return replica

    def _source(self):
        return self.__dict__.get("_dp_source") or self

    def _dev_cache(self, device):
        caches = self._source().__dict__["_caches"]
        d = str(torch.device(device))
        c = caches.get(d)
        if c is None:
            with _CACHE_LOCK:
                c = caches.setdefault(d, {"packed": {}, "plans": OrderedDict()})
        return c

    @property
    def _plans(self):
        """The plans of the device this module's parameters are on (inspection / tests)."""
        return self._dev_cache(next(self.parameters()).device)["plans"]

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    def initialize_flow(self, img):
        n, c, h, w = img.shape
        coords0 = coords_grid(n, h // 8, w // 8, device=img.device)
        coords1 = coords_grid(n, h // 8, w // 8, device=img.device)
        return coords0, coords1

    def upsample_flow(self, flow, mask):
        """Convex upsampling (core/raft.py:112-142) on the HIP kernel; flow [N,2,H,W], mask [N,576,H,W]."""
        from . import _lib
        K.require_device(flow, mask)
        n, _, h, w = flow.shape
        coords = coords_grid(n, h, w, device=flow.device) + flow
        crow = K.nchw_to_rows(coords.contiguous())
        mrow = K.nchw_to_rows(mask.contiguous())
        out = torch.empty(n, 2, 8 * h, 8 * w, device=flow.device)
        _lib.call("raft_convex_upsample", crow.data_ptr(), mrow.data_ptr(), 576, out.data_ptr(), n, h, w,
                  K.stream_handle())
        return out

    # -- weights / plans ---------------------------------------------------
    def _weights_key(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters()) + tuple(
            (b.data_ptr(), b._version) for b in self.buffers())

    def resolved_precision(self) -> str:
        from . import _lib
        prec = self.conv_precision or ("f16" if self.args.mixed_precision else DEFAULT_PRECISION)
        if prec not in _lib.PRECISIONS:
            raise ValueError(f"conv_precision must be one of {sorted(_lib.PRECISIONS)}, got {prec!r}")
        return prec

    def packed(self, device, prec=None):
        from . import _lib
        prec = prec or self.resolved_precision()
        # (a DataParallel replica's parameters are this forward's copies of its source's: the
        # source's key names the values)
        key = (self._source()._weights_key(), str(device))
        cache = self._dev_cache(device)
        packs = cache["packed"]
        got = packs.get(prec)
        if got is None or got[0] != key:
            if got is not None or any(k != key for k, _ in packs.values()):
                # new weights: every packed form and plan of this device is stale
                packs.clear()
                self._release(cache["plans"])
            with torch.no_grad():
                got = (key, PackedRaft(self, device, _lib.PRECISIONS[prec]))
            packs[prec] = got
        return got[1]

    def _plan_key(self, batch, height, width, iters, test_mode, flow_init, prec):
        # the stream layout knobs are read when a plan is built, so they are part of its key
        # (every RAFT_* variable engine.py reads: tests/test_plan_key_host.py holds the two in step)
        knobs = (os.environ.get("RAFT_CTX_SIDE", "1"), os.environ.get("RAFT_FLOW_SIDE", "1"),
                 os.environ.get("RAFT_CONV_PAIR", "1"), os.environ.get("RAFT_FUSE_CONVF1", "1"),
                 os.environ.get("RAFT_FUSE_CONVC1", "1"), os.environ.get("RAFT_EPI_STATS", "1"),
                 os.environ.get("RAFT_IN_NORM", "1"), os.environ.get("RAFT_MERGE_FUSED", "1"),
                 os.environ.get("RAFT_CTX_ORDER", "late"))
        guard = self.range_guard != "off"  # "off": no device-side checks either
        return (batch, height, width, iters, bool(test_mode), bool(self.args.alternate_corr), bool(flow_init), prec,
                knobs, guard)

    def _cached_plan(self, batch, height, width, iters, test_mode, flow_init, device):
        """The cached plan of this call and the weights key its packed weights were made from, WITHOUT
        checking that key against the parameters (forward() checks it while the plan runs); None when
        the call has no plan yet."""
        prec = self.resolved_precision()
        cache = self._dev_cache(device)
        got = cache["packed"].get(prec)
        if got is None:
            return None
        pl = cache["plans"].get(self._plan_key(batch, height, width, iters, test_mode, flow_init, prec))
        if pl is None or pl.pk is not got[1]:
            return None
        return pl, got[0]

    def plan(self, batch, height, width, iters, test_mode=True, flow_init=False, device=None, prec=None):
        device = device or next(self.parameters()).device
        prec = prec or self.resolved_precision()
        pk = self.packed(device, prec)
        key = self._plan_key(batch, height, width, iters, test_mode, flow_init, prec)
        plans = self._dev_cache(device)["plans"]
        pl = plans.get(key)
        if pl is None:
            while len(plans) >= max(1, self.max_plans):
                plans.popitem(last=False)[1].release()
            pl = RaftPlan(pk, batch, height, width, iters, test_mode=test_mode,
                          alternate=bool(self.args.alternate_corr), flow_init=flow_init, device=device,
                          range_guard=key[-1])
            plans[key] = pl
        else:
            plans.move_to_end(key)
        return pl

    @staticmethod
    def _release(plans, keep=None):
        for k in list(plans):
            if plans[k] is not keep:
                plans.pop(k).release()

    def release_plans(self, keep=None):
        """Free the cached plans' device memory and graphs (all but `keep`), on every device."""
        for cache in list(self._source().__dict__["_caches"].values()):
            self._release(cache["plans"], keep)

    # -- deferred range guard ------------------------------------------------
    _MAX_PENDING = 2  # forwards whose flag may be unread: the third waits for the oldest

    def check_range_guard(self, block=True):
        """Resolve the deferred range-guard checks of earlier forwards ("fallback" mode): with
        block=True wait for all of them, else only read those whose flag copy has completed.
        A raised flag warns and re-runs that forward on exact f32 MFMA into its output tensors."""
        while self._pending:
            rec = self._pending[0]
            if not block and len(self._pending) <= self._MAX_PENDING and not rec["event"].query():
                break
            rec["event"].synchronize()
            self._pending.popleft()
            if int(rec["flag"].item()):
                self._guard_fallback(rec)

    def _guard_fallback(self, rec):
        msg = ("f16x3 range guard (deferred): an activation of an earlier forward exceeded 2^15 in "
               "magnitude, outside the exact range of the split-f16 conv arithmetic; values read from its "
               "outputs before this point were inexact")
        ins = [x for x in rec["inputs"] if x is not None]
        if any(x._version != v for x, v in zip(ins, rec["versions"])):
            warnings.warn(msg + "; the inputs of that forward were modified in place since, so its outputs "
                          "cannot be recomputed and stay inexact", RuntimeWarning)
            return
        warnings.warn(msg + "; that forward was re-run with exact f32 MFMA convs into its output tensors",
                      RuntimeWarning)
        i1, i2, fi = rec["inputs"]
        exact = self.forward(i1, i2, rec["iters"], fi, True, rec["test_mode"], _prec="fp32")
        for o, n in zip(rec["outputs"], exact):   # (low, up) or the list of upsampled flows
            o.copy_(n)

    def forward(self, image1, image2, iters=12, flow_init=None, upsample=True, test_mode=False, _prec=None):
        if image1.is_cuda and image1.device != torch.device("cuda", torch.cuda.current_device()):
            # launches go to the current device's stream: make the images' device current
            with torch.cuda.device(image1.device):
                return self.forward(image1, image2, iters, flow_init, upsample, test_mode, _prec)
        if self.training:
            raise NotImplementedError(_TRAINING_MSG)
        K.require_device(image1, image2, flow_init)
        if image1.shape != image2.shape or image1.dim() != 4 or image1.shape[1] != 3:
            raise ValueError(f"images must both be [N, 3, H, W], got {tuple(image1.shape)} / {tuple(image2.shape)}")
        if self._pending and _prec is None:
            self.check_range_guard(block=False)  # earlier forwards whose flags have landed
        b, _, H, W = image1.shape
        mode = self.range_guard
        if mode == "deferred" and self.__dict__.get("_is_replica", False):
            mode = "fallback"  # a DataParallel replica lives for one forward: nothing can be deferred
        # Steady state (same weights, shape and settings as a cached plan): the plan is enqueued first and
        # the weights key -- a walk over every parameter, ~0.2-0.7 ms of host time -- is checked while it
        # runs, instead of leaving the GPU idle between back-to-back forwards.  Changed weights (in-place
        # edits, load_state_dict, .to()) are caught by that check: the stale run is discarded and the
        # forward re-run on freshly packed weights, so the result is the one the reference would return.
        cached = None
        if _prec is None and self.hip_graph and not self.__dict__.get("_is_replica", False):
            cached = self._cached_plan(b, H, W, iters, test_mode, flow_init is not None, image1.device)
        while True:
            if cached is not None:
                pl, wkey = cached
            else:
                pl = self.plan(b, H, W, iters, test_mode, flow_init is not None, image1.device, prec=_prec)
            pl.set_inputs(image1, image2, flow_init)
            guard = pl.guarded and mode != "off"
            if guard:
                pl.range_flag.zero_()
            if self.hip_graph and (pl.graph is not None or pl.runs > 0):
                pl.replay()
            else:
                pl.run()
            if cached is None or (self._source()._weights_key(), str(image1.device)) == wkey:
                break
            # the weights changed since the plan was packed: let the stale run finish before its plan
            # can be released, then take the checked path
            torch.cuda.current_stream().synchronize()
            cached = None
        outs = pl.outputs(clone=True)
        if not guard:
            return outs
        if mode != "deferred":  # "fallback" (default), "sync", "raise"
            if int(pl.range_flag.item()):
                msg = ("f16x3 range guard: an activation exceeded 2^15 in magnitude, outside the exact range "
                       "of the split-f16 conv arithmetic")
                if mode == "raise":
                    raise FloatingPointError(msg)
                warnings.warn(msg + "; this forward was re-run with exact f32 MFMA convs", RuntimeWarning)
                return self.forward(image1, image2, iters, flow_init, upsample, test_mode, _prec="fp32")
            return outs
        # "deferred": the flag travels to pinned host memory behind the forward; read later
        if not self._pending:
            _register_exit_check(self)
        flag = torch.empty(1, dtype=torch.int32, pin_memory=True)
        flag.copy_(pl.range_flag, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ins = (image1, image2, flow_init)
        self._pending.append({"event": ev, "flag": flag, "inputs": ins, "outputs": outs, "iters": iters,
                              "test_mode": test_mode,
                              "versions": [x._version for x in ins if x is not None]})
        if len(self._pending) > self._MAX_PENDING:
            self.check_range_guard(block=False)
        return outs


    def stream(self, iters=12, warm_start=False, pad_mode="sintel", bidirectional=False, fb_alpha=0.01, fb_beta=0.5,
               visualize=None, viz_rad_max=None, viz_stack=False, warp=None):
        """A FlowStream over consecutive video frames: `push(frame)` returns (flow_low, flow_up) of
        (previous frame, this frame), and every frame passes through the feature network once.
        bidirectional=True: push returns a BidirectionalFlow (both directions, their occlusion masks and
        forward-backward residuals; fb_alpha / fb_beta are the check's constants, utils.fb_consistency).
        visualize="rgb" / "bgr": the step also colours flow_up on the device (utils.flow_viz.flow_to_rgb) and
        push returns a FlowViz (or a BidirectionalFlowViz); viz_rad_max fixes the colour scale for the whole
        video, viz_stack puts the pair's first frame above the colours as demo.py does.
        warp="zeros" / "border": the step also warps the current frame back onto the previous one by flow_up
        (utils.warp_frame; bidirectional: both frames, each by its direction's flow) and push returns a FlowWarp
        (or the matching tuple below) with `warped, valid` appended."""
        return FlowStream(self, iters, warm_start, pad_mode, bidirectional, fb_alpha, fb_beta, visualize, viz_rad_max,
                          viz_stack, warp)


_TRAINING_MSG = ("raft_optical_flow_amd.RAFT is an inference path: call model.eval() "
                 "(training / BatchNorm batch statistics are out of scope)")


BidirectionalFlow = namedtuple("BidirectionalFlow", ["low_fw", "up_fw", "low_bw", "up_bw", "occ_fw", "occ_bw",
                                                     "err_fw", "err_bw"])
BidirectionalFlow.__doc__ = """What FlowStream.push returns with bidirectional=True.

  low_fw, up_fw    [B,2,h,w], [B,2,H,W] float32  flow previous -> current frame (the one-directional result)
  low_bw, up_bw    same                          flow current -> previous frame
  occ_fw, occ_bw   [B,1,H,W] bool                True where the direction's flow fails the forward-backward check
  err_fw, err_bw   [B,1,H,W] float32             the squared residual the masks were thresholded from
(utils.fb_consistency(up_fw, up_bw, fb_alpha, fb_beta) of the same step, computed inside the step.)"""


FlowViz = namedtuple("FlowViz", ["flow_low", "flow_up", "rgb"])
FlowViz.__doc__ = """What FlowStream.push returns with visualize set: (flow_low, flow_up) as without it, and
rgb uint8 [B,H,W,3] ([B,2H,W,3] with viz_stack; B, G, R order with visualize="bgr"):
utils.flow_viz.flow_to_rgb(flow_up, viz_rad_max, frame=the previous frame) of the same step, computed inside
the step."""

BidirectionalFlowViz = namedtuple("BidirectionalFlowViz", BidirectionalFlow._fields + ("rgb_fw", "rgb_bw"))
BidirectionalFlowViz.__doc__ = """BidirectionalFlow's fields, then rgb_fw and rgb_bw: the colour images of up_fw and
up_bw (FlowViz.rgb).  Each is normalised by its own maximum unless viz_rad_max is given; with viz_stack rgb_fw
lies under the previous frame and rgb_bw under the current one (each direction's image1)."""


FlowWarp = namedtuple("FlowWarp", ["flow_low", "flow_up", "warped", "valid"])
FlowWarp.__doc__ = """What FlowStream.push returns with warp set: (flow_low, flow_up) as without it, then
  warped  the current frame sampled at x + flow_up(x): aligned with the previous frame; in the pushed frame's own
          layout (float32 [B,3,H,W], or uint8 [B,H,W,3] for uint8 frames)
  valid   bool [B,1,H,W]: x + flow_up(x) lies in the frame (a target in the padding is outside)
utils.warp_frame(current frame, flow_up, padding=warp) of the same step, computed inside the step."""

FlowVizWarp = namedtuple("FlowVizWarp", FlowViz._fields + ("warped", "valid"))
FlowVizWarp.__doc__ = """FlowViz's fields, then FlowWarp's warped and valid (visualize and warp both set)."""

_BIDI_WARP = ("warped_fw", "warped_bw", "valid_fw", "valid_bw")
BidirectionalFlowWarp = namedtuple("BidirectionalFlowWarp", BidirectionalFlow._fields + _BIDI_WARP)
BidirectionalFlowWarp.__doc__ = """BidirectionalFlow's fields, then warped_fw: the current frame warped by up_fw
(aligned with the previous frame), warped_bw: the previous frame warped by up_bw (aligned with the current one),
and their in-frame masks valid_fw, valid_bw (FlowWarp.warped / valid)."""

BidirectionalFlowVizWarp = namedtuple("BidirectionalFlowVizWarp", BidirectionalFlowViz._fields + _BIDI_WARP)
BidirectionalFlowVizWarp.__doc__ = """BidirectionalFlowViz's fields, then BidirectionalFlowWarp's four."""


class FlowStream:
    """Optical flow over a video, one frame per call (RAFT.stream).

      s = model.stream(iters=12, warm_start=False, pad_mode="sintel")
      out = s.push(frame)   # None for the first frame after reset(); then (flow_low, flow_up) of
                            # (previous frame, this frame)
      s.reset()             # sequence boundary
      s.close()             # releases graph and buffers (also at garbage collection / `with` exit)
      s.last_flow_init      # [B,2,h,w] the last step started from (None when warm_start=False)

    visualize="rgb" / "bgr": push returns a FlowViz (flow_low, flow_up, rgb) instead: rgb is the colour-wheel image of
    flow_up, uint8 [B,H,W,3], coloured inside the step (utils.flow_viz.flow_to_rgb of the same flow, bit for bit).
    viz_rad_max=None normalises every image by its own maximum, as the reference's flow_to_image does; a positive
    number fixes the scale so that colours do not flicker from frame to frame.  viz_stack=True puts the pair's
    first frame above the colours ([B,2H,W,3], demo.py's layout).

    warp="zeros" / "border": push returns a FlowWarp (flow_low, flow_up, warped, valid): the current frame
    warped back onto the previous one by flow_up inside the step (utils.warp_frame of the same flow, bit for
    bit), in the pushed frame's layout and dtype, and the mask of the targets that lie in the frame.  With
    visualize the two fields follow rgb (FlowVizWarp); bidirectional streams append warped_fw, warped_bw,
    valid_fw, valid_bw (BidirectionalFlowWarp / BidirectionalFlowVizWarp).

    bidirectional=True: push returns a BidirectionalFlow instead (both flows, occlusion masks, residuals);
    it equals model(cat[pad(prev), pad(cur)], cat[pad(cur), pad(prev)], iters, flow_init=s.last_flow_init,
    test_mode=True) + unpad, with last_flow_init [2B,2,h,w], the forward half first; a warm start begins each
    direction from forward_interpolate of its own direction's flow of the step before.  The masks are
    utils.fb_consistency of the unpadded flows: a target in the padding is outside the frame.

    A frame is float32 [B,3,H,W] in 0..255 or uint8 [B,H,W,3], of any size (it is replicate-padded as
    InputPadder(pad_mode) does; flow_up comes back at the frame's own size, flow_low at 1/8 of the
    padded one); B > 1 is B independent streams in lockstep.  The first push fixes shape and dtype.
    What push returns equals model(pad(prev), pad(cur), iters, flow_init=s.last_flow_init,
    test_mode=True) + unpad.  With warm_start every pair starts from forward_interpolate of the
    pair before (evaluate.py:37-41), computed on the device inside the step.

    The stream owns its engine.StreamPlan: it is not in the model's plan cache (max_plans,
    release_plans() do not see it).  The range guard works as in forward(); "deferred" is treated
    as "fallback", because the next step consumes this step's flow_low."""

    def __init__(self, model, iters=12, warm_start=False, pad_mode="sintel", bidirectional=False, fb_alpha=0.01,
                 fb_beta=0.5, visualize=None, viz_rad_max=None, viz_stack=False, warp=None):
        self.visualize, self.viz_rad_max = check_viz_options(visualize, viz_rad_max)
        self.warp = check_warp_option(warp)
        if not isinstance(viz_stack, bool):
            raise TypeError(f"viz_stack must be a bool, got {type(viz_stack).__name__}")
        self.viz_stack = viz_stack
        if model.training:
            raise NotImplementedError(_TRAINING_MSG)
        if model.__dict__.get("_is_replica", False) or model.__dict__.get("_dp_source") is not None:
            raise RuntimeError("RAFT.stream(): a DataParallel replica lives for one forward; open the stream on "
                               "the source module")
        if int(iters) < 1:
            raise ValueError(f"iters must be >= 1, got {iters}")
        if not isinstance(bidirectional, bool):
            raise TypeError(f"bidirectional must be a bool, got {type(bidirectional).__name__}")
        self.bidirectional = bidirectional
        self.fb_alpha, self.fb_beta = check_fb_params(fb_alpha, fb_beta)
        self.model, self.iters, self.warm_start = model, int(iters), bool(warm_start)
        self.pad_mode = pad_mode
        self.centred = pad_mode == "sintel"   # any other mode: rows at the bottom, as InputPadder
        self.plan = None
        self.layout = None          # (dtype tag, B, H, W) of the first frame
        self.shape = None
        self.primed = False
        self.closed = False
        self.last_flow_init = None
        self._wkey = None
        self._prev_low = None       # flow_low of the step before (warm start; survives a stale step)
        self._inexact_prev = False  # the previous frame's feature map came from a step the guard flagged

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown: the GPU context may already be gone)
            pass

    def pad(self, height, width):
        """[left, right, top, bottom] this stream pads a height x width frame by (InputPadder._pad)."""
        return frame_pad(height, width, self.centred)

    def reset(self):
        """Sequence boundary: the next frame primes the stream and returns None."""
        self.primed = False
        self.last_flow_init = None
        self._prev_low = None
        self._inexact_prev = False
        if self.plan is not None:
            with torch.cuda.device(self.plan.device):
                self.plan.reset()

    def close(self):
        if self.closed:
            return
        self.closed = True
        if self.plan is not None:
            self.plan.release()
            self.plan = None

    def _build(self, device):
        m = self.model
        prec = m.resolved_precision()
        pk = m.packed(device, prec)
        self._wkey = m._weights_key()
        tag, b, h, w = self.layout
        kw = dict(dtype_tag=tag, centred=self.centred, alternate=bool(m.args.alternate_corr),
                  warm_start=self.warm_start, device=device, range_guard=m.range_guard != "off",
                  visualize=self.visualize, viz_rad_max=self.viz_rad_max, viz_stack=self.viz_stack,
                  warp=self.warp)
        if self.bidirectional:
            return BidiStreamPlan(pk, b, h, w, self.iters, fb_alpha=self.fb_alpha, fb_beta=self.fb_beta, **kw)
        return StreamPlan(pk, b, h, w, self.iters, **kw)

    def _step(self, frame):
        pl = self.plan
        pl.frame_in.copy_(frame)
        if pl.guarded:
            pl.range_flag.zero_()
        if self.model.hip_graph and (pl.graph is not None or pl.runs > 0):
            pl.replay()
        else:
            pl.run()

    def push(self, frame):
        if self.closed:
            raise RuntimeError("FlowStream.push() after close()")
        m = self.model
        if m.training:
            raise NotImplementedError(_TRAINING_MSG)
        layout = frame_layout(frame)
        device = next(m.parameters()).device
        if frame.is_cuda and frame.device != device:
            raise RuntimeError(f"the frame is on {frame.device}, the model on {device}")
        if device.type != "cuda":
            raise RuntimeError(f"raft_optical_flow_amd runs on a ROCm GPU only: the model is on {device}")
        if self.layout is None:
            self.layout, self.shape = layout, (frame.dtype, tuple(frame.shape))
        elif (frame.dtype, tuple(frame.shape)) != self.shape:
            raise ValueError(f"this stream was opened with {self.shape[0]} frames of shape {self.shape[1]}, got "
                             f"{frame.dtype} {tuple(frame.shape)} (open another stream for another shape)")
        with torch.cuda.device(device):
            return self._push(frame, device)

    def _push(self, frame, device):
        m = self.model
        if self.plan is None or (not self.primed and m._weights_key() != self._wkey):
            if self.plan is not None:
                torch.cuda.current_stream().synchronize()
                self.plan.release()
            self.plan = self._build(device)
        pl = self.plan
        if not self.primed:
            pl.reset()
            pl.frame_in.copy_(frame)
            pl.prime()
            self.primed = True
            return None
        # enqueue first, check the weights while the step runs (as forward() does)
        self._step(frame)
        if m._weights_key() != self._wkey:
            # the weights changed since the plan was packed: the step that just ran is stale.  Rebuild,
            # encode the held previous frame again with the new weights, and run the step again.
            torch.cuda.current_stream().synchronize()
            old = pl
            pl = self.plan = self._build(device)
            pl.prime(raw=old.raw_prev)
            if self._prev_low is not None:
                pl.flow_low.copy_(self._prev_low)
            torch.cuda.current_stream().synchronize()
            old.release()
            self._step(frame)
        return self._finish(pl)

    def _finish(self, pl):
        m = self.model
        left, right, top, bottom = pl.pad
        low = pl.flow_low.clone()
        up = pl.flow_up[0][..., top:pl.Hp - bottom, left:pl.Wp - right].clone()
        self.last_flow_init = pl.flow_init.clone() if self.warm_start else None
        bidi, B = self.bidirectional, pl.B
        if bidi:
            occ, err = [o.view(torch.bool).clone() for o in pl.occ], [e.clone() for e in pl.err]
        rgb = [t.clone() for t in pl.rgb] if self.visualize else None
        if self.warp:
            warped, wvalid = [t.clone() for t in pl.warped], [t.view(torch.bool).clone() for t in pl.warp_valid]
        mode = m.range_guard
        if pl.guarded and mode != "off":
            raised = bool(int(pl.range_flag.item()))
            if raised or self._inexact_prev:
                msg = ("f16x3 range guard: an activation exceeded 2^15 in magnitude, outside the exact range "
                       "of the split-f16 conv arithmetic")
                if mode == "raise":
                    raise FloatingPointError(msg)
                warnings.warn(msg + "; this step was re-run with exact f32 MFMA convs", RuntimeWarning)
                i1, i2 = pl.raw_prev, pl.raw_cur
                if bidi:
                    i1, i2 = torch.cat([i1, i2]), torch.cat([i2, i1])
                low, up_p = m.forward(i1, i2, self.iters, self.last_flow_init, True, True, _prec="fp32")
                up = up_p[..., top:pl.Hp - bottom, left:pl.Wp - right].clone()
                if bidi:  # the masks of the exact flows
                    o_fw, o_bw, e_fw, e_bw = fb_consistency(up[:B], up[B:], self.fb_alpha, self.fb_beta)
                    occ, err = [o_fw, o_bw], [e_fw, e_bw]
                if self.visualize:  # the colours of the exact flows (backward: under the current frame)
                    crop = (Ellipsis, slice(top, pl.Hp - bottom), slice(left, pl.Wp - right))
                    rgb = [flow_to_rgb(up[k * B:(k + 1) * B], self.viz_rad_max, None, self.visualize == "bgr",
                                       fr[crop] if self.viz_stack else None)
                           for k, fr in enumerate((pl.raw_prev, pl.raw_cur)[:2 if bidi else 1])]
                if self.warp:  # the warps by the exact flows (forward: of the current frame)
                    crop = (Ellipsis, slice(top, pl.Hp - bottom), slice(left, pl.Wp - right))
                    ww = [warp_frame(fr[crop], up[k * B:(k + 1) * B], self.warp, pl.warped[0].dtype)
                          for k, fr in enumerate((pl.raw_cur, pl.raw_prev)[:2 if bidi else 1])]
                    warped, wvalid = [w[0] for w in ww], [w[1] for w in ww]
                pl.flow_low.copy_(low)  # the next warm start begins from the exact flow
            # (a flagged step leaves this frame's feature map inexact: the next pair is re-run as well)
            self._inexact_prev = raised
        if self.warm_start:
            self._prev_low = low.clone()
        if bidi:
            out = BidirectionalFlow(low[:B], up[:B], low[B:], up[B:], occ[0], occ[1], err[0], err[1])
            if self.warp:
                return BidirectionalFlowVizWarp(*out, *rgb, *warped, *wvalid) if self.visualize else \
                    BidirectionalFlowWarp(*out, *warped, *wvalid)
            return BidirectionalFlowViz(*out, *rgb) if self.visualize else out
        if self.warp:
            return FlowVizWarp(low, up, rgb[0], warped[0], wvalid[0]) if self.visualize else \
                FlowWarp(low, up, warped[0], wvalid[0])
        return FlowViz(low, up, rgb[0]) if self.visualize else (low, up)


def _register_exit_check(model):
    """Resolve a model's deferred range-guard checks at interpreter exit (a weak reference: the
    hook keeps no model alive)."""
    if getattr(model, "_exit_hook", False):
        return
    ref = weakref.ref(model)

    def _flush():
        m = ref()
        if m is not None and m._pending:
            try:
                m.check_range_guard(block=True)
            except Exception as e:  # noqa: BLE001 (the GPU context may already be gone)
                warnings.warn(f"range guard: deferred checks could not be resolved at exit: {e}", RuntimeWarning)

    atexit.register(_flush)
    model.__dict__["_exit_hook"] = True
