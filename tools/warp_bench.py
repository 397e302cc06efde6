"""Video throughput with the current frame warped back onto the previous one per pair, at config 2 (436x1024
frames, iters=32, B=1): where the warp runs, four ways, for float32 [1,3,H,W] and for uint8 [1,H,W,3] frames.

    python tools/warp_bench.py [--windows 5] [--window-s 1.0] [--out FILE]

A seeded, drifting smooth_images sequence of --frames distinct frames is cycled through (stream_bench.py's).
One pair ends with the warped frame and its mask on the device, in the pushed frame's own layout and dtype.
  leg a (grid_sample)   stream.push, then the warp a caller writes in torch: a pixel grid plus the flow,
                        normalised to [-1, 1], F.grid_sample(align_corners=True), and the in-frame mask; for uint8
                        frames the permute / float / round / clamp / permute round trip around it.  The only way
                        before utils.warp_frame.
  leg b (warp_frame)    stream.push, then utils.warp_frame(frame, flow_up): one launch
  leg c (in the step)   stream.push with warp="zeros" (the launch is part of the captured step)
  leg d (no warp)       plain stream.push: the ceiling
The legs are warmed up until their graphs are captured, then a, b, c, d alternate --windows times in one
process; a window is at least --window-s seconds of work and ends in a device synchronise.

The launch inside the step is timed as bidi_bench.py times the consistency launch: a hipGraph of --reps
repetitions of the plan's own raft_warp_frame call (padded flow_up and raw frame in place) between two events;
the same graph over an 8 x 8 frame gives the floor a launch costs in such a graph.  raft_splat_density (three
launches: zero, 64-bit integer atomic splat, convert) is timed the same way on the flow_up of the last pair.
Algorithmic bytes per pixel: warp 8 B of flow + 12 B of frame read, 12 B (float32) or 3 B (uint8) + 1 B
written; density 8 B zeroed, 8 B of flow read, 4 x 8 B of atomic adds, 8 B read back and 4 B written.

Prints ONE JSON line: pairs/s of each leg per window, medians, spreads (max - min), whether leg c's gain over
leg a (and over leg b) exceeds the two legs' spreads, leg c's distance from leg d, and the launches' times."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from raft_optical_flow_amd import RAFT, _lib  # noqa: E402
from raft_optical_flow_amd.init import seeded_state_dict  # noqa: E402
from raft_optical_flow_amd.kernels import Launch  # noqa: E402
from raft_optical_flow_amd.utils import warp_frame  # noqa: E402
from bidi_bench import consistency_time as launch_time  # noqa: E402
from stream_bench import compare, make_frames  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X specification


def torch_warp(frame, flow):
    """What a caller writes today: (warped in the frame's layout and dtype, valid [B,1,H,W])."""
    u8 = frame.dtype == torch.uint8
    img = frame.permute(0, 3, 1, 2).float() if u8 else frame
    B, _, H, W = img.shape
    x = torch.arange(W, device=flow.device, dtype=torch.float32).view(1, 1, W) + flow[:, 0]
    y = torch.arange(H, device=flow.device, dtype=torch.float32).view(1, H, 1) + flow[:, 1]
    grid = torch.stack([2.0 * x / (W - 1) - 1.0, 2.0 * y / (H - 1) - 1.0], dim=3)
    out = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    valid = ((x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1))[:, None]
    if u8:
        out = out.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return out, valid


class Leg:
    def __init__(self, model, frames, iters, how):
        self.f, self.t, self.how = frames, 0, how
        self.s = model.stream(iters=iters, warp="zeros" if how == "c" else None)
        self.s.push(frames[0])
        self.last = None

    def step(self):
        self.t += 1
        cur = self.f[self.t % len(self.f)]
        out = self.s.push(cur)
        if self.how == "a":
            self.last = torch_warp(cur, out[1])
        elif self.how == "b":
            self.last = warp_frame(cur, out[1])
        elif self.how == "c":
            self.last = (out.warped, out.valid)
        return out

    def close(self):
        self.s.close()


def warp_launch(plan):
    return next(l for l in plan.launches if not isinstance(l, str) and l.name == "raft_warp_frame")


def run_legs(m, frames, args):
    """The four legs on one frame format: throughput, the legs' agreement on one pair, the launch's time."""
    H, W = args.height, args.width
    u8 = frames[0].dtype == torch.uint8
    names = {"a": "a_push_grid_sample", "b": "b_push_warp_frame", "c": "c_push_warp_in_step", "d": "d_push_only"}
    legs = {names[k]: Leg(m, frames, args.iters, k) for k in "abcd"}
    r = compare(legs, args.windows, args.window_s)
    a, b, c, d = (r[names[k]] for k in "abcd")
    for leg in legs.values():       # the legs' results on one and the same pair
        leg.s.reset()
        leg.t = 0
        leg.s.push(frames[0])
        leg.step()
    (wa, va), (wb, vb), (wc, vc) = (legs[names[k]].last for k in "abc")
    diff = (wa.float() - wc.float()).abs()
    res = {"results": {"b_equals_c": bool(torch.equal(wb, wc) and torch.equal(vb, vc)),
                       "a_vs_c_max_abs": round(float(diff.max()), 6),
                       "a_vs_c_valid_differing": int((va != vc).sum()), "pixels": H * W,
                       "valid_share": round(float(vc.float().mean()), 4)}}
    r["c_over_a"] = round(c["median"] / a["median"], 4)
    r["c_over_b"] = round(c["median"] / b["median"], 4)
    r["c_gain_over_a_exceeds_spreads"] = bool(c["median"] - a["median"] > a["spread"] + c["spread"])
    r["c_gain_over_b_exceeds_spreads"] = bool(c["median"] - b["median"] > b["spread"] + c["spread"])
    r["b_and_c_equal_within_spread"] = bool(abs(c["median"] - b["median"]) <= b["spread"] + c["spread"])
    r["d_minus_c"] = {"pairs_per_s": round(d["median"] - c["median"], 2), "spread": round(d["spread"] + c["spread"], 2),
                      "ms_per_pair": round(1e3 / c["median"] - 1e3 / d["median"], 4)}
    r["ms_per_pair"] = {k: round(1e3 / r[names[k]]["median"], 4) for k in "abcd"}
    res["throughput"] = r
    plan = legs[names["c"]].s.plan
    us, spread = launch_time(warp_launch(plan), args.reps)
    dev = frames[0].device
    tag = _lib.FRAME_U8_NHWC if u8 else _lib.FRAME_F32_NCHW
    tiny, timg = torch.zeros(1, 2, 8, 8, device=dev), torch.zeros(1, 3, 8, 8, device=dev)
    tout = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=dev) if u8 else torch.zeros(1, 3, 8, 8, device=dev)
    tval = torch.zeros(1, 1, 8, 8, dtype=torch.uint8, device=dev)
    floor_us, _ = launch_time(Launch("raft_warp_frame", tiny.data_ptr(), 128, 64, 8, timg.data_ptr(),
                                     _lib.FRAME_F32_NCHW, 192, 64, 8, 0, 0, 1, 3, 8, 8, 0, tout.data_ptr(), tag,
                                     tval.data_ptr()), args.reps)
    nbytes = H * W * (8 + 12 + (3 if u8 else 12) + 1)
    net = max(us - floor_us, 1e-3)
    res["warp_launch"] = {"launches": 1, "device_us": round(us, 2), "spread_us": round(spread, 2),
                          "launch_floor_us": round(floor_us, 2), "algorithmic_bytes": nbytes,
                          "fraction_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4),
                          "fraction_of_hbm_peak_floor_subtracted": round(nbytes / (net * 1e-6) / HBM_PEAK, 4),
                          "timed_as": f"hipGraph of {args.reps} calls between two events"}
    left, right, top, bottom = plan.pad
    flow_up = plan.flow_up[0][..., top:plan.Hp - bottom, left:plan.Wp - right].clone()
    for leg in legs.values():
        leg.close()
    return res, flow_up


def density_time(flow_up, reps):
    """raft_splat_density on a flow [1,2,H,W]: device time per call (3 launches), the floor, the bytes."""
    L = _lib.load()
    dev = flow_up.device
    _, _, H, W = flow_up.shape
    ws = torch.zeros(L.raft_splat_ws_bytes(1, H, W) // 8, dtype=torch.int64, device=dev)
    den = torch.zeros(1, 1, H, W, device=dev)
    us, spread = launch_time(Launch("raft_splat_density", flow_up.data_ptr(), 2 * H * W, H * W, W, 0, 0, 1, H, W,
                                    ws.data_ptr(), den.data_ptr()), reps)
    tiny, tws, tden = torch.zeros(1, 2, 8, 8, device=dev), torch.zeros(64, dtype=torch.int64, device=dev), \
        torch.zeros(1, 1, 8, 8, device=dev)
    floor_us, _ = launch_time(Launch("raft_splat_density", tiny.data_ptr(), 128, 64, 8, 0, 0, 1, 8, 8, tws.data_ptr(),
                                     tden.data_ptr()), reps)
    nonzero = float((den > 0).float().mean())
    nbytes = H * W * (8 + 8 + 4 * 8 + 8 + 4)
    net = max(us - floor_us, 1e-3)
    return {"launches": 3, "device_us": round(us, 2), "spread_us": round(spread, 2),
            "launch_floor_us": round(floor_us, 2), "algorithmic_bytes": nbytes,
            "atomic_bytes": H * W * 32, "fraction_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4),
            "fraction_of_hbm_peak_floor_subtracted": round(nbytes / (net * 1e-6) / HBM_PEAK, 4),
            "atomic_bytes_per_s_floor_subtracted": round(H * W * 32 / (net * 1e-6), 0),
            "density_max": round(float(den.max()), 3), "share_of_pixels_reached": round(nonzero, 4),
            "timed_as": f"hipGraph of {reps} calls (3 launches each) between two events; all three launches are "
                        "in the time, so the atomic rate is a lower bound"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.frames < 8 or args.windows < 5:
        ap.error("at least 8 distinct frames and 5 alternations")
    dev = torch.device("cuda:0")
    m = RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False))
    m.load_state_dict(seeded_state_dict(m, 0))
    m.to(dev).eval()
    m.conv_precision = args.precision
    f32 = make_frames(args.frames, args.height, args.width, dev)
    u8 = [f.permute(0, 2, 3, 1).contiguous().to(torch.uint8) for f in f32]
    res = {"tool": "warp_bench", "height": args.height, "width": args.width, "iters": args.iters, "batch": 1,
           "precision": m.resolved_precision(), "frames": args.frames, "window_s": args.window_s,
           "pair": "flow + the current frame warped onto the previous one and its mask, on the device, in the "
                   "frame's own layout (leg d: flow only)",
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        res["f32"], flow_up = run_legs(m, f32, args)
        res["uint8"], _ = run_legs(m, u8, args)
        res["splat_density"] = density_time(flow_up.contiguous(), args.reps)
        m.release_plans()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
