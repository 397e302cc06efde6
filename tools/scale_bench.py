"""Video throughput at a working size, at config 5's frames (1080x1920, iters=32, B=1) run at 544x960: where the
two resizes run, four ways, for float32 [1,3,H,W] and for uint8 [1,H,W,3] frames.

    python tools/scale_bench.py [--windows 5] [--window-s 1.0] [--out FILE]

A seeded, drifting smooth_images sequence of --frames distinct frames is cycled through (stream_bench.py's).
One pair ends with flow_up at the frame's own size, in its pixels, on the device.
  leg a (full size)     stream.push of the full-size frame: no resize at all
  leg b (F.interpolate) what a caller writes in torch, InputScaler's sequence on GPU tensors: F.interpolate of the
                        frame down to the working size (for uint8 frames the permute / float in front of it),
                        stream.push, F.interpolate of flow_up back and the two multiplies.  The only way before
                        utils.resize_frame / resize_flow.
  leg c (raft_resize)   utils.resize_frame(frame, (h, w), out_dtype=torch.float32), stream.push,
                        utils.resize_flow(flow_up, (H, W)): one raft_resize launch on either side of the step
  leg d (pre-resized)   stream.push of frames that already have the working size: the ceiling (its flow_up stays at
                        the working size)
The legs are warmed up until their graphs are captured, then a, b, c, d alternate --windows times in one
process; a window is at least --window-s seconds of work and ends in a device synchronise.

The two resize launches are timed as warp_bench.py times the warp: a hipGraph of --reps repetitions of the
raft_resize call between two events; the same graph over an 8 x 8 -> 4 x 4 frame gives the floor a launch costs
in such a graph.  Algorithmic bytes: the frame down, 12 B (float32) or 3 B (uint8) per source pixel read and 12 B
per working-size pixel written; the flow up, 8 B per working-size pixel read and 8 B per full-size pixel written.

Prints ONE JSON line: pairs/s of each leg per window, medians, spreads (max - min), whether leg c exceeds leg b
by more than the two legs' spreads, leg c's distance from legs a and d, the legs' agreement on one pair, and the
launches' times."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from raft_optical_flow_amd import RAFT, _lib  # noqa: E402
from raft_optical_flow_amd.init import seeded_state_dict  # noqa: E402
from raft_optical_flow_amd.kernels import Launch  # noqa: E402
from raft_optical_flow_amd.utils import resize_flow, resize_frame  # noqa: E402
from bidi_bench import consistency_time as launch_time  # noqa: E402
from stream_bench import compare, make_frames  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X specification


def torch_down(frame, size):
    """What a caller writes today: the frame as float32 [B,3,h,w]."""
    img = frame.permute(0, 3, 1, 2).float() if frame.dtype == torch.uint8 else frame
    return F.interpolate(img, size=size, mode="bilinear", align_corners=False)


def torch_up(flow, size):
    """InputScaler.unfill(flow, is_flow=True) on a GPU tensor."""
    h, w = flow.shape[-2:]
    up = F.interpolate(flow, size=size, mode="bilinear", align_corners=False)
    up[:, 0] = up[:, 0] * (float(size[1]) / w)
    up[:, 1] = up[:, 1] * (float(size[0]) / h)
    return up


class Leg:
    def __init__(self, model, frames, small, iters, how, work):
        self.f, self.small, self.t, self.how, self.work = frames, small, 0, how, work
        self.full = tuple(frames[0].shape[1:3] if frames[0].dtype == torch.uint8 else frames[0].shape[2:])
        self.s = model.stream(iters=iters)
        self.last = None
        self.push(0)

    def push(self, i):
        if self.how == "b":
            out = self.s.push(torch_down(self.f[i], self.work))
            return None if out is None else (out[0], torch_up(out[1], self.full))
        if self.how == "c":
            out = self.s.push(resize_frame(self.f[i], self.work, out_dtype=torch.float32))
            return None if out is None else (out[0], resize_flow(out[1], self.full))
        return self.s.push(self.small[i] if self.how == "d" else self.f[i])

    def step(self):
        self.t += 1
        self.last = self.push(self.t % len(self.f))
        return self.last

    def close(self):
        self.s.close()


def resize_times(frame, work, reps):
    """Device time of the two launches around a step: the frame down (float32 out) and flow_up back up."""
    dev = frame.device
    u8 = frame.dtype == torch.uint8
    H, W = frame.shape[1:3] if u8 else frame.shape[2:]
    h, w = work
    F32, U8 = _lib.FRAME_F32_NCHW, _lib.FRAME_U8_NHWC
    small = torch.empty(1, 3, h, w, device=dev)
    flow = torch.randn(1, 2, h, w, device=dev)
    up = torch.empty(1, 2, H, W, device=dev)
    t_in = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=dev) if u8 else torch.zeros(1, 3, 8, 8, device=dev)
    t_out = torch.zeros(1, 3, 4, 4, device=dev)

    def call(src, tag, c, hs, ws, dst, hd, wd, m0, m1):
        return Launch("raft_resize", src.data_ptr(), tag, c * hs * ws, hs * ws, ws, 0, 0, 1, c, hs, ws, dst.data_ptr(),
                      F32, hd, wd, _lib.RESIZE_BILINEAR, 0, m0, m1)

    floor_us, _ = launch_time(call(t_in, U8 if u8 else F32, 3, 8, 8, t_out, 4, 4, 1.0, 1.0), reps)
    out = {"launch_floor_us": round(floor_us, 2), "timed_as": f"hipGraph of {reps} calls between two events"}
    legs = (("frame_down", call(frame, U8 if u8 else F32, 3, H, W, small, h, w, 1.0, 1.0),
             H * W * (3 if u8 else 12) + h * w * 12),
            ("flow_up", call(flow, F32, 2, h, w, up, H, W, float(W) / w, float(H) / h), h * w * 8 + H * W * 8))
    for name, launch, nbytes in legs:
        us, spread = launch_time(launch, reps)
        net = max(us - floor_us, 1e-3)
        out[name] = {"device_us": round(us, 2), "spread_us": round(spread, 2), "algorithmic_bytes": nbytes,
                     "fraction_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4),
                     "fraction_of_hbm_peak_floor_subtracted": round(nbytes / (net * 1e-6) / HBM_PEAK, 4)}
    return out


def run_legs(m, frames, args):
    """The four legs on one frame format: throughput, the legs' agreement on one pair, the launches' times."""
    work = (args.work_height, args.work_width)
    small = [resize_frame(f, work, out_dtype=torch.float32) for f in frames]
    names = {"a": "a_push_full_size", "b": "b_interpolate_push_interpolate", "c": "c_resize_push_resize",
             "d": "d_push_pre_resized"}
    legs = {names[k]: Leg(m, frames, small, args.iters, k, work) for k in "abcd"}
    r = compare(legs, args.windows, args.window_s)
    a, b, c, d = (r[names[k]] for k in "abcd")
    for leg in legs.values():       # the legs' results on one and the same pair
        leg.s.reset()
        leg.t = 0
        leg.push(0)
        leg.step()
    ua, ub, uc = (legs[names[k]].last[1] for k in "abc")
    res = {"results": {"b_vs_c_flow_up_max_abs": round(float((ub - uc).abs().max()), 6),
                       "a_vs_c_flow_up_mean_abs": round(float((ua - uc).abs().mean()), 4),
                       "flow_up_mean_abs": round(float(uc.abs().mean()), 4), "flow_up_shape": list(uc.shape)}}
    r["c_over_b"] = round(c["median"] / b["median"], 4)
    r["c_over_a"] = round(c["median"] / a["median"], 4)
    r["c_gain_over_b_exceeds_spreads"] = bool(c["median"] - b["median"] > b["spread"] + c["spread"])
    r["b_and_c_equal_within_spread"] = bool(abs(c["median"] - b["median"]) <= b["spread"] + c["spread"])
    r["d_minus_c"] = {"pairs_per_s": round(d["median"] - c["median"], 2), "spread": round(d["spread"] + c["spread"], 2),
                      "ms_per_pair": round(1e3 / c["median"] - 1e3 / d["median"], 4)}
    r["ms_per_pair"] = {k: round(1e3 / r[names[k]]["median"], 4) for k in "abcd"}
    res["throughput"] = r
    res["resize_launches"] = resize_times(frames[0], work, args.reps)
    for leg in legs.values():
        leg.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--work-height", type=int, default=544)
    ap.add_argument("--work-width", type=int, default=960)
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
    res = {"tool": "scale_bench", "height": args.height, "width": args.width, "work_height": args.work_height,
           "work_width": args.work_width, "iters": args.iters, "batch": 1, "precision": m.resolved_precision(),
           "frames": args.frames, "window_s": args.window_s,
           "pair": "flow_up at the frame's own size, in its pixels, on the device (leg d: at the working size)",
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        res["f32"] = run_legs(m, f32, args)
        res["uint8"] = run_legs(m, u8, args)
        m.release_plans()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
