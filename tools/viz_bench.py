"""Video throughput with a flow colour image per pair, at config 2 (436x1024 frames, iters=32, B=1): where the
colour-wheel pass runs, four ways.

    python tools/viz_bench.py [--windows 5] [--window-s 1.0] [--out FILE]

A seeded, drifting smooth_images sequence of --frames distinct frames is cycled through (stream_bench.py's).
One pair ends with a host-resident uint8 [H,W,3] image (leg d: with nothing on the host).
  leg a (host numpy)    stream.push, flow_up.cpu() (8 bytes per pixel), then the colouring in plain numpy:
                        numpy_flow_to_image below, this tool's own restatement of the formula of
                        include/raft_hip.h in the reference's style (a dozen full-frame temporaries).  The only
                        way before utils.flow_viz.
  leg b (flow_to_rgb)   stream.push, utils.flow_viz.flow_to_rgb(flow_up) on the device, .cpu() (3 bytes per pixel)
  leg c (in the step)   stream.push with visualize="rgb" (the two launches are part of the captured step), .cpu()
  leg d (no image)      plain stream.push: the ceiling
The legs are warmed up until their graphs are captured, then a, b, c, d alternate --windows times in one
process; a window is at least --window-s seconds of work and ends in a device synchronise.

The two launches inside the step are timed as bidi_bench.py times the consistency launch: a hipGraph of
--viz-reps repetitions of the plan's own raft_flow_to_rgb call (its padded flow_up in place) between two events;
the same graph over an 8 x 8 frame gives the floor two launches cost in such a graph.  Algorithmic bytes per
pixel: 8 B of flow read by each launch and 3 B written.

Prints ONE JSON line: pairs/s of each leg per window, medians, spreads (max - min), whether leg c's gain over
leg a (and over leg b) exceeds the two legs' spreads, leg c's distance from leg d, and the launches' time."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from raft_optical_flow_amd import RAFT  # noqa: E402
from raft_optical_flow_amd.init import seeded_state_dict  # noqa: E402
from raft_optical_flow_amd.kernels import Launch  # noqa: E402
from raft_optical_flow_amd.utils.flow_viz import flow_to_rgb, make_colorwheel  # noqa: E402
from bidi_bench import consistency_time as launch_time  # noqa: E402
from stream_bench import compare, make_frames  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X specification
WHEEL = make_colorwheel()


def numpy_flow_to_image(flow_uv):
    """[H,W,2] float32 -> uint8 [H,W,3] on the host: the formula of include/raft_hip.h written the way a numpy
    user writes it (whole-frame operations, one temporary each; float32 in, the wheel in float64)."""
    u, v = flow_uv[:, :, 0], flow_uv[:, :, 1]
    rad_max = np.max(np.sqrt(np.square(u) + np.square(v)))
    u = u / (rad_max + 1e-5)
    v = v / (rad_max + 1e-5)
    img = np.zeros((u.shape[0], u.shape[1], 3), np.uint8)
    rad = np.sqrt(np.square(u) + np.square(v))
    fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * (len(WHEEL) - 1)
    k0 = np.floor(fk).astype(np.int32)
    k1 = k0 + 1
    k1[k1 == len(WHEEL)] = 0
    f = fk - k0
    inside = rad <= 1
    for c in range(3):
        col = (1 - f) * (WHEEL[k0, c] / 255.0) + f * (WHEEL[k1, c] / 255.0)
        col[inside] = 1 - rad[inside] * (1 - col[inside])
        col[~inside] = col[~inside] * 0.75
        img[:, :, c] = np.floor(255 * col)
    return img


class Leg:
    def __init__(self, model, frames, iters, how):
        self.f, self.t, self.how = frames, 0, how
        self.s = model.stream(iters=iters, visualize="rgb" if how == "c" else None)
        self.s.push(frames[0])
        self.last = None

    def step(self):
        self.t += 1
        out = self.s.push(self.f[self.t % len(self.f)])
        if self.how == "a":
            self.last = numpy_flow_to_image(out[1][0].permute(1, 2, 0).cpu().numpy())
        elif self.how == "b":
            self.last = flow_to_rgb(out[1])[0].cpu()
        elif self.how == "c":
            self.last = out.rgb[0].cpu()
        return out

    def close(self):
        self.s.close()


def viz_launch(plan):
    return next(l for l in plan.launches if not isinstance(l, str) and l.name == "raft_flow_to_rgb")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--viz-reps", type=int, default=200)
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
    frames = make_frames(args.frames, args.height, args.width, dev)
    H, W = args.height, args.width
    res = {"tool": "viz_bench", "height": H, "width": W, "iters": args.iters, "batch": 1,
           "precision": m.resolved_precision(), "frames": args.frames, "window_s": args.window_s,
           "pair": "flow + a host-resident uint8 [H,W,3] colour image (leg d: flow only, nothing on the host)",
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        names = {"a": "a_push_cpu_numpy", "b": "b_push_flow_to_rgb_cpu", "c": "c_push_visualize_cpu",
                 "d": "d_push_only"}
        legs = {names[k]: Leg(m, frames, args.iters, k) for k in "abcd"}
        r = compare(legs, args.windows, args.window_s)
        a, b, c, d = (r[names[k]] for k in "abcd")
        # the legs' images of one and the same pair agree (a: numpy's own roundings, within one level)
        for leg in legs.values():
            leg.s.reset()
            leg.t = 0
            leg.s.push(frames[0])
            leg.step()
        ia, ib, ic = (np.asarray(legs[names[k]].last) for k in "abc")
        diff = np.abs(ia.astype(np.int32) - ic.astype(np.int32))
        res["images"] = {"b_equals_c": bool(np.array_equal(ib, ic)), "a_vs_c_max_level": int(diff.max()),
                         "a_vs_c_pixels_differing": int((diff.max(-1) > 0).sum()), "pixels": H * W}
        r["c_over_a"] = round(c["median"] / a["median"], 4)
        r["c_over_b"] = round(c["median"] / b["median"], 4)
        r["c_gain_over_a_exceeds_spreads"] = bool(c["median"] - a["median"] > a["spread"] + c["spread"])
        r["c_gain_over_b_exceeds_spreads"] = bool(c["median"] - b["median"] > b["spread"] + c["spread"])
        r["d_minus_c"] = {"pairs_per_s": round(d["median"] - c["median"], 2),
                          "spread": round(d["spread"] + c["spread"], 2),
                          "ms_per_pair": round(1e3 / c["median"] - 1e3 / d["median"], 4)}
        r["ms_per_pair"] = {k: round(1e3 / r[names[k]]["median"], 4) for k in "abcd"}
        res["throughput"] = r
        plan = legs[names["c"]].s.plan
        us, spread = launch_time(viz_launch(plan), args.viz_reps)
        tiny = torch.zeros(1, 2, 8, 8, device=dev)
        ws, out = torch.zeros(1, device=dev), torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=dev)
        floor_us, _ = launch_time(Launch("raft_flow_to_rgb", tiny.data_ptr(), 128, 64, 8, 0, 0, 1, 8, 8, 0.0, 0.0, 0,
                                         None, 0, 0, 0, ws.data_ptr(), out.data_ptr()), args.viz_reps)
        nbytes = H * W * (8 + 8 + 3)
        res["viz_launches"] = {"launches": 2, "device_us": round(us, 2), "spread_us": round(spread, 2),
                               "launch_floor_us": round(floor_us, 2), "algorithmic_bytes": nbytes,
                               "fraction_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4),
                               "timed_as": f"hipGraph of {args.viz_reps} calls (2 launches each) between two events"}
        for leg in legs.values():
            leg.close()
        m.release_plans()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
