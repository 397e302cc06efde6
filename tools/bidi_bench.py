"""Bidirectional video throughput at config 2 (436x1024 frames, iters=32, B=1): both flows of every pair plus
their forward-backward occlusion masks, three ways.

    python tools/bidi_bench.py [--windows 5] [--window-s 1.0] [--out FILE]

A seeded, drifting smooth_images sequence of --frames distinct frames is cycled through (stream_bench.py's).
  leg a (pairwise)     InputPadder.pad + model(cat[a, b], cat[b, a], test_mode=True) per pair, then the
                       consistency check in torch (grid_sample, align_corners=True): fnet on 4 images and cnet
                       on 2 per pair.  The only way before RAFT.stream(bidirectional=True).
  leg b (two streams)  one one-directional stream over the sequence and one over the reversed sequence (the
                       backward flows of an offline video), then utils.fb_consistency on their outputs.  The
                       two streams' pairs do not coincide in time; the work per pair is that of one pair.
  leg c (bidi stream)  stream.push(f[t+1]) with bidirectional=True.
One pair = both flows plus both masks.  The legs are warmed up until their graphs are captured, then a, b, c
alternate --windows times in one process; a window is at least --window-s seconds of work and ends in a device
synchronise.  Cold start, then warm start (each direction from forward_interpolate of its own direction's flow
of the pair before; leg a runs the device-side helper on its [2,2,h,w] flow_low).

The consistency launch alone is timed as a hipGraph of --fb-reps launches of the bidirectional plan's own
launch (its padded flow_up in place) between two events; its algorithmic bytes are, per pixel and direction,
8 B of the flow, 8 B of the other flow (each tap counted once), 4 B err and 1 B occ.  The same graph over an
8 x 8 frame gives the floor a launch costs in such a graph (launch_floor_us).

Prints ONE JSON line: pairs/s of each leg per window, medians, spreads (max - min), whether leg c's gain over
leg a exceeds the two legs' spreads, and the consistency launch's time and fraction of the 8 TB/s HBM peak."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from raft_optical_flow_amd import RAFT, InputPadder  # noqa: E402
from raft_optical_flow_amd.init import seeded_state_dict  # noqa: E402
from raft_optical_flow_amd.kernels import Launch  # noqa: E402
from raft_optical_flow_amd.utils.utils import fb_consistency, forward_interpolate  # noqa: E402
from stream_bench import make_frames, window  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X specification
ALPHA, BETA = 0.01, 0.5


def torch_consistency(fw, bw, alpha=ALPHA, beta=BETA):
    """The check of include/raft_hip.h in torch ops, as a caller would write it: sample the other flow at
    x + F(x) with grid_sample(align_corners=True); a target outside the frame is occluded."""
    B, _, H, W = fw.shape
    x = torch.arange(W, device=fw.device, dtype=torch.float32).view(1, 1, W)
    y = torch.arange(H, device=fw.device, dtype=torch.float32).view(1, H, 1)
    out = []
    for F, G in ((fw, bw), (bw, fw)):
        px, py = x + F[:, 0], y + F[:, 1]
        inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
        grid = torch.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], -1)
        g = torch.nn.functional.grid_sample(G, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        err = ((F + g) ** 2).sum(1, keepdim=True)
        thr = alpha * ((F ** 2).sum(1, keepdim=True) + (g ** 2).sum(1, keepdim=True)) + beta
        inside = inside[:, None]
        out.append((~inside | ~(err <= thr), torch.where(inside, err, torch.full_like(err, float("inf")))))
    return out[0][0], out[1][0], out[0][1], out[1][1]


class Pairwise:
    def __init__(self, model, frames, iters, warm):
        self.m, self.f, self.iters, self.warm = model, frames, iters, warm
        self.t, self.flow_prev = 0, None

    def step(self):
        f = self.f
        a, b = f[self.t % len(f)], f[(self.t + 1) % len(f)]
        self.t += 1
        padder = InputPadder(a.shape)
        a, b = padder.pad(a, b)
        low, up = self.m(torch.cat([a, b]), torch.cat([b, a]), iters=self.iters, flow_init=self.flow_prev,
                         test_mode=True)
        if self.warm:
            self.flow_prev = forward_interpolate(low)
        up = padder.unpad(up)
        return low, up, torch_consistency(up[:1], up[1:])


class TwoStreams:
    def __init__(self, model, frames, iters, warm):
        self.f, self.t = frames, 0
        self.fw = model.stream(iters=iters, warm_start=warm)
        self.bw = model.stream(iters=iters, warm_start=warm)
        self.fw.push(frames[0])
        self.bw.push(frames[0])

    def step(self):
        self.t += 1
        n = len(self.f)
        fw = self.fw.push(self.f[self.t % n])
        bw = self.bw.push(self.f[-self.t % n])
        return fw, bw, fb_consistency(fw[1], bw[1], ALPHA, BETA)

    def close(self):
        self.fw.close()
        self.bw.close()


class Bidi:
    def __init__(self, model, frames, iters, warm):
        self.f, self.t = frames, 0
        self.s = model.stream(iters=iters, warm_start=warm, bidirectional=True, fb_alpha=ALPHA, fb_beta=BETA)
        self.s.push(frames[0])

    def step(self):
        self.t += 1
        return self.s.push(self.f[self.t % len(self.f)])

    def close(self):
        self.s.close()


def compare(legs, windows, seconds):
    for leg in legs.values():       # eager first run, then the capture, then a replay
        for _ in range(4):
            leg.step()
    torch.cuda.synchronize()
    rates = {k: [] for k in legs}
    for _ in range(windows):
        for k, leg in legs.items():
            rates[k].append(window(leg, seconds))
    return {k: {"pairs_per_s": [round(x, 2) for x in v], "median": round(statistics.median(v), 2),
                "spread": round(max(v) - min(v), 2)} for k, v in rates.items()}


def consistency_time(launch, reps, rounds=7):
    """Median device time (us) per launch, and its spread: a hipGraph of `reps` launches between two events,
    over `rounds` replays."""
    torch.cuda.synchronize()
    launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = torch.cuda.current_stream().cuda_stream
        for _ in range(reps):
            launch(s)
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        us.append(1e3 * a.elapsed_time(b) / reps)
    return statistics.median(us), max(us) - min(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--fb-reps", type=int, default=200)
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
    res = {"tool": "bidi_bench", "height": args.height, "width": args.width, "iters": args.iters, "batch": 1,
           "precision": m.resolved_precision(), "frames": args.frames, "window_s": args.window_s,
           "pair": "both flows + both occlusion masks", "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        for warm in (False, True):
            legs = {"a_pairwise_torch_check": Pairwise(m, frames, args.iters, warm),
                    "b_two_streams": TwoStreams(m, frames, args.iters, warm),
                    "c_bidi_stream": Bidi(m, frames, args.iters, warm)}
            r = compare(legs, args.windows, args.window_s)
            a, c = r["a_pairwise_torch_check"], r["c_bidi_stream"]
            r["c_over_a"] = round(c["median"] / a["median"], 4)
            r["c_over_b"] = round(c["median"] / r["b_two_streams"]["median"], 4)
            r["c_gain_over_a_exceeds_spreads"] = bool(c["median"] - a["median"] > a["spread"] + c["spread"])
            res["warm_start" if warm else "cold_start"] = r
            if warm:
                plan = legs["c_bidi_stream"].s.plan
                us, spread = consistency_time(next(l for l in plan.launches if not isinstance(l, str)
                                                   and l.name == "raft_fb_consistency"), args.fb_reps)
                # the same graph over an 8 x 8 frame: what a launch costs in such a graph with nothing to do
                tiny = torch.zeros(2, 2, 8, 8, device=dev)
                outs = [torch.zeros(1, 1, 8, 8, dtype=torch.uint8, device=dev) for _ in range(2)]
                outs += [torch.zeros(1, 1, 8, 8, device=dev) for _ in range(2)]
                floor_us, _ = consistency_time(
                    Launch("raft_fb_consistency", tiny.data_ptr(), 128, 64, 8, tiny[1:].data_ptr(), 128, 64, 8, 0, 0,
                           1, 8, 8, ALPHA, BETA, *[t.data_ptr() for t in outs]), args.fb_reps)
                nbytes = 2 * args.height * args.width * 21
                res["consistency_launch"] = {"device_us": round(us, 2), "spread_us": round(spread, 2),
                                             "launch_floor_us": round(floor_us, 2),
                                             "algorithmic_bytes": nbytes,
                                             "fraction_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4),
                                             "timed_as": f"hipGraph of {args.fb_reps} launches between two events"}
            legs["b_two_streams"].close()
            legs["c_bidi_stream"].close()
            m.release_plans()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
