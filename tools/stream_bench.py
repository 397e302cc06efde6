"""Video throughput: the pairwise loop against RAFT.stream, config 2 (436x1024 frames, iters=32, B=1).

    python tools/stream_bench.py [--windows 5] [--window-s 1.0] [--phases] [--out FILE]

A seeded, drifting smooth_images sequence of --frames distinct frames is cycled through.
  leg A (pairwise)  InputPadder.pad + model(f[t], f[t+1], test_mode=True) per pair: every frame passes
                    through fnet twice.  This is code the stream work did not change.
  leg B (stream)    stream.push(f[t+1]).
Both legs are warmed up until their graph is captured, then A and B alternate --windows times in one
process; a window is at least --window-s seconds of work and ends in a device synchronise.  The two legs
run with warm_start off, then with it on.  With the warm start, leg A runs evaluate.py:37-41's line,
`forward_interpolate(flow_low[0])[None]`, on this package's device-side helper ("pairwise"), and a
second time the way the reference's own helper does it, through the host ("pairwise_host": flow_low to
the CPU, the helper, the result back to the GPU).

Prints ONE JSON line: pairs/s of each leg per window, the medians and the spread (max - min over the
windows) of each leg.  --phases adds event stamps around one eager step of each leg (queued behind
other work, so the host is not what they measure): the encoder-phase span (first launch to the join of
the feature and context branches), each branch's end, and the in-step forward_interpolate."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from raft_optical_flow_amd import RAFT, InputPadder  # noqa: E402
from raft_optical_flow_amd import kernels as K  # noqa: E402
from raft_optical_flow_amd.init import seeded_state_dict, smooth_images  # noqa: E402
from raft_optical_flow_amd.utils.utils import forward_interpolate  # noqa: E402


def make_frames(n, H, W, dev):
    return [smooth_images(1, H, W, seed=7, shift=(1.5 * k, -1.0 * k))[1].to(dev) for k in range(n)]


class Pairwise:
    def __init__(self, model, frames, iters, warm, host_interp=False):
        self.m, self.f, self.iters, self.warm, self.host = model, frames, iters, warm, host_interp
        self.t, self.flow_prev = 0, None

    def step(self):
        f = self.f
        a, b = f[self.t % len(f)], f[(self.t + 1) % len(f)]
        self.t += 1
        padder = InputPadder(a.shape)
        a, b = padder.pad(a, b)
        low, up = self.m(a, b, iters=self.iters, flow_init=self.flow_prev, test_mode=True)
        if self.warm:
            if self.host:
                self.flow_prev = forward_interpolate(low[0].cpu())[None].to(a.device)
            else:
                self.flow_prev = forward_interpolate(low[0])[None]
        return low, padder.unpad(up)


class Stream:
    def __init__(self, model, frames, iters, warm):
        self.f, self.t = frames, 0
        self.s = model.stream(iters=iters, warm_start=warm)
        self.s.push(frames[0])

    def step(self):
        self.t += 1
        return self.s.push(self.f[self.t % len(self.f)])


def window(leg, seconds):
    """pairs/s over at least `seconds` of work, ending in a device synchronise."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(8):
            leg.step()
        n += 8
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


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


# -- event stamps ---------------------------------------------------------------------------------


def stamped_run(plan, marks_side=()):
    """plan.launches run eagerly as kernels.run does, with events: before the first launch, at the end of
    each branch, behind the first JOIN, behind the last launch, and around the side launches named in
    marks_side.  Returns {label: event}."""
    main = torch.cuda.current_stream()
    if plan.side_stream is None:
        plan.side_stream = torch.cuda.Stream(device=plan.device)
    side = plan.side_stream
    ev = {}

    def stamp(label, stream):
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        ev[label] = e

    stamp("start", main)
    joined = False
    for l in plan.launches:
        if l is K.FORK:
            side.wait_stream(main)
        elif l is K.JOIN:
            if not joined:
                stamp("main_end", main)
                stamp("side_end", side)
            main.wait_stream(side)
            if not joined:
                stamp("join", main)
                joined = True
        else:
            mark = l.side and l.name in marks_side
            if mark:
                stamp(l.name + ":start", side)
            l(side.cuda_stream if l.side else main.cuda_stream)
            if mark:
                stamp(l.name + ":end", side)
    stamp("end", main)
    return ev


def phases_of(plan, prepare, reps=7, marks_side=()):
    """Median over reps of the stamped spans (us).  Each stamped step is queued behind two unstamped
    eager steps, so its launches wait for the GPU rather than the GPU for the host."""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        for _ in range(2):
            prepare()
            plan.run()
        prepare()
        ev = stamped_run(plan, marks_side)
        torch.cuda.synchronize()
        us = lambda a, b: 1e3 * ev[a].elapsed_time(ev[b])  # noqa: E731
        d = {"encoder_phase_us": us("start", "join"), "main_branch_end_us": us("start", "main_end"),
             "side_branch_end_us": us("start", "side_end"), "step_us": us("start", "end")}
        for n in marks_side:
            if n + ":start" in ev:
                d[n + "_us"] = us(n + ":start", n + ":end")
                d[n + "_end_us"] = us("start", n + ":end")
        out.append(d)
    return {k: round(statistics.median(d[k] for d in out), 1) for k in out[0]}


def phases(model, frames, iters):
    from raft_optical_flow_amd.engine import StreamPlan
    dev = frames[0].device
    a, b = InputPadder(frames[0].shape).pad(frames[0], frames[1])
    res = {}
    for warm in (False, True):
        rp = model.plan(1, a.shape[2], a.shape[3], iters, True, warm, dev)
        fi = torch.zeros(1, 2, a.shape[2] // 8, a.shape[3] // 8, device=dev) if warm else None
        pair = phases_of(rp, lambda: rp.set_inputs(a, b, fi))
        sp = StreamPlan(model.packed(dev), 1, frames[0].shape[2], frames[0].shape[3], iters, warm_start=warm,
                        device=dev, range_guard=model.range_guard != "off")
        sp.frame_in.copy_(frames[0])
        sp.prime()
        flip = [0]

        def feed():
            flip[0] += 1
            sp.frame_in.copy_(frames[flip[0] % len(frames)])
        stream = phases_of(sp, feed, marks_side=("raft_forward_interpolate",) if warm else ())
        sp.release()
        res["warm" if warm else "cold"] = {"pairwise": pair, "stream": stream}
    model.release_plans()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--phases", action="store_true")
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
    res = {"tool": "stream_bench", "height": args.height, "width": args.width, "iters": args.iters, "batch": 1,
           "precision": m.resolved_precision(), "frames": args.frames, "window_s": args.window_s,
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        for warm in (False, True):
            legs = {"pairwise": Pairwise(m, frames, args.iters, warm)}
            if warm:
                legs["pairwise_host"] = Pairwise(m, frames, args.iters, warm, host_interp=True)
            legs["stream"] = Stream(m, frames, args.iters, warm)
            r = compare(legs, args.windows, args.window_s)
            best = max(r[k]["median"] for k in r if k != "stream")
            r["stream_over_pairwise"] = round(r["stream"]["median"] / best, 4)
            r["stream_gain_exceeds_spreads"] = bool(
                r["stream"]["median"] - best > max(v["spread"] for k, v in r.items() if isinstance(v, dict)))
            res["warm_start" if warm else "cold_start"] = r
            legs["stream"].s.close()
            m.release_plans()
        if args.phases:
            res["phases_us"] = phases(m, frames, args.iters)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
