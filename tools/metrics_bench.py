"""Validation throughput: scoring each predicted flow against ground truth on the host, as evaluate.py's
validate_* functions do, against utils.FlowMetrics on the device.  Config 2 (436x1024 frames, iters=32, B=1).

    python tools/metrics_bench.py [--windows 5] [--window-s 1.0] [--out profiles/metrics_bench.json]

A seeded, drifting smooth_images sequence of --frames distinct frames is cycled through (stream_bench.py's);
each pair has a ground-truth flow, float32 on the HOST in either leg (a dataset hands it out there).
  leg a (host)    validate_sintel's own sequence per pair (evaluate.py:109-116): InputPadder.pad,
                  model(..., test_mode=True), padder.unpad(flow_pr[0]).cpu(),
                  torch.sum((flow - flow_gt)**2, dim=0).sqrt() on the CPU, the numpy array appended to a Python
                  list; the means (EPE, 1 / 3 / 5 px) at the end of the window (:118-122).
  leg b (device)  the same forward, the ground truth uploaded, FlowMetrics.update on the unpadded view (no
                  copy of the flow, no synchronisation); one result() at the end of the window.
The legs are warmed up until their graphs are captured, then a and b alternate --windows times in one process; a
window is at least --window-s seconds of work and ends with the leg's means and a device synchronise.

The two launches of raft_flow_metrics are timed as bidi_bench.py times the consistency launch: a hipGraph of
--reps repetitions of the call on the unpadded view of the last pair between two events; the same graph over an
8 x 8 pair gives the floor two launches cost in such a graph.  Timed without a mask (as the legs call it) and
with validate_kitti's float mask.  Algorithmic bytes: 16 B per pixel (flow and ground truth) plus the mask (4 B
per pixel for a float mask).

Prints ONE JSON line: pairs/s of each leg per window, medians, spreads (max - min), whether leg b's gain over leg
a exceeds the two spreads, the two legs' results on the last window, and the launches' time."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from raft_optical_flow_amd import RAFT, InputPadder, _lib  # noqa: E402
from raft_optical_flow_amd.init import seeded_state_dict  # noqa: E402
from raft_optical_flow_amd.kernels import Launch  # noqa: E402
from raft_optical_flow_amd.utils import FlowMetrics  # noqa: E402
from bidi_bench import consistency_time as launch_time  # noqa: E402
from stream_bench import make_frames  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X specification


def make_ground_truth(n, H, W):
    """n (flow_gt [2,H,W], valid [H,W]) float32 host pairs: a smooth field of up to ~12 px and a mask that
    drops a fifth of the pixels (what the numbers are does not matter to the time; the mask is used for the
    launch timing only)."""
    rng = np.random.default_rng(5)
    y, x = np.mgrid[:H, :W].astype(np.float32)
    out = []
    for k in range(n):
        ph = rng.uniform(0, 2 * np.pi, size=4)
        gt = np.stack([12.0 * np.sin(2 * np.pi * x / W + ph[0]) * np.cos(2 * np.pi * y / H + ph[1]),
                       8.0 * np.cos(2 * np.pi * x / W + ph[2]) * np.sin(2 * np.pi * y / H + ph[3])]).astype(np.float32)
        valid = (rng.uniform(size=(H, W)) < 0.8).astype(np.float32)
        out.append((torch.from_numpy(gt), torch.from_numpy(valid)))
    return out


class Leg:
    def __init__(self, model, frames, truth, iters, on_device):
        self.m, self.f, self.gt, self.iters, self.on_device = model, frames, truth, iters, on_device
        self.t = 0
        self.metrics = FlowMetrics()
        self.epe_list = []
        self.last = None

    def step(self):
        f = self.f
        a, b = f[self.t % len(f)], f[(self.t + 1) % len(f)]
        flow_gt = self.gt[self.t % len(self.gt)][0]
        self.t += 1
        padder = InputPadder(a.shape)
        a, b = padder.pad(a, b)
        _, flow_pr = self.m(a, b, iters=self.iters, test_mode=True)
        if self.on_device:
            self.metrics.update(padder.unpad(flow_pr), flow_gt[None].to(a.device))
            return
        flow = padder.unpad(flow_pr[0]).cpu()                               # evaluate.py:113
        epe = torch.sum((flow - flow_gt) ** 2, dim=0).sqrt()                # :115
        self.epe_list.append(epe.view(-1).numpy())                          # :116

    def finish(self):
        """The means at the end of a window; clears the leg for the next one."""
        if self.on_device:
            r = self.metrics.result()
            self.metrics.reset()
            self.last = {k: r[k] for k in ("epe", "1px", "3px", "5px", "pixels", "images")}
            return
        epe_all = np.concatenate(self.epe_list)                             # :118-122
        self.last = {"epe": float(np.mean(epe_all)), "1px": float(np.mean(epe_all < 1)),
                     "3px": float(np.mean(epe_all < 3)), "5px": float(np.mean(epe_all < 5)),
                     "pixels": int(epe_all.size), "images": len(self.epe_list)}
        self.epe_list = []


def window(leg, seconds):
    """pairs/s over at least `seconds` of work, ending with the leg's means and a device synchronise."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(8):
            leg.step()
        n += 8
        if time.perf_counter() - t0 >= seconds:
            break
    leg.finish()
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def compare(legs, windows, seconds):
    for leg in legs.values():       # eager first run, then the capture, then a replay
        for _ in range(4):
            leg.step()
        leg.finish()
    torch.cuda.synchronize()
    rates = {k: [] for k in legs}
    for _ in range(windows):
        for k, leg in legs.items():
            rates[k].append(window(leg, seconds))
    return {k: {"pairs_per_s": [round(x, 2) for x in v], "median": round(statistics.median(v), 2),
                "spread": round(max(v) - min(v), 2)} for k, v in rates.items()}


def metrics_launch(flow, flow_gt, valid=None):
    """The raft_flow_metrics call FlowMetrics.update makes on these device tensors, as a Launch (and what it
    writes to, kept alive)."""
    L = _lib.load()
    B, _, H, W = flow.shape
    dev = flow.device
    rec = torch.zeros(B, _lib.FM_SLOTS, dtype=torch.int64, device=dev)
    tot = torch.zeros(_lib.FM_SLOTS, dtype=torch.int64, device=dev)
    ws = torch.zeros(L.raft_flow_metrics_ws_bytes(B, H, W) // 8, dtype=torch.int64, device=dev)
    keep = (flow, flow_gt, valid, rec, tot, ws)
    return Launch("raft_flow_metrics", flow.data_ptr(), flow.stride(0), flow.stride(1), flow.stride(2),
                  flow_gt.data_ptr(), flow_gt.stride(0), flow_gt.stride(1), flow_gt.stride(2),
                  None if valid is None else valid.data_ptr(), _lib.MASK_F32, 0 if valid is None else valid.stride(0),
                  0 if valid is None else valid.stride(1), B, H, W, 0.0, rec.data_ptr(), tot.data_ptr(), None,
                  ws.data_ptr(), keep=keep)


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
    H, W = args.height, args.width
    m = RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False))
    m.load_state_dict(seeded_state_dict(m, 0))
    m.to(dev).eval()
    m.conv_precision = args.precision
    frames = make_frames(args.frames, H, W, dev)
    truth = make_ground_truth(args.frames, H, W)
    res = {"tool": "metrics_bench", "height": H, "width": W, "iters": args.iters, "batch": 1,
           "precision": m.resolved_precision(), "frames": args.frames, "window_s": args.window_s,
           "pair": "forward + the pair's errors against a host-resident ground truth; the means (EPE, 1/3/5 px) "
                   "once per window",
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        legs = {"a_host_evaluate_py": Leg(m, frames, truth, args.iters, False),
                "b_device_flow_metrics": Leg(m, frames, truth, args.iters, True)}
        r = compare(legs, args.windows, args.window_s)
        a, b = r["a_host_evaluate_py"], r["b_device_flow_metrics"]
        r["b_over_a"] = round(b["median"] / a["median"], 4)
        r["b_gain_exceeds_spreads"] = bool(b["median"] - a["median"] > a["spread"] + b["spread"])
        r["equal_within_spreads"] = bool(abs(b["median"] - a["median"]) <= a["spread"] + b["spread"])
        r["ms_per_pair"] = {"a": round(1e3 / a["median"], 4), "b": round(1e3 / b["median"], 4)}
        res["throughput"] = r
        res["results_last_window"] = {k: leg.last for k, leg in legs.items()}

        # the launches, on the unpadded view of one pair's padded flow_up
        padder = InputPadder(frames[0].shape)
        p1, p2 = padder.pad(frames[0], frames[1])
        _, flow_pr = m(p1, p2, iters=args.iters, test_mode=True)
        view = padder.unpad(flow_pr.clone())
        gt, valid = truth[0][0][None].to(dev), truth[0][1][None].to(dev)
        tiny = [torch.zeros(1, 2, 8, 8, device=dev), torch.zeros(1, 2, 8, 8, device=dev),
                torch.ones(1, 8, 8, device=dev)]
        res["metrics_launches"] = {"view_is_contiguous": bool(view.is_contiguous()),
                                   "timed_as": f"hipGraph of {args.reps} calls (2 launches each) between two "
                                               "events; the operands stay in the caches between repetitions"}
        for name, mask, per_pixel in (("no_mask", None, 16), ("float_mask", valid, 20)):
            us, spread = launch_time(metrics_launch(view, gt, mask), args.reps)
            floor_us, _ = launch_time(metrics_launch(tiny[0], tiny[1], None if mask is None else tiny[2]), args.reps)
            nbytes = H * W * per_pixel
            net = max(us - floor_us, 1e-3)
            res["metrics_launches"][name] = {
                "launches": 2, "device_us": round(us, 2), "spread_us": round(spread, 2),
                "launch_floor_us": round(floor_us, 2), "algorithmic_bytes": nbytes,
                "fraction_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4),
                "fraction_of_hbm_peak_floor_subtracted": round(nbytes / (net * 1e-6) / HBM_PEAK, 4)}
        m.release_plans()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
