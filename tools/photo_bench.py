"""Video throughput with every pair scored without ground truth, at config 2 (436x1024 frames, iters=32, B=1):
where the scoring runs, for float32 [1,3,H,W] and for uint8 [1,H,W,3] frames.

    python tools/photo_bench.py [--windows 5] [--window-s 1.0] [--out profiles/photo_bench.json]

A seeded, drifting smooth_images sequence of --frames distinct frames is cycled through (stream_bench.py's).  One
pair ends with the photometric and census sums of (previous frame, current frame, flow_up) added into running
totals on the device; nothing is read back inside a window.
  leg a (torch ops)     stream.push, then utils.warp_frame and the definition of include/raft_hip.h restated in
                        torch: the grey means, two P*P-channel conv2d with an identity kernel for the neighbours,
                        the census features, the soft Hamming distance, the three pow terms, the masked sums
  leg b (PhotoMetrics)  stream.push, then utils.PhotoMetrics.update: two launches
  leg d (push only)     plain stream.push: the ceiling
The legs are warmed up until their graphs are captured, then a, b, d alternate --windows times in one process; a
window is at least --window-s seconds of work and ends in a device synchronise.

The two launches of raft_photo_metrics are timed as bidi_bench.py times the consistency launch: a hipGraph of
--reps repetitions of the call on the last pair between two events; the same graph over an 8 x 8 pair gives the
floor two launches cost in such a graph.  Algorithmic bytes per pixel: both frames (12 B each as float32, 3 B as
uint8) and the flow (8 B) read once, plus the mask where there is one (none here).

Prints ONE JSON line: pairs/s of each leg per window, medians, spreads (max - min), whether leg b's gain over leg
a exceeds the two legs' spreads together, leg b's distance from leg d, the two legs' sums on one pair, and the
launches' time."""
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
from raft_optical_flow_amd.utils import PhotoMetrics, warp_frame  # noqa: E402
from bidi_bench import consistency_time as launch_time  # noqa: E402
from stream_bench import compare, make_frames  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X specification
PATCH = 7


def torch_score(frame1, frame2, flow, patch=PATCH):
    """The record's five sums (l1, photo, hamming, census, ternary) as a float64 device tensor [5], with torch ops:
    utils.warp_frame for W2 and valid, the rest from the definition (outgoing set, no mask)."""
    if frame1.dtype == torch.uint8:
        frame1 = frame1.permute(0, 3, 1, 2).float()
    w2, valid = warp_frame(frame2, flow, out_dtype=torch.float32)
    B, _, H, W = frame1.shape
    r, n = patch // 2, patch * patch
    e = frame1 - w2
    g1 = ((frame1[:, 0] + frame1[:, 1] + frame1[:, 2]) / 3.0)[:, None]
    g2 = ((w2[:, 0] + w2[:, 1] + w2[:, 2]) / 3.0)[:, None]
    eye = torch.eye(n, device=flow.device).view(n, 1, patch, patch)

    def census(g):
        d = F.conv2d(g, eye, padding=r) - g
        return d / torch.sqrt(0.81 + d * d)

    q = (census(g1) - census(g2)) ** 2
    h = (q / (0.1 + q)).sum(dim=1, keepdim=True)
    m = valid.to(torch.float64)
    inner = torch.zeros_like(m)
    inner[..., r:H - r, r:W - r] = 1.0
    mi = m * inner
    return torch.stack([(e.abs() * m).sum(dtype=torch.float64),
                        (torch.pow(e * e + 1e-6, 0.45) * m).sum(dtype=torch.float64),
                        (h * mi).sum(dtype=torch.float64),
                        (torch.pow(h + 0.01, 0.4) * mi).sum(dtype=torch.float64),
                        (torch.pow(h * h + 1e-6, 0.45) * mi).sum(dtype=torch.float64)])


class Leg:
    def __init__(self, model, frames, iters, how):
        self.f, self.t, self.how = frames, 0, how
        self.s = model.stream(iters=iters)
        self.s.push(frames[0])
        self.metrics = PhotoMetrics(patch=PATCH)
        self.acc = torch.zeros(5, dtype=torch.float64, device=frames[0].device)

    def step(self):
        prev = self.f[self.t % len(self.f)]
        self.t += 1
        cur = self.f[self.t % len(self.f)]
        out = self.s.push(cur)
        if self.how == "a":
            self.acc += torch_score(prev, cur, out[1])
        elif self.how == "b":
            self.metrics.update(prev, cur, out[1])
        return out

    def sums(self):
        """The five sums accumulated so far, as a list (a device-to-host copy); clears them."""
        if self.how == "a":
            v = self.acc.cpu().tolist()
            self.acc.zero_()
            return v
        v = self.metrics._totals.cpu().view(torch.float64)[5:10].tolist()
        self.metrics.reset()
        return v

    def close(self):
        self.s.close()


def photo_launch(f1, f2, flow):
    """The raft_photo_metrics call PhotoMetrics.update makes on these device tensors, as a Launch."""
    lib = _lib.load()
    B, _, H, W = flow.shape
    dev = flow.device
    u8 = f1.dtype == torch.uint8
    rec = torch.zeros(B, _lib.PM_SLOTS, dtype=torch.int64, device=dev)
    tot = torch.zeros(_lib.PM_SLOTS, dtype=torch.int64, device=dev)
    ws = torch.zeros(lib.raft_photo_metrics_ws_bytes(B, H, W, PATCH) // 8, dtype=torch.int64, device=dev)
    s1 = (0, 0, 0) if u8 else f1.stride()[:3]
    s2 = (0, 0, 0) if u8 else f2.stride()[:3]
    return Launch("raft_photo_metrics", f1.data_ptr(), *s1, f2.data_ptr(), *s2,
                  _lib.FRAME_U8_NHWC if u8 else _lib.FRAME_F32_NCHW, flow.data_ptr(), *flow.stride()[:3], None, 0, 0, 0,
                  B, H, W, PATCH, _lib.PM_OUTGOING, rec.data_ptr(), tot.data_ptr(), None, ws.data_ptr(),
                  keep=(f1, f2, flow, rec, tot, ws))


def run_legs(m, frames, args):
    H, W = args.height, args.width
    u8 = frames[0].dtype == torch.uint8
    names = {"a": "a_push_torch_ops", "b": "b_push_photo_metrics", "d": "d_push_only"}
    legs = {names[k]: Leg(m, frames, args.iters, k) for k in "abd"}
    r = compare(legs, args.windows, args.window_s)
    a, b, d = (r[names[k]] for k in "abd")
    for leg in legs.values():       # the legs' sums on one and the same pair
        leg.s.reset()
        leg.t = 0
        leg.s.push(frames[0])
        if leg.how != "d":
            leg.sums()
        out = leg.step()
    sa, sb = legs[names["a"]].sums(), legs[names["b"]].sums()
    keys = ("l1_sum", "photo_sum", "hamming_sum", "census_sum", "ternary_sum")
    res = {"results": {"a": dict(zip(keys, sa)), "b": dict(zip(keys, sb)),
                       "max_relative_difference": max(abs(x - y) / max(abs(y), 1e-300) for x, y in zip(sa, sb))}}
    r["b_over_a"] = round(b["median"] / a["median"], 4)
    r["b_gain_over_a_exceeds_spreads"] = bool(b["median"] - a["median"] > a["spread"] + b["spread"])
    r["a_and_b_equal_within_spreads"] = bool(abs(b["median"] - a["median"]) <= a["spread"] + b["spread"])
    r["d_minus_b"] = {"pairs_per_s": round(d["median"] - b["median"], 2), "spread": round(d["spread"] + b["spread"], 2),
                      "ms_per_pair": round(1e3 / b["median"] - 1e3 / d["median"], 4)}
    r["ms_per_pair"] = {k: round(1e3 / r[names[k]]["median"], 4) for k in "abd"}
    res["throughput"] = r
    prev, cur, flow = frames[0], frames[1], out[1].clone()
    us, spread = launch_time(photo_launch(prev, cur, flow), args.reps)
    dev = flow.device
    tiny = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=dev) if u8 else torch.zeros(1, 3, 8, 8, device=dev)
    floor_us, _ = launch_time(photo_launch(tiny, tiny.clone(), torch.zeros(1, 2, 8, 8, device=dev)), args.reps)
    nbytes = H * W * (8 + 2 * (3 if u8 else 12))
    net = max(us - floor_us, 1e-3)
    res["photo_launches"] = {"launches": 2, "patch": PATCH, "device_us": round(us, 2), "spread_us": round(spread, 2),
                             "launch_floor_us": round(floor_us, 2), "algorithmic_bytes": nbytes,
                             "flow_is_contiguous": bool(flow.is_contiguous()),
                             "fraction_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 4),
                             "fraction_of_hbm_peak_floor_subtracted": round(nbytes / (net * 1e-6) / HBM_PEAK, 4),
                             "timed_as": f"hipGraph of {args.reps} calls (2 launches each) between two events; the "
                                         "operands stay in the caches between repetitions"}
    for leg in legs.values():
        leg.close()
    return res


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
    res = {"tool": "photo_bench", "height": args.height, "width": args.width, "iters": args.iters, "batch": 1,
           "patch": PATCH, "precision": m.resolved_precision(), "frames": args.frames, "window_s": args.window_s,
           "pair": "flow + the pair's photometric and census sums added into device totals (leg d: flow only)",
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
