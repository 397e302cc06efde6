"""Generate tests/golden/photo_reference.npz by running the REFERENCE's label-free losses.

Runs only where the reference snapshot is present (RAFT_REFERENCE, default /root/reference).  It imports the
reference's unflow_loss_pytorch (ternary_loss, photometric_loss, create_outgoing_mask) and uflow_loss_pytorch
(census_loss) at generation time, feeds them the seeded case of tests/photo_metrics_oracle.py (photo_case(2, 37,
53): integer frames in 0..255, a smooth flow plus Gaussian noise of 2.5 px, a mask) and stores the inputs and the
losses.  The reference takes NHWC images in 0..1 and the second frame already warped: it is handed frame 1 / 255
and the oracle's W2 / 255 (rounded to fp32), with mask * create_outgoing_mask(flow) as its mask.  With each loss
the measured relative distance to the oracle's value (photo_metrics_oracle.result(totals(metrics(...)))) is
stored, and whether create_outgoing_mask equalled the oracle's `valid` on every pixel.  No reference source is
copied: the fixture is numbers only, and nothing at test time reads the reference.

    python tests/golden/make_golden_photo.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RAFT_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))            # tests/: the seeded case and the oracle


def main():
    import uflow_loss_pytorch as UF      # the reference's
    import unflow_loss_pytorch as UN     # the reference's
    import photo_metrics_oracle as O

    f1, f2, flow, mask = O.photo_case(2, 37, 53)
    out = {"frame1": f1, "frame2": f2, "flow": flow, "mask": mask}
    w2, valid = O.warp(O.as_nchw(f2), flow)
    nhwc = lambda a: torch.from_numpy(np.array(a)).permute(0, 2, 3, 1).contiguous()  # noqa: E731
    im1 = nhwc(f1) / 255.0
    im2w = nhwc(w2.astype(np.float32)) / 255.0
    with torch.no_grad():
        outgoing = UN.create_outgoing_mask(nhwc(flow))
        out["outgoing_equals_valid"] = np.bool_(np.array_equal(outgoing[..., 0].numpy() > 0.5, valid))
        m = torch.from_numpy(np.array(mask))[..., None] * outgoing
        ref = {"ternary_p3": UN.ternary_loss(im1, im2w, m, max_distance=1),
               "census_p7": UF.census_loss(im1, im2w, m, patch_size=7),
               "census_p3": UF.census_loss(im1, im2w, m, patch_size=3),
               "photo": UN.photometric_loss(im1 - im2w, m)}
    want = {}
    for patch in (3, 7):
        r = O.result(O.totals(O.metrics(f1, f2, flow, mask, patch=patch)))
        want[f"census_p{patch}"] = r["census"]
        want[f"ternary_p{patch}"] = r["ternary"]
        want["photo"] = r["photo"]
    for k, v in ref.items():
        v = float(v)
        out[k] = np.float64(v)
        out["ref_dist_" + k] = np.float64(abs(v - want[k]) / abs(want[k]))
        print(f"{k}: reference {v:.9g}, oracle {want[k]:.9g}, relative distance {out['ref_dist_' + k]:.3e}")
    print(f"create_outgoing_mask == valid everywhere: {bool(out['outgoing_equals_valid'])}, valid share "
          f"{valid.mean():.3f}")
    path = os.path.join(HERE, "photo_reference.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} KB)")


if __name__ == "__main__":
    main()
