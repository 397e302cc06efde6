"""Generate tests/golden/warp_reference.npz by running the REFERENCE's frame warps.

Runs only where the reference snapshot is present (RAFT_REFERENCE, default /root/reference).  It imports the
reference's unflow_loss_pytorch.image_warp and IFNET_m.warp at generation time, feeds them the seeded case of
tests/test_warp_host.py (warp_case(2, 37, 53): values in 0..255, a smooth flow of up to about 9 px, noise on
image 1) and stores the inputs and their float32 outputs.  With each output it stores the measured maximum
distance to the fp64 restatement of the definition (tests/test_warp_host.py: warp_reference): the reference
goes through grid_sample's normalised grid, 2 x / (W - 1) - 1 and back, in fp32, which costs about 1e-3 on
values in 0..255.  No reference source is copied: the fixture is numbers only, and nothing at test time
reads the reference.

No density is stored: the reference's forward_warp_op adds with an indexed `+=`, which keeps one write per
target pixel instead of the sum its docstring describes (tests/test_warp_host.py pins the sum analytically).

    python tests/golden/make_golden_warp.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RAFT_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))            # tests/: the seeded case and the restatement
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    import IFNET_m                      # the reference's
    import unflow_loss_pytorch as R     # the reference's
    from test_warp_host import warp_case, warp_reference

    frame, flow = warp_case(2, 37, 53)
    out = {"frame": frame, "flow": flow}
    nhwc = lambda a: torch.from_numpy(a).permute(0, 2, 3, 1).contiguous()  # noqa: E731
    with torch.no_grad():
        zeros = R.image_warp(nhwc(frame), nhwc(flow)).permute(0, 3, 1, 2).contiguous().numpy()
        border = IFNET_m.warp(torch.from_numpy(frame), torch.from_numpy(flow)).numpy()
    for name, got, mode in (("zeros", zeros, False), ("border", border, True)):
        d = warp_reference(frame, flow, mode)
        out["warp_" + name] = got.astype(np.float32)
        out["ref_dist_" + name] = np.float64(np.abs(got.astype(np.float64) - d["value"]).max())
        print(f"{name}: max |reference - fp64 restatement| = {out['ref_dist_' + name]:.3e}, "
              f"valid share {d['valid'].mean():.3f}")
    path = os.path.join(HERE, "warp_reference.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} KB)")


if __name__ == "__main__":
    main()
