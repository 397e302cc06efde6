"""Generate tests/golden/resize_reference.npz by running the REFERENCE's InputScaler.

Runs only where the reference snapshot is present (RAFT_REFERENCE, default /root/reference).  It imports the
reference's liteflownet3_util.InputScaler at generation time and runs fill / unfill on the seeded case of
tests/resize_oracle.py (golden_case: a 2 x 3 x 37 x 53 frame of noise in 0..255 and a 2 x 2 x 37 x 53 flow), to
the sizes (19, 27) and (40, 56) and to stride 8, on float32 CPU tensors, and stores the inputs and the float32
outputs.  Stride 8 resolves to (40, 56): its outputs are checked here to equal that size's bit for bit and are
stored once, with the size the stride gave.  To stay under 200 KB, unfill is stored for the flow (where is_flow's
multipliers run the other way) and not for the frame, which takes the same path as fill with the sizes swapped.
With each output it stores the measured maximum distance to the fp64 definition (tests/resize_oracle.py:
resize_ref): the reference goes through F.interpolate, which forms the source coordinate in fp32.  No reference
source is copied: the fixture is numbers only, and nothing at test time reads the reference.

    python tests/golden/make_golden_resize.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RAFT_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))            # tests/: the seeded case and the definition

# name -> InputScaler's keyword
TARGETS = {"s19x27": dict(size=(19, 27)), "s40x56": dict(size=(40, 56)), "stride8": dict(stride=8)}


def main():
    from liteflownet3_util import InputScaler     # the reference's
    import resize_oracle as O

    frame, flow = O.golden_case()
    out = {"frame": frame, "flow": flow}
    runs = {}
    for name, kw in TARGETS.items():
        sc = InputScaler(frame.shape, **kw)
        size = (sc.tgt_height, sc.tgt_width)
        out[name + "_size"] = np.array(size, dtype=np.int64)
        for what, x, is_flow in (("frame", frame, False), ("flow", flow, True)):
            with torch.no_grad():
                small = sc.fill(torch.from_numpy(x).clone(), is_flow=is_flow)
                back = sc.unfill(small.clone(), is_flow=is_flow).numpy()
                small = small.numpy()
            m_fill = O.flow_muls((37, 53), size) if is_flow else (1.0, 1.0)
            m_back = O.flow_muls(size, (37, 53)) if is_flow else (1.0, 1.0)
            # unfill is checked on its own: from the reference's stored fill output, not from the definition's
            for tag, got, src, tgt, m in (("fill", small, x, size, m_fill), ("unfill", back, small, (37, 53), m_back)):
                ref = O.resize_ref(src, tgt, "bilinear", False, *m)
                key = f"{name}_{what}_{tag}"
                runs[key] = got.astype(np.float32)
                if name == "stride8" or (what, tag) == ("frame", "unfill"):
                    continue
                out[key] = runs[key]
                out["ref_dist_" + key] = np.float64(np.abs(got.astype(np.float64) - ref).max())
                print(f"{key}: {got.shape}, max |reference - fp64 definition| = {out['ref_dist_' + key]:.3e}")
    for key, got in runs.items():
        if key.startswith("stride8_"):
            assert tuple(out["stride8_size"]) == (40, 56) and np.array_equal(got, runs["s40x56_" + key[8:]]), key
    path = os.path.join(HERE, "resize_reference.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} KB)")


if __name__ == "__main__":
    main()
