"""Generate tests/golden/flow_viz.npz by running the REFERENCE's core/utils/flow_viz.py.

Runs only where the reference snapshot is present (RAFT_REFERENCE, default /root/reference).  It imports the
reference's flow_viz at generation time, feeds it seeded inputs and stores inputs and its uint8 outputs.  No
reference source is copied: the fixture is numbers only, and nothing at test time reads the reference.

    python tests/golden/make_golden_viz.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("RAFT_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "core"))

H, W = 37, 53


def fields():
    """[3, 2, H, W] float32: normal x 5 noise, a smooth sinusoid field, a rotation about the centre."""
    rng = np.random.default_rng(20)
    y, x = np.mgrid[:H, :W].astype(np.float64)
    noise = rng.standard_normal((2, H, W)) * 5
    sine = np.stack([7 * np.sin(x / 9.0) * np.cos(y / 7.0) + 2, 5 * np.cos(x / 11.0 + y / 5.0) - 1])
    rot = np.stack([-(y - (H - 1) / 2) * 0.4, (x - (W - 1) / 2) * 0.4])
    return np.stack([noise, sine, rot]).astype(np.float32)


def chart():
    """[2, 64, 64] float32: u = x - 32, v = y - 32: every wheel segment, both axes and the zero vector."""
    y, x = np.mgrid[:64, :64]
    return np.stack([x - 32, y - 32]).astype(np.float32)


def main():
    from utils import flow_viz as R   # the reference's core/utils/flow_viz.py

    f, c = fields(), chart()
    hwc = lambda a: np.ascontiguousarray(a.transpose(1, 2, 0))  # noqa: E731
    out = {"wheel": R.make_colorwheel(), "flows": f, "chart": c}
    out["img_flows"] = np.stack([R.flow_to_image(hwc(a)) for a in f])
    out["img_chart"] = R.flow_to_image(hwc(c))
    out["img_clip3"] = R.flow_to_image(hwc(f[1]), clip_flow=3.0)
    out["img_bgr"] = R.flow_to_image(hwc(f[0]), convert_to_bgr=True)
    # flow_uv_to_colors on components that are not normalised to the unit disc: a rotation about an off-grid
    # centre, radii up to ~3.  The colour has two kinds of discontinuity, and a fixture pixel on one of them tests
    # nothing but the last rounding of whichever arithmetic evaluates it (the reference mixes fp32 and fp64):
    #   - radius 1 (full colour inside, 3/4 brightness outside): with a grid-centred rotation the 3-4-5 points
    #     have radius exactly 1 in fp32 and 1 + 2e-8 in fp64;
    #   - floor(255 * col) where 255 * col is an integer in exact arithmetic: outside the unit disc, directions
    #     at exact multiples of 45 degrees give such values (fk = 47.25: 0.75 * (0.75 * 215 + 0.25 * 235) = 165),
    #     and a grid-centred rotation puts a whole row and a whole diagonal of pixels there.
    # The off-grid centre keeps every pixel away from both; the two asserts hold the fixture to that.
    y, x = np.mgrid[:H, :W].astype(np.float64)
    uv = (np.stack([-(y - 17.37), x - 25.61]) * 0.4 / 3.7).astype(np.float32)
    uv64 = uv.astype(np.float64)
    assert np.abs(np.sqrt((uv64 ** 2).sum(0)) - 1).min() > 1e-4 and np.sqrt((uv64 ** 2).sum(0)).max() > 2
    au, av = np.abs(uv64[0]), np.abs(uv64[1])
    assert min(au.min(), av.min(), np.abs(au - av).min()) > 1e-3     # no direction at a multiple of 45 degrees
    out["uv"] = uv
    out["img_uv"] = R.flow_uv_to_colors(uv[0], uv[1])
    path = os.path.join(HERE, "flow_viz.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} KB)")


if __name__ == "__main__":
    main()
