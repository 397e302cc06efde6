"""Shim for core/utils/flow_viz.py -> raft_optical_flow_amd.utils.flow_viz (the colour wheel on the GPU)."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))))
from raft_optical_flow_amd.utils.flow_viz import (  # noqa: E402,F401
    flow_to_image, flow_to_rgb, flow_uv_to_colors, make_colorwheel)
