from .utils import (FlowErrors, FlowMetrics, fb_consistency, flow_errors, ingest_frame,  # noqa: F401
                    splat_density, warp_frame)
from .flow_viz import flow_to_image, flow_to_rgb, flow_uv_to_colors, make_colorwheel  # noqa: F401
