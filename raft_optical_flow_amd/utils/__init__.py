from .utils import (FlowErrors, FlowMetrics, PhotoErrors, PhotoMetrics, fb_consistency,  # noqa: F401
                    flow_errors, ingest_frame, photo_errors, splat_density, warp_frame)
from .flow_viz import flow_to_image, flow_to_rgb, flow_uv_to_colors, make_colorwheel  # noqa: F401
