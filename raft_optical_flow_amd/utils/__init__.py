from .utils import (FlowErrors, FlowMetrics, InputScaler, PhotoErrors, PhotoMetrics, fb_consistency,  # noqa: F401
                    flow_errors, ingest_frame, photo_errors, resize_flow, resize_frame, splat_density, warp_frame)
from .flow_viz import flow_to_image, flow_to_rgb, flow_uv_to_colors, make_colorwheel  # noqa: F401
