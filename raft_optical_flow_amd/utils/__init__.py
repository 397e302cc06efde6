from .utils import fb_consistency, ingest_frame, splat_density, warp_frame  # noqa: F401
from .flow_viz import flow_to_image, flow_to_rgb, flow_uv_to_colors, make_colorwheel  # noqa: F401
