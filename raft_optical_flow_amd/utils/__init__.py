from .utils import fb_consistency, ingest_frame  # noqa: F401
