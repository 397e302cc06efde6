from .utils import ingest_frame  # noqa: F401
