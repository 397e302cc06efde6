"""The flow colour coding of include/raft_hip.h (raft_flow_to_rgb), restated in fp64 numpy.

This is the project's own restatement of the header's definition, written from the definition: the
non-finite rule, the fixed rad_max, RAFT_VIZ_UNIT and the frame stacking included.  Shared by
tests/test_flow_viz_host.py (held to the reference's recorded bytes) and tests/test_gpu_flow_viz.py (the
kernel is held to it)."""
import numpy as np

SEGMENTS = ((15, (255, 0, 0), 1, 1), (6, (255, 255, 0), 0, -1), (4, (0, 255, 0), 2, 1),
            (11, (0, 255, 255), 1, -1), (13, (0, 0, 255), 0, 1), (6, (255, 0, 255), 2, -1))


def wheel():
    """[55, 3] float64: entry i of a segment of n entries is its first colour with one channel moved by
    floor(255 * i / n)."""
    rows = []
    for n, start, chan, sign in SEGMENTS:
        for i in range(n):
            rgb = list(start)
            rgb[chan] += sign * ((255 * i) // n)
            rows.append(rgb)
    return np.asarray(rows, dtype=np.float64)


def rad_max_of(flow, clip_flow=None):
    """[B] per-image maximum of sqrt(u^2 + v^2) over the pixels with finite u and v (0 if none)."""
    f = np.asarray(flow, dtype=np.float64)
    if clip_flow is not None:
        f = np.clip(f, 0, clip_flow)
    ok = np.isfinite(f[:, 0]) & np.isfinite(f[:, 1])
    with np.errstate(invalid="ignore", over="ignore"):
        rad = np.where(ok, np.sqrt(f[:, 0] ** 2 + f[:, 1] ** 2), 0.0)
    return rad.reshape(len(f), -1).max(axis=1)


def frame_bytes(frame):
    """float [B,3,H,W] -> uint8 [B,H,W,3]: nearest (ties to even), saturated to 0..255, NaN -> 0."""
    x = np.asarray(frame, dtype=np.float64)
    x = np.where(np.isnan(x), 0.0, x)
    return np.rint(np.clip(x, 0.0, 255.0)).astype(np.uint8).transpose(0, 2, 3, 1)


def flow_to_rgb(flow, rad_max=None, clip_flow=None, bgr=False, frame=None, unit=False):
    """flow [B,2,H,W] -> uint8 [B,H,W,3] ([B,2H,W,3] under `frame` [B,3,H,W]), all arithmetic in fp64."""
    f = np.asarray(flow, dtype=np.float64)
    if clip_flow is not None:
        f = np.clip(f, 0, clip_flow)   # NaN stays NaN
    u, v = f[:, 0], f[:, 1]
    ok = np.isfinite(u) & np.isfinite(v)
    if unit:
        den = np.ones(len(f))
    elif rad_max is not None:
        den = np.full(len(f), float(rad_max) + 1e-5)
    else:
        den = rad_max_of(f) + 1e-5
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.where(ok, u, 0.0) / den[:, None, None]
        v = np.where(ok, v, 0.0) / den[:, None, None]
        rad = np.sqrt(u * u + v * v)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * 54
    k0 = np.clip(np.floor(fk), 0, 54).astype(np.int64)
    k1 = (k0 + 1) % 55
    fr = fk - k0
    w = wheel() / 255.0
    col = (1 - fr)[..., None] * w[k0] + fr[..., None] * w[k1]
    col = np.where((rad <= 1)[..., None], 1 - rad[..., None] * (1 - col), 0.75 * col)
    img = np.floor(255 * col).astype(np.uint8)
    img[~ok] = 0
    if frame is not None:
        img = np.concatenate([frame_bytes(frame), img], axis=1)
    return img[..., ::-1].copy() if bgr else img


def flow_to_image(flow_uv, clip_flow=None, convert_to_bgr=False):
    """The reference's flow_to_image ([H,W,2] -> [H,W,3]) through flow_to_rgb."""
    return flow_to_rgb(np.asarray(flow_uv).transpose(2, 0, 1)[None], None, clip_flow, convert_to_bgr)[0]


def compare(got, want):
    """(largest level difference, fraction of PIXELS that differ at all) of two uint8 [..., 3] images."""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int(d.max()), float((d.max(axis=-1) > 0).mean())
