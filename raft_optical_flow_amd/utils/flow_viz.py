"""Flow colour-wheel visualisation — drop-in for core/utils/flow_viz.py, on the GPU.

  make_colorwheel    core/utils/flow_viz.py:20-67    the 55-entry Middlebury wheel (host numpy)
  flow_uv_to_colors  :70-106                         (u, v) already normalised -> colours
  flow_to_image      :109-132                        [H,W,2] flow -> uint8 [H,W,3], normalised by its maximum
  flow_to_rgb        (no reference counterpart)      the batched tensor form: [B,2,H,W] -> uint8 [B,H,W,3],
                                                     fixed scale and frame stacking (raft_flow_to_rgb)

All three colouring functions run the one kernel pair of csrc/flow_viz.hip (definition: include/raft_hip.h):
there is one implementation and one set of numerics, in fp32.  Host input is uploaded, coloured and brought
back; there is no host computation path, so a GPU is needed.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .utils import _lib, _stream

# (entries, first colour, moving channel, direction) of the wheel's six segments: red -> yellow -> green ->
# cyan -> blue -> magenta -> red (Baker et al., "A Database and Evaluation Methodology for Optical Flow", 2007)
_SEGMENTS = ((15, (255, 0, 0), 1, 1), (6, (255, 255, 0), 0, -1), (4, (0, 255, 0), 2, 1),
             (11, (0, 255, 255), 1, -1), (13, (0, 0, 255), 0, 1), (6, (255, 0, 255), 2, -1))


def make_colorwheel():
    """The colour wheel as a [55, 3] float64 array (R, G, B in 0..255): entry i of a segment of n entries is
    the segment's first colour with one channel moved by floor(255 * i / n)."""
    rows = []
    for n, start, chan, sign in _SEGMENTS:
        for i in range(n):
            rgb = list(start)
            rgb[chan] += sign * ((255 * i) // n)
            rows.append(rgb)
    return np.asarray(rows, dtype=np.float64)


def check_viz_options(visualize, viz_rad_max):
    """The stream's options as (visualize, viz_rad_max): None / "rgb" / "bgr", None / a positive finite float."""
    if visualize is not None and visualize not in ("rgb", "bgr"):
        raise ValueError(f'visualize must be None, "rgb" or "bgr", got {visualize!r}')
    if viz_rad_max is not None:
        if isinstance(viz_rad_max, bool) or not isinstance(viz_rad_max, (int, float)):
            raise ValueError(f"viz_rad_max must be None or a positive number, got {viz_rad_max!r}")
        if not math.isfinite(viz_rad_max) or viz_rad_max <= 0:
            raise ValueError(f"viz_rad_max must be positive and finite, got {viz_rad_max}")
        viz_rad_max = float(viz_rad_max)
    return visualize, viz_rad_max


def _view(t, h, w):
    """t [B,C,H,W] as (tensor, batch stride, channel stride, pitch): unit element stride and a row pitch that
    holds a row are passed as they are; anything else (a transposed or expanded view) is copied once."""
    if t.stride(3) != 1 and w > 1 or (h > 1 and t.stride(2) < w):
        t = t.contiguous()
    return t, t.stride(0), t.stride(1), (t.stride(2) if h > 1 else w)


def _colour(flow, rad_max, clip_flow, flags, frame):
    """raft_flow_to_rgb on a float32 GPU tensor [B,2,H,W] (any strides) -> uint8 [B,H or 2H,W,3]."""
    L = _lib()
    b, _, h, w = flow.shape
    if b * h * w >= 1 << 30:
        raise ValueError(f"flow_to_rgb: {b} x {h} x {w} pixels exceed 2^30")
    if clip_flow is not None:
        clip_flow = float(clip_flow)
        if math.isnan(clip_flow) or clip_flow < 0:
            raise ValueError(f"clip_flow must not be negative or NaN, got {clip_flow}")
        flags |= L.VIZ_CLIP
    with torch.cuda.device(flow.device):
        f, sb, sc, pitch = _view(flow, h, w)
        fr, fsb, fsc, fpitch = _view(frame, h, w) if frame is not None else (None, 0, 0, 0)
        own_max = rad_max is None and not flags & L.VIZ_UNIT
        ws = torch.empty(L.load().raft_flow_viz_ws_bytes(b, h, w) // 4, device=f.device) if own_max else None
        out = torch.empty(b, 2 * h if fr is not None else h, w, 3, dtype=torch.uint8, device=f.device)
        L.call("raft_flow_to_rgb", f.data_ptr(), sb, sc, pitch, 0, 0, b, h, w, clip_flow or 0.0, rad_max or 0.0, flags,
               fr.data_ptr() if fr is not None else None, fsb, fsc, fpitch,
               ws.data_ptr() if own_max else None, out.data_ptr(), _stream())
    return out


def flow_to_rgb(flow, rad_max=None, clip_flow=None, bgr=False, frame=None):
    """A batch of flow fields as colour images (raft_flow_to_rgb; include/raft_hip.h has the definition).

    flow [B,2,H,W]: float32 on the GPU, any strides: a crop of a padded tensor such as
    up[..., t:-b, l:-r] is read in place.  Returns uint8 [B,H,W,3] on the same device.
      rad_max    None: each image is normalised by its own largest finite flow magnitude, as the reference's
                 flow_to_image does.  A positive number: that magnitude is full saturation in every image
                 (one scale for a whole video; larger flows are drawn at 3/4 brightness).
      clip_flow  clips both components to [0, clip_flow] first (the reference's behaviour, lower bound 0
                 included: negative components vanish)
      bgr        bytes in B, G, R order
      frame      [B,3,H,W] float32 0..255 on the same device: the result is [B,2H,W,3], the frame (rounded to
                 nearest, saturated) above the colours, as demo.py's viz() stacks them
    Pixels whose flow is NaN or infinite are black and do not enter the maximum."""
    L = _lib()
    for name, t, c in (("flow", flow, 2), ("frame", frame, 3)):
        if t is None and name == "frame":
            continue
        if not torch.is_tensor(t):
            raise TypeError(f"flow_to_rgb: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"flow_to_rgb: {name} must be float32, got {t.dtype}")
        if t.dim() != 4 or t.shape[1] != c or t.numel() == 0:
            raise ValueError(f"flow_to_rgb: {name} must be [B, {c}, H, W], got {tuple(t.shape)}")
    if frame is not None and (frame.shape[0], frame.shape[2:]) != (flow.shape[0], flow.shape[2:]):
        raise ValueError(f"flow_to_rgb: flow {tuple(flow.shape)} and frame {tuple(frame.shape)} differ in size")
    _, rad_max = check_viz_options(None, rad_max)
    for name, t in (("flow", flow), ("frame", frame)):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"flow_to_rgb runs on a ROCm GPU only: {name} is on {t.device} (no CPU path)")
    if frame is not None and frame.device != flow.device:
        raise RuntimeError(f"flow_to_rgb: flow is on {flow.device}, frame on {frame.device}")
    return _colour(flow, rad_max, clip_flow, L.VIZ_BGR if bgr else 0, frame)


def _to_device(x):
    """(float32 GPU tensor of x, back): `back` returns a result to where and what x was (numpy array, CPU
    tensor or GPU tensor)."""
    if torch.is_tensor(x):
        if x.is_cuda:
            return x.detach().float(), lambda r: r
        src = x.device
        as_numpy = False
    else:
        x = torch.from_numpy(np.ascontiguousarray(x))
        as_numpy = True
    if not torch.cuda.is_available():
        raise RuntimeError("raft_optical_flow_amd helpers run on a ROCm GPU only (no CPU path)")
    dev = x.detach().float().cuda()
    return dev, (lambda r: r.cpu().numpy()) if as_numpy else (lambda r: r.to(src))


def flow_uv_to_colors(u, v, convert_to_bgr=False):
    """The colour wheel applied to flow components that are already normalised (core/utils/flow_viz.py:70):
    u, v [H,W] (numpy arrays or tensors) -> uint8 [H,W,3] of u's kind.  No maximum and no epsilon: a radius of 1
    is full saturation, larger radii are drawn at 3/4 brightness.  NaN or infinite pixels are black."""
    assert u.ndim == 2 and tuple(u.shape) == tuple(v.shape), "u and v must be [H,W] and of one shape"
    L = _lib()
    du, back = _to_device(u)
    dv, _ = _to_device(v)
    flow = torch.stack([du, dv.to(du.device)])[None]
    return back(_colour(flow, None, None, L.VIZ_UNIT | (L.VIZ_BGR if convert_to_bgr else 0), None)[0])


def flow_to_image(flow_uv, clip_flow=None, convert_to_bgr=False):
    """A flow field [H,W,2] as a colour image uint8 [H,W,3] (core/utils/flow_viz.py:109), normalised by its
    largest magnitude.  A numpy array gives a numpy array, a tensor a tensor on its own device; either way
    the colouring runs on the GPU in fp32 (input of another dtype is converted to float32 first).

    clip_flow clips both components to [0, clip_flow] first.  The lower bound 0 is the reference's
    (np.clip(flow_uv, 0, clip_flow)): it removes every negative component, which is hardly what a caller
    means, and is kept for parity.  NaN or infinite pixels are black and do not enter the maximum (the
    reference's result there is undefined)."""
    assert flow_uv.ndim == 3, 'input flow must have three dimensions'
    assert flow_uv.shape[2] == 2, 'input flow must have shape [H,W,2]'
    L = _lib()
    dev, back = _to_device(flow_uv)
    flow = dev.permute(2, 0, 1)[None].contiguous()
    return back(_colour(flow, None, clip_flow, L.VIZ_BGR if convert_to_bgr else 0, None)[0])
