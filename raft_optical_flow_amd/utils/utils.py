"""Caller-side tensor helpers — drop-in for core/utils/utils.py, on the GPU.

  InputPadder          core/utils/utils.py:7-24   replicate padding to multiples of 8
                                                   (raft_pad_replicate for GPU tensors)
  forward_interpolate  :26-54                      Sintel warm start: nearest forward-splatted
                                                   flow (raft_forward_interpolate, fp64 search)
  bilinear_sampler     :57-71                      grid_sample(align_corners=True) in pixel
                                                   coordinates (raft_bilinear_sample)
  coords_grid          :74-77                      (x, y) pixel grid
  upflow8              :80-82                      8 * bilinear x8 upsampling (raft_upflow8)
  ingest_frame         (no reference counterpart)  InputPadder.pad + RAFT.forward's 2 * (x / 255) - 1
                                                   of one video frame in one launch (raft_ingest_frame)
  fb_consistency       (no reference counterpart)  forward-backward consistency of a flow pair: occlusion
                                                   masks and squared residuals (raft_fb_consistency)
  warp_frame           unflow_loss_pytorch.py:27-80 backward warp of a frame by a flow, float32 or uint8, with
                       IFNET_m.py:7-21              the in-frame mask (raft_warp_frame).  warp_frame(img, flow) is
                       unflow_ops_pytorch.py:88     the reference's image_warp(img, flow) and its
                                                   backward_warp_op(img, -flow); padding="border" is
                                                   IFNET_m.warp(img, flow).  (The reference passes NHWC
                                                   images and flows; here both are NCHW, or uint8 NHWC frames.)
  splat_density        unflow_ops_pytorch.py:6-85   UnFlow's forward-warp density, every contribution summed
                                                   (the reference's indexed `+=` keeps the last write only),
                                                   bitwise reproducible (raft_splat_density)
  flow_errors          evaluate.py:87, :115,       per-sample error statistics of a flow against ground truth, on
                       :148-157                    the device (raft_flow_metrics): the EPE sum, the 1 / 3 / 5 px
                                                   counts, KITTI's outliers, Sintel's speed classes
  FlowMetrics          evaluate.py:75-166          those statistics accumulated over a dataset without a copy or
                                                   a synchronisation per pair: validate_chairs reads "epe",
                                                   validate_sintel "epe", "1px", "3px", "5px", validate_kitti
                                                   "epe_image_mean" and "f1"
  photo_errors         unflow_loss_pytorch.py:247,  per-sample label-free scores of a flow (raft_photo_metrics): frame
                       :411, :612, :694             2 warped back by the flow against frame 1, photometrically and
                       uflow_loss_pytorch.py:609,   under the soft census transform, over the pixels that are neither
                       :880-944                     masked out nor pushed out of the frame: the sums of
                                                   photometric_loss, ternary_loss and census_loss (census_transform,
                                                   soft_hamming, abs_robust_loss, create_outgoing_mask)
  PhotoMetrics         (the same)                  those sums accumulated over a video or a dataset without a copy or
                                                   a synchronisation per pair: "census", "ternary", "photo"
  resize_frame         liteflownet3_util.py:227-232 F.interpolate(mode="bilinear" / "area") of a frame, float32 or
                                                   uint8, with exact integer source coordinates (raft_resize)
  resize_flow          liteflownet3_util.py:227-236 the same of a flow, its vectors scaled by the size ratio in the
                                                   same launch (the reference's is_flow)
  InputScaler          liteflownet3_util.py:121-241 fill: resize to a working size (next multiple of a stride, a given
                                                   size, or a scale factor); unfill: back to the original size

Every helper computes on the GPU through the HIP kernels of libraft_hip.so; a CPU tensor is
copied to the current GPU and the result copied back (there is no host computation path).
Kernels run on the tensor's own device (its current stream), whatever device is current.
"""
from __future__ import annotations

import collections

import torch


def _lib():
    from .. import _lib as L
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _on_device(fn):
    """Run fn(x, ...) with x's GPU current (so launches take that device's current stream);
    CPU inputs go to the current GPU first (inside fn)."""
    import functools

    @functools.wraps(fn)
    def wrapped(x, *args, **kw):
        if torch.is_tensor(x) and x.is_cuda:
            with torch.cuda.device(x.device):
                return fn(x, *args, **kw)
        return fn(x, *args, **kw)
    return wrapped


def _on_gpu(x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        return x
    if not torch.cuda.is_available():
        raise RuntimeError("raft_optical_flow_amd helpers run on a ROCm GPU only (no CPU path)")
    return x.cuda()


class InputPadder:
    """Replicate-pad NCHW images so H and W become multiples of 8: centred ('sintel', the
    default) or all rows at the bottom (any other mode, e.g. 'kitti'); `unpad` crops back.
    `_pad` = [left, right, top, bottom] (F.pad order), as the reference keeps it."""

    def __init__(self, dims, mode="sintel"):
        self.ht, self.wd = int(dims[-2]), int(dims[-1])
        ph, pw = -self.ht % 8, -self.wd % 8
        top = ph // 2 if mode == "sintel" else 0
        self._pad = [pw // 2, pw - pw // 2, top, ph - top]

    def _pad_one(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda:
            with torch.cuda.device(x.device):
                return self._pad_dev(x)
        return self._pad_dev(x)

    def _pad_dev(self, x: torch.Tensor) -> torch.Tensor:
        left, right, top, bottom = self._pad
        src = x
        x = _on_gpu(x).float().contiguous()
        h, w = x.shape[-2:]
        out = torch.empty(*x.shape[:-2], h + top + bottom, w + left + right, device=x.device)
        nc = x.numel() // (h * w)
        _lib().call("raft_pad_replicate", x.data_ptr(), out.data_ptr(), nc, h, w, top, bottom, left, right, _stream())
        return out.to(device=src.device, dtype=src.dtype)

    def pad(self, *inputs):
        return [self._pad_one(x) for x in inputs]

    def unpad(self, x):
        left, right, top, bottom = self._pad
        h, w = x.shape[-2:]
        return x[..., top:h - bottom, left:w - right]


@_on_device
def forward_interpolate(flow):
    """Warm-start flow for the next frame pair (evaluate.py:37-41): each pixel takes the flow of
    the nearest point the flow moves a pixel to, over the points that land strictly inside the
    frame (scipy griddata 'nearest' in the reference; 0 where none lands).  flow [2, H, W] (or
    [B, 2, H, W]) -> float32, same shape, same device.
    Where several such points are at exactly the same smallest distance the one with the lowest source
    index (row-major) is taken; scipy's choice on exact ties is implementation-defined, so only there can
    the result differ from the reference's."""
    f = _on_gpu(flow.detach()).float().contiguous()
    batched = f.dim() == 4
    if not batched:
        f = f[None]
    b, c, h, w = f.shape
    if c != 2:
        raise ValueError(f"flow must be [2, H, W] or [B, 2, H, W], got {tuple(flow.shape)}")
    out = torch.empty_like(f)
    _lib().call("raft_forward_interpolate", f.data_ptr(), out.data_ptr(), b, h, w, _stream())
    out = out if batched else out[0]
    return out.to(flow.device)


@_on_device
def bilinear_sampler(img, coords, mode="bilinear", mask=False):
    """Sample img [N, C, H, W] at pixel coordinates coords [N, Ho, Wo, 2] (x, y): bilinear,
    corners outside the image read 0 (grid_sample align_corners=True).  With mask=True also
    returns the in-range mask [N, Ho, Wo, 1] as float."""
    if mode != "bilinear":
        raise NotImplementedError("bilinear_sampler: only mode='bilinear' is on the RAFT path")
    from .. import kernels as K
    K.require_device(img, coords)
    img = img.contiguous()
    coords = coords.contiguous()
    n, c, h, w = img.shape
    ho, wo = coords.shape[1:3]
    out = torch.empty(n, c, ho, wo, device=img.device)
    m = torch.empty(n, ho, wo, 1, device=img.device) if mask else None
    _lib().call("raft_bilinear_sample", img.data_ptr(), coords.data_ptr(), out.data_ptr(),
                m.data_ptr() if mask else None, n, c, h, w, ho, wo, _stream())
    return (out, m) if mask else out


def coords_grid(batch, ht, wd, device):
    """[batch, 2, ht, wd] float grid: channel 0 = x (column index), channel 1 = y (row index)."""
    x = torch.arange(wd, device=device, dtype=torch.float32).view(1, wd).expand(ht, wd)
    y = torch.arange(ht, device=device, dtype=torch.float32).view(ht, 1).expand(ht, wd)
    return torch.stack([x, y], 0)[None].repeat(batch, 1, 1, 1)


@_on_device
def upflow8(flow, mode="bilinear"):
    """8 * bilinear(align_corners=True) x8 upsampling (raft_upflow8)."""
    from .. import kernels as K
    if mode != "bilinear":
        raise NotImplementedError("upflow8: only mode='bilinear' is on the RAFT path")
    src = flow
    flow = _on_gpu(flow).float()
    n, _, h, w = flow.shape
    coords = (coords_grid(n, h, w, flow.device) + flow).contiguous()
    crow = K.nchw_to_rows(coords)
    out = torch.empty(n, 2, 8 * h, 8 * w, device=flow.device)
    _lib().call("raft_upflow8", crow.data_ptr(), out.data_ptr(), n, h, w, K.stream_handle())
    return out.to(src.device)


def check_fb_params(alpha, beta):
    """(alpha, beta) of the forward-backward check as floats: finite and not negative."""
    import math
    for name, v in (("alpha", alpha), ("beta", beta)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError(f"fb_consistency: {name} must be a number, got {type(v).__name__}")
        if not math.isfinite(v) or v < 0:
            raise ValueError(f"fb_consistency: {name} must be finite and not negative, got {v}")
    return float(alpha), float(beta)


def fb_consistency(flow_fw, flow_bw, alpha=0.01, beta=0.5):
    """Forward-backward consistency of a flow pair (raft_fb_consistency, one launch for both directions).

    flow_fw [B,2,H,W] maps frame 1 to frame 2, flow_bw frame 2 to frame 1: float32 GPU tensors, any strides
    (crops of larger tensors are read in place).  For direction fw, F = flow_fw, G = flow_bw, at pixel x:
    p = x + F(x); p not finite or outside [0, W-1] x [0, H-1]: err = +inf, occ = True; otherwise
    g = bilinear G(p), err = |F(x) + g|^2, occ = err > alpha (|F(x)|^2 + |g|^2) + beta (the UnFlow criterion
    with its published defaults; include/raft_hip.h has the full definition).  Direction bw swaps F and G.
    Returns (occ_fw, occ_bw, err_fw, err_bw): bool and float32 [B,1,H,W]."""
    for what, t in (("flow_fw", flow_fw), ("flow_bw", flow_bw)):
        b, h, w = _check_flow("fb_consistency", t, what)
    if flow_fw.shape != flow_bw.shape:
        raise ValueError(f"fb_consistency: the flows differ in shape: {tuple(flow_fw.shape)} / {tuple(flow_bw.shape)}")
    alpha, beta = check_fb_params(alpha, beta)
    _check_devices("fb_consistency", "flow_fw", flow_fw=flow_fw, flow_bw=flow_bw)
    with torch.cuda.device(flow_fw.device):
        (fw, sfw), (bw, sbw) = _pitched(flow_fw, h, w), _pitched(flow_bw, h, w)
        occ = [torch.empty(b, 1, h, w, dtype=torch.uint8, device=fw.device) for _ in range(2)]
        err = [torch.empty(b, 1, h, w, device=fw.device) for _ in range(2)]
        _lib().call("raft_fb_consistency", fw.data_ptr(), *sfw, bw.data_ptr(), *sbw, 0, 0, b, h, w, alpha, beta,
                    occ[0].data_ptr(), occ[1].data_ptr(), err[0].data_ptr(), err[1].data_ptr(), _stream())
    return occ[0].view(torch.bool), occ[1].view(torch.bool), err[0], err[1]


@_on_device
def ingest_frame(frame, mode="sintel"):
    """The front end of RAFT.stream on its own (raft_ingest_frame): a frame, float32 [B,3,H,W] in
    0..255 or uint8 [B,H,W,3], replicate-padded as InputPadder(mode) pads it.  Returns
    (rows, padded, pad): rows [B*Hp*Wp, 3] = 2 * (padded / 255) - 1 in NHWC order, padded the raw
    float32 [B,3,Hp,Wp] frame, pad = InputPadder._pad ([left, right, top, bottom]).  The results
    stay on the GPU."""
    from .. import engine as E
    tag, b, h, w = E.frame_layout(frame)
    x = _on_gpu(frame).contiguous()
    centred = mode == "sintel"
    pad = E.frame_pad(h, w, centred)
    hp, wp = h + pad[2] + pad[3], w + pad[0] + pad[1]
    rows = torch.empty(b * hp * wp, 3, device=x.device)
    padded = torch.empty(b, 3, hp, wp, device=x.device)
    _lib().call("raft_ingest_frame", x.data_ptr(), tag, b, h, w, int(centred), rows.data_ptr(), padded.data_ptr(),
                _stream())
    return rows, padded, pad


def _check_flow(name, flow, what="flow"):
    """(B, H, W) of a flow (the argument `what`), float32 [B,2,H,W] with fewer than 2^30 pixels; raises otherwise."""
    if not torch.is_tensor(flow):
        raise TypeError(f"{name}: {what} must be a tensor, got {type(flow).__name__}")
    if flow.dtype != torch.float32:
        raise TypeError(f"{name}: {what} must be float32, got {flow.dtype}")
    if flow.dim() != 4 or flow.shape[1] != 2 or flow.numel() == 0:
        raise ValueError(f"{name}: {what} must be [B, 2, H, W], got {tuple(flow.shape)}")
    b, _, h, w = flow.shape
    if b * h * w >= 1 << 30:
        raise ValueError(f"{name}: {b} x {h} x {w} pixels exceed 2^30")
    return b, h, w


def _check_devices(name, anchor="flow", **tensors):
    """Every named tensor (None: absent) is on a GPU, and on the anchor's (one of them)."""
    tensors = {what: t for what, t in tensors.items() if t is not None}
    for what, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on a ROCm GPU only: {what} is on {t.device} (no CPU path)")
    dev = tensors[anchor].device
    for what, t in tensors.items():
        if t.device != dev:
            raise RuntimeError(f"{name}: {what} is on {t.device}, {anchor} on {dev}")


def _check_mask(name, what, mask, b, h, w):
    """A scorer's mask argument `what`: None, or bool / uint8 / float32 [B,H,W] or [B,1,H,W]; raises otherwise."""
    if mask is None:
        return
    if not torch.is_tensor(mask):
        raise TypeError(f"{name}: {what} must be a tensor or None, got {type(mask).__name__}")
    if mask.dtype not in (torch.bool, torch.uint8, torch.float32):
        raise TypeError(f"{name}: {what} must be bool, uint8 or float32, got {mask.dtype}")
    if tuple(mask.shape) not in ((b, h, w), (b, 1, h, w)):
        raise ValueError(f"{name}: {what} must be [B, H, W] or [B, 1, H, W] = {(b, h, w)}, got {tuple(mask.shape)}")


def _pitched(t, h, w):
    """t [B,C,H,W] with unit element stride and a row pitch that holds a row, as (tensor, strides)."""
    if t.stride(3) != 1 and w > 1 or (h > 1 and t.stride(2) < w):
        t = t.contiguous()
    return t, (t.stride(0), t.stride(1), t.stride(2) if h > 1 else w)


WARP_PADDING = ("zeros", "border")


def check_warp_option(warp):
    """RAFT.stream's warp option: None, "zeros" or "border"."""
    if warp is not None and warp not in WARP_PADDING:
        raise ValueError(f'warp must be None, "zeros" or "border", got {warp!r}')
    return warp


def warp_frame(frame, flow, padding="zeros", out_dtype=None):
    """Backward warp (raft_warp_frame, one launch): warped(x) = bilinear frame(x + flow(x)).

    frame is float32 [B,C,H,W] (any C >= 1) or uint8 [B,H,W,3]; flow [B,2,H,W] float32 (channel 0 = x); GPU
    tensors, crops of larger tensors are read in place.  With flow = the flow from frame 1 to frame 2 and
    frame = frame 2, the result is frame 2 aligned with frame 1.  padding="zeros": taps outside the frame read
    0 (grid_sample's zeros with align_corners=True: the reference's image_warp); "border": the position is
    clamped to the frame (IFNET_m.warp).  A pixel whose flow is not finite (or >= 2^30) is 0.
    Returns (warped, valid): warped in the frame's dtype and layout, or out_dtype's (torch.float32:
    [B,C,H,W]; torch.uint8: [B,H,W,3], rounded to nearest even and saturated; C must be 3); valid bool
    [B,1,H,W], True where x + flow(x) lies in [0, W-1] x [0, H-1].  include/raft_hip.h has the definition."""
    L = _lib()
    b, h, w = _check_flow("warp_frame", flow)
    if not torch.is_tensor(frame):
        raise TypeError(f"warp_frame: frame must be a tensor, got {type(frame).__name__}")
    if frame.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"warp_frame: frame must be float32 [B,C,H,W] or uint8 [B,H,W,3], got {frame.dtype}")
    if padding not in WARP_PADDING:
        raise ValueError(f'warp_frame: padding must be "zeros" or "border", got {padding!r}')
    if out_dtype is None:
        out_dtype = frame.dtype
    if out_dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"warp_frame: out_dtype must be None, torch.float32 or torch.uint8, got {out_dtype!r}")
    in_u8, out_u8 = frame.dtype == torch.uint8, out_dtype == torch.uint8
    if frame.dim() != 4:
        raise ValueError(f"warp_frame: frame must be float32 [B, C, H, W] or uint8 [B, H, W, 3], got "
                         f"{tuple(frame.shape)}")
    if in_u8:
        if frame.shape[3] != 3:
            raise ValueError(f"warp_frame: a uint8 frame is [B, H, W, 3], got {tuple(frame.shape)}")
        fb, c, fh, fw = frame.shape[0], 3, frame.shape[1], frame.shape[2]
    else:
        fb, c, fh, fw = frame.shape
    if (fb, fh, fw) != (b, h, w) or c < 1:
        raise ValueError(f"warp_frame: frame {tuple(frame.shape)} and flow {tuple(flow.shape)} differ in size")
    if out_u8 and c != 3:
        raise ValueError(f"warp_frame: a uint8 result needs 3 channels, the frame has {c}")
    _check_devices("warp_frame", frame=frame, flow=flow)
    with torch.cuda.device(flow.device):
        fl, sfl = _pitched(flow, h, w)
        if in_u8:
            fr, sfr = frame.contiguous(), (0, 0, 0)
        else:
            fr, sfr = _pitched(frame, h, w)
        dev = flow.device
        out = torch.empty((b, h, w, 3) if out_u8 else (b, c, h, w), dtype=out_dtype, device=dev)
        valid = torch.empty(b, 1, h, w, dtype=torch.uint8, device=dev)
        L.call("raft_warp_frame", fl.data_ptr(), *sfl, fr.data_ptr(), L.FRAME_U8_NHWC if in_u8 else L.FRAME_F32_NCHW,
               *sfr, 0, 0, b, c, h, w, L.WARP_BORDER if padding == "border" else 0, out.data_ptr(),
               L.FRAME_U8_NHWC if out_u8 else L.FRAME_F32_NCHW, valid.data_ptr(), _stream())
    return out, valid.view(torch.bool)


def splat_density(flow):
    """UnFlow's forward-warp density (raft_splat_density): every pixel x splats its four bilinear weights at
    x + flow(x); the result, float32 [B,1,H,W], is the sum of what lands on each pixel: ~1 where the flow is
    one-to-one, below 1 where nothing arrives (a disocclusion), above 1 where sources pile up.  A source whose
    flow is not finite, or whose target's floor lies outside the frame, contributes nothing; on the last
    column / row both weights land on the edge pixel (the reference's clamp).  The sum is accumulated in
    64-bit fixed point: it does not depend on the order of the adds and is bitwise equal from run to run.
    flow [B,2,H,W] float32 on a GPU, any strides."""
    L = _lib()
    b, h, w = _check_flow("splat_density", flow)
    _check_devices("splat_density", flow=flow)
    with torch.cuda.device(flow.device):
        fl, sfl = _pitched(flow, h, w)
        ws = torch.empty(L.load().raft_splat_ws_bytes(b, h, w) // 8, dtype=torch.int64, device=fl.device)
        out = torch.empty(b, 1, h, w, device=fl.device)
        L.call("raft_splat_density", fl.data_ptr(), *sfl, 0, 0, b, h, w, ws.data_ptr(), out.data_ptr(), _stream())
    return out


RESIZE_MODES = ("bilinear", "area")


def check_size(name, size, what="size"):
    """A target size as (h, w): two positive ints; raises otherwise."""
    if isinstance(size, (str, bytes)) or not hasattr(size, "__len__") or len(size) != 2:
        raise TypeError(f"{name}: {what} must be (height, width), got {size!r}")
    for v in size:
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{name}: {what} must be two ints, got {size!r}")
        if v < 1:
            raise ValueError(f"{name}: {what} must be positive, got {size!r}")
    return int(size[0]), int(size[1])


def check_resize_mode(name, mode, align_corners=False):
    """A resize mode and its align_corners: NotImplementedError for a mode that is not on the GPU path."""
    if mode not in RESIZE_MODES:
        raise NotImplementedError(f'{name}: only the modes "bilinear" and "area" are implemented, got {mode!r}')
    if not isinstance(align_corners, bool):
        raise TypeError(f"{name}: align_corners must be a bool, got {type(align_corners).__name__}")
    if align_corners and mode != "bilinear":
        raise ValueError(f"{name}: align_corners is an option of the bilinear mode, not of {mode!r}")
    return mode, align_corners


def scaled_size(name, height, width, stride=None, size=None, scale_factor=1.0):
    """InputScaler's size arithmetic (liteflownet3_util.py:158-167): the next multiple of `stride`, or `size` as
    given, or int(H * scale_factor), int(W * scale_factor)."""
    import math
    if stride is not None:
        if size is not None:
            raise ValueError(f"{name}: only stride OR size can be provided, not both")
        if isinstance(stride, bool) or not isinstance(stride, int):
            raise TypeError(f"{name}: stride must be an int, got {type(stride).__name__}")
        if stride < 1:
            raise ValueError(f"{name}: stride must be positive, got {stride}")
        return (int(math.ceil(float(height) / stride)) * stride, int(math.ceil(float(width) / stride)) * stride)
    if size is not None:
        return check_size(name, size)
    if isinstance(scale_factor, bool) or not isinstance(scale_factor, (int, float)):
        raise TypeError(f"{name}: scale_factor must be a number, got {type(scale_factor).__name__}")
    if not (0.0 < float(scale_factor) < float("inf")):
        raise ValueError(f"{name}: scale_factor must be positive and finite, got {scale_factor!r}")
    h, w = int(height * scale_factor), int(width * scale_factor)
    if h < 1 or w < 1:
        raise ValueError(f"{name}: scale_factor {scale_factor!r} leaves nothing of a {height} x {width} frame")
    return h, w


def _resize(name, frame, size, mode, align_corners, out_dtype, flow):
    """resize_frame / resize_flow after their own checks of `frame`: one raft_resize launch on frame's device.
    flow: channels 0 and 1 are multiplied by w / W and h / H (each ratio rounded to fp32 once)."""
    L = _lib()
    hd, wd = check_size(name, size)
    mode, align_corners = check_resize_mode(name, mode, align_corners)
    in_u8, out_u8 = frame.dtype == torch.uint8, out_dtype == torch.uint8
    if in_u8:
        b, c, hs, ws = frame.shape[0], 3, frame.shape[1], frame.shape[2]
    else:
        b, c, hs, ws = frame.shape
    if b * c * hs * ws >= 1 << 30 or b * c * hd * wd >= 1 << 30:
        raise ValueError(f"{name}: {b} x {c} x {hs} x {ws} -> {hd} x {wd} exceeds 2^30 elements")
    with torch.cuda.device(frame.device):
        if in_u8:
            fr, sfr = frame.contiguous(), (0, 0, 0)
        else:
            fr, sfr = _pitched(frame, hs, ws)
        out = torch.empty((b, hd, wd, 3) if out_u8 else (b, c, hd, wd), dtype=out_dtype, device=frame.device)
        mul = (float(wd) / ws, float(hd) / hs) if flow else (1.0, 1.0)
        L.call("raft_resize", fr.data_ptr(), L.FRAME_U8_NHWC if in_u8 else L.FRAME_F32_NCHW, *sfr, 0, 0, b, c, hs, ws,
               out.data_ptr(), L.FRAME_U8_NHWC if out_u8 else L.FRAME_F32_NCHW, hd, wd,
               L.RESIZE_AREA if mode == "area" else L.RESIZE_BILINEAR,
               L.RESIZE_ALIGN_CORNERS if align_corners else 0, *mul, _stream())
    return out


def resize_frame(frame, size, mode="bilinear", align_corners=False, out_dtype=None):
    """A frame at another size (raft_resize, one launch): torch.nn.functional.interpolate(frame, size, mode=mode,
    align_corners=align_corners) with exact source coordinates.

    frame is float32 [B,C,H,W] (any C >= 1; a crop of a larger tensor is read in place) or uint8 [B,H,W,3], on a
    GPU; size = (h, w).  mode="bilinear": the source index and the weight of every output sample come out of
    integer arithmetic, so the weight carries one rounding whatever the frame's size (torch forms the coordinate
    in fp32: near column 1900 that costs up to 0.05 on values in 0..255); the blend is IEEE fp32, not fused, and
    every tap is blended, so NaN / Inf spread as in torch.  mode="area": the mean over each output sample's box
    of source samples (adaptive average pooling), summed in fp32 in row-major order; align_corners is a bilinear
    option.  Returns float32 [B,C,h,w] or uint8 [B,h,w,3] (rounded to nearest even and saturated; C must be 3):
    the frame's own dtype and layout, or out_dtype's.  Runs on the frame's device and current stream without
    synchronising.  include/raft_hip.h has the definition."""
    if not torch.is_tensor(frame):
        raise TypeError(f"resize_frame: frame must be a tensor, got {type(frame).__name__}")
    if frame.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"resize_frame: frame must be float32 [B,C,H,W] or uint8 [B,H,W,3], got {frame.dtype}")
    if out_dtype is None:
        out_dtype = frame.dtype
    if out_dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"resize_frame: out_dtype must be None, torch.float32 or torch.uint8, got {out_dtype!r}")
    if frame.dim() != 4 or frame.numel() == 0:
        raise ValueError(f"resize_frame: frame must be float32 [B, C, H, W] or uint8 [B, H, W, 3], got "
                         f"{tuple(frame.shape)}")
    if frame.dtype == torch.uint8 and frame.shape[3] != 3:
        raise ValueError(f"resize_frame: a uint8 frame is [B, H, W, 3], got {tuple(frame.shape)}")
    if out_dtype == torch.uint8 and frame.dtype != torch.uint8 and frame.shape[1] != 3:
        raise ValueError(f"resize_frame: a uint8 result needs 3 channels, the frame has {frame.shape[1]}")
    check_size("resize_frame", size)
    check_resize_mode("resize_frame", mode, align_corners)
    _check_devices("resize_frame", "frame", frame=frame)
    return _resize("resize_frame", frame, size, mode, align_corners, out_dtype, False)


def resize_flow(flow, size, mode="bilinear", align_corners=False):
    """A flow at another size, in that size's pixels (raft_resize, one launch): resize_frame(flow, size, ...) with
    channel 0 (x) multiplied by w / W and channel 1 (y) by h / H in the same launch, each ratio rounded to fp32
    once: the reference's InputScaler with is_flow.  flow is float32 [B,2,H,W] on a GPU, any strides (a padded
    flow_up or InputPadder.unpad's view is read in place); returns float32 [B,2,h,w]."""
    _check_flow("resize_flow", flow)
    check_size("resize_flow", size)
    check_resize_mode("resize_flow", mode, align_corners)
    _check_devices("resize_flow", flow=flow)
    return _resize("resize_flow", flow, size, mode, align_corners, torch.float32, True)


class InputScaler:
    """Scale (..., C, H, W) tensors to a working size and back: the reference's InputScaler, on the GPU.

        scaler = InputScaler(frame.shape, size=(544, 960))
        flow = scaler.unfill(model(scaler.fill(image1), scaler.fill(image2))[-1], is_flow=True)

    The working size is the next multiple of `stride`, or `size` as given, or int(H * scale_factor),
    int(W * scale_factor).  fill resizes to it and unfill back to orig_shape's size, both through raft_resize
    (resize_frame's arithmetic); with is_flow channels 0 and 1 are multiplied by the width and height ratios.
    interpolation_mode is "bilinear" or "area" (anything else raises NotImplementedError).  A CPU tensor goes to
    the current GPU and the result comes back; the result has the input's dtype."""

    def __init__(self, orig_shape, stride=None, size=None, scale_factor=1.0, interpolation_mode="bilinear",
                 interpolation_align_corners=False):
        if len(orig_shape) < 2:
            raise ValueError(f"InputScaler: orig_shape must end in (H, W), got {tuple(orig_shape)}")
        self.orig_height, self.orig_width = check_size("InputScaler", tuple(int(v) for v in orig_shape[-2:]),
                                                       "orig_shape")
        self.interpolation_mode, self.interpolation_align_corners = check_resize_mode(
            "InputScaler", interpolation_mode, interpolation_align_corners)
        self.tgt_height, self.tgt_width = scaled_size("InputScaler", self.orig_height, self.orig_width, stride, size,
                                                      scale_factor)

    def fill(self, x, is_flow=False):
        """x at the working size."""
        return self._scale_keep_dims(x, (self.tgt_height, self.tgt_width), is_flow)

    def unfill(self, x, is_flow=False):
        """x back at the original size."""
        return self._scale_keep_dims(x, (self.orig_height, self.orig_width), is_flow)

    def _scale_keep_dims(self, x, size, is_flow):
        if not torch.is_tensor(x):
            raise TypeError(f"InputScaler: x must be a tensor, got {type(x).__name__}")
        if x.dim() < 3 or x.numel() == 0 or not x.is_floating_point():
            raise ValueError(f"InputScaler: x must be a floating-point (..., C, H, W) tensor, got {x.dtype} "
                             f"{tuple(x.shape)}")
        if is_flow and x.shape[-3] < 2:
            raise ValueError(f"InputScaler: a flow has at least 2 channels, got {tuple(x.shape)}")
        g = _on_gpu(x.detach()).float()
        g = g.reshape(-1, *x.shape[-3:])
        out = _resize("InputScaler", g, size, self.interpolation_mode, self.interpolation_align_corners,
                      torch.float32, bool(is_flow))
        return out.view(*x.shape[:-2], *size).to(device=x.device, dtype=x.dtype)


FlowErrors = collections.namedtuple(
    "FlowErrors", ("n", "n_nonfinite", "n_lt1", "n_lt3", "n_lt5", "n_outlier", "n_s0_10", "n_s10_40", "n_s40",
                   "epe_sum", "epe_sum_s0_10", "epe_sum_s10_40", "epe_sum_s40", "epe_map"))
FlowErrors.__doc__ = """Per-sample error statistics of flow_errors: device tensors [B], the counts int64 and the sums
float64 (include/raft_hip.h names the slots); epe_map float32 [B,1,H,W] or None."""


def _check_metrics_args(name, flow, flow_gt, valid, gt_limit):
    """The type, shape, value and device checks of flow_errors / FlowMetrics.update (no device work): returns
    (b, h, w, gt_limit as a float, 0.0 for none)."""
    b, h, w = _check_flow(name, flow)
    if not torch.is_tensor(flow_gt):
        raise TypeError(f"{name}: flow_gt must be a tensor, got {type(flow_gt).__name__}")
    if flow_gt.dtype != torch.float32:
        raise TypeError(f"{name}: flow_gt must be float32, got {flow_gt.dtype}")
    if tuple(flow_gt.shape) != tuple(flow.shape):
        raise ValueError(f"{name}: flow_gt {tuple(flow_gt.shape)} and flow {tuple(flow.shape)} differ in shape")
    _check_mask(name, "valid", valid, b, h, w)
    limit = _check_gt_limit(name, gt_limit)
    _check_devices(name, flow=flow, flow_gt=flow_gt, valid=valid)
    return b, h, w, limit


def _check_gt_limit(name, gt_limit):
    if gt_limit is None:
        return 0.0
    if isinstance(gt_limit, bool) or not isinstance(gt_limit, (int, float)):
        raise TypeError(f"{name}: gt_limit must be a number or None, got {type(gt_limit).__name__}")
    if not (0.0 < float(gt_limit) < float("inf")):
        raise ValueError(f"{name}: gt_limit must be positive and finite (None: no limit), got {gt_limit!r}")
    return float(gt_limit)


def _mask_args(mask, b, h, w):
    """A mask [B,H,W] or [B,1,H,W] (or None) as the C entries take it: (the tensor that is read, kept alive by the
    caller; (pointer, dtype tag, batch stride, row pitch)), strides in elements."""
    if mask is None:
        return None, (None, 0, 0, 0)
    L = _lib()
    m = mask.reshape(b, h, w) if mask.dim() == 4 else mask
    if m.stride(2) != 1 and w > 1 or (h > 1 and m.stride(1) < w):
        m = m.contiguous()
    tag = L.MASK_F32 if m.dtype == torch.float32 else L.MASK_U8
    return m, (m.data_ptr(), tag, m.stride(0), m.stride(1) if h > 1 else w)


def _record_call(entry, head, size, dev, totals, want_map):
    """One call of a scorer's C entry on device dev (current): head are its arguments up to record, size the
    arguments of its _ws_bytes, (b, h, w) first.  Returns (record int64 [B,16], the per-pixel map or None)."""
    L = _lib()
    b, h, w = size[:3]
    record = torch.empty(b, L.FM_SLOTS, dtype=torch.int64, device=dev)
    ws = torch.empty(getattr(L.load(), entry + "_ws_bytes")(*size) // 8, dtype=torch.int64, device=dev)
    pmap = torch.empty(b, 1, h, w, dtype=torch.float32, device=dev) if want_map else None
    L.call(entry, *head, record.data_ptr(), None if totals is None else totals.data_ptr(),
           None if pmap is None else pmap.data_ptr(), ws.data_ptr(), _stream())
    return record, pmap


def _record_tuple(cls, counts, sums, record, pmap):
    """A scorer's record [B,16] as its namedtuple of [B] views: the counts, the sums as float64, the map."""
    f64, nc = record.view(torch.float64), len(counts)
    return cls(*[record[:, i] for i in range(nc)], *[f64[:, nc + i] for i in range(len(sums))], pmap)


def _named_slots(counts, sums, cnt, val):
    """The 16 slots read as integers (cnt) and as floats (val) -> ({count name: int}, {sum name: float})."""
    return dict(zip(counts, cnt)), {k: val[len(counts) + i] for i, k in enumerate(sums)}


class _RunningTotals:
    """The [16] int64 device totals a scorer's entry adds into (FlowMetrics, PhotoMetrics)."""

    _totals = None

    def _totals_on(self, name, flow):
        """The totals, on flow's device: allocated at the first update."""
        if self._totals is None:
            self._totals = torch.zeros(_lib().FM_SLOTS, dtype=torch.int64, device=flow.device)
        elif self._totals.device != flow.device:
            raise RuntimeError(f"{name}: the totals are on {self._totals.device}, flow on {flow.device}")
        return self._totals

    def reset(self):
        """Clear the totals (no synchronisation)."""
        if self._totals is not None:
            self._totals.zero_()

    def _host(self):
        """The 16 slots as integers and as floats (one device-to-host copy; zeros before the first update)."""
        if self._totals is None:
            n = _lib().FM_SLOTS
            return [0] * n, [0.0] * n
        host = self._totals.cpu()
        return host.tolist(), host.view(torch.float64).tolist()


def _flow_metrics_call(flow, flow_gt, valid, limit, b, h, w, totals, want_map):
    """One raft_flow_metrics call on flow's device (current): (record int64 [B,16], epe_map or None)."""
    fl, sfl = _pitched(flow, h, w)
    gt, sgt = _pitched(flow_gt, h, w)
    v, vargs = _mask_args(valid, b, h, w)
    head = (fl.data_ptr(), *sfl, gt.data_ptr(), *sgt, *vargs, b, h, w, limit)
    return _record_call("raft_flow_metrics", head, (b, h, w), flow.device, totals, want_map)


def flow_errors(flow, flow_gt, valid=None, gt_limit=None, epe_map=False):
    """Error statistics of a flow against ground truth per sample (raft_flow_metrics: one call, two launches, no
    synchronisation): what evaluate.py's validate_* functions compute on the host from `.cpu()` copies.

    flow, flow_gt: float32 [B,2,H,W] GPU tensors of any strides (InputPadder.unpad's view of a padded flow_up is
    read in place).  valid: None, or bool / uint8 (valid where nonzero) / float32 (valid where >= 0.5, as
    validate_kitti's `valid_gt >= 0.5`), [B,H,W] or [B,1,H,W].  gt_limit: None, or ground truth with |gu| or |gv|
    >= gt_limit is invalid (core/datasets.py uses 1000).  Per valid pixel, in IEEE fp32: epe = sqrt(du^2 + dv^2),
    mag = sqrt(gu^2 + gv^2).  Returns a FlowErrors namedtuple of device tensors [B]: int64 counts n, n_nonfinite
    (valid pixels whose epe is not finite: counted in n and there only), n_lt1 / n_lt3 / n_lt5 (epe < 1, 3, 5),
    n_outlier (epe > 3 and epe / mag > 0.05: KITTI's Fl), n_s0_10 / n_s10_40 / n_s40 (Sintel's speed classes on
    mag), float64 sums epe_sum and epe_sum_s0_10 / _s10_40 / _s40, and epe_map (float32 [B,1,H,W], NaN at invalid
    pixels) if asked for, else None.  Bitwise reproducible; include/raft_hip.h has the definition."""
    b, h, w, limit = _check_metrics_args("flow_errors", flow, flow_gt, valid, gt_limit)
    L = _lib()
    with torch.cuda.device(flow.device):
        record, emap = _flow_metrics_call(flow, flow_gt, valid, limit, b, h, w, None, bool(epe_map))
    return _record_tuple(FlowErrors, L.FM_COUNTS, L.FM_SUMS, record, emap)


class FlowMetrics(_RunningTotals):
    """Running error statistics over a dataset, kept on the device: evaluate.py's validate_* loops without the
    per-pair `.cpu()` copy and synchronisation.

        m = FlowMetrics()                        # validate_sintel / validate_chairs
        for ...: m.update(padder.unpad(flow_up), flow_gt)
        r = m.result()                           # r["epe"], r["1px"], r["3px"], r["5px"]

        m = FlowMetrics()                        # validate_kitti
        for ...: m.update(padder.unpad(flow_up), flow_gt, valid_gt)
        r = m.result()                           # r["epe_image_mean"], r["f1"]

    update() takes what flow_errors takes (shapes may change from call to call) and adds into device totals
    without synchronising; result() synchronises once.  gt_limit as in flow_errors."""

    def __init__(self, gt_limit=None):
        self.gt_limit = _check_gt_limit("FlowMetrics", gt_limit)

    def update(self, flow, flow_gt, valid=None):
        b, h, w, _ = _check_metrics_args("FlowMetrics.update", flow, flow_gt, valid, None)
        totals = self._totals_on("FlowMetrics.update", flow)
        with torch.cuda.device(flow.device):
            _flow_metrics_call(flow, flow_gt, valid, self.gt_limit, b, h, w, totals, False)
        return self

    def result(self):
        """The totals as a dict (one device-to-host copy).  epe = epe_sum / n over all valid pixels; "1px", "3px",
        "5px" the shares with epe < 1, 3, 5; f1 = 100 * n_outlier / n; epe_image_mean the mean over images (with
        a valid pixel) of their mean epe; "s0-10", "s10-40", "s40+" the EPE per speed class; pixels, images,
        nonfinite the counts.  A mean over nothing is NaN.  With nonfinite > 0 the means and f1 are NaN (a
        non-finite prediction taints the reference's means in the same way); the shares stay counts over n."""
        L = _lib()
        cnt, sums = self._host()
        c, s = _named_slots(L.FM_COUNTS, L.FM_SUMS, cnt, sums)
        nan = float("nan")
        tainted = c["n_nonfinite"] > 0

        def ratio(a, n, scale=1.0):
            return scale * a / n if n > 0 else nan

        def mean(a, n):
            return nan if tainted else ratio(a, n)

        n, images = c["n"], cnt[L.FM_IMAGES]
        return {"epe": mean(s["epe_sum"], n), "1px": ratio(c["n_lt1"], n), "3px": ratio(c["n_lt3"], n),
                "5px": ratio(c["n_lt5"], n), "f1": nan if tainted else ratio(c["n_outlier"], n, 100.0),
                "epe_image_mean": mean(sums[L.FM_IMAGE_MEAN_SUM], images),
                "s0-10": mean(s["epe_sum_s0_10"], c["n_s0_10"]), "s10-40": mean(s["epe_sum_s10_40"], c["n_s10_40"]),
                "s40+": mean(s["epe_sum_s40"], c["n_s40"]), "pixels": n, "images": images,
                "nonfinite": c["n_nonfinite"]}


PhotoErrors = collections.namedtuple(
    "PhotoErrors", ("n_mask", "n_census", "n_valid", "n_nonfinite", "pixels", "l1_sum", "photo_sum", "hamming_sum",
                    "census_sum", "ternary_sum", "census_map"))
PhotoErrors.__doc__ = """Per-sample label-free scores of photo_errors: device tensors [B], the counts int64 and the
sums float64 (include/raft_hip.h names the slots); census_map float32 [B,1,H,W] or None."""


def _check_photo_args(name, frame1, frame2, flow, mask, patch, outgoing):
    """The type, shape, value and device checks of photo_errors / PhotoMetrics.update (no device work): (b, h, w)."""
    b, h, w = _check_flow(name, flow)
    for what, t in (("frame1", frame1), ("frame2", frame2)):
        if not torch.is_tensor(t):
            raise TypeError(f"{name}: {what} must be a tensor, got {type(t).__name__}")
        if t.dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"{name}: {what} must be float32 [B,3,H,W] or uint8 [B,H,W,3], got {t.dtype}")
    if frame1.dtype != frame2.dtype:
        raise TypeError(f"{name}: the frames differ in dtype: {frame1.dtype} / {frame2.dtype}")
    want = (b, h, w, 3) if frame1.dtype == torch.uint8 else (b, 3, h, w)
    for what, t in (("frame1", frame1), ("frame2", frame2)):
        if tuple(t.shape) != want:
            raise ValueError(f"{name}: {what} must be float32 [B, 3, H, W] or uint8 [B, H, W, 3] of the flow's size "
                             f"{tuple(flow.shape)}, got {t.dtype} {tuple(t.shape)}")
    _check_mask(name, "mask", mask, b, h, w)
    _check_photo_options(name, patch, outgoing)
    _check_devices(name, flow=flow, frame1=frame1, frame2=frame2, mask=mask)
    return b, h, w


def _check_photo_options(name, patch, outgoing):
    if isinstance(patch, bool) or not isinstance(patch, int):
        raise TypeError(f"{name}: patch must be an int, got {type(patch).__name__}")
    if patch not in _lib().PM_PATCHES:
        raise ValueError(f"{name}: patch must be 3, 5 or 7, got {patch}")
    if not isinstance(outgoing, bool):
        raise TypeError(f"{name}: outgoing must be a bool, got {type(outgoing).__name__}")


def _photo_metrics_call(frame1, frame2, flow, mask, patch, outgoing, b, h, w, totals, want_map):
    """One raft_photo_metrics call on flow's device (current): (record int64 [B,16], census_map or None)."""
    L = _lib()
    fl, sfl = _pitched(flow, h, w)
    if frame1.dtype == torch.uint8:
        tag = L.FRAME_U8_NHWC
        (f1, s1), (f2, s2) = (frame1.contiguous(), (0, 0, 0)), (frame2.contiguous(), (0, 0, 0))
    else:
        tag = L.FRAME_F32_NCHW
        (f1, s1), (f2, s2) = _pitched(frame1, h, w), _pitched(frame2, h, w)
    m, margs = _mask_args(mask, b, h, w)
    head = (f1.data_ptr(), *s1, f2.data_ptr(), *s2, tag, fl.data_ptr(), *sfl, *margs, b, h, w, patch,
            L.PM_OUTGOING if outgoing else 0)
    return _record_call("raft_photo_metrics", head, (b, h, w, patch), flow.device, totals, want_map)


def photo_errors(frame1, frame2, flow, mask=None, patch=7, outgoing=True, census_map=False):
    """Label-free scores of a flow per sample (raft_photo_metrics: one call, two launches, no synchronisation):
    frame 2 warped back by the flow against frame 1, photometrically and under the soft census transform.

        out = stream.push(frame)   # bidirectional=True
        utils.photo_errors(prev, frame, out.up_fw, mask=~out.occ_fw)

    frame1, frame2: both float32 [B,3,H,W] in 0..255 or both uint8 [B,H,W,3]; flow: float32 [B,2,H,W] from frame
    1 to frame 2; GPU tensors, float32 crops of larger tensors are read in place.  mask: None, or bool / uint8
    (counted where nonzero) / float32 (where >= 0.5), [B,H,W] or [B,1,H,W]: the pixels to score, ~occlusion for
    instance.  patch: the census patch, 3 (the reference's ternary_loss(max_distance=1)), 5 or 7 (census_loss's
    default).  outgoing: pixels the flow pushes out of the frame do not count (create_outgoing_mask).
    W2 = warp_frame(frame2, flow)'s float32 value bit for bit; e_c = frame1_c - W2_c; h = the soft Hamming
    distance of the two census transforms (include/raft_hip.h has the definition).  Returns a PhotoErrors
    namedtuple of device tensors [B]: int64 counts n_mask (scored pixels), n_census (those at least patch // 2
    from the border), n_valid (in-frame targets, whatever the mask), n_nonfinite (scored pixels with a value that
    is not finite: in no sum), pixels (H W); float64 sums l1_sum (|e_c|), photo_sum ((e_c^2 + 1e-6)^0.45:
    photometric_loss), hamming_sum (h), census_sum ((h + 0.01)^0.4: census_loss's numerator), ternary_sum
    ((h^2 + 1e-6)^0.45: ternary_loss's numerator); and census_map (float32 [B,1,H,W], h at every pixel, a
    confidence image) if asked for, else None.  Bitwise reproducible."""
    b, h, w = _check_photo_args("photo_errors", frame1, frame2, flow, mask, patch, outgoing)
    L = _lib()
    with torch.cuda.device(flow.device):
        record, cmap = _photo_metrics_call(frame1, frame2, flow, mask, patch, outgoing, b, h, w, None,
                                           bool(census_map))
    return _record_tuple(PhotoErrors, L.PM_COUNTS, L.PM_SUMS, record, cmap)


def photo_result(cnt, sums):
    """PhotoMetrics.result()'s dict from the totals' 16 slots read as integers (cnt) and as floats (sums)."""
    L = _lib()
    c, s = _named_slots(L.PM_COUNTS, L.PM_SUMS, cnt, sums)
    nan = float("nan")
    tainted = c["n_nonfinite"] > 0

    def mean(a, n):
        return nan if tainted or n <= 0 else a / n

    images, pixels = cnt[L.PM_IMAGES], c["pixels"]
    return {"census": nan if tainted or pixels <= 0 else s["census_sum"] / (c["n_census"] + 1e-6),
            "ternary": mean(s["ternary_sum"], pixels), "photo": mean(s["photo_sum"], 3 * pixels),
            "l1": mean(s["l1_sum"], 3 * c["n_mask"]), "hamming": mean(s["hamming_sum"], c["n_census"]),
            "census_image_mean": mean(sums[L.PM_IMAGE_CENSUS_MEAN_SUM], images),
            "valid_share": c["n_valid"] / pixels if pixels > 0 else nan, "pixels": pixels, "images": images,
            "nonfinite": c["n_nonfinite"]}


class PhotoMetrics(_RunningTotals):
    """Running label-free scores over a video or a dataset, kept on the device.

        m = PhotoMetrics()
        for frame in video:
            out = stream.push(frame)   # bidirectional=True
            if out is not None: m.update(prev, frame, out.up_fw, mask=~out.occ_fw)
            prev = frame
        r = m.result()                 # r["census"], r["ternary"], r["photo"]

    update() takes what photo_errors takes (shapes may change from call to call) and adds into device totals
    without synchronising; result() synchronises once.  patch and outgoing as in photo_errors."""

    def __init__(self, patch=7, outgoing=True):
        _check_photo_options("PhotoMetrics", patch, outgoing)
        self.patch, self.outgoing = patch, outgoing

    def update(self, frame1, frame2, flow, mask=None):
        b, h, w = _check_photo_args("PhotoMetrics.update", frame1, frame2, flow, mask, self.patch, self.outgoing)
        totals = self._totals_on("PhotoMetrics.update", flow)
        with torch.cuda.device(flow.device):
            _photo_metrics_call(frame1, frame2, flow, mask, self.patch, self.outgoing, b, h, w, totals, False)
        return self

    def result(self):
        """The totals as a dict (one device-to-host copy).  census = census_sum / (n_census + 1e-6), the
        reference's census_loss (0 where pairs were scored but none has an interior pixel, as there); ternary =
        ternary_sum / pixels, ternary_loss's normalisation over all B H W; photo = photo_sum / (3 pixels),
        photometric_loss; l1 the mean |e| per scored pixel and channel; hamming the mean h per scored interior
        pixel; census_image_mean the mean over images (with a scored interior pixel) of census_sum / n_census;
        valid_share = n_valid / pixels; pixels, images, nonfinite the counts.  A mean over nothing is NaN (every
        key before the first update).  With nonfinite > 0 the means are NaN; valid_share stays a count's share."""
        return photo_result(*self._host())
