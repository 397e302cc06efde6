"""fp64 references for the elementwise, norm-apply, upsample, layout and caller-side kernels.

Written from the reference project's formulas (core/raft.py, core/utils/utils.py, core/extractor.py) and the
comments of include/raft_hip.h, never from the kernel sources.  Rows are the library's NHWC layout: a tensor
[B, HW, C] here is the C used columns of [B*HW][ld] there.  Shared by tests/test_elementwise_oracle_host.py
(this file is held to torch and to oracle/raft_oracle.py on the CPU) and by the GPU tests (the kernels are held
to it)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import raft_oracle as O

U = 2.0 ** -24   # unit roundoff of fp32 (round to nearest)


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ----------------------------------------------------------------------------- norms


def _normalise(x, stats, gamma, beta, mags):
    """(x - mean) * rstd (* gamma) (+ beta) per (image, channel); every intermediate's magnitude goes to mags."""
    v = f64(x) - f64(stats)[:, None, :, 0]
    mags.append(np.abs(v))
    v = v * f64(stats)[:, None, :, 1]
    mags.append(np.abs(v))
    if gamma is not None:
        v = v * f64(gamma)
        mags.append(np.abs(v))
    if beta is not None:
        v = v + f64(beta)
        mags.append(np.abs(v))
    return v


def norm_apply(x, stats, mode, resid=None, resid_stats=None, gamma=None, beta=None, resid_gamma=None,
               resid_beta=None):
    """include/raft_hip.h, raft_instnorm_apply / raft_norm_apply_affine: out = act(norm(x) + resid).

    x, resid [B, HW, C]; stats, resid_stats [B, C, 2] = {mean, rstd}; gamma / beta [C] or None (1 / 0).
    norm(x) = (x - mean) * rstd * gamma + beta; resid is absent, raw, or norm(resid) with resid_stats (and
    resid_gamma / resid_beta, which apply only then); mode 0: none, 1: relu(norm(x)) before the residual,
    2: relu(resid + relu(norm(x))).  Returns (out, mag), both fp64 [B, HW, C]: mag is, per element, the largest
    magnitude of any intermediate on its path (what a derived fp32 rounding bound scales with)."""
    assert mode in (0, 1, 2)
    mags = []
    v = _normalise(x, stats, gamma, beta, mags)
    if mode >= 1:
        v = np.maximum(v, 0.0)
    if resid is not None:
        r = f64(resid)
        mags.append(np.abs(r))
        if resid_stats is not None:
            r = _normalise(resid, resid_stats, resid_gamma, resid_beta, mags)
        v = r + v
        mags.append(np.abs(v))
        if mode == 2:
            v = np.maximum(v, 0.0)
    return v, np.maximum.reduce(mags)


def groupnorm_stats(x, groups, eps=1e-5):
    """nn.GroupNorm's statistics (core/extractor.py:23-25): biased mean / variance over each group of C / G
    consecutive channels x HW pixels, per image.  x [B, HW, C] -> (mean, rstd), each [B, C], every channel
    carrying its group's pair (groups == C is nn.InstanceNorm2d)."""
    x = f64(x)
    b, hw, c = x.shape
    assert c % groups == 0
    g = x.reshape(b, hw, groups, c // groups)
    mean = g.mean(axis=(1, 3))
    var = ((g - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    rstd = 1.0 / np.sqrt(var + eps)
    rep = c // groups
    return np.repeat(mean, rep, axis=1), np.repeat(rstd, rep, axis=1)


# ----------------------------------------------------------------------------- upsampling


def flow_of_coords(coords):
    """What the upsample kernels see: float32(coords - grid), coords NCHW float32 [B, 2, H, W]."""
    coords = np.asarray(coords, dtype=np.float32)
    b, _, h, w = coords.shape
    return (coords - O.coords_grid(b, h, w)).astype(np.float32)


def mask_nchw(mask_rows, b, h, w):
    """mask rows [B*H*W][>= 576] -> the reference's [B, 576, H, W]."""
    return np.ascontiguousarray(np.asarray(mask_rows)[:, :576].reshape(b, h, w, 576).transpose(0, 3, 1, 2))


def upsample_flow(flow, mask, dtype=np.float64):
    """RAFT.upsample_flow (core/raft.py:112-142) through oracle.raft_oracle.upsample_flow, in `dtype`."""
    return O.upsample_flow(np.asarray(flow, dtype=dtype), np.asarray(mask, dtype=dtype))


def upflow8(flow):
    """core/utils/utils.py:80-82 on doubles: 8 * F.interpolate(size=(8H, 8W), bilinear, align_corners=True)."""
    f = torch.from_numpy(f64(flow))
    size = (8 * f.shape[2], 8 * f.shape[3])
    return (8 * F.interpolate(f, size=size, mode="bilinear", align_corners=True)).numpy()


def upflow8_torch(flow, dtype):
    """upflow8 (core/utils/utils.py:80-82) as plain torch ops in `dtype` on flow's device, operation for operation
    oracle.raft_oracle.upflow8 (so float32 here is the reference's float32 arithmetic and float64 the high-
    precision reference): for maps too large for a numpy reference.  flow [B, 2, H, W] -> [B, 2, 8H, 8W]."""
    f = flow.to(dtype)
    h, w = f.shape[-2:]
    H, W = 8 * h, 8 * w
    sy = (h - 1) / (H - 1) if H > 1 else 0.0
    sx = (w - 1) / (W - 1) if W > 1 else 0.0
    yy = torch.arange(H, device=f.device, dtype=dtype) * torch.tensor(sy, dtype=dtype, device=f.device)
    xx = torch.arange(W, device=f.device, dtype=dtype) * torch.tensor(sx, dtype=dtype, device=f.device)
    y0 = torch.clamp(torch.floor(yy).long(), max=h - 1)
    x0 = torch.clamp(torch.floor(xx).long(), max=w - 1)
    y1 = torch.clamp(y0 + 1, max=h - 1)
    x1 = torch.clamp(x0 + 1, max=w - 1)
    ly = (yy - y0.to(dtype))[:, None]
    lx = (xx - x0.to(dtype))[None, :]
    top = f[:, :, y0][:, :, :, x0] * (1 - lx) + f[:, :, y0][:, :, :, x1] * lx
    bot = f[:, :, y1][:, :, :, x0] * (1 - lx) + f[:, :, y1][:, :, :, x1] * lx
    return 8 * (top * (1 - ly) + bot * ly)


def upsample_flow_torch(flow, mask_rows, dtype, chunk=1 << 16):
    """RAFT.upsample_flow (core/raft.py:112-142) as plain torch ops in `dtype` on the inputs' device, a chunk of
    pixels at a time (the softmax of a large mask in fp64 would not fit beside it).  flow [B, 2, H, W], mask_rows
    [B*H*W][>= 576] (channel k*64 + a*8 + b) -> [B, 2, 8H, 8W]."""
    b, _, h, w = flow.shape
    n = b * h * w
    nb = F.unfold(8 * flow.to(dtype), [3, 3], padding=1).view(b, 2, 9, h * w).permute(0, 3, 1, 2).reshape(n, 2, 9)
    out = torch.empty(n, 2, 64, dtype=dtype, device=flow.device)
    for s in range(0, n, chunk):
        m = torch.softmax(mask_rows[s:s + chunk, :576].to(dtype).view(-1, 9, 64), dim=1)
        for c in range(2):
            out[s:s + chunk, c] = (m * nb[s:s + chunk, c, :, None]).sum(1)
    return out.view(b, h, w, 2, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(b, 2, 8 * h, 8 * w)


def measured_bound(ref32, ref64, floor):
    """The measured tolerance of the issue: 4 x the reference's own fp32 error against fp64 (E_ref), not below
    `floor`.  Returns (bound, E_ref).  Positions where either is not finite are left out."""
    a, b = f64(ref32), f64(ref64)
    ok = np.isfinite(a) & np.isfinite(b)
    e_ref = float(np.abs(a - b)[ok].max()) if ok.any() else 0.0
    return max(4.0 * e_ref, floor), e_ref


# ----------------------------------------------------------------------------- layout


def avg_pool2(x):
    """F.avg_pool2d(x, 2, stride=2) (floor) over the last two dims, fp64 (oracle.raft_oracle.avg_pool2)."""
    return O.avg_pool2(f64(x))


def avg_pool2_rows_fp32(x):
    """NHWC [B, H, W, C] float32 -> [B, H//2, W//2, C]: (((a + b) + c) + d) / 4 in fp32, a b / c d the 2 x 2
    window in row-major order."""
    x = np.asarray(x, dtype=np.float32)
    h, w = x.shape[1] // 2, x.shape[2] // 2
    x = x[:, :2 * h, :2 * w]
    a, b, c, d = x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]
    return (((a + b) + c) + d) / np.float32(4)


def prep_images(img1, img2):
    """core/raft.py:164-169 in fp64: 2 * (x / 255) - 1, NCHW [B,3,H,W] x 2 -> NHWC rows [2B*H*W, 3], image1's
    batch first."""
    x = np.concatenate([f64(img1), f64(img2)], 0)
    return (2.0 * (x / 255.0) - 1.0).transpose(0, 2, 3, 1).reshape(-1, 3)


# ----------------------------------------------------------------------------- caller side


def bilinear_sampler(img, coords, dtype=torch.float64):
    """core/utils/utils.py:57-71 on the CPU in `dtype`: the reference's normalisation 2 c / (S - 1) - 1, then
    F.grid_sample(align_corners=True, padding_mode='zeros'), and its mask.  img [N,C,H,W], coords [N,Ho,Wo,2]
    (x, y) float32 -> (out [N,C,Ho,Wo], mask [N,Ho,Wo,1]) as numpy."""
    im = torch.from_numpy(np.asarray(img, dtype=np.float32)).to(dtype)
    c = torch.from_numpy(np.asarray(coords, dtype=np.float32)).to(dtype)
    h, w = im.shape[-2:]
    xg, yg = c.split([1, 1], dim=-1)
    xg = 2 * xg / (w - 1) - 1
    yg = 2 * yg / (h - 1) - 1
    out = F.grid_sample(im, torch.cat([xg, yg], dim=-1), mode="bilinear", padding_mode="zeros", align_corners=True)
    m = (xg > -1) & (yg > -1) & (xg < 1) & (yg < 1)
    return out.numpy(), m.float().numpy()


def nearest_sources(flow):
    """The brute-force form of forward_interpolate's search (core/utils/utils.py:26-54), in fp64.

    flow [2, H, W] float32.  Source s = grid point (x, y) moved to (x + dx, y + dy) in fp64; it takes part when it
    lands strictly inside (0, W) x (0, H) (a NaN or Inf flow never does).  For every target grid point, in
    row-major order: (dmin [HW] the smallest squared distance (inf with no source), members bool [HW targets,
    HW sources] the sources at exactly that distance, lowest [HW] the lowest index of that set (-1 if empty))."""
    flow = np.asarray(flow, dtype=np.float32)
    _, h, w = flow.shape
    ys, xs = np.mgrid[0:h, 0:w]
    xt, yt = f64(xs).ravel(), f64(ys).ravel()
    with np.errstate(invalid="ignore"):
        x1, y1 = xt + f64(flow[0]).ravel(), yt + f64(flow[1]).ravel()
        valid = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    n = h * w
    d = np.full((n, n), np.inf)
    d[:, valid] = (x1[valid][None, :] - xt[:, None]) ** 2 + (y1[valid][None, :] - yt[:, None]) ** 2
    dmin = d.min(axis=1)
    members = (d == dmin[:, None]) & valid[None, :]
    lowest = np.where(members.any(axis=1), members.argmax(axis=1), -1)
    return dmin, members, lowest


def forward_interpolate_lowest(flow):
    """forward_interpolate with the library's documented tie rule: every target takes the flow of the lowest
    index among its nearest sources, 0 with none.  flow [2, H, W] float32 -> the same shape."""
    flow = np.asarray(flow, dtype=np.float32)
    _, _, lowest = nearest_sources(flow)
    src = flow.reshape(2, -1)
    out = np.where(lowest[None, :] >= 0, src[:, np.maximum(lowest, 0)], np.float32(0))
    return out.reshape(flow.shape).astype(np.float32)
