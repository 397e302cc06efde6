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


# ----------------------------------------------------------------------------- encoder InstanceNorm from the convs
#
# include/raft_hip.h, raft_conv2d_stats_slots ("Slot footprints") and the raft_instnorm_merge* comments, restated
# in torch (any device): which output pixels each statistics slot holds, the (count, mean, M2) partials by their
# definition in fp64, the documented float32 algorithm (per slot an fp32 sum, the mean, M2 about that mean; Chan's
# merge in fp64), the pooled statistics by definition, and the comparisons the GPU tests assert with
# (tests/test_encoder_norm_host.py holds these to each other and shows that the comparisons reject wrong references).

STATS_EPS = 1e-5
# The bounds of the merged statistics on the GPU: 4 x the largest error of the float32 restatement below against
# fp64 over every ENC_TABLE shape, precision-independent data condition and image (measured by
# test_encoder_norm_host.py::test_restated_statistics_against_fp64, recorded in DESIGN.md): the mean relative to
# the channel's max |v| in its image, rstd relative.  Measured: E_mean 5.61e-7 (the constant channel on 16-row
# tiles: 64 equal float32 values summed in a row round the same way at every step), E_rstd 3.51e-7 (the channel
# whose bias is 30 deviations, 1x1 8 -> 32 at 2 x 10 x 14); rounded up here.  Bounds: 2.28e-6 and 1.44e-6.
ENC_STATS_MEASURED = {"mean": 5.7e-7, "rstd": 3.6e-7}
ENC_STATS_MARGIN = 4.0


def stats_slot_ids(kind, tile_rows, ho, wo, device="cpu"):
    """The slot (within its image) of every output pixel, row-major [ho * wo] int64, and the slots per image.
    kind "halo" / "stem": tiles of tile_rows x 16, slot 4 * tile + wave, wave = tile_rows / 4 rows of the tile;
    "gemm": 64-pixel tiles of the flat image, slot 2 * tile + half."""
    pix = torch.arange(ho * wo, device=device)
    if kind == "gemm":
        return 2 * (pix // 64) + (pix % 64) // 32, 2 * (-(-(ho * wo) // 64))
    assert kind in ("halo", "stem") and tile_rows in (8, 16)
    y, x = pix // wo, pix % wo
    txn = -(-wo // 16)
    ids = 4 * ((y // tile_rows) * txn + x // 16) + (y % tile_rows) // (tile_rows // 4)
    return ids, 4 * txn * (-(-ho // tile_rows))


def slot_partials(y, ids, slots, dtype=torch.float64):
    """(count, mean, M2), each [B, slots, N] in `dtype`, of y [B, HW, N] over the pixels of each slot (ids [HW]);
    a slot without a pixel is (0, 0, 0).  dtype float32 is the documented per-wave algorithm: an fp32 sum, the
    mean = sum / count, M2 = the fp32 sum of squared fp32 deviations from that mean."""
    b, hw, n = y.shape
    y = y.to(dtype)
    cnt = torch.zeros(slots, dtype=dtype, device=y.device).index_add_(0, ids, torch.ones(hw, dtype=dtype, device=y.device))
    s = torch.zeros(b, slots, n, dtype=dtype, device=y.device).index_add_(1, ids, y)
    c3 = cnt[None, :, None]
    mean = torch.where(c3 > 0, s / c3.clamp_min(1), torch.zeros_like(s))
    d = y - mean[:, ids]
    m2 = torch.zeros_like(s).index_add_(1, ids, d * d)
    return c3.expand(b, slots, n).contiguous(), mean, m2


def chan_merge(cnt, mean, m2):
    """Chan's merge of partials [B, S, N] over S in slot order, in fp64 -> (n, mean, M2), each [B, N]."""
    cnt, mean, m2 = cnt.double(), mean.double(), m2.double()
    n, mu, q = cnt[:, 0].clone(), mean[:, 0].clone(), m2[:, 0].clone()
    for s in range(1, cnt.shape[1]):
        nb, mb, qb = cnt[:, s], mean[:, s], m2[:, s]
        nn = n + nb
        f = torch.where(nn > 0, nb / nn.clamp_min(1), torch.zeros_like(nn))
        d = mb - mu
        mu = mu + d * f
        q = q + qb + d * d * n * f
        n = nn
    return n, mu, q


def pooled_stats(cnt, mean, m2):
    """The pooled (n, mean, M2) of partials [B, S, N] by definition, in fp64: n = sum c, mean = sum c m / n,
    M2 = sum M2_i + c_i (m_i - mean)^2 (a zero-count slot adds nothing)."""
    cnt, mean, m2 = cnt.double(), mean.double(), m2.double()
    n = cnt.sum(1)
    mu = (cnt * mean).sum(1) / n
    q = (m2 + cnt * (mean - mu[:, None]) ** 2).sum(1)
    return n, mu, q


def mean_rstd(n, mean, m2, eps=STATS_EPS):
    """{mean, 1 / sqrt(M2 / n + eps)} with eps the float32 the library receives."""
    eps = float(np.float32(eps))
    return mean, 1.0 / torch.sqrt(m2 / n + eps)


def instnorm_stats_fp64(y, eps=STATS_EPS):
    """nn.InstanceNorm2d's statistics of y [B, HW, N] in fp64: (mean, rstd), each [B, N] (biased variance)."""
    y = y.double()
    mean = y.mean(1)
    var = ((y - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + float(np.float32(eps)))


def instnorm_stats_restated(y32, ids, slots, eps=STATS_EPS):
    """The documented algorithm on the float32 output y32 [B, HW, N]: float32 slot partials, Chan's merge in fp64,
    the result rounded to float32 as the library stores it.  Returns (mean, rstd) float32 [B, N]."""
    assert y32.dtype == torch.float32
    mean, rstd = mean_rstd(*chan_merge(*slot_partials(y32, ids, slots, torch.float32)), eps)
    return mean.float(), rstd.float()


def stats_errors(mean, rstd, y):
    """The errors of merged statistics [B, N] against fp64 over y [B, HW, N]: (the mean's, relative to max |v| of
    the channel in its image; rstd's, relative), each [B, N] fp64."""
    m64, r64 = instnorm_stats_fp64(y)
    vmax = y.double().abs().amax(1).clamp_min(1e-30)
    return (mean.double() - m64).abs() / vmax, (rstd.double() - r64).abs() / r64


def enc_stats_bounds():
    return ENC_STATS_MARGIN * ENC_STATS_MEASURED["mean"], ENC_STATS_MARGIN * ENC_STATS_MEASURED["rstd"]


def stats_mismatch(mean, rstd, ref_mean, ref_rstd, vmax):
    """The merged-statistics comparison of the GPU tests against reference statistics [B, N] (vmax [B, N]: max |v|
    of the channel in its image) at enc_stats_bounds().  Returns (entries over a bound, the largest mean error
    relative to vmax, the largest relative rstd error)."""
    bm, br = enc_stats_bounds()
    em = (mean.double() - ref_mean.double()).abs() / vmax.double().clamp_min(1e-30)
    er = (rstd.double() - ref_rstd.double()).abs() / ref_rstd.double()
    bad = ~(em <= bm) | ~(er <= br)
    return int(bad.sum()), float(em.max()), float(er.max())


def partials_mismatch(got, ref, y, report=None, blocks=1):
    """The slot-by-slot comparison of the GPU tests.  got: the kernel's (count, mean, M2) [B, S, N]; ref: the fp64
    partials of the kernel's own output y [B, HW, N] over the documented footprints.  Returns the number of
    entries that violate: count exactly equal; |mean - ref| <= dm = 64 u max|v| (a float32 sum of <= 64 terms and
    one division; max |v| of the channel in its image); |M2 - ref| <= 80 u M2_ref + 2 c dm^2 (a float32 sum of
    c <= 64 squares of rounded differences, taken about a mean m' that is itself up to dm off: sum (v - m')^2 =
    M2 + c (m' - m)^2, no first-order term).  blocks = 2 (the halo kernel's 16-row tiles: a slot is two 32-pixel
    blocks combined by Chan's formula in float32, M2 = M2_a + M2_b + d^2 a b / c with d the difference of the two
    block means) adds the first-order term of d's error: 2 |d| dm a b / c <= (max v - min v) dm c / 2."""
    (gc, gm, gq), (rc, rm, rq) = got, ref
    vmax = y.double().abs().amax(1)[:, None, :]
    dm = 64 * U * vmax
    bad = (gc.double() != rc.double())
    bad |= ~((gm.double() - rm.double()).abs() <= dm)
    bq = 80 * U * rq.double() + 2 * rc.double() * dm * dm
    if blocks == 2:
        bq = bq + (y.double().amax(1) - y.double().amin(1))[:, None, :] * dm * rc.double() / 2
    bad |= ~((gq.double() - rq.double()).abs() <= bq)
    if report is not None:
        for b, s, n in bad.nonzero()[:8].tolist():
            report.append(f"(image {b}, slot {s}, n {n}): count {float(gc[b, s, n])} / {float(rc[b, s, n])}, mean "
                          f"{float(gm[b, s, n])!r} / {float(rm[b, s, n])!r}, M2 {float(gq[b, s, n])!r} / "
                          f"{float(rq[b, s, n])!r}, max|v| {float(vmax[b, 0, n])!r}")
    return int(bad.sum())


def enc_conv_ref(x, w, b, stride, pad, stats=None, relu=True, mutate=None):
    """conv2d(act(instance_norm(x))) in fp64 with the {mean, rstd} given (stats [B, cin, 2]; None: the plain conv),
    zero padding staying zero.  x [B, cin, H, W].  mutate (to show that a comparison rejects it): "no_relu",
    "next_image" (image b reads the statistics of image b - 1), "pad_normalised" (the zero padding normalised like
    a pixel)."""
    x, w = x.double(), w.double()
    b = None if b is None else b.double()
    if stats is None:
        return F.conv2d(x, w, b, stride, pad)
    st = stats.double()
    if mutate == "next_image":
        st = torch.roll(st, 1, 0)
    mean, rstd = st[:, :, 0, None, None], st[:, :, 1, None, None]
    if mutate == "pad_normalised":
        x, pad = F.pad(x, (pad[1], pad[1], pad[0], pad[0])), (0, 0)
    xn = (x - mean) * rstd
    if relu and mutate != "no_relu":
        xn = torch.relu(xn)
    return F.conv2d(xn, w, b, stride, pad)


def conv_mismatch(got, ref, tol):
    """Per image: max |got - ref| against tol x max(1, max |ref|) of that image ([B, ...] tensors).  Returns
    (the number of images over the bound, the largest error / bound)."""
    bsz = ref.shape[0]
    err = (got.double() - ref.double()).abs().reshape(bsz, -1).amax(1)
    bound = tol * ref.double().abs().reshape(bsz, -1).amax(1).clamp_min(1.0)
    return int((~(err < bound)).sum()), float((err / bound).max())
