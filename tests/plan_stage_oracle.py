"""Stage oracle of the RAFT forward: plain torch fp64 restatements of the reference's operations, one per
stage of an execution plan (not a test module).

Every function takes the model's own `state_dict` (reference key names, no packing, no column permutation,
no merged or split convs) through `params()`, NCHW tensors in float64, and returns float64.  They are written
from the module tree of core/extractor.py, core/update.py, core/corr.py and core/raft.py (the citations) and
from oracle/raft_oracle.py's reading of them, never from engine.py, so that a plan stage can be compared with
the operation it stands for.  tests/test_plan_stage_oracle_host.py pins them to oracle.raft_oracle on the CPU.

A level of the correlation pyramid that is one pixel high or wide has no defined lookup in the reference
(core/utils/utils.py:60-61 divides by H - 1 = 0): `lookup` returns NaN for every tap of such a level, as the
reference and the kernels do.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

DT = torch.float64


def params(state_dict) -> dict:
    """state_dict -> {key: float64 tensor} (integer buffers left out)."""
    out = {}
    for k, v in state_dict.items():
        v = torch.as_tensor(v)
        if v.dtype.is_floating_point:
            out[k] = v.detach().cpu().to(DT)
    return out


def dims(small: bool):
    """(hidden_dim, context_dim, corr_radius) of core/raft.py:36-46."""
    return (96, 64, 3) if small else (128, 128, 4)


def conv(x, p, pre, stride=1, padding=0):
    return F.conv2d(x, p[pre + ".weight"], p.get(pre + ".bias"), stride, padding)


# ---------------------------------------------------------------------------- prep, encoders


def prep(img):
    """core/raft.py:156-157."""
    return 2.0 * (img.to(DT) / 255.0) - 1.0


def _norm(x, p, pre, norm_fn):
    if norm_fn == "instance":   # nn.InstanceNorm2d: no affine, biased variance, eps 1e-5
        mean = x.mean((2, 3), keepdim=True)
        var = ((x - mean) ** 2).mean((2, 3), keepdim=True)
        return (x - mean) / torch.sqrt(var + 1e-5)
    if norm_fn == "batch":      # nn.BatchNorm2d in eval mode
        s = p[pre + ".weight"] / torch.sqrt(p[pre + ".running_var"] + 1e-5)
        return (x - p[pre + ".running_mean"].view(1, -1, 1, 1)) * s.view(1, -1, 1, 1) + p[pre + ".bias"].view(1, -1, 1, 1)
    if norm_fn == "none":
        return x
    raise NotImplementedError(norm_fn)


def _residual(x, p, pre, norm_fn, stride):
    """core/extractor.py:6-56."""
    y = torch.relu(_norm(conv(x, p, pre + ".conv1", stride, 1), p, pre + ".norm1", norm_fn))
    y = torch.relu(_norm(conv(y, p, pre + ".conv2", 1, 1), p, pre + ".norm2", norm_fn))
    if stride != 1:
        x = _norm(conv(x, p, pre + ".downsample.0", stride, 0), p, pre + ".downsample.1", norm_fn)
    return torch.relu(x + y)


def _bottleneck(x, p, pre, norm_fn, stride):
    """core/extractor.py:60-116."""
    y = torch.relu(_norm(conv(x, p, pre + ".conv1", 1, 0), p, pre + ".norm1", norm_fn))
    y = torch.relu(_norm(conv(y, p, pre + ".conv2", stride, 1), p, pre + ".norm2", norm_fn))
    y = torch.relu(_norm(conv(y, p, pre + ".conv3", 1, 0), p, pre + ".norm3", norm_fn))
    if stride != 1:
        x = _norm(conv(x, p, pre + ".downsample.0", stride, 0), p, pre + ".downsample.1", norm_fn)
    return torch.relu(x + y)


def encoder_norm(which: str, small: bool) -> str:
    """core/raft.py:36-46: fnet 'instance'; cnet 'batch' (RAFT-full) / 'none' (RAFT-small)."""
    return "instance" if which == "fnet" else ("none" if small else "batch")


def encoder(x, p, which: str, small: bool):
    """core/extractor.py:118-192 (BasicEncoder) / :195-267 (SmallEncoder), eval mode; x is the prep output."""
    norm_fn = encoder_norm(which, small)
    block = _bottleneck if small else _residual
    x = torch.relu(_norm(conv(x, p, which + ".conv1", 2, 3), p, which + ".norm1", norm_fn))
    for li, stride in ((1, 1), (2, 2), (3, 2)):
        x = block(x, p, f"{which}.layer{li}.0", norm_fn, stride)
        x = block(x, p, f"{which}.layer{li}.1", norm_fn, 1)
    return conv(x, p, which + ".conv2", 1, 0)


def context_split(cnet, small: bool):
    """core/raft.py:195-197 -> (net, inp)."""
    hd, cd, _ = dims(small)
    return torch.tanh(cnet[:, :hd]), torch.relu(cnet[:, hd:hd + cd])


# ---------------------------------------------------------------------------- correlation


def corr_pyramid(fmap1, fmap2, levels=4):
    """core/corr.py:25-54 + :96-127: level l is [B*H*W, 1, H >> l, W >> l]."""
    b, c, h, w = fmap1.shape
    corr = torch.matmul(fmap1.reshape(b, c, h * w).transpose(1, 2), fmap2.reshape(b, c, h * w)) / math.sqrt(c)
    corr = corr.reshape(b * h * w, 1, h, w)
    pyr = [corr]
    for _ in range(levels - 1):
        corr = F.avg_pool2d(corr, 2, stride=2)
        pyr.append(corr)
    return pyr


def _bilinear(img, x, y):
    """img [N, H, W] sampled at pixel positions x, y [N, K] with zeros outside (grid_sample, align_corners,
    padding 'zeros', core/utils/utils.py:57-71)."""
    n, h, w = img.shape
    x0, y0 = torch.floor(x), torch.floor(y)
    tx, ty = x - x0, y - y0
    x0, y0 = x0.long(), y0.long()
    flat = img.reshape(n, h * w)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        v = torch.gather(flat, 1, yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1))
        return torch.where(ok, v, torch.zeros((), dtype=img.dtype))

    return (tap(y0, x0) * (1 - tx) * (1 - ty) + tap(y0, x0 + 1) * tx * (1 - ty)
            + tap(y0 + 1, x0) * (1 - tx) * ty + tap(y0 + 1, x0 + 1) * tx * ty)


def lookup(pyramid, coords, r: int):
    """core/corr.py:56-94: coords [B, 2, H, W] (x, y) -> [B, L * (2r+1)^2, H, W], channel
    lvl * (2r+1)^2 + ix * (2r+1) + iy (the delta grid is meshgrid(dy, dx) added to (x, y): the slow window
    index moves x)."""
    b, _, h, w = coords.shape
    k = 2 * r + 1
    c = coords.to(DT).permute(0, 2, 3, 1).reshape(b * h * w, 2)
    d = torch.arange(-r, r + 1, dtype=DT)
    dx = d.view(k, 1).expand(k, k).reshape(1, k * k)   # slow index
    dy = d.view(1, k).expand(k, k).reshape(1, k * k)
    outs = []
    for lvl, corr in enumerate(pyramid):
        lh, lw = corr.shape[-2:]
        x = c[:, 0:1] / 2 ** lvl + dx
        y = c[:, 1:2] / 2 ** lvl + dy
        if lh == 1 or lw == 1:
            v = torch.full((b * h * w, k * k), float("nan"), dtype=DT)
        else:
            v = _bilinear(corr[:, 0], x, y)
        outs.append(v.reshape(b, h, w, k * k))
    return torch.cat(outs, -1).permute(0, 3, 1, 2).contiguous()


def alt_lookup(fmap1, fmap2, coords, r: int, levels=4):
    """core/corr.py:140-198 (AlternateCorrBlock): fmap2 pooled per level, the dot products of fmap1 with the
    window around coords / 2^lvl, bilinear, / sqrt(C).  Mathematically the all-pairs lookup on a pyramid
    whose level l correlates fmap1 with the pooled fmap2 (pooling is linear), which is how it is computed
    here; unlike the all-pairs sampler it never normalises coordinates, so 1-px levels are defined."""
    b, c, h, w = fmap1.shape
    k = 2 * r + 1
    cc = coords.to(DT).permute(0, 2, 3, 1).reshape(b * h * w, 2)
    d = torch.arange(-r, r + 1, dtype=DT)
    dx = d.view(k, 1).expand(k, k).reshape(1, k * k)
    dy = d.view(1, k).expand(k, k).reshape(1, k * k)
    f1 = fmap1.reshape(b, c, h * w).transpose(1, 2)
    outs = []
    f2 = fmap2
    for lvl in range(levels):
        lh, lw = f2.shape[-2:]
        corr = torch.matmul(f1, f2.reshape(b, c, lh * lw)).reshape(b * h * w, lh, lw)
        v = _bilinear(corr, cc[:, 0:1] / 2 ** lvl + dx, cc[:, 1:2] / 2 ** lvl + dy)
        outs.append(v.reshape(b, h, w, k * k))
        if lvl < levels - 1:
            f2 = F.avg_pool2d(f2, 2, stride=2)
    return (torch.cat(outs, -1) / math.sqrt(c)).permute(0, 3, 1, 2).contiguous()


def coords_grid(b, h, w):
    """core/utils/utils.py:74-77: channel 0 = x, channel 1 = y."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=DT), torch.arange(w, dtype=DT), indexing="ij")
    return torch.stack([xs, ys], 0)[None].repeat(b, 1, 1, 1)


# ---------------------------------------------------------------------------- update block


def motion_encoder(flow, corr, p, small: bool, pre="update_block.encoder"):
    """core/update.py:123-167 / :169-216 -> dict of every intermediate; 'out' is cat[conv, flow]."""
    cor1 = torch.relu(conv(corr, p, pre + ".convc1", 1, 0))
    cor = cor1 if small else torch.relu(conv(cor1, p, pre + ".convc2", 1, 1))
    flo1 = torch.relu(conv(flow, p, pre + ".convf1", 1, 3))
    flo = torch.relu(conv(flo1, p, pre + ".convf2", 1, 1))
    motion = torch.relu(conv(torch.cat([cor, flo], 1), p, pre + ".conv", 1, 1))
    return dict(cor1=cor1, flo1=flo1, cor=cor, flo=flo, motion=motion, out=torch.cat([motion, flow], 1))


def gru_half(h, x, p, zk, rk, qk, pad):
    """core/update.py:52-72 / :99-121 -> (h', z, r*h)."""
    hx = torch.cat([h, x], 1)
    z = torch.sigmoid(conv(hx, p, zk, 1, pad))
    r = torch.sigmoid(conv(hx, p, rk, 1, pad))
    q = torch.tanh(conv(torch.cat([r * h, x], 1), p, qk, 1, pad))
    return (1 - z) * h + z * q, z, r * h


def gru_steps(small: bool, pre="update_block.gru"):
    """(convz, convr, convq, padding) of each GRU half-step."""
    if small:
        return [(pre + ".convz", pre + ".convr", pre + ".convq", (1, 1))]
    return [(pre + ".convz1", pre + ".convr1", pre + ".convq1", (0, 2)),
            (pre + ".convz2", pre + ".convr2", pre + ".convq2", (2, 0))]


def update_step(net, inp, corr, flow, p, small: bool, detail=False):
    """core/update.py:297-325 (BasicUpdateBlock) / :250-263 (SmallUpdateBlock): -> (net', delta, mask), mask None
    for RAFT-small.  detail=True adds a dict of the intermediates (motion encoder's, z and r*h of the last
    half-step)."""
    me = motion_encoder(flow, corr, p, small)
    x = torch.cat([inp, me["out"]], 1)
    h = net
    for zk, rk, qk, pad in gru_steps(small):
        h, z, rh = gru_half(h, x, p, zk, rk, qk, pad)
    fh = "update_block.flow_head"
    delta = conv(torch.relu(conv(h, p, fh + ".conv1", 1, 1)), p, fh + ".conv2", 1, 1)
    mask = None
    if not small:
        mask = 0.25 * conv(torch.relu(conv(h, p, "update_block.mask.0", 1, 1)), p, "update_block.mask.2", 1, 0)
    if detail:
        return h, delta, mask, dict(me, z=z, rh=rh)
    return h, delta, mask


def gru_context(inp, p, small: bool):
    """The part of each half-step's convz | convr | convq that acts on `inp` (input columns
    [hdim, hdim + cdim) of cat[h, inp, motion, flow], core/update.py:106 + :318), biases included:
    one [B, 3 * hdim, H, W] tensor per half-step."""
    hd, cd, _ = dims(small)
    out = []
    for zk, rk, qk, pad in gru_steps(small):
        out.append(torch.cat([F.conv2d(inp, p[k + ".weight"][:, hd:hd + cd], p[k + ".bias"], 1, pad)
                              for k in (zk, rk, qk)], 1))
    return out


# ---------------------------------------------------------------------------- upsampling


def convex_upsample(flow, mask):
    """core/raft.py:112-142."""
    n, _, h, w = flow.shape
    m = torch.softmax(mask.view(n, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(8 * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    up = torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3)
    return up.reshape(n, 2, 8 * h, 8 * w)


def upflow8(flow):
    """core/utils/utils.py:80-82."""
    n, _, h, w = flow.shape
    return 8 * F.interpolate(flow, size=(8 * h, 8 * w), mode="bilinear", align_corners=True)


# ---------------------------------------------------------------------------- the stages chained


def forward(state_dict, image1, image2, iters, small, alternate=False, flow_init=None):
    """The stages chained as core/raft.py:145-251 chains them -> (flow_low, [flow_up per iteration])."""
    p = params(state_dict)
    hd, cd, r = dims(small)
    x1, x2 = prep(image1), prep(image2)
    b = x1.shape[0]
    fm = encoder(torch.cat([x1, x2], 0), p, "fnet", small)
    f1, f2 = fm[:b], fm[b:]
    if alternate:
        look = lambda c: alt_lookup(f1, f2, c, r)   # noqa: E731
    else:
        pyr = corr_pyramid(f1, f2)
        look = lambda c: lookup(pyr, c, r)          # noqa: E731
    net, inp = context_split(encoder(x1, p, "cnet", small), small)
    h, w = f1.shape[-2:]
    c0 = coords_grid(b, h, w)
    c1 = c0.clone() if flow_init is None else c0 + flow_init.to(DT)
    ups = []
    for _ in range(iters):
        net, delta, mask = update_step(net, inp, look(c1), c1 - c0, p, small)
        c1 = c1 + delta
        ups.append(upflow8(c1 - c0) if mask is None else convex_upsample(c1 - c0, mask))
    return c1 - c0, ups
