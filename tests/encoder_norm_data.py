"""The operands of the encoder InstanceNorm conv tests (not a test module): per conv_forms.ENC_TABLE shape, built
once on the CPU and shared by every precision (tests/test_gpu_encoder_norm.py, which adds the launches, and
tests/test_encoder_norm_host.py, which needs no device).

Every case carries the data conditions a statistics path goes wrong on, next to the seeded tanh(randn) input:
  * images on different scales (x1, x20, x1, ...), so a partial or an in_norm pair that lands on the wrong image
    cannot pass;
  * input channels with offsets of alternating sign (+-0.5 of the scale): the normalised value of a zero padding
    tap, relu((0 - mean) * rstd), is then non-zero on every other channel;
  * output channel N - 2 with a zero weight row and the bias 1.7: a constant channel (var == 0, rstd = 1 / sqrt(eps));
  * output channel 1 with a bias 30 times its deviation in image 0.
Variants: "std" (in_norm with relu where the entry has in_norm), "nobias" (bias NULL), "norelu" (in_norm_relu = 0)."""
import functools

import numpy as np
import torch

import conv_forms as CF
import elementwise_oracle as EO

CONST_BIAS = 1.7
OFFSET_RATIO = 30.0


def key_of(c):
    return (c.B, c.H, c.W, c.cin, c.n, c.kh, c.kw, c.stride, bool(c.in_norm))


def footprint_of(c):
    """(kind, tile rows) of stats_slot_ids for the entry's form."""
    if c.form[0] == CF.HALO:
        return "halo", c.form[1]
    return ("stem", 8) if c.form[0] == CF.STEM else ("gemm", 0)


@functools.lru_cache(maxsize=None)
def case_data(key, variant="std"):
    """x [B, cin, H, W], w, b (None for "nobias"), in_stats [B, cin, 2] float32 or None (the fp64 statistics of x
    rounded to float32), relu, ref (fp64 [B, N, ho, wo], from the float32 in_stats: the conv is tested apart from
    its statistics).  All on the CPU; never modified."""
    B, H, W, cin, n, kh, kw, stride, in_norm = key
    assert n >= 8 and variant in ("std", "nobias", "norelu")
    seed = sum((i + 1) * 104729 * int(v) for i, v in enumerate(key)) % (2 ** 31)
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([1.0, 20.0] * B)[:B]
    off = torch.tensor([0.5, -0.5] * cin)[:cin]
    x = (torch.tanh(torch.randn(B, cin, H, W, generator=g)) + off[None, :, None, None]) * scale[:, None, None, None]
    w = torch.randn(n, cin, kh, kw, generator=g) / np.sqrt(cin * kh * kw)
    w[n - 2] = 0.0
    b = torch.randn(n, generator=g)
    b[n - 2] = CONST_BIAS
    pad = ((kh - 1) // 2, (kw - 1) // 2)
    relu = variant != "norelu"
    in_stats = None
    if in_norm:
        m, r = EO.instnorm_stats_fp64(x.permute(0, 2, 3, 1).reshape(B, H * W, cin))
        in_stats = torch.stack([m, r], -1).float().contiguous()
    raw = EO.enc_conv_ref(x, w, None, stride, pad, in_stats, relu)
    b[1] = OFFSET_RATIO * float(raw[0, 1].std(unbiased=False))
    if variant == "nobias":
        b = None
    ref = raw if b is None else raw + b.double()[None, :, None, None]
    return dict(x=x, w=w, b=b, pad=pad, in_stats=in_stats, relu=relu, ref=ref, ho=ref.shape[2], wo=ref.shape[3])


def rows_of(t):
    """NCHW [B, C, H, W] -> rows [B, H * W, C]."""
    b, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(b, h * w, c)
