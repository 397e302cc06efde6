"""raft_resize's definition (include/raft_hip.h) in numpy fp64, with the integer source coordinates.

  lin_coords(D, S, align)      (i0, i1, n % den, den) of every output index: Python integers, exact at any size
  resize_ref(src, size, ...)   float64 [B,C,h,w] of a float [B,C,H,W] source: bilinear (both align_corners) or
                               area, channels 0 / 1 times mul0 / mul1
  to_u8(v)                     the uint8 output's rounding: nearest even, saturated, NaN -> 0
  nchw / nhwc                  the two frame layouts
  tol_bilinear / tol_area      the fp32 kernel's derived distance to this fp64 definition

The tolerances count roundings (u = 2^-24, T = the largest tap magnitude), as the header does.  Bilinear: on the
path of one output lie lx, 1 - lx, a product and the sum of a horizontal blend (the two products' errors carry
the weights 1 - lx and lx and count once; so do the two horizontal blends under 1 - ly and ly), then ly, 1 - ly,
a product and the sum of the vertical blend: (1 + 4u)^2 - 1, i.e. 8 u to first order, 1.2e-4 on 0..255.  Area: a
sequential sum of n terms and one division: (n + 1) u.  A flow multiplier m adds two roundings, the ratio's on
the host and the product's, and scales the whole bound by |m|.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24


def lin_coords(D, S, align):
    """Per output index d of D over S source samples: lists i0, i1, rem = n % den, and den (exact integers)."""
    i0, i1, rem = [], [], []
    den = max(D - 1, 1) if align else 2 * D
    for d in range(D):
        n = d * (S - 1) if align else max((2 * d + 1) * S - D, 0)
        a = min(n // den, S - 1)
        i0.append(a)
        i1.append(min(a + 1, S - 1))
        rem.append(n % den)
    return i0, i1, rem, den


def box_coords(D, S):
    """Area mode: source samples lo[d] .. hi[d] - 1 of output index d."""
    lo = [(d * S) // D for d in range(D)]
    hi = [-((-(d + 1) * S) // D) for d in range(D)]
    return lo, hi


def resize_ref(src, size, mode="bilinear", align=False, mul0=1.0, mul1=1.0):
    """float64 [B,C,h,w].  Every tap is blended, weight 0 or not, so NaN / Inf spread as the formula says."""
    v = np.asarray(src, dtype=np.float64)
    B, C, S_h, S_w = v.shape
    h, w = size
    if mode == "area":
        ylo, yhi = box_coords(h, S_h)
        xlo, xhi = box_coords(w, S_w)
        out = np.empty((B, C, h, w))
        with np.errstate(invalid="ignore"):
            for i in range(h):
                rows = v[:, :, ylo[i]:yhi[i], :]
                for j in range(w):
                    out[:, :, i, j] = rows[:, :, :, xlo[j]:xhi[j]].mean(axis=(2, 3))
    elif mode == "bilinear":
        y0, y1, ry, dy = lin_coords(h, S_h, align)
        x0, x1, rx, dx = lin_coords(w, S_w, align)
        ly = (np.array(ry, dtype=np.float64) / dy)[None, None, :, None]
        lx = (np.array(rx, dtype=np.float64) / dx)[None, None, None, :]
        with np.errstate(invalid="ignore"):
            top = (1 - lx) * v[:, :, y0][:, :, :, x0] + lx * v[:, :, y0][:, :, :, x1]
            bot = (1 - lx) * v[:, :, y1][:, :, :, x0] + lx * v[:, :, y1][:, :, :, x1]
            out = (1 - ly) * top + ly * bot
    else:
        raise ValueError(mode)
    with np.errstate(invalid="ignore"):
        out[:, 0] = out[:, 0] * float(mul0)
        if C > 1:
            out[:, 1] = out[:, 1] * float(mul1)
    return out


def flow_muls(src_hw, size):
    """The multipliers of a flow resized from src_hw to size: each ratio rounded to fp32 once."""
    return float(np.float32(size[1] / src_hw[1])), float(np.float32(size[0] / src_hw[0]))


def to_u8(v):
    """Nearest (ties to even), saturated to 0..255, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        r = np.rint(np.clip(np.nan_to_num(v, nan=0.0, posinf=255.0, neginf=0.0), 0.0, 255.0))
    return r.astype(np.uint8)


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


def tol_bilinear(T, mul=1.0, flow=False):
    """The fp32 kernel's distance to resize_ref: ((1 + 4u)^2 - 1) T; with a multiplier two more roundings (the
    ratio's and the product's), times |mul|."""
    t = ((1 + 4 * U) ** 2 - 1) * T
    if flow:
        t = (((1 + 4 * U) ** 2) * (1 + U) ** 2 - 1) * T * abs(mul)
    return t


def max_box(src_hw, size):
    lo_y, hi_y = box_coords(size[0], src_hw[0])
    lo_x, hi_x = box_coords(size[1], src_hw[1])
    return max(b - a for a, b in zip(lo_y, hi_y)) * max(b - a for a, b in zip(lo_x, hi_x))


def tol_area(T, n, mul=1.0, flow=False):
    """(n + 1) u T for a box of n samples (one rounding per summed term and the division); with a multiplier two
    more roundings, times |mul|."""
    t = ((1 + U) ** (n + 1) - 1) * T
    if flow:
        t = (((1 + U) ** (n + 3)) - 1) * T * abs(mul)
    return t


def seeded_frame(B, C, H, W, seed=0):
    """Uniform noise in 0..255 as float32: the hardest input for an interpolation's coordinate error."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 255.0, size=(B, C, H, W)).astype(np.float32)


def seeded_flow(B, H, W, seed=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(-20.0, 20.0, size=(B, 2, H, W)).astype(np.float32)


def golden_case():
    """The seeded case of tests/golden/resize_reference.npz: a 2 x 3 x 37 x 53 frame of integer noise in 0..255
    and a 2 x 2 x 37 x 53 flow of noise in sixteenths of a pixel up to 20 px (neighbouring samples jump as far as
    uniform noise does; the few distinct values keep the compressed fixture small)."""
    rng = np.random.default_rng(20)
    frame = rng.integers(0, 256, size=(2, 3, 37, 53)).astype(np.float32)
    flow = (rng.integers(-320, 321, size=(2, 2, 37, 53)) / 16.0).astype(np.float32)
    return frame, flow


# (B, Hs, Ws) -> (Hd, Wd): the cases of tests/test_gpu_resize.py and tests/test_resize_host.py
SHAPES = [
    ((1, 1, 1), (3, 5)),          # single source sample
    ((2, 5, 7), (5, 7)),          # identity
    ((2, 37, 53), (19, 27)),      # odd downscale
    ((2, 37, 53), (74, 106)),     # exact 2x up
    ((1, 17, 23), (40, 56)),      # odd upscale
    ((1, 8, 8), (1, 1)),          # single output sample
    ((1, 3, 130), (2, 67)),       # crosses a wave and a vector-store boundary
    ((1, 64, 96), (32, 48)),      # exact 2x down
]
