"""The shape -> kernel form table of the conv tests (not a test module).

Every entry names a conv (stride, "same" padding unless strided) and the form raft_conv2d_form must report for it
on a 256-CU device (the count the library assumes without a device, and MI355X's): test_capi.py pins the table on
the host, test_gpu_conv_epilogues.py asserts each entry again before it launches.  The shapes are the smallest that
reach each form; all are ragged in both axes.  ENC_TABLE (below) is the same for the InstanceNorm encoders' convs,
whose forms depend on their stats_part / in_norm features.

A form is the tuple of `struct raft_conv2d_form` (include/raft_hip.h):
(kernel, tile_rows, tile_cols, tiles_per_wg, loader_waves, compute_waves_per_simd, gemm_k_groups, smalln_tile_rows).
"""
from collections import namedtuple

from raft_optical_flow_amd import _lib

HALO, GEMM, STEM, SMALLN, SMALLN3X3 = (_lib.CONV_KERNEL_HALO, _lib.CONV_KERNEL_GEMM, _lib.CONV_KERNEL_STEM,
                                       _lib.CONV_KERNEL_SMALLN, _lib.CONV_KERNEL_SMALLN3X3)

Conv = namedtuple("Conv", "name B H W cin n kh kw stride prec form")

SPLIT_PRECS = ("f16x3", "bf16", "f16")


def _halo(rows, cols, m, nl, ks):
    return (HALO, rows, cols, m, nl, ks, 0, 0)


def _table():
    t = []

    def add(name, shape, cin, n, k, forms, stride=1):
        B, H, W = shape
        for prec, form in forms.items():
            t.append(Conv(f"{name}-{prec}", B, H, W, cin, n, k[0], k[1], stride, prec, form))

    def split3(x3, one):  # the f16x3 form and the form both one-product precisions take
        return {"f16x3": x3, "bf16": one, "f16": one}

    # halo, 32-column tiles, one tile per work-group (f16x3: the 8-loader form)
    add("h32-3x3", (1, 9, 19), 64, 128, (3, 3), split3(_halo(8, 32, 1, 8, 1), _halo(8, 32, 1, 4, 1)))
    # halo, 64-column tiles, one tile per work-group: f16x3 3x3 / 1x5 / 5x1 take the K-split form (two compute
    # waves per SIMD); K-steps: 27 (3x3, cin 96), 15 (1x5 / 5x1), 2 (1x1, cin 64)
    for k in ((3, 3), (1, 5), (5, 1)):
        add(f"h64-{k[0]}x{k[1]}", (2, 37, 61), 96, 256, k, split3(_halo(8, 64, 1, 4, 2), _halo(8, 64, 1, 4, 1)))
    add("h64-1x1", (2, 37, 61), 64, 256, (1, 1), split3(_halo(8, 64, 1, 4, 1), _halo(8, 64, 1, 4, 1)))
    # 64-column tiles at N = 128, N = 126 (a ragged last tile) and N = 100 (a ragged half after split 64)
    add("h64-n128", (2, 37, 125), 96, 128, (3, 3), split3(_halo(8, 64, 1, 4, 2), _halo(8, 64, 1, 4, 1)))
    add("h64-n126", (2, 37, 125), 64, 126, (3, 3), split3(_halo(8, 64, 1, 4, 2), _halo(8, 64, 1, 4, 1)))
    add("h64-n100", (2, 37, 125), 64, 100, (1, 5), split3(_halo(8, 64, 1, 4, 2), _halo(8, 64, 1, 4, 1)))
    # big (16-row) tiles, one per work-group
    for k in ((3, 3), (1, 5), (5, 1)):
        add(f"big-{k[0]}x{k[1]}", (1, 37, 205), 64, 256, k, split3(_halo(16, 64, 1, 4, 1), _halo(16, 64, 1, 4, 1)))
    # big tiles, two per work-group
    add("bigmt-3x3", (2, 90, 130), 64, 256, (3, 3), {"f16x3": _halo(16, 64, 2, 4, 1)})
    add("bigmt-1x5", (2, 90, 130), 64, 256, (1, 5), split3(_halo(16, 64, 2, 4, 1), _halo(16, 64, 2, 4, 1)))
    # 8-row tiles, three per work-group (f16x3); the one-product precisions take 128-column tiles there
    add("mt-3x3", (2, 60, 130), 64, 256, (3, 3), split3(_halo(8, 64, 3, 4, 1), _halo(8, 128, 1, 4, 1)))
    add("mt-1x5", (2, 60, 130), 64, 256, (1, 5), split3(_halo(8, 64, 3, 4, 1), _halo(8, 128, 2, 4, 1)))
    add("mt-1x1", (2, 60, 130), 64, 256, (1, 1), split3(_halo(8, 64, 3, 4, 1), _halo(8, 128, 2, 4, 1)))
    # GEMM kernel: one K-group (3 K-steps), two K-groups (the strided encoder convs)
    add("gemm1-1x1", (1, 9, 19), 96, 128, (1, 1), {"fp32": (GEMM, 0, 0, 0, 0, 0, 1, 0)})
    add("gemm2-3x3s2", (1, 19, 24), 64, 96, (3, 3), {p: (GEMM, 0, 0, 0, 0, 0, 2, 0) for p in ("fp32",) + SPLIT_PRECS},
        stride=2)
    # small-N VALU kernels (always the fp32 weight)
    add("sn-n3-3x3", (1, 9, 21), 96, 3, (3, 3), {"fp32": (SMALLN, 0, 0, 0, 0, 0, 0, 0)})
    add("sn-n4-3x3", (1, 9, 21), 96, 4, (3, 3), {"fp32": (SMALLN, 0, 0, 0, 0, 0, 0, 0)})
    add("sn-n2-1x1", (1, 6, 10), 128, 2, (1, 1), {"fp32": (SMALLN, 0, 0, 0, 0, 0, 0, 0)})
    add("sn3-n2-th2", (2, 13, 35), 256, 2, (3, 3), {"fp32": (SMALLN3X3, 0, 0, 0, 0, 0, 0, 2)})
    add("sn3-n2-th4", (2, 37, 205), 64, 2, (3, 3), {"fp32": (SMALLN3X3, 0, 0, 0, 0, 0, 0, 4)})   # 260 4-row tiles
    add("sn3-n1-th2", (2, 13, 35), 256, 1, (3, 3), {"fp32": (SMALLN3X3, 0, 0, 0, 0, 0, 0, 2)})
    add("sn3-n1-th4", (2, 37, 205), 64, 1, (3, 3), {"fp32": (SMALLN3X3, 0, 0, 0, 0, 0, 0, 4)})
    # the encoders' stem (GATHER packing; LINEAR alpha 1 and RELU only)
    add("stem", (2, 37, 45), 3, 64, (7, 7), {p: (STEM, 0, 0, 0, 0, 0, 0, 0) for p in SPLIT_PRECS}, stride=2)
    return t


TABLE = _table()
BY_NAME = {c.name: c for c in TABLE}


def pad_of(c):
    return ((c.kh - 1) // 2, (c.kw - 1) // 2)


def out_hw(c):
    ph, pw = pad_of(c)
    return (c.H + 2 * ph - c.kh) // c.stride + 1, (c.W + 2 * pw - c.kw) // c.stride + 1


def k_steps(c):
    """32-wide K-steps of the conv's VEC packing."""
    return c.kh * c.kw * (-(-c.cin // 32))


def host_params(c, epilogue=_lib.EPI_LINEAR, alpha=1.0, features=True):
    """raft_conv2d_params of the conv with stand-in pointers (16-byte aligned, never dereferenced): enough for the
    host-side queries.  f16x3 3x3 / 1x5 / 5x1 convs carry the scaled weight, as kernels.conv_params sets it.  An
    ENC_TABLE entry also carries its features (stats_part with stats_ld = N + 4, in_norm with relu): halo_pick
    depends on them (features=False: the bare conv)."""
    fake = 1 << 20
    ph, pw = pad_of(c)
    ho, wo = out_hw(c)
    p = _lib.ConvParams()
    p.in0, p.in0_ld, p.in0_c = fake, c.cin, c.cin
    p.batch, p.in_h, p.in_w, p.out_h, p.out_w = c.B, c.H, c.W, ho, wo
    p.kh, p.kw, p.stride_h, p.stride_w, p.pad_h, p.pad_w = c.kh, c.kw, c.stride, c.stride, ph, pw
    p.mode = _lib.RAFT_CONV_VEC if c.cin % 4 == 0 else _lib.RAFT_CONV_GATHER
    p.weight, p.n, p.out, p.out_ld = fake, c.n, fake, c.n
    p.precision = _lib.PRECISIONS[c.prec] if c.n > 4 else _lib.PREC_FP32
    p.epilogue, p.alpha = epilogue, alpha
    if c.prec == "f16x3" and c.n > 4 and c.stride == 1 and (c.kh, c.kw) in ((3, 3), (1, 5), (5, 1)):
        p.weight_s = fake
    if features and getattr(c, "stats", False) and c.slots > 0:   # (slots == 0: raft_conv2d rejects stats_part)
        p.stats_part, p.stats_ld = fake, c.n + 4
    if features and getattr(c, "in_norm", False):
        p.in_norm, p.in_norm_relu = fake, 1
    return p


# ----------------------------------------------------------------------------- the InstanceNorm encoders' convs
#
# The convs of an InstanceNorm encoder run in instantiations of their own (conv_halo_kernel<ENC = true>, the GEMM
# kernel's per-image M tiling, the stem's statistics call), reached only with stats_part / in_norm set: ENC_TABLE
# pins the form of each WITH its features set, and the statistics slots per image (raft_conv2d_stats_slots) and
# raft_conv2d_in_norm_ok next to it.  test_encoder_norm_host.py pins the table on the host,
# test_gpu_encoder_norm.py asserts each entry again before it launches.  RAFT-small's channel counts (8, 16, 24,
# 32, 96) are in it next to RAFT-full's.

EncConv = namedtuple("EncConv", "name B H W cin n kh kw stride prec form stats in_norm slots in_norm_ok")


def _enc_table():
    t = []
    gemm1, gemm2 = (GEMM, 0, 0, 0, 0, 0, 1, 0), (GEMM, 0, 0, 0, 0, 0, 2, 0)

    def add(name, shape, cin, n, k, x3, one, slots, in_norm=False, in_norm_ok=None, stride=1, stats=True):
        B, H, W = shape
        ok = int(in_norm) if in_norm_ok is None else in_norm_ok
        for prec, form in (("f16x3", x3), ("bf16", one), ("f16", one)):
            t.append(EncConv(f"{name}-{prec}", B, H, W, cin, n, k, k, stride, prec, form, stats, in_norm, slots, ok))

    def add33(name, shape, c, rows, cols, slots, nl=8, **kw):   # 3x3 c -> c, both features
        add(name, shape, c, c, 3, _halo(rows, cols, 1, nl, 1), _halo(rows, cols, 1, 4, 1), slots, in_norm=True, **kw)

    def add11(name, shape, cin, n, cols, m, slots):             # 1x1, statistics
        add(name, shape, cin, n, 1, _halo(8, cols, m, 4, 1), _halo(8, cols, m, 4, 1), slots, in_norm_ok=0)

    # halo 8 x 32, one tile per work-group (f16x3: 8 loaders); 3 x 5: 4 slots of which 2 hold no pixel
    add33("e32-64", (1, 9, 19), 64, 8, 32, 16)
    add33("e32-64-3x5", (1, 3, 5), 64, 8, 32, 4)
    # RAFT-small's bottleneck channels: N = 8 / 24 inside a 32-column tile, in0_c < 32 in the loaders' table
    add33("e32-8", (2, 19, 27), 8, 8, 32, 24)
    add33("e32-24", (2, 10, 14), 24, 8, 32, 8)
    add11("e1-32to8", (2, 19, 27), 32, 8, 32, 1, 24)
    add11("e1-8to32", (2, 10, 14), 8, 32, 32, 1, 8)
    add11("e1-32to16", (2, 19, 27), 32, 16, 32, 1, 24)
    add11("e1-16to64", (2, 10, 14), 16, 64, 32, 1, 8)
    add11("e1-24to96", (2, 19, 27), 24, 96, 32, 1, 24)
    # the in0_c <= 256 edge of in_norm, and just past it (statistics only: raft_conv2d_in_norm_ok == 0)
    add33("e32-256", (1, 19, 27), 256, 8, 32, 24)
    add("e32-288to64", (1, 19, 27), 288, 64, 3, _halo(8, 32, 1, 8, 1), _halo(8, 32, 1, 4, 1), 24, in_norm_ok=0)
    # halo 8 x 64 and 16 x 64
    add33("e64-64", (2, 60, 130), 64, 8, 64, 288)
    add33("big-96", (2, 90, 130), 96, 16, 64, 216, nl=4)
    add33("big-128", (2, 60, 130), 128, 16, 64, 144, nl=4)
    add11("e64-96to128", (2, 37, 125), 96, 128, 64, 1, 160)
    # 1x1 with 2 and 3 tiles per work-group
    add11("mt2-64to128", (2, 60, 130), 64, 128, 64, 2, 288)
    add11("mt3-64to128", (4, 60, 130), 64, 128, 64, 3, 288)
    # the strided convs on the GEMM kernel (per-image M tiling): 3x3 two K-groups, 1x1 one
    add("g2-64to96", (1, 19, 24), 64, 96, 3, gemm2, gemm2, 4, in_norm_ok=0, stride=2)
    add("g2-16to16", (2, 19, 27), 16, 16, 3, gemm2, gemm2, 6, in_norm_ok=0, stride=2)
    add("g1-64to96", (1, 19, 24), 64, 96, 1, gemm1, gemm1, 4, in_norm_ok=0, stride=2)
    add("g1-32to64", (2, 19, 27), 32, 64, 1, gemm1, gemm1, 6, in_norm_ok=0, stride=2)
    # the stem (GATHER packing); RAFT-small's 32-output stem runs on the GEMM kernel and has no statistics slots:
    # raft_conv2d rejects stats_part for it (the engine takes raft_instnorm_stats), so its form is the bare conv's
    stem = (STEM, 0, 0, 0, 0, 0, 0, 0)
    add("stem-64", (2, 37, 45), 3, 64, 7, stem, stem, 24, in_norm_ok=0, stride=2)
    add("stem-32", (2, 37, 45), 3, 32, 7, gemm2, gemm2, 0, in_norm_ok=0, stride=2)
    return t


ENC_TABLE = _enc_table()
ENC_BY_NAME = {c.name: c for c in ENC_TABLE}
ENC_PRECS = SPLIT_PRECS
