"""ctypes binding of libraft_hip.so (the C-ABI declared in include/raft_hip.h).

The library is built in-tree by `python __graft_entry__.py build` (or
`make -C raft_optical_flow_amd/csrc`).  There is no fallback: if the library
is missing or fails to load, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RAFT_HIP_LIB") or os.path.join(_HERE, "libraft_hip.so")

c_int = ctypes.c_int
c_float = ctypes.c_float
c_size_t = ctypes.c_size_t
c_long = ctypes.c_long
c_void_p = ctypes.c_void_p
c_char_p = ctypes.c_char_p
P = c_void_p  # device pointers are passed as integers / void*

RAFT_CONV_VEC = 0
RAFT_CONV_GATHER = 1

PREC_FP32 = 0    # v_mfma_f32_32x32x2_f32
PREC_F16X3 = 1   # fp32-accurate hi/lo f16 split on v_mfma_f32_32x32x16_f16
PREC_F16 = 2     # single f16 product (mixed precision)
PREC_BF16 = 3    # single bf16 product on v_mfma_f32_32x32x16_bf16 (bf16 mixed precision)
PRECISIONS = {"fp32": PREC_FP32, "f16x3": PREC_F16X3, "f16": PREC_F16, "bf16": PREC_BF16}

ABI_VERSION = 19
RANGE_LIMIT = 32768.0  # RAFT_RANGE_LIMIT: |x| above it raises the f16x3 range guard

FRAME_F32_NCHW = 0   # raft_ingest_frame input: float32 [B, 3, H, W]
FRAME_U8_NHWC = 1    # uint8 [B, H, W, 3]

VIZ_BGR = 1    # raft_flow_to_rgb flags: bytes in B, G, R order
VIZ_UNIT = 2   # no normalisation (flow_uv_to_colors)
VIZ_CLIP = 4   # clip both components to [0, clip_flow] first

WARP_BORDER = 1   # raft_warp_frame flag: clamp the sampling position to the frame (default: zeros outside)

RESIZE_BILINEAR = 0        # raft_resize modes
RESIZE_AREA = 1            # torch's mode="area": adaptive average pooling
RESIZE_ALIGN_CORNERS = 1   # raft_resize flag: bilinear with align_corners

MASK_U8 = 0    # raft_flow_metrics mask tags: bool or uint8, valid where != 0
MASK_F32 = 1   # float32, valid where >= 0.5

# raft_flow_metrics: the record's slots (RAFT_FM_*), int64 counts then fp64 sums, and the launch constants
FM_SLOTS = 16
FM_BLOCK_PIXELS = 1024
FM_MAX_BLOCKS = 256
FM_COUNTS = ("n", "n_nonfinite", "n_lt1", "n_lt3", "n_lt5", "n_outlier", "n_s0_10", "n_s10_40", "n_s40")
FM_SUMS = ("epe_sum", "epe_sum_s0_10", "epe_sum_s10_40", "epe_sum_s40")
FM_IMAGES = 13
FM_IMAGE_MEAN_SUM = 14
FM_RESERVED = 15

# raft_photo_metrics: the record's slots (RAFT_PM_*), int64 counts then fp64 sums, the flag and the launch constants
PM_SLOTS = 16
PM_TILE_H = 16        # RAFT_PHOTO_METRICS_TILE_H / _TILE_W: the tile a work-group takes per pass
PM_TILE_W = 64
PM_MAX_BLOCKS = 512   # work-groups per sample at most; samples with more tiles wrap
PM_PATCHES = (3, 5, 7)
PM_OUTGOING = 1       # flags bit 0: pixels whose target leaves the frame do not count
PM_COUNTS = ("n_mask", "n_census", "n_valid", "n_nonfinite", "pixels")
PM_SUMS = ("l1_sum", "photo_sum", "hamming_sum", "census_sum", "ternary_sum")
PM_IMAGES = 10
PM_IMAGE_CENSUS_MEAN_SUM = 11
PM_RESERVED = 12      # 12 .. 15

EPI_LINEAR = 0
EPI_RELU = 1
EPI_RESID_RELU = 2
EPI_GRU_ZR = 3
EPI_GRU_Q = 4
EPI_TANH_RELU = 5
EPI_ADD_TO_OUT = 6


class ConvParams(ctypes.Structure):
    """Mirror of `raft_conv2d_params` (include/raft_hip.h)."""

    _fields_ = [
        ("in0", P), ("in0_ld", c_int), ("in0_c", c_int),
        ("in1", P), ("in1_ld", c_int), ("in1_c", c_int),
        ("batch", c_int), ("in_h", c_int), ("in_w", c_int),
        ("out_h", c_int), ("out_w", c_int),
        ("kh", c_int), ("kw", c_int), ("stride_h", c_int), ("stride_w", c_int), ("pad_h", c_int), ("pad_w", c_int),
        ("mode", c_int),
        ("weight", P), ("bias", P),
        ("n", c_int),
        ("out", P), ("out_ld", c_int),
        ("epilogue", c_int), ("alpha", c_float), ("split", c_int),
        ("aux0", P), ("aux0_ld", c_int),
        ("aux1", P), ("aux1_ld", c_int),
        ("out1", P), ("out1_ld", c_int),
        ("add0", P), ("add0_ld", c_int),
        ("precision", c_int),
        ("range_flag", P),
        ("stats_part", P), ("stats_ld", c_int),
        ("in_norm", P), ("in_norm_relu", c_int),
        ("weight_s", P),
    ]


CARRY_MAX_SEGS = 8   # RAFT_CARRY_MAX_SEGS


class Copy2D(ctypes.Structure):
    """Mirror of `raft_copy2d` (include/raft_hip.h): one pitched 2-D copy of raft_stream_carry_n."""

    _fields_ = [("src", P), ("src_ld", c_long), ("dst", P), ("dst_ld", c_long), ("rows", c_long), ("cols", c_long)]


CONV_KERNEL_HALO = 1
CONV_KERNEL_GEMM = 2
CONV_KERNEL_STEM = 3
CONV_KERNEL_SMALLN = 4
CONV_KERNEL_SMALLN3X3 = 5


class ConvForm(ctypes.Structure):
    """Mirror of `struct raft_conv2d_form` (include/raft_hip.h): the kernel form a conv launches."""

    _fields_ = [
        ("kernel", c_int), ("tile_rows", c_int), ("tile_cols", c_int), ("tiles_per_wg", c_int),
        ("loader_waves", c_int), ("compute_waves_per_simd", c_int), ("gemm_k_groups", c_int),
        ("smalln_tile_rows", c_int),
    ]

    def astuple(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


def conv_form(p: ConvParams) -> ConvForm:
    """raft_conv2d_form of p (host only: nothing is launched)."""
    f = ConvForm()
    call("raft_conv2d_form", ctypes.byref(p), ctypes.byref(f))
    return f


def conv_pair_form(p0: ConvParams, p1: ConvParams):
    """raft_conv2d_pair_form: (form of p0, form of p1, one_launch)."""
    f = (ConvForm * 2)()
    one = c_int(0)
    call("raft_conv2d_pair_form", ctypes.byref(p0), ctypes.byref(p1), f, ctypes.byref(one))
    return f[0], f[1], bool(one.value)


# name -> (restype, argtypes)
_PROTOS = {
    "raft_hip_abi_version": (c_int, []),
    "raft_hip_arch": (c_char_p, []),
    "raft_hip_last_error": (c_char_p, []),
    "raft_hip_source_hash": (c_char_p, []),
    "raft_debug_fill_lds_nan": (c_int, [P]),
    "raft_corr_pyramid_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "raft_corr_build": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, P, P]),
    "raft_corr_build_prec": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, P, P]),
    "raft_corr_build_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "raft_corr_build_ws_bytes_prec": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "raft_corr_build_ws": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, P, P, c_size_t, P]),
    "raft_corr_pyramid_level": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P]),
    "raft_corr_lookup": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, c_int, P, c_int, c_int, P, c_int, P, P]),
    "raft_corr_lookup_convf1": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, c_int, P, c_int, c_int, P, c_int, P,
                                        P, P, c_int, c_int, c_int, P, c_int, P, P]),
    "raft_convf1_flow": (c_int, [P, c_int, c_int, c_int, c_int, P, P, c_int, c_int, c_int, P, c_int, P, P]),
    "raft_corr_lookup_conv": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, c_int, P, P, c_int, P,
                                      c_int, P, P, P, c_int, c_int, P, c_int, P, P]),
    "raft_lookup_conv_weight_floats": (c_size_t, [c_int, c_int]),
    "raft_lookup_conv_pack_weight": (c_int, [P, c_int, c_int, c_int, P, P]),
    "raft_alt_corr_forward": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, P]),
    "raft_alt_corr_forward_prec": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                           c_int, P]),
    "raft_alt_corr_lookup_levels_prec": (c_int, [P, P, P, P, c_int, P, c_int, P, c_int, c_int, c_int, c_int, c_int,
                                                 c_int, ctypes.c_float, P, c_int, P, c_int, P]),
    "raft_alt_corr_lookup_nhwc_prec": (c_int, [P, P, P, c_int, c_float, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                               c_int, c_int, c_float, P, c_int, P, c_int, P]),
    "raft_alt_corr_lookup_levels": (c_int, [P, P, P, P, c_int, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                            ctypes.c_float, P, c_int, P, P]),
    "raft_alt_corr_lookup_nhwc": (c_int, [P, P, P, c_int, c_float, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                          c_int, c_float, P, c_int, P, P]),
    "raft_alt_corr_backward": (c_int, [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                       P, c_size_t, P]),
    "raft_alt_corr_backward_workspace_floats": (c_size_t, [c_int] * 8),
    "raft_avgpool2_nhwc": (c_int, [P, P, c_int, c_int, c_int, c_int, P]),
    "raft_conv2d_packed_shape": (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int),
                                         ctypes.POINTER(c_int)]),
    "raft_conv2d": (c_int, [ctypes.POINTER(ConvParams), P]),
    "raft_conv2d_pair": (c_int, [ctypes.POINTER(ConvParams), ctypes.POINTER(ConvParams), P]),
    "raft_conv2d_stats_slots": (c_int, [ctypes.POINTER(ConvParams)]),
    "raft_conv2d_halo_tile_rows": (c_int, [ctypes.POINTER(ConvParams)]),
    "raft_conv2d_halo_tiles_per_wg": (c_int, [ctypes.POINTER(ConvParams)]),
    "raft_conv2d_form": (c_int, [ctypes.POINTER(ConvParams), ctypes.POINTER(ConvForm)]),
    "raft_conv2d_pair_form": (c_int, [ctypes.POINTER(ConvParams), ctypes.POINTER(ConvParams),
                                      ctypes.POINTER(ConvForm), ctypes.POINTER(c_int)]),
    "raft_debug_launch_span": (c_int, [c_int]),
    "raft_debug_launch_span_read": (c_int, [P, c_int]),
    "raft_conv2d_in_norm_ok": (c_int, [ctypes.POINTER(ConvParams)]),
    "raft_instnorm_merge": (c_int, [P, c_int, c_int, c_int, c_int, c_float, P, P]),
    "raft_instnorm_merge_ws_floats": (c_size_t, [c_int, c_int, c_int]),
    "raft_instnorm_merge_ws": (c_int, [P, c_int, c_int, c_int, c_int, c_float, P, P, P]),
    "raft_instnorm_merge_counters": (c_size_t, [c_int, c_int]),
    "raft_conv2d_set_halo_loaders": (c_int, [c_int]),
    "raft_conv2d_set_halo_ks": (c_int, [c_int]),
    "raft_instnorm_merge_fused": (c_int, [P, c_int, c_int, c_int, c_int, c_float, P, P, P, P]),
    "raft_conv2d_split_weight": (c_int, [P, P, c_int, c_int, P]),
    "raft_conv2d_split_weight_prec": (c_int, [P, P, c_int, c_int, c_int, P]),
    "raft_conv2d_split_scaled_bytes": (c_size_t, [c_int, c_int]),
    "raft_conv2d_split_weight_scaled": (c_int, [P, P, c_int, c_int, P]),
    "raft_instnorm_workspace_floats": (c_size_t, [c_int, c_int, c_int]),
    "raft_instnorm_stats": (c_int, [P, c_int, c_int, c_int, c_int, c_float, P, P, P]),
    "raft_groupnorm_stats": (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_float, P, P]),
    "raft_norm_apply_affine": (c_int, [P, c_int, P, P, P, P, c_int, P, P, P, c_int, P, c_int, c_int, c_int, c_int, P]),
    "raft_instnorm_apply": (c_int, [P, c_int, P, P, c_int, P, c_int, P, c_int, c_int, c_int, c_int, P]),
    "raft_prep_images": (c_int, [P, P, P, c_int, c_int, c_int, P]),
    "raft_init_coords": (c_int, [P, P, c_int, c_int, c_int, P]),
    "raft_flow_from_coords": (c_int, [P, P, c_int, c_int, c_int, P]),
    "raft_convex_upsample": (c_int, [P, P, c_int, P, c_int, c_int, c_int, P]),
    "raft_upflow8": (c_int, [P, P, c_int, c_int, c_int, P]),
    "raft_nchw_to_nhwc": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P]),
    "raft_nhwc_to_nchw": (c_int, [P, c_int, P, c_int, c_int, c_int, c_int, P]),
    "raft_pad_replicate": (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "raft_bilinear_sample": (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    "raft_forward_interpolate": (c_int, [P, P, c_int, c_int, c_int, P]),
    "raft_frame_pad": (None, [c_int, c_int, c_int] + [ctypes.POINTER(c_int)] * 4),
    "raft_ingest_frame": (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P, P]),
    "raft_stream_carry": (c_int, [P, P, c_size_t, P, P, c_size_t, P, P, c_size_t, P]),
    "raft_stream_carry_n": (c_int, [P, c_int, P]),
    "raft_fb_consistency": (c_int, [P, c_long, c_long, c_long, P, c_long, c_long, c_long, c_int, c_int, c_int, c_int,
                                    c_int, c_float, c_float, P, P, P, P, P]),
    "raft_flow_viz_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "raft_flow_to_rgb": (c_int, [P, c_long, c_long, c_long, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_int,
                                 P, c_long, c_long, c_long, P, P, P]),
    "raft_warp_frame": (c_int, [P, c_long, c_long, c_long, P, c_int, c_long, c_long, c_long, c_int, c_int, c_int,
                                c_int, c_int, c_int, c_int, P, c_int, P, P]),
    "raft_splat_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "raft_splat_density": (c_int, [P, c_long, c_long, c_long, c_int, c_int, c_int, c_int, c_int, P, P, P]),
    "raft_resize": (c_int, [P, c_int, c_long, c_long, c_long, c_int, c_int, c_int, c_int, c_int, c_int, P, c_int,
                            c_int, c_int, c_int, c_int, c_float, c_float, P]),
    "raft_flow_metrics_ws_bytes": (c_size_t, [c_int, c_int, c_int]),
    "raft_flow_metrics": (c_int, [P, c_long, c_long, c_long, P, c_long, c_long, c_long, P, c_int, c_long, c_long,
                                  c_int, c_int, c_int, c_float, P, P, P, P, P]),
    "raft_photo_metrics_ws_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "raft_photo_metrics": (c_int, [P, c_long, c_long, c_long, P, c_long, c_long, c_long, c_int, P, c_long, c_long,
                                   c_long, P, c_int, c_long, c_long, c_int, c_int, c_int, c_int, c_int, P, P, P, P,
                                   P]),
}

EXPORTED = tuple(_PROTOS)

_lib = None
_lock = threading.Lock()


class RaftHipError(RuntimeError):
    pass


def load():
    """Load libraft_hip.so (once).  Raises RaftHipError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RaftHipError(
                f"libraft_hip.so not found at {LIB_PATH}: build it with `python __graft_entry__.py build` "
                "(there is no CPU fallback)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.raft_hip_abi_version() != ABI_VERSION:
            raise RaftHipError("libraft_hip.so ABI version mismatch")
        want = source_hash()
        got = lib.raft_hip_source_hash().decode()
        if want is not None and got != want and os.environ.get("RAFT_SKIP_SRC_CHECK", "0") != "1":
            raise RaftHipError(f"{LIB_PATH} was built from other sources (hash {got}, the sources here hash "
                               f"{want}; the hash covers csrc/*.hip, csrc/*.hpp and include/raft_hip.h): rebuild it "
                               f"with `python __graft_entry__.py build`, or set RAFT_SKIP_SRC_CHECK=1 to load it anyway")
        _lib = lib
        return lib


def source_hash() -> str | None:
    """sha256[:16] of the HIP sources beside this package, as csrc/Makefile bakes into the library
    (raft_hip_source_hash); None when the sources are not present."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    mk = os.path.join(csrc, "Makefile")
    hdr = os.path.join(os.path.dirname(_HERE), "include", "raft_hip.h")
    if not (os.path.exists(mk) and os.path.exists(hdr)):
        return None
    with open(mk) as fh:
        srcs = next((ln.split(":=", 1)[1].split() for ln in fh if ln.startswith("SRCS :=")), None)
    if not srcs:
        raise RaftHipError(f"{mk} has no one-line 'SRCS := ...' list: cannot hash the HIP sources to check "
                           f"{LIB_PATH} against them (RAFT_SKIP_SRC_CHECK=1 skips the check)")
    files = [os.path.join(csrc, f) for f in srcs] + sorted(glob.glob(os.path.join(csrc, "*.hpp"))) + [hdr]
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def check(rc: int, what: str):
    if rc != 0:
        msg = _lib.raft_hip_last_error().decode(errors="replace") if _lib is not None else ""
        raise RaftHipError(f"{what} failed (rc={rc}): {msg}")


def call(name: str, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    check(rc, name)
    return rc
