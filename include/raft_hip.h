/*
 * raft_hip.h — C-ABI of the MI355X-native RAFT inference path (libraft_hip.so).
 *
 * Plain pointers, sizes and a hipStream_t (passed as void*).  No allocation
 * happens inside any entry point (callers own every buffer, including the
 * workspaces whose sizes the *_workspace_floats queries return), nothing
 * synchronises the host, so every call is legal inside hipStreamBeginCapture
 * (hipGraph capture).  Every entry point returns 0 on success, a positive
 * hipError_t from the launch, or a negative RAFT_E_* argument error; the
 * message of the last failure on the calling thread is raft_hip_last_error().
 *
 * All device buffers are fp32.  "NHWC rows" means pixel-major rows of `ld`
 * floats: element (pixel m, channel c) lives at ptr[m * ld + c], with pixel
 * m = (b * H + y) * W + x.
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   raft_alt_corr_forward   <- alt_cuda_corr.forward   (alt_cuda_corr/correlation.cpp:23-33,
 *                                                      correlation_kernel.cu:260-286)
 *   raft_alt_corr_backward  <- alt_cuda_corr.backward  (alt_cuda_corr/correlation.cpp:36-48,
 *                                                      correlation_kernel.cu:288-324)
 *   raft_corr_build         <- CorrBlock.__init__ + CorrBlock.corr (core/corr.py:25-54, 96-127)
 *   raft_corr_lookup        <- CorrBlock.__call__ + bilinear_sampler (core/corr.py:56-94,
 *                                                      core/utils/utils.py:57-71)
 *   raft_corr_lookup_conv   <- corr_fn(coords1) + BasicMotionEncoder.convc1 / convf1
 *                              (core/raft.py:219, core/update.py:185-205)
 *   raft_conv2d             <- nn.Conv2d + fused activations / GRU gates of
 *                              core/update.py:6-325 and core/extractor.py:6-267
 *   raft_instnorm_*         <- nn.InstanceNorm2d in core/extractor.py (norm_fn='instance')
 *   raft_convex_upsample    <- RAFT.upsample_flow (core/raft.py:112-142)
 *   raft_upflow8            <- upflow8 (core/utils/utils.py:80-82)
 *   raft_prep_images        <- RAFT.forward normalisation 2*(x/255)-1 (core/raft.py:164-169)
 *   raft_avgpool2_nhwc      <- F.avg_pool2d(x, 2, stride=2) in AlternateCorrBlock (core/corr.py:157-161)
 *   raft_pad_replicate      <- InputPadder.pad (core/utils/utils.py:7-24, F.pad mode='replicate')
 *   raft_bilinear_sample    <- bilinear_sampler (core/utils/utils.py:57-71)
 *   raft_forward_interpolate <- forward_interpolate (core/utils/utils.py:26-54; scipy griddata 'nearest')
 *   raft_ingest_frame       <- InputPadder.pad + RAFT.forward's normalisation, of one video frame
 *                              (core/utils/utils.py:7-24, core/raft.py:164-169)
 */
#ifndef RAFT_HIP_H_
#define RAFT_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAFT_HIP_ABI_VERSION 19

/* Negative return codes (argument errors, raised before any launch). */
#define RAFT_E_INVALID (-1)   /* bad size / null pointer / unsupported shape */
#define RAFT_E_ALIGN (-2)     /* pointer or leading dimension not aligned as required */

typedef void* raft_stream_t;  /* hipStream_t; NULL = the legacy default stream */

int raft_hip_abi_version(void);
const char* raft_hip_arch(void);        /* offload arch the library was built for ("gfx950") */
const char* raft_hip_last_error(void);  /* message of the last failure on this thread ("" if none) */
/* first 16 hex digits of the sha256 of the sources the library was built from (csrc/Makefile
 * SRC_HASH: the .hip files in SRCS order, the csrc .hpp headers and include/raft_hip.h); the loader
 * refuses a library whose hash differs from the sources beside it (a stale prebuilt .so) */
const char* raft_hip_source_hash(void);
/* Launch-span timing (bench / profiling): after raft_debug_launch_span(1) every
 * raft_corr_lookup_conv launch takes the next of 256 slots and records the realtime counter
 * (100 MHz) at its first work-group's start and at its last work-group's end, after that
 * work-group's stores completed; raft_debug_launch_span_read copies n values (slot k: [2k] start,
 * [2k+1] end).  raft_debug_launch_span(0) clears the slots and stops numbering.  Valid for eager
 * launches from one host thread on one device only: a launch enqueued while its stream is being
 * captured takes no slot (a graph would replay the slot it baked in). */
int raft_debug_launch_span(int enable);
int raft_debug_launch_span_read(unsigned long long* host, int n);
/* Debug (tests only): fill the LDS of every CU with all-ones words (NaN as fp32, f16 and bf16) by
 * kernels that take a CU's whole 160 KiB each; no global memory is touched.  A kernel launched next
 * on the stream that reads LDS it did not write then sees NaN: the parity tests run every launch of
 * a forward behind it and require the bit-identical, finite result (round 3's conv_stem K-padding
 * read was such a bug). */
int raft_debug_fill_lds_nan(raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * All-pairs correlation pyramid (CorrBlock)
 *
 * fmap1, fmap2: NHWC rows [B*H*W][ld] (channels 0..C-1 used, C % 4 == 0, 16-B aligned).
 * pyramid: num_levels levels stored back to back, H_0 = H, H_{l+1} = floor(H_l / 2)
 *   (same for W).  Every query pixel's level-l map is stored in 4x4 TILES:
 *   TH_l = ceil(H_l/4), TW_l = ceil(W_l/4), map size S_l = TH_l*TW_l*16 floats,
 *   element (y, x) at ((y>>2)*TW_l + (x>>2))*16 + (y&3)*4 + (x&3), padding = 0;
 *   the map of query pixel p of batch b starts at pyramid + off_l + (b*H*W + p)*S_l,
 *   off_l = B*H*W * sum_{j<l} S_j.  (64-B tiles = the HBM read granule: a
 *   radius-4 window touches ~10.6 tiles instead of ten straddling row runs.)
 * Level 0 = <fmap1[p], fmap2[q]> / sqrt_c (a division, as core/corr.py:127);
 * level l+1 = 2x2 average pool (floor) of level l, bit for bit (((a0+a1)+a2)+a3)/4 of
 * the stored level l in fp32.  16-byte aligned buffers.
 *
 * What the builds read and write (every line asserted by tests/test_gpu_corr_build_forms.py):
 *   * Only channels 0..C-1 of rows 0..B*H*W-1 are read: the ld - C columns and the memory
 *     around the operands are never touched.
 *   * Every float of the pyramid is written.  The padding of every level is exactly 0 in
 *     the maps of every query whose own features are finite, whatever fmap2 holds; a query
 *     with a non-finite feature gets non-finite valid elements and unspecified padding at
 *     level 0 (deeper levels: padding 0).
 *   * Non-finite features: a NaN or +-Inf in fmap1 row p changes only query p's maps; in
 *     fmap2 row q of image b it makes non-finite exactly the level-0 element q of every
 *     query of image b and the pooled cells that contain it (a last row / column that the
 *     floor pool drops reaches no deeper level).  Every other float of the buffer is bit
 *     for bit what it is with that feature set to 0.
 *   * RAFT_PREC_F16X3 magnitude contract.  The split hi = f16(x), lo = f16(x - hi) is
 *     unscaled.  "~2^-22 relative per product" holds while lo is a normal f16, i.e. for
 *     features of size 2^-3 .. 2^15: against mag = sum_c |f1_c f2_c| / sqrt_c the largest
 *     error of the documented arithmetic in fp32 is 1.3 x 2^-24 mag (C = 256; 2.2 at
 *     C = 64) for N(0, s^2) features at every s from 2^12 down to 2^-2.  Below, lo falls
 *     into the f16 subnormals (step 2^-24) and the error grows as 1 / s: 1.7 x 2^-24 mag
 *     at s = 2^-3, 2.8 at 2^-4, 11 at 2^-6, 45 at 2^-8, 730 at 2^-12 (C = 256; C = 64:
 *     3.4, 6.4, 25, 108, 1380).  RAFT_PREC_FP32 has no such range (3.7 / 4.3 at every s).
 *   * RAFT_PREC_F16X3 needs |fmap| < 65520 (every value that rounds to a finite f16,
 *     the largest being 65504).  A larger finite value splits into hi = inf, lo = -inf:
 *     every element it enters is NaN, exactly as for a non-finite feature (rule above).
 *     RAFT_PREC_FP32 takes any finite fp32.
 * --------------------------------------------------------------------------- */
size_t raft_corr_pyramid_floats(int B, int H, int W, int num_levels);
int raft_corr_build(const float* fmap1, const float* fmap2, int ld, int B, int H, int W, int C,
                    int num_levels, float sqrt_c, float* pyramid, raft_stream_t stream);
/* The same with the GEMM arithmetic chosen: RAFT_PREC_FP32 (raft_corr_build: f32
 * MFMA) or RAFT_PREC_F16X3 (both fmaps split into f16 hi + lo at staging,
 * hi*hi + lo*hi + hi*lo with fp32 accumulation: ~2^-22 relative per product,
 * 5x the MFMA rate).  The RAFT forward uses F16X3 unless conv_precision="fp32". */
int raft_corr_build_prec(const float* fmap1, const float* fmap2, int ld, int B, int H, int W, int C,
                         int num_levels, float sqrt_c, int precision, float* pyramid, raft_stream_t stream);
/* raft_corr_build_prec with a workspace (the forward's build): in RAFT_PREC_F16X3 with C % 16 == 0,
 * 64 <= C <= 1024, both fmaps are split once into f16 hi | lo maps in ws and the volume is built on
 * 256 x 256 tiles (one fp32 accumulator chain for hi*hi, lo*hi, hi*lo; same ~2^-22 relative
 * accuracy); otherwise it is raft_corr_build_prec.  ws: >= raft_corr_build_ws_bytes(B, H, W, C)
 * bytes, 16-byte aligned; ws == NULL, or fmaps / pyramid / ws off 16-B alignment, also take
 * raft_corr_build_prec (ws_bytes may then be 0).  RAFT_CORR_BUILD4=0: always raft_corr_build_prec.
 * (Argument order since ABI 15: ..., pyramid, ws, ws_bytes, stream.) */
size_t raft_corr_build_ws_bytes(int B, int H, int W, int C);
/* The workspace raft_corr_build_ws needs for its 256 x 256 kernel at this shape and precision, or 0 when that
 * call would take raft_corr_build_prec's kernel (not f16x3, C not a multiple of 16 in [64, 1024], maps past
 * 2^31 bytes, or RAFT_CORR_BUILD4=0): callers size the workspace from it instead of restating the rule. */
size_t raft_corr_build_ws_bytes_prec(int B, int H, int W, int C, int precision);
int raft_corr_build_ws(const float* fmap1, const float* fmap2, int ld, int B, int H, int W, int C,
                       int num_levels, float sqrt_c, int precision, float* pyramid, void* ws, size_t ws_bytes,
                       raft_stream_t stream);
/* Row-major copy of one level, out [B*H*W][H_l][W_l] (the reference's corr_pyramid[l]). */
int raft_corr_pyramid_level(const float* pyramid, int B, int H, int W, int num_levels, int level,
                            float* out, raft_stream_t stream);

/* Radius-r bilinear window lookup of every level (CorrBlock.__call__).
 * coords: (x, y) per query pixel; coords_layout 0 = NHWC [B*H*W][2],
 *         1 = NCHW [B][2][H][W] (the reference's tensor as it stands).
 * out: out_layout 0 = NHWC rows [B*H*W][out_ld], channel lvl*(2r+1)^2 + ix*(2r+1) + iy;
 *      out_layout 1 = NCHW [B][L*(2r+1)^2][H][W] (out_ld ignored).
 * flow_out (optional, may be NULL): NHWC rows [B*H*W][flow_ld] receive
 *      coords - coords_grid (the RAFT loop's `flow`, core/raft.py:222).
 * range_flag (optional, may be NULL): set to 1 when an output exceeds RAFT_RANGE_LIMIT in
 *      magnitude (see the f16x3 range guard below).
 * Any fp32 coordinate is accepted and no address depends on it unchecked.  A tap's sample
 * position is computed in fp32 as the reference does (x / 2^l + offset, 2 X / (W_l - 1) - 1,
 * back through (g + 1) / 2 * (W_l - 1)): a tap whose position is finite but far off the map is
 * 0 (grid_sample's zero padding), however far (1e6, 3e9, past the int range); a tap whose
 * position on either axis is not finite (a NaN or infinite coordinate, |2 X| overflowing fp32,
 * or a 1-px level, W_l - 1 = 0) is NaN, as the reference's.  Other pixels are unaffected.
 * flow_out is coords - coords_grid in fp32 whatever the coordinate.  The same holds for
 * raft_corr_lookup_convf1 and raft_corr_lookup_conv. */
int raft_corr_lookup(const float* pyramid, int B, int H, int W, int num_levels, int radius,
                     const float* coords, int coords_layout, float* out, int out_ld, int out_layout,
                     float* flow_out, int flow_ld, int* range_flag, raft_stream_t stream);
/* raft_corr_lookup and, in the same launch, the motion encoder's first flow conv
 * (BasicMotionEncoder.convf1, core/update.py:186,205): f1_out rows [B*H*W][f1_out_ld]
 * (16-B aligned, ld % 4 == 0) = relu(conv7x7(flow) + f1_bias), flow = coords - coords_grid
 * with zero padding, as the reference's F.relu(self.convf1(flow)).  The convf1 work-groups
 * run on the VALU beside the lookup's memory-bound waves instead of as a launch of their own.
 * f1_weight: [f1_n/32][k*k][2][32] fp32 (16-B aligned), element ((g*k*k + dy*k + dx)*2 + ci)*32 + j
 * = weight[32g + j][ci][dy][dx] of the OIHW tensor; f1_k = 7, f1_n % 32 == 0.  Products are
 * exact fp32; f1_precision RAFT_PREC_F16 / RAFT_PREC_BF16 rounds the flow operand to that
 * type (round the weights the same way, as the MFMA kernels' operands).  f1_range_flag:
 * the range guard of the output (it feeds the split-precision convf2), or NULL.  The lookup
 * outputs are bit-identical to raft_corr_lookup's. */
int raft_corr_lookup_convf1(const float* pyramid, int B, int H, int W, int num_levels, int radius,
                            const float* coords, int coords_layout, float* out, int out_ld, int out_layout,
                            float* flow_out, int flow_ld, int* range_flag, const float* f1_weight,
                            const float* f1_bias, int f1_n, int f1_k, int f1_precision, float* f1_out,
                            int f1_out_ld, int* f1_range_flag, raft_stream_t stream);
/* The same convf1 alone (the alternate-correlation loop, whose lookup launch has no room
 * for it): f1_out = relu(conv7x7(coords - coords_grid) + f1_bias), arguments as above. */
int raft_convf1_flow(const float* coords, int coords_layout, int B, int H, int W, const float* f1_weight,
                     const float* f1_bias, int f1_n, int f1_k, int f1_precision, float* f1_out, int f1_out_ld,
                     int* f1_range_flag, raft_stream_t stream);

/* The lookup fused with the motion encoder's first convs (RAFT-full: radius 4, 4 levels), ONE
 * launch per iteration of the all-pairs loop (core/corr.py:56-94 + core/update.py:185-205):
 *   c1_out rows [B*H*W][c1_out_ld] = relu(convc1(corr) + c1_bias), convc1 = the 1x1 324 -> 256 conv
 *   over the lookup's 324 channels (channel order of raft_corr_lookup); the correlation rows never
 *   leave the work-group (LDS), so they are not an output;
 *   f1_out rows [B*H*W][f1_out_ld] = relu(convf1(flow) + f1_bias), convf1 the 7x7 2 -> 128 conv of
 *   flow = coords - coords_grid (zero padding), f1_k = 7;
 *   flow_out (optional): as raft_corr_lookup.
 * Both convs in `precision` (RAFT_PREC_F16X3 / F16 / BF16: the arithmetic of raft_conv2d).
 * coords: NHWC [B*H*W][2].  c1_weight / f1_weight: raft_lookup_conv_pack_weight's output for the
 * split form (raft_conv2d_split_weight_prec, `precision`) of the conv's packed weight (convc1
 * [256][352] RAFT_CONV_VEC, convf1 [128][128] RAFT_CONV_GATHER), 16-B aligned.  range_flag: raised
 * by a lookup tap above RAFT_RANGE_LIMIT (the split convc1 input); c1_range_flag / f1_range_flag:
 * by the convc1 / convf1 outputs (split convc2 / convf2 inputs).  Returns RAFT_E_INVALID for any
 * other radius / level count / channel count (the caller then runs raft_corr_lookup_convf1 +
 * raft_conv2d). */
int raft_corr_lookup_conv(const float* pyramid, int B, int H, int W, int num_levels, int radius,
                          const float* coords, float* flow_out, int flow_ld, int* range_flag, int precision,
                          const void* c1_weight, const float* c1_bias, int c1_n, float* c1_out, int c1_out_ld,
                          int* c1_range_flag, const void* f1_weight, const float* f1_bias, int f1_n, int f1_k,
                          float* f1_out, int f1_out_ld, int* f1_range_flag, raft_stream_t stream);
/* convc1's split weight [n_pad][k_pad] (k_pad % 32 == 0) -> raft_corr_lookup_conv's fragment order:
 * [k_pad/32][n/32][4][64] x 16 B, element (j, s, t, lane) = 8 halves of split row 32s + lane%32,
 * K-step j, quad (t/2)*4 + 2*(lane/32) + t%2; out holds raft_lookup_conv_weight_floats(n, k_pad)
 * floats (16-B aligned). */
size_t raft_lookup_conv_weight_floats(int n, int k_pad);
int raft_lookup_conv_pack_weight(const void* split_weight, int n_pad, int k_pad, int n, void* out,
                                 raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * On-the-fly ("alternate") correlation — the alt_cuda_corr plugin.
 *
 * fmap1 [B][H1][W1][C], fmap2 [B][H2][W2][C] (NHWC, contiguous),
 * coords [B][N][H1][W1][2] (x, y in fmap2 pixels).
 * corr [B][N][(2r+1)^2][H1][W1], channel iy + (2r+1)*ix, every element
 * written (no pre-zeroing needed), divided by `scale_div` (1.0f = the
 * reference's unscaled output; sqrtf(C) = AlternateCorrBlock's / sqrt(dim),
 * core/corr.py:198).
 *
 * Coordinates, on every entry and kernel form below (tests/test_gpu_alt_corr_forms.py):
 *   - the sample position is coords / coord_div in fp32; its window is the (2r+2)^2 integer taps
 *     from floor(position) - r, blended with the fp32 fractions position - floor(position);
 *   - a finite coordinate, however large: taps off fmap2 are 0, a window wholly off the map gives
 *     bins of exactly +-0;
 *   - a non-finite coordinate on either axis (after the division): every bin of that query at
 *     that level is NaN.  No address depends on such a coordinate.  Queries in other 8x8 query
 *     tiles are bit-identical to a call in which that query has an ordinary coordinate; queries
 *     of the same tile stay within the precision's bound (their tile is computed per pixel, in
 *     exact fp32);
 *   - flow_out (where an entry has it) is coords - coords_grid in fp32 from the coordinate as
 *     given, for any coord_div > 0 (inf and NaN follow fp32 arithmetic);
 *   - backward: a query with a non-finite coordinate, or with |coordinate| >= 1e8 on either
 *     axis, contributes nothing: no fmap1_grad / fmap2_grad contribution, coords_grad (0, 0).
 * --------------------------------------------------------------------------- */
int raft_alt_corr_forward(const float* fmap1, const float* fmap2, const float* coords, float* corr,
                          int B, int H1, int W1, int H2, int W2, int C, int N, int radius, float scale_div,
                          raft_stream_t stream);
/* Arithmetic of the alternate lookups: RAFT_PREC_FP32 = exact fp32 products on the VALU (the
 * reference kernel's arithmetic; raft_alt_corr_forward, the plugin's entry point, always uses
 * it); any other value = the fp32-accurate f16x3 box GEMM on MFMA where it applies (r = 4,
 * C % 32 == 0, C <= 256; exact only while |fmap| < 65504: the RAFT forward's range guard covers
 * it), exact fp32 elsewhere.  raft_alt_corr_lookup_nhwc / raft_alt_corr_lookup_levels below
 * are the _prec forms with RAFT_PREC_F16X3.
 * The box GEMM splits x into hi = f16(x) and an UNSCALED lo = f16(x - hi) and keeps hi*hi +
 * lo*hi + hi*lo: ~2^-22 of sum_c |f1_c f2_c| per tap while lo is a normal f16, i.e. for feature
 * values of 2^-3 <= |x| < 65504.  Below 2^-3, lo falls into the f16 subnormals (absolute step
 * 2^-24), so an element x carries an absolute error of up to 2^-25 whatever its size: maps of
 * typical magnitude s < 1 lose about a factor 1 / s (measured against fp64 on unit-variance
 * maps scaled by s, in 2^-24 sum|f1 f2|: 1.2 at s = 1 and 64, 4.4 at 2^-4, 69 at 2^-8; DESIGN.md
 * 7.3).  RAFT_PREC_FP32 has no such range. */
int raft_alt_corr_forward_prec(const float* fmap1, const float* fmap2, const float* coords, float* corr,
                               int B, int H1, int W1, int H2, int W2, int C, int N, int radius, float scale_div,
                               int precision, raft_stream_t stream);

/* Same computation, NHWC output: out rows [B*H1*W1][out_ld] at channel
 * offset already applied by the caller; coords_layout as raft_corr_lookup
 * (coordinates are divided by coord_div before use: 2**level in RAFT);
 * range_flag as raft_corr_lookup. */
int raft_alt_corr_lookup_nhwc(const float* fmap1, const float* fmap2, const float* coords, int coords_layout,
                              float coord_div, float* out, int out_ld, int B, int H1, int W1, int H2, int W2,
                              int C, int radius, float scale_div, float* flow_out, int flow_ld,
                              int* range_flag, raft_stream_t stream);
int raft_alt_corr_lookup_nhwc_prec(const float* fmap1, const float* fmap2, const float* coords, int coords_layout,
                                   float coord_div, float* out, int out_ld, int B, int H1, int W1, int H2, int W2,
                                   int C, int radius, float scale_div, float* flow_out, int flow_ld,
                                   int* range_flag, int precision, raft_stream_t stream);
/* All L levels of AlternateCorrBlock.__call__ (core/corr.py:163-198, the L calls of
 * alt_cuda_corr.forward of :176-186) as one call: level l reads fmap2_levels[l] (NHWC,
 * h2s[l] x w2s[l]) with the coordinates divided by 2^l and writes output channels
 * l*(2r+1)^2 .. of each NHWC row; flow_out as raft_alt_corr_lookup_nhwc (written once).  RAFT's
 * case (r = 4, C % 32 == 0, C <= 256) is ONE launch whose work-groups stage their fmap1 tile
 * once for every level; otherwise L launches of raft_alt_corr_lookup_nhwc.  Results equal the
 * L separate calls.  The pointer / size arrays are read on the host during the call. */
int raft_alt_corr_lookup_levels(const float* fmap1, const float* const* fmap2_levels, const int* h2s,
                                const int* w2s, int L, const float* coords, int coords_layout, float* out,
                                int out_ld, int B, int H1, int W1, int C, int radius, float scale_div,
                                float* flow_out, int flow_ld, int* range_flag, raft_stream_t stream);
int raft_alt_corr_lookup_levels_prec(const float* fmap1, const float* const* fmap2_levels, const int* h2s,
                                     const int* w2s, int L, const float* coords, int coords_layout, float* out,
                                     int out_ld, int B, int H1, int W1, int C, int radius, float scale_div,
                                     float* flow_out, int flow_ld, int* range_flag, int precision,
                                     raft_stream_t stream);

/* Gradients of raft_alt_corr_forward (unscaled), replacing correlation_kernel.cu:122-256:
 * every output is written (no pre-zeroing) and bit-identical run to run.  fmap1_grad is
 * a gather over each query's taps; fmap2_grad inverts the (query, tap) -> fmap2 pixel map
 * (a stable sort of the queries by window origin, then a gather per fmap2 pixel) instead
 * of the reference's float atomics; coords_grad is the true gradient through the bilinear
 * weights (the reference leaves it zero, correlation_kernel.cu:307).  workspace: at least
 * raft_alt_corr_backward_workspace_floats(...) floats, 256-byte aligned.  C % 4 == 0,
 * C <= 1024, radius <= 32 (the forward's range).  Absent queries (non-finite or |coordinate| >=
 * 1e8): see "Coordinates" above. */
int raft_alt_corr_backward(const float* fmap1, const float* fmap2, const float* coords, const float* corr_grad,
                           float* fmap1_grad, float* fmap2_grad, float* coords_grad,
                           int B, int H1, int W1, int H2, int W2, int C, int N, int radius,
                           float* workspace, size_t workspace_floats, raft_stream_t stream);
size_t raft_alt_corr_backward_workspace_floats(int B, int H1, int W1, int H2, int W2, int C, int N, int radius);

/* 2x2 / stride-2 average pool (floor), NHWC contiguous [B][H][W][C] -> [B][H/2][W/2][C]. */
int raft_avgpool2_nhwc(const float* in, float* out, int B, int H, int W, int C, raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * Convolution as implicit GEMM on MFMA, NHWC.
 * M = batch*out_h*out_w pixels, N = out channels, K = taps x input channels.
 * The input is a virtual concat of up to two NHWC row sources (seg 0, then
 * seg 1), which is how torch.cat([...], dim=1) of the reference is elided.
 *
 * Packed weights (see raft_conv2d_packed_shape):
 *   mode RAFT_CONV_VEC    (every segment's channel count % 4 == 0, seg0 % 32 == 0
 *                          when seg 1 is used): w[n_pad][KH*KW][c_pad],
 *                          c_pad = roundup(c0 + c1, 32), zero padded;
 *   mode RAFT_CONV_GATHER (small inputs, e.g. 2- or 3-channel):
 *                          w[n_pad][k_pad], k = (ky*KW + kx)*(c0+c1) + c,
 *                          k_pad = roundup(KH*KW*(c0+c1), 32), zero padded;
 *   n_pad = roundup(N, 64).
 *
 * Arithmetic (params.precision):
 *   RAFT_PREC_FP32   v_mfma_f32_32x32x2_f32 on the fp32 packed weight.
 *   RAFT_PREC_F16X3  fp32-accurate split: every operand x = hi + lo/2048 with
 *                    hi = f16(x), lo = f16((x - hi) * 2048); products
 *                    hi*hi + (hi*lo + lo*hi)/2048 on v_mfma_f32_32x32x16_f16
 *                    with fp32 accumulation (the lo*lo term, 2^-22 relative,
 *                    is dropped).  Weight: the split form of the packed
 *                    weight (raft_conv2d_split_weight), same byte size.
 *   RAFT_PREC_F16    one f16 product (hi*hi), fp32 accumulation: the mixed-
 *                    precision mode (reference: autocast, core/raft.py:156);
 *                    uses the same split weight.
 *   RAFT_PREC_BF16   one bf16 product, fp32 accumulation, on v_mfma_f32_32x32x16_bf16
 *                    (bf16 mixed precision: the reference under a bf16 autocast;
 *                    fp32's exponent range).  Weight: raft_conv2d_split_weight_prec
 *                    with RAFT_PREC_BF16 (32 bf16 hi then 32 bf16 lo per K-step).
 * N <= 4 convolutions always take the fp32 packed weight (VALU kernel).
 * --------------------------------------------------------------------------- */
#define RAFT_CONV_VEC 0
#define RAFT_CONV_GATHER 1

#define RAFT_PREC_FP32 0
#define RAFT_PREC_F16X3 1
#define RAFT_PREC_F16 2
#define RAFT_PREC_BF16 3

/* epilogues: v = acc + bias[n] */
#define RAFT_EPI_LINEAR 0         /* out = alpha * v                                          */
#define RAFT_EPI_RELU 1           /* out = relu(v)                                            */
#define RAFT_EPI_RESID_RELU 2     /* out = relu(aux0[m,n] + relu(v))    (ResidualBlock tail) */
#define RAFT_EPI_GRU_ZR 3         /* n <  split: out[m,n] = sigmoid(v) (z); split % 32 == 0      */
                                  /* n >= split: out1[m,n-split] = sigmoid(v)*aux0[m,n-split] (r*h) */
#define RAFT_EPI_GRU_Q 4          /* q = tanh(v); out[m,n] = (1-aux1[m,n])*aux0[m,n] + aux1[m,n]*q */
#define RAFT_EPI_TANH_RELU 5      /* n < split: out[m,n] = tanh(v); else out1[m,n-split] = relu(v); split % 32 == 0 */
#define RAFT_EPI_ADD_TO_OUT 6     /* out[m,n] = out[m,n] + v   (coords1 += delta_flow)         */

typedef struct raft_conv2d_params {
  const float* in0; int in0_ld; int in0_c;  /* seg 0: NHWC rows, first channel at in0 */
  const float* in1; int in1_ld; int in1_c;  /* seg 1 (in1_c = 0: unused) */
  int batch, in_h, in_w;
  int out_h, out_w;
  int kh, kw, stride_h, stride_w, pad_h, pad_w;
  int mode;                                 /* RAFT_CONV_VEC / RAFT_CONV_GATHER */
  const float* weight;                      /* packed, see above */
  const float* bias;                        /* [N] or NULL */
  int n;                                    /* output channels N */
  float* out; int out_ld;
  int epilogue; float alpha; int split;
  const float* aux0; int aux0_ld;
  const float* aux1; int aux1_ld;
  float* out1; int out1_ld;
  const float* add0; int add0_ld;           /* optional addend rows: v = acc + bias[n] + add0[m,n]
                                               (a precomputed partial sum, e.g. the GRU's
                                               iteration-invariant context term) */
  int precision;                            /* RAFT_PREC_* (weight format follows it) */
  int* range_flag;                          /* optional (NULL = off): set to 1 when an output
                                               exceeds RAFT_RANGE_LIMIT in magnitude */
  float* stats_part; int stats_ld;          /* optional (NULL = off): InstanceNorm partial statistics
                                               of the output, see raft_conv2d_stats_slots */
  const float* in_norm; int in_norm_relu;   /* optional (NULL = off): the conv reads
                                               act((seg0 - mean[b][c]) * rstd[b][c]) instead of seg 0,
                                               in_norm = [batch][in0_c][2] {mean, rstd} (the output of
                                               raft_instnorm_stats / _merge), act = relu if
                                               in_norm_relu; zero padding stays zero.  Only where
                                               raft_conv2d_in_norm_ok says so. */
  const void* weight_s;                     /* optional (NULL = off), RAFT_PREC_F16X3 only: the
                                               column-scaled split of the same weight
                                               (raft_conv2d_split_weight_scaled).  With it, multi-
                                               round stride-1 3x3 convs run on 256-pixel x 64-
                                               column tiles whose three products share one
                                               accumulator; without it they keep the 128-pixel
                                               tiles.  Same results to fp32 rounding. */
} raft_conv2d_params;

/* f16x3 range guard.  RAFT_PREC_F16X3 splits every activation x as hi = f16(x), which is
 * only exact for |x| < 65504: a larger conv input would silently become inf.  Producers
 * whose outputs feed a split-precision conv (conv epilogues, the correlation lookups) can
 * raise a device flag when any output exceeds RAFT_RANGE_LIMIT = 2^15 (NaN does not raise
 * it: a NaN input propagates as in fp32); the caller checks the flag after the forward and
 * re-runs it with RAFT_PREC_FP32 (or raises).  Producers with bounded outputs need no flag:
 * InstanceNorm outputs (|x| <= sqrt(H*W)), the prepared images (|x| <= 1) and the GRU
 * epilogues (sigmoid / tanh blends of |h| <= 1); neither do convs whose outputs only feed
 * fp32 consumers (the raw convs of an InstanceNorm encoder, the flow head's first conv). */
#define RAFT_RANGE_LIMIT 32768.0f

/* InstanceNorm statistics from the conv epilogue (core/extractor.py norm_fn='instance': the
 * raw conv output's per-(image, channel) mean and variance without a pass over it).  With
 * p->stats_part set, every wave of the conv writes, per output channel n, the (count, mean, M2)
 * of its <= 32 output pixels (M2 = sum of squared deviations from that mean) as 4 floats at
 * stats_part[((slot * stats_ld) + n) * 4 ..], slot = image * slots_per_image + s, s <
 * slots_per_image; raft_instnorm_merge combines them (Chan's formula in double, fixed order).
 * Only for convs with the linear epilogue (alpha 1, no add0) and more than 4 outputs (VEC) that run
 * on the halo, stem or (since round 5: the strided encoder convs) 64x64-tile GEMM kernel, whose
 * tiles then hold one image's rows each: raft_conv2d_stats_slots returns slots_per_image for such a
 * conv and 0 otherwise (raft_conv2d then rejects stats_part).
 *
 * Slot footprints (s = the slot within image b; y, x output coordinates, out_h x out_w per image):
 *   halo  spatial tiles of TH = raft_conv2d_halo_tile_rows (8 or 16) rows x 16 columns, row-major:
 *         tile t = (y / TH) * ceil(out_w / 16) + x / 16; slots_per_image = 4 * tiles; s = 4 t + w, wave w
 *         holding tile rows (TH / 4) w .. (TH / 4)(w + 1) - 1 (two image rows x 16 columns per 32-pixel
 *         block; at TH = 16 a wave's two blocks are combined by Chan's formula in fp32 before the write);
 *   stem  the same with TH = 8 (tiles of 8 rows x 16 columns, s = 4 t + w, wave w rows 2w, 2w + 1);
 *   GEMM  the image's out_h * out_w pixels in row-major order, 64 per tile (the last tile ragged):
 *         slots_per_image = 2 * ceil(out_h * out_w / 64); s = 2 * tile + half, half h holding pixels
 *         64 * tile + 32 h .. + 31.
 * Every slot of every image is written for every n < N: the pixels of a footprint that lie outside the
 * image are not counted, and a slot without a pixel holds (0, 0, 0).  The fourth float of an entry is
 * written too (its value is unspecified); nothing else of stats_part is touched, columns
 * N .. stats_ld - 1 in particular. */
int raft_conv2d_stats_slots(const raft_conv2d_params* p);
/* Tile rows of the halo kernel's launch of this conv: 8 (128-pixel tiles), 16 (the multi-round
 * 256-pixel tiles), 0 when the halo kernel does not run it (inspection / tests). */
int raft_conv2d_halo_tile_rows(const raft_conv2d_params* p);
/* Tiles each work-group of the halo kernel's launch of this conv runs back to back (1, or
 * ceil(tiles / CUs) for a launch of more tiles than CUs: the loaders run on into the next tile while
 * the compute waves store the last one), 0 when the halo kernel does not run it (inspection / tests). */
int raft_conv2d_halo_tiles_per_wg(const raft_conv2d_params* p);
/* The kernel form raft_conv2d launches for a conv (inspection / tests; since ABI 19).  The query runs
 * the launch's own decision code up to the point of the launch and records the instantiation it
 * would start instead of starting it: nothing is launched and no operand is dereferenced (the
 * pointers only have to pass raft_conv2d's argument checks), so it runs without a device (the tile
 * rules then assume 256 CUs).  Fields a kernel does not have are 0. */
#define RAFT_CONV_KERNEL_HALO 1       /* conv_halo: stride-1 "same" 1x1 / 3x3 / 1x5 / 5x1, split precisions */
#define RAFT_CONV_KERNEL_GEMM 2       /* conv_gemm: 64 x 64 implicit-GEMM tiles (everything else) */
#define RAFT_CONV_KERNEL_STEM 3       /* conv_stem: the encoders' 7x7 / stride-2 stem */
#define RAFT_CONV_KERNEL_SMALLN 4     /* N <= 4 on the VALU, any geometry */
#define RAFT_CONV_KERNEL_SMALLN3X3 5  /* N <= 2 stride-1 3x3 on the VALU (LDS row tiles) */
struct raft_conv2d_form {     /* (no typedef: the query below has the same name; say `struct raft_conv2d_form`) */
  int kernel;                  /* RAFT_CONV_KERNEL_* */
  int tile_rows;               /* halo: image rows of a spatial tile, 8 or 16 */
  int tile_cols;               /* halo: output channels of a tile, 32 / 64 / 128 */
  int tiles_per_wg;            /* halo: spatial tiles a work-group runs back to back */
  int loader_waves;            /* halo: 4 or 8 */
  int compute_waves_per_simd;  /* halo: 1, or 2 for the K-split form (raft_conv2d_set_halo_ks) */
  int gemm_k_groups;           /* gemm: 1 or 2 K-groups per tile */
  int smalln_tile_rows;        /* smalln3x3: 2 or 4 image rows per tile */
};
/* 0 and *out filled, or raft_conv2d's argument error for these params (out untouched). */
int raft_conv2d_form(const raft_conv2d_params* p, struct raft_conv2d_form* out);
/* The same for raft_conv2d_pair(p0, p1): *one_launch = 1 when the two share one halo launch (out[0]
 * and out[1] then describe that launch), 0 when they run in order (each as raft_conv2d_form). */
int raft_conv2d_pair_form(const raft_conv2d_params* p0, const raft_conv2d_params* p1,
                          struct raft_conv2d_form out[2], int* one_launch);
/* 1 when the conv can apply its input's InstanceNorm in its loaders (in_norm above: the halo
 * kernel's 3x3 convs over <= 256 channels), else 0. */
int raft_conv2d_in_norm_ok(const raft_conv2d_params* p);
/* The merges: stats[(b * C + c) * 2 + {0, 1}] = {mean, 1 / sqrt(M2 / count + eps)} of the pooled
 * partials part[((b * slots_per_image + s) * stats_ld + c) * 4 + {0, 1, 2}] = (count, mean, M2), s <
 * slots_per_image, c < C <= stats_ld (columns C .. stats_ld - 1 are not read).  A slot with count 0 is
 * skipped; it must hold finite mean and M2 (the convs write zeros).  Precondition of all three: slot 0
 * of every image holds pixels (count > 0), as every conv above guarantees (slot 0 covers pixel (0, 0));
 * raft_instnorm_merge_ws / _fused centre their sums on slot 0's mean.
 * raft_instnorm_merge: Chan's formula in double, fixed order (deterministic). */
int raft_instnorm_merge(const float* part, int slots_per_image, int B, int C, int stats_ld, float eps,
                        float* stats, raft_stream_t stream);
/* raft_instnorm_merge over many slots, spread over the CUs: level 1 sums groups of 64 slots per
 * channel relative to K = slot 0's mean (coalesced 1-KiB slot rows, no division): n = sum c_i,
 * s1 = sum c_i (m_i - K), s2 = sum M2_i + c_i (m_i - K)^2, in double; level 2 combines the groups in
 * order (deterministic, wave w of 16 the groups w, w + 16, ... in batches of 8): mean = K + s1 / n,
 * M2 = max(s2 - s1 * s1 / n, 0).  ws: raft_instnorm_merge_ws_floats(slots_per_image, B, C) floats,
 * 8-byte aligned; the same {mean, rstd} as raft_instnorm_merge to double rounding (of sums whose
 * size grows with the distance of K from the pooled mean). */
size_t raft_instnorm_merge_ws_floats(int slots_per_image, int B, int C);
int raft_instnorm_merge_ws(const float* part, int slots_per_image, int B, int C, int stats_ld, float eps, void* ws,
                           float* stats, raft_stream_t stream);
/* raft_instnorm_merge_ws as ONE launch: the level-1 block of a (64-channel group, image) whose
 * group sums land last (an agent-scope counter per group and image) runs level 2, in level 2's
 * order: the same statistics bit for bit, one kernel boundary fewer.  counters:
 * raft_instnorm_merge_counters(B, C) ints, zero before the first call; every call leaves them zero
 * (so a captured graph replays).  ws as raft_instnorm_merge_ws. */
size_t raft_instnorm_merge_counters(int B, int C);
int raft_instnorm_merge_fused(const float* part, int slots_per_image, int B, int C, int stats_ld, float eps, void* ws,
                              int* counters, float* stats, raft_stream_t stream);

/* Packed weight geometry for a conv (n_pad, k_pad in floats per row). */
int raft_conv2d_packed_shape(int mode, int n, int kh, int kw, int cin, int* n_pad, int* k_pad);
int raft_conv2d(const raft_conv2d_params* p, raft_stream_t stream);
/* Two convs with no data dependence between them (core/update.py:276-285: convc2 of the corr
 * branch beside convf2 of the flow branch), results identical to raft_conv2d(p0) then
 * raft_conv2d(p1).  When both are halo-kernel convs of one shape class and precision, their
 * tiles run side by side in ONE launch: the pair fills CUs that either alone leaves idle at
 * one frame pair, with no second stream (a cross-stream fork/join costs a graph ~7 us per
 * edge on ROCm).  Each conv keeps the tile rows raft_conv2d would pick for it
 * (raft_conv2d_halo_tile_rows), so the bits match also with weight_s set; convs that pick
 * different rows are not co-launched.  Otherwise, or when one reads what the other writes, or both write a common
 * element (column ranges of their output rows meet), the two run in order. */
int raft_conv2d_pair(const raft_conv2d_params* p0, const raft_conv2d_params* p1, raft_stream_t stream);
/* Loader waves of the halo kernel's one-tile f16x3 3x3 / 1x5 / 5x1 convs (the update block at one frame
 * pair): 4 (a 512-thread work-group) or 8 (768 threads: each loader issues half the weight DMAs
 * and stages half of each patch); the same results bit for bit.  Default 8 (RAFT_HALO_NL8=0: 4).
 * Returns the previous count; other values only query.  Process-wide; plans capture launches, so
 * set it before building / capturing a plan. */
int raft_conv2d_set_halo_loaders(int nl);
/* The compute waves per SIMD of the same convs when their N tile is 64 columns: 2 (default; the K-split form:
 * waves w and w + 4 take the even / odd K-steps of one 32 x 64 block, their partial sums meet in LDS and each
 * stores half the columns; 4 loader waves, 768 threads) or 1.  The two forms sum the K-steps in different orders
 * (results within fp32 rounding of each other; each deterministic).  Returns the previous count; other values
 * only query.  Process-wide; set it before building / capturing a plan.  (Engine-level knob; no reference
 * counterpart.) */
int raft_conv2d_set_halo_ks(int ks);
/* fp32 packed weight [n_pad][k_pad] -> split form for RAFT_PREC_F16X3 / F16:
 * per row and 32-wide K-step, 32 f16 hi then 32 f16 lo (lo scaled by 2048);
 * out holds n_pad*k_pad*4 bytes, like the input. */
int raft_conv2d_split_weight(const float* w, void* out, int n_pad, int k_pad, raft_stream_t stream);
/* Column-scaled f16x3 split (raft_conv2d_params.weight_s): per output row n a power of two
 * S_n = 2^(14 - e_n), e_n = the binary exponent of max_k |w[n][k]| (so |w * S_n| < 2^14; S_n = 1 for
 * a zero row), then per K-step 32 f16 hi = f16(w S_n) and 32 f16 lo = f16(w S_n - hi), both at
 * the scale S_n, followed by the n_pad floats 1 / S_n.  hi*hi + hi*lo + lo*hi then sum in one
 * fp32 chain and the epilogue multiplies by 1 / S_n (exact).  out holds
 * raft_conv2d_split_scaled_bytes(n_pad, k_pad) bytes, 16-byte aligned. */
size_t raft_conv2d_split_scaled_bytes(int n_pad, int k_pad);
int raft_conv2d_split_weight_scaled(const float* w, void* out, int n_pad, int k_pad, raft_stream_t stream);
/* The split form for a given precision: RAFT_PREC_F16X3 / RAFT_PREC_F16 as above;
 * RAFT_PREC_BF16: per row and K-step 32 bf16 hi = bf16(x) then 32 bf16 lo = bf16(x - hi). */
int raft_conv2d_split_weight_prec(const float* w, void* out, int n_pad, int k_pad, int precision,
                                  raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * InstanceNorm2d (affine=False, eps): statistics per (image, channel) over
 * the image's hw pixels; stats[(b*C + c)*2 + {0,1}] = {mean, 1/sqrt(var+eps)}.
 * --------------------------------------------------------------------------- */
size_t raft_instnorm_workspace_floats(int B, int HW, int C);
int raft_instnorm_stats(const float* x, int ld, int B, int HW, int C, float eps, float* stats,
                        float* workspace, raft_stream_t stream);
/* out = act( norm(x) + resid ) where resid = 0 (resid NULL), raw resid rows, or
 * norm(resid) with its own stats (resid_stats != NULL); relu_mode: 0 none, 1 relu(norm(x)),
 * 2 relu(resid + relu(norm(x)))  (ResidualBlock tail). */
/* nn.GroupNorm (core/extractor.py:23-25: ResidualBlock / BottleneckBlock with norm_fn='group', the
 * blocks' default): per (image, group of C/G consecutive channels) mean and 1/sqrt(var + eps) over the
 * group's channels x HW pixels (double, deterministic), written per (image, channel) as
 * stats[b][c] = {mean, rstd} of c's group — the layout raft_instnorm_apply reads.  C % G == 0. */
int raft_groupnorm_stats(const float* x, int ld, int B, int HW, int C, int G, float eps, float* stats,
                         raft_stream_t stream);
/* raft_instnorm_apply with a per-channel affine: v = (x - mean) * rstd * gamma[c] + beta[c]
 * (gamma / beta NULL = 1 / 0); the residual likewise with resid_gamma / resid_beta. */
int raft_norm_apply_affine(const float* x, int ld, const float* stats, const float* gamma, const float* beta,
                           const float* resid, int resid_ld, const float* resid_stats, const float* resid_gamma,
                           const float* resid_beta, int relu_mode, float* out, int out_ld, int B, int HW, int C,
                           raft_stream_t stream);
int raft_instnorm_apply(const float* x, int ld, const float* stats, const float* resid, int resid_ld,
                        const float* resid_stats, int relu_mode, float* out, int out_ld,
                        int B, int HW, int C, raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * Small elementwise / layout kernels of RAFT.forward
 * --------------------------------------------------------------------------- */
/* images NCHW [B][3][H][W] in 0..255 -> NHWC rows [2B*H*W][3]: img1 batch then img2, 2*(x/255)-1 */
int raft_prep_images(const float* img1, const float* img2, float* out, int B, int H, int W,
                     raft_stream_t stream);
/* coords NHWC [B*H*W][2] = coords_grid (+ flow_init NCHW [B][2][H][W] if not NULL) */
int raft_init_coords(float* coords, const float* flow_init, int B, int H, int W, raft_stream_t stream);
/* flow_low NCHW [B][2][H][W] = coords - coords_grid */
int raft_flow_from_coords(const float* coords, float* flow, int B, int H, int W, raft_stream_t stream);
/* convex upsample of flow = coords - grid with mask rows [B*H*W][mask_ld] (576 used)
 * -> NCHW [B][2][8H][8W] */
int raft_convex_upsample(const float* coords, const float* mask, int mask_ld, float* flow_up,
                         int B, int H, int W, raft_stream_t stream);
/* 8 * bilinear(align_corners=True) x8 upsample of flow = coords - grid -> NCHW [B][2][8H][8W] */
int raft_upflow8(const float* coords, float* flow_up, int B, int H, int W, raft_stream_t stream);
/* NCHW [B][C][H][W] <-> NHWC rows [B*H*W][ld] */
int raft_nchw_to_nhwc(const float* in, float* out, int out_ld, int B, int C, int H, int W, raft_stream_t stream);
int raft_nhwc_to_nchw(const float* in, int in_ld, float* out, int B, int C, int H, int W, raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * Caller-side helpers (demo.py / evaluate.py around RAFT.forward), NCHW fp32
 * --------------------------------------------------------------------------- */
/* replicate padding: in [NC][H][W] -> out [NC][H+top+bottom][W+left+right] */
int raft_pad_replicate(const float* in, float* out, int NC, int H, int W, int top, int bottom, int left, int right,
                       raft_stream_t stream);
/* bilinear_sampler: img [N][C][H][W], coords [N][Ho][Wo][2] pixel (x, y) -> out [N][C][Ho][Wo]
 * (grid_sample, align_corners=True, zero padding; a non-finite position gives NaN, as the
 * reference on a 1-px axis); mask (optional) [N][Ho][Wo] = 1 where -1 < grid < 1 on both axes. */
int raft_bilinear_sample(const float* img, const float* coords, float* out, float* mask, int N, int C, int H, int W,
                         int Ho, int Wo, raft_stream_t stream);
/* forward_interpolate: flow [B][2][H][W] -> out [B][2][H][W]; every grid point takes the flow of
 * the nearest (fp64 Euclidean) forward-moved point (x + dx, y + dy) strictly inside
 * (0, W) x (0, H); ties -> the lowest source index; no valid point -> 0.  An all-pairs search,
 * for the 1/8-resolution flow of the warm start: H*W <= RAFT_FI_MAX_POINTS (else RAFT_E_INVALID). */
#define RAFT_FI_MAX_POINTS 65536
int raft_forward_interpolate(const float* flow, float* out, int B, int H, int W, raft_stream_t stream);


/* ---------------------------------------------------------------------------
 * Video streams (StreamPlan / RAFT.stream): every frame is encoded once.
 * Additive entries: they change no existing entry, so RAFT_HIP_ABI_VERSION stays 19.
 * --------------------------------------------------------------------------- */
/* InputPadder's rule (core/utils/utils.py:9-16): the replicate padding that makes H and W multiples
 * of 8, centred (the reference's 'sintel' mode) or with every padding row at the bottom (any other
 * mode); columns are centred in both.  Host arithmetic only; NULL outputs are skipped. */
void raft_frame_pad(int H, int W, int centred, int* left, int* right, int* top, int* bottom);
/* dtype tags of raft_ingest_frame's input */
#define RAFT_FRAME_F32_NCHW 0 /* float32 [B][3][H][W], 0..255: what RAFT.forward takes */
#define RAFT_FRAME_U8_NHWC 1  /* uint8 [B][H][W][3]: what a video decoder delivers */
/* One frame of any size, in one launch: replicate-padded by raft_frame_pad's rule to Hp x Wp, written as
 * (a) rows   NHWC rows [B*Hp*Wp][3] of 2 * (v / 255) - 1, the expression of raft_prep_images (bit-equal
 *            to InputPadder.pad + raft_prep_images), and
 * (b) padded the raw padded frame, float32 NCHW [B][3][Hp][Wp] (what the range guard's exact re-run reads).
 * in, rows and padded are three distinct buffers. */
int raft_ingest_frame(const void* in, int dtype, int B, int H, int W, int centred, float* rows, float* padded,
                      raft_stream_t stream);
/* A stream's current frame becomes its previous frame: three device copies (feature map, prepped
 * rows, raw padded frame; element counts in floats) in one launch.  No pair may be in place. */
int raft_stream_carry(const float* fmap_cur, float* fmap_prev, size_t n_fmap, const float* rows_cur, float* rows_prev,
                      size_t n_rows, const float* raw_cur, float* raw_prev, size_t n_raw, raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * Bidirectional video streams (BidiStreamPlan / RAFT.stream(bidirectional=True)) and the
 * forward-backward consistency check.  Additive entries: RAFT_HIP_ABI_VERSION stays 19.
 * --------------------------------------------------------------------------- */
/* The n-copy form of raft_stream_carry: up to RAFT_CARRY_MAX_SEGS pitched 2-D device copies in one
 * launch (rows x cols floats each, row pitches src_ld / dst_ld >= cols; a flat copy is rows = 1).
 * 16-byte accesses where every segment's pointers, cols and pitches allow them.  No segment may
 * be in place; the segments must not overlap each other.  The segment array is read on the host. */
#define RAFT_CARRY_MAX_SEGS 8
typedef struct raft_copy2d {
  const float* src;
  long src_ld;
  float* dst;
  long dst_ld;
  long rows, cols;
} raft_copy2d;
int raft_stream_carry_n(const raft_copy2d* segs, int n, raft_stream_t stream);

/* Forward-backward consistency (the UnFlow criterion, Meister et al. 2018, published defaults
 * alpha = 0.01, beta = 0.5), both directions and all B images in one launch.
 *
 * Definition.  For direction fw at pixel x = (j, i) of the H x W frame, F = flow_fw, G = flow_bw
 * (channel 0 = x displacement, channel 1 = y displacement, in pixels):
 *   p = x + F(x)                                   the pixel's target in the other frame
 *   p not finite, or outside [0, W-1] x [0, H-1]:  err = +inf, occ = 1 (the pixel left the frame)
 *   otherwise:  g   = bilinear sample of G at p; corners at floor(p) and floor(p) + 1; a +1 corner
 *                     that falls outside the frame has weight 0 and is not read
 *               err = |F(x) + g|^2
 *               occ = err > alpha * (|F(x)|^2 + |g|^2) + beta
 * and occ = 1 wherever err is not finite (a NaN or inf of G reached it).  Direction bw is the same
 * with F and G swapped.  (Sign convention: the sample is taken at x + F(x), where the pixel goes.)
 * The sampling position is taken as floor(j + Fx) = j + floor(Fx) with weight Fx - floor(Fx) (exact in
 * fp32 but for one rounding of <= 2^-25 where -1 < Fx < 0; j + Fx itself is never rounded); the
 * blend, err and the threshold round once per operation (no contraction).
 *
 * Layout.  A flow is float32 NCHW with unit element stride: element (b, c, y, x) of the FRAME is
 * at flow[b * batch_stride + c * chan_stride + (top + y) * pitch + left + x] (strides in floats):
 * a crop at (top, left) of a larger, pitched buffer, e.g. the stream's padded [2B][2][Hp][Wp]
 * flow_up in place; a plain tensor is top = left = 0, pitch = W.  A target in the buffer's
 * padding is outside the frame.  occ_* are uint8 [B][H][W] (0 / 1), err_* float32 [B][H][W],
 * dense; err_* 16-byte and occ_* 4-byte aligned.  B * H * W < 2^30. */
int raft_fb_consistency(const float* flow_fw, long fw_batch_stride, long fw_chan_stride, long fw_pitch,
                        const float* flow_bw, long bw_batch_stride, long bw_chan_stride, long bw_pitch, int top,
                        int left, int B, int H, int W, float alpha, float beta, unsigned char* occ_fw,
                        unsigned char* occ_bw, float* err_fw, float* err_bw, raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * Flow colour-wheel visualisation (core/utils/flow_viz.py on the device; utils.flow_viz,
 * RAFT.stream(visualize=...)).  Additive entries: RAFT_HIP_ABI_VERSION stays 19.
 * --------------------------------------------------------------------------- */
/* A flow field as a colour image: hue = direction, saturation = magnitude (the Middlebury coding of
 * Baker et al., "A Database and Evaluation Methodology for Optical Flow", ICCV 2007).
 *
 * Definition.  (u, v) = channels 0 and 1 of the flow at a pixel of image b; arithmetic is fp32 and
 * every written operation rounds once (no contraction), division and sqrt correctly rounded.
 *   clip     with RAFT_VIZ_CLIP: u = min(max(u, 0), clip_flow), v likewise, before everything else
 *            (a NaN stays a NaN; +inf becomes clip_flow, -inf becomes 0).  The LOWER bound 0 is the
 *            reference's (np.clip(flow_uv, 0, clip_flow)): it removes every negative component.
 *            It is kept for parity.
 *   black    u or v not finite (after the clip): the pixel is (0, 0, 0) and takes no part in the
 *            maximum.  (The reference casts a NaN to uint8 there, which is undefined: this rule is
 *            this library's own.)
 *   rad_max  per image b: the maximum of sqrt(u*u + v*v) over the image's pixels that are not black;
 *            0 if there are none.  fixed_rad_max > 0 replaces it for all images (one scale for a
 *            whole video: colours do not flicker with each frame's own maximum).  (A finite flow
 *            whose square overflows fp32 gives rad_max = +inf: every u' and v' is 0, a white image.)
 *   scale    u' = u / (rad_max + 1e-5f), v' = v / (rad_max + 1e-5f).  With RAFT_VIZ_UNIT: u' = u,
 *            v' = v (flow_uv_to_colors: no maximum, no epsilon; fixed_rad_max is not read).
 *   wheel    rad = sqrt(u'*u' + v'*v'),  a = atan2(-v', -u') / pi,  fk = (a + 1) / 2 * 54,
 *            k0 = floor(fk) clamped to [0, 54],  k1 = (k0 + 1) mod 55,  f = fk - k0;
 *            per channel c:  col = (1 - f) * (wheel[k0][c] / 255) + f * (wheel[k1][c] / 255),
 *            col = rad <= 1 ? 1 - rad * (1 - col) : 0.75 * col,  byte = floor(255 * col).
 *   wheel[55][3]: six segments of n = 15, 6, 4, 11, 13, 6 entries through red, yellow, green, cyan,
 *            blue, magenta and back to red.  Entry i of a segment is the segment's first colour with
 *            one channel moved by t = floor(255 * i / n): G = t (red-yellow), R = 255 - t
 *            (yellow-green), B = t (green-cyan), G = 255 - t (cyan-blue), R = t (blue-magenta),
 *            B = 255 - t (magenta-red).
 * Stacking (demo.py's np.concatenate([img, flo], axis=0)).  With frame != NULL the output has 2H rows
 * per image: rows 0..H-1 are the frame (float32 NCHW, 3 channels, 0..255, the crop offsets of the
 * flow and strides of its own): each value rounded to nearest (ties to even), saturated to 0..255,
 * NaN -> 0, so an integer-valued frame passes through exactly; rows H..2H-1 are the colours.
 *
 * Layout.  The flow is raft_fb_consistency's: float32 NCHW with unit element stride, element
 * (b, c, y, x) at flow[b * batch_stride + c * chan_stride + (top + y) * pitch + left + x] (strides
 * in floats), so the stream's padded [B][2][Hp][Wp] flow_up is read in place; a plain tensor is
 * top = left = 0, pitch = W.  Nothing outside the crop is read.  out is uint8 [B][H][W][3] (or
 * [B][2H][W][3]), dense, 4-byte aligned, channel order R, G, B, or B, G, R with RAFT_VIZ_BGR (frame
 * rows included).  out may not alias flow, frame or ws.  B * H * W < 2^30.
 *
 * Launches.  Without a fixed scale: one launch writes each work-group's maximum to ws
 * (raft_flow_viz_ws_bytes(B, H, W) bytes, 4-byte aligned; every float of it is written before it is
 * read, so it needs no initialisation), and the colour launch's work-groups reduce their images'
 * partial maxima before colouring.  No atomics, no buffer zeroed between calls: a captured call
 * replays to identical bytes.  With fixed_rad_max > 0 or RAFT_VIZ_UNIT only the colour launch runs
 * and ws may be NULL. */
#define RAFT_VIZ_BGR 1  /* bytes in B, G, R order */
#define RAFT_VIZ_UNIT 2 /* no normalisation (u' = u, v' = v) */
#define RAFT_VIZ_CLIP 4 /* clip both components to [0, clip_flow] first */
/* bytes of raft_flow_to_rgb's workspace; 0 for sizes it rejects */
size_t raft_flow_viz_ws_bytes(int B, int H, int W);
int raft_flow_to_rgb(const float* flow, long batch_stride, long chan_stride, long pitch, int top, int left, int B,
                     int H, int W, float clip_flow, float fixed_rad_max, int flags, const float* frame,
                     long frame_batch_stride, long frame_chan_stride, long frame_pitch, float* ws,
                     unsigned char* out, raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * Warping by a flow field (utils.warp_frame, utils.splat_density, RAFT.stream(warp=...)).
 * Additive entries: RAFT_HIP_ABI_VERSION stays 19.
 * --------------------------------------------------------------------------- */
/* Backward warp: out(x) = bilinear sample of the frame at x + flow(x), all B images and C channels in one
 * launch, and valid(x) = whether that position lies in the frame.  With flow = the flow from frame 1 to
 * frame 2 and frame = frame 2, out is frame 2 pulled back onto frame 1.
 *
 * Definition.  At pixel (j, i) of the H x W frame the displacement is d = (dx, dy) = flow(j, i) (channel
 * 0 = x, channel 1 = y, in pixels).
 *   axes      each axis as raft_fb_consistency takes it: fl = floor(d), t = d - fl, i0 = j + (int)fl
 *             (x: base x0, weight ax; y: base y0, weight ay).  t is exact in fp32 but for one rounding of
 *             <= 2^-25 where -1 < d < 0; the sum j + d is never formed.
 *   rejected  dx or dy not finite, or |d| >= 2^30 on either axis: every channel of out is 0 and
 *             valid = 0, in both modes.
 *   valid     1 iff the position lies in [0, W-1] x [0, H-1]: per axis i0 >= 0 and (i0 < n-1, or
 *             i0 == n-1 with t == 0) -- the `inside` of raft_fb_consistency.  The same in both modes.
 *   zeros     (the default) the taps are (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1); a tap outside
 *             the H x W crop contributes 0 and is not read.  A position in (-1, 0) or (n-1, n) still
 *             blends its inside taps with their weights, as grid_sample(padding_mode='zeros',
 *             align_corners=True) does.
 *   border    (RAFT_WARP_BORDER) per axis, before the taps are taken: i0 < 0 gives i0 = 0, t = 0;
 *             i0 >= n-1 gives i0 = n-1, t = 0 (grid_sample's padding_mode='border').  The +1 tap of a
 *             clamped axis has weight 0; outside the crop it is not read.
 *   blend     wx0 = 1 - ax, wy0 = 1 - ay,
 *             out = wy0 * (wx0 * v00 + ax * v01) + ay * (wx0 * v10 + ax * v11),
 *             every written operation rounded once (no contraction): raft_fb_consistency's order, so
 *             |out_fp32 - out_exact| <= 10 * 2^-24 * max |tap|.
 *   uint8     uint8 taps are widened to float first.  A uint8 output is the blend rounded to nearest
 *             (ties to even) and saturated to 0..255 (NaN -> 0).
 *
 * Layout.  The flow is raft_fb_consistency's: float32 NCHW with unit element stride, element (b, c, y, x)
 * of the frame at flow[b * batch_stride + c * chan_stride + (top + y) * pitch + left + x] (strides in
 * floats), so a padded flow_up is read in place.  The frame is, by its dtype tag, either
 * RAFT_FRAME_F32_NCHW: float32 with strides of its own and THE SAME crop offsets (top, left), any C >= 1,
 * or RAFT_FRAME_U8_NHWC: uint8 [B][H][W][3], dense (strides and crop offsets are not read; C == 3).
 * out is, by out_dtype, float32 [B][C][H][W] dense, 16-byte aligned, or uint8 [B][H][W][3] dense,
 * 4-byte aligned (C == 3); all four combinations are supported.  valid is uint8 [B][H][W] (0 / 1),
 * 4-byte aligned.  Nothing outside the crop is read.  out and valid alias neither each other nor an
 * input.  B * H * W < 2^30. */
#define RAFT_WARP_BORDER 1 /* clamp the sampling position to the frame (default: taps outside read 0) */
int raft_warp_frame(const float* flow, long flow_batch_stride, long flow_chan_stride, long flow_pitch,
                    const void* frame, int frame_dtype, long frame_batch_stride, long frame_chan_stride,
                    long frame_pitch, int top, int left, int B, int C, int H, int W, int flags, void* out,
                    int out_dtype, unsigned char* valid, raft_stream_t stream);

/* Forward-warp density (UnFlow's forward_warp, Meister et al. 2018): how much of frame 1 lands on each
 * pixel of frame 2 under the flow.  ~1 where the flow is a bijection, < 1 where nothing arrives (a
 * disocclusion), > 1 where several sources pile up.
 *
 * Definition.  Source pixel (j, i) with d = flow(j, i), x0 / ax / y0 / ay as in raft_warp_frame,
 * contributes iff dx and dy are finite, |d| < 2^30 on both axes, 0 <= x0 <= W-1 and 0 <= y0 <= H-1.
 * With x1 = min(x0 + 1, W-1), y1 = min(y0 + 1, H-1), wx0 = 1 - ax, wy0 = 1 - ay it adds
 *   wx0 * wy0 to (y0, x0),  ax * wy0 to (y0, x1),  wx0 * ay to (y1, x0),  ax * ay to (y1, x1)
 * (on the last column / row both weights of the axis land on the edge pixel), each weight computed in
 * fp32 with one rounding per operation.  density is the SUM of all contributions to a pixel.
 *
 * Accumulation.  Each weight w is quantised to unsigned 64-bit fixed point with unit 2^-32 by truncation
 * (w * 2^32 is exact in fp32) and added with 64-bit integer atomics; a last pass converts every pixel's
 * sum to float32 with one rounding.  Integer addition is associative: the result does not depend on the
 * order the adds arrive in and is bitwise equal from run to run.  Three launches: zero, splat, convert.
 * |density_fp32 - density_exact| <= n * (3 * 2^-24 + 2^-32) + 2^-24 * density for n contributing taps.
 *
 * Layout.  The flow as above.  ws: raft_splat_ws_bytes(B, H, W) bytes, 8-byte aligned (zeroed by the
 * call itself); density float32 [B][H][W] dense.  density, ws and flow are distinct.  B * H * W < 2^30. */
/* bytes of raft_splat_density's workspace; 0 for sizes it rejects */
size_t raft_splat_ws_bytes(int B, int H, int W);
int raft_splat_density(const float* flow, long batch_stride, long chan_stride, long pitch, int top, int left, int B,
                       int H, int W, void* ws, float* density, raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * Resizing frames and flows (utils.resize_frame, utils.resize_flow, utils.InputScaler):
 * torch.nn.functional.interpolate's bilinear and area modes with exact integer coordinates.
 * An additive entry: RAFT_HIP_ABI_VERSION stays 19.
 * --------------------------------------------------------------------------- */
/* dst = the Hs x Ws source resized to Hd x Wd, all B images and C channels in one launch.
 *
 * Definition.  Per axis, output index d of D samples over S source samples:
 *   coordinate  align_corners off: n = max((2 d + 1) S - D, 0), den = 2 D   (the position
 *               S / D * (d + 0.5) - 0.5, clamped at 0, as the exact ratio n / den);
 *               align_corners on:  n = d (S - 1), den = max(D - 1, 1).
 *               i0 = min(n / den, S - 1) (integer division), i1 = min(i0 + 1, S - 1),
 *               lam = float(n % den) / float(den): both conversions are exact for D <= 2^23 and the
 *               division is correctly rounded, so lam carries one rounding and no fp32 coordinate is ever
 *               formed.  The integers are 64-bit wherever (2 d + 1) S can pass 2^31.
 *               (x: taps x0, x1, weight lx; y: taps y0, y1, weight ly.)
 *   bilinear    out = (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11)
 *               in IEEE fp32, every written operation rounded to nearest once and nothing fused.  All four
 *               taps are always read and blended: a NaN or Inf under a weight of 0 reaches the output, as
 *               the formula says and as torch computes it.  With T = max |tap| and u = 2^-24, eight
 *               roundings lie on the path of one output -- lx, 1 - lx, a product and the sum of the
 *               horizontal blend (the errors of its two products are weighted by 1 - lx and lx and count
 *               as one; the two horizontal blends are weighted by 1 - ly and ly likewise), then ly, 1 - ly,
 *               a product and the sum of the vertical one: |out_fp32 - out_exact| <= ((1 + 4 u)^2 - 1) T,
 *               8 u T to first order.
 *   area        (RAFT_RESIZE_AREA: torch's mode="area", adaptive average pooling) out = the mean over
 *               source rows floor(i Hs / Hd) .. ceil((i + 1) Hs / Hd) - 1 and the columns likewise: a
 *               sequential fp32 sum in row-major order over the box, starting from 0, then one division
 *               by the count (converted to fp32: exact below 2^24).  For a box of n samples
 *               |out_fp32 - out_exact| <= (n + 1) u T to first order.
 *   multipliers channel 0 is multiplied by mul0 and channel 1 by mul1 after the interpolation (one more
 *               rounding each); the other channels are not.  A flow resized from Hs x Ws to Hd x Wd passes
 *               mul0 = Wd / Ws and mul1 = Hd / Hs, each rounded to fp32 once on the host, so the vectors
 *               stay in pixels of the new size; a plain frame passes 1.0 (exact).
 *   uint8       uint8 taps are widened to float first.  A uint8 output is the value rounded to nearest
 *               (ties to even) and saturated to 0..255 (NaN -> 0), as raft_warp_frame's is.
 *
 * Layout.  The source is, by src_dtype, RAFT_FRAME_F32_NCHW: float32, any C >= 1, unit element stride,
 * element (b, c, y, x) at src[b * batch_stride + c * chan_stride + (top + y) * pitch + left + x] (strides
 * in floats: a padded flow_up or an unpad view is read in place), or RAFT_FRAME_U8_NHWC: uint8
 * [B][Hs][Ws][3], dense (strides and crop offsets are not read; C == 3).  dst is, by dst_dtype, float32
 * [B][C][Hd][Wd] dense, or uint8 [B][Hd][Wd][3] dense (C == 3); all four combinations are supported.
 * float32 pointers are 4-byte aligned; 16-byte (float32) and 4-byte (uint8) stores are used where the
 * address allows.  Nothing outside the crop is read.  dst does not alias src.  B * C * Hs * Ws < 2^30 and
 * B * C * Hd * Wd < 2^30.  Argument errors are reported before any launch. */
#define RAFT_RESIZE_BILINEAR 0
#define RAFT_RESIZE_AREA 1
#define RAFT_RESIZE_ALIGN_CORNERS 1 /* flags bit 0: bilinear with align_corners (not with RAFT_RESIZE_AREA) */
int raft_resize(const void* src, int src_dtype, long src_batch_stride, long src_chan_stride, long src_pitch,
                int top, int left, int B, int C, int Hs, int Ws, void* dst, int dst_dtype, int Hd, int Wd, int mode,
                int flags, float mul0, float mul1, raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * Scoring a flow against ground truth (utils.flow_errors, utils.FlowMetrics): what evaluate.py's
 * validate_chairs / validate_sintel / validate_kitti compute on the host, on the device.
 * Additive entries: RAFT_HIP_ABI_VERSION stays 19.
 * --------------------------------------------------------------------------- */
/* Definition.  At a valid pixel with prediction (u, v) = flow and ground truth (gu, gv) = flow_gt, in IEEE
 * fp32 with every operation rounded to nearest and nothing fused:
 *   du = u - gu, dv = v - gv
 *   epe   = sqrt(du * du + dv * dv)          the end-point error: torch.sum((flow - flow_gt)**2, dim=0).sqrt()
 *   mag   = sqrt(gu * gu + gv * gv)
 *   ratio = epe / mag                         (mag == 0 gives inf or NaN; the comparisons below decide)
 * A pixel is valid when both hold:
 *   mask      valid == NULL, or the mask says so: RAFT_MASK_U8 (bool or uint8, one byte) != 0;
 *             RAFT_MASK_F32 >= 0.5f (validate_kitti's `valid_gt >= 0.5`); a NaN mask value fails.
 *   gt_limit  gt_limit <= 0 (absent), or |gu| < gt_limit and |gv| < gt_limit (core/datasets.py's
 *             `(flow.abs() < 1000)`); a NaN fails.
 * An invalid pixel counts nowhere.  A valid pixel whose epe is not finite counts in RAFT_FM_N and
 * RAFT_FM_N_NONFINITE only.  Every other valid pixel counts in
 *   RAFT_FM_N_LT1 / _LT3 / _LT5    epe < 1, epe < 3, epe < 5 (strict, as the reference's np.mean(epe < k))
 *   RAFT_FM_N_OUTLIER              epe > 3 && ratio > 0.05 (KITTI's Fl, the reference's comparisons verbatim)
 *   RAFT_FM_N_S0_10 / _S10_40 / _S40   Sintel's speed classes on mag: mag < 10; 10 <= mag < 40; mag >= 40
 *   RAFT_FM_EPE_SUM                the fp64 sum of the fp32 epe values, and per speed class
 *   RAFT_FM_EPE_SUM_S0_10 / _S10_40 / _S40.
 *
 * Record.  RAFT_FLOW_METRICS_SLOTS = 16 slots of 64 bits per sample: counts are int64, sums are fp64
 * stored by their bits.  `record` is [B][16]; `totals`, if given, is one record that the call ADDS every
 * sample's record into (zero it before the first call; calls accumulate in stream order), together with
 *   RAFT_FM_IMAGES           the number of samples with n > 0
 *   RAFT_FM_IMAGE_MEAN_SUM   the fp64 sum of epe_sum / n over those samples (validate_kitti reports the mean
 *                            of per-image means)
 * which are 0 in a sample's record, as is RAFT_FM_RESERVED (written as 0).
 *
 * Reproducibility.  Two launches: every work-group sums its pixels (threads in fp64 and integers, the
 * wave by a butterfly, the waves through LDS in order) and writes one partial record to ws; one work-group
 * adds the partials in index order, writes the records and adds them to the totals in sample order, in
 * one thread.  No atomics.  The grid depends on (H, W) only: min(ceil(H * W / RAFT_FLOW_METRICS_BLOCK_PIXELS),
 * RAFT_FLOW_METRICS_MAX_BLOCKS) work-groups per sample, never spanning two samples.  Two runs are bitwise
 * equal on any device, and a sample's record does not depend on its batch index or on the other samples.
 * Any other order of the same fp64 sum lies within n * 2^-53 * sum |epe| of it.
 *
 * Layout.  flow and flow_gt: float32 NCHW with unit element stride, element (b, c, y, x) at
 * p[b * batch_stride + c * chan_stride + y * pitch + x] (strides in floats, pitch >= W): a crop of a
 * padded flow_up (InputPadder.unpad's view) is read in place by passing the crop's first element.  valid:
 * [B][H][W] with a batch stride and a row pitch in elements, or NULL (then its tag and strides are not
 * read).  epe_map, if given: float32 [B][H][W] dense, the fp32 epe per pixel, NaN at invalid pixels (every
 * NaN written is the quiet NaN 0x7fc00000).  ws: raft_flow_metrics_ws_bytes(B, H, W) bytes, needs no
 * initialisation.  flow, flow_gt, a float32 mask and epe_map are 4-byte aligned, record, totals and ws
 * 8-byte.  No output aliases an input or another output.  B * H * W < 2^30. */
#define RAFT_FLOW_METRICS_SLOTS 16
#define RAFT_FLOW_METRICS_BLOCK_PIXELS 1024 /* pixels a work-group takes per pass */
#define RAFT_FLOW_METRICS_MAX_BLOCKS 256    /* work-groups per sample at most; larger samples wrap */
#define RAFT_FM_N 0
#define RAFT_FM_N_NONFINITE 1
#define RAFT_FM_N_LT1 2
#define RAFT_FM_N_LT3 3
#define RAFT_FM_N_LT5 4
#define RAFT_FM_N_OUTLIER 5
#define RAFT_FM_N_S0_10 6
#define RAFT_FM_N_S10_40 7
#define RAFT_FM_N_S40 8
#define RAFT_FM_EPE_SUM 9
#define RAFT_FM_EPE_SUM_S0_10 10
#define RAFT_FM_EPE_SUM_S10_40 11
#define RAFT_FM_EPE_SUM_S40 12
#define RAFT_FM_IMAGES 13
#define RAFT_FM_IMAGE_MEAN_SUM 14
#define RAFT_FM_RESERVED 15
#define RAFT_MASK_U8 0  /* bool or uint8: valid where != 0 */
#define RAFT_MASK_F32 1 /* float32: valid where >= 0.5 */
/* bytes of raft_flow_metrics' workspace; 0 for sizes it rejects */
size_t raft_flow_metrics_ws_bytes(int B, int H, int W);
int raft_flow_metrics(const float* flow, long flow_batch_stride, long flow_chan_stride, long flow_pitch,
                      const float* flow_gt, long gt_batch_stride, long gt_chan_stride, long gt_pitch,
                      const void* valid, int valid_dtype, long valid_batch_stride, long valid_pitch, int B, int H,
                      int W, float gt_limit, void* record, void* totals, float* epe_map, void* ws,
                      raft_stream_t stream);

/* ---------------------------------------------------------------------------
 * Scoring a flow without ground truth (utils.photo_errors, utils.PhotoMetrics): the data term of the
 * unsupervised flow literature.  Frame 2 is warped back by the flow and compared with frame 1,
 * photometrically and under the soft census transform, over the pixels that are neither masked out nor
 * pushed out of the frame: what the reference's photometric_loss, ternary_loss (unflow_loss_pytorch.py) and
 * census_loss (uflow_loss_pytorch.py) compute from a grid_sample, two 49-channel convolutions and a dozen
 * elementwise passes.  Additive entries: RAFT_HIP_ABI_VERSION stays 19.
 * --------------------------------------------------------------------------- */
/* Definition.  I1, I2 are the two frames in 0..255 units, P = patch in {3, 5, 7}, r = P / 2.  Every value
 * is IEEE fp32, every operation rounded to nearest and nothing fused, unless said otherwise.
 *   W2_c(x)   raft_warp_frame(I2, flow, zeros mode)'s float32 value of channel c at x, bit for bit: the same
 *             taps, blend and valid(x); a flow that is not finite or >= 2^30 gives 0 and valid = 0.
 *   g1, g2    the grey values (I1_0 + I1_1 + I1_2) / 3 and (W2_0 + W2_1 + W2_2) / 3, summed left to right.
 *   census    for each of the P * P offsets o in row-major order (dy outer, dx inner), d = g(x + o) - g(x)
 *             with g(x + o) = 0 where x + o lies outside the H x W frame (the reference's 'same' zero
 *             padding), c_o = d / sqrt(0.81f + d * d).
 *   h(x)      the soft Hamming distance: the sum over o, in that order, of q_o / (0.1f + q_o) with
 *             q_o = (c1_o - c2_o)^2; 0 <= h <= P * P.
 *   e_c(x)    I1_c(x) - W2_c(x), the photometric residual of channel c.
 * Which pixels count:
 *   m(x)      the mask says so (mask == NULL: every pixel; RAFT_MASK_U8 != 0; RAFT_MASK_F32 >= 0.5f, a NaN
 *             fails) AND, with RAFT_PHOTO_OUTGOING, valid(x) (the reference's create_outgoing_mask).
 *   int(x)    r <= x < W - r and r <= y < H - r (zero_mask_border / create_mask).  H or W smaller than P
 *             is legal: no pixel is interior.
 *   finite(x) h(x) and the three squares e_c * e_c are finite.
 * Record.  RAFT_PHOTO_METRICS_SLOTS = 16 slots of 64 bits per sample, int64 counts first, fp64 sums (stored
 * by their bits) after:
 *   RAFT_PM_N_MASK        pixels with m
 *   RAFT_PM_N_CENSUS      pixels with m and int
 *   RAFT_PM_N_VALID       pixels with valid, whatever the mask and the flags
 *   RAFT_PM_N_NONFINITE   pixels with m and not finite: counted in N_MASK / N_CENSUS and in no sum
 *   RAFT_PM_PIXELS        H * W
 *   RAFT_PM_L1_SUM        over m and finite, over c: |e_c|
 *   RAFT_PM_PHOTO_SUM     over m and finite, over c: powf(e_c * e_c + 1e-6f, 0.45f)  (photometric_loss:
 *                         charbonnier(beta = 255) on 0..1 images, in 0..255 units)
 *   RAFT_PM_HAMMING_SUM   over m, int and finite: h
 *   RAFT_PM_CENSUS_SUM    over m, int and finite: powf(h + 0.01f, 0.4f)  (abs_robust_loss: census_loss's
 *                         numerator)
 *   RAFT_PM_TERNARY_SUM   over m, int and finite: powf(h * h + 1e-6f, 0.45f)  (ternary_loss's numerator)
 * each term an fp32 value, widened and added in fp64.  `totals`, if given, is one record that the call ADDS
 * every sample's record into (zero it before the first call), together with
 *   RAFT_PM_IMAGES                  the number of samples with N_CENSUS > 0
 *   RAFT_PM_IMAGE_CENSUS_MEAN_SUM   the fp64 sum of CENSUS_SUM / N_CENSUS over those samples
 * which are 0 in a sample's record, as are the reserved slots 12 .. 15 (written as 0).
 * census_map, if given: float32 [B][H][W] dense, h(x) at every pixel, whatever the mask, border pixels
 * included (with their zero-padded neighbours): the per-pixel confidence image.
 *
 * Launches.  Two, no atomics.  The tile kernel: a work-group of 256 threads owns tiles of
 * RAFT_PHOTO_METRICS_TILE_H x RAFT_PHOTO_METRICS_TILE_W pixels of one sample (a thread 4 rows of one column);
 * it fills g1 and g2 of the tile and its halo of r pixels into LDS, walks the P * P offsets from there, sums
 * in integers and fp64 per thread, by a butterfly per wave, through LDS in wave order per work-group, and
 * writes one partial record to ws.  NB = min(tiles, RAFT_PHOTO_METRICS_MAX_BLOCKS) work-groups per sample,
 * work-group p taking tiles p, p + NB, ...: a function of (H, W) only, never of the device.  The finalize
 * kernel: one work-group adds the partials in index order, writes the records and adds them into the totals
 * in sample order.  Two runs are bitwise equal, and a sample's record does not depend on its batch index.
 *
 * Layout.  frame1 and frame2 share frame_dtype: RAFT_FRAME_F32_NCHW, element (b, c, y, x) at
 * p[b * batch_stride + c * chan_stride + y * pitch + x] (strides in floats, each frame its own, pitch >= W;
 * a crop is read in place by passing its first element), or RAFT_FRAME_U8_NHWC, uint8 [B][H][W][3] dense
 * (the strides are not read).  Three channels.  flow as raft_flow_metrics takes it; mask [B][H][W] with a
 * batch stride and a pitch in elements, or NULL.  record [B][16], totals [16] or NULL, ws of
 * raft_photo_metrics_ws_bytes(B, H, W, patch) bytes (no initialisation needed): 8-byte aligned; float32
 * frames, flow, a float32 mask and census_map 4-byte.  No output aliases an input or another output.
 * B * H * W < 2^30. */
#define RAFT_PHOTO_METRICS_SLOTS 16
#define RAFT_PHOTO_METRICS_TILE_H 16
#define RAFT_PHOTO_METRICS_TILE_W 64
#define RAFT_PHOTO_METRICS_MAX_BLOCKS 512 /* work-groups per sample at most; larger samples wrap */
#define RAFT_PHOTO_OUTGOING 1             /* flags bit 0: pixels whose target leaves the frame do not count */
#define RAFT_PM_N_MASK 0
#define RAFT_PM_N_CENSUS 1
#define RAFT_PM_N_VALID 2
#define RAFT_PM_N_NONFINITE 3
#define RAFT_PM_PIXELS 4
#define RAFT_PM_L1_SUM 5
#define RAFT_PM_PHOTO_SUM 6
#define RAFT_PM_HAMMING_SUM 7
#define RAFT_PM_CENSUS_SUM 8
#define RAFT_PM_TERNARY_SUM 9
#define RAFT_PM_IMAGES 10
#define RAFT_PM_IMAGE_CENSUS_MEAN_SUM 11
#define RAFT_PM_RESERVED 12 /* 12 .. 15 */
/* bytes of raft_photo_metrics' workspace; 0 for sizes (or a patch) it rejects */
size_t raft_photo_metrics_ws_bytes(int B, int H, int W, int patch);
int raft_photo_metrics(const void* frame1, long f1_batch_stride, long f1_chan_stride, long f1_pitch,
                       const void* frame2, long f2_batch_stride, long f2_chan_stride, long f2_pitch, int frame_dtype,
                       const float* flow, long flow_batch_stride, long flow_chan_stride, long flow_pitch,
                       const void* mask, int mask_dtype, long mask_batch_stride, long mask_pitch, int B, int H, int W,
                       int patch, int flags, void* record, void* totals, float* census_map, void* ws,
                       raft_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RAFT_HIP_H_ */
