// Scoring a flow without ground truth (gfx950): the photometric and soft-census data terms of the unsupervised
// flow losses, on the device.
//
//   raft_photo_metrics_ws_bytes  size of the partial-record workspace
//   raft_photo_metrics           two frames, the flow from the first to the second and an optional mask (all read
//                                in place through their strides) -> one record of 16 64-bit slots per sample,
//                                optionally added into running totals, optionally the per-pixel soft Hamming
//                                distance; two launches, no atomics
//
// The definition is in raft_hip.h.
//
//   photo_tile_kernel<P, U8>  grid (NB, B), NB = min(tiles, RAFT_PHOTO_METRICS_MAX_BLOCKS): a function of (H, W)
//                             only.  Work-group (p, b) takes tiles p, p + NB, ... of sample b, each 16 rows x 64
//                             columns; thread t owns column t % 64 and rows 4 (t / 64) .. + 3 of the tile.
//                             Phase 1: every thread warps its 4 pixels (warp_common.hpp: raft_warp_frame's taps
//                             and blend), keeps the residuals e_c and the flags in registers and writes the grey
//                             values g1, g2 to LDS; the halo of r = P / 2 pixels round the tile is filled by all
//                             threads in turn (grey values only); positions outside the frame hold 0, which is the
//                             census transform's zero padding.  One barrier.  Phase 2: a thread walks the 4 + 2 r
//                             LDS rows its four pixels' patches span, P values of each image per row, and adds
//                             every row's P terms to the pixels whose patch holds the row: each h is summed in
//                             row-major order of the offsets, and a row is read once for up to four pixels.  The
//                             reads of a wave are 64 consecutive floats of one row (conflict-free for 4-byte
//                             reads); the LDS row pitch is odd.  Then the per-pixel terms and the per-thread sums
//                             in integers and fp64; record_common.hpp has the reduction from there
//                             (store_partial, record_finalize_kernel) and its fixed order.
//
// Rounding.  Contraction is off for the whole file; `sqrtf` and `/` are correctly rounded under hipcc's
// default -fhip-fp32-correctly-rounded-divide-sqrt; powf is the device library's (its error is measured by
// tests/test_gpu_photo_metrics.py).  Nothing depends on the launch geometry: a pixel's values depend on the
// inputs alone, and the order of every addition is fixed by (B, H, W, P).
#include "common.hpp"
#include "record_common.hpp"
#include "warp_common.hpp"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace raft {
namespace {

constexpr int kSlots = RAFT_PHOTO_METRICS_SLOTS;
constexpr int kTileH = RAFT_PHOTO_METRICS_TILE_H;
constexpr int kTileW = RAFT_PHOTO_METRICS_TILE_W;
constexpr int kMaxBlocks = RAFT_PHOTO_METRICS_MAX_BLOCKS;
constexpr int kMaxR = 3;                          // patch 7
constexpr int kPitch = kTileW + 2 * kMaxR + 1;    // 71 floats: odd
static_assert(kTileH == 16 && kTileW == 64 && kSlots == kRecordSlots, "the kernels below are written for these");
static_assert(kPitch % 2 == 1, "the LDS row pitch is odd");

// 5 counts, the last of them pixels, 5 sums; the per-image mean is CENSUS_SUM / N_CENSUS
using Layout = RecordLayout<5, RAFT_PM_PIXELS, 5, RAFT_PM_CENSUS_SUM, RAFT_PM_N_CENSUS>;
static_assert(Layout::kFirstSum == RAFT_PM_L1_SUM && Layout::kImages == RAFT_PM_IMAGES &&
                  Layout::kMeanSum == RAFT_PM_IMAGE_CENSUS_MEAN_SUM && Layout::kReserved == RAFT_PM_RESERVED &&
                  RAFT_PM_N_MASK == 0 && RAFT_PM_N_NONFINITE == Layout::kSummed - 1 &&
                  RAFT_PM_TERNARY_SUM == RAFT_PM_IMAGES - 1,
              "the layout is raft_hip.h's");

struct PhotoArgs {
  WarpArgs w;             // frame 2 and the flow as raft_warp_frame takes them (zeros mode, C = 3); B, H, W
  const void* img1;       // float32: element (0, 0, 0, 0); uint8: the dense [B][H][W][3] base
  long i1sb, i1sc, i1pitch;
  MaskView m;
  int outgoing;
  long long* ws;          // [B][nb][16]
  float* census_map;      // [B][H][W] or null
  int nb, tiles_x, tiles;
};

struct Acc {
  unsigned n_mask, n_census, n_valid, n_nonfinite;   // (a sample has fewer than 2^30 pixels)
  double l1, photo, hamming, census, ternary;
};

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < INFINITY; }

template <bool U8>
__device__ __forceinline__ float frame1_at(const PhotoArgs& a, int b, int c, int y, int x) {
  if (U8) {
    const unsigned char* p = static_cast<const unsigned char*>(a.img1);
    return (float)p[(((long)b * a.w.H + y) * a.w.W + x) * 3 + c];
  }
  const float* p = static_cast<const float*>(a.img1);
  return p[(long)b * a.i1sb + (long)c * a.i1sc + (long)y * a.i1pitch + x];
}

// Pixel (y, x) of sample b, inside the frame: the grey values, the residuals, valid.
template <bool U8>
__device__ __forceinline__ void photo_pixel(const PhotoArgs& a, int b, int y, int x, float& g1, float& g2, float* e,
                                            bool& valid) {
  const float* f = a.w.flow + (long)b * a.w.fsb + (long)y * a.w.fpitch + x;
  const Taps t = warp_taps(a.w, y, x, f[0], f[a.w.fsc]);
  float i1[3], w2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    i1[c] = frame1_at<U8>(a, b, c, y, x);
    w2[c] = warp_blend<U8>(a.w, t, b, c);
    e[c] = i1[c] - w2[c];
  }
  g1 = (i1[0] + i1[1] + i1[2]) / 3.0f;
  g2 = (w2[0] + w2[1] + w2[2]) / 3.0f;
  valid = t.valid != 0;
}

// one offset's term of h: d1, d2 the grey differences of the two images
__device__ __forceinline__ float census_term(float d1, float d2) {
  const float c1 = d1 / sqrtf(0.81f + d1 * d1);
  const float c2 = d2 / sqrtf(0.81f + d2 * d2);
  const float delta = c1 - c2;
  const float q = delta * delta;
  return q / (0.1f + q);
}

template <int P, bool U8>
__global__ __launch_bounds__(256) void photo_tile_kernel(PhotoArgs a) {
  constexpr int R = P / 2;
  constexpr int LW = kTileW + 2 * R;                 // LDS columns in use
  constexpr int kTop = R * LW;                       // halo positions above (and below) the tile
  constexpr int kHalo = 2 * kTop + kTileH * 2 * R;   // ... and beside it
  __shared__ float s_g1[(kTileH + 2 * R) * kPitch];
  __shared__ float s_g2[(kTileH + 2 * R) * kPitch];
  const int H = a.w.H, W = a.w.W;
  const int tx = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ly0 = R + 4 * wave, lx = R + tx;         // LDS position of the thread's first pixel
  for (int b = blockIdx.y; b < a.w.B; b += gridDim.y) {   // (gridDim.y = B up to the grid's limit)
    Acc acc = {};
    for (int tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
      const int trow = tile / a.tiles_x;
      const int y0 = trow * kTileH, x0 = (tile - trow * a.tiles_x) * kTileW;
      const int x = x0 + tx;

      // phase 1: the thread's own pixels
      float e[4][3];
      bool exists[4], valid[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int y = y0 + 4 * wave + k;
        float g1 = 0.0f, g2 = 0.0f;
        e[k][0] = e[k][1] = e[k][2] = 0.0f;
        valid[k] = false;
        exists[k] = x < W && y < H;
        if (exists[k]) photo_pixel<U8>(a, b, y, x, g1, g2, e[k], valid[k]);
        s_g1[(ly0 + k) * kPitch + lx] = g1;
        s_g2[(ly0 + k) * kPitch + lx] = g2;
      }
      // ... and the halo: R rows above, R below (LW wide), then R columns either side of the 16 rows
      for (int i = threadIdx.x; i < kHalo; i += 256) {
        int ly, lxh;
        if (i < 2 * kTop) {
          const int row = i / LW;
          lxh = i - row * LW;
          ly = row < R ? row : kTileH + row;
        } else {
          const int j = i - 2 * kTop;
          const int row = j / (2 * R), c = j - row * (2 * R);
          ly = R + row;
          lxh = c < R ? c : kTileW + c;
        }
        const int gy = y0 - R + ly, gx = x0 - R + lxh;
        float g1 = 0.0f, g2 = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
          float eh[3];
          bool vh;
          photo_pixel<U8>(a, b, gy, gx, g1, g2, eh, vh);
        }
        s_g1[ly * kPitch + lxh] = g1;
        s_g2[ly * kPitch + lxh] = g2;
      }
      __syncthreads();

      // phase 2: h of the four pixels, each summed over its offsets in row-major order
      float c1[4], c2[4], h[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        c1[k] = s_g1[(ly0 + k) * kPitch + lx];
        c2[k] = s_g2[(ly0 + k) * kPitch + lx];
        h[k] = 0.0f;
      }
#pragma unroll 1
      for (int j = 0; j < 4 + 2 * R; ++j) {   // LDS row ly0 - R + j: offset dy = j - k - R of pixel k
        float r1[P], r2[P];
        const int base = (ly0 - R + j) * kPitch + lx - R;
#pragma unroll
        for (int dx = 0; dx < P; ++dx) {
          r1[dx] = s_g1[base + dx];
          r2[dx] = s_g2[base + dx];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if ((unsigned)(j - k) < (unsigned)P) {   // (uniform over the work-group)
#pragma unroll
            for (int dx = 0; dx < P; ++dx) h[k] += census_term(r1[dx] - c1[k], r2[dx] - c2[k]);
          }
        }
      }

#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!exists[k]) continue;
        const int y = y0 + 4 * wave + k;
        if (a.census_map) a.census_map[((long)b * H + y) * W + x] = h[k];
        acc.n_valid += valid[k];
        if (!(mask_says(a.m, (long)b * a.m.sb + (long)y * a.m.pitch + x) && (valid[k] || !a.outgoing))) continue;
        const bool interior = x >= R && x < W - R && y >= R && y < H - R;
        ++acc.n_mask;
        acc.n_census += interior;
        const float s0 = e[k][0] * e[k][0], s1 = e[k][1] * e[k][1], s2 = e[k][2] * e[k][2];
        if (!(finite32(h[k]) && finite32(s0) && finite32(s1) && finite32(s2))) {
          ++acc.n_nonfinite;
          continue;
        }
        acc.l1 += (double)fabsf(e[k][0]);
        acc.l1 += (double)fabsf(e[k][1]);
        acc.l1 += (double)fabsf(e[k][2]);
        acc.photo += (double)powf(s0 + 1e-6f, 0.45f);
        acc.photo += (double)powf(s1 + 1e-6f, 0.45f);
        acc.photo += (double)powf(s2 + 1e-6f, 0.45f);
        if (interior) {
          acc.hamming += (double)h[k];
          acc.census += (double)powf(h[k] + 0.01f, 0.4f);
          acc.ternary += (double)powf(h[k] * h[k] + 1e-6f, 0.45f);
        }
      }
      __syncthreads();   // every read of this tile's LDS is done before the next tile is written
    }

    const unsigned cnts[Layout::kSummed] = {acc.n_mask, acc.n_census, acc.n_valid, acc.n_nonfinite};
    const double sums[Layout::kSums] = {acc.l1, acc.photo, acc.hamming, acc.census, acc.ternary};
    store_partial<Layout>(cnts, sums, a.ws + ((long)b * a.nb + blockIdx.x) * kSlots, wave);
  }
}

bool patch_ok(int patch) { return patch == 3 || patch == 5 || patch == 7; }

long photo_tiles_x(int W) { return ((long)W + kTileW - 1) / kTileW; }
long photo_tiles(int H, int W) { return (((long)H + kTileH - 1) / kTileH) * photo_tiles_x(W); }

// NB of the header comment: work-groups (and partial records) per sample
int photo_blocks(int H, int W) {
  const long t = photo_tiles(H, W);
  return (int)(t > kMaxBlocks ? kMaxBlocks : t);
}

template <int P>
void launch_tiles(const PhotoArgs& a, bool u8, dim3 grid, hipStream_t s) {
  if (u8)
    hipLaunchKernelGGL((photo_tile_kernel<P, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((photo_tile_kernel<P, false>), grid, dim3(256), 0, s, a);
}

}  // namespace
}  // namespace raft

using namespace raft;

extern "C" size_t raft_photo_metrics_ws_bytes(int B, int H, int W, int patch) {
  if (!(size_ok(B, H, W) && patch_ok(patch))) return 0;
  return (size_t)B * photo_blocks(H, W) * kSlots * sizeof(long long);
}

extern "C" int raft_photo_metrics(const void* frame1, long f1_batch_stride, long f1_chan_stride, long f1_pitch,
                                  const void* frame2, long f2_batch_stride, long f2_chan_stride, long f2_pitch,
                                  int frame_dtype, const float* flow, long flow_batch_stride, long flow_chan_stride,
                                  long flow_pitch, const void* mask, int mask_dtype, long mask_batch_stride,
                                  long mask_pitch, int B, int H, int W, int patch, int flags, void* record,
                                  void* totals, float* census_map, void* ws, raft_stream_t stream) {
  RAFT_REQUIRE(frame1 && frame2 && flow && record && ws, "raft_photo_metrics: null pointer");
  const char* who = "raft_photo_metrics";
  RAFT_REQUIRE(patch_ok(patch), "raft_photo_metrics: patch must be 3, 5 or 7, got %d", patch);
  if (const int rc = check_size(who, B, H, W)) return rc;
  RAFT_REQUIRE(frame_dtype == RAFT_FRAME_F32_NCHW || frame_dtype == RAFT_FRAME_U8_NHWC,
               "raft_photo_metrics: unknown frame dtype tag %d", frame_dtype);
  if (const int rc = check_mask(who, mask, mask_dtype, mask_batch_stride, mask_pitch, W)) return rc;
  RAFT_REQUIRE((flags & ~RAFT_PHOTO_OUTGOING) == 0, "raft_photo_metrics: unknown flags %d", flags);
  const bool u8 = frame_dtype == RAFT_FRAME_U8_NHWC;
  RAFT_REQUIRE(flow_pitch >= W && flow_batch_stride >= 0 && flow_chan_stride >= 0,
               "raft_photo_metrics: bad strides (a row pitch holds W floats; strides are not negative)");
  RAFT_REQUIRE(u8 || (f1_pitch >= W && f1_batch_stride >= 0 && f1_chan_stride >= 0 && f2_pitch >= W &&
                      f2_batch_stride >= 0 && f2_chan_stride >= 0),
               "raft_photo_metrics: bad frame strides (a row pitch holds W floats; strides are not negative)");
  RAFT_REQUIRE((((uintptr_t)flow | (uintptr_t)census_map) & 3) == 0 &&
                   (u8 || (((uintptr_t)frame1 | (uintptr_t)frame2) & 3) == 0),
               "raft_photo_metrics: misaligned pointer (float32 frames, flow, census_map 4 bytes)");
  const void* ins[4] = {frame1, frame2, flow, mask};
  if (const int rc = check_outputs(who, record, totals, ws, census_map, ins, 4)) return rc;
  PhotoArgs a;
  a.w.flow = flow;
  a.w.fsb = flow_batch_stride;
  a.w.fsc = flow_chan_stride;
  a.w.fpitch = flow_pitch;
  a.w.img = frame2;
  a.w.isb = f2_batch_stride;
  a.w.isc = f2_chan_stride;
  a.w.ipitch = f2_pitch;
  a.w.out = nullptr;
  a.w.valid = nullptr;
  a.w.B = B;
  a.w.C = 3;
  a.w.H = H;
  a.w.W = W;
  a.w.border = 0;
  a.img1 = frame1;
  a.i1sb = f1_batch_stride;
  a.i1sc = f1_chan_stride;
  a.i1pitch = f1_pitch;
  a.m = mask_view(mask, mask_dtype, mask_batch_stride, mask_pitch);
  a.outgoing = (flags & RAFT_PHOTO_OUTGOING) ? 1 : 0;
  a.ws = static_cast<long long*>(ws);
  a.census_map = census_map;
  a.nb = photo_blocks(H, W);
  a.tiles_x = (int)photo_tiles_x(W);
  a.tiles = (int)photo_tiles(H, W);
  hipStream_t s = as_stream(stream);
  const dim3 grid(a.nb, B < 65535 ? B : 65535);
  if (patch == 3)
    launch_tiles<3>(a, u8, grid, s);
  else if (patch == 5)
    launch_tiles<5>(a, u8, grid, s);
  else
    launch_tiles<7>(a, u8, grid, s);
  const int rc = check_launch("raft_photo_metrics (tiles)");
  if (rc) return rc;
  return launch_finalize<Layout>(who, ws, record, totals, B, a.nb, H, W, s);
}
