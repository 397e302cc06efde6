// Resizing frames and flows (gfx950): raft_resize, one launch.
//
//   bilinear  torch.nn.functional.interpolate(mode="bilinear", align_corners=False / True)
//   area      torch's mode="area" (adaptive average pooling)
//
// The definition is in raft_hip.h.  The source position of an output sample is a ratio of two integers, so the
// source index and the remainder come out of one integer division and the weight out of one correctly rounded
// fp32 division: no fp32 coordinate is ever formed, and the error of the weight does not grow with the frame's
// size.  The division is 32-bit where the numerator fits (2 * D * S < 2^31, decided per axis on the host) and
// 64-bit otherwise.  The blend is written as in the header with contraction off: one rounding per written
// operation, which is what the 8 u T bound of the header counts.  All four taps are always read and blended,
// so a NaN / Inf under a weight of 0 still reaches the output, as the formula (and torch) has it.
//
// Memory.  A thread owns 4 consecutive output x of one output row; a wave covers 256 consecutive x of one
// row (a work-group: 1, 2 or 4 rows of 1024, 512 or 256 x, by the output's width).  The column quantities
// (x0, x1, lx; or the box's columns) are computed once per thread and kept over the rows the thread walks; the
// row quantities (y0, y1, ly) once per row, for the thread's 4 * C outputs.  Taps are gathered: neighbouring
// outputs share them through L1 / L2, the algorithmic traffic is one read of the source.  A uint8 NHWC pixel is
// read as its 3 bytes by the thread that owns the output pixel, and written 4 pixels at a time as three dwords
// where the address is 4-byte aligned; a float32 NCHW output is one 16-byte store per channel where the address
// is 16-byte aligned, scalar stores otherwise and in a row's tail.  No LDS, no atomics.
#include "common.hpp"

#include <cmath>
#include <cstdint>

namespace raft {
namespace {

struct ResizeArgs {
  const void* src;   // float32: element (0, 0, 0, 0) of the crop; uint8: the dense [B][Hs][Ws][3] base
  long ssb, ssc, spitch;
  void* dst;
  int B, C, Hs, Ws, Hd, Wd;
  int align;           // bilinear: align_corners
  int narrow_x, narrow_y;   // the axis' numerators fit 32 bits
  int txs;             // log2 of the threads along x in a work-group (6, 7 or 8)
  float mul0, mul1;
};

// nearest (ties to even), saturated, NaN -> 0: raft_warp_frame's
__device__ __forceinline__ unsigned char resize_byte(float x) {
  return (unsigned char)rintf(fminf(fmaxf(x, 0.0f), 255.0f));
}

template <typename U>
__device__ __forceinline__ void lin_div(U n, U den, int S, int& i0, int& i1, float& lam) {
  const U q = n / den, r = n - q * den;
  i0 = q < (U)(S - 1) ? (int)q : S - 1;
  i1 = i0 + 1 < S ? i0 + 1 : S - 1;
  lam = (float)r / (float)den;   // r < den <= 2^24 (D <= 2^23): both exact, one correctly rounded division
}

// Output index d of D over S source samples: taps i0, i1 and the weight of i1.
__device__ __forceinline__ void lin_coord(int d, int D, int S, bool align, bool narrow, int& i0, int& i1,
                                          float& lam) {
  if (narrow) {
    unsigned n, den;
    if (align) {
      n = (unsigned)d * (unsigned)(S - 1);
      den = D > 1 ? (unsigned)(D - 1) : 1u;
    } else {
      const int t = (2 * d + 1) * S - D;
      n = t > 0 ? (unsigned)t : 0u;
      den = 2u * (unsigned)D;
    }
    lin_div<unsigned>(n, den, S, i0, i1, lam);
  } else {
    unsigned long long n, den;
    if (align) {
      n = (unsigned long long)d * (unsigned long long)(S - 1);
      den = D > 1 ? (unsigned long long)(D - 1) : 1ull;
    } else {
      const long long t = (2ll * d + 1) * S - D;
      n = t > 0 ? (unsigned long long)t : 0ull;
      den = 2ull * (unsigned long long)D;
    }
    lin_div<unsigned long long>(n, den, S, i0, i1, lam);
  }
}

// Area mode's box of output index d: source samples lo .. hi - 1 (never empty, inside 0 .. S - 1).
__device__ __forceinline__ void box_coord(int d, int D, int S, int& lo, int& hi) {
  lo = (int)(((long long)d * S) / D);
  hi = (int)((((long long)d + 1) * S + D - 1) / D);
}

template <bool IN_U8>
__device__ __forceinline__ float resize_tap(const ResizeArgs& a, int b, int c, int y, int x) {
  if (IN_U8) {
    const unsigned char* p = static_cast<const unsigned char*>(a.src);
    return (float)p[(((long)b * a.Hs + y) * a.Ws + x) * 3 + c];
  }
  const float* p = static_cast<const float*>(a.src);
  return p[(long)b * a.ssb + (long)c * a.ssc + (long)y * a.spitch + x];
}

// One output value before the flow multiplier.  Bilinear: (ya, yb, ly) = (y0, y1, ly), (xa, xb, lx) likewise.
// Area: rows ya .. yb - 1, columns xa .. xb - 1.
template <bool IN_U8, bool AREA>
__device__ __forceinline__ float resize_value(const ResizeArgs& a, int b, int c, int ya, int yb, float ly, int xa,
                                              int xb, float lx) {
#pragma clang fp contract(off)
  if (AREA) {
    float s = 0.0f;
    for (int y = ya; y < yb; ++y)
      for (int x = xa; x < xb; ++x) s = s + resize_tap<IN_U8>(a, b, c, y, x);
    return s / (float)((yb - ya) * (xb - xa));   // the count is < 2^30; exact in fp32 below 2^24
  }
  const float v00 = resize_tap<IN_U8>(a, b, c, ya, xa), v01 = resize_tap<IN_U8>(a, b, c, ya, xb);
  const float v10 = resize_tap<IN_U8>(a, b, c, yb, xa), v11 = resize_tap<IN_U8>(a, b, c, yb, xb);
  const float wx0 = 1.0f - lx, wy0 = 1.0f - ly;
  const float top = wx0 * v00 + lx * v01;
  const float bot = wx0 * v10 + lx * v11;
  return wy0 * top + ly * bot;
}

__device__ __forceinline__ float resize_scale(const ResizeArgs& a, int c, float v) {
#pragma clang fp contract(off)
  return c == 0 ? v * a.mul0 : c == 1 ? v * a.mul1 : v;
}

template <bool IN_U8, bool OUT_U8, bool AREA>
__global__ __launch_bounds__(256) void resize_kernel(ResizeArgs a) {
  const int tx = threadIdx.x & ((1 << a.txs) - 1), ry = threadIdx.x >> a.txs;
  const int rpb = 256 >> a.txs;   // rows a work-group takes per pass
  const long xg_l = (((long)blockIdx.x << a.txs) + tx) * 4;
  if (xg_l >= a.Wd) return;
  const int xg = (int)xg_l;
  const int cnt = a.Wd - xg < 4 ? a.Wd - xg : 4;

  int xa[4], xb[4];
  float lx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = k < cnt ? xg + k : xg;   // a tail lane repeats its first column: in bounds, never stored
    lx[k] = 0.0f;
    if (AREA)
      box_coord(x, a.Wd, a.Ws, xa[k], xb[k]);
    else
      lin_coord(x, a.Wd, a.Ws, a.align != 0, a.narrow_x != 0, xa[k], xb[k], lx[k]);
  }

  const long rows = (long)a.B * a.Hd;
  for (long row = (long)blockIdx.y * rpb + ry; row < rows; row += (long)gridDim.y * rpb) {
    const int b = (int)(row / a.Hd), y = (int)(row - (long)b * a.Hd);
    int ya, yb;
    float ly = 0.0f;
    if (AREA)
      box_coord(y, a.Hd, a.Hs, ya, yb);
    else
      lin_coord(y, a.Hd, a.Hs, a.align != 0, a.narrow_y != 0, ya, yb, ly);

    if (OUT_U8) {
      unsigned char by[12];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          by[3 * k + c] =
              resize_byte(resize_scale(a, c, resize_value<IN_U8, AREA>(a, b, c, ya, yb, ly, xa[k], xb[k], lx[k])));
      unsigned char* o = static_cast<unsigned char*>(a.dst) + (row * a.Wd + xg) * 3;
      if (cnt == 4 && (((uintptr_t)o) & 3) == 0) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          o32[j] = (uint32_t)by[4 * j] | ((uint32_t)by[4 * j + 1] << 8) | ((uint32_t)by[4 * j + 2] << 16) |
                   ((uint32_t)by[4 * j + 3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < 12; ++j)
          if (j < 3 * cnt) o[j] = by[j];
      }
    } else {
      float* out = static_cast<float*>(a.dst);
      for (int c = 0; c < a.C; ++c) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          v[k] = resize_scale(a, c, resize_value<IN_U8, AREA>(a, b, c, ya, yb, ly, xa[k], xb[k], lx[k]));
        float* o = out + (((long)b * a.C + c) * a.Hd + y) * a.Wd + xg;
        if (cnt == 4 && (((uintptr_t)o) & 15) == 0) {
          *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < cnt) o[k] = v[k];
        }
      }
    }
  }
}

template <bool IN_U8, bool OUT_U8>
void launch_resize(const ResizeArgs& a, bool area, dim3 grid, hipStream_t s) {
  if (area)
    hipLaunchKernelGGL((resize_kernel<IN_U8, OUT_U8, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((resize_kernel<IN_U8, OUT_U8, false>), grid, dim3(256), 0, s, a);
}

}  // namespace
}  // namespace raft

using namespace raft;

extern "C" int raft_resize(const void* src, int src_dtype, long src_batch_stride, long src_chan_stride,
                           long src_pitch, int top, int left, int B, int C, int Hs, int Ws, void* dst, int dst_dtype,
                           int Hd, int Wd, int mode, int flags, float mul0, float mul1, raft_stream_t stream) {
  RAFT_REQUIRE(src && dst, "raft_resize: null pointer");
  RAFT_REQUIRE(src_dtype == RAFT_FRAME_F32_NCHW || src_dtype == RAFT_FRAME_U8_NHWC,
               "raft_resize: unknown source dtype tag %d", src_dtype);
  RAFT_REQUIRE(dst_dtype == RAFT_FRAME_F32_NCHW || dst_dtype == RAFT_FRAME_U8_NHWC,
               "raft_resize: unknown destination dtype tag %d", dst_dtype);
  RAFT_REQUIRE(mode == RAFT_RESIZE_BILINEAR || mode == RAFT_RESIZE_AREA, "raft_resize: unknown mode %d", mode);
  RAFT_REQUIRE((flags & ~RAFT_RESIZE_ALIGN_CORNERS) == 0, "raft_resize: unknown flags %d", flags);
  RAFT_REQUIRE(mode == RAFT_RESIZE_BILINEAR || flags == 0, "raft_resize: align_corners is a bilinear option");
  const bool in_u8 = src_dtype == RAFT_FRAME_U8_NHWC, out_u8 = dst_dtype == RAFT_FRAME_U8_NHWC;
  RAFT_REQUIRE(B > 0 && C >= 1 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0,
               "raft_resize: bad size B %d C %d, %d x %d -> %d x %d", B, C, Hs, Ws, Hd, Wd);
  // (each factor is below 2^31, so a product that passed 2^30 cannot wrap a long back under it)
  RAFT_REQUIRE((long)B * C < (1L << 30) && (long)B * C * Hs < (1L << 30) && (long)B * C * Hs * Ws < (1L << 30) &&
                   (long)B * C * Hd < (1L << 30) && (long)B * C * Hd * Wd < (1L << 30),
               "raft_resize: B * C * H * W must stay below 2^30 for the source and for the destination");
  RAFT_REQUIRE(!(in_u8 || out_u8) || C == 3, "raft_resize: a uint8 frame has 3 channels, got C = %d", C);
  RAFT_REQUIRE(top >= 0 && left >= 0, "raft_resize: negative crop offset");
  RAFT_REQUIRE(in_u8 || (src_pitch >= (long)left + Ws && src_batch_stride >= 0 && src_chan_stride >= 0),
               "raft_resize: bad source strides (a row pitch holds left + Ws floats; strides are not negative)");
  RAFT_REQUIRE((in_u8 || ((uintptr_t)src & 3) == 0) && (out_u8 || ((uintptr_t)dst & 3) == 0),
               "raft_resize: misaligned pointer (float32 source and destination: 4 bytes)");
  RAFT_REQUIRE((const void*)dst != src, "raft_resize: the destination aliases the source");
  ResizeArgs a;
  a.src = in_u8 ? src : (const void*)(static_cast<const float*>(src) + (long)top * src_pitch + left);
  a.ssb = src_batch_stride;
  a.ssc = src_chan_stride;
  a.spitch = src_pitch;
  a.dst = dst;
  a.B = B;
  a.C = C;
  a.Hs = Hs;
  a.Ws = Ws;
  a.Hd = Hd;
  a.Wd = Wd;
  a.align = (flags & RAFT_RESIZE_ALIGN_CORNERS) ? 1 : 0;
  a.narrow_x = 2L * Wd * Ws < (1L << 31) ? 1 : 0;
  a.narrow_y = 2L * Hd * Hs < (1L << 31) ? 1 : 0;
  a.mul0 = mul0;
  a.mul1 = mul1;
  const long groups = ((long)Wd + 3) / 4;   // threads along x
  a.txs = groups > 128 ? 8 : groups > 64 ? 7 : 6;
  const long gx = (groups + (1L << a.txs) - 1) >> a.txs;   // <= 2^20
  const long rpb = 256 >> a.txs, passes = ((long)B * Hd + rpb - 1) / rpb;
  long gy = gx >= 2048 ? 1 : 2048 / gx;   // about 8 work-groups per CU; the rows beyond are walked
  gy = gy < passes ? gy : passes;
  gy = gy > 65535 ? 65535 : gy;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  hipStream_t s = as_stream(stream);
  const bool area = mode == RAFT_RESIZE_AREA;
  if (in_u8 && out_u8)
    launch_resize<true, true>(a, area, grid, s);
  else if (in_u8)
    launch_resize<true, false>(a, area, grid, s);
  else if (out_u8)
    launch_resize<false, true>(a, area, grid, s);
  else
    launch_resize<false, false>(a, area, grid, s);
  return check_launch("raft_resize");
}
