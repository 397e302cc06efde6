// Warping by a flow field (gfx950).
//
//   raft_warp_frame     backward warp of a frame: out(x) = bilinear frame(x + flow(x)), one launch
//   raft_splat_density  forward-warp density: every source pixel splats its four bilinear weights at
//                       x + flow(x); three launches (zero, splat, convert)
//
// The warp (definition: raft_hip.h).  Per axis the sampling position is taken as raft_fb_consistency takes
// it: fl = floor(d), t = d - fl, i0 = j + (int)fl; j + d is never formed, so the error of the weights does
// not grow with the frame's size and the frame test is an integer comparison.  Zeros mode: a tap outside
// the H x W crop has value 0 and is not read.  Border mode: the base is clamped per axis (t = 0 there).
// The blend is fb_pixel's, wy0 (wx0 v00 + ax v01) + ay (wx0 v10 + ax v11), contraction off: one rounding
// per written operation, which is what the 10 u T bound of tests/test_warp_host.py counts.
//
// Memory.  A thread owns 4 consecutive elements of the flat [B*H*W] pixel order.  Its two flow loads are
// 16-byte where the four pixels share a row and the addresses are aligned (always at W % 4 == 0 with an
// aligned pitch and crop), scalar otherwise.  Taps are gathered (neighbouring pixels share them through
// L1 / L2; the algorithmic traffic is one read of the frame).  Stores: `valid` one 4-byte store; a uint8
// NHWC output 12 bytes as three dwords; a float32 NCHW output one 16-byte store per channel where the four
// pixels lie in one image and the address is aligned (H * W % 4 == 0), scalar otherwise and in the tail.
// A wave covers 256 consecutive pixels: x-runs of rows.
//
// The density.  Float atomic sums depend on arrival order, so the weights are summed as integers: each
// fp32 weight (<= 1) times 2^32 is exact in fp32 and is truncated to an unsigned 64-bit integer, added
// with 64-bit integer atomics (B * H * W < 2^30 sources of at most 4 * 2^32 each: the sum stays below
// 2^62), and one last pass converts every pixel with a single rounding.  The result does not depend on
// the order the adds arrive in: two runs are bitwise equal.
#include "common.hpp"
#include "warp_common.hpp"   // WarpArgs, Taps, warp_axis, flow_ok, warp_taps, warp_tap, warp_blend

#include <cmath>
#include <cstdint>

namespace raft {
namespace {

// nearest (ties to even), saturated, NaN -> 0
__device__ __forceinline__ unsigned char warp_byte(float x) {
  return (unsigned char)rintf(fminf(fmaxf(x, 0.0f), 255.0f));
}

// The flow of a thread's (up to) four pixels e0 .. e0 + cnt - 1 of the flat order, and where they lie.
struct Run {
  int b[4], y[4], x[4];
  f32x4 fx, fy;
};

__device__ __forceinline__ void load_run(const float* flow, long fsb, long fsc, long fpitch, int H, int W, long e0,
                                         int cnt, Run& r) {
  const long HW = (long)H * W;
  int b = (int)(e0 / HW);
  const int rem = (int)(e0 - (long)b * HW);
  int y = rem / W, x = rem - y * W;
  const float* px = flow + (long)b * fsb + (long)y * fpitch + x;
  const float* py = px + fsc;
  if (cnt == 4 && x + 3 < W && ((((uintptr_t)px) | ((uintptr_t)py)) & 15) == 0) {
    r.fx = *reinterpret_cast<const f32x4*>(px);
    r.fy = *reinterpret_cast<const f32x4*>(py);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      r.b[k] = b;
      r.y[k] = y;
      r.x[k] = x + k;
    }
    return;
  }
  r.fx = r.fy = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    r.b[k] = b;
    r.y[k] = y;
    r.x[k] = x;
    if (k < cnt) {
      const float* q = flow + (long)b * fsb + (long)y * fpitch + x;
      r.fx[k] = q[0];
      r.fy[k] = q[fsc];
      const bool row_end = x + 1 == W;
      x = row_end ? 0 : x + 1;
      const bool image_end = row_end && y + 1 == H;
      y = image_end ? 0 : y + (row_end ? 1 : 0);
      b += image_end ? 1 : 0;
    }
  }
}

template <bool IN_U8, bool OUT_U8>
__global__ __launch_bounds__(256) void warp_frame_kernel(WarpArgs a) {
  const long HW = (long)a.H * a.W;
  const long n = (long)a.B * HW;   // < 2^30: checked on the host
  const long groups = (n + 3) >> 2;
  for (long gi = blockIdx.x * (long)blockDim.x + threadIdx.x; gi < groups; gi += (long)gridDim.x * blockDim.x) {
    const long e0 = gi << 2;
    const int cnt = (int)(n - e0 < 4 ? n - e0 : 4);
    Run r;
    load_run(a.flow, a.fsb, a.fsc, a.fpitch, a.H, a.W, e0, cnt, r);
    Taps t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = warp_taps(a, r.y[k], r.x[k], r.fx[k], r.fy[k]);

    unsigned char* vo = a.valid + e0;
    if (cnt == 4) {
      // e0 % 4 == 0 and the base is 4-byte aligned (host check)
      *reinterpret_cast<uint32_t*>(vo) = (uint32_t)t[0].valid | ((uint32_t)t[1].valid << 8) |
                                         ((uint32_t)t[2].valid << 16) | ((uint32_t)t[3].valid << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) vo[k] = t[k].valid;
    }

    if (OUT_U8) {
      unsigned char by[12];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) by[3 * k + c] = k < cnt ? warp_byte(warp_blend<IN_U8>(a, t[k], r.b[k], c)) : 0;
      unsigned char* o = static_cast<unsigned char*>(a.out) + 3 * e0;
      if (cnt == 4) {
        // 3 * e0 = 12 * (e0 / 4) and the base is 4-byte aligned (host check)
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
      float* out = static_cast<float*>(a.out);
      const long rem0 = e0 - (long)r.b[0] * HW;
      const bool one_image = cnt == 4 && rem0 + 3 < HW;
      for (int c = 0; c < a.C; ++c) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < cnt ? warp_blend<IN_U8>(a, t[k], r.b[k], c) : 0.0f;
        float* o = out + ((long)r.b[0] * a.C + c) * HW + rem0;
        if (one_image && (((uintptr_t)o) & 15) == 0) {
          f32x4 ov;
#pragma unroll
          for (int k = 0; k < 4; ++k) ov[k] = v[k];
          *reinterpret_cast<f32x4*>(o) = ov;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < cnt) out[((long)r.b[k] * a.C + c) * HW + ((long)r.y[k] * a.W + r.x[k])] = v[k];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------- density

struct SplatArgs {
  const float* flow;   // element (0, 0, 0, 0) of the crop
  long fsb, fsc, fpitch;
  unsigned long long* ws;   // [B*H*W] fixed-point sums, unit 2^-32
  float* density;
  int B, H, W;
};

__global__ __launch_bounds__(256) void splat_zero_kernel(SplatArgs a) {
  const long n = (long)a.B * a.H * a.W;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) a.ws[i] = 0ull;
}

// weight (0 <= w <= 1) -> fixed point, unit 2^-32: the product is exact in fp32, the cast truncates
__device__ __forceinline__ void splat_add(unsigned long long* p, float w) {
  const unsigned long long q = (unsigned long long)(w * 4294967296.0f);
  if (q) atomicAdd(p, q);
}

__global__ __launch_bounds__(256) void splat_kernel(SplatArgs a) {
#pragma clang fp contract(off)
  const long HW = (long)a.H * a.W;
  const long n = (long)a.B * HW;
  const long groups = (n + 3) >> 2;
  for (long gi = blockIdx.x * (long)blockDim.x + threadIdx.x; gi < groups; gi += (long)gridDim.x * blockDim.x) {
    const long e0 = gi << 2;
    const int cnt = (int)(n - e0 < 4 ? n - e0 : 4);
    Run r;
    load_run(a.flow, a.fsb, a.fsc, a.fpitch, a.H, a.W, e0, cnt, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= cnt || !(flow_ok(r.fx[k]) && flow_ok(r.fy[k]))) continue;
      const float flx = floorf(r.fx[k]), fly = floorf(r.fy[k]);
      const float ax = r.fx[k] - flx, ay = r.fy[k] - fly;
      const int x0 = r.x[k] + (int)flx, y0 = r.y[k] + (int)fly;
      if (x0 < 0 || x0 > a.W - 1 || y0 < 0 || y0 > a.H - 1) continue;
      const int x1 = x0 + 1 < a.W ? x0 + 1 : a.W - 1, y1 = y0 + 1 < a.H ? y0 + 1 : a.H - 1;
      const float wx0 = 1.0f - ax, wy0 = 1.0f - ay;
      unsigned long long* w = a.ws + (long)r.b[k] * HW;
      splat_add(w + (long)y0 * a.W + x0, wx0 * wy0);
      splat_add(w + (long)y0 * a.W + x1, ax * wy0);
      splat_add(w + (long)y1 * a.W + x0, wx0 * ay);
      splat_add(w + (long)y1 * a.W + x1, ax * ay);
    }
  }
}

__global__ __launch_bounds__(256) void splat_convert_kernel(SplatArgs a) {
  const long n = (long)a.B * a.H * a.W;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    a.density[i] = (float)a.ws[i] * 2.3283064365386963e-10f;   // one rounding (the cast); * 2^-32 is exact
}

}  // namespace
}  // namespace raft

using namespace raft;

extern "C" int raft_warp_frame(const float* flow, long flow_batch_stride, long flow_chan_stride, long flow_pitch,
                               const void* frame, int frame_dtype, long frame_batch_stride, long frame_chan_stride,
                               long frame_pitch, int top, int left, int B, int C, int H, int W, int flags, void* out,
                               int out_dtype, unsigned char* valid, raft_stream_t stream) {
  RAFT_REQUIRE(flow && frame && out && valid, "raft_warp_frame: null pointer");
  RAFT_REQUIRE(size_ok(B, H, W), "raft_warp_frame: bad size %d x %d x %d", B, H, W);
  RAFT_REQUIRE(frame_dtype == RAFT_FRAME_F32_NCHW || frame_dtype == RAFT_FRAME_U8_NHWC,
               "raft_warp_frame: unknown frame dtype tag %d", frame_dtype);
  RAFT_REQUIRE(out_dtype == RAFT_FRAME_F32_NCHW || out_dtype == RAFT_FRAME_U8_NHWC,
               "raft_warp_frame: unknown output dtype tag %d", out_dtype);
  RAFT_REQUIRE((flags & ~RAFT_WARP_BORDER) == 0, "raft_warp_frame: unknown flags %d", flags);
  const bool in_u8 = frame_dtype == RAFT_FRAME_U8_NHWC, out_u8 = out_dtype == RAFT_FRAME_U8_NHWC;
  RAFT_REQUIRE(C >= 1 && (long)B * C * H * W < (1L << 40), "raft_warp_frame: bad channel count %d", C);
  RAFT_REQUIRE(!(in_u8 || out_u8) || C == 3, "raft_warp_frame: a uint8 frame has 3 channels, got C = %d", C);
  RAFT_REQUIRE(top >= 0 && left >= 0, "raft_warp_frame: negative crop offset");
  RAFT_REQUIRE(flow_pitch >= (long)left + W && flow_batch_stride >= 0 && flow_chan_stride >= 0,
               "raft_warp_frame: bad strides (a row pitch holds left + W floats; strides are not negative)");
  RAFT_REQUIRE(in_u8 || (frame_pitch >= (long)left + W && frame_batch_stride >= 0 && frame_chan_stride >= 0),
               "raft_warp_frame: bad frame strides (a row pitch holds left + W floats; strides are not negative)");
  RAFT_REQUIRE(((uintptr_t)flow & 3) == 0 && (in_u8 || ((uintptr_t)frame & 3) == 0) &&
                   ((uintptr_t)out & (out_u8 ? 3 : 15)) == 0 && ((uintptr_t)valid & 3) == 0,
               "raft_warp_frame: misaligned pointer (flow 4, float32 frame 4, float32 out 16, uint8 out 4, valid 4 "
               "bytes)");
  RAFT_REQUIRE((const void*)out != (const void*)flow && (const void*)out != frame && (const void*)valid != out &&
                   (const void*)valid != (const void*)flow && (const void*)valid != frame,
               "raft_warp_frame: an output aliases an input or the other output");
  WarpArgs a;
  a.flow = flow + (long)top * flow_pitch + left;
  a.fsb = flow_batch_stride;
  a.fsc = flow_chan_stride;
  a.fpitch = flow_pitch;
  a.img = in_u8 ? frame : (const void*)(static_cast<const float*>(frame) + (long)top * frame_pitch + left);
  a.isb = frame_batch_stride;
  a.isc = frame_chan_stride;
  a.ipitch = frame_pitch;
  a.out = out;
  a.valid = valid;
  a.B = B;
  a.C = C;
  a.H = H;
  a.W = W;
  a.border = (flags & RAFT_WARP_BORDER) ? 1 : 0;
  const dim3 grid(grid_for(((long)B * H * W + 3) / 4)), block(256);
  hipStream_t s = as_stream(stream);
  if (in_u8 && out_u8)
    hipLaunchKernelGGL((warp_frame_kernel<true, true>), grid, block, 0, s, a);
  else if (in_u8)
    hipLaunchKernelGGL((warp_frame_kernel<true, false>), grid, block, 0, s, a);
  else if (out_u8)
    hipLaunchKernelGGL((warp_frame_kernel<false, true>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((warp_frame_kernel<false, false>), grid, block, 0, s, a);
  return check_launch("raft_warp_frame");
}

extern "C" size_t raft_splat_ws_bytes(int B, int H, int W) {
  if (!size_ok(B, H, W)) return 0;
  return (size_t)B * H * W * sizeof(unsigned long long);
}

extern "C" int raft_splat_density(const float* flow, long batch_stride, long chan_stride, long pitch, int top, int left,
                                  int B, int H, int W, void* ws, float* density, raft_stream_t stream) {
  RAFT_REQUIRE(flow && ws && density, "raft_splat_density: null pointer");
  RAFT_REQUIRE(size_ok(B, H, W), "raft_splat_density: bad size %d x %d x %d", B, H, W);
  RAFT_REQUIRE(top >= 0 && left >= 0, "raft_splat_density: negative crop offset");
  RAFT_REQUIRE(pitch >= (long)left + W && batch_stride >= 0 && chan_stride >= 0,
               "raft_splat_density: bad strides (a row pitch holds left + W floats; strides are not negative)");
  RAFT_REQUIRE(((uintptr_t)flow & 3) == 0 && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)density & 3) == 0,
               "raft_splat_density: misaligned pointer (flow 4, ws 8, density 4 bytes)");
  RAFT_REQUIRE((const void*)density != (const void*)flow && (const void*)density != (const void*)ws &&
                   (const void*)ws != (const void*)flow,
               "raft_splat_density: density (or ws) aliases an input");
  SplatArgs a;
  a.flow = flow + (long)top * pitch + left;
  a.fsb = batch_stride;
  a.fsc = chan_stride;
  a.fpitch = pitch;
  a.ws = static_cast<unsigned long long*>(ws);
  a.density = density;
  a.B = B;
  a.H = H;
  a.W = W;
  const long n = (long)B * H * W;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(splat_zero_kernel, dim3(grid_for(n)), dim3(256), 0, s, a);
  int rc = check_launch("raft_splat_density (zero)");
  if (rc) return rc;
  hipLaunchKernelGGL(splat_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, s, a);
  rc = check_launch("raft_splat_density (splat)");
  if (rc) return rc;
  hipLaunchKernelGGL(splat_convert_kernel, dim3(grid_for(n)), dim3(256), 0, s, a);
  return check_launch("raft_splat_density");
}
