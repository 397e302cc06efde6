// Flow colour-wheel visualisation (gfx950): core/utils/flow_viz.py on the device.
//
//   raft_flow_viz_ws_bytes   size of the partial-maxima workspace
//   raft_flow_to_rgb         flow [B,2,H,W] (a crop of a pitched buffer) -> uint8 [B][H][W][3], optionally
//                            stacked under a frame; one or two launches
//
// The definition is in raft_hip.h.  Two kernels:
//
//   viz_max_kernel     grid (NP, B): work-group (p, b) takes every NP-th run of 256 x 4 pixels of image b and
//                      writes its maximum of sqrt(u^2 + v^2) to ws[b * NP + p].  NP = viz_partials(H, W) <= 256.
//                      Every slot is written on every call (0 where a work-group has no pixel), so the workspace
//                      needs no initialisation, and a maximum is exact whatever the order: replays agree bit
//                      for bit.  No atomics.
//   viz_colour_kernel  a work-group owns 1024 consecutive pixels of the OUTPUT.  It first reduces the NP partials
//                      of each image those pixels belong to (one wave per image, one shuffle tree; nearly always
//                      one image) into LDS, then colours.  With a fixed scale the first kernel is not launched.
//
// Thread-to-pixel map: a thread owns 4 consecutive pixels of the flat output [B * Hout * W], that is 12
// consecutive bytes at a 4-byte aligned address whatever W is: three dword stores, and a wave covers 768
// contiguous bytes.  No byte stores but in the last group of the buffer.  Where the four pixels lie in one row
// and the address is 16-byte aligned (always at W % 4 == 0 with an aligned pitch and crop) the u and v planes are
// read with one 16-byte load each; otherwise (odd widths, crops at odd offsets, groups that wrap to the next
// row or image) pixel by pixel.  Traffic per pixel: 8 B read twice (maximum, colour) and 3 B written.
//
// The wheel is a compile-time table, already divided by 255; a work-group copies it to LDS, where the per-lane
// lookups (two entries per pixel) are 16-byte reads.
#include "common.hpp"

#include <cmath>
#include <cstdint>

namespace raft {
namespace {

constexpr int kWheelN = 55;

struct alignas(16) Wheel {
  float c[kWheelN][4];   // R, G, B (each / 255), pad
};

// The Middlebury wheel from its definition (raft_hip.h): six segments, one channel moving in each.
constexpr Wheel make_wheel() {
  Wheel w{};
  const int seg_n[6] = {15, 6, 4, 11, 13, 6};
  // first colour of each segment, the moving channel and its direction
  const int start[6][3] = {{255, 0, 0}, {255, 255, 0}, {0, 255, 0}, {0, 255, 255}, {0, 0, 255}, {255, 0, 255}};
  const int chan[6] = {1, 0, 2, 1, 0, 2};
  const int sign[6] = {1, -1, 1, -1, 1, -1};
  int k = 0;
  for (int s = 0; s < 6; ++s)
    for (int i = 0; i < seg_n[s]; ++i, ++k) {
      int rgb[3] = {start[s][0], start[s][1], start[s][2]};
      rgb[chan[s]] += sign[s] * ((255 * i) / seg_n[s]);
      for (int c = 0; c < 3; ++c) w.c[k][c] = (float)rgb[c] / 255.0f;
      w.c[k][3] = 0.0f;
    }
  return w;
}

__device__ const Wheel kWheel = make_wheel();

struct VizArgs {
  const float* flow;        // element (b = 0, c = 0, y = 0, x = 0) of the CROP
  long sb, sc, pitch;       // in floats
  const float* frame;       // likewise, or null
  long fsb, fsc, fpitch;
  float* ws;                // [B][np]
  unsigned char* out;
  int B, H, W, Hout, np;
  float clip, fixed;
  int flags;
};

// NP of the header comment: work-groups (and partial maxima) per image
__host__ __device__ inline int viz_partials(long hw) {
  const long runs = (hw + 1023) / 1024;
  return (int)(runs < 1 ? 1 : runs > 256 ? 256 : runs);
}

__device__ __forceinline__ float viz_clip(float x, float c) { return x < 0.0f ? 0.0f : (x > c ? c : x); }  // NaN stays

__device__ __forceinline__ bool viz_finite(float x) { return fabsf(x) < INFINITY; }

// 4 floats of one row: one 16-byte load where the address allows it
__device__ __forceinline__ void load_run(const float* p, float (&o)[4]) {
  if ((((uintptr_t)p) & 15) == 0) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = v[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = p[k];
  }
}

__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  return m;
}

__global__ __launch_bounds__(256) void viz_max_kernel(VizArgs a) {
#pragma clang fp contract(off)
  __shared__ float s_m[4];
  const long HW = (long)a.H * a.W;
  const long groups = (HW + 3) >> 2;
  const bool clip = a.flags & RAFT_VIZ_CLIP;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {   // (gridDim.y = B up to the grid's limit)
    const float* f0 = a.flow + (long)b * a.sb;
    float m = 0.0f;
    for (long g = blockIdx.x * 256L + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
      const long r0 = g << 2;
      const int cnt = (int)(HW - r0 < 4 ? HW - r0 : 4);
      int y = (int)(r0 / a.W), x = (int)(r0 - (long)y * a.W);
      float u[4], v[4];
      if (cnt == 4 && x + 3 < a.W) {
        const float* pu = f0 + (long)y * a.pitch + x;
        load_run(pu, u);
        load_run(pu + a.sc, v);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < cnt) {
            const float* q = f0 + (long)y * a.pitch + x;
            u[k] = q[0];
            v[k] = q[a.sc];
            if (++x == a.W) {
              x = 0;
              ++y;
            }
          } else {
            u[k] = v[k] = 0.0f;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float uu = u[k], vv = v[k];
        if (clip) {
          uu = viz_clip(uu, a.clip);
          vv = viz_clip(vv, a.clip);
        }
        if (viz_finite(uu) && viz_finite(vv)) m = fmaxf(m, sqrtf(uu * uu + vv * vv));
      }
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) a.ws[(long)b * a.np + blockIdx.x] = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
    __syncthreads();
  }
}

// one flow vector -> three bytes (R, G, B); den = rad_max + 1e-5f, or 1 with RAFT_VIZ_UNIT
__device__ __forceinline__ void colour_pixel(float u, float v, float den, bool clip, float clip_to,
                                             const float (*wheel)[4], unsigned char (&px)[3]) {
#pragma clang fp contract(off)
  if (clip) {
    u = viz_clip(u, clip_to);
    v = viz_clip(v, clip_to);
  }
  if (!(viz_finite(u) && viz_finite(v))) {
    px[0] = px[1] = px[2] = 0;
    return;
  }
  u = u / den;
  v = v / den;
  const float rad = sqrtf(u * u + v * v);
  const float ang = atan2f(-v, -u) / 3.14159265358979323846f;
  const float fk = (ang + 1.0f) / 2.0f * (float)(kWheelN - 1);
  int k0 = (int)floorf(fk);
  k0 = k0 < 0 ? 0 : k0 > kWheelN - 1 ? kWheelN - 1 : k0;
  const int k1 = k0 + 1 == kWheelN ? 0 : k0 + 1;
  const float f = fk - (float)k0;
  const f32x4 c0 = *reinterpret_cast<const f32x4*>(wheel[k0]);
  const f32x4 c1 = *reinterpret_cast<const f32x4*>(wheel[k1]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float col = (1.0f - f) * c0[c] + f * c1[c];
    col = rad <= 1.0f ? 1.0f - rad * (1.0f - col) : 0.75f * col;
    const float q = floorf(255.0f * col);
    px[c] = (unsigned char)(q < 0.0f ? 0.0f : q > 255.0f ? 255.0f : q);   // (in range by construction)
  }
}

// one frame value -> its byte: nearest (ties to even), saturated, NaN -> 0
__device__ __forceinline__ unsigned char frame_byte(float x) {
  return (unsigned char)rintf(fminf(fmaxf(x, 0.0f), 255.0f));
}

__global__ __launch_bounds__(256) void viz_colour_kernel(VizArgs a) {
  __shared__ __attribute__((aligned(16))) float s_wheel[kWheelN][4];
  __shared__ float s_den[1024];   // rad_max + 1e-5f of the images this work-group's pixels lie in
  const int tid = threadIdx.x;
  if (tid < kWheelN) *reinterpret_cast<f32x4*>(s_wheel[tid]) = *reinterpret_cast<const f32x4*>(kWheel.c[tid]);
  const long per = (long)a.Hout * a.W;           // output pixels per image
  const long n = (long)a.B * per;
  const long o_lo = blockIdx.x * 1024L;
  const long o_hi = o_lo + 1023 < n - 1 ? o_lo + 1023 : n - 1;
  const int b_lo = (int)(o_lo / per), b_hi = (int)(o_hi / per);
  const bool unit = a.flags & RAFT_VIZ_UNIT, clip = a.flags & RAFT_VIZ_CLIP, bgr = a.flags & RAFT_VIZ_BGR;
  const bool own_max = !unit && !(a.fixed > 0.0f);
  if (own_max) {
    for (int k = tid >> 6; k <= b_hi - b_lo; k += 4) {
      const float* part = a.ws + (long)(b_lo + k) * a.np;
      float m = 0.0f;
      for (int p = tid & 63; p < a.np; p += 64) m = fmaxf(m, part[p]);
      m = wave_max(m);
      if ((tid & 63) == 0) s_den[k] = m + 1e-5f;
    }
  }
  __syncthreads();
  const float den_all = unit ? 1.0f : a.fixed + 1e-5f;

  const long o0 = o_lo + 4L * tid;
  if (o0 >= n) return;
  const int cnt = (int)(n - o0 < 4 ? n - o0 : 4);
  int b = (int)(o0 / per);
  const long r = o0 - (long)b * per;
  int yo = (int)(r / a.W), x = (int)(r - (long)yo * a.W);
  unsigned char px[4][3];
  if (cnt == 4 && x + 3 < a.W) {
    if (a.frame && yo < a.H) {
      const float* q = a.frame + (long)b * a.fsb + (long)yo * a.fpitch + x;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float t[4];
        load_run(q + c * a.fsc, t);
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k][c] = frame_byte(t[k]);
      }
    } else {
      const int y = a.frame ? yo - a.H : yo;
      const float* pu = a.flow + (long)b * a.sb + (long)y * a.pitch + x;
      float u[4], v[4];
      load_run(pu, u);
      load_run(pu + a.sc, v);
      const float den = own_max ? s_den[b - b_lo] : den_all;
#pragma unroll
      for (int k = 0; k < 4; ++k) colour_pixel(u[k], v[k], den, clip, a.clip, s_wheel, px[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < cnt) {
        if (a.frame && yo < a.H) {
          const float* q = a.frame + (long)b * a.fsb + (long)yo * a.fpitch + x;
#pragma unroll
          for (int c = 0; c < 3; ++c) px[k][c] = frame_byte(q[c * a.fsc]);
        } else {
          const int y = a.frame ? yo - a.H : yo;
          const float* q = a.flow + (long)b * a.sb + (long)y * a.pitch + x;
          colour_pixel(q[0], q[a.sc], own_max ? s_den[b - b_lo] : den_all, clip, a.clip, s_wheel, px[k]);
        }
        if (++x == a.W) {
          x = 0;
          if (++yo == a.Hout) {
            yo = 0;
            ++b;
          }
        }
      } else {
        px[k][0] = px[k][1] = px[k][2] = 0;
      }
    }
  }
  unsigned char by[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    by[3 * k + 0] = bgr ? px[k][2] : px[k][0];
    by[3 * k + 1] = px[k][1];
    by[3 * k + 2] = bgr ? px[k][0] : px[k][2];
  }
  unsigned char* o = a.out + 3 * o0;
  if (cnt == 4) {
    // 3 * o0 = 12 * (o0 / 4) and the base is 4-byte aligned (host check)
    uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o32[j] = (uint32_t)by[4 * j] | ((uint32_t)by[4 * j + 1] << 8) | ((uint32_t)by[4 * j + 2] << 16) |
               ((uint32_t)by[4 * j + 3] << 24);
  } else {
    for (int j = 0; j < 3 * cnt; ++j) o[j] = by[j];
  }
}

bool viz_size_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 30); }

}  // namespace
}  // namespace raft

using namespace raft;

extern "C" size_t raft_flow_viz_ws_bytes(int B, int H, int W) {
  if (!viz_size_ok(B, H, W)) return 0;
  return (size_t)B * viz_partials((long)H * W) * sizeof(float);
}

extern "C" int raft_flow_to_rgb(const float* flow, long batch_stride, long chan_stride, long pitch, int top, int left,
                                int B, int H, int W, float clip_flow, float fixed_rad_max, int flags,
                                const float* frame, long frame_batch_stride, long frame_chan_stride, long frame_pitch,
                                float* ws, unsigned char* out, raft_stream_t stream) {
  RAFT_REQUIRE(flow && out, "raft_flow_to_rgb: null pointer");
  RAFT_REQUIRE(viz_size_ok(B, H, W), "raft_flow_to_rgb: bad size %d x %d x %d", B, H, W);
  RAFT_REQUIRE(top >= 0 && left >= 0, "raft_flow_to_rgb: negative crop offset");
  RAFT_REQUIRE((flags & ~(RAFT_VIZ_BGR | RAFT_VIZ_UNIT | RAFT_VIZ_CLIP)) == 0, "raft_flow_to_rgb: unknown flags %d",
               flags);
  RAFT_REQUIRE(pitch >= (long)left + W && batch_stride >= 0 && chan_stride >= 0,
               "raft_flow_to_rgb: bad strides (a row pitch holds left + W floats; strides are not negative)");
  RAFT_REQUIRE(!frame || (frame_pitch >= (long)left + W && frame_batch_stride >= 0 && frame_chan_stride >= 0),
               "raft_flow_to_rgb: bad frame strides (a row pitch holds left + W floats; strides are not negative)");
  RAFT_REQUIRE(!std::isnan(fixed_rad_max) && fixed_rad_max >= 0.f && !std::isinf(fixed_rad_max),
               "raft_flow_to_rgb: fixed_rad_max must be finite and not negative (0: each image's own maximum)");
  RAFT_REQUIRE(!std::isnan(clip_flow) && clip_flow >= 0.f, "raft_flow_to_rgb: clip_flow must not be negative or NaN");
  const bool own_max = !(flags & RAFT_VIZ_UNIT) && !(fixed_rad_max > 0.f);
  RAFT_REQUIRE(!own_max || ws, "raft_flow_to_rgb: null workspace (needed without a fixed scale)");
  RAFT_REQUIRE((((uintptr_t)flow | (uintptr_t)frame | (uintptr_t)ws | (uintptr_t)out) & 3) == 0,
               "raft_flow_to_rgb: misaligned pointer (4 bytes)");
  RAFT_REQUIRE((const void*)out != (const void*)flow && (const void*)out != (const void*)frame &&
                   (const void*)out != (const void*)ws && (const void*)ws != (const void*)flow,
               "raft_flow_to_rgb: out (or ws) aliases an input");
  VizArgs a;
  a.flow = flow + (long)top * pitch + left;
  a.sb = batch_stride;
  a.sc = chan_stride;
  a.pitch = pitch;
  a.frame = frame ? frame + (long)top * frame_pitch + left : nullptr;
  a.fsb = frame_batch_stride;
  a.fsc = frame_chan_stride;
  a.fpitch = frame_pitch;
  a.ws = ws;
  a.out = out;
  a.B = B;
  a.H = H;
  a.W = W;
  a.Hout = frame ? 2 * H : H;
  a.np = viz_partials((long)H * W);
  a.clip = clip_flow;
  a.fixed = (flags & RAFT_VIZ_UNIT) ? 0.f : fixed_rad_max;
  a.flags = flags;
  if (own_max) {
    hipLaunchKernelGGL(viz_max_kernel, dim3(a.np, B < 65535 ? B : 65535), dim3(256), 0, as_stream(stream), a);
    const int rc = check_launch("raft_flow_to_rgb (maximum)");
    if (rc) return rc;
  }
  const long groups = ((long)B * a.Hout * W + 3) / 4;
  hipLaunchKernelGGL(viz_colour_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, as_stream(stream), a);
  return check_launch("raft_flow_to_rgb");
}
