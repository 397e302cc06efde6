// The backward warp's per-pixel arithmetic (definition: raft_hip.h, raft_warp_frame), shared by flow_warp.hip
// (raft_warp_frame) and photo_metrics.hip (raft_photo_metrics), so that both produce the same bits: the taps
// of one output pixel, the frame test, the tap loads and the blend.
#pragma once

#include "common.hpp"

#include <cmath>
#include <cstdint>

namespace raft {
namespace {

struct WarpArgs {
  const float* flow;   // element (b = 0, c = 0, y = 0, x = 0) of the CROP
  long fsb, fsc, fpitch;
  const void* img;     // float32: element (0, 0, 0, 0) of the crop; uint8: the dense [B][H][W][3] base
  long isb, isc, ipitch;
  void* out;
  unsigned char* valid;
  int B, C, H, W;
  int border;
};

// The taps of one output pixel: clamped bases, weights, which of the four corners are read.
struct Taps {
  int x0, y0;
  float ax, ay;
  bool okx0, okx1, oky0, oky1;
  unsigned char valid;
};

// One axis.  |d| < 2^30 has been checked.  Returns whether j + d lies in [0, n-1] (fb_axis's test); i0 and
// t are the base and weight the blend uses (clamped in border mode), ok0 / ok1 whether taps i0 and i0 + 1
// lie in the crop.
__device__ __forceinline__ bool warp_axis(int j, float d, int n, bool border, int& i0, float& t, bool& ok0,
                                          bool& ok1) {
  const float fl = floorf(d);
  t = d - fl;             // exact, but for d in (-1, 0): one rounding
  i0 = j + (int)fl;       // exact (|fl| <= 2^30, j < 2^30)
  const bool inside = i0 >= 0 && (i0 < n - 1 || (i0 == n - 1 && t == 0.0f));
  if (border) {
    if (i0 < 0) {
      i0 = 0;
      t = 0.0f;
    } else if (i0 >= n - 1) {
      i0 = n - 1;
      t = 0.0f;
    }
  }
  ok0 = i0 >= 0 && i0 <= n - 1;
  ok1 = i0 >= -1 && i0 < n - 1;
  return inside;
}

__device__ __forceinline__ bool flow_ok(float d) { return fabsf(d) < 1073741824.0f; }  // not NaN, inf, huge

__device__ __forceinline__ Taps warp_taps(const WarpArgs& a, int y, int x, float fx, float fy) {
  Taps t;
  if (!(flow_ok(fx) && flow_ok(fy))) {
    t.x0 = t.y0 = 0;
    t.ax = t.ay = 0.0f;
    t.okx0 = t.okx1 = t.oky0 = t.oky1 = false;   // every tap 0: the output is 0
    t.valid = 0;
    return t;
  }
  const bool inx = warp_axis(x, fx, a.W, a.border, t.x0, t.ax, t.okx0, t.okx1);
  const bool iny = warp_axis(y, fy, a.H, a.border, t.y0, t.ay, t.oky0, t.oky1);
  t.valid = (inx && iny) ? 1 : 0;
  return t;
}

template <bool IN_U8>
__device__ __forceinline__ float warp_tap(const WarpArgs& a, int b, int c, int y, int x) {
  if (IN_U8) {
    const unsigned char* p = static_cast<const unsigned char*>(a.img);
    return (float)p[(((long)b * a.H + y) * a.W + x) * 3 + c];
  }
  const float* p = static_cast<const float*>(a.img);
  return p[(long)b * a.isb + (long)c * a.isc + (long)y * a.ipitch + x];
}

template <bool IN_U8>
__device__ __forceinline__ float warp_blend(const WarpArgs& a, const Taps& t, int b, int c) {
#pragma clang fp contract(off)
  const int x1 = t.x0 + 1, y1 = t.y0 + 1;
  const float v00 = (t.okx0 && t.oky0) ? warp_tap<IN_U8>(a, b, c, t.y0, t.x0) : 0.0f;
  const float v01 = (t.okx1 && t.oky0) ? warp_tap<IN_U8>(a, b, c, t.y0, x1) : 0.0f;
  const float v10 = (t.okx0 && t.oky1) ? warp_tap<IN_U8>(a, b, c, y1, t.x0) : 0.0f;
  const float v11 = (t.okx1 && t.oky1) ? warp_tap<IN_U8>(a, b, c, y1, x1) : 0.0f;
  const float wx0 = 1.0f - t.ax, wy0 = 1.0f - t.ay;
  const float top = wx0 * v00 + t.ax * v01;
  const float bot = wx0 * v10 + t.ax * v11;
  return wy0 * top + t.ay * bot;
}

}  // namespace
}  // namespace raft
