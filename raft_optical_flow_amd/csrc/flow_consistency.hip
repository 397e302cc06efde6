// Forward-backward consistency of a flow pair and the bidirectional stream's carry (gfx950).
//
//   raft_fb_consistency   occlusion masks + squared residuals of both directions, one launch
//   raft_stream_carry_n   up to RAFT_CARRY_MAX_SEGS pitched 2-D device copies in one launch
//
// The check (definition: raft_hip.h).  For direction fw at pixel x = (j, i) of the H x W frame,
// F = flow_fw, G = flow_bw:  p = x + F(x).  p not finite or outside [0, W-1] x [0, H-1]:
// err = +inf, occ = 1.  Otherwise g = bilinear G(p), err = |F(x) + g|^2,
// occ = err > alpha (|F(x)|^2 + |g|^2) + beta.  Direction bw: F and G swapped.
//
// Sampling position: j is an integer, so floor(j + Fx) = j + floor(Fx) exactly, and the fractional
// weight is Fx - floor(Fx): exact in fp32 except for Fx in (-1, 0), where 1 + Fx rounds once
// (<= 2^-25).  The sum j + Fx, whose rounding would grow with the frame's width, is never formed,
// and the frame test is an integer comparison.  The other roundings are those of the bilinear blend
// and of err / the threshold (contraction off: one rounding per written operation, which is what
// the error bound of tests/test_bidi_host.py counts).
//
// Memory: per pixel and direction 8 B of F, 4 taps x 2 channels of G (neighbouring pixels share
// them through L1/L2; the algorithmic traffic is the 8 B of the G plane), 4 B err, 1 B occ.
// A thread owns 4 consecutive elements of the flat [B*H*W] output of its direction, so the err
// store is one 16-byte and the occ store one 4-byte access whatever W is; the F loads are 16-byte
// where the four pixels share a row and the address is aligned (always at W % 4 == 0 with an
// aligned pitch and crop, e.g. 436 x 1024 in a 440 x 1024 buffer), scalar otherwise (odd frame
// sizes, crops at odd offsets).  A wave covers 256 consecutive output elements: x-runs of rows.
#include "common.hpp"

#include <cmath>
#include <cstdint>

namespace raft {
namespace {

struct FlowView {
  const float* p;   // element (b = 0, c = 0, y = 0, x = 0) of the CROP
  long sb, sc;      // batch / channel stride in floats
  long pitch;       // row pitch in floats
};

struct FbArgs {
  FlowView f[2];            // [0] = flow_fw, [1] = flow_bw
  unsigned char* occ[2];    // [B*H*W] each
  float* err[2];
  int B, H, W;
  float alpha, beta;
};

// One axis: integer base and fractional weight of j + d; false when j + d leaves [0, n-1] (or d is
// not finite).  On true: 0 <= i0 <= n-1, and i0 == n-1 only with t == 0.
__device__ __forceinline__ bool fb_axis(int j, float d, int n, int& i0, float& t) {
  if (!(fabsf(d) < 1073741824.0f)) return false;  // NaN, inf, or beyond any frame
  const float fl = floorf(d);
  t = d - fl;             // exact, but for d in (-1, 0): one rounding
  i0 = j + (int)fl;       // exact (|fl| < 2^30, j < 2^30)
  return i0 >= 0 && (i0 < n - 1 || (i0 == n - 1 && t == 0.0f));
}

__device__ __forceinline__ void fb_pixel(const FbArgs& a, const FlowView& g, int b, int y, int x, float fx, float fy,
                                         float& err, unsigned char& occ) {
#pragma clang fp contract(off)
  int x0, y0;
  float ax, ay;
  const bool inx = fb_axis(x, fx, a.W, x0, ax), iny = fb_axis(y, fy, a.H, y0, ay);
  if (!(inx && iny)) {
    err = INFINITY;
    occ = 1;
    return;
  }
  // the +1 corners: read from a clamped (in-frame) address, dropped where they are outside
  const bool x1ok = x0 + 1 <= a.W - 1, y1ok = y0 + 1 <= a.H - 1;
  const int x1 = x1ok ? x0 + 1 : x0, y1 = y1ok ? y0 + 1 : y0;
  const float* g0 = g.p + (long)b * g.sb;
  const long r0 = (long)y0 * g.pitch, r1 = (long)y1 * g.pitch;
  const float wx0 = 1.0f - ax, wy0 = 1.0f - ay;
  float gv[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float* gc = g0 + (long)c * g.sc;
    const float v00 = gc[r0 + x0];
    const float v01 = x1ok ? gc[r0 + x1] : 0.0f;
    const float v10 = y1ok ? gc[r1 + x0] : 0.0f;
    const float v11 = (x1ok && y1ok) ? gc[r1 + x1] : 0.0f;
    const float top = wx0 * v00 + ax * v01;
    const float bot = wx0 * v10 + ax * v11;
    gv[c] = wy0 * top + ay * bot;
  }
  const float sx = fx + gv[0], sy = fy + gv[1];
  err = sx * sx + sy * sy;
  const float thr = a.alpha * ((fx * fx + fy * fy) + (gv[0] * gv[0] + gv[1] * gv[1])) + a.beta;
  // err > thr for finite values; a non-finite err (a NaN or inf flow reached it) is occluded
  occ = (err <= thr && err < INFINITY) ? 0 : 1;
}

__global__ __launch_bounds__(256) void fb_consistency_kernel(FbArgs a) {
  const long n = (long)a.B * a.H * a.W;   // elements per direction (< 2^30: checked on the host)
  const long groups = (n + 3) >> 2;
  const long HW = (long)a.H * a.W;
  for (long gi = blockIdx.x * (long)blockDim.x + threadIdx.x; gi < 2 * groups; gi += (long)gridDim.x * blockDim.x) {
    const int d = gi >= groups ? 1 : 0;
    const long e0 = (gi - (d ? groups : 0)) << 2;
    int b = (int)(e0 / HW);
    const int r = (int)(e0 - (long)b * HW);
    int y = r / a.W, x = r - y * a.W;
    const FlowView f = d ? a.f[1] : a.f[0];   // the direction's own flow
    const FlowView g = d ? a.f[0] : a.f[1];   // the flow it is checked against
    float fx[4], fy[4], err[4];
    unsigned char occ[4];
    const int cnt = (int)(n - e0 < 4 ? n - e0 : 4);
    const float* px = f.p + (long)b * f.sb + (long)y * f.pitch + x;
    const float* py = px + f.sc;
    if (cnt == 4 && x + 3 < a.W && ((((uintptr_t)px) | ((uintptr_t)py)) & 15) == 0) {
      const f32x4 vx = *reinterpret_cast<const f32x4*>(px);
      const f32x4 vy = *reinterpret_cast<const f32x4*>(py);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        fx[k] = vx[k];
        fy[k] = vy[k];
        fb_pixel(a, g, b, y, x + k, fx[k], fy[k], err[k], occ[k]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < cnt) {
          const float* q = f.p + (long)b * f.sb + (long)y * f.pitch + x;
          fb_pixel(a, g, b, y, x, q[0], q[f.sc], err[k], occ[k]);
          if (++x == a.W) {
            x = 0;
            if (++y == a.H) {
              y = 0;
              ++b;
            }
          }
        } else {
          err[k] = 0.0f;
          occ[k] = 0;
        }
      }
    }
    float* eo = (d ? a.err[1] : a.err[0]) + e0;
    unsigned char* oo = (d ? a.occ[1] : a.occ[0]) + e0;
    if (cnt == 4) {
      // e0 % 4 == 0 and the output bases are 16-byte (err) / 4-byte (occ) aligned (host check)
      f32x4 ev;
#pragma unroll
      for (int k = 0; k < 4; ++k) ev[k] = err[k];
      *reinterpret_cast<f32x4*>(eo) = ev;
      *reinterpret_cast<uint32_t*>(oo) =
          (uint32_t)occ[0] | ((uint32_t)occ[1] << 8) | ((uint32_t)occ[2] << 16) | ((uint32_t)occ[3] << 24);
    } else {
      for (int k = 0; k < cnt; ++k) {
        eo[k] = err[k];
        oo[k] = occ[k];
      }
    }
  }
}

// pitched 2-D copies in one launch: segment k is rows[k] x cols[k] elements of T
struct CarryNArgs {
  const void* src[RAFT_CARRY_MAX_SEGS];
  void* dst[RAFT_CARRY_MAX_SEGS];
  long src_ld[RAFT_CARRY_MAX_SEGS], dst_ld[RAFT_CARRY_MAX_SEGS], cols[RAFT_CARRY_MAX_SEGS];
  long end[RAFT_CARRY_MAX_SEGS];  // running total of rows * cols (the total from the last segment on)
};

template <typename T>
__global__ __launch_bounds__(256) void stream_carry_n_kernel(CarryNArgs a) {
  const long total = a.end[RAFT_CARRY_MAX_SEGS - 1];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    // the segment of element i, by selects (end[] does not decrease, and end[k] = total from n - 1 on)
    const void* src = a.src[0];
    void* dst = a.dst[0];
    long sld = a.src_ld[0], dld = a.dst_ld[0], cols = a.cols[0], lo = 0;
#pragma unroll
    for (int k = 1; k < RAFT_CARRY_MAX_SEGS; ++k)
      if (i >= a.end[k - 1]) {
        src = a.src[k];
        dst = a.dst[k];
        sld = a.src_ld[k];
        dld = a.dst_ld[k];
        cols = a.cols[k];
        lo = a.end[k - 1];
      }
    const long j = i - lo;
    const long r = j / cols, c = j - r * cols;
    static_cast<T*>(dst)[r * dld + c] = static_cast<const T*>(src)[r * sld + c];
  }
}

}  // namespace
}  // namespace raft

using namespace raft;

extern "C" int raft_fb_consistency(const float* flow_fw, long fw_batch_stride, long fw_chan_stride, long fw_pitch,
                                   const float* flow_bw, long bw_batch_stride, long bw_chan_stride, long bw_pitch,
                                   int top, int left, int B, int H, int W, float alpha, float beta,
                                   unsigned char* occ_fw, unsigned char* occ_bw, float* err_fw, float* err_bw,
                                   raft_stream_t stream) {
  RAFT_REQUIRE(flow_fw && flow_bw && occ_fw && occ_bw && err_fw && err_bw, "raft_fb_consistency: null pointer");
  RAFT_REQUIRE(size_ok(B, H, W), "raft_fb_consistency: bad size %d x %d x %d", B, H, W);
  RAFT_REQUIRE(top >= 0 && left >= 0, "raft_fb_consistency: negative crop offset");
  RAFT_REQUIRE(fw_pitch >= (long)left + W && bw_pitch >= (long)left + W && fw_batch_stride >= 0 &&
                   bw_batch_stride >= 0 && fw_chan_stride >= 0 && bw_chan_stride >= 0,
               "raft_fb_consistency: bad strides (a row pitch holds left + W floats; strides are not negative)");
  RAFT_REQUIRE(std::isfinite(alpha) && std::isfinite(beta) && alpha >= 0.f && beta >= 0.f,
               "raft_fb_consistency: alpha and beta must be finite and not negative");
  RAFT_REQUIRE((((uintptr_t)flow_fw | (uintptr_t)flow_bw) & 3) == 0 &&
                   (((uintptr_t)err_fw | (uintptr_t)err_bw) & 15) == 0 &&
                   (((uintptr_t)occ_fw | (uintptr_t)occ_bw) & 3) == 0,
               "raft_fb_consistency: misaligned pointer (flows 4, err 16, occ 4 bytes)");
  RAFT_REQUIRE(occ_fw != occ_bw && err_fw != err_bw, "raft_fb_consistency: the two directions share an output");
  FbArgs a;
  const long off = (long)top;
  a.f[0] = {flow_fw + off * fw_pitch + left, fw_batch_stride, fw_chan_stride, fw_pitch};
  a.f[1] = {flow_bw + off * bw_pitch + left, bw_batch_stride, bw_chan_stride, bw_pitch};
  a.occ[0] = occ_fw;
  a.occ[1] = occ_bw;
  a.err[0] = err_fw;
  a.err[1] = err_bw;
  a.B = B;
  a.H = H;
  a.W = W;
  a.alpha = alpha;
  a.beta = beta;
  const long groups = ((long)B * H * W + 3) / 4;
  hipLaunchKernelGGL(fb_consistency_kernel, dim3(grid_for(2 * groups)), dim3(256), 0, as_stream(stream), a);
  return check_launch("raft_fb_consistency");
}

extern "C" int raft_stream_carry_n(const raft_copy2d* segs, int n, raft_stream_t stream) {
  RAFT_REQUIRE(segs, "raft_stream_carry_n: null pointer");
  RAFT_REQUIRE(n > 0 && n <= RAFT_CARRY_MAX_SEGS, "raft_stream_carry_n: %d segments (1..%d)", n, RAFT_CARRY_MAX_SEGS);
  CarryNArgs a;
  bool vec = true;
  long total = 0;
  for (int k = 0; k < n; ++k) {
    const raft_copy2d& s = segs[k];
    RAFT_REQUIRE(s.src && s.dst, "raft_stream_carry_n: null pointer in segment %d", k);
    RAFT_REQUIRE(s.rows > 0 && s.cols > 0 && s.rows < (1L << 40) && s.cols < (1L << 40) &&
                     s.rows <= (1L << 40) / s.cols && s.src_ld >= s.cols && s.dst_ld >= s.cols,
                 "raft_stream_carry_n: bad size in segment %d", k);
    RAFT_REQUIRE((const void*)s.src != (const void*)s.dst, "raft_stream_carry_n: in-place is not supported");
    vec = vec && s.cols % 4 == 0 && s.src_ld % 4 == 0 && s.dst_ld % 4 == 0 &&
          (((uintptr_t)s.src | (uintptr_t)s.dst) & 15) == 0;
    a.src[k] = s.src;
    a.dst[k] = s.dst;
    a.src_ld[k] = s.src_ld;
    a.dst_ld[k] = s.dst_ld;
    a.cols[k] = s.cols;
    total += s.rows * s.cols;
    a.end[k] = total;
  }
  for (int k = n; k < RAFT_CARRY_MAX_SEGS; ++k) {
    a.src[k] = nullptr;
    a.dst[k] = nullptr;
    a.src_ld[k] = a.dst_ld[k] = a.cols[k] = 1;
    a.end[k] = total;
  }
  if (vec) {
    for (int k = 0; k < RAFT_CARRY_MAX_SEGS; ++k) {
      if (k < n) {
        a.src_ld[k] /= 4;
        a.dst_ld[k] /= 4;
        a.cols[k] /= 4;
      }
      a.end[k] /= 4;
    }
    hipLaunchKernelGGL(stream_carry_n_kernel<f32x4>, dim3(grid_for(total / 4)), dim3(256), 0, as_stream(stream), a);
  } else {
    hipLaunchKernelGGL(stream_carry_n_kernel<float>, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), a);
  }
  return check_launch("raft_stream_carry_n");
}
