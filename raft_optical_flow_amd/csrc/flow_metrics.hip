// Scoring a flow against ground truth (gfx950): evaluate.py's validate_* arithmetic on the device.
//
//   raft_flow_metrics_ws_bytes  size of the partial-record workspace
//   raft_flow_metrics           flow, flow_gt [B,2,H,W] and an optional mask (all read in place through their
//                               strides) -> one record of 16 64-bit slots per sample, optionally added into
//                               running totals, optionally the per-pixel EPE map; two launches, no atomics
//
// The definition is in raft_hip.h.  metrics_partial_kernel, grid (NB, B), NB = metrics_blocks(H * W) <=
// RAFT_FLOW_METRICS_MAX_BLOCKS: a function of (H, W) only, never of the device.  Work-group (p, b) takes every
// NB-th run of 256 x 4 pixels of sample b (a work-group never spans two samples) and writes one partial record;
// record_common.hpp has the reduction from there (store_partial, record_finalize_kernel) and its fixed order.
//
// Rounding.  The per-pixel values are defined as IEEE fp32, every operation rounded to nearest and nothing
// fused.  hipcc's default -ffp-contract=fast fuses a * b + c across statements, so contraction is switched off
// for this whole file (the pragma below).  This toolchain's __fmul_rn / __fadd_rn are plain `*` / `+` (they
// would contract all the same) and its __fsqrt_rn is the native, not correctly rounded, square root, so they
// are NOT used: `sqrtf` and `/` are correctly rounded under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt, and tests/test_gpu_flow_metrics.py holds epe_map to the bits.
//
// Memory.  A thread owns 4 consecutive pixels of a sample's flat [H * W] order.  Where the four lie in one row
// and every operand of the group is aligned (the four planes 16 bytes, a float32 mask 16, a byte mask 4) the
// loads are one 16-byte load per plane; otherwise, and in the tail, pixel by pixel.  The epe_map store is 16
// bytes where the four pixels exist and the address allows it.  Traffic: 16 B per pixel read, plus the mask,
// plus 4 B written with epe_map.
#include "common.hpp"
#include "record_common.hpp"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace raft {
namespace {

constexpr int kSlots = RAFT_FLOW_METRICS_SLOTS;
constexpr int kBlockPixels = RAFT_FLOW_METRICS_BLOCK_PIXELS;   // 256 threads x 4 pixels
constexpr int kMaxBlocks = RAFT_FLOW_METRICS_MAX_BLOCKS;
static_assert(kBlockPixels == 1024 && kSlots == kRecordSlots, "the kernels below are written for these");

// 9 counts, no pixels slot, 4 sums; the per-image mean is EPE_SUM / N
using Layout = RecordLayout<9, -1, 4, RAFT_FM_EPE_SUM, RAFT_FM_N>;
static_assert(Layout::kFirstSum == RAFT_FM_EPE_SUM && Layout::kImages == RAFT_FM_IMAGES &&
                  Layout::kMeanSum == RAFT_FM_IMAGE_MEAN_SUM && Layout::kReserved == RAFT_FM_RESERVED &&
                  RAFT_FM_N == 0 && RAFT_FM_N_S40 == Layout::kSummed - 1 && RAFT_FM_EPE_SUM_S40 == RAFT_FM_IMAGES - 1,
              "the layout is raft_hip.h's");

struct MetricsArgs {
  const float* flow;      // element (b = 0, c = 0, y = 0, x = 0)
  long fsb, fsc, fpitch;  // in floats
  const float* gt;
  long gsb, gsc, gpitch;
  MaskView m;
  float limit;            // <= 0: absent
  long long* ws;          // [B][nb][16]
  float* epe_map;         // [B][H][W] or null
  int B, H, W, nb;
};

// NB of the header comment: work-groups (and partial records) per sample
__host__ __device__ inline int metrics_blocks(long hw) {
  const long runs = (hw + kBlockPixels - 1) / kBlockPixels;
  return (int)(runs < 1 ? 1 : runs > kMaxBlocks ? kMaxBlocks : runs);
}

struct Acc {
  unsigned n, nonfinite, lt1, lt3, lt5, outlier, s0, s1, s2;   // (a sample has fewer than 2^30 pixels)
  double sum, sum0, sum1, sum2;
};

__device__ __forceinline__ float canonical_nan() { return __uint_as_float(0x7fc00000u); }

// One pixel: counts it into a, returns the epe_map value.
__device__ __forceinline__ float metrics_pixel(float u, float v, float gu, float gv, bool valid, float limit, Acc& a) {
  if (limit > 0.0f) valid = valid && fabsf(gu) < limit && fabsf(gv) < limit;   // a NaN fails
  if (!valid) return canonical_nan();
  const float du = u - gu, dv = v - gv;
  const float epe = sqrtf(du * du + dv * dv);
  const float mag = sqrtf(gu * gu + gv * gv);
  const float ratio = epe / mag;
  ++a.n;
  if (!(fabsf(epe) < INFINITY)) {
    ++a.nonfinite;
    return epe != epe ? canonical_nan() : epe;
  }
  a.lt1 += epe < 1.0f;
  a.lt3 += epe < 3.0f;
  a.lt5 += epe < 5.0f;
  a.outlier += (epe > 3.0f && ratio > 0.05f);
  const double e = (double)epe;
  a.sum += e;
  if (mag < 10.0f) {
    ++a.s0;
    a.sum0 += e;
  } else if (mag < 40.0f) {
    ++a.s1;
    a.sum1 += e;
  } else {   // mag >= 40, inf included (mag is never NaN where epe is finite)
    ++a.s2;
    a.sum2 += e;
  }
  return epe;
}

__global__ __launch_bounds__(256) void metrics_partial_kernel(MetricsArgs a) {
  const long HW = (long)a.H * a.W;
  const long groups = (HW + 3) >> 2;
  const int wave = threadIdx.x >> 6;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {   // (gridDim.y = B up to the grid's limit)
    const float* f0 = a.flow + (long)b * a.fsb;
    const float* g0 = a.gt + (long)b * a.gsb;
    const long m0 = (long)b * a.m.sb;
    float* e0 = a.epe_map ? a.epe_map + (long)b * HW : nullptr;
    Acc acc = {};
    for (long g = blockIdx.x * 256L + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
      const long r0 = g << 2;
      const int cnt = (int)(HW - r0 < 4 ? HW - r0 : 4);
      int y = (int)(r0 / a.W), x = (int)(r0 - (long)y * a.W);
      float ev[4];
      bool vector = cnt == 4 && x + 3 < a.W;
      const float* pu = f0 + (long)y * a.fpitch + x;
      const float* pg = g0 + (long)y * a.gpitch + x;
      const long mo = m0 + (long)y * a.m.pitch + x;
      if (vector) {
        uintptr_t bits = (uintptr_t)pu | (uintptr_t)(pu + a.fsc) | (uintptr_t)pg | (uintptr_t)(pg + a.gsc);
        if (a.m.p)
          bits |= a.m.f32 ? (uintptr_t)(static_cast<const float*>(a.m.p) + mo)
                             : ((uintptr_t)(static_cast<const unsigned char*>(a.m.p) + mo) & 3) << 2;
        vector = (bits & 15) == 0;
      }
      if (vector) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(pu);
        const f32x4 v = *reinterpret_cast<const f32x4*>(pu + a.fsc);
        const f32x4 gu = *reinterpret_cast<const f32x4*>(pg);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(pg + a.gsc);
        bool ok[4] = {true, true, true, true};
        if (a.m.p) {
          if (a.m.f32) {
            const f32x4 m = *reinterpret_cast<const f32x4*>(static_cast<const float*>(a.m.p) + mo);
#pragma unroll
            for (int k = 0; k < 4; ++k) ok[k] = m[k] >= 0.5f;
          } else {
            const uint32_t m = *reinterpret_cast<const uint32_t*>(static_cast<const unsigned char*>(a.m.p) + mo);
#pragma unroll
            for (int k = 0; k < 4; ++k) ok[k] = ((m >> (8 * k)) & 0xffu) != 0;
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) ev[k] = metrics_pixel(u[k], v[k], gu[k], gv[k], ok[k], a.limit, acc);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          ev[k] = 0.0f;
          if (k < cnt) {
            const long fo = (long)y * a.fpitch + x, go = (long)y * a.gpitch + x;
            ev[k] = metrics_pixel(f0[fo], f0[fo + a.fsc], g0[go], g0[go + a.gsc],
                                  mask_says(a.m, m0 + (long)y * a.m.pitch + x), a.limit, acc);
            if (++x == a.W) {
              x = 0;
              ++y;
            }
          }
        }
      }
      if (e0) {
        float* o = e0 + r0;
        if (cnt == 4 && (((uintptr_t)o) & 15) == 0) {
          *reinterpret_cast<f32x4*>(o) = f32x4{ev[0], ev[1], ev[2], ev[3]};
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < cnt) o[k] = ev[k];
        }
      }
    }

    const unsigned cnts[Layout::kSummed] = {acc.n,       acc.nonfinite, acc.lt1, acc.lt3, acc.lt5,
                                            acc.outlier, acc.s0,        acc.s1,  acc.s2};
    const double sums[Layout::kSums] = {acc.sum, acc.sum0, acc.sum1, acc.sum2};
    store_partial<Layout>(cnts, sums, a.ws + ((long)b * a.nb + blockIdx.x) * kSlots, wave);
  }
}

}  // namespace
}  // namespace raft

using namespace raft;

extern "C" size_t raft_flow_metrics_ws_bytes(int B, int H, int W) {
  if (!size_ok(B, H, W)) return 0;
  return (size_t)B * metrics_blocks((long)H * W) * kSlots * sizeof(long long);
}

extern "C" int raft_flow_metrics(const float* flow, long flow_batch_stride, long flow_chan_stride, long flow_pitch,
                                 const float* flow_gt, long gt_batch_stride, long gt_chan_stride, long gt_pitch,
                                 const void* valid, int valid_dtype, long valid_batch_stride, long valid_pitch, int B,
                                 int H, int W, float gt_limit, void* record, void* totals, float* epe_map, void* ws,
                                 raft_stream_t stream) {
  RAFT_REQUIRE(flow && flow_gt && record && ws, "raft_flow_metrics: null pointer");
  const char* who = "raft_flow_metrics";
  if (const int rc = check_size(who, B, H, W)) return rc;
  if (const int rc = check_mask(who, valid, valid_dtype, valid_batch_stride, valid_pitch, W)) return rc;
  RAFT_REQUIRE(!std::isnan(gt_limit) && !std::isinf(gt_limit),
               "raft_flow_metrics: gt_limit must be finite (<= 0: no limit)");
  RAFT_REQUIRE(flow_pitch >= W && flow_batch_stride >= 0 && flow_chan_stride >= 0 && gt_pitch >= W &&
                   gt_batch_stride >= 0 && gt_chan_stride >= 0,
               "raft_flow_metrics: bad strides (a row pitch holds W floats; strides are not negative)");
  RAFT_REQUIRE((((uintptr_t)flow | (uintptr_t)flow_gt | (uintptr_t)epe_map) & 3) == 0,
               "raft_flow_metrics: misaligned pointer (flow, flow_gt, epe_map 4 bytes)");
  const void* ins[3] = {flow, flow_gt, valid};
  if (const int rc = check_outputs(who, record, totals, ws, epe_map, ins, 3)) return rc;
  MetricsArgs a;
  a.flow = flow;
  a.fsb = flow_batch_stride;
  a.fsc = flow_chan_stride;
  a.fpitch = flow_pitch;
  a.gt = flow_gt;
  a.gsb = gt_batch_stride;
  a.gsc = gt_chan_stride;
  a.gpitch = gt_pitch;
  a.m = mask_view(valid, valid_dtype, valid_batch_stride, valid_pitch);
  a.limit = gt_limit > 0.f ? gt_limit : 0.f;
  a.ws = static_cast<long long*>(ws);
  a.epe_map = epe_map;
  a.B = B;
  a.H = H;
  a.W = W;
  a.nb = metrics_blocks((long)H * W);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(metrics_partial_kernel, dim3(a.nb, B < 65535 ? B : 65535), dim3(256), 0, s, a);
  const int rc = check_launch("raft_flow_metrics (partial)");
  if (rc) return rc;
  return launch_finalize<Layout>(who, ws, record, totals, B, a.nb, H, W, s);
}
