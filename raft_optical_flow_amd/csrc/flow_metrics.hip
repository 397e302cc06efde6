// Scoring a flow against ground truth (gfx950): evaluate.py's validate_* arithmetic on the device.
//
//   raft_flow_metrics_ws_bytes  size of the partial-record workspace
//   raft_flow_metrics           flow, flow_gt [B,2,H,W] and an optional mask (all read in place through their
//                               strides) -> one record of 16 64-bit slots per sample, optionally added into
//                               running totals, optionally the per-pixel EPE map; two launches, no atomics
//
// The definition is in raft_hip.h.  Two kernels:
//
//   metrics_partial_kernel   grid (NB, B), NB = metrics_blocks(H * W) <= RAFT_FLOW_METRICS_MAX_BLOCKS: a function
//                            of (H, W) only, never of the device.  Work-group (p, b) takes every NB-th run of
//                            256 x 4 pixels of sample b (a work-group never spans two samples).  A thread sums in
//                            integers and in fp64; the wave reduces with the __shfl_xor butterfly (a + b is
//                            commutative: every lane ends with the same bits), the four waves' sums are added
//                            through LDS in wave order, and the work-group writes its partial record to
//                            ws[b][p][16].  Every slot is written on every call: the workspace needs no
//                            initialisation.
//   metrics_finalize_kernel  one work-group.  The partials are staged in LDS; thread (b, slot) adds the NB
//                            partials of its slot in index order and writes the sample's record; one thread adds
//                            every sample's record, in sample order, into the totals (if given), with `images`
//                            and `image_mean_sum`.
//
// The order of every addition is fixed by (B, H, W): two runs are bitwise equal, and a sample's record does not
// depend on its batch index or on the other samples.
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

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace raft {
namespace {

constexpr int kSlots = RAFT_FLOW_METRICS_SLOTS;
constexpr int kBlockPixels = RAFT_FLOW_METRICS_BLOCK_PIXELS;   // 256 threads x 4 pixels
constexpr int kMaxBlocks = RAFT_FLOW_METRICS_MAX_BLOCKS;
static_assert(kBlockPixels == 1024 && kSlots == 16, "the kernels below are written for these");

struct MetricsArgs {
  const float* flow;      // element (b = 0, c = 0, y = 0, x = 0)
  long fsb, fsc, fpitch;  // in floats
  const float* gt;
  long gsb, gsc, gpitch;
  const void* mask;       // or null
  long msb, mpitch;       // in elements
  int mask_f32;
  float limit;            // <= 0: absent
  long long* ws;          // [B][nb][16]
  long long* record;      // [B][16]
  long long* totals;      // [16] or null
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

__device__ __forceinline__ bool mask_says(const MetricsArgs& a, long off) {
  if (!a.mask) return true;
  if (a.mask_f32) return static_cast<const float*>(a.mask)[off] >= 0.5f;   // a NaN fails
  return static_cast<const unsigned char*>(a.mask)[off] != 0;
}

__device__ __forceinline__ unsigned wave_sum(unsigned x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

__global__ __launch_bounds__(256) void metrics_partial_kernel(MetricsArgs a) {
  __shared__ long long s_part[4][kSlots];
  const long HW = (long)a.H * a.W;
  const long groups = (HW + 3) >> 2;
  const int wave = threadIdx.x >> 6;
  for (int b = blockIdx.y; b < a.B; b += gridDim.y) {   // (gridDim.y = B up to the grid's limit)
    const float* f0 = a.flow + (long)b * a.fsb;
    const float* g0 = a.gt + (long)b * a.gsb;
    const long m0 = (long)b * a.msb;
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
      const long mo = m0 + (long)y * a.mpitch + x;
      if (vector) {
        uintptr_t bits = (uintptr_t)pu | (uintptr_t)(pu + a.fsc) | (uintptr_t)pg | (uintptr_t)(pg + a.gsc);
        if (a.mask)
          bits |= a.mask_f32 ? (uintptr_t)(static_cast<const float*>(a.mask) + mo)
                             : ((uintptr_t)(static_cast<const unsigned char*>(a.mask) + mo) & 3) << 2;
        vector = (bits & 15) == 0;
      }
      if (vector) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(pu);
        const f32x4 v = *reinterpret_cast<const f32x4*>(pu + a.fsc);
        const f32x4 gu = *reinterpret_cast<const f32x4*>(pg);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(pg + a.gsc);
        bool ok[4] = {true, true, true, true};
        if (a.mask) {
          if (a.mask_f32) {
            const f32x4 m = *reinterpret_cast<const f32x4*>(static_cast<const float*>(a.mask) + mo);
#pragma unroll
            for (int k = 0; k < 4; ++k) ok[k] = m[k] >= 0.5f;
          } else {
            const uint32_t m = *reinterpret_cast<const uint32_t*>(static_cast<const unsigned char*>(a.mask) + mo);
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
                                  mask_says(a, m0 + (long)y * a.mpitch + x), a.limit, acc);
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

    const unsigned cnts[9] = {wave_sum(acc.n),   wave_sum(acc.nonfinite), wave_sum(acc.lt1),
                              wave_sum(acc.lt3), wave_sum(acc.lt5),       wave_sum(acc.outlier),
                              wave_sum(acc.s0),  wave_sum(acc.s1),        wave_sum(acc.s2)};
    const double sums[4] = {wave_sum(acc.sum), wave_sum(acc.sum0), wave_sum(acc.sum1), wave_sum(acc.sum2)};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) s_part[wave][RAFT_FM_N + k] = (long long)cnts[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) s_part[wave][RAFT_FM_EPE_SUM + k] = __double_as_longlong(sums[k]);
    }
    __syncthreads();
    if (threadIdx.x < kSlots) {
      const int s = threadIdx.x;
      long long out = 0;   // the slots past the sums: 0 in a partial and in a sample's record
      if (s < RAFT_FM_EPE_SUM) {
        out = s_part[0][s] + s_part[1][s] + s_part[2][s] + s_part[3][s];
      } else if (s < RAFT_FM_IMAGES) {
        const double d = ((__longlong_as_double(s_part[0][s]) + __longlong_as_double(s_part[1][s])) +
                          __longlong_as_double(s_part[2][s])) +
                         __longlong_as_double(s_part[3][s]);
        out = __double_as_longlong(d);
      }
      a.ws[((long)b * a.nb + blockIdx.x) * kSlots + s] = out;
    }
    __syncthreads();
  }
}

// One work-group.  The partials are staged in LDS, kFinalizeSlots of them at a time (whole samples: NB <= 256
// partials of 16 slots), by all 256 threads, so that the adds in index order do not wait on one global load
// each; thread (sample, slot) then adds its NB partials from LDS.  Thread 0 carries the totals in registers and
// adds each staged sample's record in sample order.
constexpr int kFinalizeSlots = kMaxBlocks * kSlots;   // 4096 x 8 B = 32 KiB

__global__ __launch_bounds__(256) void metrics_finalize_kernel(MetricsArgs a) {
  __shared__ long long s_ws[kFinalizeSlots];
  __shared__ long long s_rec[256];   // the staged samples' records: (sample, slot) = thread
  const int tid = threadIdx.x;
  // samples staged at a time: what the LDS holds (>= 1), and one thread per (sample, slot)
  const int per = kMaxBlocks / a.nb < 256 / kSlots ? kMaxBlocks / a.nb : 256 / kSlots;
  const bool totals = a.totals != nullptr && tid == 0;
  long long cnt[RAFT_FM_EPE_SUM] = {};
  double sum[4] = {};
  double mean_sum = 0.0;
  long long images = 0;
  if (totals) {
#pragma unroll
    for (int s = 0; s < RAFT_FM_EPE_SUM; ++s) cnt[s] = a.totals[s];
#pragma unroll
    for (int k = 0; k < 4; ++k) sum[k] = __longlong_as_double(a.totals[RAFT_FM_EPE_SUM + k]);
    images = a.totals[RAFT_FM_IMAGES];
    mean_sum = __longlong_as_double(a.totals[RAFT_FM_IMAGE_MEAN_SUM]);
  }
  for (int b0 = 0; b0 < a.B; b0 += per) {
    const int nsamp = a.B - b0 < per ? a.B - b0 : per;
    const int staged = nsamp * a.nb * kSlots;            // <= kFinalizeSlots
    const long long* src = a.ws + (long)b0 * a.nb * kSlots;
    {
      // kFinalizeSlots / 256 = 16 loads per thread, all issued before the first is stored
      long long v[kFinalizeSlots / 256];
#pragma unroll
      for (int k = 0; k < kFinalizeSlots / 256; ++k) v[k] = tid + 256 * k < staged ? src[tid + 256 * k] : 0;
#pragma unroll
      for (int k = 0; k < kFinalizeSlots / 256; ++k)
        if (tid + 256 * k < staged) s_ws[tid + 256 * k] = v[k];
    }
    __syncthreads();
    if (tid < nsamp * kSlots) {
      const int j = tid / kSlots, s = tid - j * kSlots;
      const long long* part = s_ws + j * a.nb * kSlots + s;
      long long out = 0;   // the slots past the sums: 0 in a sample's record
      if (s < RAFT_FM_EPE_SUM) {
#pragma unroll 16
        for (int p = 0; p < a.nb; ++p) out += part[p * kSlots];
      } else if (s < RAFT_FM_IMAGES) {
        double d = 0.0;
#pragma unroll 16   // (the reads are issued ahead of the chain of adds; the order of the adds stays)
        for (int p = 0; p < a.nb; ++p) d += __longlong_as_double(part[p * kSlots]);
        out = __double_as_longlong(d);
      }
      a.record[(long)b0 * kSlots + tid] = out;
      s_rec[tid] = out;
    }
    __syncthreads();
    if (totals) {
      for (int j = 0; j < nsamp; ++j) {
        const long long* r = s_rec + j * kSlots;
#pragma unroll
        for (int s = 0; s < RAFT_FM_EPE_SUM; ++s) cnt[s] += r[s];
#pragma unroll
        for (int k = 0; k < 4; ++k) sum[k] += __longlong_as_double(r[RAFT_FM_EPE_SUM + k]);
        if (r[RAFT_FM_N] > 0) {
          ++images;
          mean_sum += __longlong_as_double(r[RAFT_FM_EPE_SUM]) / (double)r[RAFT_FM_N];
        }
      }
    }
    __syncthreads();   // thread 0 has read s_rec before the next pass overwrites it
  }
  if (!totals) return;
#pragma unroll
  for (int s = 0; s < RAFT_FM_EPE_SUM; ++s) a.totals[s] = cnt[s];
#pragma unroll
  for (int k = 0; k < 4; ++k) a.totals[RAFT_FM_EPE_SUM + k] = __double_as_longlong(sum[k]);
  a.totals[RAFT_FM_IMAGES] = images;
  a.totals[RAFT_FM_IMAGE_MEAN_SUM] = __double_as_longlong(mean_sum);
  a.totals[RAFT_FM_RESERVED] = 0;
}

bool metrics_size_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 30); }

}  // namespace
}  // namespace raft

using namespace raft;

extern "C" size_t raft_flow_metrics_ws_bytes(int B, int H, int W) {
  if (!metrics_size_ok(B, H, W)) return 0;
  return (size_t)B * metrics_blocks((long)H * W) * kSlots * sizeof(long long);
}

extern "C" int raft_flow_metrics(const float* flow, long flow_batch_stride, long flow_chan_stride, long flow_pitch,
                                 const float* flow_gt, long gt_batch_stride, long gt_chan_stride, long gt_pitch,
                                 const void* valid, int valid_dtype, long valid_batch_stride, long valid_pitch, int B,
                                 int H, int W, float gt_limit, void* record, void* totals, float* epe_map, void* ws,
                                 raft_stream_t stream) {
  RAFT_REQUIRE(flow && flow_gt && record && ws, "raft_flow_metrics: null pointer");
  RAFT_REQUIRE(metrics_size_ok(B, H, W), "raft_flow_metrics: bad size %d x %d x %d", B, H, W);
  RAFT_REQUIRE(!valid || valid_dtype == RAFT_MASK_U8 || valid_dtype == RAFT_MASK_F32,
               "raft_flow_metrics: unknown mask dtype tag %d", valid_dtype);
  RAFT_REQUIRE(!std::isnan(gt_limit) && !std::isinf(gt_limit),
               "raft_flow_metrics: gt_limit must be finite (<= 0: no limit)");
  RAFT_REQUIRE(flow_pitch >= W && flow_batch_stride >= 0 && flow_chan_stride >= 0 && gt_pitch >= W &&
                   gt_batch_stride >= 0 && gt_chan_stride >= 0,
               "raft_flow_metrics: bad strides (a row pitch holds W floats; strides are not negative)");
  RAFT_REQUIRE(!valid || (valid_pitch >= W && valid_batch_stride >= 0),
               "raft_flow_metrics: bad mask strides (a row pitch holds W elements; strides are not negative)");
  const bool mask_f32 = valid && valid_dtype == RAFT_MASK_F32;
  RAFT_REQUIRE((((uintptr_t)flow | (uintptr_t)flow_gt | (uintptr_t)epe_map) & 3) == 0 &&
                   (!mask_f32 || ((uintptr_t)valid & 3) == 0) &&
                   (((uintptr_t)record | (uintptr_t)totals | (uintptr_t)ws) & 7) == 0,
               "raft_flow_metrics: misaligned pointer (flow, flow_gt, float32 mask, epe_map 4 bytes; record, totals, "
               "ws 8)");
  const void* ins[3] = {flow, flow_gt, valid};
  const void* outs[4] = {record, ws, totals, epe_map};
  for (int i = 0; i < 4; ++i) {
    if (!outs[i]) continue;
    for (int j = 0; j < 3; ++j)
      RAFT_REQUIRE(outs[i] != ins[j], "raft_flow_metrics: an output aliases an input or another output");
    for (int j = 0; j < i; ++j)
      RAFT_REQUIRE(outs[i] != outs[j], "raft_flow_metrics: an output aliases an input or another output");
  }
  MetricsArgs a;
  a.flow = flow;
  a.fsb = flow_batch_stride;
  a.fsc = flow_chan_stride;
  a.fpitch = flow_pitch;
  a.gt = flow_gt;
  a.gsb = gt_batch_stride;
  a.gsc = gt_chan_stride;
  a.gpitch = gt_pitch;
  a.mask = valid;
  a.msb = valid ? valid_batch_stride : 0;
  a.mpitch = valid ? valid_pitch : 0;
  a.mask_f32 = mask_f32 ? 1 : 0;
  a.limit = gt_limit > 0.f ? gt_limit : 0.f;
  a.ws = static_cast<long long*>(ws);
  a.record = static_cast<long long*>(record);
  a.totals = static_cast<long long*>(totals);
  a.epe_map = epe_map;
  a.B = B;
  a.H = H;
  a.W = W;
  a.nb = metrics_blocks((long)H * W);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(metrics_partial_kernel, dim3(a.nb, B < 65535 ? B : 65535), dim3(256), 0, s, a);
  const int rc = check_launch("raft_flow_metrics (partial)");
  if (rc) return rc;
  hipLaunchKernelGGL(metrics_finalize_kernel, dim3(1), dim3(256), 0, s, a);
  return check_launch("raft_flow_metrics");
}
