// The record reduction of the two flow scorers (definitions: raft_hip.h, raft_flow_metrics and
// raft_photo_metrics), shared by flow_metrics.hip and photo_metrics.hip: a record is 16 slots of 64 bits, int64
// counts first, then fp64 sums by their bits, then (in the totals only) `images` and the sum of per-image means.
//
//   work-group (p, b) of a scorer's pixel kernel: per-thread sums in 32-bit integers and fp64; store_partial adds
//     them over the wave with the __shfl_xor butterfly (a + b is commutative: every lane ends with the same bits)
//     and over the four waves through LDS in wave order, ((w0 + w1) + w2) + w3, and writes one partial record to
//     ws[b][p][16].  Every slot is written on every call: the workspace needs no initialisation.
//   record_finalize_kernel<Layout>: one work-group adds each sample's nb partials in index order, starting at 0,
//     writes the sample's record, and thread 0 adds the records into the totals (if given) in sample order.
//
// No atomics.  The order of every addition is fixed by (B, nb): two runs are bitwise equal, and a sample's record
// does not depend on its batch index or on the other samples.  Also here: the argument checks that the two C
// entries share.
#pragma once

#include "common.hpp"

#include <cstdint>

namespace raft {
namespace {

constexpr int kRecordSlots = 16;

// A scorer's slots: COUNTS int64 counts from slot 0 (PIXELS, if not -1, is the last of them and is H * W, written
// by the finalize kernel), SUMS fp64 sums after them, then `images` and the sum over images of
// slot MEAN_NUM / slot MEAN_DEN (where that is > 0), then reserved slots (0).
template <int COUNTS, int PIXELS, int SUMS, int MEAN_NUM, int MEAN_DEN>
struct RecordLayout {
  static constexpr int kCounts = COUNTS, kPixels = PIXELS, kSums = SUMS, kMeanNum = MEAN_NUM, kMeanDen = MEAN_DEN;
  static constexpr int kSummed = PIXELS < 0 ? COUNTS : COUNTS - 1;   // counts a thread carries
  static constexpr int kFirstSum = COUNTS, kImages = COUNTS + SUMS, kMeanSum = kImages + 1, kReserved = kImages + 2;
  static_assert(PIXELS == -1 || PIXELS == COUNTS - 1, "the pixels slot is the last count");
  static_assert(kReserved <= kRecordSlots && MEAN_DEN < kSummed && MEAN_NUM >= kFirstSum && MEAN_NUM < kImages, "");
};

struct MaskView {
  const void* p;    // or null: every pixel
  long sb, pitch;   // in elements
  int f32;
};

// the mask's word on the pixel at element offset off
__device__ __forceinline__ bool mask_says(const MaskView& m, long off) {
  if (!m.p) return true;
  if (m.f32) return static_cast<const float*>(m.p)[off] >= 0.5f;   // a NaN fails
  return static_cast<const unsigned char*>(m.p)[off] != 0;
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

// The end of a 256-thread work-group's pass over a sample: the threads' counts and sums -> the partial record at
// ws_rec[16].  Called by every thread, wave = threadIdx.x / 64 as the caller holds it (recomputed here it costs the
// photo tile kernel two VGPRs); ends with a barrier, so it may be called again at once.
template <class L>
__device__ __forceinline__ void store_partial(const unsigned (&cnt)[L::kSummed], const double (&sum)[L::kSums],
                                              long long* ws_rec, int wave) {
  __shared__ long long s_part[4][kRecordSlots];
  unsigned c[L::kSummed];
  double d[L::kSums];
#pragma unroll
  for (int k = 0; k < L::kSummed; ++k) c[k] = wave_sum(cnt[k]);
#pragma unroll
  for (int k = 0; k < L::kSums; ++k) d[k] = wave_sum(sum[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < L::kSummed; ++k) s_part[wave][k] = (long long)c[k];
#pragma unroll
    for (int k = 0; k < L::kSums; ++k) s_part[wave][L::kFirstSum + k] = __double_as_longlong(d[k]);
  }
  __syncthreads();
  if (threadIdx.x < kRecordSlots) {
    const int s = threadIdx.x;
    long long out = 0;   // pixels (the finalize kernel writes it), the totals' slots and the reserved ones
    if (s < L::kSummed) {
      out = s_part[0][s] + s_part[1][s] + s_part[2][s] + s_part[3][s];
    } else if (s >= L::kFirstSum && s < L::kImages) {
      const double v = ((__longlong_as_double(s_part[0][s]) + __longlong_as_double(s_part[1][s])) +
                        __longlong_as_double(s_part[2][s])) +
                       __longlong_as_double(s_part[3][s]);
      out = __double_as_longlong(v);
    }
    ws_rec[s] = out;
  }
  __syncthreads();
}

struct FinalizeArgs {
  const long long* ws;   // [B][nb][16]
  long long* record;     // [B][16]
  long long* totals;     // [16] or null
  int B, nb;
  long long pixels;      // H * W
};

// One work-group.  The partials are staged in LDS, 256 of them at a time, by all 256 threads, so that the adds
// in index order do not wait on one global load each.  Where a sample has fewer than 256 partials several
// samples (whole ones, 16 at most) are staged together and thread (sample, slot) adds its sample's; a sample
// with more is staged alone in runs of 256 and its 16 threads carry their sums from run to run.  Thread 0
// carries the totals in registers and adds each sample's record in sample order.
constexpr int kStage = 256;   // partials per staging pass: 256 x 16 x 8 B = 32 KiB

template <class L>
__global__ __launch_bounds__(256) void record_finalize_kernel(FinalizeArgs a) {
  constexpr int kSlots = kRecordSlots;
  __shared__ long long s_ws[kStage * kSlots];
  __shared__ long long s_rec[256];   // the staged samples' records: (sample, slot) = thread
  const int tid = threadIdx.x;
  const int nb = a.nb;
  const int per = nb >= kStage ? 1 : (kStage / nb < 256 / kSlots ? kStage / nb : 256 / kSlots);
  const bool totals = a.totals != nullptr && tid == 0;
  long long cnt[L::kCounts] = {};
  double sum[L::kSums] = {};
  double mean_sum = 0.0;
  long long images = 0;
  if (totals) {
#pragma unroll
    for (int k = 0; k < L::kCounts; ++k) cnt[k] = a.totals[k];
#pragma unroll
    for (int k = 0; k < L::kSums; ++k) sum[k] = __longlong_as_double(a.totals[L::kFirstSum + k]);
    images = a.totals[L::kImages];
    mean_sum = __longlong_as_double(a.totals[L::kMeanSum]);
  }
  for (int b0 = 0; b0 < a.B; b0 += per) {
    const int nsamp = a.B - b0 < per ? a.B - b0 : per;
    const int j = tid / kSlots, s = tid - j * kSlots;    // the thread's (sample, slot), where tid < nsamp * 16
    long long icnt = 0;
    double dsum = 0.0;
    for (int p0 = 0; p0 < nb; p0 += kStage) {            // (one pass unless nb > kStage)
      const int pn = nb - p0 < kStage ? nb - p0 : kStage;
      const int staged = nsamp * pn * kSlots;            // <= kStage * 16 (nsamp > 1 only where pn == nb)
      const long long* src = a.ws + ((long)b0 * nb + p0) * kSlots;
      {
        // 16 loads per thread, all issued before the first is stored
        long long v[kStage * kSlots / 256];
#pragma unroll
        for (int k = 0; k < kStage * kSlots / 256; ++k) v[k] = tid + 256 * k < staged ? src[tid + 256 * k] : 0;
#pragma unroll
        for (int k = 0; k < kStage * kSlots / 256; ++k)
          if (tid + 256 * k < staged) s_ws[tid + 256 * k] = v[k];
      }
      __syncthreads();
      if (tid < nsamp * kSlots) {
        const long long* part = s_ws + j * pn * kSlots + s;
        if (s < L::kSummed) {
#pragma unroll 16
          for (int p = 0; p < pn; ++p) icnt += part[p * kSlots];
        } else if (s >= L::kFirstSum && s < L::kImages) {
#pragma unroll 16   // (the reads are issued ahead of the chain of adds; the order of the adds stays)
          for (int p = 0; p < pn; ++p) dsum += __longlong_as_double(part[p * kSlots]);
        }
      }
      __syncthreads();   // s_ws is read before the next pass overwrites it
    }
    if (tid < nsamp * kSlots) {
      long long out = 0;   // the totals' slots and the reserved ones: 0 in a sample's record
      if (s < L::kSummed) out = icnt;
      else if (s == L::kPixels) out = a.pixels;
      else if (s >= L::kFirstSum && s < L::kImages) out = __double_as_longlong(dsum);
      a.record[(long)b0 * kSlots + tid] = out;
      s_rec[tid] = out;
    }
    __syncthreads();
    if (totals) {
      for (int q = 0; q < nsamp; ++q) {
        const long long* r = s_rec + q * kSlots;
#pragma unroll
        for (int k = 0; k < L::kCounts; ++k) cnt[k] += r[k];
#pragma unroll
        for (int k = 0; k < L::kSums; ++k) sum[k] += __longlong_as_double(r[L::kFirstSum + k]);
        if (r[L::kMeanDen] > 0) {
          ++images;
          mean_sum += __longlong_as_double(r[L::kMeanNum]) / (double)r[L::kMeanDen];
        }
      }
    }
    __syncthreads();   // thread 0 has read s_rec before the next pass overwrites it
  }
  if (!totals) return;
#pragma unroll
  for (int k = 0; k < L::kCounts; ++k) a.totals[k] = cnt[k];
#pragma unroll
  for (int k = 0; k < L::kSums; ++k) a.totals[L::kFirstSum + k] = __double_as_longlong(sum[k]);
  a.totals[L::kImages] = images;
  a.totals[L::kMeanSum] = __double_as_longlong(mean_sum);
#pragma unroll
  for (int k = L::kReserved; k < kSlots; ++k) a.totals[k] = 0;
}

// The second launch of a scorer's entry (`who`, for the message).
template <class L>
int launch_finalize(const char* who, void* ws, void* record, void* totals, int B, int nb, int H, int W,
                    hipStream_t s) {
  const FinalizeArgs f = {static_cast<const long long*>(ws), static_cast<long long*>(record),
                          static_cast<long long*>(totals), B, nb, (long long)H * W};
  hipLaunchKernelGGL(record_finalize_kernel<L>, dim3(1), dim3(256), 0, s, f);
  return check_launch(who);
}

// ---- the argument checks the two entries share: 0, or RAFT_E_INVALID with the message set ----

inline int check_size(const char* who, int B, int H, int W) {
  RAFT_REQUIRE(size_ok(B, H, W), "%s: bad size %d x %d x %d", who, B, H, W);
  return 0;
}

// an absent mask's tag and strides are not read; a byte mask needs no alignment
inline int check_mask(const char* who, const void* mask, int dtype, long batch_stride, long pitch, int W) {
  if (!mask) return 0;
  RAFT_REQUIRE(dtype == RAFT_MASK_U8 || dtype == RAFT_MASK_F32, "%s: unknown mask dtype tag %d", who, dtype);
  RAFT_REQUIRE(pitch >= W && batch_stride >= 0,
               "%s: bad mask strides (a row pitch holds W elements; strides are not negative)", who);
  RAFT_REQUIRE(dtype != RAFT_MASK_F32 || ((uintptr_t)mask & 3) == 0, "%s: misaligned pointer (a float32 mask 4 bytes)",
               who);
  return 0;
}

inline MaskView mask_view(const void* mask, int dtype, long batch_stride, long pitch) {
  return MaskView{mask, mask ? batch_stride : 0, mask ? pitch : 0, mask && dtype == RAFT_MASK_F32 ? 1 : 0};
}

// record, totals (or null), ws and the map (or null) against the n inputs (null ones are skipped) and each other
inline int check_outputs(const char* who, const void* record, const void* totals, const void* ws, const void* map,
                         const void* const* ins, int n) {
  RAFT_REQUIRE((((uintptr_t)record | (uintptr_t)totals | (uintptr_t)ws) & 7) == 0,
               "%s: misaligned pointer (record, totals, ws 8 bytes)", who);
  const void* outs[4] = {record, ws, totals, map};
  for (int i = 0; i < 4; ++i) {
    if (!outs[i]) continue;
    bool alias = false;
    for (int j = 0; j < n; ++j) alias = alias || outs[i] == ins[j];
    for (int j = 0; j < i; ++j) alias = alias || outs[i] == outs[j];
    RAFT_REQUIRE(!alias, "%s: an output aliases an input or another output", who);
  }
  return 0;
}

}  // namespace
}  // namespace raft
