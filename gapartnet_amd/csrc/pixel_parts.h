// pixel_parts.h — what the frame-level stages (articulate.hip, multiview.hip) share: the wave helpers over small integer keys, the
// stable multi-way partition of the pixels of V frames by key, and the workgroup arg-max over an exact ratio.
//
// Pixels are walked in chunks of kChunk: thread tid of workgroup (chunk, v) owns the pixels chunk * kChunk + e * kThreads + tid,
// e < kPer, of frame v.  Every kernel here is launched with kThreads threads.
//
// The partition (pp_partition) writes, for every key, its pixels in ascending (frame, pixel) order:
//   count  per chunk, the members of every key (an LDS histogram, one add per group of equal keys in a wave)
//   scan   one workgroup per segment of `counts`: the exclusive prefix over the segment's cells, in place
//   store  the rank of a pixel among the earlier pixels of its key = the scanned count of its chunk + the members in the
//          earlier (slot e, wave) pairs of the chunk (LDS counters, added in that order) + the earlier lanes of its wave with
//          the same key (ballots); then the policy's row write
// A policy is a struct passed to the kernels by value:
//   static constexpr int kMaxKeys       width of the LDS tables (keys are 0 .. kMaxKeys - 1)
//   static constexpr int kKeyBits       bits of a key: kMaxKeys <= 1 << kKeyBits
//   int live_keys(v)                    device: the key slots of frame v that are counted, scanned and walked (<= kMaxKeys)
//   int key(v, g, inside)               device: the key of pixel g = v * HW + p, or -1 for no key (always -1 when not inside)
//   int64_t counts_index(v, key, chunk, nchunk, V)   device: the cell of (frame, key, chunk) in `counts`
//   dim3 scan_grid(V), int64_t scan_len(V, nchunk)   host: one workgroup per segment (segment = blockIdx.y * gridDim.x +
//                                       blockIdx.x), the cells of a segment; the segments tile `counts`
//   void store(v, key, rank, g)         device: write pixel g as member `rank` of its key - or drop it (a key without a
//                                       segment, a row beyond the output)
// No float atomics; integer atomics only on the LDS histogram (order-free): the result does not depend on timing.
#pragma once
#include "gpn_common.h"
#include "wg_scan.h"

namespace gpn {
namespace pp {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 4;  // pixels per thread: pixel = chunk * kChunk + e * kThreads + tid
constexpr int kChunk = kThreads * kPer;
constexpr int kGroupRounds = 8;  // key groups a wave resolves by ballots before its remaining lanes add one by one

// bins[key] += 1 for every lane with key >= 0, one LDS atomic per group of equal keys.  Called by whole waves.
__device__ __forceinline__ void wave_hist_add(int* bins, int key) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(key >= 0);
  for (int round = 0; todo != 0ull && round < kGroupRounds; ++round) {  // (todo is wave-uniform)
    const int lead = __ffsll((long long)todo) - 1;
    const int k = __shfl(key, lead, 64);
    const unsigned long long same = __ballot(key == k);
    if (lane == lead) atomicAdd(&bins[k], __popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) atomicAdd(&bins[key], 1);
}

// the lanes of the wave whose key (kBits bits, `ok` lanes only) equals this lane's: kBits + 1 ballots.  0 for a lane that is not ok.
template <int kBits>
__device__ __forceinline__ unsigned long long wave_match(int key, bool ok) {
  unsigned long long same = __ballot(ok);
#pragma unroll
  for (int b = 0; b < kBits; ++b) {
    const bool bit = ((key >> b) & 1) != 0;
    const unsigned long long m = __ballot(ok && bit);
    same &= bit ? m : ~m;
  }
  return ok ? same : 0ull;
}

// ---- the stable multi-way partition ---------------------------------------------------------------------------------------------
template <class Policy>
__global__ __launch_bounds__(kThreads) void pp_count_kernel(const Policy pol, int64_t HW, int32_t* __restrict__ counts) {
  __shared__ int h[Policy::kMaxKeys];
  const int v = blockIdx.y, tid = threadIdx.x;
  for (int k = tid; k < Policy::kMaxKeys; k += kThreads) h[k] = 0;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    wave_hist_add(h, pol.key(v, (int64_t)v * HW + p, p < HW));
  }
  __syncthreads();
  const int live = min(pol.live_keys(v), Policy::kMaxKeys);  // (the clamp bounds the walk by the LDS table, whatever the policy says)
  for (int k = tid; k < live; k += kThreads) counts[pol.counts_index(v, k, blockIdx.x, gridDim.x, gridDim.y)] = h[k];
}

// (static: not a template, and defined in every file that includes this header)
static __global__ __launch_bounds__(kThreads) void pp_scan_kernel(int32_t* __restrict__ counts, int64_t seg_len) {
  __shared__ int wsum[kWaves];
  int32_t* c = counts + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * seg_len;
  block_scan_tiled<kWaves, int>(seg_len, [&](int64_t i) { return c[i]; }, c, wsum);
}

template <class Policy>
__global__ __launch_bounds__(kThreads) void pp_store_kernel(const Policy pol, int64_t HW, const int32_t* __restrict__ base) {
  __shared__ int cnt[kPer * kWaves][Policy::kMaxKeys];  // members of a key in (slot e, wave), then the members before that (slot, wave)
  const int v = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int i = tid; i < kPer * kWaves * Policy::kMaxKeys; i += kThreads) (&cnt[0][0])[i] = 0;
  __syncthreads();
  int key[kPer], rank[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    key[e] = pol.key(v, (int64_t)v * HW + p, p < HW);
    const unsigned long long same = wave_match<Policy::kKeyBits>(key[e], key[e] >= 0);
    rank[e] = __popcll(same & below);
    if (key[e] >= 0 && rank[e] == 0) cnt[e * kWaves + wave][key[e]] = __popcll(same);  // (the group's lowest lane)
  }
  __syncthreads();
  const int live = min(pol.live_keys(v), Policy::kMaxKeys);  // (the clamp bounds the walk by the LDS table, whatever the policy says)
  for (int k = tid; k < live; k += kThreads) {  // (slot order: e first, then the wave)
    int run = base[pol.counts_index(v, k, blockIdx.x, gridDim.x, gridDim.y)];
#pragma unroll
    for (int s = 0; s < kPer * kWaves; ++s) {
      const int c = cnt[s][k];
      cnt[s][k] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    if (key[e] < 0) continue;
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    pol.store(v, key[e], cnt[e * kWaves + wave][key[e]] + rank[e], (int64_t)v * HW + p);
  }
}

// counts: the workspace, one cell per (frame, live key, chunk) in the policy's layout.  Three launches, no host read.
template <class Policy>
int pp_partition(const Policy& pol, int V, int64_t HW, int32_t* counts, hipStream_t stream) {
  const int64_t nchunk = cdiv(HW, kChunk);
  const dim3 grid((unsigned)nchunk, (unsigned)V);
  hipLaunchKernelGGL(pp_count_kernel<Policy>, grid, dim3(kThreads), 0, stream, pol, HW, counts);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(pp_scan_kernel, pol.scan_grid(V), dim3(kThreads), 0, stream, counts, pol.scan_len(V, nchunk));
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(pp_store_kernel<Policy>, grid, dim3(kThreads), 0, stream, pol, HW, counts);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

// ---- the arg-max over an exact ratio --------------------------------------------------------------------------------------------
struct RatioCand {
  int num, den, e;  // the ratio num / den (den > 0) of candidate e; e = -1: none
};
// a before b: the larger ratio by 64-bit cross-multiplication, ties to the smaller e
__device__ __forceinline__ bool ratio_better(const RatioCand& a, const RatioCand& b) {
  if (a.e < 0) return false;
  if (b.e < 0) return true;
  const long long l = (long long)a.num * b.den, r = (long long)b.num * a.den;
  if (l != r) return l > r;
  return a.e < b.e;
}

// the best of the workgroup's candidates, to every thread.  wbest: kWaves entries of LDS, read until the call returns: THE CALLER
// places a barrier between two calls (both callers have one anyway, behind the winner's bookkeeping - a second one in here would
// be one more barrier in every serial round).  Contains a barrier: the whole workgroup of kWaves waves calls it.
template <int kWaves>
__device__ __forceinline__ RatioCand block_best(RatioCand best, RatioCand* wbest) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    RatioCand o;
    o.num = __shfl_xor(best.num, off, 64);
    o.den = __shfl_xor(best.den, off, 64);
    o.e = __shfl_xor(best.e, off, 64);
    if (ratio_better(o, best)) best = o;
  }
  static_assert(kWaves >= 1 && kWaves <= 64 && (kWaves & (kWaves - 1)) == 0, "the waves' candidates are reduced by a butterfly");
  const int lane = threadIdx.x & 63;
  if (lane == 0) wbest[threadIdx.x >> 6] = best;
  __syncthreads();
  // every wave reduces the kWaves candidates in its first kWaves lanes (log2 kWaves steps, not kWaves - 1 in every thread)
  best = lane < kWaves ? wbest[lane] : RatioCand{0, 1, -1};
#pragma unroll
  for (int off = kWaves / 2; off >= 1; off >>= 1) {
    RatioCand o;
    o.num = __shfl_xor(best.num, off, 64);
    o.den = __shfl_xor(best.den, off, 64);
    o.e = __shfl_xor(best.e, off, 64);
    if (ratio_better(o, best)) best = o;
  }
  best.num = __shfl(best.num, 0, 64);
  best.den = __shfl(best.den, 0, 64);
  best.e = __shfl(best.e, 0, 64);
  return best;
}

}  // namespace pp
}  // namespace gpn
