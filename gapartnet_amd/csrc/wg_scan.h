// wg_scan.h — the integer sum and prefix sum of one workgroup: the only definition in the library.  Counting steps (rulebooks,
// sort-free voxelisation, cluster relabelling, re-voxelisation, mask proposals, scene maps, the point front ends) all end here.
// Integer arithmetic without overflow: any regrouping of the sums gives the same bits.
//   block_sum / block_scan   one value per thread
//   block_scan_tiled         n values streamed in tiles of 64 kWaves (arrays in global memory, coalesced)
//   block_scan_runs          an array in place, one contiguous run per thread (arrays in LDS)
// Every function contains barriers: the whole workgroup of kWaves waves calls it, and a loop around a call has a
// workgroup-uniform trip count.  T: int, uint32_t or long long.
#pragma once
#include "gpn_common.h"

namespace gpn {

// ---- one value per thread; wsum: kWaves values of LDS, free again when the call returns ------------------------------------------
// sum (every thread gets it)
template <int kWaves, typename T = int>
__device__ __forceinline__ T block_sum(T c, T* wsum) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  T tot = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) tot += wsum[w];
  __syncthreads();  // wsum is rewritten by the next call
  return tot;
}

// inclusive scan: -> (this thread's inclusive sum, the workgroup's total)
template <int kWaves, typename T = int>
__device__ __forceinline__ T block_scan(T c, T* wsum, T* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  T before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const T s = wsum[w];
    before += w < wave ? s : 0;
    tot += s;
  }
  __syncthreads();  // wsum is rewritten by the next call
  *total = tot;
  return before + incl;
}

// ---- tiled: out[i] = load(0) + ... + load(i - 1) for i < n, returns the total (to every thread) -----------------------------------
// Thread t takes element t of every tile; the carry between tiles is a register, since block_scan hands the tile's total to
// every thread.  `out` may be the array that `load` reads (a thread reads its element before it writes it).
template <int kWaves, typename T, typename Load>
__device__ __forceinline__ T block_scan_tiled(int64_t n, Load load, T* out, T* wsum) {
  T carry = 0;
  for (int64_t t0 = 0; t0 < n; t0 += 64 * kWaves) {
    const int64_t i = t0 + threadIdx.x;
    const T v = i < n ? (T)load(i) : (T)0;
    T total;
    const T incl = block_scan<kWaves>(v, wsum, &total);
    if (i < n) out[i] = carry + incl - v;
    carry += total;
  }
  return carry;
}

// ---- runs: a[0 .. n) -> its exclusive prefix in place, returns the total ----------------------------------------------------------
// Thread t owns the run [t len, (t + 1) len), len = ceil(n / threads).  a is complete when the call begins (the caller's barrier)
// and readable by every thread when it returns.
template <int kWaves, typename T>
__device__ __forceinline__ T block_scan_runs(T* a, int n, T* wsum) {
  const int len = (n + 64 * kWaves - 1) / (64 * kWaves);
  const int b = min((int)threadIdx.x * len, n), e = min(b + len, n);
  T sum = 0;
  for (int i = b; i < e; ++i) sum += a[i];
  T total;
  T run = block_scan<kWaves>(sum, wsum, &total) - sum;
  for (int i = b; i < e; ++i) {
    const T v = a[i];
    a[i] = run;
    run += v;
  }
  __syncthreads();
  return total;
}

}  // namespace gpn
