// point_prims.h — the building blocks the point front ends share (pointnet2.hip, viewprep.hip, cloudprep.hip, frameprep.hip,
// gridsample.hip): the no-fma distance, the seeded hash with the resolve step of its radix select,
// ballot-ordered ranks, the furthest-point-sampling candidate with its three reduction steps, and the ball normalisation.  Every one of them is pinned bit for bit by the oracle; this is their only definition.
#pragma once
#include "gpn_common.h"
#include "wg_scan.h"  // block_sum / block_scan: the workgroup integer sum and scan

namespace gpn {

// fp32 (dx^2 + dy^2) + dz^2, every operation rounded on its own
__device__ __forceinline__ float dist2_nofma(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ double wave_min(double a) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a = fmin(a, __shfl_xor(a, off, 64));
  return a;
}
__device__ __forceinline__ double wave_max(double a) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a = fmax(a, __shfl_xor(a, off, 64));
  return a;
}

// ---- seeded radix select (include/gpn.h sections FR and GS): the k smallest 64-bit keys (hash << 32) | item of a set -------------
__device__ __forceinline__ uint32_t hash_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// the hash of section FR, cut to its top hash_bits bits (1 .. 32)
__device__ __forceinline__ uint32_t hash_key(uint32_t seed, uint32_t item, int hash_bits) {
  const uint32_t h = hash_mix(hash_mix(item + seed * 0x9E3779B9u) ^ seed);
  return hash_bits >= 32 ? h : h >> (32 - hash_bits);
}

constexpr int kSelectPasses = 4;  // 32-bit hash, 8 bits a pass
constexpr int kSelectBins = 256;  // one histogram bin per thread of a 256-thread workgroup

// the digits of the k-th smallest hash that the first `npass` merged histograms fix (most significant first) and the rank left
// inside them.  Every thread returns the same values.  hist [kSelectPasses][kSelectBins] of the set; sh: 2 ints of LDS.
template <int kWaves>
__device__ __forceinline__ void select_resolve(const uint32_t* __restrict__ hist, int npass, int k, int* wsum, int* sh,
                                               uint32_t* prefix_out, int* k_out) {
  static_assert(kWaves * 64 == kSelectBins, "one histogram bin per thread in the resolve");
  uint32_t prefix = 0;
  for (int j = 0; j < npass; ++j) {
    if (threadIdx.x == 0) { sh[0] = kSelectBins - 1; sh[1] = 1; }  // (never read back unless the histogram is short of k)
    const int h = (int)hist[j * kSelectBins + threadIdx.x];
    int total;
    const int incl = block_scan<kWaves>(h, wsum, &total);  // (its barriers order the two writes to sh)
    if (incl - h < k && k <= incl) { sh[0] = threadIdx.x; sh[1] = k - (incl - h); }
    __syncthreads();
    prefix = (prefix << 8) | (uint32_t)sh[0];
    k = sh[1];
    __syncthreads();
  }
  *prefix_out = prefix;
  *k_out = k;
}

// A workgroup of kWaves waves holds kPer * 64 * kWaves slots, slot = e * 64 * kWaves + thread: the number of set flags in the
// slots before each of this thread's kPer slots (slot order: e first, then the wave, then the lane), plus `base`; returns the
// workgroup's count of set flags.  wcnt: LDS, free again when the call returns.
template <int kWaves, int kPer>
__device__ __forceinline__ int ordered_ranks(const bool (&f)[kPer], int (*wcnt)[kWaves] /* [kPer] */, int base, int (&rank)[kPer]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const unsigned long long b = __ballot(f[e]);
    rank[e] = __popcll(b & below);
    if (lane == 0) wcnt[e][wave] = __popcll(b);
  }
  __syncthreads();
  int before = base;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
#pragma unroll
    for (int w = 0; w < kWaves; ++w) before += w < wave ? wcnt[e][w] : 0;
    rank[e] += before;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) before += w >= wave ? wcnt[e][w] : 0;
  }
  __syncthreads();  // wcnt is rewritten by the next call
  return before - base;
}

// ---- furthest point sampling: the candidate (running distance, point index) and its reduction ---------------------------------
// The arg-max reproduces the reference's result (sampling_gpu.cu:93-209) for ITS block size Bref = opt_n_threads(n): highest
// distance, ties to the lowest reference thread id (k mod Bref) in the order of its tree, then to the lowest k.  A total order: any
// split of a cloud's points over threads, waves and workgroups gives the same winner.
struct FpsCand {
  float v;
  int k;
};

// opt_n_threads(n) - 1 (cuda_utils.h:10-14): the largest power of two <= n, at most 1024, less one.  The reference's
// (int)(log(n) / log(2)) equals floor(log2(n)) for every n in [1, 2^21] (tests/test_convert_cpu.py), and n >= 1024 gives 1024.
__host__ __device__ __forceinline__ int fps_bmask(int n) {
  const int v = n >= 1024 ? 1024 : (1 << (31 - __builtin_clz((unsigned)n)));
  return v - 1;
}

__device__ __forceinline__ bool fps_better(float av, int ak, float bv, int bk, int bmask) {
  if (av != bv) return av > bv;
  // the reference's tree (sampling_gpu.cu:143-200) merges slot j with j+s for s = B/2 ... 1 and keeps slot j on
  // ties, so two tied candidates are decided at the lowest bit where their thread ids differ, the 0-bit winning:
  // ascending order of the bit-reversed thread id
  const unsigned ta = __brev((unsigned)(ak & bmask)), tb = __brev((unsigned)(bk & bmask));
  if (ta != tb) return ta < tb;
  return ak < bk;
}

// the wave's best candidate, in lane 0
__device__ __forceinline__ FpsCand fps_wave_best(FpsCand c, int bmask) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_down(c.v, off, 64);
    const int ok = __shfl_down(c.k, off, 64);
    if (lane + off < 64 && fps_better(ov, ok, c.v, c.k, bmask)) { c.v = ov; c.k = ok; }
  }
  return c;
}

// the workgroup's best candidate, in lane 0 of wave 0 (other threads: unspecified); wv / wk: kWaves words of LDS each.  A barrier
// must separate the caller's reads of the result from the next call.
template <int kWaves>
__device__ __forceinline__ FpsCand fps_block_best(FpsCand c, int bmask, float* wv, int* wk) {
  static_assert(kWaves == 16, "the tree below folds 16 wave candidates");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  c = fps_wave_best(c, bmask);
  if (lane == 0) { wv[wave] = c.v; wk[wave] = c.k; }
  __syncthreads();
  if (wave == 0) {
    c.v = lane < kWaves ? wv[lane] : -2.f;
    c.k = lane < kWaves ? wk[lane] : 0x7fffffff;
#pragma unroll
    for (int off = kWaves / 2; off >= 1; off >>= 1) {
      const float ov = __shfl_down(c.v, off, 64);
      const int ok = __shfl_down(c.k, off, 64);
      if (fps_better(ov, ok, c.v, c.k, bmask)) { c.v = ov; c.k = ok; }
    }
  }
  return c;
}

// The j-th meeting (j = 1, 2, ...) of the G <= 64 workgroups that share a cloud, called by ONE whole wave of each: member w
// publishes its candidate (lane 0's `c`) in the double-buffered slot (j & 1) * G + w of cv / ck [2][G], all G meet at `counter`
// (zeroed by the host before the launch), and every member reduces the G candidates itself, so the winner (in lane 0) never has
// to be broadcast.  The counter is never reset: the j-th meeting waits for G * j (fps_meetings_fit bounds it).  Every workgroup
// of the launch must be resident: cooperative launches only (fps_launch).
__device__ __forceinline__ FpsCand fps_meet(FpsCand c, int j, int G, int w, int bmask, float* cv, int* ck, unsigned* counter) {
  const int lane = threadIdx.x & 63;
  const int slot = (j & 1) * G;
  if (lane == 0) {
    __hip_atomic_store(cv + slot + w, c.v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(ck + slot + w, c.k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned want = (unsigned)G * (unsigned)j;
    while (__hip_atomic_load(counter, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < want) __builtin_amdgcn_s_sleep(1);
    __threadfence();
  }
  // lane 0 has passed the barrier; the wave re-converges here and reads every workgroup's candidate
  __threadfence();  // every lane: the candidate reads below stay behind lane 0's acquire
  c.v = -2.f;
  c.k = 0x7fffffff;
  if (lane < G) {
    c.v = __hip_atomic_load(cv + slot + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c.k = __hip_atomic_load(ck + slot + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return fps_wave_best(c, bmask);
}

// ---- host side of fps_meet ------------------------------------------------------------------------------------------------------
// The bound on a launch's meetings: the 32-bit counter of fps_meet reaches (m - 1) * G; the host keeps m * G below 2^31.
inline bool fps_meetings_fit(int m, int G) { return (int64_t)m * G < (int64_t)0x7fffffff; }

// Launch an FPS kernel of 1024-thread workgroups for entry point `who`; `args` hold the kernels' (common) arguments, *G among them:
// the workgroups per cloud, grid = wgs_per_group * G.  *G > 1: zero the `counters` arrival counters and launch `shared`
// cooperatively - the runtime starts the grid only when ALL its workgroups can be resident at once (and refuses a grid that
// cannot be), which is what the in-kernel counter meeting needs: a plain launch next to other streams' kernels, other ranks
// sharing the device or a CU mask could leave some workgroups unscheduled while the resident ones spin.  Refused (not
// co-schedulable here: too large for this device / partition): the error is cleared and `single` runs with *G = 1, the form
// without any inter-workgroup wait.
inline int fps_launch(const char* who, const void* shared, const void* single, unsigned wgs_per_group, int* G, void** args,
                      unsigned* arrived, size_t counters, hipStream_t stream) {
  if (*G > 1) {
    hipError_t e = hipMemsetAsync(arrived, 0, counters * sizeof(unsigned), stream);
    if (e != hipSuccess) {
      gpn::set_error("%s: hipMemsetAsync of the arrival counters failed: %s", who, hipGetErrorString(e));
      return GPN_ERR_HIP;
    }
    if (hipLaunchCooperativeKernel(shared, dim3(wgs_per_group * (unsigned)*G), dim3(1024), args, 0, stream) == hipSuccess) return GPN_OK;
    (void)hipGetLastError();
    *G = 1;
  }
  hipError_t e = hipLaunchKernel(single, dim3(wgs_per_group), dim3(1024), args, 0, stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) {
    gpn::set_error("%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return GPN_ERR_HIP;
  }
  return GPN_OK;
}

// ---- ball normalisation (convert_rendered_into_input.py:71-87, FindMaxDis) -------------------------------------------------------
// Over the m >= 1 samples a workgroup of kWaves waves owns, float64: centre (max + min) / 2 per axis, r = sqrt(max((dx^2 + dy^2) +
// dz^2)) - to every thread.  sample(j, P) writes sample j's coordinates to double P[3]; it is called twice per sample.  Minima and
// maxima are exact in any order, and the square root is monotonic, so sqrt(max) = max(sqrt).  red: LDS, read until the return.
template <int kWaves, typename Sample>
__device__ __forceinline__ void ball_of_samples(Sample sample, int m, double (*red)[kWaves] /* [6] */, double ctr[3], double* r) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, threads = kWaves * 64;
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int j = tid; j < m; j += threads) {
    double P[3];
    sample(j, P);
#pragma unroll
    for (int c = 0; c < 3; ++c) { mn[c] = fmin(mn[c], P[c]); mx[c] = fmax(mx[c], P[c]); }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { mn[c] = wave_min(mn[c]); mx[c] = wave_max(mx[c]); }
  if (lane == 0)
    for (int c = 0; c < 3; ++c) { red[c][wave] = mn[c]; red[3 + c][wave] = mx[c]; }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double a = red[c][0], b = red[3 + c][0];
    for (int q = 1; q < kWaves; ++q) { a = fmin(a, red[c][q]); b = fmax(b, red[3 + c][q]); }
    ctr[c] = (b + a) / 2.0;
  }
  __syncthreads();  // red is reused below
  double r2 = -INFINITY;
  for (int j = tid; j < m; j += threads) {
    double P[3];
    sample(j, P);
    const double dx = P[0] - ctr[0], dy = P[1] - ctr[1], dz = P[2] - ctr[2];
    r2 = fmax(r2, (dx * dx + dy * dy) + dz * dz);
  }
  r2 = wave_max(r2);
  if (lane == 0) red[0][wave] = r2;
  __syncthreads();
  r2 = red[0][0];
  for (int q = 1; q < kWaves; ++q) r2 = fmax(r2, red[0][q]);
  *r = __dsqrt_rn(r2);
}

}  // namespace gpn
