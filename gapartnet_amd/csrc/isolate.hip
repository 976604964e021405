// isolate.hip — the object of a raw RGB-D frame (include/gpn.h section OB): seeded RANSAC planes, the cut at them, connected
// components of what is left and the choice of the object's component.  A batch of V frames of one size H x W, on the rows that
// gpn_frame_backproject wrote:
//   candidates   valid pixels inside a depth range
//   hypotheses   three hashed candidate pixels per hypothesis -> a float64 plane
//   score        a workgroup per 1024-pixel chunk stages its candidates' xyz in LDS as float64; a thread per hypothesis walks them
//                (every lane reads the same LDS address: a broadcast), counts in registers, one integer atomicAdd per hypothesis
//   winner       the largest count, ties to the lowest k: a 64-bit key under max
//   refit        per-chunk float64 partial sums about the winner's p0, added in chunk order; svd3 of the scatter; the inliers of
//                the refit counted; accepted or not on the device
//   cut          candidates strictly on the camera's side of an accepted plane stay
//   components   union-find: 16 x 16 tiles in LDS, tile borders merged by atomicMin on the global parent array, flatten.  parent[i]
//                <= i at every moment, so every find loop ends; no workgroup ever waits for another
//   select       largest / centre / all, by 64-bit keys under integer max / min
// No float atomics; integer atomics only where order cannot matter; no host read; every output bit-reproducible.
#include <cmath>

#include "gpn_common.h"
#include "point_prims.h"
#include "pose_math.h"

namespace {

using namespace gpn;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 4;  // pixels per thread: pixel = chunk * kChunk + e * kThreads + tid (the chunk of section FR)
constexpr int kChunk = kThreads * kPer;
constexpr int kTile = 16;  // components: a tile of kTile x kTile pixels per workgroup, a pixel per thread
constexpr int kTries = GPN_ISOLATE_TRIES;
constexpr int kMaxPlanes = GPN_ISOLATE_MAX_PLANES;
constexpr int kMaxHyp = GPN_ISOLATE_MAX_HYP;
constexpr int kSums = 9;  // sx sy sz, sxx sxy sxz syy syz szz

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ __forceinline__ double plane_dist(const double* pl, double x, double y, double z) {
  return ((pl[0] * x + pl[1] * y) + pl[2] * z) + pl[3];
}

// n . p + d = 0 with d > 0 (the camera on the positive side); false: d == 0 or not a number
__device__ __forceinline__ bool orient(double (&n)[3], double& d) {
  if (d < 0.0) {
    n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2];
    d = -d;
  }
  return d > 0.0;
}

// ---- 0. candidates ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ob_candidates_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ valid,
                                                                 int64_t total, double z_min, double z_max, uint8_t* __restrict__ cand) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= total) return;
  const double z = fabs((double)rows[g * 6 + 2]);
  cand[g] = (valid[g] != 0 && z >= z_min && z <= z_max) ? 1 : 0;  // (NaN fails both)
}

// ---- 1. hypotheses: a thread per (frame, k) --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ob_hypotheses_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ cand,
                                                                 const int32_t* __restrict__ pix, const int32_t* __restrict__ valid_counts,
                                                                 const uint32_t* __restrict__ seeds, int64_t HW, int n_hyp, int round,
                                                                 double* __restrict__ hyp, int32_t* __restrict__ hyp_pix) {
  const int v = blockIdx.y, k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n_hyp) return;
  const int nv = valid_counts[v];
  const uint32_t seed = seeds[v];
  int rank[3] = {-1, -1, -1}, px[3] = {-1, -1, -1};
  bool ok = nv >= 3 && (int64_t)nv <= HW;
  for (int j = 0; ok && j < 3; ++j) {
    const uint32_t c = 3u * (uint32_t)n_hyp * (uint32_t)round + 3u * (uint32_t)k + (uint32_t)j;
    for (int t = 0; t < kTries; ++t) {
      const uint32_t r = hash_key(seed, c + (uint32_t)t * (3u * (uint32_t)n_hyp * (uint32_t)kMaxPlanes), 32) % (uint32_t)nv;
      const int p = pix[(int64_t)v * HW + r];
      if (p >= 0 && p < HW && cand[(int64_t)v * HW + p]) {
        rank[j] = (int)r;
        px[j] = p;
        break;
      }
    }
    ok = px[j] >= 0;
  }
  ok = ok && rank[0] != rank[1] && rank[0] != rank[2] && rank[1] != rank[2];
  double n[3] = {0, 0, 0}, d = 0;
  if (ok) {
    double P[3][3];
    for (int j = 0; j < 3; ++j)
      for (int a = 0; a < 3; ++a) P[j][a] = (double)rows[((int64_t)v * HW + px[j]) * 6 + a];
    const double e1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
    const double e2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const double a2 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2], b2 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
    ok = nn > 1e-12 * (a2 * b2);  // (false for NaN)
    if (ok) {
      const double len = __dsqrt_rn(nn);
      n[0] = n[0] / len; n[1] = n[1] / len; n[2] = n[2] / len;
      d = -((n[0] * P[0][0] + n[1] * P[0][1]) + n[2] * P[0][2]);
      ok = orient(n, d);
    }
  }
  double* h = hyp + ((int64_t)v * n_hyp + k) * 4;
  h[0] = ok ? n[0] : nan64(); h[1] = ok ? n[1] : nan64(); h[2] = ok ? n[2] : nan64(); h[3] = ok ? d : nan64();
  hyp_pix[(int64_t)v * n_hyp + k] = ok ? px[0] : -1;
}

// the chunk's candidates, compacted into LDS as float64 (in pixel order); returns their number
__device__ __forceinline__ int stage_chunk(const float* __restrict__ rows, const uint8_t* __restrict__ cand, int v, int64_t HW,
                                           double* sx, double* sy, double* sz, int (*wcnt)[kWaves]) {
  bool f[kPer];
  int rank[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + threadIdx.x;
    f[e] = p < HW && cand[(int64_t)v * HW + p] != 0;
  }
  const int m = ordered_ranks<kWaves, kPer>(f, wcnt, 0, rank);
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    if (!f[e]) continue;
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + threadIdx.x;
    const float* q = rows + ((int64_t)v * HW + p) * 6;
    sx[rank[e]] = (double)q[0]; sy[rank[e]] = (double)q[1]; sz[rank[e]] = (double)q[2];  // (rank < m <= kChunk)
  }
  __syncthreads();
  return m;
}

// ---- 2. score: a workgroup per chunk, a thread per hypothesis ----------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ob_score_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ cand,
                                                            const double* __restrict__ hyp, int64_t HW, int n_hyp, double tol,
                                                            int32_t* __restrict__ counts) {
  __shared__ double sx[kChunk], sy[kChunk], sz[kChunk];
  __shared__ int wcnt[kPer][kWaves];
  const int v = blockIdx.y;
  const int m = stage_chunk(rows, cand, v, HW, sx, sy, sz, wcnt);
  if (m == 0) return;  // (uniform)
  for (int k = threadIdx.x; k < n_hyp; k += kThreads) {
    const double* h = hyp + ((int64_t)v * n_hyp + k) * 4;
    const double pl[4] = {h[0], h[1], h[2], h[3]};
    int c = 0;
    for (int i = 0; i < m; ++i) c += fabs(plane_dist(pl, sx[i], sy[i], sz[i])) <= tol ? 1 : 0;  // (NaN plane: 0)
    if (c) atomicAdd(counts + (int64_t)v * n_hyp + k, c);  // (an integer counter: order-free)
  }
}

// the other shape: a pixel per lane (kPer in registers), the hypotheses read from global memory (a scalar load: the address is
// uniform), ballot + popcount per hypothesis.  Kept for the comparison in tools/isolate_bench.py (variant 1).
__global__ __launch_bounds__(kThreads) void ob_score_ballot_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ cand,
                                                                   const double* __restrict__ hyp, int64_t HW, int n_hyp, double tol,
                                                                   int32_t* __restrict__ counts) {
  __shared__ int acc[kMaxHyp];
  const int v = blockIdx.y, tid = threadIdx.x;
  double X[kPer], Y[kPer], Z[kPer];
  bool f[kPer];
  for (int k = tid; k < n_hyp; k += kThreads) acc[k] = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    f[e] = p < HW && cand[(int64_t)v * HW + p] != 0;
    const float* q = rows + ((int64_t)v * HW + (f[e] ? p : 0)) * 6;
    X[e] = (double)q[0]; Y[e] = (double)q[1]; Z[e] = (double)q[2];
  }
  __syncthreads();
  for (int k = 0; k < n_hyp; ++k) {
    const double* h = hyp + ((int64_t)v * n_hyp + k) * 4;
    const double pl[4] = {h[0], h[1], h[2], h[3]};
    int c = 0;
#pragma unroll
    for (int e = 0; e < kPer; ++e) c += __popcll(__ballot(f[e] && fabs(plane_dist(pl, X[e], Y[e], Z[e])) <= tol));
    if ((tid & 63) == 0 && c) atomicAdd(&acc[k], c);
  }
  __syncthreads();
  for (int k = tid; k < n_hyp; k += kThreads)
    if (acc[k]) atomicAdd(counts + (int64_t)v * n_hyp + k, acc[k]);
}

// ---- winner: a workgroup per frame ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ob_winner_kernel(const int32_t* __restrict__ counts, int n_hyp, int32_t* __restrict__ winner) {
  __shared__ unsigned long long best[kThreads];
  const int v = blockIdx.x, tid = threadIdx.x;
  unsigned long long b = 0;
  for (int k = tid; k < n_hyp; k += kThreads) {
    const int c = counts[(int64_t)v * n_hyp + k];
    if (c > 0) {
      const unsigned long long key = ((unsigned long long)(uint32_t)c << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)k);
      b = key > b ? key : b;
    }
  }
  best[tid] = b;
  __syncthreads();
  for (int s = kThreads / 2; s >= 1; s >>= 1) {
    if (tid < s && best[tid + s] > best[tid]) best[tid] = best[tid + s];
    __syncthreads();
  }
  if (tid == 0) winner[v] = best[0] ? (int)(0xFFFFFFFFu - (uint32_t)(best[0] & 0xFFFFFFFFull)) : -1;
}

// ---- 3. refit --------------------------------------------------------------------------------------------------------------------
// per chunk: the float64 sums of the winner's inliers about its p0, their number and the chunk's candidates
__global__ __launch_bounds__(kThreads) void ob_refit_sums_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ cand,
                                                                 const double* __restrict__ hyp, const int32_t* __restrict__ hyp_pix,
                                                                 const int32_t* __restrict__ winner, int64_t HW, int n_hyp, double tol,
                                                                 double* __restrict__ part, int32_t* __restrict__ part_n) {
  __shared__ double red[kWaves * kSums];
  __shared__ int wsum[kWaves];
  const int v = blockIdx.y, tid = threadIdx.x;
  const int64_t ci = (int64_t)v * gridDim.x + blockIdx.x;
  const int w = winner[v];
  const bool have = w >= 0 && w < n_hyp && hyp_pix[(int64_t)v * n_hyp + (w >= 0 && w < n_hyp ? w : 0)] >= 0;
  double pl[4] = {0, 0, 0, 0}, p0[3] = {0, 0, 0};
  if (have) {
    const int px = hyp_pix[(int64_t)v * n_hyp + w];
    for (int a = 0; a < 4; ++a) pl[a] = hyp[((int64_t)v * n_hyp + w) * 4 + a];
    for (int a = 0; a < 3; ++a) p0[a] = px < HW ? (double)rows[((int64_t)v * HW + px) * 6 + a] : 0.0;
  }
  double s[kSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int n_in = 0, n_cand = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (p >= HW || !cand[(int64_t)v * HW + p]) continue;
    ++n_cand;
    if (!have) continue;
    const float* q = rows + ((int64_t)v * HW + p) * 6;
    const double x = (double)q[0], y = (double)q[1], z = (double)q[2];
    if (!(fabs(plane_dist(pl, x, y, z)) <= tol)) continue;
    ++n_in;
    const double dx = x - p0[0], dy = y - p0[1], dz = z - p0[2];
    s[0] += dx; s[1] += dy; s[2] += dz;
    s[3] += dx * dx; s[4] += dx * dy; s[5] += dx * dz;
    s[6] += dy * dy; s[7] += dy * dz; s[8] += dz * dz;
  }
  block_reduce<kSums>(s, red, SumOp());
  n_in = block_sum<kWaves>(n_in, wsum);
  n_cand = block_sum<kWaves>(n_cand, wsum);
  if (tid < kSums) part[ci * kSums + tid] = s[tid];
  if (tid == 0) { part_n[ci * 2] = n_in; part_n[ci * 2 + 1] = n_cand; }
}

// per frame: the partials added in chunk order, the scatter's smallest singular vector, the plane
__global__ __launch_bounds__(64) void ob_refit_solve_kernel(const float* __restrict__ rows, const int32_t* __restrict__ hyp_pix,
                                                            const int32_t* __restrict__ winner, int64_t HW, int n_hyp, int nchunk,
                                                            const double* __restrict__ part, const int32_t* __restrict__ part_n,
                                                            double* __restrict__ fit, int32_t* __restrict__ fit_n) {
  __shared__ double tot[kSums];
  __shared__ int ntot[2];
  const int v = blockIdx.x, tid = threadIdx.x;
  if (tid < kSums) {
    double a = 0.0;
    for (int c = 0; c < nchunk; ++c) a += part[((int64_t)v * nchunk + c) * kSums + tid];
    tot[tid] = a;
  } else if (tid < kSums + 2) {
    int a = 0;
    for (int c = 0; c < nchunk; ++c) a += part_n[((int64_t)v * nchunk + c) * 2 + (tid - kSums)];
    ntot[tid - kSums] = a;
  }
  __syncthreads();
  if (tid != 0) return;
  const int w = winner[v];
  const int n_in = ntot[0];
  double n[3] = {nan64(), nan64(), nan64()}, d = nan64();
  bool ok = w >= 0 && w < n_hyp && n_in >= 3;
  if (ok) {
    const int px = hyp_pix[(int64_t)v * n_hyp + w];
    ok = px >= 0 && px < HW;
    if (ok) {
      const double cnt = (double)n_in;
      double mean[3];
      for (int a = 0; a < 3; ++a) mean[a] = (double)rows[((int64_t)v * HW + px) * 6 + a] + tot[a] / cnt;
      M3 C, U, Vm;
      double S[3];
      C.a[0][0] = tot[3] - tot[0] * tot[0] / cnt;
      C.a[0][1] = C.a[1][0] = tot[4] - tot[0] * tot[1] / cnt;
      C.a[0][2] = C.a[2][0] = tot[5] - tot[0] * tot[2] / cnt;
      C.a[1][1] = tot[6] - tot[1] * tot[1] / cnt;
      C.a[1][2] = C.a[2][1] = tot[7] - tot[1] * tot[2] / cnt;
      C.a[2][2] = tot[8] - tot[2] * tot[2] / cnt;
      svd3(C, U, S, Vm);
      n[0] = Vm.a[0][2]; n[1] = Vm.a[1][2]; n[2] = Vm.a[2][2];
      const double len = __dsqrt_rn((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
      n[0] = n[0] / len; n[1] = n[1] / len; n[2] = n[2] / len;
      d = -((n[0] * mean[0] + n[1] * mean[1]) + n[2] * mean[2]);
      ok = orient(n, d);
    }
  }
  double* f = fit + (int64_t)v * 4;
  f[0] = ok ? n[0] : nan64(); f[1] = ok ? n[1] : nan64(); f[2] = ok ? n[2] : nan64(); f[3] = ok ? d : nan64();
  fit_n[v * 2] = 0;            // the refit's inliers: counted by the next launch
  fit_n[v * 2 + 1] = ntot[1];  // the frame's candidates
}

__global__ __launch_bounds__(kThreads) void ob_refit_count_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ cand,
                                                                  const double* __restrict__ fit, int64_t HW, double tol,
                                                                  int32_t* __restrict__ fit_n) {
  __shared__ int wsum[kWaves];
  const int v = blockIdx.y, tid = threadIdx.x;
  const double pl[4] = {fit[v * 4], fit[v * 4 + 1], fit[v * 4 + 2], fit[v * 4 + 3]};
  int c = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (p >= HW || !cand[(int64_t)v * HW + p]) continue;
    const float* q = rows + ((int64_t)v * HW + p) * 6;
    c += fabs(plane_dist(pl, (double)q[0], (double)q[1], (double)q[2])) <= tol ? 1 : 0;
  }
  c = block_sum<kWaves>(c, wsum);
  if (tid == 0 && c) atomicAdd(fit_n + v * 2, c);  // (an integer counter: order-free)
}

__global__ __launch_bounds__(kThreads) void ob_refit_accept_kernel(const double* __restrict__ fit, const int32_t* __restrict__ fit_n, int V,
                                                                   double min_plane_fraction, int round, int max_planes,
                                                                   double* __restrict__ planes, int32_t* __restrict__ plane_inliers,
                                                                   int32_t* __restrict__ n_planes) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= V) return;
  const int n_in = fit_n[v * 2], n_cand = fit_n[v * 2 + 1];
  const bool ok = n_in >= 3 && (double)n_in >= min_plane_fraction * (double)n_cand && fit[v * 4 + 3] > 0.0;
  double* pl = planes + ((int64_t)v * max_planes + round) * 4;
  for (int a = 0; a < 4; ++a) pl[a] = ok ? fit[v * 4 + a] : nan64();
  plane_inliers[(int64_t)v * max_planes + round] = ok ? n_in : 0;
  if (round == 0) n_planes[v] = ok ? 1 : 0;
  else if (ok) n_planes[v] += 1;  // (this thread owns frame v)
}

// ---- 4. cut ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ob_cut_kernel(const float* __restrict__ rows, const double* __restrict__ planes, int64_t HW,
                                                          int max_planes, int round, double tol, uint8_t* __restrict__ cand) {
  const int v = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const double* h = planes + ((int64_t)v * max_planes + round) * 4;
  const double pl[4] = {h[0], h[1], h[2], h[3]};
  if (p >= HW || !(pl[3] > 0.0)) return;  // (a round that was not accepted leaves the frame untouched)
  const int64_t g = (int64_t)v * HW + p;
  if (!cand[g]) return;
  const float* q = rows + g * 6;
  if (!(plane_dist(pl, (double)q[0], (double)q[1], (double)q[2]) > tol)) cand[g] = 0;
}

// ---- 5. components ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool linked(double za, double zb, double jump_abs, double jump_rel) {
  return fabs(za - zb) <= jump_abs + jump_rel * fmin(za, zb);
}

// union of the sets of a and b in the LDS array L (L[i] <= i always, so every walk goes down and ends)
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
  while (true) {
    while (true) { const int pa = ((volatile int*)L)[a]; if (pa == a) break; a = pa; }
    while (true) { const int pb = ((volatile int*)L)[b]; if (pb == b) break; b = pb; }
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[b], a);  // (min by integer compare: order-free)
    if (old == b) return;
    b = old;  // b had a parent by now: join that one
  }
}

__device__ __forceinline__ int glb_find(int32_t* parent, int a) {
  while (true) {
    const int pa = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pa == a || pa < 0) return a;  // (pa < 0 cannot happen for a candidate; it ends the walk all the same)
    a = pa;
  }
}
__device__ __forceinline__ void glb_union(int32_t* parent, int a, int b) {
  while (true) {
    a = glb_find(parent, a);
    b = glb_find(parent, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + b, a);
    if (old == b) return;
    b = old;
  }
}

// a tile per workgroup: labels of the tile's own components, as frame pixel indices of their first pixel
__global__ __launch_bounds__(kTile * kTile) void ob_cc_tile_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ cand,
                                                                   int H, int W, double jump_abs, double jump_rel,
                                                                   int32_t* __restrict__ labels) {
  __shared__ int L[kTile * kTile];
  __shared__ double Z[kTile * kTile];
  const int v = blockIdx.z, tid = threadIdx.x, lx = tid % kTile, ly = tid / kTile;
  const int x = blockIdx.x * kTile + lx, y = blockIdx.y * kTile + ly;
  const int64_t HW = (int64_t)H * W;
  const bool in = x < W && y < H;
  const int64_t g = (int64_t)v * HW + (in ? (int64_t)y * W + x : 0);
  const bool c = in && cand[g] != 0;
  Z[tid] = c ? fabs((double)rows[g * 6 + 2]) : -1.0;
  L[tid] = tid;
  __syncthreads();
  if (c) {
    if (lx + 1 < kTile && Z[tid + 1] >= 0.0 && linked(Z[tid], Z[tid + 1], jump_abs, jump_rel)) lds_union(L, tid, tid + 1);
    if (ly + 1 < kTile && Z[tid + kTile] >= 0.0 && linked(Z[tid], Z[tid + kTile], jump_abs, jump_rel)) lds_union(L, tid, tid + kTile);
  }
  __syncthreads();
  if (!in) return;
  int r = tid;
  while (L[r] != r) r = L[r];
  labels[g] = c ? (int)((int64_t)(blockIdx.y * kTile + r / kTile) * W + (blockIdx.x * kTile + r % kTile)) : -1;
}

// the links that cross a tile border, a pixel per thread
__global__ __launch_bounds__(kThreads) void ob_cc_border_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ cand, int H, int W,
                                                                double jump_abs, double jump_rel, int32_t* __restrict__ labels) {
  const int v = blockIdx.y;
  const int64_t HW = (int64_t)H * W, p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= HW) return;
  const int x = (int)(p % W), y = (int)(p / W);
  const bool right = x % kTile == kTile - 1 && x + 1 < W, down = y % kTile == kTile - 1 && y + 1 < H;
  if (!right && !down) return;
  const int64_t g = (int64_t)v * HW + p;
  if (!cand[g]) return;
  const double z = fabs((double)rows[g * 6 + 2]);
  int32_t* parent = labels + (int64_t)v * HW;
  if (right && cand[g + 1] && linked(z, fabs((double)rows[(g + 1) * 6 + 2]), jump_abs, jump_rel)) glb_union(parent, (int)p, (int)p + 1);
  if (down && cand[g + W] && linked(z, fabs((double)rows[(g + W) * 6 + 2]), jump_abs, jump_rel)) glb_union(parent, (int)p, (int)p + W);
}

// every pixel takes its root (no union runs beside this launch: the roots are final); sizes by integer adds at the root
__global__ __launch_bounds__(kThreads) void ob_cc_flatten_kernel(int64_t HW, int32_t* __restrict__ labels, int32_t* __restrict__ sizes) {
  const int v = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= HW) return;
  int32_t* parent = labels + (int64_t)v * HW;
  if (__hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
  const int r = glb_find(parent, (int)p);
  if (r != (int)p) __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (an ancestor for an ancestor; a root keeps itself)
  atomicAdd(sizes + (int64_t)v * HW + r, 1);
}

__global__ __launch_bounds__(kThreads) void ob_cc_count_kernel(int64_t HW, const int32_t* __restrict__ labels, const int32_t* __restrict__ sizes,
                                                               int min_pixels, int32_t* __restrict__ n_components) {
  __shared__ int wsum[kWaves];
  const int v = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int c = 0;
  if (p < HW && labels[(int64_t)v * HW + p] == (int)p && sizes[(int64_t)v * HW + p] >= min_pixels) c = 1;
  c = block_sum<kWaves>(c, wsum);
  if (threadIdx.x == 0 && c) atomicAdd(n_components + v, c);
}

// ---- 6. select -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clamp_anchor(int a) { return a < -16384 ? -16384 : (a > 32767 ? 32767 : a); }

__global__ __launch_bounds__(kThreads) void ob_select_key_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ sizes,
                                                                 const int32_t* __restrict__ anchor, int64_t HW, int W, int select,
                                                                 int min_pixels, unsigned long long* __restrict__ best) {
  const int v = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= HW) return;
  const int lab = labels[(int64_t)v * HW + p];
  if (lab < 0 || lab >= HW) return;
  const int sz = sizes[(int64_t)v * HW + lab];
  if (sz < min_pixels) return;
  if (select == GPN_ISOLATE_SELECT_CENTER) {
    const long long dx = (long long)(p % W) - clamp_anchor(anchor[v * 2]), dy = (long long)(p / W) - clamp_anchor(anchor[v * 2 + 1]);
    const unsigned long long key = ((unsigned long long)(dx * dx + dy * dy) << 32) | (unsigned long long)p;
    atomicMin(best + v, key);
  } else if (lab == (int)p) {
    const unsigned long long key = ((unsigned long long)(uint32_t)sz << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)p);
    atomicMax(best + v, key);
  }
}

__global__ __launch_bounds__(kThreads) void ob_select_keep_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ sizes,
                                                                  const int32_t* __restrict__ n_planes, int64_t HW, int select, int min_pixels,
                                                                  const unsigned long long* __restrict__ best, uint8_t* __restrict__ keep,
                                                                  int32_t* __restrict__ chosen, int32_t* __restrict__ status) {
  const int v = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long b = best[v];
  int root = -1;
  if (select == GPN_ISOLATE_SELECT_CENTER) {
    if (b != ~0ull) root = labels[(int64_t)v * HW + (int64_t)(b & 0xFFFFFFFFull)];
  } else if (b != 0ull) {
    root = (int)(0xFFFFFFFFu - (uint32_t)(b & 0xFFFFFFFFull));
  }
  if (p == 0) {
    chosen[v] = root;
    status[v] = root < 0 ? GPN_ISOLATE_EMPTY : (n_planes[v] > 0 ? GPN_ISOLATE_OK : GPN_ISOLATE_NO_PLANE);
  }
  if (p >= HW) return;
  const int lab = labels[(int64_t)v * HW + p];
  bool k = false;
  if (lab >= 0 && lab < HW && root >= 0) k = select == GPN_ISOLATE_SELECT_ALL ? sizes[(int64_t)v * HW + lab] >= min_pixels : lab == root;
  keep[(int64_t)v * HW + p] = k ? 1 : 0;
}

inline bool frames_ok(int V, int H, int W) {
  return V >= 0 && V <= 65535 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && (int64_t)H * W < (int64_t)0x7fffffff - kChunk &&
         (int64_t)V * H * W < ((int64_t)1 << 40);
}
inline bool finite_nonneg(double x) { return x >= 0.0 && x < (double)INFINITY; }

}  // namespace

extern "C" int gpn_frame_candidates(const float* rows, const uint8_t* valid, int V, int H, int W, double z_min, double z_max,
                                    uint8_t* cand, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(frames_ok(V, H, W));
  GPN_CHECK_ARG(z_min >= 0.0 && z_max >= z_min);  // (z_max may be +inf; NaN fails)
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(rows && valid && cand);
  const int64_t total = (int64_t)V * H * W;
  hipLaunchKernelGGL(ob_candidates_kernel, dim3((unsigned)gpn::cdiv(total, kThreads)), dim3(kThreads), 0, stream, rows, valid, total,
                     z_min, z_max, cand);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_frame_plane_hypotheses(const float* rows, const uint8_t* cand, const int32_t* pix, const int32_t* valid_counts,
                                          const uint32_t* seeds, int V, int H, int W, int n_hyp, int round, double* hyp,
                                          int32_t* hyp_pix, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(frames_ok(V, H, W));
  GPN_CHECK_ARG(n_hyp >= 1 && n_hyp <= kMaxHyp && round >= 0 && round < kMaxPlanes);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(rows && cand && pix && valid_counts && seeds && hyp && hyp_pix);
  hipLaunchKernelGGL(ob_hypotheses_kernel, dim3((unsigned)gpn::cdiv(n_hyp, kThreads), (unsigned)V), dim3(kThreads), 0, stream, rows, cand,
                     pix, valid_counts, seeds, (int64_t)H * W, n_hyp, round, hyp, hyp_pix);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_frame_plane_score(const float* rows, const uint8_t* cand, const double* hyp, int V, int H, int W, int n_hyp,
                                     double tol, int variant, int32_t* counts, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(frames_ok(V, H, W));
  GPN_CHECK_ARG(n_hyp >= 1 && n_hyp <= kMaxHyp && finite_nonneg(tol) && (variant == 0 || variant == 1));
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(rows && cand && hyp && counts);
  const int64_t HW = (int64_t)H * W;
  GPN_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)V * n_hyp * sizeof(int32_t), stream));
  const dim3 grid((unsigned)gpn::cdiv(HW, kChunk), (unsigned)V);
  if (variant == 0)
    hipLaunchKernelGGL(ob_score_kernel, grid, dim3(kThreads), 0, stream, rows, cand, hyp, HW, n_hyp, tol, counts);
  else
    hipLaunchKernelGGL(ob_score_ballot_kernel, grid, dim3(kThreads), 0, stream, rows, cand, hyp, HW, n_hyp, tol, counts);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_frame_plane_winner(const int32_t* counts, int V, int n_hyp, int32_t* winner, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(V >= 0 && V <= 65535 && n_hyp >= 1 && n_hyp <= kMaxHyp);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(counts && winner);
  hipLaunchKernelGGL(ob_winner_kernel, dim3((unsigned)V), dim3(kThreads), 0, stream, counts, n_hyp, winner);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" size_t gpn_frame_plane_refit_ws_bytes(int V, int H, int W) {
  if (V <= 0 || H <= 0 || W <= 0) return 0;
  const size_t nchunk = (size_t)gpn::cdiv((int64_t)H * W, kChunk);
  return gpn::align_up((size_t)V * nchunk * kSums * sizeof(double)) + gpn::align_up((size_t)V * nchunk * 2 * sizeof(int32_t)) +
         gpn::align_up((size_t)V * 4 * sizeof(double)) + gpn::align_up((size_t)V * 2 * sizeof(int32_t));
}

extern "C" int gpn_frame_plane_refit(const float* rows, const uint8_t* cand, const double* hyp, const int32_t* hyp_pix,
                                     const int32_t* winner, int V, int H, int W, int n_hyp, double tol, double min_plane_fraction,
                                     int round, int max_planes, double* planes, int32_t* plane_inliers, int32_t* n_planes, void* ws,
                                     size_t ws_bytes, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(frames_ok(V, H, W));
  GPN_CHECK_ARG(n_hyp >= 1 && n_hyp <= kMaxHyp && finite_nonneg(tol) && min_plane_fraction >= 0.0 && min_plane_fraction <= 1.0);
  GPN_CHECK_ARG(max_planes >= 1 && max_planes <= kMaxPlanes && round >= 0 && round < max_planes);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(rows && cand && hyp && hyp_pix && winner && planes && plane_inliers && n_planes);
  const int64_t HW = (int64_t)H * W, nchunk = gpn::cdiv(HW, kChunk);
  gpn::WsCarver carve(ws, ws_bytes);
  double* part = carve.take<double>((size_t)V * nchunk * kSums);
  int32_t* part_n = carve.take<int32_t>((size_t)V * nchunk * 2);
  double* fit = carve.take<double>((size_t)V * 4);
  int32_t* fit_n = carve.take<int32_t>((size_t)V * 2);
  GPN_CHECK_WS(carve);
  const dim3 grid((unsigned)nchunk, (unsigned)V);
  hipLaunchKernelGGL(ob_refit_sums_kernel, grid, dim3(kThreads), 0, stream, rows, cand, hyp, hyp_pix, winner, HW, n_hyp, tol, part, part_n);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(ob_refit_solve_kernel, dim3((unsigned)V), dim3(64), 0, stream, rows, hyp_pix, winner, HW, n_hyp, (int)nchunk, part,
                     part_n, fit, fit_n);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(ob_refit_count_kernel, grid, dim3(kThreads), 0, stream, rows, cand, fit, HW, tol, fit_n);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(ob_refit_accept_kernel, dim3((unsigned)gpn::cdiv(V, kThreads)), dim3(kThreads), 0, stream, fit, fit_n, V,
                     min_plane_fraction, round, max_planes, planes, plane_inliers, n_planes);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_frame_plane_cut(const float* rows, const double* planes, int V, int H, int W, int max_planes, int round, double tol,
                                   uint8_t* cand, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(frames_ok(V, H, W));
  GPN_CHECK_ARG(finite_nonneg(tol) && max_planes >= 1 && max_planes <= kMaxPlanes && round >= 0 && round < max_planes);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(rows && planes && cand);
  const int64_t HW = (int64_t)H * W;
  hipLaunchKernelGGL(ob_cut_kernel, dim3((unsigned)gpn::cdiv(HW, kThreads), (unsigned)V), dim3(kThreads), 0, stream, rows, planes, HW,
                     max_planes, round, tol, cand);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_frame_components(const float* rows, const uint8_t* cand, int V, int H, int W, double jump_abs, double jump_rel,
                                    int min_pixels, int32_t* labels, int32_t* sizes, int32_t* n_components, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(frames_ok(V, H, W));
  GPN_CHECK_ARG(finite_nonneg(jump_abs) && finite_nonneg(jump_rel) && min_pixels >= 1);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(rows && cand && labels && sizes && n_components);
  const int64_t HW = (int64_t)H * W;
  GPN_CHECK_HIP(hipMemsetAsync(sizes, 0, (size_t)V * HW * sizeof(int32_t), stream));
  GPN_CHECK_HIP(hipMemsetAsync(n_components, 0, (size_t)V * sizeof(int32_t), stream));
  const dim3 pixels((unsigned)gpn::cdiv(HW, kThreads), (unsigned)V);
  hipLaunchKernelGGL(ob_cc_tile_kernel, dim3((unsigned)gpn::cdiv(W, kTile), (unsigned)gpn::cdiv(H, kTile), (unsigned)V), dim3(kTile * kTile), 0,
                     stream, rows, cand, H, W, jump_abs, jump_rel, labels);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(ob_cc_border_kernel, pixels, dim3(kThreads), 0, stream, rows, cand, H, W, jump_abs, jump_rel, labels);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(ob_cc_flatten_kernel, pixels, dim3(kThreads), 0, stream, HW, labels, sizes);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(ob_cc_count_kernel, pixels, dim3(kThreads), 0, stream, HW, labels, sizes, min_pixels, n_components);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" size_t gpn_frame_component_select_ws_bytes(int V) { return V <= 0 ? 0 : gpn::align_up((size_t)V * sizeof(unsigned long long)); }

extern "C" int gpn_frame_component_select(const int32_t* labels, const int32_t* sizes, const int32_t* n_planes, const int32_t* anchor,
                                          int V, int H, int W, int select, int min_pixels, uint8_t* keep, int32_t* chosen,
                                          int32_t* status, void* ws, size_t ws_bytes, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(frames_ok(V, H, W));
  GPN_CHECK_ARG(select == GPN_ISOLATE_SELECT_LARGEST || select == GPN_ISOLATE_SELECT_CENTER || select == GPN_ISOLATE_SELECT_ALL);
  GPN_CHECK_ARG(min_pixels >= 1);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(labels && sizes && n_planes && keep && chosen && status && (select != GPN_ISOLATE_SELECT_CENTER || anchor));
  gpn::WsCarver carve(ws, ws_bytes);
  unsigned long long* best = carve.take<unsigned long long>((size_t)V);
  GPN_CHECK_WS(carve);
  const int64_t HW = (int64_t)H * W;
  GPN_CHECK_HIP(hipMemsetAsync(best, select == GPN_ISOLATE_SELECT_CENTER ? 0xff : 0, (size_t)V * sizeof(unsigned long long), stream));
  const dim3 pixels((unsigned)gpn::cdiv(HW, kThreads), (unsigned)V);
  hipLaunchKernelGGL(ob_select_key_kernel, pixels, dim3(kThreads), 0, stream, labels, sizes, anchor, HW, W, select, min_pixels, best);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(ob_select_keep_kernel, pixels, dim3(kThreads), 0, stream, labels, sizes, n_planes, HW, select, min_pixels, best, keep,
                     chosen, status);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
