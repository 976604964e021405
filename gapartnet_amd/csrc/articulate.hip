// articulate.hip — the parts of two frames of one scene, associated and cut out for the joint kernels (include/gpn.h section AR).
// A batch of V frame pairs of one size H x W, at most GPN_PARTS_MAX parts a frame:
//   overlap  the contingency table of the two instance maps: inter [V,PA,PB], area_a [V,PA], area_b [V,PB].  One workgroup per chunk
//            of 1024 pixels (the chunk of frameprep.hip); a PA x PB histogram in LDS.  The maps are piecewise constant, so a wave
//            first groups its lanes by key (ballots) and adds each group's popcount with ONE LDS atomic; non-zero bins are merged
//            into the frame pair's table by integer global adds.
//   match    greedy one-to-one matching by exact IoU: one workgroup a frame pair, the table in LDS, one arg-max a round.
//   gather   a stable multi-way partition of every frame's pixels by part: per-chunk per-part counts, one scan over the chunks per
//            (frame, part), then ordered stores - the rank of a pixel among the earlier pixels of its own part comes from ballots
//            over equal keys inside a wave and from LDS counters added in (slot, wave) order across the chunk.
// No float atomics; integer atomics only on histograms (order-free); no host read; every result is independent of timing.
#include "gpn_common.h"
#include "wg_scan.h"

namespace {

using namespace gpn;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 4;  // pixels per thread: pixel = chunk * kChunk + e * kThreads + tid
constexpr int kChunk = kThreads * kPer;
constexpr int kMaxP = GPN_PARTS_MAX;
constexpr int kGroupRounds = 8;  // key groups a wave resolves by ballots before its remaining lanes add one by one

// the membership rule: the part of pixel g, or -1.  n is the frame's live part count, already clamped to the table width.
__device__ __forceinline__ int part_key(const int32_t* __restrict__ inst, const uint8_t* __restrict__ valid, int64_t g, bool inside,
                                        int n) {
  if (!inside) return -1;
  const int p = inst[g];
  return (valid[g] != 0 && p >= 0 && p < n) ? p : -1;
}

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

// the lanes of the wave whose key (0 .. 63, `ok` lanes only) equals this lane's: seven ballots.  0 for a lane that is not ok.
__device__ __forceinline__ unsigned long long wave_match6(int key, bool ok) {
  unsigned long long same = __ballot(ok);
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const bool bit = ((key >> b) & 1) != 0;
    const unsigned long long m = __ballot(ok && bit);
    same &= bit ? m : ~m;
  }
  return ok ? same : 0ull;
}

// ---- overlap ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ar_overlap_kernel(const int32_t* __restrict__ inst_a, const uint8_t* __restrict__ valid_a,
                                                              const int32_t* __restrict__ n_a, const int32_t* __restrict__ inst_b,
                                                              const uint8_t* __restrict__ valid_b, const int32_t* __restrict__ n_b,
                                                              int64_t HW, int PA, int PB, int32_t* __restrict__ inter,
                                                              int32_t* __restrict__ area_a, int32_t* __restrict__ area_b) {
  __shared__ int hist[kMaxP * kMaxP];
  __shared__ int ha[kMaxP], hb[kMaxP];
  const int v = blockIdx.y, tid = threadIdx.x;
  const int na = min(max(n_a[v], 0), PA), nb = min(max(n_b[v], 0), PB);
  const int nbins = PA * PB;
  for (int i = tid; i < nbins; i += kThreads) hist[i] = 0;
  if (tid < kMaxP) { ha[tid] = 0; hb[tid] = 0; }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    const bool inside = p < HW;
    const int64_t g = (int64_t)v * HW + p;
    const int ka = part_key(inst_a, valid_a, g, inside, na), kb = part_key(inst_b, valid_b, g, inside, nb);
    wave_hist_add(ha, ka);
    wave_hist_add(hb, kb);
    wave_hist_add(hist, (ka >= 0 && kb >= 0) ? ka * PB + kb : -1);
  }
  __syncthreads();
  // (merged by integer adds: order-free)
  for (int i = tid; i < nbins; i += kThreads) {
    const int c = hist[i];
    if (c) atomicAdd(inter + (int64_t)v * nbins + i, c);
  }
  if (tid < PA && ha[tid]) atomicAdd(area_a + (int64_t)v * PA + tid, ha[tid]);
  if (tid < PB && hb[tid]) atomicAdd(area_b + (int64_t)v * PB + tid, hb[tid]);
}

// ---- match ------------------------------------------------------------------------------------------------------------------------
struct Cand {
  int inter, uni, e;  // e = i * PB + j, -1 = none
};
// a better than b: the larger IoU by 64-bit cross-multiplication, ties to the smaller (i, j)
__device__ __forceinline__ bool cand_better(const Cand& a, const Cand& b) {
  if (a.e < 0) return false;
  if (b.e < 0) return true;
  const long long l = (long long)a.inter * b.uni, r = (long long)b.inter * a.uni;
  if (l != r) return l > r;
  return a.e < b.e;
}

__global__ __launch_bounds__(kThreads) void ar_match_kernel(const int32_t* __restrict__ inter, const int32_t* __restrict__ area_a,
                                                            const int32_t* __restrict__ area_b, const int32_t* __restrict__ n_a,
                                                            const int32_t* __restrict__ n_b, const int32_t* __restrict__ cls_a,
                                                            const int32_t* __restrict__ cls_b, double min_iou, int PA, int PB,
                                                            int32_t* __restrict__ match_ab, int32_t* __restrict__ match_ba,
                                                            int32_t* __restrict__ n_matched, int32_t* __restrict__ m_inter,
                                                            int32_t* __restrict__ m_union) {
  __shared__ int tab[kMaxP * kMaxP];  // inter of the eligible pairs, 0 elsewhere
  __shared__ int aa[kMaxP], ab[kMaxP], mab[kMaxP], mba[kMaxP], mi[kMaxP], mu[kMaxP];
  __shared__ Cand wbest[kWaves];
  __shared__ int won;
  const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int na = min(max(n_a[v], 0), PA), nb = min(max(n_b[v], 0), PB);
  const int nbins = PA * PB;
  if (tid < kMaxP) {
    aa[tid] = tid < na ? area_a[(int64_t)v * PA + tid] : 0;
    ab[tid] = tid < nb ? area_b[(int64_t)v * PB + tid] : 0;
    mab[tid] = -1;
    mba[tid] = -1;
    mi[tid] = 0;
    mu[tid] = 0;
  }
  __syncthreads();
  for (int e = tid; e < nbins; e += kThreads) {
    const int i = e / PB, j = e - i * PB;
    int c = 0;
    if (i < na && j < nb) {
      c = inter[(int64_t)v * nbins + e];
      const int uni = aa[i] + ab[j] - c;
      const bool same_cls = !cls_a || !cls_b || cls_a[(int64_t)v * PA + i] == cls_b[(int64_t)v * PB + j];
      if (!(same_cls && c > 0 && (double)c >= min_iou * (double)uni)) c = 0;
    }
    tab[e] = c;
  }
  __syncthreads();
  int matched = 0;
  const int rounds = min(na, nb);
  for (int round = 0; round < rounds; ++round) {  // (workgroup-uniform: the exit below is read from LDS by every thread)
    Cand best{0, 1, -1};
    for (int e = tid; e < nbins; e += kThreads) {
      const int c = tab[e];
      if (c == 0) continue;
      const int i = e / PB, j = e - i * PB;
      if (mab[i] >= 0 || mba[j] >= 0) continue;
      const Cand cand{c, aa[i] + ab[j] - c, e};
      if (cand_better(cand, best)) best = cand;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      Cand o;
      o.inter = __shfl_xor(best.inter, off, 64);
      o.uni = __shfl_xor(best.uni, off, 64);
      o.e = __shfl_xor(best.e, off, 64);
      if (cand_better(o, best)) best = o;
    }
    if (lane == 0) wbest[wave] = best;
    __syncthreads();
    if (tid == 0) {
      Cand b = wbest[0];
      for (int w = 1; w < kWaves; ++w)
        if (cand_better(wbest[w], b)) b = wbest[w];
      won = b.e;
      if (b.e >= 0) {
        const int i = b.e / PB, j = b.e - i * PB;
        mab[i] = j;
        mba[j] = i;
        mi[i] = b.inter;
        mu[i] = b.uni;
      }
    }
    __syncthreads();
    if (won < 0) break;
    ++matched;
  }
  if (tid < PA) {
    match_ab[(int64_t)v * PA + tid] = mab[tid];
    m_inter[(int64_t)v * PA + tid] = mi[tid];
    m_union[(int64_t)v * PA + tid] = mu[tid];
  }
  if (tid < PB) match_ba[(int64_t)v * PB + tid] = mba[tid];
  if (tid == 0) n_matched[v] = matched;
}

// ---- gather -----------------------------------------------------------------------------------------------------------------------
// per chunk: the members of every part.  counts [V][P][nchunk]
__global__ __launch_bounds__(kThreads) void ar_count_kernel(const int32_t* __restrict__ inst, const uint8_t* __restrict__ valid,
                                                            const int32_t* __restrict__ n_parts, int64_t HW, int P,
                                                            int32_t* __restrict__ counts) {
  __shared__ int h[kMaxP];
  const int v = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(n_parts[v], 0), P);
  if (tid < kMaxP) h[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    wave_hist_add(h, part_key(inst, valid, (int64_t)v * HW + p, p < HW, n));
  }
  __syncthreads();
  if (tid < P) counts[((int64_t)v * P + tid) * gridDim.x + blockIdx.x] = h[tid];
}

// one workgroup per (part, frame): the counts of its chunks -> their exclusive prefix, in place
__global__ __launch_bounds__(kThreads) void ar_scan_kernel(int32_t* __restrict__ counts, int nchunk) {
  __shared__ int wsum[kWaves];
  int32_t* c = counts + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nchunk;
  block_scan_tiled<kWaves, int>(nchunk, [&](int64_t i) { return c[i]; }, c, wsum);
}

__global__ __launch_bounds__(kThreads) void ar_store_kernel(const float* __restrict__ rows, const int32_t* __restrict__ inst,
                                                            const uint8_t* __restrict__ valid, const int32_t* __restrict__ n_parts,
                                                            const int64_t* __restrict__ seg_start, const int32_t* __restrict__ base,
                                                            int64_t HW, int P, int64_t n_total, double* __restrict__ pc) {
  __shared__ int cnt[kPer * kWaves][kMaxP];  // members of a part in (slot e, wave), then the members before that (slot, wave)
  const int v = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(max(n_parts[v], 0), P);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int i = tid; i < kPer * kWaves * kMaxP; i += kThreads) (&cnt[0][0])[i] = 0;
  __syncthreads();
  int key[kPer], rank[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    key[e] = part_key(inst, valid, (int64_t)v * HW + p, p < HW, n);
    const unsigned long long same = wave_match6(key[e], key[e] >= 0);
    rank[e] = __popcll(same & below);
    if (key[e] >= 0 && rank[e] == 0) cnt[e * kWaves + wave][key[e]] = __popcll(same);  // (the group's lowest lane)
  }
  __syncthreads();
  if (tid < P) {  // (slot order: e first, then the wave)
    int run = base[((int64_t)v * P + tid) * gridDim.x + blockIdx.x];
#pragma unroll
    for (int s = 0; s < kPer * kWaves; ++s) {
      const int c = cnt[s][tid];
      cnt[s][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    if (key[e] < 0) continue;
    const int64_t s0 = seg_start[(int64_t)v * P + key[e]];
    if (s0 < 0) continue;
    const int64_t pos = s0 + cnt[e * kWaves + wave][key[e]] + rank[e];
    if (pos >= n_total) continue;
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    const float* q = rows + ((int64_t)v * HW + p) * 6;
    double* o = pc + pos * 3;
    o[0] = (double)q[0];
    o[1] = (double)q[1];
    o[2] = (double)q[2];
  }
}

inline bool frames_ok(int V, int H, int W) { return V >= 0 && V <= 65535 && H >= 1 && H <= 16384 && W >= 1 && W <= 16384; }

}  // namespace

extern "C" int gpn_parts_overlap(const int32_t* inst_a, const uint8_t* valid_a, const int32_t* n_a, const int32_t* inst_b,
                                 const uint8_t* valid_b, const int32_t* n_b, int V, int H, int W, int PA, int PB, int32_t* inter,
                                 int32_t* area_a, int32_t* area_b, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(frames_ok(V, H, W));
  GPN_CHECK_ARG(PA >= 0 && PA <= GPN_PARTS_MAX && PB >= 0 && PB <= GPN_PARTS_MAX);
  if (V == 0 || (PA == 0 && PB == 0)) return GPN_OK;
  GPN_CHECK_ARG(inst_a && valid_a && n_a && inst_b && valid_b && n_b);
  GPN_CHECK_ARG((inter || PA * PB == 0) && (area_a || PA == 0) && (area_b || PB == 0));
  if (PA * PB > 0) GPN_CHECK_HIP(hipMemsetAsync(inter, 0, (size_t)V * PA * PB * sizeof(int32_t), stream));
  if (PA > 0) GPN_CHECK_HIP(hipMemsetAsync(area_a, 0, (size_t)V * PA * sizeof(int32_t), stream));
  if (PB > 0) GPN_CHECK_HIP(hipMemsetAsync(area_b, 0, (size_t)V * PB * sizeof(int32_t), stream));
  const int64_t HW = (int64_t)H * W;
  const dim3 grid((unsigned)gpn::cdiv(HW, kChunk), (unsigned)V);
  hipLaunchKernelGGL(ar_overlap_kernel, grid, dim3(kThreads), 0, stream, inst_a, valid_a, n_a, inst_b, valid_b, n_b, HW, PA, PB, inter,
                     area_a, area_b);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_parts_match(const int32_t* inter, const int32_t* area_a, const int32_t* area_b, const int32_t* n_a,
                               const int32_t* n_b, const int32_t* cls_a, const int32_t* cls_b, double min_iou, int V, int PA, int PB,
                               int32_t* match_ab, int32_t* match_ba, int32_t* n_matched, int32_t* m_inter, int32_t* m_union,
                               gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(V >= 0 && V <= 65535);
  GPN_CHECK_ARG(PA >= 0 && PA <= GPN_PARTS_MAX && PB >= 0 && PB <= GPN_PARTS_MAX);
  GPN_CHECK_ARG(min_iou == min_iou);  // (not NaN)
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(n_a && n_b && n_matched);
  GPN_CHECK_ARG((inter || PA * PB == 0) && (PA == 0 || (area_a && match_ab && m_inter && m_union)) && (PB == 0 || (area_b && match_ba)));
  hipLaunchKernelGGL(ar_match_kernel, dim3((unsigned)V), dim3(kThreads), 0, stream, inter, area_a, area_b, n_a, n_b, cls_a, cls_b, min_iou,
                     PA, PB, match_ab, match_ba, n_matched, m_inter, m_union);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" size_t gpn_parts_gather_ws_bytes(int V, int H, int W, int P) {
  if (V <= 0 || H <= 0 || W <= 0 || P <= 0) return 0;
  return gpn::align_up((size_t)V * P * gpn::cdiv((int64_t)H * W, kChunk) * sizeof(int32_t));
}

extern "C" int gpn_parts_gather(const float* rows, const int32_t* inst, const uint8_t* valid, const int32_t* n_parts,
                                const int64_t* seg_start, int V, int H, int W, int P, int64_t n_total, double* pc, void* ws,
                                size_t ws_bytes, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(frames_ok(V, H, W));
  GPN_CHECK_ARG(P >= 0 && P <= GPN_PARTS_MAX && n_total >= 0);
  if (V == 0 || P == 0 || n_total == 0) return GPN_OK;
  GPN_CHECK_ARG(rows && inst && valid && n_parts && seg_start && pc);
  const int64_t HW = (int64_t)H * W, nchunk = gpn::cdiv(HW, kChunk);
  gpn::WsCarver carve(ws, ws_bytes);
  int32_t* counts = carve.take<int32_t>((size_t)V * P * nchunk);
  GPN_CHECK_WS(carve);
  const dim3 grid((unsigned)nchunk, (unsigned)V);
  hipLaunchKernelGGL(ar_count_kernel, grid, dim3(kThreads), 0, stream, inst, valid, n_parts, HW, P, counts);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(ar_scan_kernel, dim3((unsigned)P, (unsigned)V), dim3(kThreads), 0, stream, counts, (int)nchunk);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(ar_store_kernel, grid, dim3(kThreads), 0, stream, rows, inst, valid, n_parts, seg_start, counts, HW, P, n_total, pc);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
