// articulate.hip — the parts of two frames of one scene, associated and cut out for the joint kernels (include/gpn.h section AR).
// A batch of V frame pairs of one size H x W, at most GPN_PARTS_MAX parts a frame:
//   overlap  the contingency table of the two instance maps: inter [V,PA,PB], area_a [V,PA], area_b [V,PB].  One workgroup per chunk
//            of 1024 pixels (the chunk of frameprep.hip); a PA x PB histogram in LDS.  The maps are piecewise constant, so a wave
//            first groups its lanes by key (ballots) and adds each group's popcount with ONE LDS atomic; non-zero bins are merged
//            into the frame pair's table by integer global adds.
//   match    greedy one-to-one matching by exact IoU: one workgroup a frame pair, the table in LDS, one arg-max a round.
//   gather   the stable multi-way partition of pixel_parts.h over 6-bit keys (the part of a pixel): counts [V][P][chunk], one scan
//            over the chunks per (frame, part), the xyz of a member row stored as float64.
// The wave helpers (wave_hist_add, wave_match), the partition and the workgroup arg-max (block_best) are pixel_parts.h's, shared with
// multiview.hip.
// No float atomics; integer atomics only on histograms (order-free); no host read; every result is independent of timing.
#include "pixel_parts.h"

namespace {

using namespace gpn;
using namespace gpn::pp;

constexpr int kMaxP = GPN_PARTS_MAX;

// the membership rule: the part of pixel g, or -1.  n is the frame's live part count, already clamped to the table width.
__device__ __forceinline__ int part_key(const int32_t* __restrict__ inst, const uint8_t* __restrict__ valid, int64_t g, bool inside,
                                        int n) {
  if (!inside) return -1;
  const int p = inst[g];
  return (valid[g] != 0 && p >= 0 && p < n) ? p : -1;
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
// a candidate: num = inter, den = union, e = i * PB + j.  The larger IoU first, ties to the smaller (i, j).
__global__ __launch_bounds__(kThreads) void ar_match_kernel(const int32_t* __restrict__ inter, const int32_t* __restrict__ area_a,
                                                            const int32_t* __restrict__ area_b, const int32_t* __restrict__ n_a,
                                                            const int32_t* __restrict__ n_b, const int32_t* __restrict__ cls_a,
                                                            const int32_t* __restrict__ cls_b, double min_iou, int PA, int PB,
                                                            int32_t* __restrict__ match_ab, int32_t* __restrict__ match_ba,
                                                            int32_t* __restrict__ n_matched, int32_t* __restrict__ m_inter,
                                                            int32_t* __restrict__ m_union) {
  __shared__ int tab[kMaxP * kMaxP];  // inter of the eligible pairs, 0 elsewhere
  __shared__ int aa[kMaxP], ab[kMaxP], mab[kMaxP], mba[kMaxP], mi[kMaxP], mu[kMaxP];
  __shared__ RatioCand wbest[kWaves];
  const int v = blockIdx.x, tid = threadIdx.x;
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
  for (int round = 0; round < rounds; ++round) {  // (workgroup-uniform: block_best hands every thread the same winner)
    RatioCand best{0, 1, -1};
    for (int e = tid; e < nbins; e += kThreads) {
      const int c = tab[e];
      if (c == 0) continue;
      const int i = e / PB, j = e - i * PB;
      if (mab[i] >= 0 || mba[j] >= 0) continue;
      const RatioCand cand{c, aa[i] + ab[j] - c, e};
      if (ratio_better(cand, best)) best = cand;
    }
    const RatioCand b = block_best<kWaves>(best, wbest);
    if (b.e < 0) break;
    if (tid == 0) {
      const int i = b.e / PB, j = b.e - i * PB;
      mab[i] = j;
      mba[j] = i;
      mi[i] = b.num;
      mu[i] = b.den;
    }
    __syncthreads();  // the next round reads mab and mba, and writes wbest
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
// the partition's policy: key = the part of a pixel; counts [V][P][nchunk], one scan per (part, frame); a member's xyz as float64
struct ArParts {
  static constexpr int kMaxKeys = kMaxP, kKeyBits = 6;
  const float* rows;
  const int32_t* inst;
  const uint8_t* valid;
  const int32_t* n_parts;
  const int64_t* seg_start;
  int P;
  int64_t n_total;
  double* pc;
  __device__ int live_keys(int) const { return P; }
  __device__ int key(int v, int64_t g, bool inside) const { return part_key(inst, valid, g, inside, min(max(n_parts[v], 0), P)); }
  __device__ int64_t counts_index(int v, int key, int chunk, int nchunk, int) const { return ((int64_t)v * P + key) * nchunk + chunk; }
  dim3 scan_grid(int V) const { return dim3((unsigned)P, (unsigned)V); }
  int64_t scan_len(int, int64_t nchunk) const { return nchunk; }
  __device__ void store(int v, int key, int rank, int64_t g) const {
    const int64_t s0 = seg_start[(int64_t)v * P + key];
    if (s0 < 0) return;
    const int64_t pos = s0 + rank;
    if (pos >= n_total) return;
    const float* q = rows + g * 6;
    double* o = pc + pos * 3;
    o[0] = (double)q[0];
    o[1] = (double)q[1];
    o[2] = (double)q[2];
  }
};

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
  return pp_partition(ArParts{rows, inst, valid, n_parts, seg_start, P, n_total, pc}, V, HW, counts, stream);
}
