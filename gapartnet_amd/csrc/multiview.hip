// multiview.hip — the part predictions of several posed RGB-D views of ONE object fused into object parts (include/gpn.h section MV).
// V <= GPN_VIEWS_MAX views of one size H x W, GT <= GPN_FUSE_PARTS_MAX parts over all views (global id g = base[v] + p):
//   world    every member pixel's camera row -> world frame in float64 (fixed order, no contraction), stored as f32; part_of, the
//            parts' areas (a per-chunk LDS histogram, one add per group of equal keys in a wave) and the per-axis minimum of the
//            stored rows: atomicMin on the order-preserving integer image of the value, decoded by a three-thread finish kernel
//   overlap  one 64-bit key (vox << 9 | g) per pixel, ONE rocprim::radix_sort_keys over the 40 low bits (39 live ones and the bit
//            that puts the all-ones key of a non-member behind them), rocprim::unique -> the distinct (vox, g); one lane per distinct
//            entry adds 1 to vol[g] and walks the LATER entries of its voxel (at most GT - 1) for the pair increments.  The pair
//            table is summed in LDS while GT * GT * 4 bytes fit in 64 KiB (GT <= 128) and flushed by global integer adds, and is
//            summed in global memory otherwise; gpn_views_overlap_lds_parts moves the switch (tools/multiview_bench.py measured it)
//   merge    one workgroup of 1024 threads: the pairs that pass the rules which never change (class, min_inter, min_overlap) are
//            listed once in LDS (up to 3072 of them; a table with more is scanned row by row every round instead), then per round
//            the arg-max of the pairs still eligible (exact 64-bit cross products), one union, at most GT - 1 rounds; a listed pair
//            refused for its clusters is struck from the list, since clusters only grow
//   relabel  fused_inst = fused_of[part_of]
//   gather   the stable multi-way partition of pixel_parts.h over 9-bit keys (the fused id of a pixel): counts [F][V][chunk], one
//            scan over (view, chunk) per fused part, a member's world row, its NPCS and its pixel stored
// The wave helpers (wave_hist_add, wave_match), the partition and the workgroup arg-max (block_best) are pixel_parts.h's, shared with
// articulate.hip: that file's policy holds 64-wide tables and 6-bit ballots per frame, this one's 512-wide tables over all views.
// No float atomics; integer atomics only on minima, histograms and counters (order-free); no host read; every result is
// independent of timing.
#include "pixel_parts.h"  // first: gpn_common.h pulls <cstring> ahead of the HIP/rocPRIM headers

#include <algorithm>

#include <rocprim/rocprim.hpp>

namespace {

using namespace gpn;
using namespace gpn::pp;

constexpr int kMaxV = GPN_VIEWS_MAX;
constexpr int kMaxG = GPN_FUSE_PARTS_MAX;
constexpr uint64_t kDeadKey = ~0ull;    // a pixel outside the occupancy
constexpr unsigned kSortBits = 40;      // 30 voxel bits, 9 part bits, and the bit that sorts the dead key last
constexpr int kGridCells = 1024;        // cells per axis
constexpr int kLdsPartsMax = 128;       // GT * GT * 4 <= 64 KiB
constexpr int kMergeThreads = 1024;
constexpr int kMergeWaves = kMergeThreads / 64;
constexpr int kMergeList = 3072;  // statically eligible pairs the merge keeps in LDS

int g_lds_parts = kLdsPartsMax;  // the pair table is summed in LDS for GT <= this

// the live parts of view v and the global id of its part 0 (workgroup-uniform; contains a barrier)
__device__ __forceinline__ int view_base(const int32_t* __restrict__ n_parts, int v, int GT, int* sh) {
  if (threadIdx.x < 64) {
    int c = (int)threadIdx.x < v ? min(max(n_parts[threadIdx.x], 0), GT) : 0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if (threadIdx.x == 0) *sh = c;
  }
  __syncthreads();
  return *sh;
}

// ---- 1. world rows, part_of, areas, bounds ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void mv_world_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ valid,
                                                            const int32_t* __restrict__ inst, const int32_t* __restrict__ n_parts,
                                                            const double* __restrict__ R, const double* __restrict__ t, int64_t HW,
                                                            int GT, float* __restrict__ wrows, int32_t* __restrict__ part_of,
                                                            int32_t* __restrict__ area, unsigned long long* __restrict__ lo_img) {
  __shared__ int h[kMaxG];
  __shared__ int sh_base;
  __shared__ uint32_t red[3][kWaves];
  const int v = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(max(n_parts[v], 0), GT);
  const int base = view_base(n_parts, v, GT, &sh_base);
  for (int i = tid; i < kMaxG; i += kThreads) h[i] = 0;
  __syncthreads();
  double r[9], tt[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) r[i] = R[(int64_t)v * 9 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) tt[i] = t[(int64_t)v * 3 + i];
  const float nanf_ = __uint_as_float(0x7fc00000u);
  uint32_t b[3] = {0u, 0u, 0u};  // ~image of the minimum: grows
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    const bool inside = p < HW;
    const int64_t g = (int64_t)v * HW + p;
    int key = -1;
    if (inside) {
      const int q = inst[g];
      if (valid[g] != 0 && q >= 0 && q < n && base + q < GT) key = q;
    }
    wave_hist_add(h, key);
    if (!inside) continue;
    float w[3] = {nanf_, nanf_, nanf_};
    if (key >= 0) {
      const double x = (double)rows[g * 6 + 0], y = (double)rows[g * 6 + 1], z = (double)rows[g * 6 + 2];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        w[k] = (float)(((x * r[k * 3 + 0] + y * r[k * 3 + 1]) + z * r[k * 3 + 2]) + tt[k]);
        b[k] = max(b[k], ~f2ord(w[k]));
      }
    }
    wrows[g * 3 + 0] = w[0];
    wrows[g * 3 + 1] = w[1];
    wrows[g * 3 + 2] = w[2];
    part_of[g] = key >= 0 ? base + key : -1;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) b[a] = max(b[a], (uint32_t)__shfl_xor((int)b[a], off, 64));
    if (lane == 0) red[a][wave] = b[a];
  }
  __syncthreads();
  if (tid < 3) {
    uint32_t m = red[tid][0];
    for (int w = 1; w < kWaves; ++w) m = max(m, red[tid][w]);
    if (m != 0u) atomicMin(lo_img + tid, d2ord((double)ord2f(~m)));  // (integer compare: order-free)
  }
  for (int i = tid; i < n; i += kThreads)
    if (h[i]) atomicAdd(area + base + i, h[i]);  // (base + i < GT wherever h[i] != 0)
}

// lo: the integer image -> the float64 value, in place; 0.0 when no pixel is a member
__global__ void mv_lo_finish_kernel(double* lo) {
  const int a = threadIdx.x;
  if (a >= 3) return;
  const unsigned long long k = reinterpret_cast<unsigned long long*>(lo)[a];
  lo[a] = k == ~0ull ? 0.0 : ord2d(k);
}

// ---- 2. voxel keys -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void mv_keys_kernel(const float* __restrict__ wrows, const int32_t* __restrict__ part_of,
                                                           const double* __restrict__ lo, double cell, int64_t HW, int GT,
                                                           uint64_t* __restrict__ keys, uint64_t* __restrict__ keys_out,
                                                           int32_t* __restrict__ dropped) {
  __shared__ int wsum[kWaves];
  const int v = blockIdx.y, tid = threadIdx.x;
  const double l[3] = {lo[0], lo[1], lo[2]};
  int drop = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (p >= HW) continue;
    const int64_t g = (int64_t)v * HW + p;
    const int part = part_of[g];
    uint64_t key = kDeadKey;
    if (part >= 0 && part < GT) {
      bool ok = true;
      uint64_t vox = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double q = floor(((double)wrows[g * 3 + a] - l[a]) / cell);
        if (!(q >= 0.0 && q < (double)kGridCells)) ok = false;  // (a NaN is dropped as well)
        else vox = (vox << 10) | (uint64_t)(int)q;
      }
      if (ok) key = (vox << 9) | (uint64_t)part;
      else ++drop;
    }
    keys[g] = key;
    if (keys_out) keys_out[g] = key;
  }
  drop = block_sum<kWaves>(drop, wsum);
  if (tid == 0 && drop) atomicAdd(dropped + v, drop);  // (integer add: order-free)
}

// ---- 3. occupancy tables over the distinct (vox, g) -----------------------------------------------------------------------------------
template <bool kLds>
__global__ __launch_bounds__(kThreads) void mv_tables_kernel(const uint64_t* __restrict__ uniq, const unsigned int* __restrict__ n_uniq,
                                                             int64_t n_bound, int GT, int32_t* __restrict__ vol,
                                                             int32_t* __restrict__ inter) {
  extern __shared__ int tab[];  // [GT][GT] when kLds
  const int tid = threadIdx.x;
  const int64_t n = min((int64_t)*n_uniq, n_bound);
  if (kLds) {
    for (int i = tid; i < GT * GT; i += kThreads) tab[i] = 0;
    __syncthreads();
  }
  for (int64_t i = (int64_t)blockIdx.x * kThreads + tid; i < n; i += (int64_t)gridDim.x * kThreads) {
    const uint64_t k = uniq[i];
    if (k == kDeadKey) continue;
    const int g = (int)(k & 511u);
    const uint64_t vox = k >> 9;
    if (g >= GT) continue;
    atomicAdd(vol + g, 1);
    for (int64_t j = i + 1; j < n; ++j) {  // the later parts of this voxel: at most GT - 1
      const uint64_t kj = uniq[j];
      if ((kj >> 9) != vox) break;
      const int hh = (int)(kj & 511u);
      if (hh >= GT) continue;
      if (kLds) {
        atomicAdd(&tab[g * GT + hh], 1);
        atomicAdd(&tab[hh * GT + g], 1);
      } else {
        atomicAdd(inter + g * GT + hh, 1);
        atomicAdd(inter + hh * GT + g, 1);
      }
    }
  }
  if (kLds) {
    __syncthreads();
    for (int i = tid; i < GT * GT; i += kThreads) {
      const int c = tab[i];
      if (c) atomicAdd(inter + i, c);  // (merged by integer adds: order-free)
    }
  }
}

// ---- 4. merge -----------------------------------------------------------------------------------------------------------------------
// a candidate: num = inter, den = min(vol), e = g << 9 | h with g < h.  The larger ratio first, ties to the smaller (g, h).
__global__ __launch_bounds__(kMergeThreads) void mv_merge_kernel(
    const int32_t* __restrict__ inter, const int32_t* __restrict__ vol, const int32_t* __restrict__ cls,
    const int32_t* __restrict__ n_parts, int V, int GT, int min_inter, double min_overlap, int32_t* __restrict__ fused_of,
    int32_t* __restrict__ n_fused, unsigned long long* __restrict__ fused_views, int32_t* __restrict__ fused_class,
    int32_t* __restrict__ fused_vol, int32_t* __restrict__ fused_parts, int32_t* __restrict__ links, int32_t* __restrict__ n_links) {
  __shared__ int rep[kMaxG], svol[kMaxG], cvol[kMaxG], scls[kMaxG], sview[kMaxG], isrep[kMaxG], frep[kMaxG], fidx[kMaxG];
  __shared__ int sbase[kMaxV + 1];
  __shared__ unsigned long long cviews[kMaxG];
  __shared__ RatioCand wbest[kMergeWaves];
  __shared__ int list_e[kMergeList], list_c[kMergeList];  // the statically eligible pairs: e (-1: struck) and inter
  __shared__ int n_list;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    n_list = 0;
    int run = 0;
    for (int v = 0; v < V; ++v) {
      sbase[v] = run;
      run = min(run + min(max(n_parts[v], 0), GT), GT);
    }
    sbase[V] = run;
  }
  __syncthreads();
  if (tid < GT) {
    int view = -1;
    for (int v = 0; v < V; ++v)
      if (tid >= sbase[v] && tid < sbase[v + 1]) view = v;
    sview[tid] = view;
    svol[tid] = view >= 0 ? max(vol[tid], 0) : 0;
    cvol[tid] = svol[tid];
    rep[tid] = tid;
    scls[tid] = cls ? cls[tid] : 0;
    cviews[tid] = view >= 0 ? 1ull << view : 0ull;
  }
  __syncthreads();
  const int mi = max(min_inter, 1);
  // the rules that never change: class, min_inter, min_overlap
  auto static_ok = [&](int g, int hh, int c) {
    if (c < mi || svol[hh] == 0 || scls[hh] != scls[g]) return false;
    return (double)c >= min_overlap * (double)min(svol[g], svol[hh]);
  };
  for (int g = wave; g < GT; g += kMergeWaves) {  // a wave per table row
    if (svol[g] == 0) continue;
    for (int hh = g + 1 + lane; hh < GT; hh += 64) {
      const int c = inter[g * GT + hh];
      if (!static_ok(g, hh, c)) continue;
      const int slot = atomicAdd(&n_list, 1);  // (the list's order does not matter: the arg-max is over a total order)
      if (slot < kMergeList) {
        list_e[slot] = (g << 9) | hh;
        list_c[slot] = c;
      }
    }
  }
  __syncthreads();
  const int nc = n_list;
  const bool listed = nc <= kMergeList;
  int nl = 0;
  for (int round = 0; round < GT; ++round) {  // (workgroup-uniform: block_best hands every thread the same winner)
    RatioCand best{0, 1, -1};
    if (listed) {
      for (int i = tid; i < nc; i += kMergeThreads) {  // (entry i is always this thread's)
        const int e = list_e[i];
        if (e < 0) continue;
        const int g = e >> 9, hh = e & 511;
        const int rg = rep[g], rh = rep[hh];
        if (rh == rg || (cviews[rh] & cviews[rg]) != 0ull) {
          list_e[i] = -1;  // refused for good: clusters only grow
          continue;
        }
        const RatioCand cand{list_c[i], min(svol[g], svol[hh]), e};
        if (ratio_better(cand, best)) best = cand;
      }
    } else {
      for (int g = wave; g < GT; g += kMergeWaves) {
        if (svol[g] == 0) continue;
        const int rg = rep[g];
        const unsigned long long mg = cviews[rg];
        for (int hh = g + 1 + lane; hh < GT; hh += 64) {
          const int c = inter[g * GT + hh];
          if (!static_ok(g, hh, c)) continue;
          const int rh = rep[hh];
          if (rh == rg || (cviews[rh] & mg) != 0ull) continue;
          const RatioCand cand{c, min(svol[g], svol[hh]), (g << 9) | hh};
          if (ratio_better(cand, best)) best = cand;
        }
      }
    }
    const RatioCand w = block_best<kMergeWaves>(best, wbest);
    if (w.e < 0) break;
    const int g = w.e >> 9, hh = w.e & 511;
    const int ra = rep[g], rb = rep[hh];
    const int keep = min(ra, rb), gone = max(ra, rb);
    __syncthreads();  // every thread has read rep
    if (tid < GT && rep[tid] == gone) rep[tid] = keep;
    if (tid == 0) {
      cviews[keep] |= cviews[gone];
      cvol[keep] += cvol[gone];
      links[nl * 3 + 0] = g;
      links[nl * 3 + 1] = hh;
      links[nl * 3 + 2] = w.num;
    }
    ++nl;
    __syncthreads();
  }
  // fused ids in ascending order of the cluster's smallest g (= its rep)
  if (tid < GT) isrep[tid] = (svol[tid] > 0 && rep[tid] == tid) ? 1 : 0;
  __syncthreads();
  int F = 0;
  for (int j = 0; j < GT; ++j) {
    if (j == tid) fidx[tid] = F;
    F += isrep[j];
  }
  if (tid < GT && isrep[tid]) frep[fidx[tid]] = tid;
  for (int i = tid; i < GT * V; i += kMergeThreads) fused_parts[i] = -1;
  __syncthreads();
  if (tid < GT) {
    const int f = svol[tid] > 0 ? fidx[rep[tid]] : -1;
    fused_of[tid] = f;
    if (f >= 0) fused_parts[f * V + sview[tid]] = tid - sbase[sview[tid]];
    const bool live = tid < F;
    const int r = live ? frep[tid] : 0;
    fused_views[tid] = live ? cviews[r] : 0ull;
    fused_class[tid] = live ? scls[r] : -1;
    fused_vol[tid] = live ? cvol[r] : 0;
    if (tid >= nl) {
      links[tid * 3 + 0] = -1;
      links[tid * 3 + 1] = -1;
      links[tid * 3 + 2] = 0;
    }
  }
  if (tid == 0) {
    *n_fused = F;
    *n_links = nl;
  }
}

// ---- 5. relabel and gather ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void mv_relabel_kernel(const int32_t* __restrict__ part_of, const int32_t* __restrict__ fused_of,
                                                              int64_t N, int GT, int32_t* __restrict__ fused_inst) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const int g = part_of[i];
  fused_inst[i] = (g >= 0 && g < GT) ? fused_of[g] : -1;
}

// the partition's policy: key = the fused part of a pixel; counts [F][V][nchunk], one scan per fused part over its V * nchunk cells;
// a member's world row and NPCS as float64, and its pixel
struct MvParts {
  static constexpr int kMaxKeys = kMaxG, kKeyBits = 9;
  const float* wrows;
  const float* npcs;
  const int32_t* fused_inst;
  const int64_t* seg_start;
  int F;
  int64_t n_total;
  double* xyz;
  double* npcs_out;
  int64_t* src;
  __device__ int live_keys(int) const { return F; }
  __device__ int key(int, int64_t g, bool inside) const {
    if (!inside) return -1;
    const int f = fused_inst[g];
    return (f >= 0 && f < F) ? f : -1;
  }
  __device__ int64_t counts_index(int v, int key, int chunk, int nchunk, int V) const { return ((int64_t)key * V + v) * nchunk + chunk; }
  dim3 scan_grid(int) const { return dim3((unsigned)F); }
  int64_t scan_len(int V, int64_t nchunk) const { return (int64_t)V * nchunk; }
  __device__ void store(int, int key, int rank, int64_t g) const {
    const int64_t s0 = seg_start[key];
    if (s0 < 0) return;
    const int64_t pos = s0 + rank;
    if (pos >= n_total) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      xyz[pos * 3 + k] = (double)wrows[g * 3 + k];
      if (npcs_out) npcs_out[pos * 3 + k] = (double)npcs[g * 3 + k];
    }
    src[pos] = g;
  }
};

inline bool views_ok(int V, int H, int W) {
  return V >= 0 && V <= kMaxV && H >= 1 && H <= 16384 && W >= 1 && W <= 16384 &&
         (int64_t)V * H * W < (int64_t)0x7fffffff - kChunk;
}

struct OverlapWs {
  uint64_t *keys, *sorted, *uniq;
  unsigned int* n_uniq;
  char* prim;
  size_t prim_bytes, total;
};
OverlapWs overlap_ws(void* ws, size_t N) {
  gpn::WsCarver w(ws, ~(size_t)0);
  OverlapWs o;
  o.keys = w.take<uint64_t>(N);
  o.sorted = w.take<uint64_t>(N);
  o.uniq = w.take<uint64_t>(N);
  o.n_uniq = w.take<unsigned int>(1);
  size_t a = 0, b = 0;
  (void)rocprim::radix_sort_keys(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, N, 0u, kSortBits, (hipStream_t) nullptr);
  (void)rocprim::unique(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (unsigned int*)nullptr, N,
                        rocprim::equal_to<uint64_t>(), (hipStream_t) nullptr);
  o.prim_bytes = a > b ? a : b;
  o.prim = w.take<char>(o.prim_bytes);
  o.total = w.used;
  return o;
}

}  // namespace

extern "C" int gpn_views_world(const float* rows, const uint8_t* valid, const int32_t* inst, const int32_t* n_parts, const double* R,
                               const double* t, int V, int H, int W, int GT, float* wrows, int32_t* part_of, int32_t* area, double* lo,
                               gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(views_ok(V, H, W));
  GPN_CHECK_ARG(GT >= 0 && GT <= kMaxG);
  GPN_CHECK_ARG(lo && (area || GT == 0));
  GPN_CHECK_ARG(V == 0 || (rows && valid && inst && n_parts && R && t && wrows && part_of));
  if (GT > 0) GPN_CHECK_HIP(hipMemsetAsync(area, 0, (size_t)GT * sizeof(int32_t), stream));
  GPN_CHECK_HIP(hipMemsetAsync(lo, 0xff, 3 * sizeof(double), stream));
  if (V > 0) {
    const int64_t HW = (int64_t)H * W;
    const dim3 grid((unsigned)gpn::cdiv(HW, kChunk), (unsigned)V);
    hipLaunchKernelGGL(mv_world_kernel, grid, dim3(kThreads), 0, stream, rows, valid, inst, n_parts, R, t, HW, GT, wrows, part_of, area,
                       reinterpret_cast<unsigned long long*>(lo));
    GPN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(mv_lo_finish_kernel, dim3(1), dim3(64), 0, stream, lo);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_views_overlap_lds_parts(int parts) {
  if (parts >= 0) g_lds_parts = parts < kLdsPartsMax ? parts : kLdsPartsMax;
  return g_lds_parts;
}

extern "C" size_t gpn_views_overlap_ws_bytes(int V, int H, int W) {
  if (V <= 0 || !views_ok(V, H, W)) return 0;
  return overlap_ws(nullptr, (size_t)V * H * W).total;
}

extern "C" int gpn_views_overlap(const float* wrows, const int32_t* part_of, const double* lo, double cell, int V, int H, int W, int GT,
                                 int32_t* vol, int32_t* inter, int32_t* dropped, uint64_t* keys_out, void* ws, size_t ws_bytes,
                                 gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(views_ok(V, H, W));
  GPN_CHECK_ARG(GT >= 0 && GT <= kMaxG);
  GPN_CHECK_ARG(cell > 0.0 && cell <= 1.7e308);  // (finite, not NaN)
  GPN_CHECK_ARG((vol && inter) || GT == 0);
  GPN_CHECK_ARG(V == 0 || (wrows && part_of && lo && dropped));
  GPN_CHECK_ARG(V == 0 || GT == 0 || (ws && ws_bytes >= gpn_views_overlap_ws_bytes(V, H, W)));
  if (GT > 0) {
    GPN_CHECK_HIP(hipMemsetAsync(vol, 0, (size_t)GT * sizeof(int32_t), stream));
    GPN_CHECK_HIP(hipMemsetAsync(inter, 0, (size_t)GT * GT * sizeof(int32_t), stream));
  }
  if (V == 0) return GPN_OK;
  GPN_CHECK_HIP(hipMemsetAsync(dropped, 0, (size_t)V * sizeof(int32_t), stream));
  if (GT == 0) {  // no part: no member, nothing dropped
    if (keys_out) GPN_CHECK_HIP(hipMemsetAsync(keys_out, 0xff, (size_t)V * H * W * sizeof(uint64_t), stream));
    return GPN_OK;
  }
  const int64_t HW = (int64_t)H * W;
  const size_t N = (size_t)V * (size_t)HW;
  const OverlapWs o = overlap_ws(ws, N);
  const dim3 grid((unsigned)gpn::cdiv(HW, kChunk), (unsigned)V);
  hipLaunchKernelGGL(mv_keys_kernel, grid, dim3(kThreads), 0, stream, wrows, part_of, lo, cell, HW, GT, o.keys, keys_out, dropped);
  GPN_CHECK_LAUNCH();
  size_t tmp = o.prim_bytes;
  GPN_CHECK_HIP(rocprim::radix_sort_keys(o.prim, tmp, (const uint64_t*)o.keys, o.sorted, N, 0u, kSortBits, stream));
  tmp = o.prim_bytes;
  GPN_CHECK_HIP(rocprim::unique(o.prim, tmp, (const uint64_t*)o.sorted, o.uniq, o.n_uniq, N, rocprim::equal_to<uint64_t>(), stream));
  const bool lds = GT <= g_lds_parts;
  const unsigned wgs = (unsigned)std::min<int64_t>(gpn::cdiv((int64_t)N, kThreads), lds ? 512 : 2048);
  if (lds)
    hipLaunchKernelGGL(mv_tables_kernel<true>, dim3(wgs), dim3(kThreads), (size_t)GT * GT * sizeof(int), stream, o.uniq, o.n_uniq,
                       (int64_t)N, GT, vol, inter);
  else
    hipLaunchKernelGGL(mv_tables_kernel<false>, dim3(wgs), dim3(kThreads), 0, stream, o.uniq, o.n_uniq, (int64_t)N, GT, vol, inter);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_views_merge(const int32_t* inter, const int32_t* vol, const int32_t* cls, const int32_t* n_parts, int V, int GT,
                               int min_inter, double min_overlap, int32_t* fused_of, int32_t* n_fused, uint64_t* fused_views,
                               int32_t* fused_class, int32_t* fused_vol, int32_t* fused_parts, int32_t* links, int32_t* n_links,
                               gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(V >= 0 && V <= kMaxV && GT >= 0 && GT <= kMaxG);
  GPN_CHECK_ARG(min_overlap == min_overlap);  // (not NaN)
  GPN_CHECK_ARG(n_fused && n_links);
  GPN_CHECK_ARG(GT == 0 || (inter && vol && fused_of && fused_views && fused_class && fused_vol && links));
  GPN_CHECK_ARG(GT == 0 || V == 0 || (n_parts && fused_parts));
  hipLaunchKernelGGL(mv_merge_kernel, dim3(1), dim3(kMergeThreads), 0, stream, inter, vol, cls, n_parts, V, GT, min_inter, min_overlap,
                     fused_of, n_fused, reinterpret_cast<unsigned long long*>(fused_views), fused_class, fused_vol, fused_parts, links,
                     n_links);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_views_relabel(const int32_t* part_of, const int32_t* fused_of, int V, int H, int W, int GT, int32_t* fused_inst,
                                 gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(views_ok(V, H, W));
  GPN_CHECK_ARG(GT >= 0 && GT <= kMaxG);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(part_of && fused_inst && (fused_of || GT == 0));
  const int64_t N = (int64_t)V * H * W;
  hipLaunchKernelGGL(mv_relabel_kernel, dim3((unsigned)gpn::cdiv(N, kThreads)), dim3(kThreads), 0, stream, part_of, fused_of, N, GT,
                     fused_inst);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" size_t gpn_views_gather_ws_bytes(int V, int H, int W, int F) {
  if (V <= 0 || H <= 0 || W <= 0 || F <= 0) return 0;
  return gpn::align_up((size_t)F * V * gpn::cdiv((int64_t)H * W, kChunk) * sizeof(int32_t));
}

extern "C" int gpn_views_gather(const float* wrows, const float* npcs, const int32_t* fused_inst, const int64_t* seg_start, int V, int H,
                                int W, int F, int64_t n_total, double* xyz, double* npcs_out, int64_t* src, void* ws, size_t ws_bytes,
                                gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(views_ok(V, H, W));
  GPN_CHECK_ARG(F >= 0 && F <= kMaxG && n_total >= 0);
  GPN_CHECK_ARG((npcs == nullptr) == (npcs_out == nullptr) || n_total == 0);
  if (V == 0 || F == 0 || n_total == 0) return GPN_OK;
  GPN_CHECK_ARG(wrows && fused_inst && seg_start && xyz && src);
  const int64_t HW = (int64_t)H * W, nchunk = gpn::cdiv(HW, kChunk);
  gpn::WsCarver carve(ws, ws_bytes);
  int32_t* counts = carve.take<int32_t>((size_t)F * V * nchunk);
  GPN_CHECK_WS(carve);
  return pp_partition(MvParts{wrows, npcs, fused_inst, seg_start, F, n_total, xyz, npcs_out, src}, V, HW, counts, stream);
}
