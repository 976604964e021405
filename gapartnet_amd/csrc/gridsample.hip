// gridsample.hip — the opt-in octree-cell sampler of inference (include/gpn.h section GS): per cloud m of its n > m packed rows,
// one per occupied cell of the deepest octree level L* with at most m cells, the rest from the level below by a seeded hash.
//   bounds   per-axis min / max of a cloud: integer atomicMin / atomicMax on the order-preserving integer image of the floats;
//            the status rule of gpn_view_fps (n < m: FEW, n == m: arange)
//   keys     the 30-bit Morton code of every row; sort key (cloud, dead, code), payload = the row
//   (sort)   ONE stable rocprim::radix_sort_pairs over all S * n_bound rows: a cloud's live rows first in its own segment, by (code, j)
//   levels   per sorted row the first level at which it opens a new cell (from the code of the row before it); a 12-bin histogram
//            of that per cloud = all eleven cell counts C_L
//   mark     L* and r = m - C_L* from the histogram; flag[j] = stage A (the row opens a cell at a level <= L*); the stage-B candidates
//            in the order that breaks their hash ties: sorted position (= ascending cell) for L* < 10, row index for L* == 10
//   select   the r-th smallest candidate hash: the radix select of frameprep.hip (8 bits a pass, LDS histograms, resolved on the
//            device by select_resolve), per-chunk tie counts, ties admitted in slot order by wave ballots; picks set flag[j]
//   emit     per-chunk flag counts, then ballot-ordered stores: idx ascending, no second sort
// A cloud is shared by cdiv(n_bound, kChunk) workgroups in every pass.  No float atomics; integer atomics only on bounds, histograms
// and counters (order-free); no host read; every result is independent of timing.
#include "gpn_common.h"  // first: pulls <cstring> ahead of the HIP/rocPRIM headers

#include <rocprim/rocprim.hpp>

#include "point_prims.h"

namespace {

using namespace gpn;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 4;  // slots per thread: slot = chunk * kChunk + e * kThreads + tid
constexpr int kChunk = kThreads * kPer;
constexpr int kLevels = 11;      // octree levels 0 .. 10 (10 bits an axis)
constexpr int kNever = kLevels;  // "opens no cell at any level": the row's code equals the code before it
// per cloud, one zeroed block of words: [0, 6) bounds, [8, 20) rows per first-opened level, [kHdrHist, +4 * 256) select histograms
constexpr int kHdrCnt = 8, kHdrHist = 24, kHdrWords = kHdrHist + kSelectPasses * kSelectBins;
constexpr uint32_t kDead = 1u << 30;  // sort key = cloud << 31 | dead | code

struct GridPlan {  // per cloud, written by gs_mark_kernel
  int32_t level;   // L*, -1: not sampled
  int32_t r;       // stage-B picks
};

// the rows of cloud s that are sampled: n > m of a cloud whose status is OK, else 0 (uniform over the workgroup)
__device__ __forceinline__ int sampled_rows(const int32_t* counts, const int32_t* status, int s, int m, int64_t n_bound) {
  const int n = (int)min((int64_t)max(counts[s], 0), n_bound);
  return (status[s] == GPN_CLOUD_OK && n > m) ? n : 0;
}

__device__ __forceinline__ uint32_t spread3(uint32_t v) {  // bit i of v (i < 10) -> bit 3 i
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// the first level at which sorted row p opens a new cell: 0 for the cloud's first row, kNever when its code repeats
__device__ __forceinline__ int first_level(const uint64_t* __restrict__ keys, int p) {
  if (p == 0) return 0;
  const uint32_t d = ((uint32_t)keys[p] ^ (uint32_t)keys[p - 1]) & (kDead - 1u);
  if (d == 0) return kNever;
  return 10 - (31 - __clz(d)) / 3;  // cells of level L differ when a bit >= 30 - 3 L differs
}

// L* = the largest L with C_L <= m, and C_L* (cnt: rows per first-opened level; C_L is its running sum, C_0 = 1)
__device__ __forceinline__ int pick_level(const uint32_t* __restrict__ cnt, int m, int* cstar) {
  int c = 0, L = 0;
  for (int l = 0; l < kLevels; ++l) {
    c += (int)cnt[l];
    if (c <= m) { L = l; *cstar = c; }
  }
  return L;
}

// the sum of a[0 .. c) - a chunk's first slot from the per-chunk counts before it
__device__ __forceinline__ int chunk_prefix(const int32_t* __restrict__ a, int c, int* wsum) {
  int v = 0;
  for (int i = threadIdx.x; i < c; i += kThreads) v += a[i];
  return block_sum<kWaves>(v, wsum);
}

// ---- 1. bounds and the status rule -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gs_bounds_kernel(const float4* __restrict__ packed, int64_t n_bound,
                                                             const int32_t* __restrict__ counts, int32_t* __restrict__ status, int m,
                                                             uint32_t* __restrict__ hdr, int32_t* __restrict__ idx,
                                                             int32_t* __restrict__ level) {
  __shared__ uint32_t red[6][kWaves];
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int st = status[s];
  const int cnt = (int)min((int64_t)max(counts[s], 0), n_bound);
  const int n = (st == GPN_CLOUD_OK && cnt > m) ? cnt : 0;  // (a FEW written below by chunk 0 reads as "not sampled" as well)
  if (n == 0) {
    if (st == GPN_CLOUD_OK && cnt == m)
      for (int e = 0; e < kPer; ++e) {
        const int64_t j = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
        if (j < m) idx[(int64_t)s * m + j] = (int)j;
      }
    if (blockIdx.x == 0 && tid == 0) {
      level[s] = -1;
      if (st == GPN_CLOUD_OK && cnt < m) status[s] = GPN_CLOUD_FEW;
    }
    return;
  }
  if ((int64_t)blockIdx.x * kChunk >= n) return;
  uint32_t b[6] = {0u, 0u, 0u, 0u, 0u, 0u};  // [0, 3): ~image of the minimum, [3, 6): image of the maximum - both grow
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t j = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (j >= n) continue;
    const float4 p = packed[(int64_t)s * n_bound + j];
    const uint32_t k[3] = {f2ord(p.x), f2ord(p.y), f2ord(p.z)};
#pragma unroll
    for (int a = 0; a < 3; ++a) { b[a] = max(b[a], ~k[a]); b[3 + a] = max(b[3 + a], k[a]); }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) b[a] = max(b[a], (uint32_t)__shfl_xor((int)b[a], off, 64));
    if (lane == 0) red[a][wave] = b[a];
  }
  __syncthreads();
  if (tid < 6) {
    uint32_t v = red[tid][0];
    for (int w = 1; w < kWaves; ++w) v = max(v, red[tid][w]);
    atomicMax(hdr + (int64_t)s * kHdrWords + tid, v);  // (integer compare: order-free)
  }
}

// ---- 2. Morton codes and sort keys: every one of the S * n_bound slots gets a key ------------------------------------------------
__global__ __launch_bounds__(kThreads) void gs_keys_kernel(const float4* __restrict__ packed, int64_t n_bound,
                                                           const int32_t* __restrict__ counts, const int32_t* __restrict__ status,
                                                           int m, const uint32_t* __restrict__ hdr, uint64_t* __restrict__ keys,
                                                           uint32_t* __restrict__ vals) {
  const int s = blockIdx.y, tid = threadIdx.x;
  const int n = sampled_rows(counts, status, s, m, n_bound);
  float lo[3] = {0.f, 0.f, 0.f}, scale = 0.f;
  bool flat = true;
  if (n > 0) {
    const uint32_t* b = hdr + (int64_t)s * kHdrWords;
    float ext = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = ord2f(~b[a]);
      ext = fmaxf(ext, __fsub_rn(ord2f(b[3 + a]), lo[a]));
    }
    flat = !(ext > 0.f) || !finite_bits(ext);
    if (!flat) scale = (float)(1024.0 / (double)ext);
  }
  const uint64_t hi = (uint64_t)s << 31;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t j = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (j >= n_bound) continue;
    const int64_t g = (int64_t)s * n_bound + j;
    uint32_t code = kDead;
    if (j < n) {
      code = 0;
      if (!flat) {
        const float4 p = packed[g];
        const float c[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float x = __fmul_rn(__fsub_rn(c[a], lo[a]), scale);
          code |= spread3((uint32_t)(x < 1023.f ? x : 1023.f)) << a;  // (a NaN, 0 * inf, takes 1023)
        }
      }
    }
    keys[g] = hi | code;
    vals[g] = (uint32_t)j;
  }
}

// ---- 3. rows per first-opened level ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gs_levels_kernel(const uint64_t* __restrict__ keys, int64_t n_bound,
                                                             const int32_t* __restrict__ counts, const int32_t* __restrict__ status,
                                                             int m, uint32_t* __restrict__ hdr) {
  __shared__ uint32_t bins[kLevels + 1];
  const int s = blockIdx.y, tid = threadIdx.x;
  const int n = sampled_rows(counts, status, s, m, n_bound);
  if ((int64_t)blockIdx.x * kChunk >= n) return;
  if (tid <= kLevels) bins[tid] = 0;
  __syncthreads();
  const uint64_t* ks = keys + (int64_t)s * n_bound;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (p < n) atomicAdd(&bins[first_level(ks, (int)p)], 1u);
  }
  __syncthreads();
  if (tid <= kLevels && bins[tid]) atomicAdd(hdr + (int64_t)s * kHdrWords + kHdrCnt + tid, bins[tid]);  // (integer adds: order-free)
}

// ---- 4. stage A and the stage-B candidates -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gs_mark_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order,
                                                           int64_t n_bound, const int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ status, int m,
                                                           const uint32_t* __restrict__ hdr, GridPlan* __restrict__ plan,
                                                           uint8_t* __restrict__ flag, uint8_t* __restrict__ cand,
                                                           int32_t* __restrict__ level) {
  const int s = blockIdx.y, tid = threadIdx.x;
  const int n = sampled_rows(counts, status, s, m, n_bound);
  if (n == 0) {
    if (blockIdx.x == 0 && tid == 0) plan[s] = GridPlan{-1, 0};
    return;
  }
  int cstar = 1;
  const int L = pick_level(hdr + (int64_t)s * kHdrWords + kHdrCnt, m, &cstar);
  if (blockIdx.x == 0 && tid == 0) {
    plan[s] = GridPlan{L, m - cstar};
    level[s] = L;
  }
  const int64_t base = (int64_t)s * n_bound;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (p >= n) continue;
    const int lf = first_level(keys + base, (int)p);
    const int64_t j = min((int64_t)order[base + p], (int64_t)n - 1);  // (the sort's payload is a live row of this cloud)
    flag[base + j] = lf <= L ? 1 : 0;
    if (L < kLevels - 1)
      cand[base + p] = lf == L + 1 ? 1 : 0;  // the first row of a level-(L+1) cell that holds no stage-A point
    else
      cand[base + j] = lf == kNever ? 1 : 0;  // a point stage A did not take
  }
}

// the stage-B item of candidate slot q: the level-(L+1) cell of the sorted row for L < 10 (the 3 (L+1) top bits of its code), else the row
__device__ __forceinline__ uint32_t cand_item(const uint64_t* __restrict__ keys, int64_t q, int L) {
  if (L >= kLevels - 1) return (uint32_t)q;
  return ((uint32_t)keys[q] & (kDead - 1u)) >> (30 - 3 * (L + 1));
}

// ---- 5. radix select over the candidates: pass j's digit histogram -----------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gs_hist_kernel(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ cand,
                                                           int64_t n_bound, const int32_t* __restrict__ counts,
                                                           const uint32_t* __restrict__ seeds, const GridPlan* __restrict__ plan,
                                                           int hash_bits, int pass, uint32_t* __restrict__ hdr) {
  __shared__ int wsum[kWaves];
  __shared__ int sh[2];
  __shared__ uint32_t bins[kSelectBins];
  const int s = blockIdx.y, tid = threadIdx.x;
  const GridPlan pl = plan[s];
  if (pl.r <= 0) return;  // (uniform over the workgroup)
  const int n = (int)min((int64_t)counts[s], n_bound);
  if ((int64_t)blockIdx.x * kChunk >= n) return;
  uint32_t* hist = hdr + (int64_t)s * kHdrWords + kHdrHist;
  uint32_t prefix;
  int k;
  select_resolve<kWaves>(hist, pass, pl.r, wsum, sh, &prefix, &k);
  bins[tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)s * n_bound;
  const uint32_t seed = seeds[s];
  const int shift = 24 - 8 * pass;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t q = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (q >= n || !cand[base + q]) continue;
    const uint32_t hq = hash_key(seed, cand_item(keys + base, q, pl.level), hash_bits);
    if (pass == 0 || (hq >> (shift + 8)) == prefix) atomicAdd(&bins[(hq >> shift) & 255u], 1u);
  }
  __syncthreads();
  const uint32_t b = bins[tid];
  if (b) atomicAdd(hist + pass * kSelectBins + tid, b);  // (merged by integer adds: order-free)
}

// per chunk: the candidates on the threshold
__global__ __launch_bounds__(kThreads) void gs_ties_kernel(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ cand,
                                                           int64_t n_bound, const int32_t* __restrict__ counts,
                                                           const uint32_t* __restrict__ seeds, const GridPlan* __restrict__ plan,
                                                           int hash_bits, const uint32_t* __restrict__ hdr,
                                                           int32_t* __restrict__ chunk_eq) {
  __shared__ int wsum[kWaves];
  __shared__ int sh[2];
  const int s = blockIdx.y, tid = threadIdx.x;
  const GridPlan pl = plan[s];
  if (pl.r <= 0) return;
  const int n = (int)min((int64_t)counts[s], n_bound);
  if ((int64_t)blockIdx.x * kChunk >= n) return;
  uint32_t t;
  int k;
  select_resolve<kWaves>(hdr + (int64_t)s * kHdrWords + kHdrHist, kSelectPasses, pl.r, wsum, sh, &t, &k);
  const int64_t base = (int64_t)s * n_bound;
  const uint32_t seed = seeds[s];
  int eq = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t q = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (q >= n || !cand[base + q]) continue;
    eq += hash_key(seed, cand_item(keys + base, q, pl.level), hash_bits) == t ? 1 : 0;
  }
  eq = block_sum<kWaves>(eq, wsum);
  if (tid == 0) chunk_eq[(int64_t)s * gridDim.x + blockIdx.x] = eq;
}

// the picks: every candidate below the threshold and the first k on it in slot order
__global__ __launch_bounds__(kThreads) void gs_pick_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order,
                                                           const uint8_t* __restrict__ cand, int64_t n_bound,
                                                           const int32_t* __restrict__ counts, const uint32_t* __restrict__ seeds,
                                                           const GridPlan* __restrict__ plan, int hash_bits,
                                                           const uint32_t* __restrict__ hdr, const int32_t* __restrict__ chunk_eq,
                                                           uint8_t* __restrict__ flag) {
  __shared__ int wsum[kWaves];
  __shared__ int sh[2];
  __shared__ int wcnt[kPer][kWaves];
  const int s = blockIdx.y, tid = threadIdx.x;
  const GridPlan pl = plan[s];
  if (pl.r <= 0) return;
  const int n = (int)min((int64_t)counts[s], n_bound);
  if ((int64_t)blockIdx.x * kChunk >= n) return;
  uint32_t t;
  int k;
  select_resolve<kWaves>(hdr + (int64_t)s * kHdrWords + kHdrHist, kSelectPasses, pl.r, wsum, sh, &t, &k);
  const int eq_before = chunk_prefix(chunk_eq + (int64_t)s * gridDim.x, blockIdx.x, wsum);
  const int64_t base = (int64_t)s * n_bound;
  const uint32_t seed = seeds[s];
  bool lessf[kPer], eqf[kPer];
  int rank[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t q = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    const bool ok = q < n && cand[base + q] != 0;
    const uint32_t hq = ok ? hash_key(seed, cand_item(keys + base, q, pl.level), hash_bits) : 0u;
    lessf[e] = ok && hq < t;
    eqf[e] = ok && hq == t;
  }
  ordered_ranks<kWaves, kPer>(eqf, wcnt, eq_before, rank);
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    if (!(lessf[e] || (eqf[e] && rank[e] < k))) continue;
    const int64_t q = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    const int64_t j = pl.level < kLevels - 1 ? min((int64_t)order[base + q], (int64_t)n - 1) : q;
    flag[base + j] = 1;
  }
}

// ---- 6. the flagged rows in ascending order ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gs_count_kernel(const uint8_t* __restrict__ flag, int64_t n_bound,
                                                            const int32_t* __restrict__ counts, const GridPlan* __restrict__ plan,
                                                            int32_t* __restrict__ chunk_n) {
  __shared__ int wsum[kWaves];
  const int s = blockIdx.y, tid = threadIdx.x;
  if (plan[s].level < 0) return;
  const int n = (int)min((int64_t)counts[s], n_bound);
  if ((int64_t)blockIdx.x * kChunk >= n) return;
  int c = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t j = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    c += (j < n && flag[(int64_t)s * n_bound + j]) ? 1 : 0;
  }
  c = block_sum<kWaves>(c, wsum);
  if (tid == 0) chunk_n[(int64_t)s * gridDim.x + blockIdx.x] = c;
}

__global__ __launch_bounds__(kThreads) void gs_emit_kernel(const uint8_t* __restrict__ flag, int64_t n_bound,
                                                           const int32_t* __restrict__ counts, const GridPlan* __restrict__ plan,
                                                           const int32_t* __restrict__ chunk_n, int m, int32_t* __restrict__ idx) {
  __shared__ int wsum[kWaves];
  __shared__ int wcnt[kPer][kWaves];
  const int s = blockIdx.y, tid = threadIdx.x;
  if (plan[s].level < 0) return;
  const int n = (int)min((int64_t)counts[s], n_bound);
  if ((int64_t)blockIdx.x * kChunk >= n) return;
  const int before = chunk_prefix(chunk_n + (int64_t)s * gridDim.x, blockIdx.x, wsum);
  bool f[kPer];
  int pos[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t j = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    f[e] = j < n && flag[(int64_t)s * n_bound + j] != 0;
  }
  ordered_ranks<kWaves, kPer>(f, wcnt, before, pos);
#pragma unroll
  for (int e = 0; e < kPer; ++e)
    if (f[e] && pos[e] < m) idx[(int64_t)s * m + pos[e]] = (int)((int64_t)blockIdx.x * kChunk + e * kThreads + tid);
}

unsigned key_bits(int S) {
  unsigned b = 1;
  while (((int64_t)1 << b) < (int64_t)S) ++b;
  return 31u + b;
}

struct GridWs {
  uint32_t* hdr;
  GridPlan* plan;
  int32_t *chunk_eq, *chunk_n;
  uint64_t *keys, *keys_sorted;
  uint32_t *vals, *order;
  uint8_t *flag, *cand;
  char* prim;
  size_t prim_bytes, total;
};
GridWs grid_ws(void* ws, int S, int64_t n_bound) {
  const size_t N = (size_t)S * (size_t)n_bound, chunks = (size_t)S * (size_t)gpn::cdiv(n_bound, kChunk);
  gpn::WsCarver w(ws, ~(size_t)0);
  GridWs o;
  o.hdr = w.take<uint32_t>((size_t)S * kHdrWords);
  o.plan = w.take<GridPlan>((size_t)S);
  o.chunk_eq = w.take<int32_t>(chunks);
  o.chunk_n = w.take<int32_t>(chunks);
  o.keys = w.take<uint64_t>(N);
  o.keys_sorted = w.take<uint64_t>(N);
  o.vals = w.take<uint32_t>(N);
  o.order = w.take<uint32_t>(N);
  o.flag = w.take<uint8_t>(N);
  o.cand = w.take<uint8_t>(N);
  o.prim_bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, o.prim_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, N, 0u, key_bits(S), (hipStream_t) nullptr);
  o.prim = w.take<char>(o.prim_bytes);
  o.total = w.used;
  return o;
}

}  // namespace

extern "C" size_t gpn_cloud_grid_sample_ws_bytes(int S, int64_t n_bound) {
  if (S <= 0 || S > 65535 || n_bound <= 0 || (int64_t)S * n_bound >= (int64_t)0x7fffffff) return 0;
  return grid_ws(nullptr, S, n_bound).total;
}

extern "C" int gpn_cloud_grid_sample(const float* packed, int64_t n_bound, const int32_t* counts, int32_t* status,
                                     const uint32_t* seeds, int S, int m, int hash_bits, int32_t* idx, int32_t* level, void* ws,
                                     size_t ws_bytes, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(S >= 0 && S <= 65535 && m >= 1 && hash_bits >= 1 && hash_bits <= 32);
  GPN_CHECK_ARG(n_bound >= 1 && (int64_t)S * n_bound < (int64_t)0x7fffffff - kChunk);
  if (S == 0) return GPN_OK;
  GPN_CHECK_ARG(packed && counts && status && seeds && idx && level);
  GPN_CHECK_ARG(ws && ws_bytes >= gpn_cloud_grid_sample_ws_bytes(S, n_bound));
  const GridWs g = grid_ws(ws, S, n_bound);
  const float4* rows = reinterpret_cast<const float4*>(packed);
  const dim3 grid((unsigned)gpn::cdiv(n_bound, kChunk), (unsigned)S), block(kThreads);
  const size_t N = (size_t)S * (size_t)n_bound;
  GPN_CHECK_HIP(hipMemsetAsync(g.hdr, 0, (size_t)S * kHdrWords * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(gs_bounds_kernel, grid, block, 0, stream, rows, n_bound, counts, status, m, g.hdr, idx, level);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(gs_keys_kernel, grid, block, 0, stream, rows, n_bound, counts, status, m, g.hdr, g.keys, g.vals);
  GPN_CHECK_LAUNCH();
  size_t tmp = g.prim_bytes;
  GPN_CHECK_HIP(rocprim::radix_sort_pairs(g.prim, tmp, g.keys, g.keys_sorted, g.vals, g.order, N, 0u, key_bits(S), stream));
  hipLaunchKernelGGL(gs_levels_kernel, grid, block, 0, stream, g.keys_sorted, n_bound, counts, status, m, g.hdr);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(gs_mark_kernel, grid, block, 0, stream, g.keys_sorted, g.order, n_bound, counts, status, m, g.hdr, g.plan, g.flag,
                     g.cand, level);
  GPN_CHECK_LAUNCH();
  for (int pass = 0; pass < kSelectPasses; ++pass) {
    hipLaunchKernelGGL(gs_hist_kernel, grid, block, 0, stream, g.keys_sorted, g.cand, n_bound, counts, seeds, g.plan, hash_bits, pass,
                       g.hdr);
    GPN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(gs_ties_kernel, grid, block, 0, stream, g.keys_sorted, g.cand, n_bound, counts, seeds, g.plan, hash_bits, g.hdr,
                     g.chunk_eq);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(gs_pick_kernel, grid, block, 0, stream, g.keys_sorted, g.order, g.cand, n_bound, counts, seeds, g.plan, hash_bits,
                     g.hdr, g.chunk_eq, g.flag);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(gs_count_kernel, grid, block, 0, stream, g.flag, n_bound, counts, g.plan, g.chunk_n);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(gs_emit_kernel, grid, block, 0, stream, g.flag, n_bound, counts, g.plan, g.chunk_n, m, idx);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
