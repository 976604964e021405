// ground.hip — class labels for class-agnostic 2D masks (include/gpn.h section GR).  Reference: structure/utils.py:491-528
// (mask_change_reso, load_data_single_file, KNN_classifier), structure/gapartnet.py:145-158 (mask_fea_process /
// sam_mask_fea_process), :180-204 (get_GAPart_grounding_result / get_sam_grounding_result): every pixel mask is shrunk to the
// resolution of an image feature map, the masked map is max-pooled into one vector per mask, and that vector is classified by a
// 5-nearest-neighbour vote against a bank of labelled part features.
//
//  * mask_resize: Pillow's 8-bit bicubic resample as the two integer passes it is (ImagingResampleHorizontal_8bpc, then
//    ...Vertical_8bpc): out = clip8((2^21 + sum c * p) >> 22) with the host's coefficient tables.  The horizontal pass stages
//    kRowsPerWg rows of the mask in LDS as the bytes 128 (1 - m) and writes a [K, H, Wf] u8 intermediate; the vertical pass is a
//    thread per output byte.  All-integer: byte-equal to Pillow by construction, no rounding mode to match.
//  * mask_pool: feat[k, c] = max_p fea[view[k], p, c] * (128 - min(level[k, p], 128)) / 128.  A workgroup holds kPoolMasks masks
//    x 32 channels: 8 lanes of float4 along C (one 128-byte line of a map row), 32 pixel phases; the masks' levels come through
//    LDS in chunks, a map row is loaded once for all masks of the group that share its view, and the phases' maxima meet in LDS.
//    max is order-independent and each product is one fp32 rounding: bit-equal however the masks are grouped.
//  * knn: d2(q, b) = (|q|^2 + |b|^2) - 2 q.b with the dot products on v_mfma_f32_16x16x4_f32 (exact fp32, bitwise an fmaf chain in
//    a fixed k order).  A workgroup owns a tile of 64 queries and a slice of bank rows; it streams the slice in tiles of 128 rows
//    through LDS (K steps of 16, the next step's global loads in flight, the operand layout of pointmlp.hip), drops the 64 x 128
//    dot products into the same LDS, turns them into distances with all four waves, and lets one thread per query fold them into
//    that query's running top-k (a sorted list in LDS: after the first tiles almost every candidate fails the comparison with the
//    k-th entry; the thread reads eight distances at a time, so only an insertion waits for LDS).  A second launch merges the
//    slices' lists of a query (one wave: every lane walks the heads of its slices, a shuffle reduction picks the smallest
//    (d2, row) pair k times), counts the votes and picks the label.  (d2, row) is a total order, so the result does not depend on
//    the slicing, the tile a query sits in, or the other queries.  No float atomics, nothing read back.
#include "gpn_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- gpn_ground_mask_resize ---------------------------------------------------------------------------------------------------
constexpr int kResizeThreads = 256;
constexpr int kRowsPerWg = 8;  // mask rows staged per workgroup of the horizontal pass

__device__ __forceinline__ uint8_t clip8_22(int ss) {  // Pillow's clip8: (ss >> 22) saturated to 0..255
  const int v = ss >> 22;
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ __launch_bounds__(kResizeThreads) void resize_h_kernel(const uint8_t* __restrict__ masks, int H, int W, int Wf,
                                                                  const int32_t* __restrict__ xbounds, const int32_t* __restrict__ xcoef,
                                                                  int ksx, int vec, uint8_t* __restrict__ mid) {
  extern __shared__ uint8_t rows_sh[];  // [kRowsPerWg][Wp] bytes 128 (1 - m)
  const int Wp = (W + 3) & ~3;
  const int k = blockIdx.y, y0 = blockIdx.x * kRowsPerWg;
  const int nrows = H - y0 < kRowsPerWg ? H - y0 : kRowsPerWg;
  const uint8_t* src = masks + ((int64_t)k * H + y0) * W;
  if (vec) {  // W % 4 == 0 and an aligned base: four bytes a load
    const int wq = W >> 2;
    for (int e = threadIdx.x; e < nrows * wq; e += kResizeThreads) {
      const uint32_t m = reinterpret_cast<const uint32_t*>(src)[e];
      uint32_t p = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) p |= ((m >> (8 * b)) & 0xffu) ? 0u : (128u << (8 * b));
      reinterpret_cast<uint32_t*>(rows_sh)[(e / wq) * (Wp >> 2) + e % wq] = p;
    }
  } else {
    for (int e = threadIdx.x; e < nrows * W; e += kResizeThreads) rows_sh[(e / W) * Wp + e % W] = src[e] ? 0 : 128;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nrows * Wf; e += kResizeThreads) {
    const int r = e / Wf, xo = e % Wf;
    const int xmin = xbounds[xo * 2], n = xbounds[xo * 2 + 1];  // (validated on the host: 0 <= xmin, xmin + n <= W, n <= ksx)
    const int32_t* c = xcoef + (int64_t)xo * ksx;
    const uint8_t* p = rows_sh + r * Wp + xmin;
    int ss = 1 << 21;
    for (int x = 0; x < n; ++x) ss += (int)p[x] * c[x];
    mid[((int64_t)k * H + y0 + r) * Wf + xo] = clip8_22(ss);
  }
}

__global__ __launch_bounds__(kResizeThreads) void resize_v_kernel(const uint8_t* __restrict__ mid, int H, int Wf, int Hf,
                                                                  const int32_t* __restrict__ ybounds, const int32_t* __restrict__ ycoef,
                                                                  int ksy, int64_t total, uint8_t* __restrict__ levels) {
  const int64_t e = (int64_t)blockIdx.x * kResizeThreads + threadIdx.x;
  if (e >= total) return;
  const int xo = (int)(e % Wf), yo = (int)((e / Wf) % Hf);
  const int64_t k = e / ((int64_t)Wf * Hf);
  const int ymin = ybounds[yo * 2], n = ybounds[yo * 2 + 1];
  const int32_t* c = ycoef + (int64_t)yo * ksy;
  const uint8_t* p = mid + (k * H + ymin) * Wf + xo;
  int ss = 1 << 21;
  for (int y = 0; y < n; ++y) ss += (int)p[(int64_t)y * Wf] * c[y];
  const uint8_t v = clip8_22(ss);
  levels[e] = v > 128 ? 128 : v;  // the reference's clip(0, 128)
}

// a coefficient table as Pillow lays it out: bounds [n_out, 2] = (first input index, count), coef [n_out, ksize]
bool table_ok(const int32_t* bounds, int n_out, int ksize, int n_in) {
  for (int i = 0; i < n_out; ++i) {
    const int64_t lo = bounds[i * 2], n = bounds[i * 2 + 1];
    if (lo < 0 || n < 0 || n > ksize || lo + n > n_in) return false;
  }
  return true;
}

// ---- gpn_ground_mask_pool -----------------------------------------------------------------------------------------------------
constexpr int kPoolThreads = 256;
constexpr int kPoolMasks = 8;    // masks of a workgroup: their running maxima live in registers
constexpr int kPoolLanes = 8;    // float4 lanes along C: 32 channels (one 128-byte line of a map row) a workgroup
constexpr int kPoolPhases = kPoolThreads / kPoolLanes;
constexpr int kPoolChunk = 2048;  // pixels whose levels are staged in LDS at a time

__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }  // a NaN stays, as in np.max

__global__ __launch_bounds__(kPoolThreads) void mask_pool_kernel(const float* __restrict__ fea, const uint8_t* __restrict__ levels,
                                                                 const int32_t* __restrict__ mask_view, int V, int P, int C, int K,
                                                                 int vec, float* __restrict__ feat) {
  __shared__ float red[kPoolPhases][kPoolMasks][kPoolLanes * 4];
  __shared__ uint8_t lv_sh[kPoolMasks][kPoolChunk];
  const int lane = threadIdx.x % kPoolLanes, phase = threadIdx.x / kPoolLanes;
  const int c0 = blockIdx.x * kPoolLanes * 4 + lane * 4;
  const int k0 = blockIdx.y * kPoolMasks;
  const int nk = K - k0 < kPoolMasks ? K - k0 : kPoolMasks;
  int view[kPoolMasks];
#pragma unroll
  for (int g = 0; g < kPoolMasks; ++g) {
    const int v = g < nk ? mask_view[k0 + g] : 0;
    view[g] = v < 0 ? 0 : (v >= V ? V - 1 : v);  // (checked by the wrapper; clamped so that a bad entry cannot leave the buffer)
  }
  f32x4 mx[kPoolMasks];
#pragma unroll
  for (int g = 0; g < kPoolMasks; ++g) mx[g] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int p0 = 0; p0 < P; p0 += kPoolChunk) {  // (uniform over the workgroup, and so are the barriers)
    const int cnt = P - p0 < kPoolChunk ? P - p0 : kPoolChunk;
    __syncthreads();  // the previous chunk's levels have been read
    for (int e = threadIdx.x; e < nk * cnt; e += kPoolThreads) lv_sh[e / cnt][e % cnt] = levels[(int64_t)(k0 + e / cnt) * P + p0 + e % cnt];
    __syncthreads();
#pragma unroll 2
    for (int i = c0 < C ? phase : cnt; i < cnt; i += kPoolPhases) {
      const int p = p0 + i;
      f32x4 f = {0.f, 0.f, 0.f, 0.f};
      int have = -1;
#pragma unroll
      for (int g = 0; g < kPoolMasks; ++g) {
        if (g >= nk) break;  // (uniform over the workgroup)
        if (view[g] != have) {  // the map row is loaded once for the run of masks that share the view
          have = view[g];
          const float* src = fea + ((int64_t)have * P + p) * C + c0;
          if (vec) {
            f = *reinterpret_cast<const f32x4*>(src);
          } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) f[u] = c0 + u < C ? src[u] : 0.f;
          }
        }
        const int lv = lv_sh[g][i];
        const float w = (float)(128 - (lv > 128 ? 128 : lv)) * 0.0078125f;  // a multiple of 1/128: exact
#pragma unroll
        for (int u = 0; u < 4; ++u) mx[g][u] = nanmax(mx[g][u], f[u] * w);
      }
    }
  }
#pragma unroll
  for (int g = 0; g < kPoolMasks; ++g)
#pragma unroll
    for (int u = 0; u < 4; ++u) red[phase][g][lane * 4 + u] = mx[g][u];
  __syncthreads();
  for (int e = threadIdx.x; e < kPoolMasks * kPoolLanes * 4; e += kPoolThreads) {
    const int g = e / (kPoolLanes * 4), cc = e % (kPoolLanes * 4);
    const int c = blockIdx.x * kPoolLanes * 4 + cc;
    if (g >= nk || c >= C) continue;
    float m = red[0][g][cc];
    for (int ph = 1; ph < kPoolPhases; ++ph) m = nanmax(m, red[ph][g][cc]);
    feat[(int64_t)(k0 + g) * C + c] = m;
  }
}

// ---- gpn_ground_bank_norms ----------------------------------------------------------------------------------------------------
// one wave per row: lane l sums the squares of elements l, l + 64, ... in order, then six shuffle steps: a fixed shape
constexpr int kNormThreads = 256;
__global__ __launch_bounds__(kNormThreads) void row_norms_kernel(const float* __restrict__ x, int64_t M, int D, float* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * (kNormThreads / 64) + (threadIdx.x >> 6);
  if (row >= M) return;  // (whole waves leave; no barrier follows)
  const int lane = threadIdx.x & 63;
  const float* p = x + row * D;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s = fmaf(p[d], p[d], s);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) out[row] = s;
}

// ---- gpn_ground_knn -----------------------------------------------------------------------------------------------------------
constexpr int kKnnThreads = 256;
constexpr int kQT = 64;            // queries of a workgroup
constexpr int kBT = 128;           // bank rows of a tile
constexpr int kBK = 16;            // K per LDS stage
constexpr int kPitch = kBK + 4;    // floats per LDS row of a stage (conflict-free ds_read_b128, as in pointmlp.hip)
constexpr int kDistPitch = kBT + 1;
constexpr int kListPitch = GPN_GROUND_MAX_K + 1;
constexpr int kKnnTargetWgs = 512;  // slices x query tiles the sweep aims at: two workgroups a CU
constexpr int kNoRow = 0x7fffffff;

// slices of the bank for Q queries and M rows: whole tiles of kBT rows, about kKnnTargetWgs workgroups in all
inline int knn_slices(int64_t Q, int64_t M, int* tiles_per_slice) {
  const int64_t qt = gpn::cdiv(Q > 0 ? Q : 1, kQT), tiles = gpn::cdiv(M > 0 ? M : 1, kBT);
  int64_t want = gpn::cdiv(kKnnTargetWgs, qt);
  if (want > tiles) want = tiles;
  const int64_t per = gpn::cdiv(tiles, want);
  *tiles_per_slice = (int)per;
  return (int)gpn::cdiv(tiles, per);
}

__device__ __forceinline__ bool before(float d, int i, float ld, int li) { return d < ld || (d == ld && i < li); }

// 16 bytes k .. k + 3 of row `row` of a [rows, D] matrix; zero past the rows and past D
__device__ __forceinline__ f32x4 load_row4(const float* __restrict__ x, int64_t rows, int D, int64_t row, int k, int vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row >= rows || k >= D) return v;
  const float* p = x + row * D + k;
  if (vec) return *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (k + u < D) v[u] = p[u];
  return v;
}

__global__ __launch_bounds__(kKnnThreads) void knn_sweep_kernel(const float* __restrict__ queries, const float* __restrict__ bank,
                                                                const float* __restrict__ qnorm, const float* __restrict__ bnorm,
                                                                int64_t Q, int64_t M, int D, int k, int tiles_per_slice, int S, int vec,
                                                                float* __restrict__ cand_d, int32_t* __restrict__ cand_i) {
  // the stage buffers and the distance tile share their LDS: a tile's distances are written behind its last stage's reads
  static_assert(kQT * kDistPitch >= (kQT + kBT) * kPitch, "the stage buffers fit under the distance tile");
  __shared__ __attribute__((aligned(16))) float buf[kQT * kDistPitch];
  float* const As = buf;                 // [kQT][kPitch]
  float* const Bs = buf + kQT * kPitch;  // [kBT][kPitch]
  float* const dist = buf;               // [kQT][kDistPitch]
  __shared__ float bn_sh[kBT];
  __shared__ float list_d[kQT * kListPitch];
  __shared__ int list_i[kQT * kListPitch];

  const int slice = blockIdx.x;
  const int64_t q0 = (int64_t)blockIdx.y * kQT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, q4 = lane >> 4;
  const int64_t b_begin = (int64_t)slice * tiles_per_slice * kBT;
  int64_t b_end = b_begin + (int64_t)tiles_per_slice * kBT;
  if (b_end > M) b_end = M;

  if (tid < kQT)
    for (int j = 0; j < k; ++j) list_d[tid * kListPitch + j] = INFINITY, list_i[tid * kListPitch + j] = kNoRow;
  const float qn = q0 + lane < Q ? qnorm[q0 + lane] : 0.f;  // (thread (lane, wave) turns dot products of query `lane` into distances)

  for (int64_t b0 = b_begin; b0 < b_end; b0 += kBT) {  // (uniform over the workgroup)
    // the tile's bank norms: written here, read after the K loop's barriers; the previous tile's readers are behind a barrier
    if (tid < kBT) bn_sh[tid] = b0 + tid < b_end ? bnorm[b0 + tid] : 0.f;
    f32x4 acc[4][2];  // the wave's 64 queries x 32 bank rows: 8 independent chains
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ra, rb[2];
    ra = load_row4(queries, Q, D, q0 + (tid >> 2), (tid & 3) * 4, vec);
#pragma unroll
    for (int u = 0; u < 2; ++u) rb[u] = load_row4(bank, b_end, D, b0 + ((tid + u * kKnnThreads) >> 2), (tid & 3) * 4, vec);
    for (int k0 = 0; k0 < D; k0 += kBK) {
      __syncthreads();  // the previous stage's reads (and the previous tile's fold) are done
      *reinterpret_cast<f32x4*>(&As[(tid >> 2) * kPitch + (tid & 3) * 4]) = ra;
#pragma unroll
      for (int u = 0; u < 2; ++u) *reinterpret_cast<f32x4*>(&Bs[((tid + u * kKnnThreads) >> 2) * kPitch + (tid & 3) * 4]) = rb[u];
      __syncthreads();
      if (k0 + kBK < D) {  // the next stage's loads fly under this stage's MFMAs
        ra = load_row4(queries, Q, D, q0 + (tid >> 2), k0 + kBK + (tid & 3) * 4, vec);
#pragma unroll
        for (int u = 0; u < 2; ++u)
          rb[u] = load_row4(bank, b_end, D, b0 + ((tid + u * kKnnThreads) >> 2), k0 + kBK + (tid & 3) * 4, vec);
      }
      f32x4 fa[4], fb[2];
#pragma unroll
      for (int t = 0; t < 4; ++t) fa[t] = *reinterpret_cast<const f32x4*>(&As[(t * 16 + i16) * kPitch + q4 * 4]);
#pragma unroll
      for (int n = 0; n < 2; ++n) fb[n] = *reinterpret_cast<const f32x4*>(&Bs[((wave * 2 + n) * 16 + i16) * kPitch + q4 * 4]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int n = 0; n < 2; ++n) acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t][j], fb[n][j], acc[t][n], 0, 0, 0);
    }
    __syncthreads();  // every wave has read its last stage: the distance tile may overwrite it
    // lane (i16, q4) holds queries t * 16 + 4 q4 + v at bank row (wave * 2 + n) * 16 + i16 of the tile
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int col = (wave * 2 + n) * 16 + i16;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) dist[(t * 16 + 4 * q4 + v) * kDistPitch + col] = acc[t][n][v];
    }
    __syncthreads();
    // dot products -> distances, in place and by all four waves: wave w takes bank rows 32 w .. 32 w + 31 of every query
#pragma unroll 8
    for (int c = wave * (kBT / 4); c < (wave + 1) * (kBT / 4); ++c) {
      const float d = (qn + bn_sh[c]) - 2.f * dist[lane * kDistPitch + c];
      dist[lane * kDistPitch + c] = d < 0.f ? 0.f : d;  // (a NaN passes through and never enters a list)
    }
    __syncthreads();
    if (tid < kQT && q0 + tid < Q) {  // one thread per query folds the tile into its list, bank rows ascending
      float* ld = list_d + tid * kListPitch;
      int* li = list_i + tid * kListPitch;
      const int cnt = b_end - b0 < kBT ? (int)(b_end - b0) : kBT;
      float worst_d = ld[k - 1];
      int worst_i = li[k - 1];
      for (int c0 = 0; c0 < cnt; c0 += 8) {
        float d8[8];  // (read together: the reads of a group do not wait for the comparisons of the one before)
#pragma unroll
        for (int u = 0; u < 8; ++u) d8[u] = dist[tid * kDistPitch + c0 + u];  // (c0 + u < kBT: inside the tile's row)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int row = (int)(b0 + c0 + u);
          const float d = d8[u];
          if (c0 + u < cnt && before(d, row, worst_d, worst_i)) {
            int p = k - 1;
            while (p > 0 && before(d, row, ld[p - 1], li[p - 1])) ld[p] = ld[p - 1], li[p] = li[p - 1], --p;
            ld[p] = d, li[p] = row;
            worst_d = ld[k - 1], worst_i = li[k - 1];
          }
        }
      }
    }
    // (the next tile's first barrier orders this fold before the next write into the shared LDS)
  }
  __syncthreads();
  for (int e = tid; e < kQT * k; e += kKnnThreads) {
    const int q = e / k, j = e % k;
    if (q0 + q >= Q) continue;
    const int64_t o = ((q0 + q) * S + slice) * k + j;
    cand_d[o] = list_d[q * kListPitch + j], cand_i[o] = list_i[q * kListPitch + j];
  }
}

// one wave per query: the k smallest (d2, row) pairs of its S sorted lists, the votes of their labels, the label
__global__ __launch_bounds__(64) void knn_merge_kernel(const float* __restrict__ cand_d, const int32_t* __restrict__ cand_i, int S,
                                                       int k, const int32_t* __restrict__ bank_labels, int n_classes,
                                                       int32_t* __restrict__ nn_index, float* __restrict__ nn_d2,
                                                       int32_t* __restrict__ votes, int32_t* __restrict__ label) {
  constexpr int kMaxOwn = kKnnTargetWgs / 64;  // S <= kKnnTargetWgs: at most this many lists a lane
  __shared__ int lab_sh[GPN_GROUND_MAX_K];
  __shared__ int vote_sh[GPN_GROUND_MAX_CLASSES];
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x;
  const float* cd = cand_d + q * S * k;
  const int32_t* ci = cand_i + q * S * k;
  int head[kMaxOwn];
#pragma unroll
  for (int u = 0; u < kMaxOwn; ++u) head[u] = 0;
  int my_row = kNoRow;  // lane j keeps the j-th neighbour
  float my_d = INFINITY;
  for (int j = 0; j < k; ++j) {
    float bd = INFINITY;
    int bi = kNoRow, bu = -1;
#pragma unroll
    for (int u = 0; u < kMaxOwn; ++u) {
      const int s = lane + u * 64;
      if (s < S && head[u] < k) {
        const float d = cd[s * k + head[u]];
        const int i = ci[s * k + head[u]];
        if (bu < 0 || before(d, i, bd, bi)) bd = d, bi = i, bu = u;
      }
    }
    float wd = bd;
    int wi = bi;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float od = __shfl_xor(wd, o);
      const int oi = __shfl_xor(wi, o);
      if (before(od, oi, wd, wi)) wd = od, wi = oi;
    }
    if (bu >= 0 && bi == wi && bd == wd) {  // the winner's lane moves on (rows are unique; empty entries may move together)
#pragma unroll
      for (int u = 0; u < kMaxOwn; ++u)
        if (u == bu) ++head[u];
    }
    if (lane == j) my_row = wi, my_d = wd;
  }
  if (lane < k) {
    const bool have = my_row != kNoRow;
    nn_index[q * k + lane] = have ? my_row : -1;
    nn_d2[q * k + lane] = my_d;
    const int l = have ? bank_labels[my_row] : -1;
    lab_sh[lane] = (l >= 0 && l < n_classes) ? l : -1;  // (labels are checked where the bank is built; a bad one casts no vote)
  }
  __syncthreads();
  if (lane < n_classes) {
    int v = 0;
    for (int j = 0; j < k; ++j) v += lab_sh[j] == lane ? 1 : 0;
    vote_sh[lane] = v;
    votes[q * n_classes + lane] = v;
  }
  __syncthreads();
  if (lane == 0) {
    int best = 0;
    for (int c = 1; c < n_classes; ++c)
      if (vote_sh[c] > vote_sh[best]) best = c;  // equal votes: the smallest class id
    label[q] = best;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int gpn_ground_mask_resize(const uint8_t* masks, int K, int H, int W, int Hf, int Wf, const int32_t* xbounds_host,
                                      const int32_t* xcoef_host, int ksize_x, const int32_t* ybounds_host, const int32_t* ycoef_host,
                                      int ksize_y, const int32_t* tables_dev, uint8_t* levels, void* ws, size_t ws_bytes,
                                      gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(K >= 0 && K <= 65535 && H >= 1 && W >= 1 && H <= GPN_GROUND_MAX_SIDE && W <= GPN_GROUND_MAX_SIDE);
  GPN_CHECK_ARG(Hf >= 1 && Wf >= 1 && Hf <= GPN_GROUND_MAX_SIDE && Wf <= GPN_GROUND_MAX_SIDE && ksize_x >= 1 && ksize_y >= 1);
  GPN_CHECK_ARG(xbounds_host && xcoef_host && ybounds_host && ycoef_host);
  GPN_CHECK_ARG(table_ok(xbounds_host, Wf, ksize_x, W) && table_ok(ybounds_host, Hf, ksize_y, H));
  if (K == 0) return GPN_OK;
  GPN_CHECK_ARG(masks && tables_dev && levels);
  gpn::WsCarver carve(ws, ws_bytes);
  uint8_t* mid = carve.take<uint8_t>((size_t)K * H * Wf);
  GPN_CHECK_WS(carve);
  // tables_dev: the four host tables back to back, as the wrapper uploaded them: xbounds | xcoef | ybounds | ycoef
  const int32_t* xb = tables_dev;
  const int32_t* xc = xb + (size_t)Wf * 2;
  const int32_t* yb = xc + (size_t)Wf * ksize_x;
  const int32_t* yc = yb + (size_t)Hf * 2;
  const int Wp = (W + 3) & ~3;
  const int vec = (W % 4 == 0 && (reinterpret_cast<uintptr_t>(masks) & 3) == 0) ? 1 : 0;
  hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)gpn::cdiv(H, kRowsPerWg), (unsigned)K), dim3(kResizeThreads),
                     (size_t)kRowsPerWg * Wp, stream, masks, H, W, Wf, xb, xc, ksize_x, vec, mid);
  GPN_CHECK_LAUNCH();
  const int64_t total = (int64_t)K * Hf * Wf;
  GPN_CHECK_ARG(gpn::cdiv(total, kResizeThreads) <= 0x7fffffff);
  hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)gpn::cdiv(total, kResizeThreads)), dim3(kResizeThreads), 0, stream, mid, H, Wf,
                     Hf, yb, yc, ksize_y, total, levels);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" size_t gpn_ground_mask_resize_ws_bytes(int K, int H, int Wf) {
  if (K < 0 || H < 0 || Wf < 0) return 0;
  return gpn::align_up((size_t)K * H * Wf);
}

extern "C" int gpn_ground_mask_pool(const float* fea, const uint8_t* levels, const int32_t* mask_view, int V, int Hf, int Wf, int C,
                                    int K, float* feat, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(V >= 1 && Hf >= 1 && Wf >= 1 && C >= 1 && K >= 0 && (int64_t)Hf * Wf <= 0x7fffffff);
  GPN_CHECK_ARG(gpn::cdiv(K, kPoolMasks) <= 65535);
  if (K == 0) return GPN_OK;
  GPN_CHECK_ARG(fea && levels && mask_view && feat);
  const int vec = (C % 4 == 0 && aligned16(fea)) ? 1 : 0;
  hipLaunchKernelGGL(mask_pool_kernel, dim3((unsigned)gpn::cdiv(C, kPoolLanes * 4), (unsigned)gpn::cdiv(K, kPoolMasks)),
                     dim3(kPoolThreads), 0, stream, fea, levels, mask_view, V, Hf * Wf, C, K, vec, feat);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_ground_bank_norms(const float* bank, int64_t M, int D, float* norms, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(M >= 0 && M <= 0x7fffffff && D >= 1);
  if (M == 0) return GPN_OK;
  GPN_CHECK_ARG(bank && norms);
  hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)gpn::cdiv(M, kNormThreads / 64)), dim3(kNormThreads), 0, stream, bank, M, D,
                     norms);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" size_t gpn_ground_knn_ws_bytes(int64_t Q, int64_t M, int k) {
  if (Q < 0 || M < 0 || k < 1 || k > GPN_GROUND_MAX_K) return 0;
  int per;
  const int S = knn_slices(Q, M, &per);
  return gpn::align_up((size_t)Q * sizeof(float)) + 2 * gpn::align_up((size_t)Q * S * k * sizeof(float));
}

extern "C" int gpn_ground_knn(const float* queries, int64_t Q, const float* bank, const float* bank_norms, const int32_t* bank_labels,
                              int64_t M, int D, int k, int n_classes, int32_t* nn_index, float* nn_d2, int32_t* votes, int32_t* label,
                              void* ws, size_t ws_bytes, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(k >= 1 && k <= GPN_GROUND_MAX_K && D >= 1 && n_classes >= 1 && n_classes <= GPN_GROUND_MAX_CLASSES);
  GPN_CHECK_ARG(M >= k && M <= 0x7fffffff - kBT && Q >= 0 && Q <= (int64_t)65535 * kQT);
  if (Q == 0) return GPN_OK;
  GPN_CHECK_ARG(queries && bank && bank_norms && bank_labels && nn_index && nn_d2 && votes && label);
  int per;
  const int S = knn_slices(Q, M, &per);
  gpn::WsCarver carve(ws, ws_bytes);
  float* qnorm = carve.take<float>((size_t)Q);
  float* cand_d = carve.take<float>((size_t)Q * S * k);
  int32_t* cand_i = carve.take<int32_t>((size_t)Q * S * k);
  GPN_CHECK_WS(carve);
  hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)gpn::cdiv(Q, kNormThreads / 64)), dim3(kNormThreads), 0, stream, queries, Q, D,
                     qnorm);
  GPN_CHECK_LAUNCH();
  const int vec = (D % 4 == 0 && aligned16(queries) && aligned16(bank)) ? 1 : 0;
  hipLaunchKernelGGL(knn_sweep_kernel, dim3((unsigned)S, (unsigned)gpn::cdiv(Q, kQT)), dim3(kKnnThreads), 0, stream, queries, bank,
                     qnorm, bank_norms, Q, M, D, k, per, S, vec, cand_d, cand_i);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)Q), dim3(64), 0, stream, cand_d, cand_i, S, k, bank_labels, n_classes, nn_index,
                     nn_d2, votes, label);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
