// cloudprep.hip — unlabelled raw point clouds -> the network's input, and the network's per-sample predictions -> every row of the
// caller's cloud (include/gpn.h section CP).  A batch of S ragged clouds (rows offsets[s]:offsets[s+1] of points [M, stride]):
//   pack     the rows whose three coordinates are finite, in ascending row order, into the layout gpn_view_fps reads (a scan per
//            tile, no atomic counter); per-cloud counts and statuses
//   (fps)    gpn_view_fps as it is (viewprep.hip): counts > m sampled, == m arange, < m flagged = "keep every valid point"
//   finish   per cloud over its m_s = min(count, m) samples, float64: centre (max + min) / 2, r = sqrt(max((dx^2 + dy^2) + dz^2))
//            (point_prims.h, ball_of_samples - as gpn_view_finish), xyz = float32((p - c) / r); the other columns copied bit for bit
//   nearest  for every caller row the nearest sample of its cloud (fp32 (dx^2 + dy^2) + dz^2 without fma, ties to the lowest
//            sample): a per-cloud uniform grid over the samples' box (histogram, scan, stable scatter), queries walk Chebyshev
//            rings of cells and stop when no unvisited ring can beat the best distance; exact, with a scan of all samples after
//            kMaxRings rings
// No float atomics; every result is independent of timing.
#include <cmath>

#include "gpn_common.h"
#include "point_prims.h"

namespace {

using namespace gpn;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerThread = 4;  // pack: consecutive rows per thread and tile step
constexpr int kMaxRes = 64;        // nearest: cells along the box's longest axis, at most
constexpr int kMaxCells = kMaxRes * kMaxRes * kMaxRes;
constexpr int kMaxRings = 3;       // nearest: rings 0 .. kMaxRings around the query's cell, then all samples
constexpr int kQueryThreads = 256;

struct CloudGrid {  // per cloud, written by cn_build_kernel
  float mn[3], mx[3];  // the samples' box (exact)
  float h, inv_h;      // cell edge and its inverse (0, 0: one cell)
  int dims[3];
  int n;               // samples (0: the cloud has none - status not OK)
};

// rows [lo, lo + n) of the caller's array that cloud s owns, clamped so that nothing outside [0, M) or past n_bound is touched
__device__ __forceinline__ int cloud_rows(const int64_t* offsets, int s, int64_t M, int64_t n_bound, int64_t* lo_out) {
  int64_t lo = offsets[s], hi = offsets[s + 1];
  lo = lo < 0 ? 0 : (lo > M ? M : lo);
  hi = hi < lo ? lo : (hi > M ? M : hi);
  *lo_out = lo;
  const int64_t n = hi - lo;
  return (int)(n < n_bound ? n : n_bound);
}

// ---- 1. pack: one workgroup per cloud, tiles of kThreads * kRowsPerThread rows (the compaction of vp_backproject_kernel) ------
__global__ __launch_bounds__(kThreads) void cp_pack_kernel(const float* __restrict__ points, int stride,
                                                           const int64_t* __restrict__ offsets, int64_t M, int64_t n_bound,
                                                           float4* __restrict__ packed, int32_t* __restrict__ rows,
                                                           int32_t* __restrict__ counts, int32_t* __restrict__ status) {
  __shared__ int wsum[kWaves];
  const int s = blockIdx.x, tid = threadIdx.x;
  int64_t lo;
  const int n = cloud_rows(offsets, s, M, n_bound, &lo);
  const float* src = points + lo * stride;
  float4* dp = packed + (int64_t)s * n_bound;
  int32_t* dr = rows + (int64_t)s * n_bound;
  int base = 0;
  for (int64_t p0 = 0; p0 < n; p0 += kThreads * kRowsPerThread) {
    const int64_t q0 = p0 + (int64_t)tid * kRowsPerThread;
    float x[kRowsPerThread], y[kRowsPerThread], z[kRowsPerThread];
    unsigned vm = 0;
    int c = 0;
#pragma unroll
    for (int e = 0; e < kRowsPerThread; ++e) {
      const int64_t p = q0 + e;
      x[e] = y[e] = z[e] = 0.f;
      if (p < n) {
        const float* q = src + p * stride;
        x[e] = q[0]; y[e] = q[1]; z[e] = q[2];
        if (finite_bits(x[e]) && finite_bits(y[e]) && finite_bits(z[e])) {
          vm |= 1u << e;
          ++c;
        }
      }
    }
    int total;
    int pos = base + block_scan<kWaves>(c, wsum, &total) - c;
#pragma unroll
    for (int e = 0; e < kRowsPerThread; ++e) {
      if (vm >> e & 1u) {
        dp[pos] = make_float4(x[e], y[e], z[e], 1e10f);
        dr[pos] = (int)(q0 + e);
        ++pos;
      }
    }
    base += total;
  }
  if (tid == 0) {
    counts[s] = base;
    status[s] = base > 0 ? GPN_CLOUD_OK : GPN_CLOUD_EMPTY;
  }
}

// ---- 2. finish: one workgroup per cloud -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cp_finish_kernel(const float* __restrict__ points, int stride, int cols,
                                                             const int64_t* __restrict__ offsets, int64_t M, int64_t n_bound,
                                                             const int32_t* __restrict__ rows, const int32_t* __restrict__ counts,
                                                             const int32_t* __restrict__ idx, int m, int32_t* __restrict__ status,
                                                             float* __restrict__ out, int32_t* __restrict__ sample_rows,
                                                             double* __restrict__ scale) {
  __shared__ double red[6][kWaves];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int st = status[s];
  int64_t lo;
  const int n_rows = cloud_rows(offsets, s, M, n_bound, &lo);
  const bool keep_all = st == GPN_CLOUD_FEW;  // gpn_view_fps: fewer valid points than m, no indices written
  int n = 0;
  if (st == GPN_CLOUD_OK || keep_all) n = min(max(counts[s], 0), n_rows);
  const int ms = min(n, m);
  float* o = out + (int64_t)s * m * cols;  // (rows of `cols` floats; the caller's rows are `stride` floats apart)
  int32_t* sr = sample_rows + (int64_t)s * m;
  for (int64_t e = (int64_t)ms * cols + tid; e < (int64_t)m * cols; e += kThreads) o[e] = 0.f;
  for (int j = ms + tid; j < m; j += kThreads) sr[j] = -1;
  if (ms == 0) {
    if (tid < 4) scale[(int64_t)s * 4 + tid] = 0.0;
    return;
  }
  const float* src = points + lo * stride;
  const int32_t* fi = idx + (int64_t)s * m;
  const int32_t* rw = rows + (int64_t)s * n_bound;
  // the caller's row of sample j (an index gpn_view_fps wrote is in [0, n); the clamp keeps a stale one inside the cloud)
  auto row_of = [&](int j) {
    const int sel = keep_all ? j : min(max(fi[j], 0), n - 1);
    return min(max(rw[sel], 0), n_rows - 1);
  };
  double ctr[3], r;
  ball_of_samples<kWaves>(
      [&](int j, double* P) {
        const float* p = src + (int64_t)row_of(j) * stride;
        P[0] = (double)p[0]; P[1] = (double)p[1]; P[2] = (double)p[2];
      },
      ms, red, ctr, &r);
  const bool degenerate = !(r > 0.0);
  for (int j = tid; j < ms; j += kThreads) {
    const int row = row_of(j);
    const float* p = src + (int64_t)row * stride;
    float* q = o + (int64_t)j * cols;
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = degenerate ? 0.f : (float)(((double)p[c] - ctr[c]) / r);
    for (int c = 3; c < cols; ++c) reinterpret_cast<uint32_t*>(q)[c] = reinterpret_cast<const uint32_t*>(p)[c];
    sr[j] = row;
  }
  if (tid == 0) {
    status[s] = degenerate ? GPN_CLOUD_DEGENERATE : GPN_CLOUD_OK;
    scale[(int64_t)s * 4] = r;
    for (int c = 0; c < 3; ++c) scale[(int64_t)s * 4 + 1 + c] = ctr[c];
  }
}

// ---- 3. nearest sample ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cell_axis(float v, float mn, float inv_h, int dim) {
  // fmaxf / fminf drop a NaN (inf * 0): cell 0
  const float u = fminf(fmaxf(floorf(__fmul_rn(__fsub_rn(v, mn), inv_h)), 0.f), (float)(dim - 1));
  return (int)u;
}

// One workgroup per cloud: the samples' box, the grid, a histogram of the samples over its cells, its scan, and a STABLE scatter
// (a cell keeps its samples in ascending sample order): `cells[c]` ends as the END of cell c in `sorted`, so cell c is
// sorted[cells[c - 1] : cells[c]] (from 0 for c == 0).  sorted[i] = (x, y, z, sample index as bits).
__global__ __launch_bounds__(kThreads) void cn_build_kernel(const float* __restrict__ points, int stride,
                                                            const int64_t* __restrict__ offsets, int64_t M,
                                                            const int32_t* __restrict__ sample_rows,
                                                            const int32_t* __restrict__ counts, const int32_t* __restrict__ status,
                                                            int m, CloudGrid* __restrict__ grids, int* __restrict__ cells_all,
                                                            float4* __restrict__ sorted_all) {
  __shared__ float red[6][kWaves];
  __shared__ int wsum[kWaves];
  __shared__ __attribute__((aligned(16))) int tile[kThreads];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t lo;
  const int n_rows = cloud_rows(offsets, s, M, (int64_t)0x7fffffff, &lo);
  int ms = 0;
  if (status[s] == GPN_CLOUD_OK) ms = min(min(max(counts[s], 0), m), n_rows);
  CloudGrid* g = grids + s;
  if (ms == 0) {
    if (tid == 0) g->n = 0;
    return;
  }
  const float* src = points + lo * stride;
  const int32_t* sr = sample_rows + (int64_t)s * m;
  auto sample = [&](int j) { return src + (int64_t)min(max(sr[j], 0), n_rows - 1) * stride; };
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int j = tid; j < ms; j += kThreads) {
    const float* p = sample(j);
#pragma unroll
    for (int c = 0; c < 3; ++c) { mn[c] = fminf(mn[c], p[c]); mx[c] = fmaxf(mx[c], p[c]); }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      mn[c] = fminf(mn[c], __shfl_xor(mn[c], off, 64));
      mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], off, 64));
    }
  if (lane == 0)
    for (int c = 0; c < 3; ++c) { red[c][wave] = mn[c]; red[3 + c][wave] = mx[c]; }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    mn[c] = red[c][0]; mx[c] = red[3 + c][0];
    for (int q = 1; q < kWaves; ++q) { mn[c] = fminf(mn[c], red[c][q]); mx[c] = fmaxf(mx[c], red[3 + c][q]); }
  }
  // cubic cells of edge h = longest extent / R, R ~ 2 cbrt(samples); an axis of zero extent has one layer of cells
  const float ext[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
  const float emax = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
  float h = 0.f, inv_h = 0.f;
  int dims[3] = {1, 1, 1};
  if (emax > 0.f && finite_bits(emax)) {
    int R = (int)ceilf(2.f * cbrtf((float)ms));
    R = min(max(R, 1), kMaxRes);
    h = emax / (float)R;
    inv_h = (float)R / emax;
    if (h > 0.f && finite_bits(inv_h)) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dims[c] = min(R, (int)floorf(ext[c] * inv_h) + 1);
    } else {
      h = inv_h = 0.f;
    }
  }
  const int ncells = dims[0] * dims[1] * dims[2];
  if (tid == 0) {
    for (int c = 0; c < 3; ++c) { g->mn[c] = mn[c]; g->mx[c] = mx[c]; g->dims[c] = dims[c]; }
    g->h = h; g->inv_h = inv_h; g->n = ms;
  }
  int* cells = cells_all + (int64_t)s * kMaxCells;
  float4* sorted = sorted_all + (int64_t)s * m;
  auto cell_of = [&](const float* p) {
    return (cell_axis(p[2], mn[2], inv_h, dims[2]) * dims[1] + cell_axis(p[1], mn[1], inv_h, dims[1])) * dims[0] +
           cell_axis(p[0], mn[0], inv_h, dims[0]);
  };
  for (int c = tid; c < ncells; c += kThreads) cells[c] = 0;
  __syncthreads();
  for (int j = tid; j < ms; j += kThreads) atomicAdd(&cells[cell_of(sample(j))], 1);  // (integer counts: order-free)
  __syncthreads();
  block_scan_runs<kWaves>(cells, ncells, wsum);  // counts -> first slots, in place
  // stable scatter, a tile of kThreads samples at a time in sample order: a sample's slot is its cell's cursor plus the number
  // of earlier samples of the tile in the same cell; the cell's last sample of the tile moves the cursor
  for (int t0 = 0; t0 < ms; t0 += kThreads) {
    const int j = t0 + tid;
    const float* p = j < ms ? sample(j) : nullptr;
    const int c = p ? cell_of(p) : -1;
    tile[tid] = c;
    __syncthreads();
    int before = 0, same = 0, cur = 0;
    if (p) {
      const int len4 = (min(kThreads, ms - t0) + 3) / 4;
      const int4* t4 = reinterpret_cast<const int4*>(tile);
      for (int i = 0; i < len4; ++i) {
        const int4 v = t4[i];
        const int b = i * 4;
        const int e0 = v.x == c, e1 = v.y == c, e2 = v.z == c, e3 = v.w == c;
        same += e0 + e1 + e2 + e3;
        before += (e0 & (b < tid)) + (e1 & (b + 1 < tid)) + (e2 & (b + 2 < tid)) + (e3 & (b + 3 < tid));
      }
      cur = cells[c];
      sorted[cur + before] = make_float4(p[0], p[1], p[2], __int_as_float(j));
    }
    __syncthreads();  // every cursor of the tile has been read
    if (p && before == same - 1) cells[c] = cur + same;
    __syncthreads();  // ... and moved, before the next tile reads it (and before `tile` is rewritten)
  }
}

__global__ __launch_bounds__(kQueryThreads) void cn_query_kernel(const float* __restrict__ points, int stride,
                                                                 const int64_t* __restrict__ offsets, int S, int64_t M, int m,
                                                                 const CloudGrid* __restrict__ grids,
                                                                 const int* __restrict__ cells_all,
                                                                 const float4* __restrict__ sorted_all, int32_t* __restrict__ nn,
                                                                 float* __restrict__ d2_out) {
  const int64_t row = (int64_t)blockIdx.x * kQueryThreads + threadIdx.x;
  if (row >= M) return;
  // the cloud that owns the row: the last s with offsets[s] <= row
  int a = 0, b = S;  // offsets[a] <= row < offsets[b] once found
  int s = -1;
  if (offsets[0] <= row && row < offsets[S]) {
    while (b - a > 1) {
      const int mid = (a + b) >> 1;
      if (offsets[mid] <= row) a = mid; else b = mid;
    }
    s = a;
  }
  int bestj = -1;
  float best = INFINITY;
  const float* q = points + row * stride;
  const float qx = q[0], qy = q[1], qz = q[2];
  if (s >= 0 && grids[s].n > 0 && finite_bits(qx) && finite_bits(qy) && finite_bits(qz)) {
    const CloudGrid g = grids[s];
    const int* cells = cells_all + (int64_t)s * kMaxCells;
    const float4* sorted = sorted_all + (int64_t)s * m;
    bestj = 0x7fffffff;
    auto scan = [&](int i0, int i1) {
      for (int i = i0; i < i1; ++i) {
        const float4 p = sorted[i];
        const float d2 = dist2_nofma(qx, qy, qz, p.x, p.y, p.z);
        const int j = __float_as_int(p.w);
        if (d2 < best || (d2 == best && j < bestj)) { best = d2; bestj = j; }
      }
    };
    const int dx = g.dims[0], dy = g.dims[1], dz = g.dims[2];
    const int cx = cell_axis(qx, g.mn[0], g.inv_h, dx), cy = cell_axis(qy, g.mn[1], g.inv_h, dy),
              cz = cell_axis(qz, g.mn[2], g.inv_h, dz);
    auto visit = [&](int x, int y, int z) {
      const int c = (z * dy + y) * dx + x;
      scan(c ? cells[c - 1] : 0, cells[c]);
    };
    // squared distance from the query to the samples' box (every sample lies in it): 0 inside
    const float ox = fmaxf(fmaxf(g.mn[0] - qx, qx - g.mx[0]), 0.f), oy = fmaxf(fmaxf(g.mn[1] - qy, qy - g.mx[1]), 0.f),
                oz = fmaxf(fmaxf(g.mn[2] - qz, qz - g.mx[2]), 0.f);
    const float O2 = ox * ox + oy * oy + oz * oz;
    const int cover = max(max(max(cx, dx - 1 - cx), max(cy, dy - 1 - cy)), max(cz, dz - 1 - cz));
    bool done = false;
    for (int k = 0; k <= kMaxRings && !done; ++k) {
      const int z0 = max(cz - k, 0), z1 = min(cz + k, dz - 1), y0 = max(cy - k, 0), y1 = min(cy + k, dy - 1);
      const int x0 = max(cx - k, 0), x1 = min(cx + k, dx - 1);
      for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
          if (abs(z - cz) == k || abs(y - cy) == k) {
            for (int x = x0; x <= x1; ++x) visit(x, y, z);
          } else {
            if (cx - k >= 0) visit(cx - k, y, z);
            if (cx + k < dx) visit(cx + k, y, z);  // (k >= 1 here: k == 0 takes the branch above)
          }
        }
      if (k >= cover) {
        done = true;  // every cell has been visited
      } else if (k >= 1) {
        // a sample in an unvisited cell is at least k cells away along one axis beyond the box distance of that axis (the
        // 0.001 cell and 2^-18 margins are far above the rounding of the cell assignment and of the fp32 distances):
        // nothing unvisited can equal or beat `best`
        const float gap = ((float)k - 0.001f) * g.h;
        const float lb = (O2 + gap * gap) * (1.f - 1.f / 262144.f);
        done = best < lb;
      }
    }
    if (!done) {  // pathological occupancy or a query far from the box: all samples of the cloud
      best = INFINITY;
      bestj = 0x7fffffff;
      scan(0, g.n);
    }
  }
  nn[row] = bestj;
  if (d2_out) d2_out[row] = best;
}

}  // namespace

extern "C" int gpn_cloud_pack(const float* points, int64_t M, int stride, const int64_t* offsets, int S, int64_t n_bound,
                              float* packed, int32_t* rows, int32_t* counts, int32_t* status, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(S >= 0 && M >= 0 && stride >= 3 && n_bound >= 1 && n_bound < (int64_t)0x7fffffff - kThreads * kRowsPerThread);
  if (S == 0) return GPN_OK;
  GPN_CHECK_ARG((points || M == 0) && offsets && packed && rows && counts && status);
  hipLaunchKernelGGL(cp_pack_kernel, dim3(S), dim3(kThreads), 0, stream, points, stride, offsets, M, n_bound,
                     reinterpret_cast<float4*>(packed), rows, counts, status);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_cloud_finish(const float* points, int64_t M, int stride, int cols, const int64_t* offsets, int S, int64_t n_bound,
                                const int32_t* rows, const int32_t* counts, const int32_t* idx, int m, int32_t* status, float* out,
                                int32_t* sample_rows, double* scale, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(S >= 0 && M >= 0 && cols >= 3 && stride >= cols && m >= 1 && n_bound >= 1 && n_bound < (int64_t)0x7fffffff);
  if (S == 0) return GPN_OK;
  GPN_CHECK_ARG((points || M == 0) && offsets && rows && counts && idx && status && out && sample_rows && scale);
  hipLaunchKernelGGL(cp_finish_kernel, dim3(S), dim3(kThreads), 0, stream, points, stride, cols, offsets, M, n_bound, rows, counts,
                     idx, m, status, out, sample_rows, scale);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" size_t gpn_cloud_nearest_ws_bytes(int S, int m) {
  if (S <= 0 || m <= 0) return 0;
  return gpn::align_up((size_t)S * sizeof(CloudGrid)) + gpn::align_up((size_t)S * kMaxCells * sizeof(int)) +
         gpn::align_up((size_t)S * m * sizeof(float4));
}

extern "C" int gpn_cloud_nearest(const float* points, int64_t M, int stride, const int64_t* offsets, int S,
                                 const int32_t* sample_rows, const int32_t* counts, const int32_t* status, int m, int32_t* nn,
                                 float* d2_out, void* ws, size_t ws_bytes, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(S >= 0 && M >= 0 && stride >= 3 && m >= 1);
  GPN_CHECK_ARG(M < (int64_t)0x7fffffff * kQueryThreads);
  if (S == 0 || M == 0) return GPN_OK;
  GPN_CHECK_ARG(points && offsets && sample_rows && counts && status && nn);
  gpn::WsCarver carve(ws, ws_bytes);
  CloudGrid* grids = carve.take<CloudGrid>((size_t)S);
  int* cells = carve.take<int>((size_t)S * kMaxCells);
  float4* sorted = carve.take<float4>((size_t)S * m);
  GPN_CHECK_WS(carve);
  hipLaunchKernelGGL(cn_build_kernel, dim3(S), dim3(kThreads), 0, stream, points, stride, offsets, M, sample_rows, counts, status, m,
                     grids, cells, sorted);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(cn_query_kernel, dim3((unsigned)gpn::cdiv(M, kQueryThreads)), dim3(kQueryThreads), 0, stream, points, stride,
                     offsets, S, M, m, grids, cells, sorted, nn, d2_out);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
