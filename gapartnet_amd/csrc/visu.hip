// visu.hip — the back end of the test path: kept proposals -> per-point maps, and the 3 x 4 panel of images the reference's
// on_test_epoch_end writes per sampled scene (network/model.py:930-999, misc/visu.py, misc/visu_util.py), for all sampled scenes at
// once:
//   scene_maps     per-point instance / NPCS maps of one batch and the NPCS the pose fit reads (model.py:954-971)
//   points_winner  the geometry half of map2image (visu_util.py:107-139): which point a pixel shows, once per scene for all tiles
//   points_paint   the colour half: every requested tile of every scene, straight into the canvas
//   boxes_draw     draw_bbox (visu_util.py:37-71): all boxes of all scenes, lines by the rule stated in include/gpn.h
// "The last writer wins" of the reference's loops is an integer atomicMax over the writer's position followed by a resolve pass:
// no result depends on timing, and there are no float atomics.
#include <cmath>

#include "gpn_common.h"
#include "wg_scan.h"

namespace {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kMaxExtent = 16384;  // H, W: 5 * extent and 9 * (H + W) stay far inside int32

struct Cam {
  double fx, fy, u0, v0;
};
struct PaintArgs {
  int n;
  gpn_visu_layer_t l[GPN_VISU_MAX_LAYERS];
};
struct TileList {
  int n;
  int row[GPN_VISU_MAX_LAYERS], col[GPN_VISU_MAX_LAYERS];
};

// the largest s in [0, S) with off[s] <= g (for off[0] <= g < off[S]: the CSR segment that holds g, empty segments skipped)
__device__ __forceinline__ int csr_find(const int64_t* __restrict__ off, int S, int64_t g) {
  int lo = 0, hi = S;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// visu_util.py:42 / visu.py:62 then :50-51 / :123-124, float64, left to right, no contraction: p * r + c, around(x * f / z + c0)
__device__ __forceinline__ void project(double x, double y, double z, const double* __restrict__ t, const Cam& cam, double& u,
                                        double& v) {
  const double X = x * t[0] + t[1], Y = y * t[0] + t[2], Z = z * t[0] + t[3];
  u = rint(X * cam.fx / Z + cam.u0);  // half to even, like np.around
  v = rint(Y * cam.fy / Z + cam.v0);
}

__device__ __forceinline__ int floormod(int a, int b) {
  const int r = a % b;
  return r < 0 ? r + b : r;
}

// the C cast of a float to uint8 where it is defined (truncation toward zero); clamped outside [0, 256), NaN -> 0
__device__ __forceinline__ uint8_t to_u8(float f) {
  if (!(f > 0.f)) return 0;
  if (f >= 255.f) return 255;
  return (uint8_t)(int)f;
}

// ---- scene maps ---------------------------------------------------------------------------------------------------------------
// rank[m] = number of true mask entries before m: one workgroup, tiles of kScanThreads entries
__global__ __launch_bounds__(kScanThreads) void visu_rank_kernel(const uint8_t* __restrict__ mask, int64_t M,
                                                                 int32_t* __restrict__ rank) {
  __shared__ int32_t wsum[kScanWaves];
  gpn::block_scan_tiled<kScanWaves>(M, [&](int64_t m) { return mask[m] ? 1 : 0; }, rank, wsum);
}

// row of proposal point m in the batch's point matrix, -1 if an index is out of range
__device__ __forceinline__ int64_t point_row(const int64_t* __restrict__ valid_indices, int64_t V,
                                             const int64_t* __restrict__ sorted_indices, int64_t N, int64_t m) {
  const int64_t si = sorted_indices[m];
  if (si < 0 || si >= V) return -1;
  const int64_t row = valid_indices[si];
  return (row < 0 || row >= N) ? -1 : row;
}

// the reference's loops run over m in order, so the highest m that writes a row is what the row keeps: max over m per row,
// separately for the instance map (every point of proposals 0 .. P-1) and the NPCS map (the points inside the mask)
__global__ __launch_bounds__(kThreads) void visu_owner_kernel(const int64_t* __restrict__ valid_indices, int64_t V,
                                                              const int64_t* __restrict__ sorted_indices,
                                                              const int64_t* __restrict__ offsets, int64_t P,
                                                              const uint8_t* __restrict__ mask, int64_t M, int64_t N,
                                                              int32_t* __restrict__ own_all, int32_t* __restrict__ own_msk) {
  const int64_t lo = P > 0 ? offsets[0] : 0, hi = P > 0 ? offsets[P] : 0;
  for (int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x; m < M; m += (int64_t)gridDim.x * kThreads) {
    const int64_t row = point_row(valid_indices, V, sorted_indices, N, m);
    if (row < 0) continue;
    if (m >= lo && m < hi) atomicMax(&own_all[row], (int)m);
    if (mask[m]) atomicMax(&own_msk[row], (int)m);
  }
}

__global__ __launch_bounds__(kThreads) void visu_maps_kernel(const int32_t* __restrict__ own_all,
                                                             const int32_t* __restrict__ own_msk,
                                                             const int32_t* __restrict__ rank,
                                                             const int64_t* __restrict__ offsets, int64_t P,
                                                             const float* __restrict__ npcs_preds, int64_t Mv, int64_t N,
                                                             int32_t* __restrict__ ins_map, float* __restrict__ npcs_map) {
  for (int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x; n < N; n += (int64_t)gridDim.x * kThreads) {
    const int o = own_all[n];
    ins_map[n] = o < 0 ? 0 : csr_find(offsets, (int)P, o) + 1;
    const int k = own_msk[n];
    float a = 0.f, b = 0.f, c = 0.f;
    if (k >= 0) {
      const int64_t r = rank[k];
      if (r < Mv) { a = npcs_preds[r * 3]; b = npcs_preds[r * 3 + 1]; c = npcs_preds[r * 3 + 2]; }
    }
    npcs_map[n * 3] = a;
    npcs_map[n * 3 + 1] = b;
    npcs_map[n * 3 + 2] = c;
  }
}

// model.py:969-970: the map gathered back at every proposal point, minus 0.5 (a point outside the mask whose row no masked
// point wrote enters the fit as (-0.5, -0.5, -0.5))
__global__ __launch_bounds__(kThreads) void visu_fit_npcs_kernel(const int64_t* __restrict__ valid_indices, int64_t V,
                                                                 const int64_t* __restrict__ sorted_indices, int64_t M, int64_t N,
                                                                 const float* __restrict__ npcs_map, float* __restrict__ fit_npcs) {
  for (int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x; m < M; m += (int64_t)gridDim.x * kThreads) {
    const int64_t row = point_row(valid_indices, V, sorted_indices, N, m);
#pragma unroll
    for (int c = 0; c < 3; ++c) fit_npcs[m * 3 + c] = (row < 0 ? 0.f : npcs_map[row * 3 + c]) - 0.5f;
  }
}

// ---- points -> pixels -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void visu_winner_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ off,
                                                               const double* __restrict__ trans, int S, int64_t n_total, int H,
                                                               int W, Cam cam, int32_t* __restrict__ winner) {
  const int64_t first = off[0], last = off[S];
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < n_total; g += (int64_t)gridDim.x * kThreads) {
    if (g < first || g >= last) continue;
    const int s = csr_find(off, S, g);
    double u, v;
    project((double)xyz[g * 3], (double)xyz[g * 3 + 1], (double)xyz[g * 3 + 2], trans + (int64_t)s * 4, cam, u, v);
    // visu_util.py:130 (-0.0 is not < 0 and passes, as the reference's integer 0 does)
    if (!isfinite(u) || !isfinite(v) || v + 1.0 >= (double)H || v < 0.0 || u + 1.0 >= (double)W || u < 0.0) continue;
    const int iu = (int)u, iv = (int)v, i = (int)(g - off[s]);
    int32_t* w = winner + ((int64_t)s * H + iv) * W + iu;
    atomicMax(w, i);
    atomicMax(w + W, i);
    atomicMax(w + W + 1, i);
    atomicMax(w + 1, i);
  }
}

__global__ __launch_bounds__(kThreads) void visu_paint_kernel(PaintArgs a, const int32_t* __restrict__ winner,
                                                              const int64_t* __restrict__ off,
                                                              const uint8_t* __restrict__ palette, int K, int H, int W, int edge,
                                                              int CH, int CW, uint8_t* __restrict__ canvas) {
  const int pix = blockIdx.x * kThreads + threadIdx.x, s = blockIdx.y;
  if (pix >= H * W) return;
  const int y = pix / W, x = pix - y * W;
  const int i = winner[(int64_t)s * H * W + pix];
  const int64_t g = off[s] + i;
  for (int l = 0; l < a.n; ++l) {
    const gpn_visu_layer_t& L = a.l[l];
    uint8_t c0 = 255, c1 = 255, c2 = 255;
    if (i >= 0 && L.kind != GPN_VISU_BLANK) {
      if (L.kind == GPN_VISU_RGB) {
        const float* src = (const float*)L.src + g * 3;
        c0 = to_u8((src[0] + L.offset) * 255.0f);
        c1 = to_u8((src[1] + L.offset) * 255.0f);
        c2 = to_u8((src[2] + L.offset) * 255.0f);
      } else {
        const int label = ((const int32_t*)L.src)[g];
        if (L.kind == GPN_VISU_LABEL_MOD19P1 && label == -100) {
          c0 = c1 = c2 = 230;
        } else {
          const int k = L.kind == GPN_VISU_LABEL ? floormod(label, K)
                        : L.kind == GPN_VISU_LABEL_MOD20 ? floormod(label, 20) : floormod(label, 19) + 1;
          c0 = palette[k * 3]; c1 = palette[k * 3 + 1]; c2 = palette[k * 3 + 2];
        }
      }
    }
    const int64_t o = (((int64_t)s * CH + edge + (int64_t)L.row * (H + edge) + y) * CW + edge + (int64_t)L.col * (W + edge) + x) * 3;
    canvas[o] = c0;
    canvas[o + 1] = c1;
    canvas[o + 2] = c2;
  }
}

// ---- boxes ----------------------------------------------------------------------------------------------------------------------
// visu_util.py:56-70: the 12 edges, then the three axes
__device__ const int8_t kEdgeA[GPN_VISU_BOX_DRAWS] = {0, 0, 0, 1, 1, 2, 6, 4, 5, 3, 2, 6, 0, 0, 0};
__device__ const int8_t kEdgeB[GPN_VISU_BOX_DRAWS] = {1, 2, 3, 4, 5, 6, 3, 7, 7, 5, 4, 7, 1, 3, 2};

// one thread per (box, draw): the line rule of include/gpn.h; every covered pixel keeps the highest draw number q * 15 + e
__global__ __launch_bounds__(kThreads) void visu_edges_kernel(const double* __restrict__ bbox,
                                                              const int32_t* __restrict__ box_scene, int64_t Q,
                                                              const double* __restrict__ trans, int S, int H, int W, Cam cam,
                                                              int32_t* __restrict__ prio) {
  const int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (id >= Q * GPN_VISU_BOX_DRAWS) return;
  const int64_t q = id / GPN_VISU_BOX_DRAWS;
  const int e = (int)(id - q * GPN_VISU_BOX_DRAWS);
  const int s = box_scene[q];
  if (s < 0 || s >= S) return;
  const double* pa = bbox + (q * 8 + kEdgeA[e]) * 3;
  const double* pb = bbox + (q * 8 + kEdgeB[e]) * 3;
  double ua, va, ub, vb;
  project(pa[0], pa[1], pa[2], trans + (int64_t)s * 4, cam, ua, va);
  project(pb[0], pb[1], pb[2], trans + (int64_t)s * 4, cam, ub, vb);
  const double xl = -4.0 * W, xh = 5.0 * W, yl = -4.0 * H, yh = 5.0 * H;
  if (!(ua >= xl && ua < xh && ub >= xl && ub < xh && va >= yl && va < yh && vb >= yl && vb < yh)) return;  // (NaN fails too)
  int x = (int)ua, y = (int)va;
  const int x1 = (int)ub, y1 = (int)vb;
  const int dx = abs(x1 - x), dy = -abs(y1 - y), sx = x < x1 ? 1 : -1, sy = y < y1 ? 1 : -1;
  int err = dx + dy;
  const int t = e < 12 ? 2 : 3;
  int32_t* img = prio + (int64_t)s * H * W;
  const int cap = 9 * (H + W) + 2;  // the walk takes max(dx, -dy) + 1 <= 9 max(H, W) steps
  for (int it = 0; it < cap; ++it) {
    const int tx = x - t / 2, ty = y - t / 2;
    for (int j = 0; j < t; ++j)
      for (int k = 0; k < t; ++k) {
        const int px = tx + k, py = ty + j;
        if (px >= 0 && px < W && py >= 0 && py < H) atomicMax(&img[(int64_t)py * W + px], (int)id);
      }
    if (x == x1 && y == y1) break;
    const int e2 = 2 * err;
    if (e2 >= dy) { err += dy; x += sx; }
    if (e2 <= dx) { err += dx; y += sy; }
  }
}

__global__ __launch_bounds__(kThreads) void visu_lines_kernel(const int32_t* __restrict__ prio, TileList tiles, int H, int W,
                                                              int edge, int CH, int CW, uint8_t* __restrict__ canvas) {
  const int pix = blockIdx.x * kThreads + threadIdx.x, s = blockIdx.y;
  if (pix >= H * W) return;
  const int p = prio[(int64_t)s * H * W + pix];
  if (p < 0) return;
  const int e = p % GPN_VISU_BOX_DRAWS;
  // colours as they appear in the written file: magenta edges, then 0-1 red, 0-3 blue, 0-2 green
  const uint8_t c0 = (e < 12 || e == 12) ? 255 : 0, c1 = e == 14 ? 255 : 0, c2 = (e < 12 || e == 13) ? 255 : 0;
  const int y = pix / W, x = pix - y * W;
  for (int l = 0; l < tiles.n; ++l) {
    const int64_t o =
        (((int64_t)s * CH + edge + (int64_t)tiles.row[l] * (H + edge) + y) * CW + edge + (int64_t)tiles.col[l] * (W + edge) + x) * 3;
    canvas[o] = c0;
    canvas[o + 1] = c1;
    canvas[o + 2] = c2;
  }
}

unsigned grid_for(int64_t items) {
  int64_t g = gpn::cdiv(items, kThreads);
  if (g < 1) g = 1;
  if (g > 65536) g = 65536;  // (grid-stride loops)
  return (unsigned)g;
}

bool tile_fits(int row, int col, int H, int W, int edge, int CH, int CW) {
  return row >= 0 && col >= 0 && row < 64 && col < 64 && edge + (int64_t)row * (H + edge) + H <= CH &&
         edge + (int64_t)col * (W + edge) + W <= CW;
}

bool image_args_ok(int S, int H, int W) { return S >= 0 && S <= 65535 && H >= 2 && W >= 2 && H <= kMaxExtent && W <= kMaxExtent; }

}  // namespace

extern "C" size_t gpn_scene_maps_ws_bytes(int64_t N, int64_t M) {
  if (N < 0 || M < 0) return 0;
  return gpn::align_up((size_t)2 * N * sizeof(int32_t)) + gpn::align_up((size_t)M * sizeof(int32_t));
}

extern "C" int gpn_scene_maps(const int64_t* valid_indices, int64_t V, const int64_t* sorted_indices,
                              const int64_t* proposal_offsets, int64_t P, const uint8_t* npcs_valid_mask, int64_t M,
                              const float* npcs_preds, int64_t Mv, int64_t N, int32_t* ins_map, float* npcs_map, float* fit_npcs,
                              void* ws, size_t ws_bytes, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t lim = 0x7fffffff;
  GPN_CHECK_ARG(V >= 0 && P >= 0 && M >= 0 && Mv >= 0 && N >= 0 && N < lim && M < lim && P < lim && Mv <= M);
  GPN_CHECK_ARG(N == 0 || (ins_map && npcs_map));
  GPN_CHECK_ARG(M == 0 || (sorted_indices && npcs_valid_mask && fit_npcs && N > 0));
  GPN_CHECK_ARG(V == 0 || valid_indices);
  GPN_CHECK_ARG(P == 0 || proposal_offsets);
  GPN_CHECK_ARG(Mv == 0 || npcs_preds);
  if (N == 0) return GPN_OK;
  gpn::WsCarver carve(ws, ws_bytes);
  int32_t* own = carve.take<int32_t>((size_t)2 * N);
  int32_t* rank = carve.take<int32_t>((size_t)M);
  GPN_CHECK_WS(carve);
  GPN_CHECK_HIP(hipMemsetAsync(own, 0xff, (size_t)2 * N * sizeof(int32_t), stream));  // -1: no writer
  if (M > 0) {
    hipLaunchKernelGGL(visu_rank_kernel, dim3(1), dim3(kScanThreads), 0, stream, npcs_valid_mask, M, rank);
    hipLaunchKernelGGL(visu_owner_kernel, dim3(grid_for(M)), dim3(kThreads), 0, stream, valid_indices, V, sorted_indices,
                       proposal_offsets, P, npcs_valid_mask, M, N, own, own + N);
  }
  hipLaunchKernelGGL(visu_maps_kernel, dim3(grid_for(N)), dim3(kThreads), 0, stream, own, own + N, rank, proposal_offsets, P,
                     npcs_preds, Mv, N, ins_map, npcs_map);
  if (M > 0)
    hipLaunchKernelGGL(visu_fit_npcs_kernel, dim3(grid_for(M)), dim3(kThreads), 0, stream, valid_indices, V, sorted_indices, M, N,
                       npcs_map, fit_npcs);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_points_winner(const float* xyz, const int64_t* scene_offsets, int64_t n_total, const double* trans, int S, int H,
                                 int W, double fx, double fy, double u0, double v0, int32_t* winner, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(image_args_ok(S, H, W) && n_total >= 0 && n_total < (int64_t)0x7fffffff);
  if (S == 0) return GPN_OK;
  GPN_CHECK_ARG(scene_offsets && trans && winner && (n_total == 0 || xyz));
  GPN_CHECK_HIP(hipMemsetAsync(winner, 0xff, (size_t)S * H * W * sizeof(int32_t), stream));  // -1: no point
  if (n_total == 0) return GPN_OK;
  hipLaunchKernelGGL(visu_winner_kernel, dim3(grid_for(n_total)), dim3(kThreads), 0, stream, xyz, scene_offsets, trans, S, n_total,
                     H, W, Cam{fx, fy, u0, v0}, winner);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_points_paint(const int32_t* winner, const int64_t* scene_offsets, int S, int H, int W,
                                const gpn_visu_layer_t* layers_host, int n_layers, const uint8_t* palette, int K, int edge, int CH,
                                int CW, uint8_t* canvas, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(image_args_ok(S, H, W) && n_layers >= 0 && n_layers <= GPN_VISU_MAX_LAYERS && edge >= 0 && K >= 0);
  GPN_CHECK_ARG(n_layers == 0 || layers_host);
  PaintArgs a;
  a.n = n_layers;
  for (int l = 0; l < n_layers; ++l) {
    const gpn_visu_layer_t& L = layers_host[l];
    GPN_CHECK_ARG(L.kind >= GPN_VISU_RGB && L.kind <= GPN_VISU_BLANK);
    GPN_CHECK_ARG(L.kind == GPN_VISU_BLANK || L.src != nullptr || S == 0);
    GPN_CHECK_ARG(tile_fits(L.row, L.col, H, W, edge, CH, CW));
    if (L.kind == GPN_VISU_LABEL) GPN_CHECK_ARG(palette && K >= 1);
    if (L.kind == GPN_VISU_LABEL_MOD20 || L.kind == GPN_VISU_LABEL_MOD19P1) GPN_CHECK_ARG(palette && K >= 20);
    a.l[l] = L;
  }
  if (S == 0 || n_layers == 0) return GPN_OK;
  GPN_CHECK_ARG(winner && scene_offsets && canvas);
  hipLaunchKernelGGL(visu_paint_kernel, dim3((unsigned)gpn::cdiv((int64_t)H * W, kThreads), (unsigned)S), dim3(kThreads), 0, stream,
                     a, winner, scene_offsets, palette, K, H, W, edge, CH, CW, canvas);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" size_t gpn_boxes_draw_ws_bytes(int S, int H, int W) {
  if (S <= 0 || H <= 0 || W <= 0) return 0;
  return gpn::align_up((size_t)S * H * W * sizeof(int32_t));
}

extern "C" int gpn_boxes_draw(const double* bbox, const int32_t* box_scene, int64_t Q, const double* trans, int S, int H, int W,
                              double fx, double fy, double u0, double v0, const int32_t* tiles_host, int n_tiles, int edge, int CH,
                              int CW, uint8_t* canvas, void* ws, size_t ws_bytes, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(image_args_ok(S, H, W) && Q >= 0 && Q * GPN_VISU_BOX_DRAWS < (int64_t)0x7fffffff);
  GPN_CHECK_ARG(n_tiles >= 0 && n_tiles <= GPN_VISU_MAX_LAYERS && edge >= 0 && (n_tiles == 0 || tiles_host));
  TileList tiles;
  tiles.n = n_tiles;
  for (int l = 0; l < n_tiles; ++l) {
    tiles.row[l] = tiles_host[2 * l];
    tiles.col[l] = tiles_host[2 * l + 1];
    GPN_CHECK_ARG(tile_fits(tiles.row[l], tiles.col[l], H, W, edge, CH, CW));
  }
  if (S == 0 || Q == 0 || n_tiles == 0) return GPN_OK;
  GPN_CHECK_ARG(bbox && box_scene && trans && canvas);
  gpn::WsCarver carve(ws, ws_bytes);
  int32_t* prio = carve.take<int32_t>((size_t)S * H * W);
  GPN_CHECK_WS(carve);
  GPN_CHECK_HIP(hipMemsetAsync(prio, 0xff, (size_t)S * H * W * sizeof(int32_t), stream));  // -1: no line
  hipLaunchKernelGGL(visu_edges_kernel, dim3((unsigned)gpn::cdiv(Q * GPN_VISU_BOX_DRAWS, kThreads)), dim3(kThreads), 0, stream, bbox,
                     box_scene, Q, trans, S, H, W, Cam{fx, fy, u0, v0}, prio);
  hipLaunchKernelGGL(visu_lines_kernel, dim3((unsigned)gpn::cdiv((int64_t)H * W, kThreads), (unsigned)S), dim3(kThreads), 0, stream,
                     prio, tiles, H, W, edge, CH, CW, canvas);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
