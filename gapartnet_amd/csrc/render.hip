// render.hip — section RD of include/gpn.h: articulated triangle meshes -> the training views of the reference's
// dataset/render_tools/render.py (depth, link labels, NPCS map, flat-shaded RGB) for a batch of V views of one size H x W:
//   setup     one thread per (view, triangle): float64 camera transform and projection, snap to 1/256 px, drop rules, records
//   raster    one 256-lane workgroup per 16 x 16 tile per view, one pixel per lane: box scan in chunks of 256, ballot compaction
//             into LDS, int64 edge functions with the top-left rule, float64 1/z interpolation; every pixel stored once
//   annotate  link areas (LDS histogram, integer atomics), instance ids in annotation order, per-pixel sem / ins / NPCS / RGB
//   shade     section RS, opt-in: one 256-lane workgroup per 16 x 16 tile per view, one pixel per lane; the winner's corners are
//             projected again by the function setup uses, perspective-correct uv, bilinear wrapping texel fetch, the view's light
//             rows from LDS; overwrites the RGB of annotate, every byte once, no atomics, no workspace
// No float atomics and no binning workspace: the images do not depend on launch order.  -ffp-contract=off: every float64
// expression below is evaluated exactly as written.
#include <cmath>

#include "gpn_common.h"

namespace {

constexpr int kTile = 16;
constexpr int kLanes = kTile * kTile;  // 256: the chunk of the triangle scan as well
constexpr int kWavesRD = kLanes / 64;
constexpr int kMaxLinks = 1024;        // annotate: LDS tables per view
constexpr int kCam = 20;               // doubles per view: fx fy cx cy | R[9] | t[3] | light in the camera frame [3] | pad
constexpr int kFrame = 13;             // doubles per link: T[3] | scaler | R[9]
constexpr double kNear = 0.1;
constexpr int kGuard = 16384 * 256;    // snapped coordinates stay inside +-16384 px

struct __align__(16) TriRec {  // 64 bytes
  int32_t x[3], y[3];  // snapped to 1/256 px, oriented to positive doubled area
  double iz[3];        // 1 / Z of the three vertices (same order)
  double shade;        // 0.5 + 0.5 |n . l|
  int16_t box[4];      // pixel box clipped to the image: x0, y0, x1, y1 (inclusive)
};
static_assert(sizeof(TriRec) == 64, "padded record");

struct __align__(8) TriBox {
  int16_t x0, y0, x1, y1;  // x0 > x1: nothing to draw
};

__device__ __forceinline__ int64_t edge_fn(int ax, int ay, int bx, int by, int px, int py) {
  return (int64_t)(bx - ax) * (int64_t)(py - ay) - (int64_t)(by - ay) * (int64_t)(px - ax);
}
// an edge through the sample counts when it is a left edge (going up) or a top edge (level, going right): one of d and -d
__device__ __forceinline__ bool edge_owns(int ax, int ay, int bx, int by) {
  const int dx = bx - ax, dy = by - ay;
  return dy < 0 || (dy == 0 && dx > 0);
}
__device__ __forceinline__ int floor_div256(int a) { return a >> 8; }
__device__ __forceinline__ int ceil_div256(int a) { return (a + 255) >> 8; }

struct AssetSpan {
  int first, count, visuals, links;
};
__device__ __forceinline__ AssetSpan asset_span(const int32_t* __restrict__ assets, int A, const int32_t* __restrict__ view_asset,
                                                int v, int Nt) {
  AssetSpan s{0, 0, 0, 0};
  const int a = view_asset[v];
  if (a < 0 || a >= A) return s;
  s.first = assets[a * 4];
  s.count = assets[a * 4 + 1];
  s.visuals = assets[a * 4 + 2];
  s.links = assets[a * 4 + 3];
  if (s.first < 0 || s.count < 0 || s.first > Nt || s.count > Nt - s.first) s.count = 0;
  return s;
}

// camera-space corners P (parsed vertex order) and their screen positions snapped to 1/256 px, shared by setup and shade so that
// both see the same bits.  -> -1, or the drop rule that applies first (GPN_RENDER_DROP_INDEX / _NEAR / _GUARD)
__device__ __forceinline__ int project_triangle(const float* __restrict__ verts, int Nv, const int32_t* __restrict__ tris,
                                                const int32_t* __restrict__ tri_visual, int t, int visuals, int M,
                                                const double* __restrict__ c, const double* __restrict__ view_mat,
                                                double (&P)[3][3], int (&X)[3], int (&Y)[3]) {
  const int vis = tri_visual[t];
  const int i0 = tris[t * 3], i1 = tris[t * 3 + 1], i2 = tris[t * 3 + 2];
  if (vis < 0 || vis >= M || vis >= visuals || i0 < 0 || i0 >= Nv || i1 < 0 || i1 >= Nv || i2 < 0 || i2 >= Nv)
    return GPN_RENDER_DROP_INDEX;
  const double fx = c[0], fy = c[1], cx = c[2], cy = c[3];
  const double* m = view_mat + (int64_t)vis * 12;
  const int idx[3] = {i0, i1, i2};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double x = (double)verts[idx[j] * 3], y = (double)verts[idx[j] * 3 + 1], z = (double)verts[idx[j] * 3 + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) P[j][r] = ((m[r * 4] * x + m[r * 4 + 1] * y) + m[r * 4 + 2] * z) + m[r * 4 + 3];
  }
  if (!(P[0][2] >= kNear && P[1][2] >= kNear && P[2][2] >= kNear)) return GPN_RENDER_DROP_NEAR;  // (a NaN depth is dropped here too)
  bool guard = false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double u = (fx * P[j][0]) / P[j][2] + cx, w = (fy * P[j][1]) / P[j][2] + cy;
    const double su = rint(u * 256.0), sv = rint(w * 256.0);
    guard |= !(fabs(su) <= (double)kGuard && fabs(sv) <= (double)kGuard);
    X[j] = (int)su;
    Y[j] = (int)sv;
  }
  return guard ? GPN_RENDER_DROP_GUARD : -1;
}

// ---- setup -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rd_setup_kernel(const float* __restrict__ verts, int Nv, const int32_t* __restrict__ tris,
                                                       const int32_t* __restrict__ tri_visual, int Nt,
                                                       const int32_t* __restrict__ assets, int A,
                                                       const int32_t* __restrict__ view_asset, const double* __restrict__ cam,
                                                       const double* __restrict__ vis_mat, int M, int H, int W, int Nt_max,
                                                       TriRec* __restrict__ recs, TriBox* __restrict__ boxes,
                                                       int32_t* __restrict__ counters) {
  const int v = blockIdx.y;
  const int k = blockIdx.x * 256 + threadIdx.x;  // triangle inside the view's asset
  if (k >= Nt_max) return;
  const AssetSpan sp = asset_span(assets, A, view_asset, v, Nt);
  TriBox* bo = boxes + (int64_t)v * Nt_max + k;
  const TriBox none{1, 1, 0, 0};
  if (k >= sp.count) {
    *bo = none;
    return;
  }
  const int t = sp.first + k;
  int32_t* cnt = counters + v * GPN_RENDER_COUNTERS;
  const double* c = cam + (int64_t)v * kCam;
  double P[3][3];
  int X[3], Y[3];
  const int drop = project_triangle(verts, Nv, tris, tri_visual, t, sp.visuals, M, c, vis_mat + (int64_t)v * M * 12, P, X, Y);
  if (drop >= 0) {
    atomicAdd(cnt + drop, 1);
    *bo = none;
    return;
  }
  TriRec r;
  int o[3] = {0, 1, 2};
  const int64_t area2 = edge_fn(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
  if (area2 == 0) {
    atomicAdd(cnt + GPN_RENDER_DROP_ZERO_AREA, 1);
    *bo = none;
    return;
  }
  if (area2 < 0) { o[1] = 2; o[2] = 1; }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    r.x[j] = X[o[j]];
    r.y[j] = Y[o[j]];
    r.iz[j] = 1.0 / P[o[j]][2];
  }
  // flat normal from the camera-space cross product (parsed vertex order), shade 0.5 + 0.5 |n . l|
  const double ax = P[1][0] - P[0][0], ay = P[1][1] - P[0][1], az = P[1][2] - P[0][2];
  const double bx = P[2][0] - P[0][0], by = P[2][1] - P[0][1], bz = P[2][2] - P[0][2];
  const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const double nn = sqrt((nx * nx + ny * ny) + nz * nz);
  const double d = (nx * c[16] + ny * c[17]) + nz * c[18];
  r.shade = nn > 0.0 ? 0.5 + 0.5 * (fabs(d) / nn) : 0.5;
  const int mnx = min(X[0], min(X[1], X[2])), mxx = max(X[0], max(X[1], X[2]));
  const int mny = min(Y[0], min(Y[1], Y[2])), mxy = max(Y[0], max(Y[1], Y[2]));
  const int x0 = max(ceil_div256(mnx), 0), x1 = min(floor_div256(mxx), W - 1);
  const int y0 = max(ceil_div256(mny), 0), y1 = min(floor_div256(mxy), H - 1);
  if (x0 > x1 || y0 > y1) {
    atomicAdd(cnt + GPN_RENDER_DROP_OFFSCREEN, 1);
    *bo = none;
    return;
  }
  r.box[0] = (int16_t)x0; r.box[1] = (int16_t)y0; r.box[2] = (int16_t)x1; r.box[3] = (int16_t)y1;
  recs[(int64_t)v * Nt_max + k] = r;
  *bo = TriBox{(int16_t)x0, (int16_t)y0, (int16_t)x1, (int16_t)y1};
}

// ---- raster ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLanes) void rd_raster_kernel(const int32_t* __restrict__ assets, int A,
                                                           const int32_t* __restrict__ view_asset, int Nt, int H, int W,
                                                           int Nt_max, const TriRec* __restrict__ recs,
                                                           const TriBox* __restrict__ boxes, float* __restrict__ depth,
                                                           int32_t* __restrict__ tri_out) {
  __shared__ TriRec s_rec[kLanes];
  __shared__ int s_idx[kLanes];
  __shared__ int s_wcnt[kWavesRD];
  const int v = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
  const int tx1 = tx0 + kTile - 1, ty1 = ty0 + kTile - 1;
  const int px = tx0 + (tid & (kTile - 1)), py = ty0 + (tid >> 4);
  const int sx = px * 256, sy = py * 256;
  const AssetSpan sp = asset_span(assets, A, view_asset, v, Nt);
  const int n = min(sp.count, Nt_max);
  const TriRec* vr = recs + (int64_t)v * Nt_max;
  const TriBox* vb = boxes + (int64_t)v * Nt_max;
  double best = 0.0;  // 1 / z of the winner (every drawn triangle has 1 / z > 0)
  int besti = -1;
  for (int k0 = 0; k0 < n; k0 += kLanes) {
    const int k = k0 + tid;
    bool hit = false;
    if (k < n) {
      const TriBox b = vb[k];
      hit = b.x0 <= b.x1 && b.x0 <= tx1 && b.x1 >= tx0 && b.y0 <= ty1 && b.y1 >= ty0;
    }
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) s_wcnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWavesRD; ++w) {
      const int c = s_wcnt[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (hit) {
      const int pos = before + __popcll(mask & ((1ull << lane) - 1ull));
      s_rec[pos] = vr[k];
      s_idx[pos] = k;
    }
    __syncthreads();
    for (int j = 0; j < total; ++j) {
      const TriRec& r = s_rec[j];
      if (px < r.box[0] || px > r.box[2] || py < r.box[1] || py > r.box[3]) continue;
      const int64_t e0 = edge_fn(r.x[1], r.y[1], r.x[2], r.y[2], sx, sy);
      const int64_t e1 = edge_fn(r.x[2], r.y[2], r.x[0], r.y[0], sx, sy);
      const int64_t e2 = edge_fn(r.x[0], r.y[0], r.x[1], r.y[1], sx, sy);
      if (e0 < 0 || e1 < 0 || e2 < 0) continue;
      if (e0 == 0 && !edge_owns(r.x[1], r.y[1], r.x[2], r.y[2])) continue;
      if (e1 == 0 && !edge_owns(r.x[2], r.y[2], r.x[0], r.y[0])) continue;
      if (e2 == 0 && !edge_owns(r.x[0], r.y[0], r.x[1], r.y[1])) continue;
      const double a2 = (double)((e0 + e1) + e2);  // the doubled area (exact: the three edge functions sum to it)
      const double l0 = (double)e0 / a2, l1 = (double)e1 / a2, l2 = (double)e2 / a2;
      const double invz = (l0 * r.iz[0] + l1 * r.iz[1]) + l2 * r.iz[2];
      if (invz > best) {  // the list is in ascending triangle order (ordered compaction, ascending chunks): a tie keeps the lower one
        best = invz;
        besti = s_idx[j];
      }
    }
    __syncthreads();  // the lists are rewritten by the next chunk
  }
  if (px < W && py < H) {
    const int64_t o = ((int64_t)v * H + py) * W + px;
    depth[o] = besti >= 0 ? (float)(1.0 / best) : 0.f;
    tri_out[o] = besti >= 0 ? sp.first + besti : -1;
  }
}

// ---- annotate --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pixel_link(const int32_t* __restrict__ tri_link, int t, int Nt, int links) {
  if (t < 0 || t >= Nt) return -1;
  const int l = tri_link[t];
  return l >= 0 && l < links ? l : -1;
}

__global__ __launch_bounds__(256) void rd_area_kernel(const int32_t* __restrict__ tri, const int32_t* __restrict__ tri_link,
                                                      int Nt, const int32_t* __restrict__ assets, int A,
                                                      const int32_t* __restrict__ view_asset, int64_t HW, int L,
                                                      int32_t* __restrict__ link_area) {
  __shared__ int hist[kMaxLinks];
  const int v = blockIdx.y;
  const AssetSpan sp = asset_span(assets, A, view_asset, v, Nt);
  const int links = min(sp.links, L);
  for (int q = threadIdx.x; q < L; q += 256) hist[q] = 0;
  __syncthreads();
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    const int l = pixel_link(tri_link, tri[(int64_t)v * HW + p], Nt, links);
    if (l >= 0) atomicAdd(&hist[l], 1);
  }
  __syncthreads();
  for (int q = threadIdx.x; q < L; q += 256)
    if (hist[q]) atomicAdd(link_area + (int64_t)v * L + q, hist[q]);
}

// instance ids in annotation order for the target links with area > 0 (render_sem_ins_seg_map's part_ins_cnt loop)
__global__ __launch_bounds__(256) void rd_inst_kernel(const int32_t* __restrict__ link_cat, const int32_t* __restrict__ link_rank,
                                                      const int32_t* __restrict__ link_area, int L,
                                                      int32_t* __restrict__ link_inst) {
  __shared__ int by_rank[kMaxLinks];
  const int v = blockIdx.x;
  for (int q = threadIdx.x; q < L; q += 256) {
    by_rank[q] = -1;
    link_inst[(int64_t)v * L + q] = -1;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < L; q += 256) {
    const int r = link_rank[(int64_t)v * L + q];
    if (r >= 0 && r < L && link_cat[(int64_t)v * L + q] >= 0) by_rank[r] = q;  // (ranks are distinct)
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int cnt = 0;
    for (int r = 0; r < L; ++r) {
      const int l = by_rank[r];
      if (l >= 0 && link_area[(int64_t)v * L + l] > 0) link_inst[(int64_t)v * L + l] = cnt++;
    }
  }
}

__global__ __launch_bounds__(256) void rd_pixel_kernel(const float* __restrict__ depth, const int32_t* __restrict__ tri,
                                                       const int32_t* __restrict__ tri_link, const float* __restrict__ tri_color,
                                                       int Nt, const int32_t* __restrict__ assets, int A,
                                                       const int32_t* __restrict__ view_asset, const double* __restrict__ cam,
                                                       const int32_t* __restrict__ link_cat, const int32_t* __restrict__ link_inst,
                                                       const double* __restrict__ link_frame, int L, int H, int W, int Nt_max,
                                                       const TriRec* __restrict__ recs, int bg_r, int bg_g, int bg_b,
                                                       int32_t* __restrict__ sem, int32_t* __restrict__ ins,
                                                       float* __restrict__ npcs, uint8_t* __restrict__ rgb) {
  const int v = blockIdx.y;
  const int64_t HW = (int64_t)H * W;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int64_t o = (int64_t)v * HW + p;
  const AssetSpan sp = asset_span(assets, A, view_asset, v, Nt);
  const int t = tri[o];
  const float df = depth[o];
  const int l = pixel_link(tri_link, t, Nt, min(sp.links, L));
  int s = -1, i = -1;
  if (l >= 0 && link_cat[(int64_t)v * L + l] >= 0) {
    const int id = link_inst[(int64_t)v * L + l];
    if (id >= 0) {
      s = link_cat[(int64_t)v * L + l];
      i = id;
    }
  }
  if (fabsf(df) < 1e-6f) s = i = -2;
  sem[o] = s;
  ins[o] = i;
  float q[3] = {0.f, 0.f, 0.f};
  if (i >= 0) {
    const double* c = cam + (int64_t)v * kCam;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const double z = (double)df;
    const double pc[3] = {(((double)x - c[2]) * z) / c[0], (((double)y - c[3]) * z) / c[1], z};
    const double* R = c + 4;
    const double* f = link_frame + ((int64_t)v * L + l) * kFrame;
    double g[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double w = ((pc[0] * R[r * 3] + pc[1] * R[r * 3 + 1]) + pc[2] * R[r * 3 + 2]) + c[13 + r];
      g[r] = (w - f[r]) / f[3];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = (float)((g[0] * f[4 + r * 3] + g[1] * f[4 + r * 3 + 1]) + g[2] * f[4 + r * 3 + 2]);
  }
  npcs[o * 3] = q[0]; npcs[o * 3 + 1] = q[1]; npcs[o * 3 + 2] = q[2];
  int col[3] = {bg_r, bg_g, bg_b};
  if (t >= sp.first && t < sp.first + min(sp.count, Nt_max)) {
    const double shade = recs[(int64_t)v * Nt_max + (t - sp.first)].shade;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double val = rint(((double)tri_color[(int64_t)t * 3 + r] * shade) * 255.0);
      col[r] = val >= 255.0 ? 255 : (val > 0.0 ? (int)val : 0);
    }
  }
  rgb[o * 3] = (uint8_t)col[0]; rgb[o * 3 + 1] = (uint8_t)col[1]; rgb[o * 3 + 2] = (uint8_t)col[2];
}

// ---- shade (section RS) ------------------------------------------------------------------------------------------------------
constexpr int kMaxLights = 16;
constexpr int kLight = 8;  // doubles per light: kind | x y z | r g b | pad

__device__ __forceinline__ int wrap_index(int i, int n) {  // i mod n for i in [-1, n]
  return i < 0 ? i + n : (i >= n ? i - n : i);
}

__global__ __launch_bounds__(kLanes) void rs_shade_kernel(
    const float* __restrict__ verts, int Nv, const int32_t* __restrict__ tris, const int32_t* __restrict__ tri_visual,
    const float* __restrict__ tri_color, int Nt, const int32_t* __restrict__ assets, int A, const int32_t* __restrict__ view_asset,
    const double* __restrict__ cam, const double* __restrict__ vis_mat, int M, const float* __restrict__ tri_uv,
    const int32_t* __restrict__ tri_tex, const int32_t* __restrict__ tex_table, int T, const uint32_t* __restrict__ tex_data,
    int64_t texels, const double* __restrict__ lights, int NL, const float* __restrict__ depth, const int32_t* __restrict__ tri,
    int H, int W, int Nt_max, int bg_r, int bg_g, int bg_b, uint8_t* __restrict__ rgb) {
  __shared__ double s_light[kMaxLights * kLight];
  const int v = blockIdx.z;
  const int tid = threadIdx.x;
  if (tid < NL * kLight) s_light[tid] = lights[(int64_t)v * NL * kLight + tid];  // NL <= 16: at most 128 lanes load
  __syncthreads();
  const int px = blockIdx.x * kTile + (tid & (kTile - 1)), py = blockIdx.y * kTile + (tid >> 4);
  if (px >= W || py >= H) return;
  const int64_t o = ((int64_t)v * H + py) * W + px;
  const AssetSpan sp = asset_span(assets, A, view_asset, v, Nt);
  const int t = tri[o];
  int col[3] = {bg_r, bg_g, bg_b};
  double P[3][3];
  int X[3], Y[3];
  const double* c = cam + (int64_t)v * kCam;
  bool drawn = t >= sp.first && t < sp.first + min(sp.count, Nt_max);
  if (drawn) drawn = project_triangle(verts, Nv, tris, tri_visual, t, sp.visuals, M, c, vis_mat + (int64_t)v * M * 12, P, X, Y) < 0;
  int64_t area2 = 0;
  if (drawn) {
    area2 = edge_fn(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
    drawn = area2 != 0;  // (the raster never hands out such a triangle)
  }
  if (drawn) {
    // barycentrics over the oriented corners (0, 1, 2) or (0, 2, 1), perspective-corrected, back in parsed order
    const bool flip = area2 < 0;
    const int x1 = flip ? X[2] : X[1], y1 = flip ? Y[2] : Y[1], x2 = flip ? X[1] : X[2], y2 = flip ? Y[1] : Y[2];
    const double z1 = flip ? P[2][2] : P[1][2], z2 = flip ? P[1][2] : P[2][2];
    const int sx = px * 256, sy = py * 256;
    const int64_t e0 = edge_fn(x1, y1, x2, y2, sx, sy), e1 = edge_fn(x2, y2, X[0], Y[0], sx, sy), e2 = edge_fn(X[0], Y[0], x1, y1, sx, sy);
    const double a2 = (double)((e0 + e1) + e2);
    const double w0 = ((double)e0 / a2) * (1.0 / P[0][2]), w1 = ((double)e1 / a2) * (1.0 / z1), w2 = ((double)e2 / a2) * (1.0 / z2);
    const double ws = (w0 + w1) + w2;
    const double b0 = w0 / ws, bo1 = w1 / ws, bo2 = w2 / ws;
    const double b1 = flip ? bo2 : bo1, b2 = flip ? bo1 : bo2;
    // albedo in 0 ... 255
    double alb[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) alb[r] = (double)tri_color[(int64_t)t * 3 + r] * 255.0;
    int tx = T > 0 ? tri_tex[t] : -1;
    int tw = 0, th = 0;
    int64_t first = 0;
    if (tx >= 0 && tx < T) {
      first = tex_table[tx * 4];
      tw = tex_table[tx * 4 + 1];
      th = tex_table[tx * 4 + 2];
      if (first < 0 || tw < 1 || th < 1 || (int64_t)tw * th > texels - first) tx = -1;  // (refused on the host as well)
    } else {
      tx = -1;
    }
    if (tx >= 0) {
      const float* q = tri_uv + (int64_t)t * 6;
      const float u0 = q[0], v0 = q[1], u1 = q[2], v1 = q[3], u2 = q[4], v2 = q[5];
      if (isfinite(u0) && isfinite(v0) && isfinite(u1) && isfinite(v1) && isfinite(u2) && isfinite(v2)) {
        const double tu = (b0 * (double)u0 + b1 * (double)u1) + b2 * (double)u2;
        const double tv = (b0 * (double)v0 + b1 * (double)v1) + b2 * (double)v2;
        const double fv = 1.0 - tv;
        const double uu = tu - floor(tu), vv = fv - floor(fv);
        if (uu >= 0.0 && uu <= 1.0 && vv >= 0.0 && vv <= 1.0) {  // (false only for a NaN: b is finite for a drawn pixel)
          const double Xc = uu * (double)tw - 0.5, Yc = vv * (double)th - 0.5;
          const double fi = floor(Xc), fk = floor(Yc);
          const double fx = Xc - fi, fy = Yc - fk;
          const int i0 = wrap_index((int)fi, tw), i1 = wrap_index((int)fi + 1, tw);
          const int k0 = wrap_index((int)fk, th), k1 = wrap_index((int)fk + 1, th);
          const uint32_t a00 = tex_data[first + (int64_t)k0 * tw + i0], a01 = tex_data[first + (int64_t)k0 * tw + i1];
          const uint32_t a10 = tex_data[first + (int64_t)k1 * tw + i0], a11 = tex_data[first + (int64_t)k1 * tw + i1];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const double c00 = (double)((a00 >> (8 * r)) & 255u), c01 = (double)((a01 >> (8 * r)) & 255u);
            const double c10 = (double)((a10 >> (8 * r)) & 255u), c11 = (double)((a11 >> (8 * r)) & 255u);
            alb[r] = (c00 * (1.0 - fx) + c01 * fx) * (1.0 - fy) + (c10 * (1.0 - fx) + c11 * fx) * fy;
          }
        }
      }
    }
    // flat two-sided normal, towards the camera
    const double ax = P[1][0] - P[0][0], ay = P[1][1] - P[0][1], az = P[1][2] - P[0][2];
    const double bx = P[2][0] - P[0][0], by = P[2][1] - P[0][1], bz = P[2][2] - P[0][2];
    double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const double nn = sqrt((nx * nx + ny * ny) + nz * nz);
    const bool lit = nn > 0.0;
    if (lit) {
      nx = nx / nn; ny = ny / nn; nz = nz / nn;
      if ((nx * P[0][0] + ny * P[0][1]) + nz * P[0][2] > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    }
    const double z = (double)depth[o];
    const double p0 = (((double)px - c[2]) * z) / c[0], p1 = (((double)py - c[3]) * z) / c[1];
    double I[3] = {0.0, 0.0, 0.0};
    for (int l = 0; l < NL; ++l) {
      const double* s = s_light + l * kLight;
      const double kind = s[0];
      if (kind == 0.0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) I[r] = I[r] + s[4 + r];
      } else if (kind == 1.0 && lit) {
        const double nd = (nx * s[1] + ny * s[2]) + nz * s[3];
        const double m = nd > 0.0 ? nd : 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) I[r] = I[r] + s[4 + r] * m;
      } else if (kind == 2.0 && lit) {
        const double dx = s[1] - p0, dy = s[2] - p1, dz = s[3] - z;
        const double r2 = (dx * dx + dy * dy) + dz * dz;
        const double rr = sqrt(r2);
        if (rr > 0.0) {
          const double nd = ((nx * dx + ny * dy) + nz * dz) / rr;
          const double m = nd > 0.0 ? nd : 0.0;
#pragma unroll
          for (int r = 0; r < 3; ++r) I[r] = I[r] + (s[4 + r] * m) / r2;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double val = rint(alb[r] * I[r]);
      col[r] = val >= 255.0 ? 255 : (val > 0.0 ? (int)val : 0);
    }
  }
  rgb[o * 3] = (uint8_t)col[0]; rgb[o * 3 + 1] = (uint8_t)col[1]; rgb[o * 3 + 2] = (uint8_t)col[2];
}

int check_shape(const char* who, int V, int H, int W, int Nt_max) {
  if (!(V >= 0 && V <= 65535 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && Nt_max >= 0 &&
        (int64_t)V * H * W < (int64_t)0x7fffffff && (int64_t)V * (Nt_max > 0 ? Nt_max : 1) < (int64_t)0x7fffffff)) {
    gpn::set_error("%s: bad argument: need 0 <= V <= 65535, 1 <= H, W <= 16384, Nt_max >= 0, V*H*W and V*Nt_max below 2^31", who);
    return GPN_ERR_ARG;
  }
  return GPN_OK;
}

struct RenderWs {
  TriRec* recs;
  TriBox* boxes;
};

}  // namespace

extern "C" size_t gpn_render_ws_bytes(int V, int Nt_max) {
  if (V <= 0 || Nt_max <= 0) return 0;
  return gpn::align_up((size_t)V * Nt_max * sizeof(TriRec)) + gpn::align_up((size_t)V * Nt_max * sizeof(TriBox));
}

#define RD_CARVE_WS()                                              \
  gpn::WsCarver carve(ws, ws_bytes);                               \
  RenderWs rw;                                                     \
  rw.recs = carve.take<TriRec>((size_t)V * (size_t)Nt_max);        \
  rw.boxes = carve.take<TriBox>((size_t)V * (size_t)Nt_max);       \
  GPN_CHECK_WS(carve)

extern "C" int gpn_render_setup(const float* verts, int Nv, const int32_t* tris, const int32_t* tri_visual, int Nt,
                                const int32_t* assets, int A, const int32_t* view_asset, const double* cam, const double* vis_mat,
                                int M, int V, int H, int W, int Nt_max, void* ws, size_t ws_bytes, int32_t* counters,
                                gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_shape(__func__, V, H, W, Nt_max)) return rc;
  GPN_CHECK_ARG(Nv >= 0 && Nt >= 0 && A >= 0 && M >= 0 && Nt_max <= Nt && (int64_t)Nv * 3 < (int64_t)0x7fffffff &&
                (int64_t)Nt * 3 < (int64_t)0x7fffffff);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(counters && view_asset && cam && (A == 0 || assets));
  GPN_CHECK_HIP(hipMemsetAsync(counters, 0, (size_t)V * GPN_RENDER_COUNTERS * sizeof(int32_t), stream));
  if (Nt_max == 0) return GPN_OK;
  GPN_CHECK_ARG(verts && tris && tri_visual && assets && vis_mat && M >= 1);
  RD_CARVE_WS();
  hipLaunchKernelGGL(rd_setup_kernel, dim3((unsigned)gpn::cdiv(Nt_max, 256), (unsigned)V), dim3(256), 0, stream, verts, Nv, tris,
                     tri_visual, Nt, assets, A, view_asset, cam, vis_mat, M, H, W, Nt_max, rw.recs, rw.boxes, counters);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_render_raster(const int32_t* assets, int A, const int32_t* view_asset, int Nt, int V, int H, int W, int Nt_max,
                                 const void* ws_, size_t ws_bytes, float* depth, int32_t* tri, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  void* ws = const_cast<void*>(ws_);
  if (int rc = check_shape(__func__, V, H, W, Nt_max)) return rc;
  GPN_CHECK_ARG(Nt >= 0 && A >= 0 && Nt_max <= Nt);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(depth && tri && view_asset && (A == 0 || assets));
  RD_CARVE_WS();
  hipLaunchKernelGGL(rd_raster_kernel, dim3((unsigned)gpn::cdiv(W, kTile), (unsigned)gpn::cdiv(H, kTile), (unsigned)V),
                     dim3(kLanes), 0, stream, assets, A, view_asset, Nt, H, W, Nt_max, rw.recs, rw.boxes, depth, tri);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_render_max_links(void) { return kMaxLinks; }

extern "C" int gpn_render_annotate(const float* depth, const int32_t* tri, const int32_t* tri_link, const float* tri_color, int Nt,
                                   const int32_t* assets, int A, const int32_t* view_asset, const double* cam,
                                   const int32_t* link_cat, const int32_t* link_rank, const double* link_frame, int L, int V, int H,
                                   int W, int Nt_max, const void* ws_, size_t ws_bytes, int bg_r, int bg_g, int bg_b,
                                   int32_t* link_area, int32_t* link_inst, int32_t* sem, int32_t* ins, float* npcs, uint8_t* rgb,
                                   gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  void* ws = const_cast<void*>(ws_);
  if (int rc = check_shape(__func__, V, H, W, Nt_max)) return rc;
  GPN_CHECK_ARG(Nt >= 0 && A >= 0 && Nt_max <= Nt && L >= 0 && L <= kMaxLinks);
  GPN_CHECK_ARG(bg_r >= 0 && bg_r <= 255 && bg_g >= 0 && bg_g <= 255 && bg_b >= 0 && bg_b <= 255);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(depth && tri && view_asset && cam && sem && ins && npcs && rgb && (A == 0 || assets));
  GPN_CHECK_ARG(L == 0 || (link_cat && link_rank && link_frame && link_area && link_inst));
  GPN_CHECK_ARG(Nt == 0 || (tri_link && tri_color));
  RD_CARVE_WS();
  const int64_t HW = (int64_t)H * W;
  if (L > 0) {
    GPN_CHECK_HIP(hipMemsetAsync(link_area, 0, (size_t)V * L * sizeof(int32_t), stream));
    int64_t gx = gpn::cdiv(HW, 256 * 16);  // 16 pixels a thread: the LDS histogram absorbs most atomics
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(rd_area_kernel, dim3((unsigned)gx, (unsigned)V), dim3(256), 0, stream, tri, tri_link, Nt, assets, A,
                       view_asset, HW, L, link_area);
    GPN_CHECK_LAUNCH();
    hipLaunchKernelGGL(rd_inst_kernel, dim3((unsigned)V), dim3(256), 0, stream, link_cat, link_rank, link_area, L, link_inst);
    GPN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(rd_pixel_kernel, dim3((unsigned)gpn::cdiv(HW, 256), (unsigned)V), dim3(256), 0, stream, depth, tri, tri_link,
                     tri_color, Nt, assets, A, view_asset, cam, link_cat, link_inst, link_frame, L, H, W, Nt_max, rw.recs, bg_r,
                     bg_g, bg_b, sem, ins, npcs, rgb);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_render_max_lights(void) { return kMaxLights; }

extern "C" int gpn_render_shade(const float* verts, int Nv, const int32_t* tris, const int32_t* tri_visual, const float* tri_color,
                                int Nt, const int32_t* assets, int A, const int32_t* view_asset, const double* cam,
                                const double* vis_mat, int M, const float* tri_uv, const int32_t* tri_tex, const int32_t* tex_table,
                                int T, const void* tex_data, int64_t texels, const double* lights, int NL, const float* depth,
                                const int32_t* tri, int V, int H, int W, int Nt_max, int bg_r, int bg_g, int bg_b, uint8_t* rgb,
                                gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_shape(__func__, V, H, W, Nt_max)) return rc;
  GPN_CHECK_ARG(Nv >= 0 && Nt >= 0 && A >= 0 && M >= 0 && Nt_max <= Nt && (int64_t)Nv * 3 < (int64_t)0x7fffffff &&
                (int64_t)Nt * 6 < (int64_t)0x7fffffff);
  GPN_CHECK_ARG(NL >= 0 && NL <= kMaxLights);
  GPN_CHECK_ARG(T >= 0 && T <= 0x7fffffff / 4 && texels >= 0 && texels < (int64_t)0x7fffffff);
  GPN_CHECK_ARG(bg_r >= 0 && bg_r <= 255 && bg_g >= 0 && bg_g <= 255 && bg_b >= 0 && bg_b <= 255);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(depth && tri && rgb && view_asset && cam && (A == 0 || assets) && (NL == 0 || lights));
  GPN_CHECK_ARG(Nt_max == 0 || (verts && tris && tri_visual && tri_color && assets && vis_mat && M >= 1));
  GPN_CHECK_ARG(T == 0 || (tri_uv && tri_tex && tex_table && tex_data && texels >= T));
  hipLaunchKernelGGL(rs_shade_kernel, dim3((unsigned)gpn::cdiv(W, kTile), (unsigned)gpn::cdiv(H, kTile), (unsigned)V), dim3(kLanes),
                     0, stream, verts, Nv, tris, tri_visual, tri_color, Nt, assets, A, view_asset, cam, vis_mat, M, tri_uv, tri_tex,
                     tex_table, T, (const uint32_t*)tex_data, texels, lights, NL, depth, tri, H, W, Nt_max, bg_r, bg_g, bg_b, rgb);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
