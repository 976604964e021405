// viewprep.hip — rendered RGB-D views -> training scenes for a batch of V views of one size H x W, the work of the reference's
// dataset/process_tools/convert_rendered_into_input.py (sample_and_save, :90-175) in three launches:
//   backproject  valid pixels (sem != -2 and ins != -2, :55) in row-major order, float64 back-projection (:57-59), the float32
//                cast FPS samples from, per-view counts and the label-mismatch status (:112)
//   fps          ragged multi-view furthest point sampling (utils/sample_utils.py:46-66): per view the samples of
//                gpn_pn2_furthest_point_sampling on that view alone; "too few" and "exactly m" decided in the kernel
//   finish       gather, ball normalisation (:71-87), label mapping and the relabel loop (:136-147), gt labels (:162-171)
// Counts and statuses stay on the device between the launches.
#include <cmath>

#include "gpn_common.h"
#include "point_prims.h"

namespace {

using namespace gpn;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kPixPerThread = 4;  // back-projection: consecutive pixels per thread and tile step
constexpr int kPpt = 16;          // fps: points per thread held in VGPRs for all m iterations
constexpr int kMaxGroups = 64;    // fps: workgroups per view (one wave reduces their candidates)
constexpr int kMaxInst = 4096;    // finish: instance ids 0 .. kMaxInst - 1 (LDS presence / remap / first-point tables)

__device__ __forceinline__ double depth_at(const void* depth, int depth_f64, int64_t i) {
  return depth_f64 ? ((const double*)depth)[i] : (double)((const float*)depth)[i];
}

// reference :58-59, float64, left to right: ((pix - c) * z) / f  (-ffp-contract=off: no fused multiply-add)
__device__ __forceinline__ double unproject(int pix, double c, double z, double f) { return (((double)pix - c) * z) / f; }

// ---- 1. back-projection + stable compaction: one workgroup per view, tiles of kThreads * kPixPerThread pixels ----------------
// A thread takes kPixPerThread consecutive pixels; an inclusive scan of the per-thread counts over the workgroup (block_scan)
// gives every valid pixel its row-major rank; the running tile base is the cross-tile scan.
__global__ __launch_bounds__(kThreads) void vp_backproject_kernel(const void* __restrict__ depth, int depth_f64,
                                                                  const int32_t* __restrict__ sem,
                                                                  const int32_t* __restrict__ ins,
                                                                  const double* __restrict__ Ks, int H, int W,
                                                                  int32_t* __restrict__ pixel, float4* __restrict__ points,
                                                                  int32_t* __restrict__ counts, int32_t* __restrict__ status) {
  __shared__ int wsum[kWaves];
  const int v = blockIdx.x;
  const int64_t HW = (int64_t)H * W, off = (int64_t)v * HW;
  const double* K = Ks + (int64_t)v * 9;
  const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
  const int tid = threadIdx.x;
  int base = 0, bad = 0;
  for (int64_t p0 = 0; p0 < HW; p0 += kThreads * kPixPerThread) {
    const int64_t q0 = p0 + (int64_t)tid * kPixPerThread;
    unsigned vm = 0;
    int c = 0;
#pragma unroll
    for (int e = 0; e < kPixPerThread; ++e) {
      const int64_t p = q0 + e;
      if (p < HW) {
        const int s = sem[off + p], i = ins[off + p];
        if (s != -2 && i != -2) {
          vm |= 1u << e;
          ++c;
          bad |= (s == -1) != (i == -1);
        }
      }
    }
    int total;
    int pos = base + block_scan<kWaves>(c, wsum, &total) - c;
#pragma unroll
    for (int e = 0; e < kPixPerThread; ++e) {
      if (vm >> e & 1u) {
        const int p = (int)(q0 + e);
        const int y = p / W, x = p - y * W;
        const double z = depth_at(depth, depth_f64, off + p);
        const double X = unproject(x, cx, z, fx), Y = unproject(y, cy, z, fy);
        pixel[off + pos] = p;
        points[off + pos] = make_float4((float)X, (float)Y, (float)z, 1e10f);
        ++pos;
      }
    }
    base += total;
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    counts[v] = base;
    status[v] = bad ? GPN_VIEW_LABEL_MISMATCH : GPN_VIEW_OK;
  }
}

// ---- 2. ragged multi-view FPS ------------------------------------------------------------------------------------------------
// G workgroups per view; member w owns the contiguous chunk [lo, hi) of the view's n points.  The first kPpt * kThreads points of
// the chunk and their running distances live in VGPRs for all m iterations; the rest (views larger than G * kPpt * kThreads
// points) stream through memory with the running distance in .w.  Per sample: the chunk's candidate (point_prims.h: the candidate
// order of gpn_pn2_furthest_point_sampling for the view's own n, fps_block_best), then (G > 1) one exchange of the G candidates at
// a per-view counter (fps_meet).  G == 1: no inter-workgroup wait at all.  Workgroup i serves view (i / 8 / G) * 8 + i % 8: the G
// members of a view share i % 8, the XCD of round-robin dispatch (speed only).
__global__ __launch_bounds__(kThreads) void vp_fps_kernel(float4* __restrict__ points, int64_t n_bound,
                                                          const int32_t* __restrict__ counts, int32_t* __restrict__ status,
                                                          int V, int m, int G, int32_t* __restrict__ idxs, float* cand_v,
                                                          int* cand_k, unsigned* arrived) {
  __shared__ float wv[kWaves];
  __shared__ int wk[kWaves];
  __shared__ int s_old;
  const int slot = blockIdx.x >> 3;
  const int v = (slot / G) * 8 + (blockIdx.x & 7), w = slot % G;
  if (v >= V || status[v] != GPN_VIEW_OK) return;  // (the same answer for every member of the view)
  const int n = (int)min((int64_t)counts[v], n_bound);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* out = idxs + (int64_t)v * m;
  if (n < m) {  // sample_utils.py:55-57
    if (w == 0 && tid == 0) status[v] = GPN_VIEW_TOO_FEW;
    return;
  }
  if (n == m) {  // sample_utils.py:59-60: arange, no sampling
    if (w == 0)
      for (int j = tid; j < m; j += kThreads) out[j] = j;
    return;
  }
  const int bmask = fps_bmask(n);
  float4* d = points + (int64_t)v * n_bound;
  const int chunk = (n + G - 1) / G;
  const int lo = min(w * chunk, n), hi = min(lo + chunk, n);
  const int rlo = lo + kPpt * kThreads;  // first streamed point of the chunk
  float px[kPpt], py[kPpt], pz[kPpt], pd[kPpt];
#pragma unroll
  for (int e = 0; e < kPpt; ++e) {
    const int k = lo + tid + e * kThreads;
    if (k < hi) {
      const float4 q = d[k];
      px[e] = q.x; py[e] = q.y; pz[e] = q.z; pd[e] = 1e10f;
    } else {
      px[e] = py[e] = pz[e] = 0.f;
      pd[e] = -1.f;  // no point: never a candidate (distances are >= 0)
    }
  }
  for (int k = rlo + tid; k < hi; k += kThreads) reinterpret_cast<float*>(d + k)[3] = 1e10f;
  float* cv = cand_v + (int64_t)v * 2 * G;
  int* ck = cand_k + (int64_t)v * 2 * G;
  unsigned* counter = arrived + v;
  int old = 0;
  if (w == 0 && tid == 0) out[0] = 0;
  for (int j = 1; j < m; ++j) {
    const float* o = reinterpret_cast<const float*>(d + old);
    const float x1 = o[0], y1 = o[1], z1 = o[2];
    // a thread's points share k & bmask (k steps by 1024): within the thread, the larger distance then the lower k wins
    FpsCand c = {-1.f, 0x7fffffff};
#pragma unroll
    for (int e = 0; e < kPpt; ++e) {
      const float dd = dist2_nofma(px[e], py[e], pz[e], x1, y1, z1);
      const float d2 = dd < pd[e] ? dd : pd[e];
      pd[e] = d2;
      if (d2 > c.v) { c.v = d2; c.k = lo + tid + e * kThreads; }
    }
    for (int k = rlo + tid; k < hi; k += kThreads) {
      const float4 q = d[k];
      const float dd = dist2_nofma(q.x, q.y, q.z, x1, y1, z1);
      const float d2 = dd < q.w ? dd : q.w;
      reinterpret_cast<float*>(d + k)[3] = d2;
      if (d2 > c.v) { c.v = d2; c.k = k; }
    }
    c = fps_block_best<kWaves>(c, bmask, wv, wk);
    if (wave == 0) {
      if (G > 1) c = fps_meet(c, j, G, w, bmask, cv, ck, counter);
      if (lane == 0) {
        s_old = c.k;
        if (w == 0) out[j] = c.k;
      }
    }
    __syncthreads();
    old = s_old;
  }
}

// ---- 3. finish: one workgroup per view ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void vp_finish_kernel(
    const void* __restrict__ depth, int depth_f64, const uint8_t* __restrict__ rgb, const int32_t* __restrict__ sem,
    const int32_t* __restrict__ ins, const float* __restrict__ npcs, const double* __restrict__ Ks, int H, int W,
    const int32_t* __restrict__ pixel, const int32_t* __restrict__ fps_idx, int m, int32_t* __restrict__ status,
    float* __restrict__ xyz_out, float* __restrict__ rgb_out, int32_t* __restrict__ sem_out, int32_t* __restrict__ ins_out,
    float* __restrict__ npcs_out, int32_t* __restrict__ pix_out, int32_t* __restrict__ gt_out, double* __restrict__ scale_out) {
  __shared__ int present[kMaxInst];
  __shared__ int remap[kMaxInst];
  __shared__ int first[kMaxInst];
  __shared__ double red[6][kWaves];
  const int v = blockIdx.x, tid = threadIdx.x;
  if (status[v] != GPN_VIEW_OK) return;
  const int64_t HW = (int64_t)H * W, off = (int64_t)v * HW;
  const double* K = Ks + (int64_t)v * 9;
  const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
  const int32_t* fi = fps_idx + (int64_t)v * m;
  const int32_t* pix = pixel + off;
  for (int q = tid; q < kMaxInst; q += kThreads) { present[q] = 0; remap[q] = q; first[q] = 0x7fffffff; }
  // centre (:74, (max + min) / 2) and radius (:75) of the sampled float64 points
  double ctr[3], r;
  ball_of_samples<kWaves>(
      [&](int j, double* P) {
        const int p = pix[fi[j]];
        const int y = p / W, x = p - y * W;
        const double z = depth_at(depth, depth_f64, off + p);
        P[0] = unproject(x, cx, z, fx); P[1] = unproject(y, cy, z, fy); P[2] = z;
      },
      m, red, ctr, &r);
  // outputs; instance ids before the relabel loop
  int over = 0;
  for (int j = tid; j < m; j += kThreads) {
    const int p = pix[fi[j]];
    const int y = p / W, x = p - y * W;
    const int64_t g = off + p;
    const double z = depth_at(depth, depth_f64, g);
    const double P[3] = {unproject(x, cx, z, fx), unproject(y, cy, z, fy), z};
    const int64_t o = (int64_t)v * m + j;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      xyz_out[o * 3 + c] = (float)((P[c] - ctr[c]) / r);            // :86, then astype(float32)
      rgb_out[o * 3 + c] = (float)((double)rgb[g * 3 + c] / 255.0);  // :61
      npcs_out[o * 3 + c] = npcs[g * 3 + c];
    }
    const int s = sem[g], i = ins[g];
    sem_out[o] = s + 1;                 // :136
    const int io = i == -1 ? -100 : i;  // :137-139
    ins_out[o] = io;
    pix_out[o * 2] = y;
    pix_out[o * 2 + 1] = x;
    if (io >= kMaxInst) over = 1;
    else if (io >= 0) present[io] = 1;
  }
  if (__syncthreads_or(over)) {
    if (tid == 0) status[v] = GPN_VIEW_INSTANCE_BOUND;
    return;
  }
  if (tid == 0) {
    // :142-147: while j < max: if j is absent, the points holding the current max get j.  A moved id is always the current
    // maximum and never moves again, so one table from original to final id describes the loop.
    int top = kMaxInst - 1;
    while (top >= 0 && !present[top]) --top;
    for (int j = 0; j < top; ++j) {
      if (!present[j]) {
        remap[top] = j;
        present[j] = 1;
        present[top] = 0;
        while (!present[top]) --top;
      }
    }
    scale_out[(int64_t)v * 4] = r;
    for (int c = 0; c < 3; ++c) scale_out[(int64_t)v * 4 + 1 + c] = ctr[c];
  }
  __syncthreads();
  for (int j = tid; j < m; j += kThreads) {
    const int64_t o = (int64_t)v * m + j;
    const int io = ins_out[o];  // (written by this thread above)
    if (io >= 0) {
      const int in = remap[io];
      ins_out[o] = in;
      atomicMin(&first[in], j);
    }
  }
  __syncthreads();
  // :162-171: sem of the instance's first point * 1000 + id, -100 elsewhere
  for (int j = tid; j < m; j += kThreads) {
    const int64_t o = (int64_t)v * m + j;
    const int in = ins_out[o];
    int gt = -100;
    if (in >= 0) gt = (sem[off + pix[fi[first[in]]]] + 1) * 1000 + in;
    gt_out[o] = gt;
  }
}

int fps_groups(int V, int max_groups) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
    (void)hipGetLastError();
    return 1;
  }
  const int v8 = (V + 7) / 8 * 8;
  int g = cus / v8;  // grid = v8 * g <= CUs: one 1024-thread workgroup per CU is all the residency the wait needs
  if (g > kMaxGroups) g = kMaxGroups;
  if (max_groups > 0 && g > max_groups) g = max_groups;
  return g < 2 ? 1 : g;
}

}  // namespace

extern "C" int gpn_view_max_instance_ids(void) { return kMaxInst; }

extern "C" int gpn_view_backproject(const void* depth, int depth_bytes, const int32_t* sem, const int32_t* ins, const double* K,
                                    int V, int H, int W, int32_t* pixel, float* points, int32_t* counts, int32_t* status,
                                    gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(V >= 0 && H >= 1 && W >= 1 && (int64_t)H * W < (int64_t)0x7fffffff);
  GPN_CHECK_ARG(depth_bytes == 4 || depth_bytes == 8);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(depth && sem && ins && K && pixel && points && counts && status);
  hipLaunchKernelGGL(vp_backproject_kernel, dim3(V), dim3(kThreads), 0, stream, depth, depth_bytes == 8 ? 1 : 0, sem, ins, K, H,
                     W, pixel, reinterpret_cast<float4*>(points), counts, status);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" size_t gpn_view_fps_ws_bytes(int V) {
  if (V <= 0) return 0;
  return gpn::align_up((size_t)V * 2 * kMaxGroups * sizeof(float)) + gpn::align_up((size_t)V * 2 * kMaxGroups * sizeof(int)) +
         gpn::align_up((size_t)V * sizeof(unsigned));
}

extern "C" int gpn_view_fps(float* points, int64_t n_bound, const int32_t* counts, int32_t* status, int V, int m, int max_groups,
                            int32_t* idx, void* ws, size_t ws_bytes, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(V >= 0 && m >= 1 && n_bound >= 1 && n_bound < (int64_t)0x7fffffff);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(points && counts && status && idx);
  gpn::WsCarver carve(ws, ws_bytes);
  float* cand_v = carve.take<float>((size_t)V * 2 * kMaxGroups);
  int* cand_k = carve.take<int>((size_t)V * 2 * kMaxGroups);
  unsigned* arrived = carve.take<unsigned>((size_t)V);
  GPN_CHECK_WS(carve);
  int G = fps_groups(V, max_groups);
  if (!fps_meetings_fit(m, G)) G = 1;
  float4* pts = reinterpret_cast<float4*>(points);
  void* args[] = {&pts, &n_bound, &counts, &status, &V, &m, &G, &idx, &cand_v, &cand_k, &arrived};
  return fps_launch(__func__, (const void*)vp_fps_kernel, (const void*)vp_fps_kernel, (unsigned)((V + 7) / 8 * 8), &G, args, arrived,
                    (size_t)V, stream);
}

extern "C" int gpn_view_finish(const void* depth, int depth_bytes, const uint8_t* rgb, const int32_t* sem, const int32_t* ins,
                               const float* npcs, const double* K, int V, int H, int W, const int32_t* pixel, const int32_t* idx,
                               int m, int32_t* status, float* xyz_out, float* rgb_out, int32_t* sem_out, int32_t* ins_out,
                               float* npcs_out, int32_t* pix_out, int32_t* gt_out, double* scale_out, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(V >= 0 && H >= 1 && W >= 1 && (int64_t)H * W < (int64_t)0x7fffffff && m >= 1);
  GPN_CHECK_ARG(depth_bytes == 4 || depth_bytes == 8);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(depth && rgb && sem && ins && npcs && K && pixel && idx && status);
  GPN_CHECK_ARG(xyz_out && rgb_out && sem_out && ins_out && npcs_out && pix_out && gt_out && scale_out);
  hipLaunchKernelGGL(vp_finish_kernel, dim3(V), dim3(kThreads), 0, stream, depth, depth_bytes == 8 ? 1 : 0, rgb, sem, ins, npcs, K,
                     H, W, pixel, idx, m, status, xyz_out, rgb_out, sem_out, ins_out, npcs_out, pix_out, gt_out, scale_out);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
