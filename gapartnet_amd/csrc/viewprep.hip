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

namespace {

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

__device__ __forceinline__ float dist2_nofma(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// the candidate order of pointnet2.hip (fps_better): distance, then the reference's block-reduction tie-break for its block
// size opt_n_threads(n) (bit-reversed thread id k & bmask), then index.  A total order: any split of a view's points over
// workgroups gives the same winner.
__device__ __forceinline__ bool fps_better(float av, int ak, float bv, int bk, int bmask) {
  if (av != bv) return av > bv;
  const unsigned ta = __brev((unsigned)(ak & bmask)), tb = __brev((unsigned)(bk & bmask));
  if (ta != tb) return ta < tb;
  return ak < bk;
}

// opt_n_threads(n) - 1 (cuda_utils.h:10-14): the largest power of two <= n, at most 1024.  The host form
// (int)(log(n) / log(2)) equals floor(log2(n)) for every n in [1, 2^21] (tests/test_convert_cpu.py), and n >= 1024 gives 1024.
__device__ __forceinline__ int fps_bmask(int n) {
  const int v = n >= 1024 ? 1024 : (1 << (31 - __clz(n)));
  return v - 1;
}

// ---- 1. back-projection + stable compaction: one workgroup per view, tiles of kThreads * kPixPerThread pixels ----------------
// A thread takes kPixPerThread consecutive pixels; an inclusive shuffle scan of the per-thread counts inside each wave and a scan
// of the 16 wave totals give every valid pixel its row-major rank; the running tile base is the cross-tile scan.
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
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int s = wsum[w];
      before += w < wave ? s : 0;
      total += s;
    }
    int pos = base + before + incl - c;
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
    __syncthreads();  // wsum is rewritten by the next tile
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
// points) stream through memory with the running distance in .w.  Per sample: the chunk's candidate by wave shuffles and LDS,
// then (G > 1) one exchange of the G (value, index) candidates at a per-view counter, as pn2_fps_multi_kernel does.  G == 1: no
// inter-workgroup wait at all.  Workgroup i serves view (i / 8 / G) * 8 + i % 8: the G members of a view share i % 8, the XCD of
// round-robin dispatch (speed only).
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
    float best = -1.f;
    int besti = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < kPpt; ++e) {
      const float dd = dist2_nofma(px[e], py[e], pz[e], x1, y1, z1);
      const float d2 = dd < pd[e] ? dd : pd[e];
      pd[e] = d2;
      if (d2 > best) { best = d2; besti = lo + tid + e * kThreads; }
    }
    for (int k = rlo + tid; k < hi; k += kThreads) {
      const float4 q = d[k];
      const float dd = dist2_nofma(q.x, q.y, q.z, x1, y1, z1);
      const float d2 = dd < q.w ? dd : q.w;
      reinterpret_cast<float*>(d + k)[3] = d2;
      if (d2 > best) { best = d2; besti = k; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ov = __shfl_down(best, off, 64);
      const int ok = __shfl_down(besti, off, 64);
      if (lane + off < 64 && fps_better(ov, ok, best, besti, bmask)) { best = ov; besti = ok; }
    }
    if (lane == 0) { wv[wave] = best; wk[wave] = besti; }
    __syncthreads();
    if (wave == 0) {
      float bv = lane < kWaves ? wv[lane] : -2.f;
      int bk = lane < kWaves ? wk[lane] : 0x7fffffff;
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) {
        const float ov = __shfl_down(bv, off, 64);
        const int ok = __shfl_down(bk, off, 64);
        if (fps_better(ov, ok, bv, bk, bmask)) { bv = ov; bk = ok; }
      }
      if (G > 1) {
        const int sl = (j & 1) * G;
        if (lane == 0) {
          __hip_atomic_store(cv + sl + w, bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(ck + sl + w, bk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __threadfence();
          __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          const unsigned want = (unsigned)G * (unsigned)j;  // j-th meeting of the G members (m * G < 2^31: host-checked)
          while (__hip_atomic_load(counter, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < want) __builtin_amdgcn_s_sleep(1);
          __threadfence();
        }
        __threadfence();  // every lane: the candidate reads below stay behind lane 0's acquire
        bv = -2.f;
        bk = 0x7fffffff;
        if (lane < G) {
          bv = __hip_atomic_load(cv + sl + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          bk = __hip_atomic_load(ck + sl + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          const float ov = __shfl_down(bv, off, 64);
          const int ok = __shfl_down(bk, off, 64);
          if (lane + off < 64 && fps_better(ov, ok, bv, bk, bmask)) { bv = ov; bk = ok; }
        }
      }
      if (lane == 0) {
        s_old = bk;
        if (w == 0) out[j] = bk;
      }
    }
    __syncthreads();
    old = s_old;
  }
}

// ---- 3. finish: one workgroup per view ---------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_min(double a) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a = fmin(a, __shfl_xor(a, off, 64));
  return a;
}
__device__ __forceinline__ double wave_max(double a) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a = fmax(a, __shfl_xor(a, off, 64));
  return a;
}

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
  const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (status[v] != GPN_VIEW_OK) return;
  const int64_t HW = (int64_t)H * W, off = (int64_t)v * HW;
  const double* K = Ks + (int64_t)v * 9;
  const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
  const int32_t* fi = fps_idx + (int64_t)v * m;
  const int32_t* pix = pixel + off;
  for (int q = tid; q < kMaxInst; q += kThreads) { present[q] = 0; remap[q] = q; first[q] = 0x7fffffff; }
  // min / max of the sampled float64 points (exact: the order of a min / max does not matter)
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int j = tid; j < m; j += kThreads) {
    const int p = pix[fi[j]];
    const int y = p / W, x = p - y * W;
    const double z = depth_at(depth, depth_f64, off + p);
    const double P[3] = {unproject(x, cx, z, fx), unproject(y, cy, z, fy), z};
#pragma unroll
    for (int c = 0; c < 3; ++c) { mn[c] = fmin(mn[c], P[c]); mx[c] = fmax(mx[c], P[c]); }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { mn[c] = wave_min(mn[c]); mx[c] = wave_max(mx[c]); }
  if (lane == 0)
    for (int c = 0; c < 3; ++c) { red[c][wave] = mn[c]; red[3 + c][wave] = mx[c]; }
  __syncthreads();
  double ctr[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double a = red[c][0], b = red[3 + c][0];
    for (int q = 1; q < kWaves; ++q) { a = fmin(a, red[c][q]); b = fmax(b, red[3 + c][q]); }
    ctr[c] = (b + a) / 2.0;  // :74 (max + min) / 2
  }
  __syncthreads();  // red is reused below
  // r^2 = max of (dx^2 + dy^2) + dz^2 (:75; the square root is monotonic, so sqrt(max) = max(sqrt))
  double r2 = -INFINITY;
  for (int j = tid; j < m; j += kThreads) {
    const int p = pix[fi[j]];
    const int y = p / W, x = p - y * W;
    const double z = depth_at(depth, depth_f64, off + p);
    const double dx = unproject(x, cx, z, fx) - ctr[0], dy = unproject(y, cy, z, fy) - ctr[1], dz = z - ctr[2];
    r2 = fmax(r2, (dx * dx + dy * dy) + dz * dz);
  }
  r2 = wave_max(r2);
  if (lane == 0) red[0][wave] = r2;
  __syncthreads();
  r2 = red[0][0];
  for (int q = 1; q < kWaves; ++q) r2 = fmax(r2, red[0][q]);
  const double r = __dsqrt_rn(r2);
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
  if ((int64_t)m * G >= (int64_t)0x7fffffff) G = 1;
  float4* pts = reinterpret_cast<float4*>(points);
  int nv = V, mm = m;
  int64_t nb = n_bound;
  if (G > 1) {
    GPN_CHECK_HIP(hipMemsetAsync(arrived, 0, (size_t)V * sizeof(unsigned), stream));
    // the counter wait runs only under a cooperative launch: the runtime starts the grid only when all of its workgroups can be
    // resident at once, and refuses one that cannot be
    void* args[] = {&pts, &nb, &counts, &status, &nv, &mm, &G, &idx, &cand_v, &cand_k, &arrived};
    const unsigned grid = (unsigned)((V + 7) / 8 * 8 * G);
    if (hipLaunchCooperativeKernel((const void*)vp_fps_kernel, dim3(grid), dim3(kThreads), args, 0, stream) == hipSuccess)
      return GPN_OK;
    (void)hipGetLastError();  // refused: the form without any inter-workgroup wait
  }
  hipLaunchKernelGGL(vp_fps_kernel, dim3((unsigned)((V + 7) / 8 * 8)), dim3(kThreads), 0, stream, pts, nb, counts, status, nv, mm,
                     1, idx, cand_v, cand_k, arrived);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
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
