// frameprep.hip — RGB-D frames -> the rows and the packed layout the raw-cloud path reads (include/gpn.h section FR).  A batch of V
// frames of one size H x W:
//   backproject  one row [x y z r g b] per pixel in row-major order, float32 cast of the float64 pinhole arithmetic; an invalid
//                pixel's xyz is NaN; a validity byte per pixel and the valid count per frame
//   select       the seeded presample: per frame the `cap` valid pixels with the smallest (hash, pixel) key.  A radix select of the
//                cap-th smallest hash, 8 bits a pass: every workgroup histograms its chunk's digits in LDS and merges them into the
//                frame's histogram with integer adds; the next pass (and the count pass) resolves the digit from that histogram
//                on the device.  The last resolve leaves the threshold hash t and the number r of pixels with hash == t to admit,
//                lowest pixel first.  Then per-chunk counts, one scan over the chunks per frame, and an ORDERED compaction: wave
//                ballots give every kept pixel its slot, so rows come out in ascending pixel order.
// A frame is shared by cdiv(H W, kChunk) workgroups in every pass but the scan over its chunks.  No float atomics; integer atomics
// only on histograms and counters (order-free); no host read; every result is independent of timing.
#include <cmath>

#include "gpn_common.h"
#include "point_prims.h"

namespace {

using namespace gpn;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 4;                    // pixels per thread: pixel = chunk * kChunk + e * kThreads + tid
constexpr int kChunk = kThreads * kPer;
constexpr int kPasses = kSelectPasses;     // 32-bit hash, 8 bits a pass (point_prims.h)
constexpr int kBins = kSelectBins;

struct FrameSel {  // per frame, written by fr_count_kernel
  uint32_t t;      // threshold: hashes below it are kept
  int32_t r;       // pixels with hash == t to admit, lowest pixel first
  int32_t keep_all;
  int32_t pad;
};

// ---- 1. back-projection: one workgroup per chunk of a frame ---------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void fr_backproject_kernel(const T* __restrict__ depth, double depth_scale,
                                                                  const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ keep,
                                                                  const double* __restrict__ K, int H, int W, int flip,
                                                                  float* __restrict__ rows, uint8_t* __restrict__ valid,
                                                                  int32_t* __restrict__ valid_counts) {
  __shared__ int wsum[kWaves];
  const int v = blockIdx.y, tid = threadIdx.x;
  const int64_t HW = (int64_t)H * W;
  const double* Kv = K + (int64_t)v * 9;
  const double fx = Kv[0], cx = Kv[2], fy = Kv[4], cy = Kv[5];
  const float nan = __int_as_float(0x7fc00000);
  int c = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (p >= HW) continue;
    const int64_t g = (int64_t)v * HW + p;
    const double z = (double)depth[g] / depth_scale;
    bool ok = z > 0.0 && z < (double)INFINITY && (!keep || keep[g] != 0);  // (NaN fails z > 0)
    float X = nan, Y = nan, Z = nan;
    if (ok) {
      const double u = (double)(p % W), w = (double)(p / W);
      X = (float)(((u - cx) * z) / fx);
      Y = (float)(((w - cy) * z) / fy);
      Z = (float)z;
      ok = finite_bits(X) && finite_bits(Y) && finite_bits(Z);  // DECISION: a float32 overflow is "no point"
      if (flip) { Y = -Y; Z = -Z; }
      if (!ok) X = Y = Z = nan;
    }
    float* q = rows + g * 6;
    q[0] = X; q[1] = Y; q[2] = Z;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) q[3 + ch] = (float)((double)rgb[g * 3 + ch] / 255.0);
    valid[g] = ok ? 1 : 0;
    c += ok ? 1 : 0;
  }
  const int tot = block_sum<kWaves>(c, wsum);
  if (tid == 0 && tot > 0) atomicAdd(valid_counts + v, tot);  // (an integer counter: order-free)
}

// ---- 2. radix select ------------------------------------------------------------------------------------------------------------
// (the resolve of the cap-th smallest hash from the merged histograms: select_resolve, point_prims.h)
// pass j: the histogram of digit j over the valid pixels whose higher digits equal the resolved prefix
__global__ __launch_bounds__(kThreads) void fr_hist_kernel(const uint8_t* __restrict__ valid, const int32_t* __restrict__ valid_counts,
                                                           const uint32_t* __restrict__ seeds, int64_t HW, int cap, int hash_bits,
                                                           int pass, uint32_t* __restrict__ hist_all) {
  __shared__ int wsum[kWaves];
  __shared__ int sh[2];
  __shared__ uint32_t bins[kBins];
  const int v = blockIdx.y, tid = threadIdx.x;
  if (valid_counts[v] <= cap) return;  // the frame keeps every valid pixel (uniform over the workgroup)
  uint32_t* hist = hist_all + (int64_t)v * kPasses * kBins;
  uint32_t prefix;
  int k;
  select_resolve<kWaves>(hist, pass, cap, wsum, sh, &prefix, &k);
  bins[tid] = 0;
  __syncthreads();
  const uint32_t seed = seeds[v];
  const int shift = 24 - 8 * pass;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (p >= HW || !valid[(int64_t)v * HW + p]) continue;
    const uint32_t hq = hash_key(seed, (uint32_t)p, hash_bits);
    if (pass == 0 || (hq >> (shift + 8)) == prefix) atomicAdd(&bins[(hq >> shift) & 255u], 1u);
  }
  __syncthreads();
  const uint32_t b = bins[tid];
  if (b) atomicAdd(hist + pass * kBins + tid, b);  // (merged by integer adds: order-free)
}

// per chunk: the pixels below the threshold and the pixels on it
__global__ __launch_bounds__(kThreads) void fr_count_kernel(const uint8_t* __restrict__ valid, const int32_t* __restrict__ valid_counts,
                                                            const uint32_t* __restrict__ seeds, int64_t HW, int cap, int hash_bits,
                                                            const uint32_t* __restrict__ hist_all, FrameSel* __restrict__ sel,
                                                            int32_t* __restrict__ chunk_less, int32_t* __restrict__ chunk_eq) {
  __shared__ int wsum[kWaves];
  __shared__ int sh[2];
  const int v = blockIdx.y, tid = threadIdx.x;
  const bool keep_all = cap <= 0 || valid_counts[v] <= cap;
  uint32_t t = 0xffffffffu;
  int r = 0;
  if (!keep_all) select_resolve<kWaves>(hist_all + (int64_t)v * kPasses * kBins, kPasses, cap, wsum, sh, &t, &r);
  const uint32_t seed = seeds[v];
  int less = 0, eq = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    if (p >= HW || !valid[(int64_t)v * HW + p]) continue;
    const uint32_t hq = hash_key(seed, (uint32_t)p, hash_bits);
    less += (keep_all || hq < t) ? 1 : 0;
    eq += (!keep_all && hq == t) ? 1 : 0;
  }
  less = block_sum<kWaves>(less, wsum);
  eq = block_sum<kWaves>(eq, wsum);
  if (tid == 0) {
    const int64_t ci = (int64_t)v * gridDim.x + blockIdx.x;
    chunk_less[ci] = less;
    chunk_eq[ci] = eq;
    if (blockIdx.x == 0) sel[v] = FrameSel{t, r, keep_all ? 1 : 0, 0};
  }
}

// one workgroup per frame: the first slot and the first tie rank of every chunk; counts and status
__global__ __launch_bounds__(kThreads) void fr_scan_kernel(const FrameSel* __restrict__ sel, const int32_t* __restrict__ chunk_less,
                                                           const int32_t* __restrict__ chunk_eq, int nchunk,
                                                           int32_t* __restrict__ chunk_base, int32_t* __restrict__ chunk_eqbase,
                                                           int32_t* __restrict__ counts, int32_t* __restrict__ status) {
  __shared__ int wsum[kWaves];
  const int v = blockIdx.x, tid = threadIdx.x;
  const int r = sel[v].r;
  int eq_run = 0, run = 0;
  for (int c0 = 0; c0 < nchunk; c0 += kThreads) {
    const int c = c0 + tid;
    const int64_t ci = (int64_t)v * nchunk + c;
    const int less = c < nchunk ? chunk_less[ci] : 0, eq = c < nchunk ? chunk_eq[ci] : 0;
    int eq_total, total;
    const int eq_before = eq_run + block_scan<kWaves>(eq, wsum, &eq_total) - eq;
    const int kept = less + min(max(r - eq_before, 0), eq);
    const int before = run + block_scan<kWaves>(kept, wsum, &total) - kept;
    if (c < nchunk) {
      chunk_eqbase[ci] = eq_before;
      chunk_base[ci] = before;
    }
    eq_run += eq_total;
    run += total;
  }
  if (tid == 0) {
    counts[v] = run;
    status[v] = run > 0 ? GPN_CLOUD_OK : GPN_CLOUD_EMPTY;
  }
}

// ---- 3. ordered compaction: one workgroup per chunk; slots by wave ballots -------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fr_compact_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ valid,
                                                              const uint32_t* __restrict__ seeds, int64_t HW, int hash_bits,
                                                              const FrameSel* __restrict__ sel, const int32_t* __restrict__ chunk_base,
                                                              const int32_t* __restrict__ chunk_eqbase, int64_t n_bound,
                                                              float4* __restrict__ packed, int32_t* __restrict__ pix) {
  __shared__ int wcnt[kPer][kWaves];
  const int v = blockIdx.y, tid = threadIdx.x;
  const FrameSel s = sel[v];
  const int64_t ci = (int64_t)v * gridDim.x + blockIdx.x;
  const uint32_t seed = seeds[v];
  bool lessf[kPer], eqf[kPer], keptf[kPer];
  int rank[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
    const bool ok = p < HW && valid[(int64_t)v * HW + p] != 0;
    const uint32_t hq = hash_key(seed, (uint32_t)p, hash_bits);
    lessf[e] = ok && (s.keep_all || hq < s.t);
    eqf[e] = ok && !s.keep_all && hq == s.t;
  }
  // (slots in pixel order: e first, then the wave, then the lane - ordered_ranks, point_prims.h)
  ordered_ranks<kWaves, kPer>(eqf, wcnt, chunk_eqbase[ci], rank);
#pragma unroll
  for (int e = 0; e < kPer; ++e) keptf[e] = lessf[e] || (eqf[e] && rank[e] < s.r);
  ordered_ranks<kWaves, kPer>(keptf, wcnt, chunk_base[ci], rank);
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int64_t pos = rank[e];
    if (keptf[e] && pos < n_bound) {
      const int64_t p = (int64_t)blockIdx.x * kChunk + e * kThreads + tid;
      const float* q = rows + ((int64_t)v * HW + p) * 6;
      packed[(int64_t)v * n_bound + pos] = make_float4(q[0], q[1], q[2], 1e10f);
      pix[(int64_t)v * HW + pos] = (int)p;
    }
  }
}

struct FrameWs {
  uint32_t* hist;
  FrameSel* sel;
  int32_t *less, *eq, *base, *eqbase;
};
inline size_t frame_ws_bytes(int V, int64_t nchunk) {
  return gpn::align_up((size_t)V * kPasses * kBins * sizeof(uint32_t)) + gpn::align_up((size_t)V * sizeof(FrameSel)) +
         4 * gpn::align_up((size_t)V * nchunk * sizeof(int32_t));
}

}  // namespace

extern "C" int gpn_frame_backproject(const void* depth, int depth_kind, double depth_scale, const uint8_t* rgb, const uint8_t* keep,
                                     const double* K, int V, int H, int W, int flip, float* rows, uint8_t* valid,
                                     int32_t* valid_counts, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(V >= 0 && V <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W < (int64_t)0x7fffffff - kChunk);
  GPN_CHECK_ARG(depth_kind == GPN_FRAME_DEPTH_F32 || depth_kind == GPN_FRAME_DEPTH_F64 || depth_kind == GPN_FRAME_DEPTH_U16);
  GPN_CHECK_ARG(depth_scale > 0.0 && depth_scale < (double)INFINITY);
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(depth && rgb && K && rows && valid && valid_counts);
  GPN_CHECK_HIP(hipMemsetAsync(valid_counts, 0, (size_t)V * sizeof(int32_t), stream));
  const dim3 grid((unsigned)gpn::cdiv((int64_t)H * W, kChunk), (unsigned)V);
  if (depth_kind == GPN_FRAME_DEPTH_F32)
    hipLaunchKernelGGL(fr_backproject_kernel<float>, grid, dim3(kThreads), 0, stream, (const float*)depth, depth_scale, rgb, keep, K, H,
                       W, flip, rows, valid, valid_counts);
  else if (depth_kind == GPN_FRAME_DEPTH_F64)
    hipLaunchKernelGGL(fr_backproject_kernel<double>, grid, dim3(kThreads), 0, stream, (const double*)depth, depth_scale, rgb, keep, K,
                       H, W, flip, rows, valid, valid_counts);
  else
    hipLaunchKernelGGL(fr_backproject_kernel<uint16_t>, grid, dim3(kThreads), 0, stream, (const uint16_t*)depth, depth_scale, rgb, keep,
                       K, H, W, flip, rows, valid, valid_counts);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" size_t gpn_frame_select_ws_bytes(int V, int H, int W) {
  if (V <= 0 || H <= 0 || W <= 0) return 0;
  return frame_ws_bytes(V, gpn::cdiv((int64_t)H * W, kChunk));
}

extern "C" int gpn_frame_select(const float* rows, const uint8_t* valid, const int32_t* valid_counts, const uint32_t* seeds, int V,
                                int H, int W, int cap, int hash_bits, int64_t n_bound, float* packed, int32_t* pix, int32_t* counts,
                                int32_t* status, void* ws, size_t ws_bytes, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(V >= 0 && V <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W < (int64_t)0x7fffffff - kChunk);
  const int64_t HW = (int64_t)H * W;
  GPN_CHECK_ARG(cap >= 0 && hash_bits >= 1 && hash_bits <= 32 && n_bound == (cap > 0 ? (int64_t)cap : HW));
  if (V == 0) return GPN_OK;
  GPN_CHECK_ARG(rows && valid && valid_counts && seeds && packed && pix && counts && status);
  const int64_t nchunk = gpn::cdiv(HW, kChunk);
  gpn::WsCarver carve(ws, ws_bytes);
  FrameWs f;
  f.hist = carve.take<uint32_t>((size_t)V * kPasses * kBins);
  f.sel = carve.take<FrameSel>((size_t)V);
  f.less = carve.take<int32_t>((size_t)V * nchunk);
  f.eq = carve.take<int32_t>((size_t)V * nchunk);
  f.base = carve.take<int32_t>((size_t)V * nchunk);
  f.eqbase = carve.take<int32_t>((size_t)V * nchunk);
  GPN_CHECK_WS(carve);
  const dim3 grid((unsigned)nchunk, (unsigned)V);
  if (cap > 0) {
    GPN_CHECK_HIP(hipMemsetAsync(f.hist, 0, (size_t)V * kPasses * kBins * sizeof(uint32_t), stream));
    for (int pass = 0; pass < kPasses; ++pass) {
      hipLaunchKernelGGL(fr_hist_kernel, grid, dim3(kThreads), 0, stream, valid, valid_counts, seeds, HW, cap, hash_bits, pass, f.hist);
      GPN_CHECK_LAUNCH();
    }
  }
  hipLaunchKernelGGL(fr_count_kernel, grid, dim3(kThreads), 0, stream, valid, valid_counts, seeds, HW, cap, hash_bits, f.hist, f.sel,
                     f.less, f.eq);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(fr_scan_kernel, dim3(V), dim3(kThreads), 0, stream, f.sel, f.less, f.eq, (int)nchunk, f.base, f.eqbase, counts,
                     status);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(fr_compact_kernel, grid, dim3(kThreads), 0, stream, rows, valid, seeds, HW, hash_bits, f.sel, f.base, f.eqbase,
                     n_bound, reinterpret_cast<float4*>(packed), pix);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
