// pointmlp.hip — the dense point-MLP layers of the PointNet backbone on the fp32 MFMA (include/gpn.h section PM).
//
// Reference: network/pointnet/pointnet_utils.py:10-133, pointnet_sem_seg.py:8-30 — Conv1d(k = 1) / Linear layers of widths
// 6 .. 1088 over B x N points, two torch.bmm with per-scene 3 x 3 / 64 x 64 transforms, and three 1024-wide layers that exist
// only to be max-pooled over a scene's points.  One LDS-tiled GEMM kernel covers all of them:
//
//   Y[r, :] = epi( X~[r, :] . W_s(r)^T + b + G[s(r), :] ),   M[s, :] = max over the rows of segment s of the same values
//
//   * rows belong to contiguous segments (scenes); a row tile never crosses a segment boundary, so one tile has one weight
//     matrix (the bmm form, W [S, cout, cin]), one G row (the scene-constant half of the 1088-wide concatenation) and one
//     row of M.  Tiles find their segment by a scan over the S + 1 offsets (S is a batch size).
//   * X~ is row-major [N, cin] or a strided view (segment, channel, point) -> base + b sb + c sc + n sn: the first layer
//     reads the batch's point array in either input layout without a transposing copy.
//   * Y == NULL: only M is produced - the 1024-wide activations of an inference pass never reach memory.
//   * M is an integer atomicMax over an order-preserving encoding of the floats (max is order-independent: deterministic),
//     initialised and decoded in place by two one-line launches.  No float atomics anywhere.
//   * dgrad is the same kernel on host-transposed weights.  wgrad (dW = dY^T X~, db = column sums of dY) is a second MFMA
//     kernel: per-workgroup partials over fixed row chunks (cut at segment boundaries), summed in chunk order.
//
// Tile: 128 rows x 128 (or 32) columns per workgroup of four waves, K in steps of 16 through LDS with the next step's global
// loads in flight.  Each wave holds 4 x 4 (2 x 2) accumulator tiles of v_mfma_f32_16x16x4_f32 - 16 (4) independent chains: a
// dependent 16x16x4_f32 issues after 40 cycles, an independent one after 32.  An LDS row is 16 + 4 floats: lane (i, q) reads
// the 16 bytes k = 4q .. 4q + 3 of row i with one ds_read_b128 (conflict-free at this pitch) and feeds element j to the j-th
// MFMA of the step; A and B use the same k assignment, so each MFMA sums four matching products.
#include "gpn_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kBM = 128;         // rows of a forward tile
constexpr int kBK = 16;          // K per LDS stage
constexpr int kPitch = kBK + 4;  // floats per LDS row of the forward tiles
constexpr int kMaxSegments = 4096;
constexpr int kMaxCin = 4096, kMaxCout = 8192;
// wgrad: 64 x 64 output tile, 16 rows per LDS stage, row-major stages of pitch 64 + 16 (lane groups 16 banks apart)
constexpr int kWT = 64, kWK = 16, kWPitch = kWT + 16;

struct XView {  // X~: row-major [N, cin] (strided == 0) or base + b sb + c sc + n sn
  const float* p;
  int strided;
  int64_t sb, sc, sn;
};

struct Seg {
  int s;
  int64_t begin;   // first row of the segment
  int64_t r0, r1;  // rows of this tile / chunk
};

// the t-th tile of `step` rows when every segment is cut into its own tiles; false past the last one.  Offsets are clamped to
// [0, N]: a malformed device array cannot send a row index out of the buffers
__device__ __forceinline__ bool find_tile(const int64_t* __restrict__ off, int S, int64_t N, int64_t t, int step, Seg& g) {
  if (!off) {
    g.s = 0, g.begin = 0, g.r0 = t * step, g.r1 = g.r0 + step < N ? g.r0 + step : N;
    return g.r0 < N;
  }
  for (int s = 0; s < S; ++s) {
    int64_t b = off[s], e = off[s + 1];
    b = b < 0 ? 0 : (b > N ? N : b);
    e = e < b ? b : (e > N ? N : e);
    const int64_t nt = (e - b + step - 1) / step;
    if (t < nt) {
      g.s = s, g.begin = b, g.r0 = b + t * step, g.r1 = g.r0 + step < e ? g.r0 + step : e;
      return true;
    }
    t -= nt;
  }
  return false;
}

struct FwdArgs {
  XView x;
  const float* W;
  int64_t w_seg;  // floats between two segments' weights (0: shared)
  const float *b, *G, *ea, *ed;
  int relu;
  const int64_t* off;
  int S;
  int64_t N;
  int cin, cout;
  int vec_a, vec_b;  // 16-byte loads allowed
  float* Y;
  int* M;
};

// 16 bytes k .. k + 3 of row `row` (tile-local) of X~; zero past the tile's rows and past cin
__device__ __forceinline__ f32x4 load_a(const FwdArgs& a, const Seg& g, int rows, int row, int k) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row >= rows || k >= a.cin) return v;
  if (a.vec_a) return *reinterpret_cast<const f32x4*>(a.x.p + (g.r0 + row) * a.cin + k);
  const float* p;
  int64_t st;
  if (a.x.strided) {
    p = a.x.p + g.s * a.x.sb + (int64_t)k * a.x.sc + (g.r0 - g.begin + row) * a.x.sn, st = a.x.sc;
  } else {
    p = a.x.p + (g.r0 + row) * a.cin + k, st = 1;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (k + u < a.cin) v[u] = p[u * st];
  return v;
}

__device__ __forceinline__ f32x4 load_b(const FwdArgs& a, const float* __restrict__ W, int col, int k) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (col >= a.cout || k >= a.cin) return v;
  const float* p = W + (int64_t)col * a.cin + k;
  if (a.vec_b) return *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (k + u < a.cin) v[u] = p[u];
  return v;
}

template <int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(kThreads) void pointmlp_fwd_kernel(const FwdArgs a) {
  constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
  static_assert(WM * WN == 4 && BM == kBM, "four waves, 128 rows");
  constexpr int LA = BM * 4 / kThreads;                        // 16-byte loads of A per thread and stage
  constexpr int LB = (BN * 4 + kThreads - 1) / kThreads;       // of B (BN = 32: the first 128 threads, one each)
  __shared__ __attribute__((aligned(16))) float As[BM * kPitch];
  __shared__ __attribute__((aligned(16))) float Bs[BN * kPitch];

  Seg g;
  if (!find_tile(a.off, a.S, a.N, blockIdx.x, BM, g)) return;  // (uniform over the workgroup)
  const int rows = (int)(g.r1 - g.r0);
  const int n0 = blockIdx.y * BN;
  const float* __restrict__ W = a.W + g.s * a.w_seg;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, q = lane >> 4;
  const int wm = wave / WN, wn = wave % WN;

  f32x4 acc[TM][TN];
#pragma unroll
  for (int t = 0; t < TM; ++t)
#pragma unroll
    for (int n = 0; n < TN; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 ra[LA], rb[LB];
#pragma unroll
  for (int u = 0; u < LA; ++u) ra[u] = load_a(a, g, rows, (tid + u * kThreads) >> 2, ((tid + u * kThreads) & 3) * 4);
#pragma unroll
  for (int u = 0; u < LB; ++u) {
    const int e = tid + u * kThreads;
    if (e < BN * 4) rb[u] = load_b(a, W, n0 + (e >> 2), (e & 3) * 4);
  }
  for (int k0 = 0; k0 < a.cin; k0 += kBK) {
    __syncthreads();  // the previous stage's reads are done
#pragma unroll
    for (int u = 0; u < LA; ++u) {
      const int e = tid + u * kThreads;
      *reinterpret_cast<f32x4*>(&As[(e >> 2) * kPitch + (e & 3) * 4]) = ra[u];
    }
#pragma unroll
    for (int u = 0; u < LB; ++u) {
      const int e = tid + u * kThreads;
      if (e < BN * 4) *reinterpret_cast<f32x4*>(&Bs[(e >> 2) * kPitch + (e & 3) * 4]) = rb[u];
    }
    __syncthreads();
    if (k0 + kBK < a.cin) {  // the next stage's loads fly under this stage's MFMAs
#pragma unroll
      for (int u = 0; u < LA; ++u)
        ra[u] = load_a(a, g, rows, (tid + u * kThreads) >> 2, k0 + kBK + ((tid + u * kThreads) & 3) * 4);
#pragma unroll
      for (int u = 0; u < LB; ++u) {
        const int e = tid + u * kThreads;
        if (e < BN * 4) rb[u] = load_b(a, W, n0 + (e >> 2), k0 + kBK + (e & 3) * 4);
      }
    }
    f32x4 fa[TM], fb[TN];
#pragma unroll
    for (int t = 0; t < TM; ++t) fa[t] = *reinterpret_cast<const f32x4*>(&As[((wm * TM + t) * 16 + i16) * kPitch + q * 4]);
#pragma unroll
    for (int n = 0; n < TN; ++n) fb[n] = *reinterpret_cast<const f32x4*>(&Bs[((wn * TN + n) * 16 + i16) * kPitch + q * 4]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int n = 0; n < TN; ++n) acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t][j], fb[n][j], acc[t][n], 0, 0, 0);
  }

  // epilogue: lane (i16, q) holds rows 4 q + v of each 16 x 16 tile at column i16
#pragma unroll
  for (int n = 0; n < TN; ++n) {
    const int col = n0 + (wn * TN + n) * 16 + i16;
    const bool col_ok = col < a.cout;
    float add = 0.f, ea = 1.f, ed = 0.f;
    if (col_ok) {
      if (a.b) add = a.b[col];
      if (a.G) add += a.G[(int64_t)g.s * a.cout + col];
      if (a.ea) ea = a.ea[col], ed = a.ed[col];
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = (wm * TM + t) * 16 + 4 * q + v;
        float y = acc[t][n][v] + add;
        if (a.ea) y = ea * y + ed;
        if (a.relu) y = y > 0.f ? y : 0.f;
        if (row < rows && col_ok) {
          if (a.Y) a.Y[(g.r0 + row) * a.cout + col] = y;
          mx = y > mx ? y : mx;
        }
      }
    if (a.M) {
      float o = __shfl_xor(mx, 16);
      mx = o > mx ? o : mx;
      o = __shfl_xor(mx, 32);
      mx = o > mx ? o : mx;
      if (q == 0 && col_ok && mx > -INFINITY) atomicMax(&a.M[(int64_t)g.s * a.cout + col], gpn::float_order(mx));
    }
  }
}

__global__ void max_init_kernel(int* __restrict__ M, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) M[e] = gpn::float_order(-INFINITY);
}
__global__ void max_decode_kernel(int* __restrict__ M, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) M[e] = __float_as_int(gpn::order_float(M[e]));  // (M now holds the floats' bits)
}

// ---- wgrad -------------------------------------------------------------------------------------------------------------------
struct WgArgs {
  XView x;
  const float* dy;
  const int64_t* off;
  int S;
  int64_t N;
  int cin, cout, chunk_rows;
  int vec_x, vec_d;
  float* partial;  // [chunks][cout cin + cout]
};

// partial[chunk][o][c] = sum over the chunk's rows of dy[r, o] x~[r, c] (blockIdx = (chunk, cout tile, cin tile)); the workgroups of
// cin tile 0 also write the column sums of dy, rows ascending
__global__ __launch_bounds__(kThreads) void pointmlp_wgrad_kernel(const WgArgs a) {
  __shared__ __attribute__((aligned(16))) float Ds[kWK * kWPitch];  // [row][o]
  __shared__ __attribute__((aligned(16))) float Xs[kWK * kWPitch];  // [row][c]
  Seg g;
  if (!find_tile(a.off, a.S, a.N, blockIdx.x, a.chunk_rows, g)) return;
  const int rows = (int)(g.r1 - g.r0);
  const int o0 = blockIdx.y * kWT, c0 = blockIdx.z * kWT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i16 = lane & 15, q = lane >> 4;
  const int wo = wave >> 1, wc = wave & 1;  // 2 x 2 waves of 32 x 32
  const int lr = tid >> 4, lc = (tid & 15) * 4;  // this thread's 16 bytes of a stage: row lr, columns lc .. lc + 3

  auto load_d = [&](int r) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int o = o0 + lc;
    if (r + lr >= rows || o >= a.cout) return v;
    const float* p = a.dy + (g.r0 + r + lr) * a.cout + o;
    if (a.vec_d) return *reinterpret_cast<const f32x4*>(p);  // (cout % 4 == 0: o + 3 < cout)
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (o + u < a.cout) v[u] = p[u];
    return v;
  };
  auto load_x = [&](int r) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int c = c0 + lc;
    if (r + lr >= rows || c >= a.cin) return v;
    if (a.vec_x) return *reinterpret_cast<const f32x4*>(a.x.p + (g.r0 + r + lr) * a.cin + c);
    const float* p;
    int64_t st;
    if (a.x.strided) {
      p = a.x.p + g.s * a.x.sb + (int64_t)c * a.x.sc + (g.r0 - g.begin + r + lr) * a.x.sn, st = a.x.sc;
    } else {
      p = a.x.p + (g.r0 + r + lr) * a.cin + c, st = 1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (c + u < a.cin) v[u] = p[u * st];
    return v;
  };

  f32x4 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  f32x4 rd = load_d(0), rx = load_x(0);
  for (int r = 0; r < rows; r += kWK) {
    __syncthreads();
    *reinterpret_cast<f32x4*>(&Ds[lr * kWPitch + lc]) = rd;
    *reinterpret_cast<f32x4*>(&Xs[lr * kWPitch + lc]) = rx;
    __syncthreads();
    if (r + kWK < rows) rd = load_d(r + kWK), rx = load_x(r + kWK);
    if (blockIdx.z == 0 && tid < kWT) {
#pragma unroll
      for (int k = 0; k < kWK; ++k) bsum += Ds[k * kWPitch + tid];
    }
#pragma unroll
    for (int ks = 0; ks < kWK / 4; ++ks) {
      float fa[2], fb[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) fa[t] = Ds[(ks * 4 + q) * kWPitch + (wo * 2 + t) * 16 + i16];
#pragma unroll
      for (int n = 0; n < 2; ++n) fb[n] = Xs[(ks * 4 + q) * kWPitch + (wc * 2 + n) * 16 + i16];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t], fb[n], acc[t][n], 0, 0, 0);
    }
  }
  const int64_t per = (int64_t)a.cout * a.cin + a.cout;
  float* __restrict__ out = a.partial + (int64_t)blockIdx.x * per;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int o = o0 + (wo * 2 + t) * 16 + 4 * q + v, c = c0 + (wc * 2 + n) * 16 + i16;
        if (o < a.cout && c < a.cin) out[(int64_t)o * a.cin + c] = acc[t][n][v];
      }
  if (blockIdx.z == 0 && tid < kWT && o0 + tid < a.cout) out[(int64_t)a.cout * a.cin + o0 + tid] = bsum;
}

// dW[s][e] = the partials of segment s's chunks (all chunks for shared weights) added in chunk order, four interleaved running
// sums combined in a fixed order; db = the column sums over all chunks
__global__ __launch_bounds__(kThreads) void pointmlp_wgrad_sum_kernel(const float* __restrict__ partial, const int64_t* __restrict__ off,
                                                                      int S, int64_t N, int chunk_rows, int cin, int cout,
                                                                      int per_segment, float* __restrict__ dW, float* __restrict__ db) {
  const int64_t wsz = (int64_t)cout * cin, per = wsz + cout;
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= per) return;
  const int s = blockIdx.y;  // segment (0 for shared weights)
  if (e >= wsz && (s != 0 || !db)) return;
  if (e < wsz && !dW) return;
  int64_t c_begin = 0, c_end = 0;
  if (!off) {
    c_end = (N + chunk_rows - 1) / chunk_rows;
  } else {
    for (int t = 0; t < S; ++t) {
      int64_t b = off[t], en = off[t + 1];
      b = b < 0 ? 0 : (b > N ? N : b);
      en = en < b ? b : (en > N ? N : en);
      const int64_t nt = (en - b + chunk_rows - 1) / chunk_rows;
      if (per_segment && e < wsz) {
        if (t < s) c_begin += nt;
        if (t <= s) c_end += nt;
      } else {
        c_end += nt;
      }
    }
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int64_t c = c_begin;
  for (; c + 3 < c_end; c += 4) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = partial[(c + u) * per + e];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] += v[u];
  }
  for (int u = 0; c < c_end; ++c, ++u) acc[u] += partial[c * per + e];
  const float r = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  if (e < wsz) dW[(per_segment ? (int64_t)s * wsz : 0) + e] = r;
  else db[e - wsz] = r;
}

bool widths_ok(int cin, int cout) { return cin >= 1 && cin <= kMaxCin && cout >= 1 && cout <= kMaxCout; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// a host copy of the offsets, when the caller has one: 0 = off[0] < off[1] < ... < off[S] = N
bool host_offsets_ok(const int64_t* h, int64_t S, int64_t N) {
  if (h[0] != 0 || h[S] != N) return false;
  for (int64_t s = 0; s < S; ++s)
    if (h[s + 1] <= h[s]) return false;
  return true;
}

int wgrad_chunk_rows(int cin, int cout) { return (int64_t)cin * cout >= 65536 ? 2048 : 512; }
int64_t wgrad_chunks(int64_t N, int64_t S, int cin, int cout) {
  return gpn::cdiv(N > 0 ? N : 1, wgrad_chunk_rows(cin, cout)) + (S > 1 ? S - 1 : 0);
}

}  // namespace

extern "C" int gpn_pointmlp_supported(int cin, int cout) { return widths_ok(cin, cout) ? 1 : 0; }

extern "C" int gpn_pointmlp_fwd(const float* x, int strided, int64_t sb, int64_t sc, int64_t sn, const float* W, int per_segment,
                                const float* b, const float* G, const float* epi_scale, const float* epi_shift, int relu,
                                const int64_t* offsets, const int64_t* offsets_host, int64_t S, int64_t N, int cin, int cout,
                                float* Y, float* M, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(widths_ok(cin, cout));
  GPN_CHECK_ARG(N >= 0 && S >= 1 && S <= kMaxSegments);
  if (N == 0) return GPN_OK;
  GPN_CHECK_ARG(S <= N);  // (no empty segments)
  GPN_CHECK_ARG(x && W && (Y || M));
  GPN_CHECK_ARG(offsets || S == 1);
  GPN_CHECK_ARG((epi_scale == nullptr) == (epi_shift == nullptr));
  GPN_CHECK_ARG(!offsets_host || host_offsets_ok(offsets_host, S, N));
  FwdArgs a;
  a.x = XView{x, strided ? 1 : 0, sb, sc, sn};
  a.W = W, a.w_seg = per_segment ? (int64_t)cout * cin : 0;
  a.b = b, a.G = G, a.ea = epi_scale, a.ed = epi_shift, a.relu = relu ? 1 : 0;
  a.off = offsets, a.S = (int)S, a.N = N, a.cin = cin, a.cout = cout;
  a.vec_a = !strided && cin % 4 == 0 && aligned16(x);
  a.vec_b = cin % 4 == 0 && aligned16(W);
  a.Y = Y, a.M = reinterpret_cast<int*>(M);
  const int64_t tiles = gpn::cdiv(N, kBM) + (S - 1);  // every segment boundary can add one partly filled tile
  const double rd = 4.0 * ((double)N * cin + (double)(per_segment ? S : 1) * cin * cout);
  gpn::ProfScope prof(GPN_K_POINTMLP, stream, 2.0 * (double)N * cin * cout, rd + (Y ? 4.0 * (double)N * cout : 0.0) + (M ? 4.0 * S * cout : 0.0));
  const int64_t mn = S * (int64_t)cout;
  if (M) {
    hipLaunchKernelGGL(max_init_kernel, dim3((unsigned)gpn::cdiv(mn, kThreads)), dim3(kThreads), 0, stream, a.M, mn);
    GPN_CHECK_LAUNCH();
  }
  if (cout <= 64) {
    hipLaunchKernelGGL((pointmlp_fwd_kernel<4, 1, 2, 2>), dim3((unsigned)tiles, (unsigned)gpn::cdiv(cout, 32)), dim3(kThreads), 0, stream, a);
  } else {
    hipLaunchKernelGGL((pointmlp_fwd_kernel<2, 2, 4, 4>), dim3((unsigned)tiles, (unsigned)gpn::cdiv(cout, 128)), dim3(kThreads), 0, stream, a);
  }
  GPN_CHECK_LAUNCH();
  if (M) {
    hipLaunchKernelGGL(max_decode_kernel, dim3((unsigned)gpn::cdiv(mn, kThreads)), dim3(kThreads), 0, stream, a.M, mn);
    GPN_CHECK_LAUNCH();
  }
  return GPN_OK;
}

extern "C" size_t gpn_pointmlp_wgrad_ws_bytes(int64_t N, int64_t S, int cin, int cout) {
  if (!widths_ok(cin, cout)) return 0;
  return gpn::align_up((size_t)wgrad_chunks(N, S, cin, cout) * ((size_t)cout * cin + cout) * sizeof(float));
}

extern "C" int gpn_pointmlp_wgrad(const float* x, int strided, int64_t sb, int64_t sc, int64_t sn, const float* dy,
                                  const int64_t* offsets, const int64_t* offsets_host, int64_t S, int64_t N, int cin, int cout,
                                  int per_segment, float* dW, float* db, void* ws, size_t ws_bytes, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(widths_ok(cin, cout));
  GPN_CHECK_ARG(N >= 0 && S >= 1 && S <= kMaxSegments);
  GPN_CHECK_ARG(dW || db);
  const size_t wsz = (size_t)cout * cin;
  if (N == 0) {
    if (dW) GPN_CHECK_HIP(hipMemsetAsync(dW, 0, sizeof(float) * wsz * (per_segment ? S : 1), stream));
    if (db) GPN_CHECK_HIP(hipMemsetAsync(db, 0, sizeof(float) * (size_t)cout, stream));
    return GPN_OK;
  }
  GPN_CHECK_ARG(S <= N);
  GPN_CHECK_ARG(x && dy);
  GPN_CHECK_ARG(offsets || S == 1);
  GPN_CHECK_ARG(!offsets_host || host_offsets_ok(offsets_host, S, N));
  const int64_t chunks = wgrad_chunks(N, S, cin, cout);
  if (!ws || ws_bytes < (size_t)chunks * (wsz + cout) * sizeof(float)) {
    gpn::set_error("gpn_pointmlp_wgrad: workspace too small");
    return GPN_ERR_WS;
  }
  WgArgs a;
  a.x = XView{x, strided ? 1 : 0, sb, sc, sn};
  a.dy = dy, a.off = offsets, a.S = (int)S, a.N = N, a.cin = cin, a.cout = cout, a.chunk_rows = wgrad_chunk_rows(cin, cout);
  a.vec_x = !strided && cin % 4 == 0 && aligned16(x);
  a.vec_d = cout % 4 == 0 && aligned16(dy);
  a.partial = static_cast<float*>(ws);
  gpn::ProfScope prof(GPN_K_POINTMLP, stream, 2.0 * (double)N * cin * cout, 4.0 * ((double)N * (cin + cout) + 2.0 * (double)chunks * (wsz + cout)));
  hipLaunchKernelGGL(pointmlp_wgrad_kernel, dim3((unsigned)chunks, (unsigned)gpn::cdiv(cout, kWT), (unsigned)gpn::cdiv(cin, kWT)), dim3(kThreads),
                     0, stream, a);
  GPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(pointmlp_wgrad_sum_kernel, dim3((unsigned)gpn::cdiv((int64_t)(wsz + cout), kThreads), (unsigned)(per_segment ? S : 1)),
                     dim3(kThreads), 0, stream, (const float*)a.partial, offsets, (int)S, N, a.chunk_rows, cin, cout, per_segment ? 1 : 0, dW, db);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
