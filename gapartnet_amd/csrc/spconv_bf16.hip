// spconv_bf16.hip — the reduced-precision INFERENCE sparse convolution for gfx950 (include/gpn.h section C16): bf16 activations,
// bf16 pre-packed weights, fp32 accumulators, fused BatchNorm / residual / ReLU epilogue, one rounding per stored activation.
// Forward only, off by default; nothing of the fp32 path runs through this file.
//
// Work mapping (what the masked-tile kernel of spconv_tiles.hip learned, one kernel family for every level):
//   * output-stationary: MFMA row i of a 16-row tile IS destination row i for every tap; a wave owns one row tile and NT (1..7)
//     column tiles - the widest divisor of the layer's column tiles, whatever the row count - so every output row is written
//     once by one wave: no partial sums, no atomics, no workspace.
//   * prologue, once per wave: the wave's column of the neighbour table for all K taps with a handful of coalesced loads in
//     flight together, a ballot per tap, and the byte offsets of the LIVE taps' source rows compacted into a per-wave LDS slab.
//   * tap loop over the live taps only (a tap no row of the tile has costs nothing): the gathered row pieces of the next tap are
//     requested while the current tap is in the MFMAs (two operand slots with compile-time indices).  An absent neighbour reads at
//     an out-of-range buffer offset: zeros, no memory access.
//   * operands: with v_mfma_f32_16x16x32_bf16 a lane's A fragment of a 32-channel block is 8 consecutive bf16 of one row = ONE
//     16-byte load from the gathered row, no shuffle; the odd 16-channel block of the widths 16, 48, 80, 112 goes through
//     v_mfma_f32_16x16x16_bf16 (4 bf16 = 8 bytes per lane) instead of padding K with zeros.
// Packed weight layout (gpn_spconv_pack_weights_bf16), per tap k cin*cout bf16:
//   full 32-channel blocks b < cin/32:  [b][nt][lane][j < 8] = W[k][32 b + 8 (lane >> 4) + j][16 nt + (lane & 15)]
//   then the odd 16-channel block:      [nt][lane][j < 4]    = W[k][32 (cin/32) + 4 (lane >> 4) + j][16 nt + (lane & 15)]
// Summation order per output element, FIXED: the 32-channel blocks of all taps are ONE fp32 accumulation chain (ascending tap,
// within a tap ascending block, inside a block whatever the MFMA does), the odd 16-channel block of all taps a SECOND chain
// (ascending tap), and the result is chain32 + chain16 in fp32 (a width without 32-channel blocks, or without an odd block, has
// one chain: 0 + x = x).  Two chains because each then holds ONE MFMA opcode: v_mfma_f32_16x16x16_bf16 accumulating onto the
// result of a v_mfma_f32_16x16x32_bf16 issued right before it (one column tile per wave, k = 1: nothing in between) gave wrong
// rows on the MI355X - in 2 to 400 of 400 back-to-back launches, by shape; with one opcode per chain 0 of 400.  A product of two
// bf16 values is exact in fp32, so fp32 accumulation is the only error before the store.  Taps a row does not have contribute
// exact zeros (x + 0 = x), and a column tile's sums do not depend on which other column tiles share its wave: the result of a
// row does not depend on the tile order or on the instantiation, and a launch is deterministic.
// Epilogue per output element, in fp32, the arithmetic of gpn::affine_apply: v = (acc - mean) * (1 / sqrtf(var + eps)) * weight
// + bias, then + res (bf16, widened exactly), then max(0, .), each optional; then ONE round-to-nearest-even to bf16 - or none,
// when the caller asks for the fp32 output.
#include <algorithm>
#include <type_traits>

#include "spconv_dispatch.h"  // (the instantiation lists)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
constexpr int kMaxTaps = 27;
constexpr int kThreads = 256;

// fp32 -> bf16, round to nearest even (NaN stays a quiet NaN); bf16 -> fp32 is exact
__device__ __forceinline__ uint16_t bf16_rne(float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf16_widen(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }

struct Bf16ConvArgs {
  const uint16_t* in;
  const uint16_t* packed;
  const int32_t* nbr;
  const int32_t* perm;
  void* out;
  int64_t n_dst;
  int K, n_tiles, n_units, nt_total, col_groups;
  uint32_t packed_bytes;
  gpn_conv_epilogue_bf16_t ep;
};

// CB = cin / 16, NT = column tiles of a wave
template <int CB, int NT>
__global__ __launch_bounds__(kThreads) void spconv_bf16_kernel(const Bf16ConvArgs p) {
  constexpr int NB2 = CB / 2;    // full 32-channel blocks
  constexpr bool TAIL = CB & 1;  // an odd 16-channel block behind them
  constexpr int cin = CB * 16;
  constexpr int TPI = 4;  // taps covered by one table load of the prologue (64 lanes / 16 rows)
  constexpr int NI = (kMaxTaps + TPI - 1) / TPI;
  constexpr uint32_t kOob = 0x80000000u;
  __shared__ uint32_t slab[4][kMaxTaps + 1][16];  // per wave: byte offset of the gathered row (kOob = none) by live-tap slot

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i16 = lane & 15, g = lane >> 4;
  // workgroups are dealt round-robin to the 8 XCDs: every XCD takes one contiguous eighth of the units (the rows its waves
  // gather are fetched into one L2)
  const int wg = (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
  const int unit = __builtin_amdgcn_readfirstlane(wg * 4 + wave);
  if (unit >= p.n_units) return;  // whole wave; no barrier in this kernel
  const int tile = unit / p.col_groups;
  const int nt0 = (unit - tile * p.col_groups) * NT;
  const int nt_total = p.nt_total;
  const int cout = nt_total * 16;
  const int64_t n_dst = p.n_dst;
  const int K = p.K;

  const __amdgpu_buffer_rsrc_t in_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.in), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t nbr_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(p.nbr), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.packed), 0, (int)p.packed_bytes, 0x00020000);
  const uint32_t col_bytes = (uint32_t)n_dst * 4u;

  int32_t orow[4];  // destination rows of this lane's four accumulator rows
  if (p.perm) {
    const int4 pv = *reinterpret_cast<const int4*>(p.perm + (int64_t)tile * 16 + 4 * g);
    orow[0] = pv.x, orow[1] = pv.y, orow[2] = pv.z, orow[3] = pv.w;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) orow[r] = tile * 16 + 4 * g + r;
  }

  // ---- prologue: table column of the wave's rows, all taps; live taps; compacted offsets into the slab ----------------------
  const int lr = lane & 15, lt = lane >> 4;
  const int64_t pos = (int64_t)tile * 16 + lr;
  const bool row_ok = pos < n_dst;
  const uint32_t tvoff = (uint32_t)(row_ok ? pos : n_dst - 1) * 4u;
  int32_t raw[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int tap = i * TPI + lt;
    const int tc = tap < K ? tap : 0;  // (lanes past the last tap re-read tap 0 and are masked below)
    raw[i] = -1;
    if (i * TPI < K)
      raw[i] = __builtin_bit_cast(int32_t, __builtin_amdgcn_raw_buffer_load_b32(nbr_rsrc, (int)(tvoff + (uint32_t)tc * col_bytes), 0, 0));
  }
  uint32_t um = 0;  // bit k = some row of the wave has tap k
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int tap = i * TPI + lt;
    const bool valid = row_ok && tap < K && raw[i] >= 0;
    const uint64_t b = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
    for (int s = 0; s < TPI; ++s)
      if (((b >> (16 * s)) & 0xffffull) != 0 && i * TPI + s < kMaxTaps) um |= 1u << (i * TPI + s);
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int tap = i * TPI + lt;
    const bool valid = row_ok && tap < K && raw[i] >= 0;
    const bool live = tap < kMaxTaps && ((um >> tap) & 1u) != 0u;
    const int slot = __builtin_popcount(um & ((1u << tap) - 1u));
    if (live) slab[wave][slot][lr] = valid ? (uint32_t)raw[i] * (uint32_t)(cin * 2) : kOob;
  }
  int remaining = __builtin_popcount(um);

  f32x4 acc[NT], acct[TAIL ? NT : 1];  // the 32-channel blocks' chain; the odd 16-channel block's chain
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int nt = 0; nt < (TAIL ? NT : 1); ++nt) acct[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- the tap loop: two operand slots for the gathered rows; the weights of a tap come from L2 next to its MFMAs ---------------
  u32x4 ra[2][NB2 > 0 ? NB2 : 1];
  u32x2 rt[2];
  int tap_of[2] = {0, 0};
  int issued = 0;
  const uint32_t tap_bytes = (uint32_t)(cin * cout) * 2u;
  auto issue = [&](auto slot_tag) {
    constexpr int sl = decltype(slot_tag)::value;
    const bool has = um != 0u;
    tap_of[sl] = has ? __builtin_ctz(um) : 0;
    um &= um - 1u;
    const int ls = issued < kMaxTaps ? issued : kMaxTaps;  // (the slab has kMaxTaps + 1 slots)
    issued += 1;
    const uint32_t ao = has ? slab[wave][ls][i16] : kOob;  // (kOob + a row's bytes stays out of range)
#pragma unroll
    for (int b = 0; b < NB2; ++b)
      ra[sl][b] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(in_rsrc, (int)(ao + (uint32_t)g * 16u), b * 64, 0));
    if constexpr (TAIL)
      rt[sl] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(in_rsrc, (int)(ao + (uint32_t)g * 8u), NB2 * 64, 0));
  };
  auto consume = [&](auto slot_tag) {
    constexpr int sl = decltype(slot_tag)::value;
    const uint32_t wbase = (uint32_t)tap_of[sl] * tap_bytes;
#pragma unroll
    for (int b = 0; b < NB2; ++b) {
      u32x4 rb[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        rb[nt] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                               w_rsrc, (int)(wbase + (uint32_t)((b * nt_total + nt0) * 1024 + lane * 16)), nt * 1024, 0));
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ra[sl][b]), __builtin_bit_cast(bf16x8, rb[nt]),
                                                          acc[nt], 0, 0, 0);
    }
    if constexpr (TAIL) {
      u32x2 rb[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        rb[nt] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(
                                               w_rsrc, (int)(wbase + (uint32_t)(NB2 * nt_total * 1024 + nt0 * 512 + lane * 8)), nt * 512, 0));
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acct[nt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(bf16x4, rt[sl]), __builtin_bit_cast(bf16x4, rb[nt]),
                                                             acct[nt], 0, 0, 0);
    }
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  issue(S0());
  while (remaining >= 2) {
    remaining -= 2;
    issue(S1());
    consume(S0());
    issue(S0());
    consume(S1());
  }
  if (remaining) consume(S0());
  if constexpr (TAIL) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] += acct[nt];
  }

  // ---- D[row = 4g + r][col = i16] of every column tile -> epilogue -> out --------------------------------------------------
  const gpn_conv_epilogue_bf16_t& ep = p.ep;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const uint32_t col = (uint32_t)((nt0 + nt) * 16 + i16);
    float mu = 0.f, is = 1.f, w = 1.f, bb = 0.f;
    if (ep.mean) mu = ep.mean[col], is = 1.0f / sqrtf(ep.var[col] + ep.eps), w = ep.weight[col], bb = ep.bias[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if ((int64_t)tile * 16 + 4 * g + r < n_dst) {
        const size_t e = (size_t)orow[r] * (size_t)cout + col;
        float v = acc[nt][r];
        if (ep.mean) v = (v - mu) * is * w + bb;
        if (ep.res) v += bf16_widen(ep.res[e]);
        if (ep.relu) v = v > 0.f ? v : 0.f;
        if (ep.out_f32) static_cast<float*>(p.out)[e] = v;
        else static_cast<uint16_t*>(p.out)[e] = bf16_rne(v);
      }
    }
  }
}

template <int CB, int NT>
int launch_bf16(const Bf16ConvArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)(gpn::cdiv(gpn::cdiv(a.n_units, 4), 8) * 8));
  hipLaunchKernelGGL((spconv_bf16_kernel<CB, NT>), grid, dim3(kThreads), 0, stream, a);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

// (instantiated for the fp32 masked-tile kernel's input widths and column tiles per wave: GPN_CONV_CB x GPN_TILES_NT)
template <int CB>
int dispatch_cols(int NT, const Bf16ConvArgs& a, hipStream_t stream) {
#define GPN_X(nt) if (NT == nt) return launch_bf16<CB, nt>(a, stream);
  GPN_TILES_NT(GPN_X)
#undef GPN_X
  gpn::set_error("gpn_spconv_fwd_bf16: no bf16 kernel for %d column tiles per wave", NT);
  return GPN_ERR_ARG;
}

// column tiles per wave: the widest divisor (<= 7) of the layer's column tiles - a function of the shape alone
int cols_per_wave(int nt_total) {
  for (int d = nt_total < 7 ? nt_total : 7; d > 1; --d)
    if (nt_total % d == 0) return d;
  return 1;
}

// element t of the packed bf16 weight <- (tap, input channel, output channel) of the stored weight
__device__ __forceinline__ float packed_bf16_source(const float* __restrict__ W, int K, int cin, int cout, int oki, int64_t t) {
  const int per_tap = cin * cout;
  const int k = (int)(t / per_tap);
  int r = (int)(t - (int64_t)k * per_tap);
  const int NTt = cout / 16, NB2 = cin / 32;
  const int full = NB2 * NTt * 512;
  int ci, co;
  if (r < full) {
    const int b = r / (NTt * 512);
    r -= b * NTt * 512;
    const int nt = r >> 9, l = (r & 511) >> 3, j = r & 7;
    ci = 32 * b + 8 * (l >> 4) + j, co = 16 * nt + (l & 15);
  } else {
    r -= full;
    const int nt = r >> 8, l = (r & 255) >> 2, j = r & 3;
    ci = 32 * NB2 + 4 * (l >> 4) + j, co = 16 * nt + (l & 15);
  }
  if (oki) return W[((int64_t)co * K + k) * cin + ci];  // [Cout][K][Cin]
  return W[((int64_t)k * cin + ci) * cout + co];       // [K][Cin][Cout]
}

constexpr int kPackBatch = 24;
struct PackBatch {
  gpn::PackBf16Desc d[kPackBatch];
};
__global__ __launch_bounds__(kThreads) void pack_bf16_kernel(PackBatch batch) {
  const gpn::PackBf16Desc d = batch.d[blockIdx.y];
  const int64_t total = (int64_t)d.K * d.cin * d.cout;
  for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads)
    d.packed[t] = bf16_rne(packed_bf16_source(d.W, d.K, d.cin, d.cout, d.oki, t));
}

inline int grid_for(int64_t total) {
  const int64_t g = gpn::cdiv(total, kThreads);
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

__global__ __launch_bounds__(kThreads) void rows_to_bf16_kernel(const float* __restrict__ x, int64_t total, uint16_t* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) y[i] = bf16_rne(x[i]);
}

// y = act(bn_eval(x) [+ res]): the conv epilogue's arithmetic on a slot no conv produced
__global__ __launch_bounds__(kThreads) void bn_act_bf16_kernel(const void* __restrict__ x, int x_is_f32, const uint16_t* __restrict__ res,
                                                               const float* __restrict__ weight, const float* __restrict__ bias,
                                                               const float* __restrict__ mean, const float* __restrict__ var,
                                                               float eps, int64_t total, int C, int relu, int out_f32,
                                                               void* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int c = (int)(i % C);
    float v = x_is_f32 ? static_cast<const float*>(x)[i] : bf16_widen(static_cast<const uint16_t*>(x)[i]);
    v = (v - mean[c]) * (1.0f / sqrtf(var[c] + eps)) * weight[c] + bias[c];
    if (res) v += bf16_widen(res[i]);
    if (relu) v = v > 0.f ? v : 0.f;
    if (out_f32) static_cast<float*>(y)[i] = v;
    else static_cast<uint16_t*>(y)[i] = bf16_rne(v);
  }
}

// dst[r, 0:ca] = a[r, :], dst[r, ca:ca+cb] = b[r, :] in units of 4 bf16 (channel counts are multiples of 4)
__global__ __launch_bounds__(kThreads) void concat_bf16_kernel(const uint2* __restrict__ a, const uint2* __restrict__ b,
                                                               uint2* __restrict__ dst, int64_t rows, int ca4, int cb4) {
  const int c4 = ca4 + cb4;
  const int64_t total = rows * c4;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t r = i / c4;
    const int c = (int)(i - r * c4);
    dst[i] = c < ca4 ? a[r * ca4 + c] : b[r * cb4 + (c - ca4)];
  }
}

}  // namespace

namespace gpn {

int spconv_bf16_check(const char* who, int K, int64_t n_dst, int cin, int cout) {
  if (K < 1 || K > kMaxTaps || n_dst < 0) {
    gpn::set_error("%s: bad argument: 1 <= K <= 27 and n_dst >= 0 (K = %d, n_dst = %lld)", who, K, (long long)n_dst);
    return GPN_ERR_ARG;
  }
  if (cin < 16 || cin % 16 || cout < 16 || cout % 16) {
    gpn::set_error("%s: channel counts must be multiples of 16 (cin = %d, cout = %d)", who, cin, cout);
    return GPN_ERR_ARG;
  }
  if (!conv_width(cin / 16)) {
    gpn::set_error("%s: no bf16 kernel for %d input channels (16 ... 128, 160, 192, 224)", who, cin);
    return GPN_ERR_ARG;
  }
  // 32-bit byte offsets: source rows (at most 8 n_dst of them, for a stride-2 conv), output rows, the neighbour table
  if (n_dst * (int64_t)8 * std::max(cin, cout) * 2 >= ((int64_t)1 << 31) || (int64_t)K * n_dst * 4 >= ((int64_t)1 << 31)) {
    gpn::set_error("%s: %lld rows of %d channels exceed the kernel's 32-bit byte offsets", who, (long long)n_dst, std::max(cin, cout));
    return GPN_ERR_ARG;
  }
  return GPN_OK;
}

int spconv_bf16_launch(const uint16_t* in, const uint16_t* packed, const int32_t* nbr, const int32_t* nbr_p, const int32_t* perm,
                       int K, int64_t n_dst, int cin, int cout, const gpn_conv_epilogue_bf16_t* ep, void* out, hipStream_t stream) {
  const int CB = cin / 16, nt_total = cout / 16;
  const int NT = cols_per_wave(nt_total);
  Bf16ConvArgs a;
  a.in = in, a.packed = packed, a.nbr = perm ? nbr_p : nbr, a.perm = perm, a.out = out;
  a.n_dst = n_dst, a.K = K, a.n_tiles = (int)gpn::cdiv(n_dst, 16), a.nt_total = nt_total, a.col_groups = nt_total / NT;
  a.n_units = a.n_tiles * a.col_groups;
  a.packed_bytes = (uint32_t)((size_t)K * cin * cout * 2);
  if (ep) a.ep = *ep;
  else a.ep = gpn_conv_epilogue_bf16_t{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0, 0};
  const double pairs = (double)K * (double)n_dst;  // (an upper bound: the launch does not know the live pairs)
  gpn::ProfScope prof(GPN_K_SPCONV_FWD, stream, 2.0 * pairs * cin * cout, (double)n_dst * (cin + cout) * 2.0,
                      gpn::prof_shape_tag(K, n_dst, cin, cout, false));
#define GPN_X(cb) if (CB == cb) return dispatch_cols<cb>(NT, a, stream);
  GPN_CONV_CB(GPN_X)
#undef GPN_X
  gpn::set_error("gpn_spconv_fwd_bf16: no bf16 kernel for %d -> %d channels", cin, cout);
  return GPN_ERR_ARG;
}

int pack_bf16_many(const PackBf16Desc* descs, int n, hipStream_t stream) {
  for (int i0 = 0; i0 < n; i0 += kPackBatch) {
    PackBatch batch;
    const int fill = std::min(kPackBatch, n - i0);
    int64_t max_total = 0;
    for (int i = 0; i < fill; ++i) {
      batch.d[i] = descs[i0 + i];
      max_total = std::max<int64_t>(max_total, (int64_t)descs[i0 + i].K * descs[i0 + i].cin * descs[i0 + i].cout);
    }
    const int gx = (int)std::min<int64_t>(gpn::cdiv(max_total, kThreads), 256);
    hipLaunchKernelGGL(pack_bf16_kernel, dim3(gx, fill), dim3(kThreads), 0, stream, batch);
    GPN_CHECK_LAUNCH();
  }
  return GPN_OK;
}

int rows_to_bf16_launch(const float* x, int64_t total, uint16_t* y, hipStream_t stream) {
  if (total == 0) return GPN_OK;
  hipLaunchKernelGGL(rows_to_bf16_kernel, dim3(grid_for(total)), dim3(kThreads), 0, stream, x, total, y);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

int bn_act_bf16_launch(const void* x, int x_is_f32, const uint16_t* res, const float* weight, const float* bias, const float* mean,
                       const float* var, float eps, int64_t N, int C, int relu, int out_f32, void* y, hipStream_t stream) {
  if (N == 0) return GPN_OK;
  hipLaunchKernelGGL(bn_act_bf16_kernel, dim3(grid_for(N * C)), dim3(kThreads), 0, stream, x, x_is_f32, res, weight, bias, mean, var,
                     eps, N * C, C, relu, out_f32, y);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

int concat_bf16_launch(const uint16_t* a, const uint16_t* b, uint16_t* dst, int64_t rows, int ca, int cb, hipStream_t stream) {
  hipLaunchKernelGGL(concat_bf16_kernel, dim3(grid_for(rows * ((ca + cb) / 4))), dim3(kThreads), 0, stream, (const uint2*)a,
                     (const uint2*)b, (uint2*)dst, rows, ca / 4, cb / 4);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

}  // namespace gpn

extern "C" {

int gpn_spconv_pack_weights_bf16(const float* W, int K, int cin_w, int cout_w, int flags, uint16_t* packed, gpn_stream_t stream) {
  GPN_CHECK_ARG(W && packed);
  GPN_CHECK_ARG(flags == 0 || flags == GPN_LAYOUT_OKI);
  int rc = gpn::spconv_bf16_check(__func__, K, 0, cin_w, cout_w);
  if (rc) return rc;
  const gpn::PackBf16Desc d{W, packed, K, cin_w, cout_w, flags == GPN_LAYOUT_OKI ? 1 : 0};
  return gpn::pack_bf16_many(&d, 1, (hipStream_t)stream);
}

int gpn_spconv_fwd_bf16(const uint16_t* in, const uint16_t* packed_w, const int32_t* nbr, const int32_t* nbr_p, const int32_t* perm,
                        int K, int64_t n_dst, int cin, int cout, const gpn_conv_epilogue_bf16_t* ep, void* out,
                        gpn_stream_t stream) {
  GPN_CHECK_ARG((nbr_p == nullptr) == (perm == nullptr));
  int rc = gpn::spconv_bf16_check(__func__, K, n_dst, cin, cout);
  if (rc) return rc;
  if (ep && ep->mean) GPN_CHECK_ARG(ep->var && ep->weight && ep->bias);
  if (n_dst == 0) return GPN_OK;
  GPN_CHECK_ARG(in && packed_w && nbr && out);
  return gpn::spconv_bf16_launch(in, packed_w, nbr, nbr_p, perm, K, n_dst, cin, cout, ep, out, (hipStream_t)stream);
}

int gpn_rows_to_bf16(const float* x, int64_t n, int C, uint16_t* y, gpn_stream_t stream) {
  GPN_CHECK_ARG(n >= 0 && C >= 1);
  if (n == 0) return GPN_OK;
  GPN_CHECK_ARG(x && y);
  return gpn::rows_to_bf16_launch(x, n * C, y, (hipStream_t)stream);
}

int gpn_bn_act_bf16(const void* x, int x_is_f32, const uint16_t* res, const float* weight, const float* bias, const float* mean,
                    const float* var, float eps, int64_t N, int C, int relu, uint16_t* y, gpn_stream_t stream) {
  GPN_CHECK_ARG(N >= 0 && C >= 1);
  GPN_CHECK_ARG(weight && bias && mean && var);
  if (N == 0) return GPN_OK;
  GPN_CHECK_ARG(x && y);
  return gpn::bn_act_bf16_launch(x, x_is_f32, res, weight, bias, mean, var, eps, N, C, relu, 0, y, (hipStream_t)stream);
}

}
