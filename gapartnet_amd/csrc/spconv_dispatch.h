// spconv_dispatch.h — what the sparse-conv launchers (spconv_fwd.hip, spconv_tiles.hip, spconv_msplit.hip; the lists also
// spconv.hip and spconv_bf16.hip) share: the instantiation lists, the 32-bit offset guard, the argument set of one conv call
// and the run-time-bool -> template-bool step of a launch.  Which kernel a shape takes is gpn::spconv_fwd_route (gpn_common.h).
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "gpn_common.h"

// ---- instantiation lists: every template argument a dispatch can produce is an entry here, and a dispatch is an expansion of
// its list (tests/test_conv_instantiations.py reads these lists and constants, nothing else) ---------------------------------
// input widths (16-channel blocks): those of a residual U-Net with channels 16 (l + 1), l < 7, and of its decoder convs behind
// the skip concats (2c -> c).  The direct kernel has no 14.
#define GPN_CONV_CB(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(10) X(12) X(14)
#define GPN_DIRECT_CB(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(10) X(12)
// masked-tile kernel (and its bf16 sibling, spconv_bf16.hip): column tiles per wave (row tiles per wave: kTilesR)
#define GPN_TILES_NT(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
// masked tap-split kernel: column tiles per workgroup, waves per row tile (9 where CB (1 + NT) <= kMsplitSp9MaxRegs4)
#define GPN_MSPLIT_NT(X) X(1) X(2) X(3) X(4)
#define GPN_MSPLIT_SP(X) X(4) X(9)
// direct kernel: taps; its tap-split form's ways, in the order they are tried, for layers of at least kSplitMinTaps taps
#define GPN_DIRECT_KT(X) X(27) X(8) X(1)
#define GPN_SPLIT_WAYS(X) X(4) X(2)
// lock-step kernel: column tiles per wave, input blocks per stage, waves per workgroup (NS = ceil(CW NTW / waves))
#define GPN_LOCKSTEP_NTW(X) X(1) X(2) X(3) X(4)
#define GPN_LOCKSTEP_CW(X) X(1) X(2) X(4)
#define GPN_LOCKSTEP_WAVES(X) X(4) X(8) X(16)
// weight gradient: input-block tiles per workgroup (wider inputs run as 4), column tiles
#define GPN_WGRAD_CT(X) X(1) X(2) X(3) X(4)
#define GPN_WGRAD_NT(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

namespace gpn {

constexpr int kTilesR = 1;  // (two row tiles per wave lost 25-38 % at the 80k-row level: spconv_tiles.hip)
// the nine-wave form is instantiated where its ring fits the 168 registers a wave of a 576-thread workgroup can have
constexpr int kMsplitSp9MaxRegs4 = 28;
constexpr int kSplitMinTaps = 8;  // (a k = 1 layer has no taps to split)

inline bool conv_width(int CB) {
#define GPN_X(cb) if (CB == cb) return true;
  GPN_CONV_CB(GPN_X)
#undef GPN_X
  return false;
}

// 32-bit byte offsets: source rows (at most 8 n_dst of them, for a stride-2 conv), output rows, the neighbour table
inline bool conv_offsets_fit32(int K, int64_t n_dst, int cin, int cout) {
  return n_dst * (int64_t)8 * std::max(cin, cout) * 4 < ((int64_t)1 << 31) && (int64_t)K * n_dst * 4 < ((int64_t)1 << 31);
}

template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>()), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {  // f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>)
  static_for_impl(f, std::make_integer_sequence<int, N>());
}

// one conv call, filled once by spconv_fwd_into and read by every dispatch level and launcher below it (host only: kernels
// take scalars).  nbr / perm: the table the kernel reads - in tile order with its row permutation, or plain with perm == nullptr.
struct ConvCall {
  const float* in;
  const float* packed;
  const int32_t* nbr;
  const int32_t* perm;
  int K;
  int64_t n_dst;
  int cin, cout, accumulate;
  const ConvStats& stats;
  float* out;
  hipStream_t stream;
  DevRows rows;
};

// f(std::bool_constant<a>()) / f(std::bool_constant<a>(), std::bool_constant<b>()): a launcher's run-time bools (device-counted
// rows, BatchNorm in the epilogue) as template arguments, so that its launch statement is written once
template <class F>
inline void with_bool(bool a, F&& f) {
  a ? f(std::true_type()) : f(std::false_type());
}
template <class F>
inline void with_bools(bool a, bool b, F&& f) {
  with_bool(a, [&](auto ta) { with_bool(b, [&](auto tb) { f(ta, tb); }); });
}

inline int conv_no_kernel(const char* which, const ConvCall& c) {
  set_error("gpn_spconv_fwd: no %s kernel for %d -> %d channels", which, c.cin, c.cout);
  return GPN_ERR_ARG;
}

// the masked-tile kernel (spconv_tiles.hip) and the masked tap-split kernel (spconv_msplit.hip: k = 27 / 8 layers below the
// masked-tile kernel's size): which shapes they take, and their launches
bool spconv_tiles_supported(int K, int64_t n_dst, int cin, int cout);
int spconv_tiles_launch(const ConvCall& c);
bool spconv_msplit_supported(int K, int64_t n_dst, int cin, int cout);
int spconv_msplit_launch(const ConvCall& c);

}  // namespace gpn
