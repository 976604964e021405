// poseeval.hip — pose evaluation (include/gpn.h section PE): the ground-truth pose of every instance, the exact IoU of two
// oriented boxes, and rotation / translation / scale error and box IoU of matched pairs under the part's symmetry group.  The
// reference has no counterpart (its on_test_epoch_end stops at a commented-out "# pose estimation"); the errors are the ones the
// GAPartNet paper reports for its second task.
//
// Float64 throughout, no float atomics, every reduction of a fixed shape, no host read:
//  * pose_gt_fit_kernel: one workgroup per (scene, slot).  It walks its scene's rows in chunks of the workgroup's size, ranks the
//    rows of its slot by a ballot prefix and queues their row numbers in an LDS ring; whenever the ring holds a workgroup's worth,
//    thread t takes the row of rank = t (mod the workgroup's size).  So which thread adds which point, and in which order, depends
//    on the instance's own points alone: an instance's result is bit-equal whatever else shares its scene or batch.  Two such
//    walks: sums for the means (and count and max |npcs|), then the centred moments; each reduced by a shuffle tree per wave and
//    the waves in order.  Thread 0 then runs the 3x3 Umeyama and writes.
//  * box_iou_kernel / pose_pair_errors_kernel: one lane per (box pair, face): the face (4 corners) is clipped by the six half-spaces
//    of the other box (Sutherland-Hodgman, at most 10 vertices) and its cone volume from A's centre is taken.  The two polygon
//    buffers of a lane are a slice of LDS ([buffer][vertex][component][lane]: a runtime-indexed private array would live in
//    scratch), the boxes sit in LDS as well.  The twelve face volumes of a pair are summed in face order by one lane; the extrema
//    over symmetry candidates are a sequential scan in candidate order with strict comparisons (the first extremum wins).
// The tie rule of the clipping (gpn.h): a vertex ON a clipping plane is inside only while A's faces are clipped by B and only where
// the face's outward normal and the plane's normal have a positive dot product.  ON = within 2^-26 x the largest half extent of
// the two boxes: with an exact test the sign of a rounding error decides whether a coincident face of a turned box counts, and a
// box against itself (or against a copy that differs in the last bits) comes out anywhere between 0.1 and 15; with the snap the
// worst case is about sqrt(eps), where faces meet at an angle near 2^-26 rad (conditioning eps / angle beyond, the snap below).
#include "gpn_common.h"
#include "pose_math.h"

namespace {

constexpr int kFitThreads = 256;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kRing = 2 * kFitThreads;  // fewer than kFitThreads rows wait when a chunk adds at most kFitThreads
constexpr int kClipThreads = 64;        // one wave: a lane a face
constexpr int kPolyMax = 10;            // a quadrilateral cut by six planes
constexpr int kPairsPerBlock = 5;       // 5 x 12 faces = 60 of the 64 lanes
constexpr int kMaxCand = 24;            // candidates of the largest symmetry group
constexpr double kSnap = 1.0 / 67108864.0;  // 2^-26 ~ sqrt(eps): a vertex this close to a plane (x the larger box's extent) is ON it

// ---- gpn_pose_gt_fit ----------------------------------------------------------------------------------------------------------
// One walk over the scene's rows; `take(row)` is called by thread t for the slot's rows of rank t, t + kFitThreads, ... in that
// order.  Every thread of the workgroup must call it (barriers inside; trip counts depend on the scene alone).
template <typename Take>
__device__ __forceinline__ void walk_slot_rows(const int32_t* __restrict__ slot, int64_t r0, int64_t r1, int32_t want,
                                               int64_t* ring /* [kRing] */, int* wave_total /* [kFitWaves] */, Take take) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t queued = 0, taken = 0;  // (the same in every thread)
  for (int64_t c0 = r0; c0 < r1; c0 += kFitThreads) {
    const int64_t row = c0 + tid;
    const bool mine = row < r1 && slot[row] == want;
    const unsigned long long votes = __ballot(mine);
    const int before = __popcll(votes & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(votes);
    __syncthreads();
    int base = 0, added = 0;
#pragma unroll
    for (int w = 0; w < kFitWaves; ++w) {
      const int n = wave_total[w];
      if (w < wave) base += n;
      added += n;
    }
    if (mine) ring[(queued + base + before) & (kRing - 1)] = row;
    queued += added;
    __syncthreads();  // (the totals were read before it, the ring is read after it: the next chunk may write both)
    if (queued - taken >= kFitThreads) {  // (uniform)
      take(ring[(taken + tid) & (kRing - 1)]);
      taken += kFitThreads;
    }
  }
  if (tid < queued - taken) take(ring[(taken + tid) & (kRing - 1)]);
  __syncthreads();  // (the ring and the totals are free for the next walk)
}

__global__ __launch_bounds__(kFitThreads) void pose_gt_fit_kernel(
    const float* __restrict__ xyz, const float* __restrict__ npcs, const int32_t* __restrict__ slot,
    const int64_t* __restrict__ scene_offsets, int64_t N, int W, int64_t* __restrict__ count_out, uint8_t* __restrict__ valid_out,
    double* __restrict__ scale_out, double* __restrict__ rot_out, double* __restrict__ trans_out, double* __restrict__ half_out,
    double* __restrict__ bbox_out) {
  __shared__ int64_t ring[kRing];
  __shared__ int wave_total[kFitWaves];
  __shared__ double red[kFitWaves * 15];
  const int64_t g = blockIdx.x;  // the flat slot
  const int64_t s = g / W;
  const int tid = threadIdx.x;
  int64_t r0 = scene_offsets[s], r1 = scene_offsets[s + 1];
  r0 = r0 < 0 ? 0 : (r0 > N ? N : r0);  // (offsets outside the arrays read nothing)
  r1 = r1 < r0 ? r0 : (r1 > N ? N : r1);
  const int32_t want = (int32_t)g;
  // ---- walk 1: count, sums, max |npcs| ----
  double sum[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // npcs [3] | xyz [3] | count
  double ext[3] = {0.0, 0.0, 0.0};
  walk_slot_rows(slot, r0, r1, want, ring, wave_total, [&](int64_t row) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double q = (double)npcs[row * 3 + c];
      sum[c] += q, sum[3 + c] += (double)xyz[row * 3 + c];
      ext[c] = fmax(ext[c], fabs(q));  // (fmax drops a NaN here; the sums keep it, so the slot comes out invalid)
    }
    sum[6] += 1.0;
  });
  block_reduce<7>(sum, red, SumOp());
  block_reduce<3>(ext, red, MaxOp());
  const double n = sum[6];
  double mu_s[3], mu_d[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) mu_s[c] = sum[c] / n, mu_d[c] = sum[3 + c] / n;
  // ---- walk 2: centred moments ----
  double mom[15];  // sum (d - mu_d)(s - mu_s)^T [9] | sum (s - mu_s)(s - mu_s)^T: xx xy xz yy yz zz
#pragma unroll
  for (int i = 0; i < 15; ++i) mom[i] = 0.0;
  walk_slot_rows(slot, r0, r1, want, ring, wave_total, [&](int64_t row) {
    double ds[3], dd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ds[c] = (double)npcs[row * 3 + c] - mu_s[c], dd[c] = (double)xyz[row * 3 + c] - mu_d[c];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) mom[a * 3 + b] += dd[a] * ds[b];
    mom[9] += ds[0] * ds[0], mom[10] += ds[0] * ds[1], mom[11] += ds[0] * ds[2];
    mom[12] += ds[1] * ds[1], mom[13] += ds[1] * ds[2], mom[14] += ds[2] * ds[2];
  });
  block_reduce<15>(mom, red, SumOp());
  if (tid != 0) return;  // (no barrier follows)
  // ---- Umeyama (pose_fitting_batched._umeyama: xyz ~ npcs @ (s R) + t) ----
  M3 cov, css, U, V, U2, V2;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) cov.a[a][b] = mom[a * 3 + b] / n;
  css.a[0][0] = mom[9] / n, css.a[0][1] = css.a[1][0] = mom[10] / n, css.a[0][2] = css.a[2][0] = mom[11] / n;
  css.a[1][1] = mom[12] / n, css.a[1][2] = css.a[2][1] = mom[13] / n, css.a[2][2] = mom[14] / n;
  const double var = css.a[0][0] + css.a[1][1] + css.a[2][2];
  double S[3], S2[3];
  svd3(css, U2, S2, V2);
  svd3(cov, U, S, V);
  M3 Vh;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Vh.a[i][j] = V.a[j][i];
  if (det3(U) * det3(Vh) < 0.0) {
    S[2] = -S[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) U.a[r][2] = -U.a[r][2];
  }
  const double scale = (S[0] + S[1] + S[2]) / var;
  M3 R;  // (U Vh)^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R.a[i][j] = U.a[j][0] * Vh.a[0][i] + U.a[j][1] * Vh.a[1][i] + U.a[j][2] * Vh.a[2][i];
  double t[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) t[j] = mu_d[j] - (mu_s[0] * (scale * R.a[0][j]) + mu_s[1] * (scale * R.a[1][j]) + mu_s[2] * (scale * R.a[2][j]));
  bool ok = n >= 3.0 && S2[1] >= 1e-9 * S2[0] && S2[0] > 0.0 && isfinite(scale);  // (NaN moments fail the comparisons)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) ok = ok && isfinite(R.a[i][j]);
#pragma unroll
  for (int j = 0; j < 3; ++j) ok = ok && isfinite(t[j]);
  const double qn = nan("");
  count_out[g] = (int64_t)n;
  valid_out[g] = ok ? 1 : 0;
  scale_out[g] = ok ? scale : qn;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    trans_out[g * 3 + i] = ok ? t[i] : qn;
    half_out[g * 3 + i] = ok ? ext[i] : qn;
#pragma unroll
    for (int j = 0; j < 3; ++j) rot_out[g * 9 + i * 3 + j] = ok ? R.a[i][j] : qn;
  }
  const int sg[8][3] = {{-1, -1, -1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}, {1, 1, -1}, {1, -1, 1}, {-1, 1, 1}, {1, 1, 1}};
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) acc += (double)sg[k][i] * ext[i] * scale * R.a[i][j];
      bbox_out[g * 24 + k * 3 + j] = ok ? acc + t[j] : qn;
    }
}

// ---- oriented boxes and the clipping ------------------------------------------------------------------------------------------
struct Box {              // in LDS
  double corner[8][3];    // _CORNER_SIGNS order: --- +-- -+- --+ ++- +-+ -++ +++
  double c[3];            // centre = mean of the corners
  double u[3][3];         // unit axes: (corner 1, 2, 3 - corner 0) normalised
  double h[3];            // half extents = half the lengths of those edges
  double vol;             // 8 h0 h1 h2, NaN for a non-finite corner or a zero extent
};

// the corners of face f = 2 * axis + (0: the -axis side, 1: the +axis side), in cyclic order
__device__ const int kFaceCorner[6][4] = {{0, 2, 6, 3}, {1, 4, 7, 5}, {0, 1, 5, 3}, {2, 4, 7, 6}, {0, 1, 4, 2}, {3, 5, 7, 6}};

// centre, axes, extents and volume from the corners (one thread a box)
__device__ void box_finish(Box& b) {
  bool finite = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += b.corner[k][j], finite = finite && isfinite(b.corner[k][j]);
    b.c[j] = acc / 8.0;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double e0 = (b.corner[i + 1][0] - b.corner[0][0]) / 2.0, e1 = (b.corner[i + 1][1] - b.corner[0][1]) / 2.0,
                 e2 = (b.corner[i + 1][2] - b.corner[0][2]) / 2.0;
    const double len = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    b.h[i] = len;
    b.u[i][0] = e0 / len, b.u[i][1] = e1 / len, b.u[i][2] = e2 / len;
  }
  const double vol = 8.0 * b.h[0] * b.h[1] * b.h[2];
  b.vol = finite && vol > 0.0 && isfinite(vol) ? vol : nan("");
}

// the corners of the box with half extents `half` * scale along the rows of R about t (what gpn_pose_fit's bbox is)
__device__ void box_from_pose(Box& b, double scale, const double (&R)[3][3], const double* t, const double* half) {
  const int sg[8][3] = {{-1, -1, -1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}, {1, 1, -1}, {1, -1, 1}, {-1, 1, 1}, {1, 1, 1}};
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) acc += (double)sg[k][i] * half[i] * scale * R[i][j];
      b.corner[k][j] = acc + t[j];
    }
  box_finish(b);
}

// Face `face` of box X clipped by the six half-spaces of box Y; its cone volume from `apex`: area * height / 3 with the height
// along the face's outward normal.  poly = this lane's LDS slice, element (buffer, vertex, component) at
// ((buffer * kPolyMax + vertex) * 3 + component) * kClipThreads.  a_by_b: X is A and Y is B (the pass in which ties may be inside).
__device__ double clipped_face_cone(const Box& X, const Box& Y, int face, bool a_by_b, const double* apex, double* poly) {
  const int axis = face >> 1;
  const double sgn = (face & 1) ? 1.0 : -1.0;
  const double nx = sgn * X.u[axis][0], ny = sgn * X.u[axis][1], nz = sgn * X.u[axis][2];
#define POLY(buf, v, c) poly[(((buf) * kPolyMax + (v)) * 3 + (c)) * kClipThreads]
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int k = kFaceCorner[face][v];
#pragma unroll
    for (int c = 0; c < 3; ++c) POLY(0, v, c) = X.corner[k][c];
  }
  const double snap = kSnap * fmax(fmax(fmax(X.h[0], X.h[1]), X.h[2]), fmax(fmax(Y.h[0], Y.h[1]), Y.h[2]));
  int n = 4, cur = 0;
  for (int pl = 0; pl < 6 && n > 0; ++pl) {
    const int pa = pl >> 1;
    const double ps = (pl & 1) ? 1.0 : -1.0;
    const double px = ps * Y.u[pa][0], py = ps * Y.u[pa][1], pz = ps * Y.u[pa][2];
    const double ph = Y.h[pa];
    const bool tie_in = a_by_b && (nx * px + ny * py + nz * pz) > 0.0;
    int m = 0;
    // signed distance of a vertex: positive outside
    double p0 = POLY(cur, 0, 0), p1 = POLY(cur, 0, 1), p2 = POLY(cur, 0, 2);
    double dp = ((p0 - Y.c[0]) * px + (p1 - Y.c[1]) * py + (p2 - Y.c[2]) * pz) - ph;
    if (fabs(dp) <= snap) dp = 0.0;
    for (int i = 0; i < n; ++i) {
      const int j = i + 1 == n ? 0 : i + 1;
      const double q0 = POLY(cur, j, 0), q1 = POLY(cur, j, 1), q2 = POLY(cur, j, 2);
      double dq = ((q0 - Y.c[0]) * px + (q1 - Y.c[1]) * py + (q2 - Y.c[2]) * pz) - ph;
      if (fabs(dq) <= snap) dq = 0.0;
      const bool in_p = dp < 0.0 || (dp == 0.0 && tie_in), in_q = dq < 0.0 || (dq == 0.0 && tie_in);
      if (in_p && m < kPolyMax) {
        POLY(cur ^ 1, m, 0) = p0, POLY(cur ^ 1, m, 1) = p1, POLY(cur ^ 1, m, 2) = p2;
        ++m;
      }
      if (in_p != in_q && m < kPolyMax) {
        const double t = dp / (dp - dq);
        POLY(cur ^ 1, m, 0) = p0 + t * (q0 - p0), POLY(cur ^ 1, m, 1) = p1 + t * (q1 - p1), POLY(cur ^ 1, m, 2) = p2 + t * (q2 - p2);
        ++m;
      }
      p0 = q0, p1 = q1, p2 = q2, dp = dq;
    }
    n = m, cur ^= 1;
  }
  if (n < 3) return 0.0;
  const double v0 = POLY(cur, 0, 0), v1 = POLY(cur, 0, 1), v2 = POLY(cur, 0, 2);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;  // sum of (v_i - v_0) x (v_i+1 - v_0): twice the area vector
  for (int i = 1; i + 1 < n; ++i) {
    const double a0 = POLY(cur, i, 0) - v0, a1 = POLY(cur, i, 1) - v1, a2 = POLY(cur, i, 2) - v2;
    const double b0 = POLY(cur, i + 1, 0) - v0, b1 = POLY(cur, i + 1, 1) - v1, b2 = POLY(cur, i + 1, 2) - v2;
    s0 += a1 * b2 - a2 * b1, s1 += a2 * b0 - a0 * b2, s2 += a0 * b1 - a1 * b0;
  }
#undef POLY
  const double area = 0.5 * fabs(s0 * nx + s1 * ny + s2 * nz);
  const double height = (v0 - apex[0]) * nx + (v1 - apex[1]) * ny + (v2 - apex[2]) * nz;
  return area * height / 3.0;
}

// face task f of a pair: 0 - 5 the faces of A cut by B, 6 - 11 the faces of B cut by A; the apex is A's centre in both
__device__ __forceinline__ double pair_face_cone(const Box& A, const Box& B, int f, double* poly) {
  return f < 6 ? clipped_face_cone(A, B, f, true, A.c, poly) : clipped_face_cone(B, A, f - 6, false, A.c, poly);
}

__device__ __forceinline__ double iou_from_faces(const Box& A, const Box& B, const double* cone /* [12] */) {
  double inter = 0.0;
#pragma unroll
  for (int f = 0; f < 12; ++f) inter += cone[f];
  return inter / (A.vol + B.vol - inter);  // (a NaN volume: NaN)
}

__global__ __launch_bounds__(kClipThreads) void box_iou_kernel(const double* __restrict__ a, const double* __restrict__ b, int64_t P,
                                                               double* __restrict__ iou) {
  __shared__ Box boxes[kPairsPerBlock][2];
  __shared__ double poly[2 * kPolyMax * 3 * kClipThreads];
  __shared__ double cone[kPairsPerBlock][12];
  const int tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * kPairsPerBlock;
  // the corners of this block's boxes: 5 pairs x 2 boxes x 24 doubles
  for (int e = tid; e < kPairsPerBlock * 2 * 24; e += kClipThreads) {
    const int q = e / 48, r = e - q * 48, side = r / 24, w = r - side * 24;
    if (p0 + q < P) boxes[q][side].corner[w / 3][w % 3] = (side ? b : a)[(p0 + q) * 24 + w];
  }
  __syncthreads();
  if (tid < kPairsPerBlock * 2 && p0 + tid / 2 < P) box_finish(boxes[tid / 2][tid & 1]);
  __syncthreads();
  const int q = tid / 12, f = tid - q * 12;
  const bool live = q < kPairsPerBlock && p0 + q < P;
  if (live) {
    const Box& A = boxes[q][0];
    const Box& B = boxes[q][1];
    // (a box without a volume has NaN axes: nothing to clip, and the NaN volume makes the IoU NaN)
    cone[q][f] = (A.vol == A.vol && B.vol == B.vol) ? pair_face_cone(A, B, f, poly + tid) : 0.0;
  }
  __syncthreads();
  if (live && f == 0) iou[p0 + q] = iou_from_faces(boxes[q][0], boxes[q][1], cone[q]);
}

// ---- gpn_pose_pair_errors -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kClipThreads) void pose_pair_errors_kernel(
    const double* __restrict__ scale_p, const double* __restrict__ rot_p, const double* __restrict__ trans_p,
    const double* __restrict__ half_p, const double* __restrict__ scale_g, const double* __restrict__ rot_g,
    const double* __restrict__ trans_g, const double* __restrict__ half_g, const int32_t* __restrict__ sym_type,
    const double* __restrict__ sym_table, int K, const int32_t* __restrict__ sym_start, const int32_t* __restrict__ sym_count, int T,
    double* __restrict__ re_deg, int32_t* __restrict__ k_re, double* __restrict__ te, double* __restrict__ se,
    double* __restrict__ iou, int32_t* __restrict__ k_iou) {
  __shared__ Box box_p;
  __shared__ Box box_c[kMaxCand];
  __shared__ double poly[2 * kPolyMax * 3 * kClipThreads];
  __shared__ double cone[kMaxCand][12];
  __shared__ double re_sh[kMaxCand], iou_sh[kMaxCand];
  const int64_t p = blockIdx.x;
  const int tid = threadIdx.x;
  const int ty = sym_type[p];
  int first = 0, cnt = 0;
  if (ty >= 0 && ty < T) first = sym_start[ty], cnt = sym_count[ty];
  const bool table_ok = cnt >= 1 && cnt <= kMaxCand && first >= 0 && first + cnt <= K;  // (uniform over the workgroup)
  const double qn = nan("");
  if (!table_ok) {  // a type outside the table: nothing to compare with
    if (tid == 0) re_deg[p] = qn, k_re[p] = -1, te[p] = qn, se[p] = qn, iou[p] = qn, k_iou[p] = -1;
    return;
  }
  if (tid < cnt) {  // candidate k: the frame S_k R_gt, the angle to R_pred, the re-framed ground-truth box
    const double* Sk = sym_table + (int64_t)(first + tid) * 9;
    const double* Rg = rot_g + p * 9;
    const double* Rp = rot_p + p * 9;
    double F[3][3], M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) F[i][j] = Sk[i * 3 + 0] * Rg[0 * 3 + j] + Sk[i * 3 + 1] * Rg[1 * 3 + j] + Sk[i * 3 + 2] * Rg[2 * 3 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) M[i][j] = Rp[i * 3 + 0] * F[j][0] + Rp[i * 3 + 1] * F[j][1] + Rp[i * 3 + 2] * F[j][2];  // R_pred F^T
    const double v0 = (M[2][1] - M[1][2]) / 2.0, v1 = (M[0][2] - M[2][0]) / 2.0, v2 = (M[1][0] - M[0][1]) / 2.0;
    const double tr = M[0][0] + M[1][1] + M[2][2];
    re_sh[tid] = atan2(sqrt(v0 * v0 + v1 * v1 + v2 * v2), (tr - 1.0) / 2.0) * (180.0 / M_PI);
    box_from_pose(box_c[tid], scale_g[p], F, trans_g + p * 3, half_g + p * 3);
  }
  if (tid == kClipThreads - 1) {  // (a lane no candidate uses: cnt <= 24)
    double Rp[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Rp[i][j] = rot_p[p * 9 + i * 3 + j];
    box_from_pose(box_p, scale_p[p], Rp, trans_p + p * 3, half_p + p * 3);
  }
  __syncthreads();
  const int tasks = cnt * 12;
  for (int e = tid; e < tasks; e += kClipThreads) {
    const int k = e / 12, f = e - k * 12;
    cone[k][f] = (box_p.vol == box_p.vol && box_c[k].vol == box_c[k].vol) ? pair_face_cone(box_p, box_c[k], f, poly + tid) : 0.0;
  }
  __syncthreads();
  if (tid < cnt) iou_sh[tid] = iou_from_faces(box_p, box_c[tid], cone[tid]);
  __syncthreads();
  if (tid == 0) {
    double best_re = re_sh[0], best_iou = iou_sh[0];
    int kr = 0, ki = 0;
    for (int k = 1; k < cnt; ++k) {  // strict comparisons: the first extremum stays (a NaN never replaces, and is never replaced)
      if (re_sh[k] < best_re) best_re = re_sh[k], kr = k;
      if (iou_sh[k] > best_iou) best_iou = iou_sh[k], ki = k;
    }
    const double d0 = trans_p[p * 3] - trans_g[p * 3], d1 = trans_p[p * 3 + 1] - trans_g[p * 3 + 1], d2 = trans_p[p * 3 + 2] - trans_g[p * 3 + 2];
    re_deg[p] = best_re, k_re[p] = kr;
    te[p] = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    se[p] = fabs(scale_p[p] - scale_g[p]);
    iou[p] = best_iou, k_iou[p] = ki;
  }
}

}  // namespace

extern "C" int gpn_pose_gt_fit(const float* xyz, const float* npcs, const int32_t* slot, const int64_t* scene_offsets, int64_t N, int S,
                               int W, int64_t* count, uint8_t* valid, double* scale, double* rotation, double* translation,
                               double* half, double* bbox, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(N >= 0 && S >= 0 && W >= 0 && (int64_t)S * W <= 0x7fffffff);
  if (S == 0 || W == 0) return GPN_OK;
  GPN_CHECK_ARG(scene_offsets && count && valid && scale && rotation && translation && half && bbox);
  GPN_CHECK_ARG(N == 0 || (xyz && npcs && slot));
  hipLaunchKernelGGL(pose_gt_fit_kernel, dim3((unsigned)((int64_t)S * W)), dim3(kFitThreads), 0, stream, xyz, npcs, slot, scene_offsets,
                     N, W, count, valid, scale, rotation, translation, half, bbox);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_box_iou_3d(const double* a, const double* b, int64_t P, double* iou, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(P >= 0 && P <= (int64_t)0x7fffffff * kPairsPerBlock);
  if (P == 0) return GPN_OK;
  GPN_CHECK_ARG(a && b && iou);
  hipLaunchKernelGGL(box_iou_kernel, dim3((unsigned)gpn::cdiv(P, kPairsPerBlock)), dim3(kClipThreads), 0, stream, a, b, P, iou);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_pose_pair_errors(const double* scale_pred, const double* rotation_pred, const double* translation_pred,
                                    const double* half_pred, const double* scale_gt, const double* rotation_gt,
                                    const double* translation_gt, const double* half_gt, const int32_t* sym_type, int64_t P,
                                    const double* sym_table, int K, const int32_t* sym_start, const int32_t* sym_count, int T,
                                    double* re_deg, int32_t* k_re, double* te, double* se, double* iou, int32_t* k_iou,
                                    gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(P >= 0 && P <= 0x7fffffff && K >= 1 && T >= 1);
  if (P == 0) return GPN_OK;
  GPN_CHECK_ARG(scale_pred && rotation_pred && translation_pred && half_pred && scale_gt && rotation_gt && translation_gt && half_gt);
  GPN_CHECK_ARG(sym_type && sym_table && sym_start && sym_count && re_deg && k_re && te && se && iou && k_iou);
  hipLaunchKernelGGL(pose_pair_errors_kernel, dim3((unsigned)P), dim3(kClipThreads), 0, stream, scale_pred, rotation_pred,
                     translation_pred, half_pred, scale_gt, rotation_gt, translation_gt, half_gt, sym_type, sym_table, K, sym_start,
                     sym_count, T, re_deg, k_re, te, se, iou, k_iou);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
