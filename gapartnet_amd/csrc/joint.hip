// joint.hip — joint axis, pivot and angle from two observations of one part (include/gpn.h section JE).  Reference:
// structure/gapartnet.py:819-963 (estimate_joint_angle): normalise both clouds by the second one's mean and extent, sample K
// rows of each, register the samples rigidly (Coherent Point Drift, Myronenko & Song 2010, as pycpd.RigidRegistration runs it
// with its defaults), turn the rotation and translation into an axis direction, a point on the axis and an angle.
//
// Three launches, float64 throughout (the reference is numpy float64), no float atomics, every reduction of a fixed shape:
//  * joint_sample_kernel: one workgroup per pair: mean and extent of the second cloud, the picked rows of both, normalised.
//  * cpd_rigid_kernel: one workgroup per pair runs the WHOLE EM loop.  A thread owns a column n of the M x N responsibility
//    matrix (a point of the fixed set X) and walks the rows m (the moving set) through LDS tiles, so column sums need no atomics
//    and the matrix is never stored.  Every moment the M-step needs is a per-column sum over m divided by the column's
//    denominator: c_n = sum_m e_mn, v_n = sum_m e_mn y_m, q_n = sum_m e_mn |y_m|^2 with e_mn = exp(-|x_n - TY_m|^2 / (2 sigma2)),
//    so one sweep over the tiles per iteration is enough: the exponentials are computed once and never revisited.  The
//    moments are taken about the previous iteration's means (the plain means at the start), which keeps the subtraction of the
//    mean products free of cancellation.  The 18 column moments are reduced over the workgroup (wave shuffles, then the waves'
//    partials in wave order), every thread then does the 3x3 M-step itself, and the decision to go on is one LDS word that
//    thread 0 writes and every thread reads after a barrier: no barrier sits under a divergent branch.  Nothing is sized by
//    K: a thread strides over its columns and the rows come in tiles, so K = 500 (one column a thread, one tile) pays nothing
//    for K = 4096.
//  * joint_from_rigid_kernel: one thread per transform: matrix -> quaternion (w >= 0) -> rotation vector as scipy does it, the
//    half-angle construction of the pivot, or the prismatic reading of the translation.
#include <cfloat>

#include "gpn_common.h"
#include "pose_math.h"

namespace {

constexpr int kSampleThreads = 256;
constexpr int kCpdThreads = 512;          // 8 waves: a column a thread at the default K = 500
constexpr int kCpdTile = kCpdThreads;     // rows of the moving set staged per pass (a row a thread)
constexpr int kCpdSums = 18;              // Np | sum P x [3] | sum P y [3] | sum P x y^T [9] | sum P |x|^2 | sum P |y|^2
constexpr int kMaxWaves = kCpdThreads / 64;

// ---- gpn_joint_sample ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSampleThreads) void joint_sample_kernel(
    const double* __restrict__ pc1, const double* __restrict__ pc2, const int64_t* __restrict__ off1,
    const int64_t* __restrict__ off2, const int64_t* __restrict__ picks1, const int64_t* __restrict__ picks2,
    const int32_t* __restrict__ k1, const int32_t* __restrict__ k2, int K, double* __restrict__ X, double* __restrict__ Y,
    double* __restrict__ norm) {
  __shared__ double red[kMaxWaves * 6];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t o1 = off1[b], n1 = off1[b + 1] - o1, o2 = off2[b], n2 = off2[b + 1] - o2;
  double sum[3] = {0.0, 0.0, 0.0};
  for (int64_t i = tid; i < n2; i += kSampleThreads) {
    const double* p = pc2 + (o2 + i) * 3;
    sum[0] += p[0], sum[1] += p[1], sum[2] += p[2];
  }
  block_reduce<3>(sum, red, SumOp());
  const double qn = nan("");
  const double mean[3] = {n2 > 0 ? sum[0] / (double)n2 : qn, n2 > 0 ? sum[1] / (double)n2 : qn, n2 > 0 ? sum[2] / (double)n2 : qn};
  double ext[6] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY};  // max (p - M) [3] | max -(p - M) [3]
  for (int64_t i = tid; i < n2; i += kSampleThreads) {
    const double* p = pc2 + (o2 + i) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double d = p[c] - mean[c];
      ext[c] = fmax(ext[c], d), ext[3 + c] = fmax(ext[3 + c], -d);
    }
  }
  block_reduce<6>(ext, red, MaxOp());
  // (max - min per axis; -max(-d) is min(d) exactly)
  const double S = n2 > 0 ? fmax(fmax(ext[0] - (-ext[3]), ext[1] - (-ext[4])), ext[2] - (-ext[5])) : qn;
  if (tid == 0) norm[b * 4 + 0] = S, norm[b * 4 + 1] = mean[0], norm[b * 4 + 2] = mean[1], norm[b * 4 + 3] = mean[2];
  const int live1 = min(max(k1[b], 0), K), live2 = min(max(k2[b], 0), K);
  for (int e = tid; e < 2 * K; e += kSampleThreads) {
    const bool second = e >= K;
    const int r = second ? e - K : e;
    const int live = second ? live2 : live1;
    const int64_t n = second ? n2 : n1, o = second ? o2 : o1;
    double* dst = (second ? Y : X) + (b * K + r) * 3;
    if (r >= live) {
      dst[0] = 0.0, dst[1] = 0.0, dst[2] = 0.0;
      continue;
    }
    const int64_t pick = (second ? picks2 : picks1)[b * K + r];
    if (pick < 0 || pick >= n) {  // a pick outside the segment: no point
      dst[0] = qn, dst[1] = qn, dst[2] = qn;
      continue;
    }
    const double* p = (second ? pc2 : pc1) + (o + pick) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = (p[c] - mean[c]) / S;
  }
}

// ---- gpn_cpd_rigid ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCpdThreads) void cpd_rigid_kernel(
    const double* __restrict__ X, const double* __restrict__ Y, const int32_t* __restrict__ nx, const int32_t* __restrict__ ny,
    int K, int max_iterations, double tolerance, double w, int fit_scale, double* __restrict__ s_out, double* __restrict__ R_out,
    double* __restrict__ t_out, double* __restrict__ sigma2_out, double* __restrict__ q_out, double* __restrict__ diff_out,
    int32_t* __restrict__ iterations_out, double* __restrict__ sigma2_trace) {
  __shared__ double tile[kCpdTile][8];  // TY [3] | y - cY [3] | |y - cY|^2 | pad: a 64-byte row, read by every lane at once
  __shared__ double red[kMaxWaves * kCpdSums];
  __shared__ int go_sh;
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int N = nx[b], M = ny[b];
  const double* Xb = X + b * K * 3;
  const double* Yb = Y + b * K * 3;
  const double qn = nan("");
  if (sigma2_trace)
    for (int i = tid; i < max_iterations; i += kCpdThreads) sigma2_trace[b * max_iterations + i] = qn;
  if (N <= 0 || M <= 0 || N > K || M > K) {  // (the whole workgroup leaves: no barrier has been met yet)
    if (tid == 0) {
      s_out[b] = qn, sigma2_out[b] = qn, q_out[b] = qn, diff_out[b] = qn, iterations_out[b] = 0;
      for (int i = 0; i < 9; ++i) R_out[b * 9 + i] = qn;
      for (int i = 0; i < 3; ++i) t_out[b * 3 + i] = qn;
    }
    return;
  }
  // ---- start: the plain means (the first shift of the moments) and sigma2 = sum_mn |x_n - y_m|^2 / (3 M N), which is
  //      (M sum |x - mx|^2 + N sum |y - my|^2 + M N |mx - my|^2) / (3 M N): three non-negative terms, no M x N pass ----
  double cX[3], cY[3];
  {
    double m6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int n = tid; n < N; n += kCpdThreads) m6[0] += Xb[n * 3 + 0], m6[1] += Xb[n * 3 + 1], m6[2] += Xb[n * 3 + 2];
    for (int m = tid; m < M; m += kCpdThreads) m6[3] += Yb[m * 3 + 0], m6[4] += Yb[m * 3 + 1], m6[5] += Yb[m * 3 + 2];
    block_reduce<6>(m6, red, SumOp());
#pragma unroll
    for (int c = 0; c < 3; ++c) cX[c] = m6[c] / (double)N, cY[c] = m6[3 + c] / (double)M;
  }
  double sigma2;
  {
    double v2[2] = {0.0, 0.0};
    for (int n = tid; n < N; n += kCpdThreads) {
      const double d0 = Xb[n * 3 + 0] - cX[0], d1 = Xb[n * 3 + 1] - cX[1], d2 = Xb[n * 3 + 2] - cX[2];
      v2[0] += d0 * d0 + d1 * d1 + d2 * d2;
    }
    for (int m = tid; m < M; m += kCpdThreads) {
      const double d0 = Yb[m * 3 + 0] - cY[0], d1 = Yb[m * 3 + 1] - cY[1], d2 = Yb[m * 3 + 2] - cY[2];
      v2[1] += d0 * d0 + d1 * d1 + d2 * d2;
    }
    block_reduce<2>(v2, red, SumOp());
    const double g0 = cX[0] - cY[0], g1 = cX[1] - cY[1], g2 = cX[2] - cY[2];
    const double dM = (double)M, dN = (double)N;
    sigma2 = (dM * v2[0] + dN * v2[1] + dM * dN * (g0 * g0 + g1 * g1 + g2 * g2)) / (3.0 * dM * dN);
  }
  double s = 1.0, t[3] = {0.0, 0.0, 0.0}, q = INFINITY, diff = INFINITY;
  M3 R;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R.a[i][j] = i == j ? 1.0 : 0.0;
  int it = 0;
  if (tid == 0) go_sh = diff > tolerance ? 1 : 0;
  __syncthreads();
  // every thread reads the same LDS word: the branch is uniform, and the word is next written after the barriers below
  while (it < max_iterations && go_sh != 0) {
    // (the exponent is formed with the reciprocal, once per iteration, instead of a float64 division per responsibility: the
    //  two differ by at most one rounding of the exponent, |exponent| ulps of the term, far below the sums' own round-off)
    const double neg_inv_two_s2 = -1.0 / (2.0 * sigma2);
    const double cc = pow(2.0 * M_PI * sigma2, 1.5) * w / (1.0 - w) * (double)M / (double)N;
    double acc[kCpdSums];
#pragma unroll
    for (int i = 0; i < kCpdSums; ++i) acc[i] = 0.0;
    for (int n0 = 0; n0 < N; n0 += kCpdThreads) {  // (trip counts depend on N and M alone: uniform over the workgroup)
      const int n = n0 + tid;
      const bool live = n < N;
      const double x0 = live ? Xb[n * 3 + 0] : 0.0, x1 = live ? Xb[n * 3 + 1] : 0.0, x2 = live ? Xb[n * 3 + 2] : 0.0;
      double c = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0, vq = 0.0;
      for (int m0 = 0; m0 < M; m0 += kCpdTile) {
        const int cnt = M - m0 < kCpdTile ? M - m0 : kCpdTile;
        if (tid < cnt) {
          const double* y = Yb + (m0 + tid) * 3;
          const double y0 = y[0], y1 = y[1], y2 = y[2];
#pragma unroll
          for (int j = 0; j < 3; ++j) tile[tid][j] = s * (y0 * R.a[0][j] + y1 * R.a[1][j] + y2 * R.a[2][j]) + t[j];
          const double e0 = y0 - cY[0], e1 = y1 - cY[1], e2 = y2 - cY[2];
          tile[tid][3] = e0, tile[tid][4] = e1, tile[tid][5] = e2;
          tile[tid][6] = e0 * e0 + e1 * e1 + e2 * e2;
        }
        __syncthreads();
        if (live) {
          for (int i = 0; i < cnt; ++i) {
            const double d0 = x0 - tile[i][0], d1 = x1 - tile[i][1], d2 = x2 - tile[i][2];
            const double e = exp((d0 * d0 + d1 * d1 + d2 * d2) * neg_inv_two_s2);
            c += e;
            v0 += e * tile[i][3], v1 += e * tile[i][4], v2 += e * tile[i][5];
            vq += e * tile[i][6];
          }
        }
        __syncthreads();
      }
      if (live) {
        const double den = fmax(c, DBL_EPSILON) + cc;
        const double pt1 = c / den;
        const double py[3] = {v0 / den, v1 / den, v2 / den};
        const double xs[3] = {x0 - cX[0], x1 - cX[1], x2 - cX[2]};
        acc[0] += pt1;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          acc[1 + i] += pt1 * xs[i];
          acc[4 + i] += py[i];
#pragma unroll
          for (int j = 0; j < 3; ++j) acc[7 + i * 3 + j] += xs[i] * py[j];
        }
        acc[16] += pt1 * (xs[0] * xs[0] + xs[1] * xs[1] + xs[2] * xs[2]);
        acc[17] += vq / den;
      }
    }
    block_reduce<kCpdSums>(acc, red, SumOp());
    // ---- M-step and variance, in every thread (the same arithmetic on the same values) ----
    const double Np = acc[0];
    double dX[3], dY[3], muX[3], muY[3];  // the means about the shifts, and the means
#pragma unroll
    for (int i = 0; i < 3; ++i) dX[i] = acc[1 + i] / Np, dY[i] = acc[4 + i] / Np, muX[i] = cX[i] + dX[i], muY[i] = cY[i] + dY[i];
    M3 A, U, V;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) A.a[i][j] = acc[7 + i * 3 + j] - Np * dX[i] * dY[j];
    const double xPx = acc[16] - Np * (dX[0] * dX[0] + dX[1] * dX[1] + dX[2] * dX[2]);
    const double YPY = acc[17] - Np * (dY[0] * dY[0] + dY[1] * dY[1] + dY[2] * dY[2]);
    double sv[3];
    svd3(A, U, sv, V);
    M3 UVt;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) UVt.a[i][j] = U.a[i][0] * V.a[j][0] + U.a[i][1] * V.a[j][1] + U.a[i][2] * V.a[j][2];
    const double dt = det3(UVt);
    // R = (U diag(1, 1, det(U V^T)) V^T)^T
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R.a[j][i] = U.a[i][0] * V.a[j][0] + U.a[i][1] * V.a[j][1] + dt * U.a[i][2] * V.a[j][2];
    double trAR = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) trAR += A.a[i][j] * R.a[j][i];
    s = fit_scale ? trAR / YPY : 1.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = muX[i] - s * (R.a[0][i] * muY[0] + R.a[1][i] * muY[1] + R.a[2][i] * muY[2]);
    const double q_new = (xPx - 2.0 * s * trAR + s * s * YPY) / (2.0 * sigma2) + 1.5 * Np * log(sigma2);
    diff = fabs(q_new - q);
    q = q_new;
    sigma2 = (xPx - s * trAR) / (3.0 * Np);
    if (sigma2 <= 0.0) sigma2 = tolerance / 10.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) cX[i] = muX[i], cY[i] = muY[i];
    if (tid == 0) {
      if (sigma2_trace) sigma2_trace[b * max_iterations + it] = sigma2;
      go_sh = diff > tolerance ? 1 : 0;  // (a NaN diff ends the loop, as NaN > tolerance is false)
    }
    ++it;
    __syncthreads();
  }
  if (tid == 0) {
    s_out[b] = s, sigma2_out[b] = sigma2, q_out[b] = q, diff_out[b] = diff, iterations_out[b] = it;
    for (int i = 0; i < 3; ++i) {
      t_out[b * 3 + i] = t[i];
      for (int j = 0; j < 3; ++j) R_out[b * 9 + i * 3 + j] = R.a[i][j];
    }
  }
}

// ---- gpn_joint_from_rigid -----------------------------------------------------------------------------------------------------
// rotation matrix -> unit quaternion (x, y, z, w), the branch by the largest of (m00, m11, m22, trace) as scipy's from_matrix
__device__ void quat_from_matrix(const double* m, double (&qv)[4]) {
  const double tr = m[0] + m[4] + m[8];
  const double dec[4] = {m[0], m[4], m[8], tr};
  int choice = 0;
  for (int i = 1; i < 4; ++i)
    if (dec[i] > dec[choice]) choice = i;
  if (choice != 3) {
    const int i = choice, j = (i + 1) % 3, k = (j + 1) % 3;
    qv[i] = 1.0 - tr + 2.0 * m[i * 3 + i];
    qv[j] = m[j * 3 + i] + m[i * 3 + j];
    qv[k] = m[k * 3 + i] + m[i * 3 + k];
    qv[3] = m[k * 3 + j] - m[j * 3 + k];
  } else {
    qv[0] = m[7] - m[5];
    qv[1] = m[2] - m[6];
    qv[2] = m[3] - m[1];
    qv[3] = 1.0 + tr;
  }
  const double nrm = sqrt(qv[0] * qv[0] + qv[1] * qv[1] + qv[2] * qv[2] + qv[3] * qv[3]);
  for (int i = 0; i < 4; ++i) qv[i] /= nrm;
}

__global__ __launch_bounds__(64) void joint_from_rigid_kernel(const double* __restrict__ rotation, const double* __restrict__ translation,
                                                             const double* __restrict__ norm, int64_t G, int joint_type,
                                                             double* __restrict__ axis, double* __restrict__ pivot,
                                                             double* __restrict__ angle_out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const double S = norm[g * 4], Mv[3] = {norm[g * 4 + 1], norm[g * 4 + 2], norm[g * 4 + 3]};
  const double tv[3] = {translation[g * 3], translation[g * 3 + 1], translation[g * 3 + 2]};
  if (joint_type == GPN_JOINT_PRISMATIC) {
    const double len = sqrt(tv[0] * tv[0] + tv[1] * tv[1] + tv[2] * tv[2]);
    for (int c = 0; c < 3; ++c) axis[g * 3 + c] = tv[c] / len, pivot[g * 3 + c] = Mv[c];
    angle_out[g] = len * S;
    return;
  }
  double qv[4];
  quat_from_matrix(rotation + g * 9, qv);
  if (qv[3] < 0.0)
    for (int i = 0; i < 4; ++i) qv[i] = -qv[i];
  // as_rotvec: angle = 2 atan2(|xyz|, w); rotvec = xyz * angle / sin(angle / 2) (a series below 1e-3)
  const double ang = 2.0 * atan2(sqrt(qv[0] * qv[0] + qv[1] * qv[1] + qv[2] * qv[2]), qv[3]);
  double sc;
  if (ang <= 1e-3) {
    const double a2 = ang * ang;
    sc = 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0;
  } else {
    sc = ang / sin(ang / 2.0);
  }
  const double rv[3] = {sc * qv[0], sc * qv[1], sc * qv[2]};
  const double angle = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
  const double ax[3] = {rv[0] / angle, rv[1] / angle, rv[2] / angle};  // (angle == 0: NaN, as in the reference)
  // r = the matrix of the rotation vector (pi / 2 - angle / 2) * axis  (from_rotvec, then as_matrix)
  const double hv[3] = {(M_PI / 2.0 - angle / 2.0) * ax[0], (M_PI / 2.0 - angle / 2.0) * ax[1], (M_PI / 2.0 - angle / 2.0) * ax[2]};
  const double ha = sqrt(hv[0] * hv[0] + hv[1] * hv[1] + hv[2] * hv[2]);
  double hs;
  if (ha <= 1e-3) {
    const double a2 = ha * ha;
    hs = 0.5 - a2 / 48.0 + a2 * a2 / 3840.0;
  } else {
    hs = sin(ha / 2.0) / ha;
  }
  const double x = hs * hv[0], y = hs * hv[1], z = hs * hv[2], wq = cos(ha / 2.0);
  const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = wq * wq, xy = x * y, zw = z * wq, xz = x * z, yw = y * wq, yz = y * z, xw = x * wq;
  const double r[3][3] = {{x2 - y2 - z2 + w2, 2.0 * (xy - zw), 2.0 * (xz + yw)},
                          {2.0 * (xy + zw), -x2 + y2 - z2 + w2, 2.0 * (yz - xw)},
                          {2.0 * (xz - yw), 2.0 * (yz + xw), -x2 - y2 + z2 + w2}};
  const double sh = sin(angle / 2.0);
  for (int j = 0; j < 3; ++j) {
    const double tr_j = tv[0] * r[0][j] + tv[1] * r[1][j] + tv[2] * r[2][j];
    axis[g * 3 + j] = ax[j];
    pivot[g * 3 + j] = tr_j / 2.0 / sh * S + Mv[j];
  }
  angle_out[g] = angle;
}

}  // namespace

// pc1 [n1_total,3] / pc2 [n2_total,3] f64 (pair b = rows off[b]:off[b+1]), picks [B,K] i64 (rows inside the pair's segment),
// k1 / k2 [B] i32 (live picks of the row) -> X, Y [B,K,3] (zero beyond k), norm [B,4] = (S, Mx, My, Mz)
extern "C" int gpn_joint_sample(const double* pc1, const double* pc2, const int64_t* off1, const int64_t* off2, const int64_t* picks1,
                                const int64_t* picks2, const int32_t* k1, const int32_t* k2, int64_t B, int K, double* X, double* Y,
                                double* norm, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(B >= 0 && B <= 0x7fffffff && K >= 1 && K <= GPN_JOINT_MAX_K);
  if (B == 0) return GPN_OK;
  GPN_CHECK_ARG(off1 && off2 && picks1 && picks2 && k1 && k2 && X && Y && norm);
  hipLaunchKernelGGL(joint_sample_kernel, dim3((unsigned)B), dim3(kSampleThreads), 0, stream, pc1, pc2, off1, off2, picks1, picks2,
                     k1, k2, K, X, Y, norm);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_cpd_rigid(const double* X, const double* Y, const int32_t* nx, const int32_t* ny, int64_t B, int K,
                             int max_iterations, double tolerance, double w, int scale, double* s, double* R, double* t,
                             double* sigma2, double* q, double* diff, int32_t* iterations, double* sigma2_trace,
                             gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(B >= 0 && B <= 0x7fffffff && K >= 1 && K <= GPN_JOINT_MAX_K && max_iterations >= 0);
  GPN_CHECK_ARG(w >= 0.0 && w < 1.0);
  if (B == 0) return GPN_OK;
  GPN_CHECK_ARG(X && Y && nx && ny && s && R && t && sigma2 && q && diff && iterations);
  hipLaunchKernelGGL(cpd_rigid_kernel, dim3((unsigned)B), dim3(kCpdThreads), 0, stream, X, Y, nx, ny, K, max_iterations, tolerance, w,
                     scale ? 1 : 0, s, R, t, sigma2, q, diff, iterations, sigma2_trace);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}

extern "C" int gpn_joint_from_rigid(const double* rotation, const double* translation, const double* norm, int64_t G, int joint_type,
                                    double* axis, double* pivot, double* angle, gpn_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GPN_CHECK_ARG(G >= 0 && (joint_type == GPN_JOINT_REVOLUTE || joint_type == GPN_JOINT_PRISMATIC));
  if (G == 0) return GPN_OK;
  GPN_CHECK_ARG(rotation && translation && norm && axis && pivot && angle);
  hipLaunchKernelGGL(joint_from_rigid_kernel, dim3((unsigned)gpn::cdiv(G, 64)), dim3(64), 0, stream, rotation, translation, norm, G,
                     joint_type, axis, pivot, angle);
  GPN_CHECK_LAUNCH();
  return GPN_OK;
}
