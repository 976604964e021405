// pose_math.h - the float64 helpers shared by the pose kernels (pose.hip), the joint kernels (joint.hip) and the pose-evaluation
// kernels (poseeval.hip): the 3x3 matrix type, its determinant, the one-sided Jacobi SVD and the fixed-shape workgroup reduction.  Device code only; every function is internal to the including file.
#pragma once
#include "gpn_common.h"

namespace {

struct M3 {
  double a[3][3];
};

__device__ __forceinline__ double det3(const M3& m) {
  return m.a[0][0] * (m.a[1][1] * m.a[2][2] - m.a[1][2] * m.a[2][1]) - m.a[0][1] * (m.a[1][0] * m.a[2][2] - m.a[1][2] * m.a[2][0]) +
         m.a[0][2] * (m.a[1][0] * m.a[2][1] - m.a[1][1] * m.a[2][0]);
}

// A = U diag(S) V^T with S descending (one-sided Jacobi on the columns of A; zero singular values get unit vectors that
// complete the basis).  NaN input: NaN output.
__device__ void svd3(const M3& A, M3& U, double (&S)[3], M3& V) {
  double g[3][3], v[3][3];  // columns: g[col][row]
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) g[c][r] = A.a[r][c], v[c][r] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double al = g[p][0] * g[p][0] + g[p][1] * g[p][1] + g[p][2] * g[p][2];
      const double be = g[q][0] * g[q][0] + g[q][1] * g[q][1] + g[q][2] * g[q][2];
      const double ga = g[p][0] * g[q][0] + g[p][1] * g[q][1] + g[p][2] * g[q][2];
      if (fabs(ga) > 1e-17 * sqrt(al * be) && fabs(ga) > 0.0) {
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double gp = g[p][r], gq = g[q][r];
          g[p][r] = c * gp - s * gq;
          g[q][r] = s * gp + c * gq;
          const double vp = v[p][r], vq = v[q][r];
          v[p][r] = c * vp - s * vq;
          v[q][r] = s * vp + c * vq;
        }
      }
    }
    if (!rotated) break;
  }
  double sig[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) sig[c] = sqrt(g[c][0] * g[c][0] + g[c][1] * g[c][1] + g[c][2] * g[c][2]);
  // order: descending singular values (stable for ties)
  int ord[3] = {0, 1, 2};
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2 - i; ++j)
      if (sig[ord[j]] < sig[ord[j + 1]]) {
        const int t = ord[j];
        ord[j] = ord[j + 1];
        ord[j + 1] = t;
      }
  double u[3][3];
  const double tiny = 1e-300;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = ord[k];
    S[k] = sig[c];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      V.a[r][k] = v[c][r];
      u[k][r] = sig[c] > tiny ? g[c][r] / sig[c] : 0.0;
    }
  }
  // complete U where singular values vanished (rank 2: cross product; rank <= 1: any orthonormal completion)
  if (!(S[2] > tiny)) {
    if (!(S[1] > tiny)) {
      if (!(S[0] > tiny)) u[0][0] = 1.0, u[0][1] = 0.0, u[0][2] = 0.0;
      // a unit vector orthogonal to u0
      const int m = fabs(u[0][0]) <= fabs(u[0][1]) ? (fabs(u[0][0]) <= fabs(u[0][2]) ? 0 : 2) : (fabs(u[0][1]) <= fabs(u[0][2]) ? 1 : 2);
      double e[3] = {0.0, 0.0, 0.0};
      e[m] = 1.0;
      const double d = u[0][m];
      double w[3] = {e[0] - d * u[0][0], e[1] - d * u[0][1], e[2] - d * u[0][2]};
      const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
      u[1][0] = w[0] / n, u[1][1] = w[1] / n, u[1][2] = w[2] / n;
    }
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int r = 0; r < 3; ++r) U.a[r][k] = u[k][r];
}

struct SumOp {
  __device__ __forceinline__ double operator()(double a, double b) const { return a + b; }
};
struct MaxOp {
  __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};

// fixed-shape reduction of NV doubles per thread over the workgroup (blockDim.x a multiple of 64): a shuffle tree inside every
// wave, then the waves' partials in wave order; the result in every thread.  Every thread of the workgroup must call it.
template <int NV, typename Op>
__device__ __forceinline__ void block_reduce(double (&v)[NV], double* red /* [waves][NV] */, Op op) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double x = v[q];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = op(x, __shfl_down(x, off, 64));
    if (lane == 0) red[wave * NV + q] = x;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    double acc = red[q];
    for (int w = 1; w < waves; ++w) acc = op(acc, red[w * NV + q]);
    v[q] = acc;
  }
  __syncthreads();
}

}  // namespace
