// The fp64 fits that are solved in one thread's registers: the cyclic Jacobi rotation for a small symmetric matrix
// (cloud_normals.hip at 3x3, Horn's quaternion matrix here at 4x4), the rotation of a 3x3 covariance (lgr.hip and the fit
// below), and the similarity fit from sums of ransac.hip (hypotheses and the refit) and cloud_icp.hip (the update of an ICP
// iteration): scale = sum(ref_c . R src_c) / sum |src_c|^2, the 3x4 result rounded once to fp32.
#pragma once
#include "common.hpp"

namespace gr {
namespace {

// A (symmetric, destroyed) -> eigenvalues on its diagonal, eigenvectors in the columns of V.  Every index is known at
// compile time: one that is only known at run time would put the matrices into scratch memory, so callers pick a column
// of V by selects.  It stops at fp64 resolution of the matrix -- off-diagonal mass below 1e-15 of the Frobenius norm:
// waiting for it to underflow costs four more sweeps of serial fp64 work in the one thread that runs this.
template <int N, int SWEEPS>
__device__ void jacobi_sym(double (&A)[N][N], double (&V)[N][N]) {
  double fro2 = 0.0;
#pragma unroll
  for (int p = 0; p < N; ++p)
#pragma unroll
    for (int r = 0; r < N; ++r) {
      V[p][r] = p == r ? 1.0 : 0.0;
      fro2 += A[p][r] * A[p][r];
    }
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
    double off = 0.0;
#pragma unroll
    for (int p = 0; p < N; ++p)
#pragma unroll
      for (int r = p + 1; r < N; ++r) off += A[p][r] * A[p][r];
    if (off <= 1e-30 * fro2) break;
    // the pair loops unroll fully as well, but are left to the compiler: forcing them with the pragma costs the 4x4
    // callers 22 VGPRs and a wave per SIMD (icp_fold_kernel, ransac_hypotheses_kernel: 148 against 126)
    for (int p = 0; p < N - 1; ++p)
      for (int r = p + 1; r < N; ++r) {
        if (fabs(A[p][r]) < 1e-300) continue;
        const double theta = (A[r][r] - A[p][p]) / (2.0 * A[p][r]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < N; ++k) { const double a = A[k][p], b = A[k][r]; A[k][p] = c * a - s * b; A[k][r] = s * a + c * b; }
#pragma unroll
        for (int k = 0; k < N; ++k) { const double a = A[p][k], b = A[r][k]; A[p][k] = c * a - s * b; A[r][k] = s * a + c * b; }
#pragma unroll
        for (int k = 0; k < N; ++k) { const double a = V[k][p], b = V[k][r]; V[k][p] = c * a - s * b; V[k][r] = s * a + c * b; }
      }
  }
}

// The proper rotation R (3x3) maximising tr(R H), H[a][b] = sum w src_a ref_b: Horn's unit quaternion, the eigenvector of
// the largest eigenvalue (the first among equals) of a symmetric 4x4 built from H
__device__ void rotation_from_covariance(const double* H, double* R) {
  double A[4][4] = {{H[0] + H[4] + H[8], H[5] - H[7], H[6] - H[2], H[1] - H[3]},
                    {H[5] - H[7], H[0] - H[4] - H[8], H[1] + H[3], H[6] + H[2]},
                    {H[6] - H[2], H[1] + H[3], -H[0] + H[4] - H[8], H[5] + H[7]},
                    {H[1] - H[3], H[6] + H[2], H[5] + H[7], -H[0] - H[4] + H[8]}};
  double V[4][4];
  jacobi_sym<4, 16>(A, V);
  int best = 0;
  double top = A[0][0];
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > top) { best = k; top = A[k][k]; }
  double q[4], n = 0;
  for (int k = 0; k < 4; ++k) {
    q[k] = best == 0 ? V[k][0] : best == 1 ? V[k][1] : best == 2 ? V[k][2] : V[k][3];
    n += q[k] * q[k];
  }
  n = sqrt(n);
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}

// Umeyama similarity from sums: n, sum src, sum ref, sum src_a*ref_b (9), sum |src|^2  ->  T (3x4: sR | t)
__device__ bool umeyama_from_sums(double n, const double* ss, const double* sr, const double* sxy, double s2, int with_scale,
                                  float* T) {
  if (n < 1.0) return false;
  double cs[3], cr[3], H[9], R[9];
  for (int k = 0; k < 3; ++k) { cs[k] = ss[k] / n; cr[k] = sr[k] / n; }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) H[a * 3 + b] = sxy[a * 3 + b] - n * cs[a] * cr[b];  // sum (src-cs)_a (ref-cr)_b
  const double var = s2 - n * (cs[0] * cs[0] + cs[1] * cs[1] + cs[2] * cs[2]);
  rotation_from_covariance(H, R);
  double scale = 1.0;
  if (with_scale) {
    double tr = 0;  // sum_i ref_c . (R src_c) = sum_ab R[b][a] H[a][b]
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) tr += R[b * 3 + a] * H[a * 3 + b];
    if (!(var > 1e-300)) return false;
    scale = tr / var;
    if (!(scale > 0.0) || !isfinite(scale)) return false;
  }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[r * 4 + c] = (float)(scale * R[r * 3 + c]);
    T[r * 4 + 3] = (float)(cr[r] - scale * (R[r * 3] * cs[0] + R[r * 3 + 1] * cs[1] + R[r * 3 + 2] * cs[2]));
  }
  return true;
}

}  // namespace
}  // namespace gr
