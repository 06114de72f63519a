// The fp64 similarity fit from sums, shared by ransac.hip (hypotheses and the refit) and cloud_icp.hip (the update of an
// ICP iteration): Horn's quaternion rotation by a Jacobi eigen-solve of the 4x4 matrix, scale = sum(ref_c . R src_c) /
// sum |src_c|^2, the 3x4 result rounded once to fp32.
#pragma once
#include "common.hpp"

namespace gr {
namespace {

__device__ void jacobi_maxvec4(double A[4][4], double* q) {
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  double fro2 = 0.0;  // stop at fp64 resolution of the matrix (see lgr.hip)
  for (int p = 0; p < 4; ++p)
    for (int r = 0; r < 4; ++r) fro2 += A[p][r] * A[p][r];
  for (int sweep = 0; sweep < 16; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 4; ++p)
      for (int r = p + 1; r < 4; ++r) off += A[p][r] * A[p][r];
    if (off <= 1e-30 * fro2) break;
    for (int p = 0; p < 3; ++p)
      for (int r = p + 1; r < 4; ++r) {
        if (fabs(A[p][r]) < 1e-300) continue;
        const double theta = (A[r][r] - A[p][p]) / (2.0 * A[p][r]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) { const double a = A[k][p], b = A[k][r]; A[k][p] = c * a - s * b; A[k][r] = s * a + c * b; }
        for (int k = 0; k < 4; ++k) { const double a = A[p][k], b = A[r][k]; A[p][k] = c * a - s * b; A[r][k] = s * a + c * b; }
        for (int k = 0; k < 4; ++k) { const double a = V[k][p], b = V[k][r]; V[k][p] = c * a - s * b; V[k][r] = s * a + c * b; }
      }
  }
  // the column of the largest diagonal entry (the first among equals), picked by selects: an index that is only known at
  // run time would put V into scratch memory
  int best = 0;
  double top = A[0][0];
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > top) { best = k; top = A[k][k]; }
  double n = 0;
  for (int k = 0; k < 4; ++k) {
    q[k] = best == 0 ? V[k][0] : best == 1 ? V[k][1] : best == 2 ? V[k][2] : V[k][3];
    n += q[k] * q[k];
  }
  n = sqrt(n);
  for (int k = 0; k < 4; ++k) q[k] /= n;
}

// Umeyama similarity from sums: n, sum src, sum ref, sum src_a*ref_b (9), sum |src|^2  ->  T (3x4: sR | t)
__device__ bool umeyama_from_sums(double n, const double* ss, const double* sr, const double* sxy, double s2, int with_scale,
                                  float* T) {
  if (n < 1.0) return false;
  double cs[3], cr[3], H[9];
  for (int k = 0; k < 3; ++k) { cs[k] = ss[k] / n; cr[k] = sr[k] / n; }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) H[a * 3 + b] = sxy[a * 3 + b] - n * cs[a] * cr[b];  // sum (src-cs)_a (ref-cr)_b
  const double var = s2 - n * (cs[0] * cs[0] + cs[1] * cs[1] + cs[2] * cs[2]);
  double A[4][4] = {{H[0] + H[4] + H[8], H[5] - H[7], H[6] - H[2], H[1] - H[3]},
                    {H[5] - H[7], H[0] - H[4] - H[8], H[1] + H[3], H[6] + H[2]},
                    {H[6] - H[2], H[1] + H[3], -H[0] + H[4] - H[8], H[5] + H[7]},
                    {H[1] - H[3], H[6] + H[2], H[5] + H[7], -H[0] - H[4] + H[8]}};
  double q[4];
  jacobi_maxvec4(A, q);
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                       2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
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
