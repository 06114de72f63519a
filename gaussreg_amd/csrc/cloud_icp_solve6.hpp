// The 6x6 solve-and-compose that point-to-plane ICP (cloud_icp_plane.hip) and generalised ICP
// (cloud_icp_gicp.hip, 3.15) share.  Both keep their sums in one layout: n, S, the upper triangle of H row by row (21), g (6).
#pragma once
#include <cmath>

namespace gr {
namespace {

constexpr int P_H = 2, P_G = 23;
constexpr int PLANE_SWEEPS = 32;

// thread 0 of icp_fold_kernel: H = V diag(l) V^T by a cyclic Jacobi eigen-decomposition whose matrices live in LDS (run-time
// row and column indices, so not in registers), refuses l_min <= 1e-12 l_max, x = -V diag(1 / l) V^T g, dR = Rz Ry Rx and
// Tn = fl32(dT . double(T)).  __forceinline__: each estimator's fold kernel holds its own copy of the LDS matrices.
__device__ __forceinline__ bool solve6_compose(const double* sum, const float* T, float* Tn) {
  __shared__ double Hm[36], Vm[36], ys[6], xs[6];  // thread 0's 6x6 solve: indexed at run time, so in LDS
  // H and V = I
  int e = P_H;
  double fro2 = 0.0;
  for (int c = 0; c < 6; ++c)
    for (int d = c; d < 6; ++d) {
      const double h = sum[e++];
      Hm[c * 6 + d] = Hm[d * 6 + c] = h;
      fro2 += (c == d ? 1.0 : 2.0) * h * h;
    }
  for (int k = 0; k < 36; ++k) Vm[k] = (k % 7 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < PLANE_SWEEPS; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 5; ++p)
      for (int r = p + 1; r < 6; ++r) off += Hm[p * 6 + r] * Hm[p * 6 + r];
    if (off <= 1e-30 * fro2) break;
#pragma unroll 1
    for (int p = 0; p < 5; ++p) {
#pragma unroll 1
      for (int r = p + 1; r < 6; ++r) {
        const double hpr = Hm[p * 6 + r];
        if (fabs(hpr) < 1e-300) continue;
        const double theta = (Hm[r * 6 + r] - Hm[p * 6 + p]) / (2.0 * hpr);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 6; ++k) {
          const double a = Hm[k * 6 + p], b = Hm[k * 6 + r];
          Hm[k * 6 + p] = c * a - s * b;
          Hm[k * 6 + r] = s * a + c * b;
        }
        for (int k = 0; k < 6; ++k) {
          const double a = Hm[p * 6 + k], b = Hm[r * 6 + k];
          Hm[p * 6 + k] = c * a - s * b;
          Hm[r * 6 + k] = s * a + c * b;
        }
        for (int k = 0; k < 6; ++k) {
          const double a = Vm[k * 6 + p], b = Vm[k * 6 + r];
          Vm[k * 6 + p] = c * a - s * b;
          Vm[k * 6 + r] = s * a + c * b;
        }
      }
    }
  }
  double lmin = Hm[0], lmax = Hm[0];
  for (int k = 1; k < 6; ++k) {
    lmin = fmin(lmin, Hm[k * 7]);
    lmax = fmax(lmax, Hm[k * 7]);
  }
  if (!(lmin > 1e-12 * lmax)) return false;  // a NaN as well
  for (int k = 0; k < 6; ++k) {  // y = diag(1 / l) V^T g
    double a = 0.0;
    for (int j = 0; j < 6; ++j) a += Vm[j * 6 + k] * sum[P_G + j];
    ys[k] = a / Hm[k * 7];
  }
  for (int i = 0; i < 6; ++i) {  // x = -V y
    double a = 0.0;
    for (int k = 0; k < 6; ++k) a += Vm[i * 6 + k] * ys[k];
    xs[i] = -a;
  }
  const double ca = cos(xs[0]), sa = sin(xs[0]), cb = cos(xs[1]), sb = sin(xs[1]), cg = cos(xs[2]), sg = sin(xs[2]);
  // dR = Rz(gamma) Ry(beta) Rx(alpha)
  const double dR[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                        sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                        -sb,     cb * sa,                cb * ca};
  const double dt[3] = {xs[3], xs[4], xs[5]};
  double A[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) A[k] = (double)T[k];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double a = (dR[r * 3] * A[c] + dR[r * 3 + 1] * A[4 + c]) + dR[r * 3 + 2] * A[8 + c];
      if (c == 3) a += dt[r];
      Tn[r * 4 + c] = (float)a;
    }
  }
  return true;
}

}  // namespace
}  // namespace gr
