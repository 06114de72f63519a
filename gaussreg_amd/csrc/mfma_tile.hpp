// The fp32 matrix-core tile shared by the GEMM-shaped kernels (pairwise distance, the KPConv products forward and backward,
// the geometric embedding): v_mfma_f32_32x32x2_f32 fed from a padded LDS slab.  Device-only.
//
// One instruction computes D (32 x 32) = A (32 x 2) . B (2 x 32) + C per WAVE.  Operands, one float per lane:
//   A: lane l holds A[i = l & 31][k = l >> 5]           B: lane l holds B[k = l >> 5][j = l & 31]
// so with both matrices staged k-fast in LDS (s[row][k], row = the i of A / the j of B) the two fetches are the same
// expression, s[origin + (l & 31)][k + (l >> 5)].  C / D, sixteen floats per lane (register r = 0..15):
//   column = l & 31,   row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)
// i.e. a lane owns one column and four groups of four consecutive rows, the two half-waves interleaved by four rows.  Every
// 32 x 32 MFMA of gfx950 uses this C / D layout whatever its operand type.  The accumulation of one output element is an fmaf
// chain over k in the order the instructions are issued (ascending here), which is what makes the kernels' bits comparable.
#pragma once
#include "common.hpp"

namespace gr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int TA, int TB>
__device__ __forceinline__ void mfma_zero(f32x16 (&acc)[TA][TB]) {
#pragma unroll
  for (int a = 0; a < TA; ++a)
#pragma unroll
    for (int b = 0; b < TB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
}

// C / D layout: the row of register r and the column of a lane, for the 32 x 32 block whose first row / column is `origin`
// (int or int64_t, as the kernel counts its rows)
template <class T>
__device__ __forceinline__ T mfma_row(T origin, int r, int lane) { return origin + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ int mfma_col(int origin, int lane) { return origin + (lane & 31); }

// acc[a][b] += A block (rows wi + 32 a ..) . B block (rows wj + 32 b ..) over the BK columns of one slab, k ascending in
// steps of two: the TA A fragments, the TB B fragments, then the MFMAs in (a, b) row-major order.
// sa / sb must be LDS (__shared__) slabs: the fetches are typed as such here, which keeps them ds_read even where the slab is
// chosen at run time (sa[buf] of a double buffer).
template <int BK, int TA, int TB, int LD>
__device__ __forceinline__ void mfma_slab(f32x16 (&acc)[TA][TB], const float (*sa)[LD], const float (*sb)[LD], int wi, int wj,
                                          int lane) {
  typedef const __attribute__((address_space(3))) float (*lds_rows)[LD];
  const lds_rows la = (lds_rows)sa, lb = (lds_rows)sb;
#pragma unroll
  for (int k = 0; k < BK; k += 2) {
    const int kk = k + (lane >> 5), rr = lane & 31;
    float av[TA], bv[TB];
#pragma unroll
    for (int a = 0; a < TA; ++a) av[a] = la[wi + 32 * a + rr][kk];
#pragma unroll
    for (int b = 0; b < TB; ++b) bv[b] = lb[wj + 32 * b + rr][kk];
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
      for (int b = 0; b < TB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
  }
}

// ---- the 64 x 64 single-buffer product: 256 threads, 2 x 2 waves of one 32 x 32 accumulator, k slabs of 32 through one
// padded LDS buffer per operand.  C (Mi x Nj) = A . B over k in [kb, ke) for the tile (blockIdx.y, blockIdx.x):
//   A(i,k) = A_KFAST ? A[i lda + k] : A[k lda + i]      B(k,j) = B_KFAST ? B[j ldb + k] : B[k ldb + j]
// The staging loops run along whichever index is contiguous in memory.  STAGE_DIV: the operands are divided while they are
// staged, A(i,k) / denA[i] and B(k,j) / denB[k], each when its pointer is given.  ld_t: the type of the strides at the call
// site (a kernel with int sizes keeps its 32-bit index arithmetic).  epi(gi, gj, v) receives every element inside Mi x Nj; give
// it its pointers by copy ([=]): captured by reference they are re-read after every store.
constexpr int GT = 64, GK = 32, GLD = GK + 1;

template <bool A_KFAST, bool B_KFAST, bool STAGE_DIV, typename ld_t, typename Epi>
__device__ __forceinline__ void gemm64_tile(const float* A, ld_t lda, const float* B, ld_t ldb, int Mi,
                                            int Nj, int kb, int ke, const float* denA,
                                            const float* denB, Epi epi) {
  __shared__ float sa[GT][GLD];
  __shared__ float sb[GT][GLD];
  const int i0 = blockIdx.y * GT, j0 = blockIdx.x * GT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wi = (w >> 1) * 32, wj = (w & 1) * 32;
  f32x16 acc[1][1];
  mfma_zero(acc);
  for (int k0 = kb; k0 < ke; k0 += GK) {
    for (int e = tid; e < GT * GK; e += 256) {
      {
        const int r = A_KFAST ? e / GK : e % GT, k = A_KFAST ? e % GK : e / GT;
        const int gi = i0 + r, gk = k0 + k;
        float v = 0.f;
        if (gi < Mi && gk < ke) {
          v = A_KFAST ? A[(int64_t)gi * lda + gk] : A[(int64_t)gk * lda + gi];
          if (STAGE_DIV && denA) v = v / denA[gi];
        }
        sa[r][k] = v;
      }
      {
        const int r = B_KFAST ? e / GK : e % GT, k = B_KFAST ? e % GK : e / GT;
        const int gj = j0 + r, gk = k0 + k;
        float v = 0.f;
        if (gj < Nj && gk < ke) {
          v = B_KFAST ? B[(int64_t)gj * ldb + gk] : B[(int64_t)gk * ldb + gj];
          if (STAGE_DIV && denB) v = v / denB[gk];
        }
        sb[r][k] = v;
      }
    }
    __syncthreads();
    mfma_slab<GK>(acc, sa, sb, wi, wj, lane);
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int gi = mfma_row(i0 + wi, r, lane), gj = mfma_col(j0 + wj, lane);
    if (gi < Mi && gj < Nj) epi(gi, gj, acc[0][0][r]);
  }
}

}  // namespace gr
