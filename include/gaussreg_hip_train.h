/* gaussreg_hip_train.h -- the training entry points of libgaussreg_hip.so that came after include/gaussreg_hip.h was
 * closed at its present symbol count.  Same library, same conventions (gaussreg_hip.h, top): device pointers unless a name
 * starts with h_, status codes GR_OK / GR_ERR_*, gr_last_error() for the text, asynchronous on `stream`, no hidden
 * allocation (the caller passes the workspace the *_workspace_bytes query asks for).  The binding reads this header with the
 * parser that reads gaussreg_hip.h (gaussreg_amd/_lib.py: TRAIN_SIGNATURES / TRAIN_DEFINES).
 */
#ifndef GAUSSREG_HIP_TRAIN_H_
#define GAUSSREG_HIP_TRAIN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* gr_geo_embedding_backward: the gradients of GeometricStructureEmbedding.forward (gr_geo_embedding / gr_geo_embedding_table)
 * with respect to proj_d and proj_a for one cloud.  With out[r, :] = W_d phi(xd_r) + b_d + red_i (W_a phi(xa_{r,i}) + b_a),
 * r = (a, b) over the n * n pairs, and grad_out (n, n, c):
 *   grad_w_d[c, j] = sum_r go[r, c] phi_j(xd_r)            grad_b_d[c] = sum_r go[r, c]
 *   mean: grad_w_a[c, j] = sum_r go[r, c] (1 / k) sum_i phi_j(xa_{r,i})
 *   max:  grad_w_a[c, j] = sum_i sum_r [win(r, c) = i] go[r, c] phi_j(xa_{r,i})          grad_b_a = grad_b_d (angle_k > 0)
 * Three launches: the forward's neighbour kernel (the neighbour sets and the indices xd, xa are the forward's bit for bit:
 * the same device code), a GEMM kernel on the fp32 matrix cores whose workgroups own a slab of consecutive pairs and a tile of
 * output rows and write partial tiles to the workspace, and a reduction that adds the partials in ascending slab order.  No
 * float atomics: two calls leave the same bits.  How the pairs are cut depends on (n, c) only (gr_..._plan).
 * 'max' winners: the values of the forward's TABLE evaluation (tab_a: rows_a x c fp32, 16-byte aligned, step 1 / inv_h, as
 * for gr_geo_embedding_table; w_a, b_a serve an index beyond the table), the lowest i among equal values -- exactly the
 * winner of gr_geo_embedding_table; gr_geo_embedding's values differ from the table's by the interpolation error (~2e-8).
 * tab_a may be null for the mean or angle_k == 0.  grad_out must be 16-byte aligned, c % 32 == 0, 0 <= angle_k <= 8,
 * angle_k < n, n * n < 2^31: every refusal comes before the first launch.
 * accumulate == 0: the four gradients (c x c, c, c x c, c) are written; != 0: this cloud's sums are added to what they hold
 * (a batch is summed in index order without further launches).  n == 0: zeros (accumulate == 0) or nothing.  angle_k == 0:
 * grad_w_a / grad_b_a may be null; given, they get zeros (accumulate == 0) or stay.  Points get no gradient.
 * gr_timing_* name: "geo_embedding_backward" (launches 2 and 3 together). */
/* host only; 0 for a shape the call refuses */
size_t gr_geo_embedding_backward_workspace_bytes(int64_t n, int64_t c, int64_t angle_k);
/* host only: how the call is cut, for tests (as gr_kpconv_plan): the number of pair slabs, the pairs of a slab (a multiple of
 * 32; the last slab may be shorter) and the number of 64-row tiles of the outputs.  GR_ERR_INVALID for shapes the call refuses. */
int gr_geo_embedding_backward_plan(int64_t n, int64_t c, int64_t angle_k, int64_t* slabs, int64_t* pairs_per_slab,
                                   int64_t* c_tiles);
int gr_geo_embedding_backward(const float* points, int64_t n, const float* grad_out, const float* tab_a, int64_t rows_a,
                              float inv_h, const float* w_a, const float* b_a, const float* div_term, int64_t c,
                              float sigma_d, float factor_a, int64_t angle_k, int reduction_mean, int accumulate,
                              float* grad_w_d, float* grad_b_d, float* grad_w_a, float* grad_b_a, void* ws, size_t ws_bytes,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GAUSSREG_HIP_TRAIN_H_ */
