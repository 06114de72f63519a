/* gaussreg_hip_train_matching.h -- the training entry points of the matching stage of libgaussreg_hip.so.  They came after
 * include/gaussreg_hip.h and include/gaussreg_hip_train.h were closed at their present symbol counts.  Same library, same
 * conventions (gaussreg_hip.h, top): device pointers unless a name starts with h_, status codes GR_OK / GR_ERR_*,
 * gr_last_error() for the text, asynchronous on `stream`, no hidden allocation (the caller passes the workspace the
 * *_workspace_bytes query asks for).  The binding reads this header with the parser that reads gaussreg_hip.h
 * (gaussreg_amd/_lib.py: MATCH_TRAIN_SIGNATURES / MATCH_TRAIN_DEFINES).
 */
#ifndef GAUSSREG_HIP_TRAIN_MATCHING_H_
#define GAUSSREG_HIP_TRAIN_MATCHING_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* gr_sinkhorn_backward: the gradients of gr_sinkhorn (LearnableLogOptimalTransport.forward, num_iterations fixed log-domain
 * Sinkhorn steps on the matrix padded with the dustbin row and column) with respect to the scores and to alpha, in one
 * launch.  scores (batch, m, n), row_masks (batch, m) / col_masks (batch, n) (1 = valid, null = all valid), alpha_dev,
 * num_iterations, inf: the forward's arguments.
 * grad_out: the gradient of the forward's output, (batch, m+1, n+1); with drop_dustbin != 0 it is (batch, m, n) and the
 * dustbin row and column have no upstream gradient.  Entries of grad_out on masked rows or columns are never used (they are
 * selected away, not multiplied: a NaN there reaches no output).
 * grad_scores (batch, m, n): every element is written, exact 0.0f on masked rows and columns.
 * grad_alpha_per_matrix (batch): the sum of the padded matrix's gradient over the dustbin row, dustbin column and corner of
 * each matrix; the caller adds the batch up.  No float atomics: two calls leave the same bits, and a matrix gives the same
 * bits whatever batch it is part of.
 * num_iterations == 0: grad_scores = grad_out on the live entries, grad_alpha = its dustbin sum.  batch == 0: GR_OK, no launch.
 * One 512-thread workgroup per matrix repeats the forward iterations, keeps every u^t, v^t in a history slot of the
 * workspace and sweeps back (csrc/sinkhorn.hip); at most 512 workgroups walk the batch, a slot per workgroup:
 *   workspace bytes = 4 * min(batch, 512) * roundup64(num_iterations * (m + 1 + n + 1)) + 256
 * -- bounded by the grid, not by the batch.  Refused before any launch: max(m, n) + 1 > 144, null pointers, a workspace that
 * is too small, an LDS need above 160 KB.  gr_timing_* name: "sinkhorn_backward". */
/* host only; 0 for a shape the call refuses */
size_t gr_sinkhorn_backward_workspace_bytes(int64_t batch, int64_t m, int64_t n, int num_iterations);
int gr_sinkhorn_backward(const float* scores, int64_t batch, int64_t m, int64_t n, const uint8_t* row_masks,
                         const uint8_t* col_masks, const float* alpha_dev, int num_iterations, float inf, int drop_dustbin,
                         const float* grad_out, float* grad_scores, float* grad_alpha_per_matrix, void* ws, size_t ws_bytes,
                         void* stream);

/* gr_node_correspondences: the ground-truth superpoint correspondences of a training step (get_node_correspondences,
 * geotransformer/modules/registration/matching.py:231-315) without the reference's per-pair (B, K, K) / (B, K, 3) tensors.
 * ref_nodes (m,3), src_nodes (n,3), ref_knn_points (m,k,3), src_knn_points (n,k,3); transform_dev: the 4 x 4 row-major
 * transform of the source, on the device; pos_radius_sq: the squared positive radius as the fp32 value the comparison
 * uses.  ref_masks (m) / src_masks (n) / ref_knn_masks (m,k) / src_knn_masks (n,k): 1 = valid, null = all valid.
 * A point pair matches when |p - (R q + t)|^2 < pos_radius_sq, evaluated as differences, then squares, in fp32 without
 * FMA; only valid points of valid nodes take part.  overlap(i, j) = (ref_count / ref_valid + src_count / src_valid) / 2 in
 * fp32 in this order, the counts being the points that have at least one partner; a pair where one side has no valid
 * point has overlap 0.  The pairs with overlap > 0 leave in row-major (ref, src) order:
 *   corr_indices (capacity, 2) int64, corr_overlaps (capacity): rows [0, min(C, capacity)) are written, nothing else;
 *   count_dev: one int64 on the device, C itself -- the caller repeats with a larger buffer when C > capacity
 *   (capacity = m * n always suffices; capacity == 0 allows null corr_* pointers);
 *   dense_overlaps (m, n) or null: the whole overlap matrix, every element written (0 where the pair does not overlap).
 * The enclosing-sphere test of the reference only prunes; here it is widened so that it never rejects a pair with a match.
 * No float atomics, no atomics for ordering: two calls leave the same bits.  Three kernels and a scan (csrc/
 * node_correspondences.hip); workspace = the transformed source patches, per-node records and the (m, n) overlap matrix:
 *   about 4 * (m * n + 3 * n * k) + 24 * (m + n) bytes -- O(m n + n k).
 * m, n or k == 0: GR_OK, *count_dev = 0, no kernel.  Refused before any launch: k > 256 (GR_ERR_UNSUPPORTED), m * n >= 2^31,
 * null pointers, a workspace that is too small (GR_ERR_WORKSPACE).  gr_timing_* name: "node_correspondences". */
/* host only; 0 for a shape the call refuses */
size_t gr_node_correspondences_workspace_bytes(int64_t m, int64_t n, int64_t k);
int gr_node_correspondences(const float* ref_nodes, const float* src_nodes, const float* ref_knn_points,
                            const float* src_knn_points, int64_t m, int64_t n, int64_t k, const float* transform_dev,
                            float pos_radius_sq, const uint8_t* ref_masks, const uint8_t* src_masks,
                            const uint8_t* ref_knn_masks, const uint8_t* src_knn_masks, int64_t* corr_indices,
                            float* corr_overlaps, int64_t capacity, int64_t* count_dev, float* dense_overlaps, void* ws,
                            size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GAUSSREG_HIP_TRAIN_MATCHING_H_ */
