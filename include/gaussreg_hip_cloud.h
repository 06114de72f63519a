/* gaussreg_hip_cloud.h -- the cross-cloud nearest-neighbour entry points of libgaussreg_hip.so (csrc/cloud_nn.hip,
 * DESIGN.md 3.10).  They came after include/gaussreg_hip.h and the three training headers were closed at their present
 * symbol counts.  Same library, same conventions (gaussreg_hip.h, top): device pointers unless a name starts with h_,
 * status codes GR_OK / GR_ERR_*, gr_last_error() for the text, work enqueued on `stream`, no hidden allocation (the caller
 * passes the workspace the *_workspace_bytes query asks for).  The binding reads this header with the parser that reads
 * gaussreg_hip.h (gaussreg_amd/_lib.py: CLOUD_SIGNATURES / CLOUD_DEFINES).
 *
 * Both clouds are (n, 3) fp32, contiguous, finite and in ONE frame (a transform is the caller's business).  Every result
 * is defined as that of an exhaustive enumeration:
 *   d(i, j) = ((dx dx + dy dy) + dz dz) in fp32,  dx = support[j].x - query[i].x  (three multiplies, two adds, no FMA),
 *   candidates of query i ordered by (d, j).
 * That order is total, so the result does not depend on the order in which a search meets the candidates: only integer
 * atomics are used and two calls leave the same bits.  A support point equal to the query is a neighbour at distance 0;
 * nothing is excluded.  A non-finite coordinate in either cloud: GR_ERR_INVALID ("points must be finite"), no output is
 * written.  Every call synchronises the stream once (the finiteness flag, and the total of gr_cloud_radius_count).
 */
#ifndef GAUSSREG_HIP_CLOUD_H_
#define GAUSSREG_HIP_CLOUD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GR_CLOUD_KNN_MAX_K 8

/* gr_cloud_knn: row i of the outputs = the k support points smallest under (d, j) among those with d <= max_dist2
 * (+inf: no cap; a negative or NaN max_dist2 is refused).  dist2 (nq, k) fp32 ascending, index (nq, k) int64; either may
 * be null.  Slots beyond the number of qualifying points hold +inf / -1 (ns < k and the cap alike).
 * 1 <= k <= GR_CLOUD_KNN_MAX_K, 0 <= nq < 2^31, 1 <= ns < 2^31.  nq == 0: GR_OK, nothing is written.
 * gr_timing_* names: "cloud_nn_grid", "cloud_nn_query". */
/* host only; 0 for a shape the call refuses */
size_t gr_cloud_knn_workspace_bytes(int64_t nq, int64_t ns, int k);
int gr_cloud_knn(const float* query, int64_t nq, const float* support, int64_t ns, int k, float max_dist2, float* dist2,
                 int64_t* index, void* ws, size_t ws_bytes, void* stream);

/* gr_cloud_radius_count + gr_cloud_radius_pairs: every pair (i, j) with d(i, j) <= r2 (r2 >= 0, +inf allowed).
 * gr_cloud_radius_count builds the search structure in the workspace, writes count (nq) int32 = the number of such j per
 * query (may be null) and returns the number of pairs in *h_total with the call's one read-back; more than 2^31 - 1 pairs
 * are refused (GR_ERR_INVALID).  gr_cloud_radius_pairs, called next with the SAME clouds, r2 and workspace (which nothing
 * else may have written in between) and with total = *h_total, writes pairs (total, 2) int64 = (i, j), ordered by (i, j)
 * ascending: this order is the library's own (a k-d tree's order inside a row is its traversal order).  row_scratch: total
 * int32 of device scratch.  total == 0: GR_OK, nothing is written, pairs and row_scratch may be null.
 * 0 <= nq < 2^31, 1 <= ns < 2^31.  gr_timing_* names: "cloud_nn_grid", "cloud_nn_radius". */
/* host only; 0 for a shape the calls refuse */
size_t gr_cloud_radius_workspace_bytes(int64_t nq, int64_t ns);
int gr_cloud_radius_count(const float* query, int64_t nq, const float* support, int64_t ns, float r2, int32_t* count,
                          int64_t* h_total, void* ws, size_t ws_bytes, void* stream);
int gr_cloud_radius_pairs(const float* query, int64_t nq, const float* support, int64_t ns, float r2, int64_t total,
                          int32_t* row_scratch, int64_t* pairs, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GAUSSREG_HIP_CLOUD_H_ */
