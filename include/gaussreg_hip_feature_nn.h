/* gaussreg_hip_feature_nn.h -- nearest neighbours in feature space of libgaussreg_hip.so (csrc/feature_nn.hip, DESIGN.md
 * 3.12).  It came after include/gaussreg_hip_cloud.h and include/gaussreg_hip_icp.h were closed.  Same library, same
 * conventions (gaussreg_hip.h, top): device pointers, status codes GR_OK / GR_ERR_*, gr_last_error() for the text, work
 * enqueued on `stream`, no hidden allocation, no host synchronisation.  The binding reads this header with the parser that
 * reads gaussreg_hip.h (gaussreg_amd/_lib.py: FEATURE_NN_SIGNATURES / FEATURE_NN_DEFINES).
 *
 * x (n, c) and y (m, c) are fp32, row-major, contiguous; any alignment, any c in the limits.
 *
 * Distance.  d(i, j) is, bit for bit, element (i, j) of gr_pairwise_distance(x, y, n, m, c, normalized):
 *   xy    = the fmaf chain over k = 0, 1, ..., c - 1 (ascending) of x[i][k] y[j][k], starting from 0 (the fp32 MFMA tile);
 *   x2(i) = the squared norm of row i as that call sums it: lane l of a wave adds x[i][k]^2 for k = l, l + 64, ... in
 *           ascending order, then the 64 partial sums are folded by an xor butterfly at distances 32, 16, ..., 1; y2(j) alike;
 *   d     = (x2(i) - 2 xy) + y2(j), or 2 - 2 xy when `normalized` (the rows are then taken to be unit rows and no norm is
 *           computed), then clamped at 0 from below.
 * Both pairwise kernels of the library return these bits, so d does not depend on a choice of tile.  A NaN d -- with finite
 * features only an overflowed norm produces one (inf - inf) -- is ordered and reported as +inf.
 * Rows.     row_index[i] = the j smallest under the total order (d(i, j), j); row_dist2[i] = that d.
 * Columns.  col_index[j] = the i smallest under (d(i, j), i) over THE SAME matrix; col_dist2[j] = that d.  This is not the
 *           row answer of the swapped call: (x2 - 2 xy) + y2 and (y2 - 2 xy) + x2 round differently.  With normalized = 1
 *           the two coincide.
 * m == 0: row_index = -1, row_dist2 = +inf.  n == 0: col_index = -1, col_dist2 = +inf.
 * Each output pair may be null (both pointers of the pair); with neither pair requested, or half a pair: GR_ERR_INVALID.
 *
 * Limits.  0 <= n, m < 2^31 - 128 (an index is the low half of a 64-bit key, and the last tile of 128 is addressed in 32-bit
 * integers); 1 <= c <= GR_FEATURE_NN_MAX_C (the staging counts channels in 32-bit integers; the bound keeps every such sum
 * far from overflow).
 * Workspace.  8 (n + m) bytes of keys and 4 (n + m) bytes of squared norms, in four carves aligned to 256 bytes: at most
 * 12 (n + m) + GR_FEATURE_NN_WORKSPACE_CAP bytes, whatever c is.  Nothing of size n x m, and no table per (row, column
 * tile): a workgroup sweeps a strip of column tiles and keeps its running minima on chip.
 * Reproducibility.  The minima are taken over a total order, by lane-local compares, fixed exchanges inside a workgroup and
 * 64-bit INTEGER atomicMin on the key (bits(d) << 32 | index) across workgroups; there are no float atomics.  Two calls,
 * calls on different streams, and a rows-only, a columns-only and a both-directions call leave the same bits in every
 * output they share.  gr_timing_* name: "feature_nn".
 */
#ifndef GAUSSREG_HIP_FEATURE_NN_H_
#define GAUSSREG_HIP_FEATURE_NN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GR_FEATURE_NN_MAX_C 65536
#define GR_FEATURE_NN_WORKSPACE_CAP 4096

/* host only; 0 for a shape the call refuses */
size_t gr_feature_nn_workspace_bytes(int64_t n, int64_t m, int64_t c);

/* row_index (n) int64 / row_dist2 (n) fp32: the nearest row of y for every row of x; may be null together.
 * col_index (m) int64 / col_dist2 (m) fp32: the nearest row of x for every row of y; may be null together. */
int gr_feature_nn(const float* x, int64_t n, const float* y, int64_t m, int64_t c, int normalized, int64_t* row_index,
                  float* row_dist2, int64_t* col_index, float* col_dist2, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GAUSSREG_HIP_FEATURE_NN_H_ */
