/* gaussreg_hip_train_backbone.h -- the training entry points of the backbone's normalisation layers in libgaussreg_hip.so.
 * They came after include/gaussreg_hip.h, gaussreg_hip_train.h and gaussreg_hip_train_matching.h were closed at their
 * present symbol counts.  Same library, same conventions (gaussreg_hip.h, top): device pointers unless a name starts with
 * h_, status codes GR_OK / GR_ERR_*, gr_last_error() for the text, asynchronous on `stream`, no host synchronisation, no
 * hidden allocation (the caller passes the workspace the *_workspace_bytes query asks for).  The binding reads this header
 * with the parser that reads gaussreg_hip.h (gaussreg_amd/_lib.py: BACKBONE_TRAIN_SIGNATURES / BACKBONE_TRAIN_DEFINES).
 */
#ifndef GAUSSREG_HIP_TRAIN_BACKBONE_H_
#define GAUSSREG_HIP_TRAIN_BACKBONE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* gr_group_norm_train: gr_group_norm_res (GroupNorm over the rows of every segment of a (n, c) matrix, + residual,
 * LeakyReLU; seg_off null: one segment, nseg and max_seg_rows ignored; residual null: no shortcut; negative_slope 1: plain
 * norm) that also leaves the statistics its apply pass used: stats (nseg, 2, groups) fp32, [s][0][g] = mean, [s][1][g] =
 * rstd = 1 / sqrt(var + eps).  `out` holds the bits gr_group_norm / _seg / _res write for the same inputs (the same three
 * launches; a fourth copies the statistics out of the workspace).  Workspace: gr_group_norm_seg_workspace_bytes(groups,
 * nseg).  n == 0 or nseg == 0: GR_OK, nothing is written.  gr_timing_* name: "group_norm". */
int gr_group_norm_train(const float* x, int64_t n, int64_t c, int64_t groups, const float* gamma, const float* beta,
                        float eps, float negative_slope, const float* residual, float* out, float* stats,
                        const int64_t* seg_off, int64_t nseg, int64_t max_seg_rows, void* ws, size_t ws_bytes,
                        void* stream);

/* gr_group_norm_backward: the gradients of gr_group_norm_train.  x (n, c): the forward's input; out (n, c): the forward's
 * OUTPUT; grad_out (n, c); gamma (c) or null (= 1); stats: what the forward left; seg_off / nseg / max_seg_rows as in the
 * forward (seg_off null: one segment).  Per segment s and group g, cnt = rows_s * c / groups, xhat = (x - mean) * rstd:
 *   dy            = grad_out * (pre > 0 ? 1 : negative_slope)        (torch's leaky_relu convention at 0)
 *   grad_residual = dy
 *   grad_beta[ch] = sum over all rows of dy,  grad_gamma[ch] = sum over all rows of dy * xhat
 *   B = sum dy * gamma,  A = sum dy * gamma * xhat                   (over the group's rows and channels)
 *   grad_x        = rstd * (dy * gamma - (B + xhat * A) / cnt)
 * With negative_slope > 0 the sign of the pre-activation `pre` is the sign of `out` (out > 0 exactly when pre > 0), so
 * neither the pre-activation nor the residual is an input: x, out, stats and gamma are all the forward has to keep.
 * negative_slope <= 0 is refused; negative_slope == 1 is the plain norm and `out` is then not read (it may be null).
 * Outputs, each may be null when not wanted: grad_x (n, c), grad_residual (n, c), grad_gamma (c), grad_beta (c).  None may
 * alias an input.  Every element of a wanted output is written.
 * Pass 1 streams x, out and grad_out once and leaves per-workgroup, per-column fp64 sums of dy and dy * xhat for every
 * segment (and dy itself in grad_residual when that is wanted); two small fold launches add them up in a fixed order into
 * grad_gamma, grad_beta and A / cnt, B / cnt per (segment, group); pass 2 streams again and writes grad_x.  No float
 * atomics anywhere: two calls on the same inputs leave the same bits.
 *   workspace bytes = nseg * (16 * blocks * c + 16 * c + 8 * groups) + 768,
 *   blocks = min(clamp(131072 / c, 32, 1024), max(1, 2048 / nseg))    -- no term in n.
 * n == 0 or nseg == 0: grad_gamma and grad_beta are zeroed, GR_OK.  Refused before any launch (GR_ERR_INVALID): the
 * channel counts gr_group_norm refuses (c / 4 must divide 256 or be a multiple of it), groups > 64 or not a divisor of c,
 * nseg >= 65536, negative_slope <= 0, null or unaligned (16 B) pointers, a workspace that is too small.
 * gr_timing_* name: "group_norm_backward". */
/* host only; 0 for a shape the call refuses */
size_t gr_group_norm_backward_workspace_bytes(int64_t c, int64_t groups, int64_t nseg);
int gr_group_norm_backward(const float* x, const float* out, const float* grad_out, const float* gamma, const float* stats,
                           int64_t n, int64_t c, int64_t groups, float negative_slope, const int64_t* seg_off,
                           int64_t nseg, int64_t max_seg_rows, float* grad_x, float* grad_residual, float* grad_gamma,
                           float* grad_beta, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GAUSSREG_HIP_TRAIN_BACKBONE_H_ */
