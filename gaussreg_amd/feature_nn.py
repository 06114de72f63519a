"""Nearest neighbours in feature space on the HIP kernel of csrc/feature_nn.hip, and the reference's descriptor matching
(geotransformer/utils/registration.py:210-265, where scipy's cKDTree searches 32- to 256-dimensional rows on the host) on
top of it.

    dist2, index = nearest(q_feats, s_feats)                          # (nq,) fp32 squared distance / int64
    ri, rd, si, sd = mutual_nearest(ref_feats, src_feats)             # both directions, one kernel call
    ref_idx, src_idx = extract_corr_indices_from_feats(ref_feats, src_feats, mutual=True)
    ref_pts, src_pts = extract_correspondences_from_feats(ref_points, src_points, ref_feats, src_feats)

Definition (include/gaussreg_hip_feature_nn.h): d(i, j) is element (i, j) of ops.pairwise_distance(q, s, normalized), bit
for bit -- the squared distance in its expanded form, clamped at 0 -- and the neighbour of a row is the smallest under the
total order (d, index); a NaN distance counts as +inf.  The matrix is never written: the workspace is 12 bytes per row of
the two inputs.  Features are (n, c) float32 tensors on the GPU, 1 <= c <= 65536.  There is no CPU fallback.
"""
import torch

from . import _lib

MAX_C = _lib.FEATURE_NN_MAX_C


def _check_feats(feats, name):
    if not isinstance(feats, torch.Tensor) or feats.dim() != 2:
        raise ValueError(f"{name}: must be a tensor of shape (N, C), got {tuple(getattr(feats, 'shape', ()))}")
    if feats.dtype != torch.float32:
        raise ValueError(f"{name}: dtype {feats.dtype}, must be float32")
    if not feats.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if feats.shape[0] >= 2 ** 31 - 128:
        raise ValueError(f"{name}: {feats.shape[0]} rows, at most 2^31 - 129")
    if not 1 <= feats.shape[1] <= MAX_C:
        raise ValueError(f"{name}: {feats.shape[1]} channels, outside 1..{MAX_C}")
    if not feats.is_cuda:
        raise ValueError(f"{name}: on {feats.device}, must be on the GPU (there is no CPU fallback)")


def _check_pair(x, y, xname, yname):
    _check_feats(x, xname)
    _check_feats(y, yname)
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"{xname} has {x.shape[1]} channels, {yname} {y.shape[1]}")
    if x.device != y.device:
        raise ValueError(f"{xname} is on {x.device}, {yname} on {y.device}")


@torch.no_grad()
def feature_nn(x, y, normalized=False, rows=True, cols=True):
    """gr_feature_nn: -> (row_index (n) int64, row_dist2 (n) fp32, col_index (m), col_dist2 (m)); the pair of a direction
    that is not requested is (None, None).  Requesting neither raises."""
    _check_pair(x, y, "x", "y")
    if not (rows or cols):
        raise ValueError("feature_nn: neither the row nor the column outputs are requested")
    x, y = x.detach(), y.detach()
    dev, n, m, c = x.device, x.shape[0], y.shape[0], x.shape[1]
    ri = torch.empty(n, dtype=torch.int64, device=dev) if rows else None
    rd = torch.empty(n, dtype=torch.float32, device=dev) if rows else None
    ci = torch.empty(m, dtype=torch.int64, device=dev) if cols else None
    cd = torch.empty(m, dtype=torch.float32, device=dev) if cols else None
    if (rows and n) or (cols and m):     # (an empty output has no address: the library would read it as not requested)
        _lib.call(dev, "gr_feature_nn", x, n, y, m, c, int(bool(normalized)), ri if n else None, rd if n else None,
                  ci if m else None, cd if m else None, ws=_lib.lib().gr_feature_nn_workspace_bytes(n, m, c))
    return ri, rd, ci, cd


def nearest(q_feats, s_feats, normalized=False, return_index=True):
    """-> (dist2 (nq,) fp32, index (nq,) int64): for every row of q_feats its nearest row of s_feats (-1 / +inf when s_feats
    is empty).  Rows only: the kernel instantiation without the columns' side runs."""
    index, dist2, _, _ = feature_nn(q_feats, s_feats, normalized, rows=True, cols=False)
    return (dist2, index) if return_index else dist2


def mutual_nearest(ref_feats, src_feats, normalized=False):
    """-> (ref_nn_index (N,), ref_nn_dist2 (N,), src_nn_index (M,), src_nn_dist2 (M,)): the nearest src row of every ref row
    and the nearest ref row of every src row, over one distance matrix, in one kernel call."""
    return feature_nn(ref_feats, src_feats, normalized, rows=True, cols=True)


@torch.no_grad()
def extract_corr_indices_from_feats(ref_feats, src_feats, mutual=False, bilateral=False):
    """The reference's function (utils/registration.py:210-243), its three branches and its output order: ->
    (ref_corr_indices, src_corr_indices), int64 on the device.  `bilateral` is ignored when `mutual` is set."""
    if not (mutual or bilateral):
        _, ref_nn = nearest(ref_feats, src_feats)
        return torch.arange(ref_feats.shape[0], dtype=torch.int64, device=ref_feats.device), ref_nn
    ref_nn, _, src_nn, _ = mutual_nearest(ref_feats, src_feats)
    dev = ref_feats.device
    ref_indices = torch.arange(ref_feats.shape[0], dtype=torch.int64, device=dev)
    if mutual:
        if src_feats.shape[0] == 0:
            return ref_indices[:0], ref_nn[:0]
        ref_corr = ref_indices[src_nn[ref_nn] == ref_indices]
        return ref_corr, ref_nn[ref_corr]
    src_indices = torch.arange(src_feats.shape[0], dtype=torch.int64, device=dev)
    return torch.cat([ref_indices, src_nn]), torch.cat([ref_nn, src_indices])


@torch.no_grad()
def extract_correspondences_from_feats(ref_points, src_points, ref_feats, src_feats, mutual=False, return_feat_dist=False):
    """The reference's function (utils/registration.py:246-265): -> [ref_corr_points, src_corr_points] and, with
    return_feat_dist, the norm of the gathered feature difference (as the reference computes it, not sqrt(d))."""
    ref_corr, src_corr = extract_corr_indices_from_feats(ref_feats, src_feats, mutual=mutual)
    outputs = [ref_points[ref_corr], src_points[src_corr]]
    if return_feat_dist:
        outputs.append(torch.linalg.norm(ref_feats[ref_corr] - src_feats[src_corr], dim=1))
    return outputs
