"""PCA normals of a point cloud on the HIP kernel of csrc/cloud_normals.hip.

    n = estimate_normals(points, k=8)                              # scene_init.knn, then the neighbours and the point itself
    n, curv, valid = normals_from_neighbors(points, table, return_curvature=True, return_valid=True)

`normals_from_neighbors` does no search: `neighbors` (N, K) int64, K <= 64, is any table of indices into `support` (None:
`points`) -- `scene_init.knn`, `cloud_nn.knn`, `radius_search` -- and an entry outside [0, M) is padding (-1, or M as
`radius_search` pads).  Definition (include/gaussreg_hip_icp_plane.h): the covariance of the listed points (and the point
itself with include_self) about their mean, accumulated in float64 relative to the first of them; the normal is the unit
eigenvector of its smallest eigenvalue, rounded once to float32; curvature = l0 / (l0 + l1 + l2); fewer than three points
or a collinear set give valid = False, normal 0, curvature 0.  Sign: towards `toward` (a point, e.g. the sensor) when
given, else the component of largest magnitude is positive.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .cloud_nn import _check_cloud

MAX_K = _lib.CLOUD_NORMALS_MAX_K


def _toward(toward):
    if toward is None:
        return None
    t = toward.detach().cpu().numpy() if isinstance(toward, torch.Tensor) else np.asarray(toward)
    if t.shape != (3,):
        raise ValueError(f"toward: shape {t.shape}, must be (3,)")
    t = np.ascontiguousarray(t, np.float32)
    if not np.isfinite(t).all():
        raise ValueError("toward: every entry must be finite")
    return t


@torch.no_grad()
def normals_from_neighbors(points, neighbors, support=None, include_self=False, toward=None, return_curvature=False,
                           return_valid=False):
    """-> normals (N, 3) fp32, or a tuple (normals[, curvature (N,) fp32][, valid (N,) bool]) with the flags."""
    _check_cloud(points, "points")
    if support is None:
        support = points
    _check_cloud(support, "support")
    if support.device != points.device:
        raise ValueError(f"points is on {points.device}, support on {support.device}")
    n, m = points.shape[0], support.shape[0]
    if not isinstance(neighbors, torch.Tensor) or neighbors.dim() != 2 or neighbors.shape[0] != n:
        raise ValueError(f"neighbors: must be a tensor of shape ({n}, K), got {tuple(getattr(neighbors, 'shape', ()))}")
    if neighbors.dtype != torch.int64:
        raise ValueError(f"neighbors: dtype {neighbors.dtype}, must be int64")
    if not 1 <= neighbors.shape[1] <= MAX_K:
        raise ValueError(f"neighbors: K = {neighbors.shape[1]} outside 1..{MAX_K}")
    if not neighbors.is_contiguous():
        raise ValueError("neighbors: must be contiguous")
    if neighbors.device != points.device:
        raise ValueError(f"points is on {points.device}, neighbors on {neighbors.device}")
    t = _toward(toward)
    points, support, dev, k = points.detach(), support.detach(), points.device, neighbors.shape[1]
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    curvature = torch.empty(n, dtype=torch.float32, device=dev) if return_curvature else None
    valid = torch.empty(n, dtype=torch.uint8, device=dev) if return_valid else None
    _lib.call(dev, "gr_cloud_normals", points, n, support, m, neighbors, k, int(bool(include_self)),
              t.ctypes.data_as(ctypes.c_void_p) if t is not None else None, normals, curvature, valid,
              ws=_lib.lib().gr_cloud_normals_workspace_bytes(n, m, k))
    out = (normals,) + ((curvature,) if return_curvature else ()) + ((valid.bool(),) if return_valid else ())
    return out[0] if len(out) == 1 else out


def estimate_normals(points, k=8, toward=None, return_curvature=False, return_valid=False):
    """Normals of `points` (N, 3) from its k nearest neighbours (`scene_init.knn`, k <= 8, N > k) and the point itself."""
    from . import scene_init
    _, index = scene_init.knn(points, k)
    return normals_from_neighbors(points, index, include_self=True, toward=toward, return_curvature=return_curvature,
                                  return_valid=return_valid)
