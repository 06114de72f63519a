"""Point-to-point ICP on the HIP kernels of csrc/cloud_icp.hip: nearest-neighbour matching over a grid
of the reference cloud that is built once, fp64 sums in a fixed order, the fp64 Umeyama fit (rigid, or rigid plus uniform
scale) and the stop test, all on the device; one host read-back per call.

    res = icp(src, ref, init_transform=T0, max_dist=0.1, with_scale=True)
    res.transform            # (4, 4) fp32 on the device: maps src into ref's frame
    res.fitness, res.inlier_rmse, res.iterations, res.converged, res.status
    ev = evaluate_registration(src, ref, 0.1, T)      # the max_iterations=0 call: fitness and inlier_rmse of T

Definition (include/gaussreg_hip_icp.h): a source point is transformed in fp32, ((A0 x + A1 y) + A2 z) + t, and matched to
the reference point smallest under (d, j) among those with d <= float32(max_dist^2), exactly as `cloud_nn.knn` does;
fitness = matched / all, inlier_rmse = sqrt(mean d) over the matched.  Every update is fitted to the ORIGINAL source
coordinates.  The loop stops when fitness and inlier_rmse both change by less than their tolerances ("converged"), at
max_iterations ("iteration_limit"), or when fewer than three points match or the fit has no spread ("degenerate": the
transform is the last valid one).  Two calls give the same bits.  These are the semantics of Open3D's registration_icp
with TransformationEstimationPointToPoint(with_scaling); parity with Open3D is unpinned.  There is no CPU fallback.

    res = icp_point_to_plane(src, ref, estimate_normals(ref), init_transform=T0, max_dist=0.1)

is the same loop with the point-to-plane update (csrc/cloud_icp_plane.hip): rigid only, the estimator for
scans of walls, floors and table tops, along which point-to-point slides slowly.

    res = icp_generalized(src, ref, src_cov, ref_cov, init_transform=T0, max_dist=0.1)

is the same loop with the update of generalised ICP (csrc/cloud_icp_gicp.hip): every residual weighted by
(C_ref + R C_src R^T)^-1, with the (N, 6) covariances of `gaussreg_amd.covariances` -- a scene's own Gaussians among them.
"""
import ctypes
import sys
import types
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from .cloud_nn import _check_cloud, _finite, _r2

MAX_ITERATIONS = _lib.CLOUD_ICP_MAX_ITERATIONS
STATUS = {_lib.ICP_DEFINES["GR_CLOUD_ICP_CONVERGED"]: "converged",
          _lib.ICP_DEFINES["GR_CLOUD_ICP_ITERATION_LIMIT"]: "iteration_limit",
          _lib.ICP_DEFINES["GR_CLOUD_ICP_DEGENERATE"]: "degenerate"}


@dataclass
class IcpResult:
    transform: torch.Tensor               # (4, 4) fp32 on the device
    fitness: float
    inlier_rmse: float
    iterations: int
    converged: bool
    status: str                           # "converged", "iteration_limit" or "degenerate"
    index: Optional[torch.Tensor] = None   # (N,) int64: the matched ref point of every src point, -1 for none
    dist2: Optional[torch.Tensor] = None   # (N,) fp32: its squared distance, +inf for none
    history: Optional[torch.Tensor] = None  # (iterations + 1, 16) fp64 on the host: T_t[12], n, S, fitness, rmse


def _transform0(init_transform):
    """-> (3, 4) fp32 numpy, contiguous: the upper rows of a (4, 4) transform given as a tensor, an array or nested lists."""
    if init_transform is None:
        return np.ascontiguousarray(np.eye(4, dtype=np.float32)[:3])
    t = init_transform.detach().cpu().numpy() if isinstance(init_transform, torch.Tensor) else np.asarray(init_transform)
    if t.shape != (4, 4):
        raise ValueError(f"init_transform: shape {t.shape}, must be (4, 4)")
    t = t.astype(np.float32)
    if not np.isfinite(t).all():
        raise ValueError("init_transform: every entry must be finite")
    if not (t[3] == np.array([0, 0, 0, 1], np.float32)).all():
        raise ValueError(f"init_transform: last row {t[3].tolist()}, must be [0, 0, 0, 1]")
    return np.ascontiguousarray(t[:3])


def _check_arguments(src_points, ref_points, max_dist, max_iterations, relative_fitness, relative_rmse):
    """The checks the estimators share -> (float32(max_dist^2), relative_fitness, relative_rmse) as floats."""
    _check_cloud(src_points, "src_points")
    _check_cloud(ref_points, "ref_points")
    if ref_points.shape[0] < 1:
        raise ValueError("ref_points: 0 points, at least 1")
    if src_points.device != ref_points.device:
        raise ValueError(f"src_points is on {src_points.device}, ref_points on {ref_points.device}")
    if max_dist is None or not np.isfinite(float(max_dist)):
        raise ValueError(f"max_dist = {max_dist!r} must be finite and >= 0")
    cap = _r2(max_dist, "max_dist")
    if not np.isfinite(cap):
        raise ValueError(f"max_dist = {max_dist!r}: its square is not a finite float32")
    if isinstance(max_iterations, bool) or not isinstance(max_iterations, int) or not 0 <= max_iterations <= MAX_ITERATIONS:
        raise ValueError(f"max_iterations = {max_iterations!r} outside 0..{MAX_ITERATIONS}")
    relative_fitness, relative_rmse = float(relative_fitness), float(relative_rmse)
    if np.isnan(relative_fitness) or np.isnan(relative_rmse):
        raise ValueError("relative_fitness and relative_rmse must not be NaN")
    return cap, relative_fitness, relative_rmse


def _run(entry, src_points, ref_points, extra_clouds, init_transform, extra_scalars, cap, max_iterations, relative_fitness,
         relative_rmse, return_correspondences, return_history, src_extra=()):
    """Allocate the outputs, call `entry` -- gr_cloud_icp(src, n, *src_extra, ref, *extra_clouds, m, T0, cap, *extra_scalars,
    ...) -- and read the result."""
    t0 = _transform0(init_transform)
    src, ref = src_points.detach(), ref_points.detach()
    dev, n, m = src.device, src.shape[0], ref.shape[0]
    transform = torch.empty((4, 4), dtype=torch.float32, device=dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    index = torch.empty(n, dtype=torch.int64, device=dev) if return_correspondences else None
    dist2 = torch.empty(n, dtype=torch.float32, device=dev) if return_correspondences else None
    history = torch.zeros((max_iterations + 1, 16), dtype=torch.float64, device=dev) if return_history else None
    h_status = (ctypes.c_int * 2)(0, 0)
    _finite(lambda: _lib.call(dev, entry, src, n, *src_extra, ref, *extra_clouds, m, t0.ctypes.data_as(ctypes.c_void_p), cap, *extra_scalars,
                              max_iterations, relative_fitness, relative_rmse, transform, stats, index, dist2, history, h_status,
                              ws=getattr(_lib.lib(), entry + "_workspace_bytes")(n, m, max_iterations)))
    status, iterations = STATUS[h_status[0]], int(h_status[1])
    fitness, rmse = stats[:2].tolist()
    return IcpResult(transform=transform, fitness=fitness, inlier_rmse=rmse, iterations=iterations,
                     converged=status == "converged", status=status, index=index, dist2=dist2,
                     history=history[:iterations + 1].cpu() if history is not None else None)


@torch.no_grad()
def icp(src_points, ref_points, init_transform=None, max_dist=0.1, with_scale=False, max_iterations=30,
        relative_fitness=1e-6, relative_rmse=1e-6, return_correspondences=False, return_history=False):
    """Refine `init_transform` (None: identity) so that it maps src_points onto ref_points -> IcpResult."""
    cap, relative_fitness, relative_rmse = _check_arguments(src_points, ref_points, max_dist, max_iterations, relative_fitness,
                                                            relative_rmse)
    return _run("gr_cloud_icp", src_points, ref_points, (), init_transform, (int(bool(with_scale)),), cap, max_iterations,
                relative_fitness, relative_rmse, return_correspondences, return_history)


def evaluate_registration(src_points, ref_points, max_dist, transform=None, return_correspondences=False):
    """Fitness and inlier RMSE of `transform` as it stands (Open3D's evaluate_registration): the max_iterations=0 call."""
    return icp(src_points, ref_points, transform, max_dist=max_dist, max_iterations=0,
               return_correspondences=return_correspondences)


@torch.no_grad()
def icp_point_to_plane(src_points, ref_points, ref_normals, init_transform=None, max_dist=0.1, max_iterations=30,
                       relative_fitness=1e-6, relative_rmse=1e-6, return_correspondences=False, return_history=False):
    """Point-to-plane ICP (csrc/cloud_icp_plane.hip, DESIGN.md 3.14, include/gaussreg_hip_icp_plane.h): the loop of `icp`
    -- the same evaluation, stop rule, statuses and history -- whose update minimises sum ((T p - q) . n)^2 over the
    matched pairs, linearised at the current transform and solved in float64 on the device; rigid only.  `ref_normals`
    (M, 3) fp32, one per reference point (`normals.estimate_normals(ref_points)`), finite, used as given; a zero normal
    (an invalid row of the normals kernel) drops out of the update.  Fewer than six matches or a system without a unique
    solution (a single plane) is "degenerate".  Open3D's TransformationEstimationPointToPlane; parity unpinned."""
    cap, relative_fitness, relative_rmse = _check_arguments(src_points, ref_points, max_dist, max_iterations, relative_fitness,
                                                            relative_rmse)
    _check_cloud(ref_normals, "ref_normals")
    if ref_normals.shape[0] != ref_points.shape[0]:
        raise ValueError(f"ref_normals: {ref_normals.shape[0]} rows for {ref_points.shape[0]} reference points")
    if ref_normals.device != ref_points.device:
        raise ValueError(f"ref_points is on {ref_points.device}, ref_normals on {ref_normals.device}")
    try:
        return _run("gr_cloud_icp_plane", src_points, ref_points, (ref_normals.detach(),), init_transform, (), cap,
                    max_iterations, relative_fitness, relative_rmse, return_correspondences, return_history)
    except RuntimeError as e:
        if "normals must be finite" in str(e):
            raise ValueError("normals must be finite") from None
        raise


def _check_covariances(cov, name, points, points_name):
    if not isinstance(cov, torch.Tensor) or cov.dim() != 2 or cov.shape[1] != 6:
        raise ValueError(f"{name}: must be a tensor of shape (N, 6), got shape {tuple(getattr(cov, 'shape', ()))}")
    if cov.dtype != torch.float32:
        raise ValueError(f"{name}: dtype {cov.dtype}, must be float32")
    if not cov.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if not cov.is_cuda:
        raise ValueError(f"{name}: on {cov.device}, must be on the GPU (there is no CPU fallback)")
    if cov.shape[0] != points.shape[0]:
        raise ValueError(f"{name}: {cov.shape[0]} rows for {points.shape[0]} points of {points_name}")
    if cov.device != points.device:
        raise ValueError(f"{points_name} is on {points.device}, {name} on {cov.device}")


@torch.no_grad()
def icp_generalized(src_points, ref_points, src_covariances, ref_covariances, init_transform=None, max_dist=0.1,
                    max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6, return_correspondences=False,
                    return_history=False):
    """Generalised ICP (csrc/cloud_icp_gicp.hip, DESIGN.md 3.15, include/gaussreg_hip_gicp.h): the loop of `icp` -- the same
    evaluation, stop rule, statuses and history, fitness and inlier RMSE Euclidean -- whose update minimises
    sum d^T (C_ref + A C_src A^T)^-1 d over the matched pairs, d = T p - q, A the rotation of the current transform, linearised
    there and solved in float64 on the device; rigid only.  `src_covariances` (N, 6) and `ref_covariances` (M, 6) fp32, the
    upper triangles xx, xy, xz, yy, yz, zz (`covariances.covariances_from_gaussians`, `covariances_from_normals`,
    `estimate_covariances`), finite; a pair whose combined covariance is singular (two zero rows) drops out of the update
    and still counts.  Fewer than three matches or a system without a unique solution is "degenerate".  Open3D's
    TransformationEstimationForGeneralizedICP; parity unpinned."""
    cap, relative_fitness, relative_rmse = _check_arguments(src_points, ref_points, max_dist, max_iterations, relative_fitness,
                                                            relative_rmse)
    _check_covariances(src_covariances, "src_covariances", src_points, "src_points")
    _check_covariances(ref_covariances, "ref_covariances", ref_points, "ref_points")
    try:
        return _run("gr_cloud_gicp", src_points, ref_points, (ref_covariances.detach(),), init_transform, (), cap,
                    max_iterations, relative_fitness, relative_rmse, return_correspondences, return_history,
                    src_extra=(src_covariances.detach(),))
    except RuntimeError as e:
        if "covariances must be finite" in str(e):
            raise ValueError("covariances must be finite") from None
        raise


class _CallableModule(types.ModuleType):
    """The package exports the function under the submodule's own name, so `gaussreg_amd.icp` is both: calling the module
    calls `icp`."""

    def __call__(self, *args, **kwargs):
        return icp(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
