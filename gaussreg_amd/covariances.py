"""The per-point covariances generalised ICP takes (`icp.icp_generalized`), on the HIP kernels of csrc/cloud_covariances.hip
(DESIGN.md 3.15).  A covariance is a row of six float32 values, the upper triangle xx, xy, xz, yy, yz, zz -- the order of
the rasterizer's `cov3D_precomp`.

    c = covariances_from_normals(normals)                          # the plane prior I - (1 - eps) n n^T
    c = covariances_from_gaussians(scales, rotations)              # the same prior about each Gaussian's thinnest axis
    c, n = covariances_from_gaussians(scales, rotations, return_normals=True)     # ... and that axis as a normal
    c = covariances_from_gaussians(scales, rotations, mode="raw")  # R S^2 R^T as the rasterizer computes it, bit for bit
    c = estimate_covariances(points, k=8)                          # estimate_normals, then covariances_from_normals

Definition (include/gaussreg_hip_gicp.h): arithmetic in float64, every output rounded once; a zero normal or a zero
quaternion gives the identity (and, from Gaussians, a zero normal); a non-finite input makes its own row non-finite,
which `icp_generalized` refuses.  `scales` are the activated scales and `rotations` the quaternions (r, x, y, z) that
`GaussianRasterizer` takes; "raw" uses them as given, "plane" normalises the quaternion.  There is no CPU fallback.
"""
import torch

from . import _lib
from .cloud_nn import _check_cloud

MODES = {"raw": _lib.GS_COV_RAW, "plane": _lib.GS_COV_PLANE}


def _epsilon(epsilon):
    epsilon = float(epsilon)
    if not 0.0 <= epsilon <= 1.0:
        raise ValueError(f"epsilon = {epsilon!r} outside [0, 1]")
    return epsilon


def _check_rows(t, name, width):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f"{name}: must be a tensor of shape (N, {width}), got {tuple(getattr(t, 'shape', ()))}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: dtype {t.dtype}, must be float32")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if not t.is_cuda:
        raise ValueError(f"{name}: on {t.device}, must be on the GPU (there is no CPU fallback)")


@torch.no_grad()
def covariances_from_normals(normals, epsilon=1e-3):
    """-> (N, 6) fp32: I - (1 - epsilon) v v^T with v = normal / |normal|, eigenvalues (epsilon, 1, 1)."""
    _check_cloud(normals, "normals")
    epsilon = _epsilon(epsilon)
    normals, n = normals.detach(), normals.shape[0]
    cov = torch.empty((n, 6), dtype=torch.float32, device=normals.device)
    _lib.call(normals.device, "gr_cloud_covariances_from_normals", normals, n, epsilon, cov, None, 0)
    return cov


@torch.no_grad()
def covariances_from_gaussians(scales, rotations, scale_modifier=1.0, mode="plane", epsilon=1e-3, return_normals=False):
    """-> (N, 6) fp32, or (covariances, normals (N, 3) fp32, valid (N,) bool) with return_normals: the unit axis of every
    Gaussian's smallest scale, its largest component positive; valid is False (and the normal zero) for a zero quaternion."""
    _check_rows(scales, "scales", 3)
    _check_rows(rotations, "rotations", 4)
    if scales.shape[0] != rotations.shape[0]:
        raise ValueError(f"rotations: {rotations.shape[0]} rows for {scales.shape[0]} rows of scales")
    if scales.device != rotations.device:
        raise ValueError(f"scales is on {scales.device}, rotations on {rotations.device}")
    if mode not in MODES:
        raise ValueError(f"mode = {mode!r}, must be 'raw' or 'plane'")
    epsilon, scale_modifier = _epsilon(epsilon), float(scale_modifier)
    if scale_modifier != scale_modifier or scale_modifier in (float("inf"), float("-inf")):
        raise ValueError(f"scale_modifier = {scale_modifier!r} must be finite")
    scales, rotations, n, dev = scales.detach(), rotations.detach(), scales.shape[0], scales.device
    cov = torch.empty((n, 6), dtype=torch.float32, device=dev)
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev) if return_normals else None
    valid = torch.empty(n, dtype=torch.uint8, device=dev) if return_normals else None
    _lib.call(dev, "gr_gs_covariances", scales, rotations, n, scale_modifier, MODES[mode], epsilon, cov, normals, valid, None, 0)
    return (cov, normals, valid.bool()) if return_normals else cov


def estimate_covariances(points, k=8, epsilon=1e-3):
    """`normals.estimate_normals(points, k)`, then `covariances_from_normals`: what Open3D's generalised ICP builds for a
    cloud without covariances.  A point without a valid normal gets the identity."""
    from .normals import estimate_normals
    return covariances_from_normals(estimate_normals(points, k=k), epsilon)
