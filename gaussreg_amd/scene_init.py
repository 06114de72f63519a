"""Scene initialisation from a point cloud on the HIP kernels of csrc/scene_init.hip: the exact k nearest neighbours inside
one cloud, upstream 3DGS's create_from_pcd on top of them, and its position learning-rate schedule.

    d2 = mean_knn_dist2(points)                    # (N,) what simple_knn._C.distCUDA2 returns
    dist2, index = knn(points, k=8)                # (N, k) fp32 ascending, (N, k) int64
    params = gaussians_from_points(points, colors) # upstream's raw parameters, ready to be GaussianAdam groups
    lr = expon_lr(step, 1.6e-4, 1.6e-6, max_steps=30_000)

The neighbours are those of an exhaustive enumeration under the order (distance, index), bit for bit.
There is no CPU fallback.
"""
import math

import torch

from . import _lib

SH_C0 = 0.28209479177387814


def _check_points(points, k):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points: must be a tensor of shape (N, 3), got {tuple(getattr(points, 'shape', ()))}")
    if points.dtype != torch.float32:
        raise ValueError(f"points: dtype {points.dtype}, must be float32")
    if not points.is_contiguous():
        raise ValueError("points: must be contiguous")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.GS_KNN_MAX_K:
        raise ValueError(f"k = {k!r} outside 1..{_lib.GS_KNN_MAX_K}")
    if points.shape[0] <= k:
        raise ValueError(f"points: {points.shape[0]} points, k = {k} neighbours need more than {k}")
    if points.shape[0] >= 2 ** 31:
        raise ValueError(f"points: {points.shape[0]} points, at most 2^31 - 1")
    if not points.is_cuda:
        raise ValueError(f"points: on {points.device}, must be on the GPU (there is no CPU fallback)")


@torch.no_grad()
def _run(points, k, want_dist2, want_index, want_mean):
    _check_points(points, k)
    points = points.detach()
    dev, N = points.device, points.shape[0]
    dist2 = torch.empty((N, k), dtype=torch.float32, device=dev) if want_dist2 else None
    index = torch.empty((N, k), dtype=torch.int64, device=dev) if want_index else None
    mean = torch.empty(N, dtype=torch.float32, device=dev) if want_mean else None
    try:
        _lib.call(dev, "gr_gs_knn", points, N, k, dist2, index, mean, ws=_lib.lib().gr_gs_knn_workspace_bytes(N, k))
    except RuntimeError as e:
        if "points must be finite" in str(e):
            raise ValueError("points must be finite") from None
        raise
    return dist2, index, mean


def knn(points, k=3):
    """-> (dist2 (N, k) fp32 ascending, index (N, k) int64) of the k nearest other points of every point of `points` (N, 3)."""
    dist2, index, _ = _run(points, k, True, True, False)
    return dist2, index


def mean_knn_dist2(points, k=3):
    """-> (N,) fp32: the mean squared distance of every point to its k nearest other points (k = 3: upstream's distCUDA2)."""
    return _run(points, k, False, False, True)[2]


def scene_from_dist2(points, colors, dist2, sh_degree=3, initial_opacity=0.1):
    """The element-wise part of create_from_pcd, in torch on whatever device `points` is on: `dist2` (N,) is
    mean_knn_dist2(points)."""
    N = points.shape[0]
    dev, dt = points.device, points.dtype
    f_dc = ((colors - 0.5) / SH_C0).reshape(N, 1, 3)
    f_rest = torch.zeros((N, (sh_degree + 1) ** 2 - 1, 3), dtype=dt, device=dev)
    opacity = torch.full((N, 1), math.log(initial_opacity / (1.0 - initial_opacity)), dtype=dt, device=dev)
    scaling = torch.log(torch.sqrt(torch.clamp_min(dist2, 1e-7)))[:, None].repeat(1, 3)
    rotation = torch.zeros((N, 4), dtype=dt, device=dev)
    rotation[:, 0] = 1.0
    out = {"xyz": points.detach().clone(), "f_dc": f_dc.contiguous(), "f_rest": f_rest, "opacity": opacity,
           "scaling": scaling.contiguous(), "rotation": rotation}
    return {name: t.requires_grad_(True) for name, t in out.items()}


@torch.no_grad()
def gaussians_from_points(points, colors, sh_degree=3, initial_opacity=0.1):
    """Upstream's create_from_pcd: `points` (N, 3) fp32 on the GPU, `colors` (N, 3) in [0, 1] -> dict of the raw parameters
    xyz, f_dc, f_rest, opacity, scaling, rotation under upstream's names, each a leaf with requires_grad."""
    _check_points(points, 3)
    if not isinstance(colors, torch.Tensor) or tuple(colors.shape) != tuple(points.shape):
        raise ValueError(f"colors: must be a tensor of shape {tuple(points.shape)}")
    if colors.dtype != torch.float32 or colors.device != points.device:
        raise ValueError(f"colors: must be a float32 tensor on {points.device}")
    if isinstance(sh_degree, bool) or not isinstance(sh_degree, int) or not 0 <= sh_degree <= 3:
        raise ValueError(f"sh_degree = {sh_degree!r} outside 0..3")
    if not 0.0 < initial_opacity < 1.0:
        raise ValueError(f"initial_opacity {initial_opacity} outside (0, 1)")
    return scene_from_dist2(points, colors, mean_knn_dist2(points, 3), sh_degree, initial_opacity)


def expon_lr(step, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=30_000):
    """Upstream's get_expon_lr_func evaluated at `step`: log-linear from lr_init to lr_final over max_steps, times a sine
    ramp from lr_delay_mult to 1 over the first lr_delay_steps."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    if lr_delay_steps > 0:
        delay = lr_delay_mult + (1.0 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
    else:
        delay = 1.0
    t = min(max(step / max_steps, 0.0), 1.0)
    return delay * math.exp(math.log(lr_init) * (1.0 - t) + math.log(lr_final) * t)
