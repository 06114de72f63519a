"""Cross-cloud nearest neighbours on the HIP kernels of csrc/cloud_nn.hip, and the reference's overlap, ground-truth
correspondence and evaluation functions (geotransformer/utils/registration.py, where scipy's cKDTree does the search) on
top of them.

    dist2, index = knn(query, support, k=3, max_dist=0.1)   # (nq, k) fp32 ascending / int64; +inf / -1 where nothing qualifies
    dist = nearest(query, support)                          # (nq,) Euclidean, what get_nearest_neighbor returns
    pairs = radius_pairs(query, support, 0.05)              # (total, 2) int64 (i, j), ordered by (i, j) ascending
    overlap = compute_overlap(ref, src, transform, positive_radius=0.1)
    corr = get_correspondences(ref, src, transform, matching_radius=0.1)

Definition (include/gaussreg_hip_cloud.h): d(i, j) = ((dx dx + dy dy) + dz dz) in fp32, candidates ordered by (d, j); the
result is that of an exhaustive enumeration, bit for bit.  A radius r enters as the fp32 number r2 = float32(r * r) and
qualifies d <= r2.  Clouds are (n, 3) float32 tensors on the GPU, in one frame; the functions that take a transform apply
it in torch (fp32) first.  The order of pairs inside a row is ascending j -- this library's choice: a k-d tree's order is
its traversal order and means nothing.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_K = _lib.CLOUD_KNN_MAX_K


def _check_cloud(points, name):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{name}: must be a tensor of shape (N, 3), got {tuple(getattr(points, 'shape', ()))}")
    if points.dtype != torch.float32:
        raise ValueError(f"{name}: dtype {points.dtype}, must be float32")
    if not points.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if points.shape[0] >= 2 ** 31:
        raise ValueError(f"{name}: {points.shape[0]} points, at most 2^31 - 1")
    if not points.is_cuda:
        raise ValueError(f"{name}: on {points.device}, must be on the GPU (there is no CPU fallback)")


def _check_pair(query, support):
    _check_cloud(query, "query")
    _check_cloud(support, "support")
    if support.shape[0] < 1:
        raise ValueError("support: 0 points, at least 1")
    if query.device != support.device:
        raise ValueError(f"query is on {query.device}, support on {support.device}")


def _r2(radius, name):
    """float32(r * r): the number the kernels compare d with."""
    if radius is None:
        return float("inf")
    radius = float(radius)
    if not radius >= 0.0:
        raise ValueError(f"{name} = {radius!r} must be >= 0")
    return float(np.float32(radius * radius))


def _finite(call):
    try:
        return call()
    except RuntimeError as e:
        if "points must be finite" in str(e):
            raise ValueError("points must be finite") from None
        raise


@torch.no_grad()
def _knn(query, support, k, max_dist2):
    _check_pair(query, support)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f"k = {k!r} outside 1..{MAX_K}")
    query, support = query.detach(), support.detach()
    dev, nq, ns = query.device, query.shape[0], support.shape[0]
    dist2 = torch.empty((nq, k), dtype=torch.float32, device=dev)
    index = torch.empty((nq, k), dtype=torch.int64, device=dev)
    _finite(lambda: _lib.call(dev, "gr_cloud_knn", query, nq, support, ns, k, max_dist2, dist2, index,
                              ws=_lib.lib().gr_cloud_knn_workspace_bytes(nq, ns, k)))
    return dist2, index


def knn(query, support, k=1, max_dist=None):
    """-> (dist2 (nq, k) fp32 ascending, index (nq, k) int64): per query the k support points smallest under (d, index)
    among those with d <= float32(max_dist^2) (None: all).  Slots nothing qualifies for hold +inf / -1."""
    return _knn(query, support, k, _r2(max_dist, "max_dist"))


def nearest(query, support, max_dist=None, return_index=False):
    """The reference's get_nearest_neighbor: -> (nq,) fp32 Euclidean distance to the nearest support point (and its index);
    with max_dist, +inf / -1 where the nearest is farther."""
    dist2, index = knn(query, support, 1, max_dist)
    dist = torch.sqrt(dist2[:, 0])
    return (dist, index[:, 0]) if return_index else dist


@torch.no_grad()
def radius_pairs(query, support, radius):
    """-> (total, 2) int64: every (i, j) with d(i, j) <= float32(radius^2), ordered by (i, j) ascending."""
    _check_pair(query, support)
    r2 = _r2(radius, "radius")
    query, support = query.detach(), support.detach()
    dev, nq, ns = query.device, query.shape[0], support.shape[0]
    # the grid stays in this buffer between the two calls, so it is the call's own and not the shared scratch
    ws = torch.empty(max(_lib.lib().gr_cloud_radius_workspace_bytes(nq, ns), 1), dtype=torch.uint8, device=dev)
    h_total = ctypes.c_int64(0)
    _finite(lambda: _lib.call(dev, "gr_cloud_radius_count", query, nq, support, ns, r2, None, ctypes.byref(h_total), ws=ws))
    total = h_total.value
    pairs = torch.empty((total, 2), dtype=torch.int64, device=dev)
    if total:
        scratch = torch.empty(total, dtype=torch.int32, device=dev)
        _lib.call(dev, "gr_cloud_radius_pairs", query, nq, support, ns, r2, total, scratch, pairs, ws=ws)
    return pairs


# ---- the reference's functions (geotransformer/utils/registration.py) ------------------------------------------------------

def _transform(transform):
    """A (4, 4) transform given as a tensor, an array or nested lists -> float64 on the host."""
    t = transform.detach().cpu().numpy() if isinstance(transform, torch.Tensor) else np.asarray(transform)
    if t.shape != (4, 4):
        raise ValueError(f"transform: shape {t.shape}, must be (4, 4)")
    return t.astype(np.float64)


def apply_transform(points, transform):
    """points (N, 3) fp32 -> R points + t, in fp32 on the device of `points`."""
    t = torch.as_tensor(_transform(transform), dtype=torch.float32, device=points.device)
    return (points @ t[:3, :3].T + t[:3, 3]).contiguous()


def _strict_cap(radius):
    """A cap for the nearest-neighbour search of a test `distance < radius` that leaves the test's outcome as the uncapped
    search gives it.  The distance is fl(sqrt(d)) in fp32.  fl(sqrt(d)) < r does NOT imply d <= fl(r r): sqrt rounds to
    nearest, so sqrt(d) may exceed the fp32 number below r by half an ulp, and fl(r r) may lie half an ulp under r r; together
    d < fl(r r) (1 + 2^-24)^2 / (1 - 2^-24) < fl(r r) (1 + 3 2^-24), which is at most three ulps above fl(r r).  Four ulps
    cover it; rows the wider cap lets in are judged by the test itself afterwards."""
    cap = np.float32(_r2(radius, "positive_radius"))
    for _ in range(4):
        cap = np.nextafter(cap, np.float32(np.inf))
    return float(cap)


def compute_overlap(ref_points, src_points, transform=None, positive_radius=0.1):
    """The share of ref points whose nearest (transformed) src point is closer than positive_radius."""
    if transform is not None:
        src_points = apply_transform(src_points, transform)
    if ref_points.shape[0] == 0:
        return float("nan")
    dist2, _ = _knn(ref_points, src_points, 1, _strict_cap(positive_radius))
    near = torch.sqrt(dist2[:, 0]).double() < float(positive_radius)
    return int(near.sum()) / ref_points.shape[0]


def get_correspondences(ref_points, src_points, transform, matching_radius):
    """Ground-truth correspondences: (total, 2) int64 [index in ref_points, index in src_points] of every pair within
    matching_radius after the transform, ordered by (ref, src) ascending."""
    return radius_pairs(ref_points, apply_transform(src_points, transform), matching_radius)


def compute_modified_chamfer_distance(raw_points, ref_points, src_points, gt_transform, est_transform):
    """The modified chamfer distance of RPMNet, as the reference computes it."""
    est, gt = _transform(est_transform), _transform(gt_transform)
    p_q = nearest(apply_transform(src_points, est), raw_points).double().mean()
    q_p = nearest(ref_points, apply_transform(raw_points, est @ np.linalg.inv(gt))).double().mean()
    return float(p_q + q_p)


def _residuals(ref_corr_points, src_corr_points, transform):
    return torch.sqrt(((ref_corr_points - apply_transform(src_corr_points, transform)) ** 2).sum(1))


def compute_correspondence_residual(ref_corr_points, src_corr_points, transform):
    """Mean distance between corresponding points after the transform."""
    return float(_residuals(ref_corr_points, src_corr_points, transform).double().mean())


def compute_inlier_ratio(ref_corr_points, src_corr_points, transform, positive_radius=0.1):
    """The share of correspondences closer than positive_radius after the transform."""
    return float((_residuals(ref_corr_points, src_corr_points, transform).double() < float(positive_radius)).double().mean())


def evaluate_correspondences(ref_points, src_points, transform, positive_radius=0.1):
    return {"overlap": compute_overlap(ref_points, src_points, transform, positive_radius=positive_radius),
            "inlier_ratio": compute_inlier_ratio(ref_points, src_points, transform, positive_radius=positive_radius),
            "residual": compute_correspondence_residual(ref_points, src_points, transform),
            "num_corr": ref_points.shape[0]}


def compute_registration_rmse(src_points, gt_transform, est_transform):
    """Mean distance between the points under the two transforms (the reference's approximated RMSE of 3DMatch)."""
    diff = apply_transform(src_points, gt_transform) - apply_transform(src_points, est_transform)
    return float(torch.linalg.norm(diff, dim=1).double().mean())


REFERENCE_NAMES = ("compute_overlap", "get_correspondences", "compute_modified_chamfer_distance", "compute_inlier_ratio",
                   "compute_correspondence_residual", "evaluate_correspondences", "compute_registration_rmse")


def array_api(fn, clouds):
    """`fn` for callers that hold numpy arrays (the alias tree geotransformer/utils): the first `clouds` positional
    arguments are point clouds; arrays among them go to the current GPU as contiguous fp32 tensors, and then what comes
    back is numpy: tensors as arrays, numbers as numpy scalars.  Tensors in, tensors out, as without the wrapper."""
    import functools

    def out(v):
        if isinstance(v, torch.Tensor):
            return v.cpu().numpy()
        if isinstance(v, (tuple, list)):
            return type(v)(out(x) for x in v)
        if isinstance(v, dict):
            return {k: out(x) for k, x in v.items()}
        return np.float64(v) if isinstance(v, float) else v

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        args = list(args)
        from_numpy = False
        for i in range(min(clouds, len(args))):
            if isinstance(args[i], np.ndarray):
                from_numpy = True
                args[i] = torch.from_numpy(np.ascontiguousarray(args[i], dtype=np.float32)).to(_lib.require_gpu())
        res = fn(*args, **kwargs)
        return out(res) if from_numpy else res
    return wrapper
