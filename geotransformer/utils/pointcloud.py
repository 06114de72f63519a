"""utils/pointcloud.py of the reference: `get_nearest_neighbor` (:11-22, scipy's cKDTree there) runs on the HIP kernels of
gaussreg_amd.cloud_nn -- numpy in, numpy out; tensors in, tensors out.  Every other name of the reference's file
(apply_transform, random_sample_rotation, ...) is the reference's own when its checkout is on sys.path: the file runs in
this module first, then the name below replaces its one search."""
from gaussreg_amd._alias import inline_shadowed as _inline

_inline(globals())

from gaussreg_amd import cloud_nn as _nn  # noqa: E402


def _nearest(q_points, s_points, return_index=False):
    return _nn.nearest(q_points, s_points, return_index=return_index)


get_nearest_neighbor = _nn.array_api(_nearest, 2)
get_nearest_neighbor.__name__ = get_nearest_neighbor.__qualname__ = "get_nearest_neighbor"
get_nearest_neighbor.__doc__ = "Euclidean distance from every query point to its nearest support point (and its index)."
