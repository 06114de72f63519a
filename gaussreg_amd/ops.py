"""Mirror of ``geotransformer.modules.ops`` for the hot-path operators (HIP-backed).

reference: geotransformer/modules/ops/grid_subsample.py:7-22, radius_search.py:7-27.
"""
from . import ext


def grid_subsample(points, lengths, voxel_size, order="reference"):
    """Grid subsampling in stack mode -> (s_points (M,3), s_lengths (B,)).  grid_subsample.py:7-22."""
    s_points, s_lengths = ext.grid_subsampling(points, lengths, voxel_size, order=order)
    return s_points, s_lengths


def radius_search(q_points, s_points, q_lengths, s_lengths, radius, neighbor_limit, grid=None, contiguous=True):
    """Radius search in stack mode -> (N, min(max_count, neighbor_limit)) int64, padded with M.

    radius_search.py:7-27.  The reference materialises the full width and returns a NON-contiguous
    column slice (radius_search.py:26); here the truncation happens inside the fill kernel, so only
    the kept columns are ever written and the result is contiguous (what KPConv's index_select
    needs once the CPU->GPU copy that used to re-densify it is gone -- SURVEY.md section 8b).
    `grid` (optional ext.SupportGrid): reuse the support binning across searches over the same supports and radius.
    `contiguous=False`: where the rows were searched wider than the result, return the column slice (as the reference does)
    instead of a dense copy."""
    for t, n in ((q_points, "q_points"), (s_points, "s_points")):
        ext._check_points(t, n)
        ext._check_float(t, n)
        ext._check_contig(t, n)
    for t, n in ((q_lengths, "q_lengths"), (s_lengths, "s_lengths")):
        ext._check_long(t, n)
        ext._check_contig(t, n)
    return ext.radius_neighbors_limited(q_points, s_points, q_lengths, s_lengths, radius, neighbor_limit, grid=grid,
                                        contiguous=contiguous)


# ---------------------------------------------------------------------------------------------
# dense / partition operators (reference: modules/ops/pairwise_distance.py, pointcloud_partition.py)
import math  # noqa: E402

import torch  # noqa: E402

from . import _lib  # noqa: E402


def pairwise_distance(x, y, normalized=False, channel_first=False):
    """pairwise_distance.py:4-31.  (*, N, C) x (*, M, C) -> (*, N, M); the leading dims are one launch (grid.z)."""
    if channel_first:
        x, y = x.transpose(-1, -2), y.transpose(-1, -2)
    out_device = x.device
    lead = x.shape[:-2]
    if y.shape[:-2] != lead:
        raise RuntimeError("pairwise_distance: x and y must have the same leading (batch) dimensions")
    B = math.prod(lead)  # (not reshape(-1, ...): with N = 0 or M = 0 the batch count cannot be inferred)
    xs = _lib.to_device(x, None, torch.float32, "x", cast=False).reshape(B, x.shape[-2], x.shape[-1])
    ys = _lib.to_device(y, None, torch.float32, "y", cast=False).reshape(B, y.shape[-2], y.shape[-1])
    N, C = xs.shape[1:]
    M = ys.shape[1]
    out = torch.empty((B, N, M), dtype=torch.float32, device=xs.device)
    _lib.call(xs.device, "gr_pairwise_distance_batch", xs, ys, B, N, M, C, int(bool(normalized)), out,
              ws=_lib.lib().gr_pairwise_distance_batch_workspace_bytes(B, N, M))
    return _lib.like_input(out.reshape(*lead, N, M), out_device)


@torch.no_grad()
def point_to_node_partition(points, nodes, point_limit, return_count=False):
    """pointcloud_partition.py:61-111 without the (M, N) matrix.  Returns
    (point_to_node (N,), [node_sizes (M,)], node_masks (M,), node_knn_indices (M,K), node_knn_masks (M,K))."""
    out_device = points.device
    p = _lib.to_device(points, None, torch.float32, "points", cast=False)
    nd = _lib.to_device(nodes, None, torch.float32, "nodes", cast=False)
    N, M, K = p.shape[0], nd.shape[0], int(point_limit)
    dev = p.device
    p2n = torch.empty((N,), dtype=torch.int64, device=dev)
    masks = torch.empty((M,), dtype=torch.bool, device=dev)
    knn_idx = torch.empty((M, K), dtype=torch.int64, device=dev)
    knn_masks = torch.empty((M, K), dtype=torch.bool, device=dev)
    _lib.call(dev, "gr_point_to_node_partition", p, N, nd, M, K, p2n, masks, knn_idx, knn_masks,
              ws=_lib.lib().gr_point_to_node_workspace_bytes(N, M))
    res = [p2n, masks, knn_idx, knn_masks]
    if return_count:
        res.insert(1, torch.bincount(p2n, minlength=M))
    return _lib.like_input(tuple(res), out_device)


@torch.no_grad()
def point_to_node_partition_batch(points, point_lengths, nodes, node_lengths, point_limit):
    """point_to_node_partition (pointcloud_partition.py:61-111) for every (cloud, superpoints) pair of a stack in one call
    (gr_point_to_node_partition_batch): `points` (sum N_c, 3) / `nodes` (sum M_c, 3) with per-cloud lengths.  Returns
    (point_to_node (sum N,), node_masks (sum M,), node_knn_indices (sum M, K), node_knn_masks (sum M, K)); indices are LOCAL
    to their cloud, exactly what the single-cloud call returns for it."""
    p = _lib.to_device(points, None, torch.float32, "points", cast=False)
    nd = _lib.to_device(nodes, None, torch.float32, "nodes", cast=False)
    K = int(point_limit)
    dev = p.device
    po, no = _lib.offsets(point_lengths), _lib.offsets(node_lengths)
    if len(po) != len(no) or po[-1] != p.shape[0] or no[-1] != nd.shape[0]:
        raise ValueError("lengths do not match the stacked tensors")
    nclouds = len(po) - 1
    p2n = torch.empty((po[-1],), dtype=torch.int64, device=dev)
    masks = torch.empty((no[-1],), dtype=torch.bool, device=dev)
    knn_idx = torch.empty((no[-1], K), dtype=torch.int64, device=dev)
    knn_masks = torch.empty((no[-1], K), dtype=torch.bool, device=dev)
    h_po, h_no = _lib.host_i64(po), _lib.host_i64(no)
    _lib.call(dev, "gr_point_to_node_partition_batch", p, h_po, nd, h_no, nclouds, K, p2n, masks, knn_idx, knn_masks,
              ws=_lib.lib().gr_point_to_node_batch_workspace_bytes(h_po, h_no, nclouds))
    return p2n, masks, knn_idx, knn_masks


_gather_flags = {}


class _GatherRowsFunction(torch.autograd.Function):
    """index_select along dim 0 of a float32 (n, c) matrix with a gradient: the forward is the inference path of
    `index_select` itself, the backward gr_neighbor_pool_backward in mode 1 -- an (m,) index is an (m, 1) neighbour table, and
    kpconv.inverted_index supplies the fixed order in which the rows that name one source row are summed (no atomics)."""

    @staticmethod
    def forward(ctx, data, index):
        ctx.save_for_backward(data, index)
        return index_select(data.detach(), index, 0)

    @staticmethod
    def backward(ctx, grad_out):
        from .kpconv import inverted_index
        data, index = ctx.saved_tensors
        n, c = data.shape
        m = index.shape[0]
        go = grad_out.to(torch.float32).contiguous()
        gx = torch.empty_like(data)
        if n == 0 or c == 0:
            return gx, None
        table = index.reshape(m, 1)
        edges, offsets = inverted_index(table, n, first_column_only=True)
        _lib.call(data.device, "gr_neighbor_pool_backward", data, n, c, table, m, 1, 1, go, edges, offsets, gx, ws=256)
        return gx, None


def index_select(data, index, dim):
    """Advanced index select (modules/ops/index_select.py:4-31): `index` may have any shape; the `dim`-th dimension of
    `data` is replaced by index.shape.  The case the backbone runs (dim 0 of a 2-D fp32 feature / point tensor:
    kpconv.py:93-105, functional.py:17,63) is a HIP row gather; other dims / dtypes are reshaped onto it or, for
    non-float data, use torch's own gather on the device.
    Inside `gaussreg_amd.differentiable()` with grad mode on, the dim-0 case of a float32 `data` that requires grad returns a
    tensor with a grad_fn (backward: gr_neighbor_pool_backward, mode 1); outside the context nothing changes."""
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64:
        raise RuntimeError("index must be a LongTensor")
    nd = data.dim()
    dim = dim + nd if dim < 0 else dim
    if not (0 <= dim < nd):
        raise IndexError("dim out of range")
    if dim == 0 and data.dtype == torch.float32 and data.requires_grad:
        from .kpconv import differentiable_active
        if differentiable_active():
            dev = data.device if data.is_cuda else _lib.require_gpu()
            d = data.to(dev)                                  # (differentiable: the gradient arrives in the caller's tensor)
            flat = d.reshape(d.shape[0], -1).contiguous()
            out = _GatherRowsFunction.apply(flat, index.to(dev).reshape(-1).contiguous())
            out = out.reshape(tuple(index.shape) + tuple(data.shape[1:]))
            return out if data.is_cuda else out.to(data.device)
    if data.dtype != torch.float32:
        out = data.index_select(dim, index.reshape(-1))
    else:
        dev = _lib.require_gpu()
        out_device = data.device
        d = data if data.is_cuda else data.to(dev)
        dev = d.device
        # bring `dim` to the front and flatten the rest: (a_dim, rest)
        moved = d.movedim(dim, 0).contiguous()
        n = moved.shape[0]
        rest = moved.shape[1:]
        c = 1
        for r in rest:
            c *= int(r)
        flat = moved.reshape(n, max(c, 1))
        idx = index.to(dev).reshape(-1).contiguous()
        m = idx.shape[0]
        res = torch.empty((m, max(c, 1)), dtype=torch.float32, device=dev)
        key = (dev.type, dev.index)
        flag = _gather_flags.get(key)
        if flag is None:
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            _gather_flags[key] = flag
        if m > 0 and c > 0:
            eager = m <= 65536
            if eager:
                # a small gather is checked eagerly like torch's: its own flag word, so an earlier LARGE gather's pending
                # error is neither raised here nor lost (that one poisons its rows with NaN and is reported by
                # gather_error_pending)
                own = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.call(dev, "gr_gather_rows", flat, n, max(c, 1), idx, m, res, own if eager else flag)
            if eager and int(own.item()) != 0:
                raise IndexError("index out of range in index_select")
        out = _lib.like_input(res.reshape((m,) + tuple(rest)).movedim(0, dim), out_device).contiguous()
    if index.dim() > 1:
        out = out.view(*(tuple(data.shape[:dim]) + tuple(index.shape) + tuple(data.shape[dim:][1:])))
    return out


def gather_error_pending(device=None):
    """True if a large index_select (more than 65 536 rows) on `device` met an out-of-range index since the last check.  torch
    raises eagerly; the HIP gather records it on the device instead of synchronising every call, and fills the offending
    rows with NaN so that nothing downstream can mistake them for data.  GeoTransformer.forward checks this at its first
    natural synchronisation point."""
    dev = _lib.require_gpu() if device is None else torch.device(device)
    flag = _gather_flags.get((dev.type, dev.index))
    if flag is None:
        return False
    bad = int(flag.item()) != 0
    flag.zero_()
    return bad
