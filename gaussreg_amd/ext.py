"""Mirror of the reference's native module ``geotransformer.ext`` (setup.py:10, pybind.cpp:6-18).

Same two functions, same positional signatures, same error texts -- backed by the HIP kernels:

    radius_neighbors(q_points, s_points, q_lengths, s_lengths, radius) -> LongTensor (Nq, max_count)
        reference: geotransformer/extensions/cpu/radius_neighbors/radius_neighbors.cpp:5-68
    grid_subsampling(points, lengths, voxel_size) -> [s_points (M,3) f32, s_lengths (B,) i64]
        reference: geotransformer/extensions/cpu/grid_subsampling/grid_subsampling.cpp:5-62

Differences from the reference (documented in INTEGRATION.md): tensors may live on the GPU (the
reference insists on CPU tensors); CPU tensors are accepted, computed on the GPU and returned on
the CPU; outputs follow the input's device like the reference's `at::device(points.device())`.
Nothing is ever computed on the CPU.
"""
import ctypes

import torch

from . import _lib

_ORDER = {"reference": _lib.DEFINES["GR_ORDER_REFERENCE"], "cell": _lib.DEFINES["GR_ORDER_CELL"]}


def _check_float(x, name):
    if x.dtype != torch.float32:
        raise RuntimeError(f"{name} must be a float tensor")  # torch_helper.h:31-35


def _check_long(x, name):
    if x.dtype != torch.int64:
        raise RuntimeError(f"{name} must be an long tensor")  # torch_helper.h:25-29 (sic)


def _check_contig(x, name):
    if not x.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")  # torch_helper.h:12-13


def _check_points(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if x.dim() != 2 or x.shape[1] != 3:
        raise RuntimeError(f"{name} must have shape (N, 3)")


class SupportGrid:
    """Cell grid of one support cloud, kept between searches that use the SAME supports, lengths and radius with
    different queries (the data pyramid does three per level, geotransformer/utils/data.py:44-75): the first search
    bins the supports, the following ones only bin their queries (gr_radius_count_cached).  Owns its workspace, sized
    for the largest query set announced in `max_queries`.  The support tensor must not be modified in between."""

    def __init__(self, max_queries):
        self.max_queries = int(max_queries)
        self.ws = None
        self.sig = (ctypes.c_int64 * 4)()
        self.key = None          # (data_ptr, ns, nb, radius): what the grid was built for
        self._keep = None        # keeps the support tensor alive

    def workspace(self, dev, nq, ns, nb):
        need = _lib.lib().gr_radius_workspace_bytes(max(nq, self.max_queries), ns, nb)
        if self.ws is None or self.ws.numel() < need or self.ws.device != dev:
            self.ws = torch.empty((need,), dtype=torch.uint8, device=dev)
            self.key = None      # a new buffer holds no grid
        return self.ws


def _stage(dev, q_points, s_points, q_lengths, s_lengths, radius, grid):
    """What both searches do first: the clouds on the GPU (a self-search stays ONE tensor), the lengths on the host, the
    workspace -- the shared one, or the grid's -- and whether the grid already holds these supports.
    -> q, s, head (the arguments every radius entry point begins with), ws, sig, reuse, key (what the grid holds afterwards)"""
    same = s_points is q_points or (s_points.data_ptr() == q_points.data_ptr() and s_points.shape == q_points.shape)
    q = q_points if q_points.is_cuda else q_points.to(dev)
    s = q if same else (s_points if s_points.is_cuda else s_points.to(dev))
    ql, sl = q_lengths.tolist(), s_lengths.tolist()
    nq, ns, nb = q.shape[0], s.shape[0], len(ql)
    head = (q, s, _lib.host_i64(ql), _lib.host_i64(sl), nq, ns, nb, float(radius))
    # (the radius entry points take their workspace in the middle of the argument list: it is passed like any tensor)
    if grid is None:
        return q, s, head, _lib.workspace(q.device, _lib.lib().gr_radius_workspace_bytes(nq, ns, nb)), None, 0, None
    ws = grid.workspace(q.device, nq, ns, nb)
    key = (s.data_ptr(), ns, nb, float(radius), tuple(sl))
    reuse = 1 if (grid.key == key and ns > 0 and nq > 0) else 0
    return q, s, head, ws, grid.sig, reuse, key if (ns > 0 and nq > 0 and nb > 0) else None


def _searched(grid, key, s):
    """After a search: the grid holds the supports `s` (key None: nothing was binned) -> `reuse` for a repeat of the call."""
    if grid is None:
        return 0
    grid.key, grid._keep = key, s
    return 1 if key is not None else 0


def _radius(q_points, s_points, q_lengths, s_lengths, radius, neighbor_limit, grid, checks):
    dev = _lib.require_gpu()
    if checks:
        for t, n in ((q_points, "q_points"), (s_points, "s_points")):
            _check_points(t, n)
            _check_float(t, n)
        for t, n in ((q_lengths, "q_lengths"), (s_lengths, "s_lengths")):
            _check_long(t, n)
        for t, n in ((q_points, "q_points"), (s_points, "s_points"), (q_lengths, "q_lengths"), (s_lengths, "s_lengths")):
            _check_contig(t, n)
        if q_lengths.numel() != s_lengths.numel():
            raise RuntimeError("q_lengths and s_lengths must have the same number of batch elements")
    q, s, head, ws, sig, reuse, key = _stage(dev, q_points, s_points, q_lengths, s_lengths, radius, grid)
    dev, (nq, ns, nb) = q.device, head[4:7]
    info = (ctypes.c_int64 * 4)()
    _lib.call(dev, "gr_radius_count_cached", *head, ws, ws.numel(), info, sig, reuse)
    _searched(grid, key, s)
    width = int(info[0])
    if neighbor_limit is not None and neighbor_limit > 0:
        width = min(width, int(neighbor_limit))
    out = torch.empty((nq, width), dtype=torch.int64, device=dev)
    if nq > 0 and width > 0:
        _lib.call(dev, "gr_radius_fill", q, s, nq, ns, nb, float(radius), width, info, out, ws=ws)
    return _lib.like_input(out, q_points.device)


_WIDTH_HINT = {}  # (radius, neighbor_limit) -> largest neighbour count of the LAST search of that call site (not a running maximum)


def _radius_limited(q_points, s_points, q_lengths, s_lengths, radius, neighbor_limit, grid, contiguous=True):
    """radius_search with neighbor_limit > 0: the (nq, limit) rows are allocated before anything is counted and ONE
    kernel searches, ranks and writes them (gr_radius_search); the read-back of max_count only decides whether the
    reference would have returned fewer columns (radius_search.py:25-26 keeps min(max_count, limit))."""
    q, s, head, ws, sig, reuse, key = _stage(_lib.require_gpu(), q_points, s_points, q_lengths, s_lengths, radius, grid)
    dev, (nq, ns, nb) = q.device, head[4:7]
    limit = int(neighbor_limit)
    info = (ctypes.c_int64 * 6)()
    # Row stride of the search.  The reference's limit is an upper bound chosen by calibration and can be far above
    # what a level ever returns (the demo pyramid: limit 89, largest count 18): rows of `limit` columns would be 5 x the
    # bytes, written by the kernel and read again by the truncating copy.  A call site (radius, limit) therefore
    # remembers the largest count of its last call and searches with rows of that width + a margin (a multiple of 8: whole
    # 64-byte sectors per row piece, streaming stores); a call whose largest count does not fit is repeated at the full
    # limit -- the result is the same tensor either way.
    hint = _WIDTH_HINT.get((float(radius), limit))
    stride = limit if hint is None else min(limit, max(8, (hint + max(2, hint // 4) + 7) // 8 * 8))
    while True:
        out = torch.empty((nq, stride), dtype=torch.int64, device=dev)
        _lib.call(dev, "gr_radius_search", *head, stride, out, ws, ws.numel(), info, sig, reuse)
        reuse = _searched(grid, key, s)
        if int(info[0]) <= stride or stride == limit:
            break
        stride = limit
    if nq > 0 and ns > 0 and nb > 0:
        _WIDTH_HINT[(float(radius), limit)] = int(info[0])
        if len(_WIDTH_HINT) > 4096:
            _WIDTH_HINT.clear()
    width = min(int(info[0]), limit)
    if width < stride:
        # (contiguous=False: the column slice of the searched rows, row stride `stride` -- what the reference itself returns
        # when it truncates, radius_search.py:26; saves a copy of the whole result where nobody needs it dense)
        out = out[:, :width].contiguous() if contiguous else out[:, :width]
    return _lib.like_input(out, q_points.device)


def radius_neighbors(q_points, s_points, q_lengths, s_lengths, radius, grid=None):
    """`grid`: optional SupportGrid shared by consecutive searches over the same supports and radius."""
    return _radius(q_points, s_points, q_lengths, s_lengths, radius, None, grid, True)


def radius_neighbors_limited(q_points, s_points, q_lengths, s_lengths, radius, neighbor_limit, grid=None, two_pass=False,
                             contiguous=True):
    """radius_neighbors + the column truncation of modules/ops/radius_search.py:25-26 done inside the
    kernel: only min(max_count, neighbor_limit) columns are ever written (contiguous result).  With a positive limit the
    search is ONE pass (gr_radius_search); `two_pass=True` forces the count + fill pair the bare radius_neighbors uses."""
    if neighbor_limit is not None and neighbor_limit > 0 and not two_pass:
        return _radius_limited(q_points, s_points, q_lengths, s_lengths, radius, neighbor_limit, grid, contiguous)
    return _radius(q_points, s_points, q_lengths, s_lengths, radius, neighbor_limit, grid, False)


def grid_subsampling(points, lengths, voxel_size, order="reference"):
    """`order="reference"` (default) reproduces the reference's row order bit for bit;
    `order="cell"` keeps everything on the device (rows sorted by voxel key)."""
    dev = _lib.require_gpu()
    _check_points(points, "points")
    _check_float(points, "points")
    _check_long(lengths, "lengths")
    _check_contig(points, "points")
    _check_contig(lengths, "lengths")
    out_device = points.device
    p = points if points.is_cuda else points.to(dev)
    dev = p.device
    lens = lengths.tolist()
    n, nb = p.shape[0], len(lens)
    hl = _lib.host_i64(lens)
    out_l = (ctypes.c_int64 * max(nb, 1))()
    total = ctypes.c_int64(0)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    _lib.call(dev, "gr_grid_subsample", p, hl, n, nb, float(voxel_size), _ORDER[order], out, out_l, ctypes.byref(total),
              ws=_lib.lib().gr_grid_subsample_workspace_bytes(n, nb))
    s_points = out[: total.value]
    if total.value * 4 < 3 * n:
        s_points = s_points.clone()  # do not pin the (n, 3) allocation behind a view of less than three quarters of it: the
                                     # pyramid keeps every level's output (the copy costs 20 - 40 us per call)
    s_lengths = torch.tensor([out_l[b] for b in range(nb)], dtype=torch.int64, device=lengths.device)
    if out_device.type != "cuda":
        s_points = s_points.to(out_device)
    return [s_points, s_lengths]
