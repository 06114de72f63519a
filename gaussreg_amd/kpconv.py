"""Mirror of geotransformer/modules/kpconv: KPConv + maxpool + nearest_upsample on HIP -- inference by default, with
autograd (HIP backward, csrc/kpconv_backward.hip) inside `differentiable()`.

`KPConv` keeps the reference's parameters / buffers (`weights` (K,Cin,Cout), optional `bias`, buffer
`kernel_points` (K,3)) so reference checkpoints load with the same state-dict keys (kpconv.py:54-65).
Kernel points: like the reference, a fresh module gets the disposition `k_015_center_3D` (the only one GaussReg uses:
kernel_size 15, config.py:81) scaled by the radius, jittered and rotated about z (kernel_points.py:389-455); the
reference reads those 15 points from a PLY asset through open3d, here they are a table.  Other kernel sizes would need
the reference's kernel optimiser, which is not reproduced: such a module must get `kernel_points` passed in or loaded
from a checkpoint and refuses to run until then.
"""
import contextlib
import functools
import math
import threading
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _lib

# the 15 points of geotransformer/modules/kpconv/dispositions/k_015_center_3D.ply (unit-radius disposition, first = centre)
K015_CENTER_3D = np.array([
    [0.0, 0.0, 0.0], [-0.49820612, 0.41826797, 0.11736718], [-0.24123565, -0.34214048, -0.5115481],
    [-0.2828808, -0.58614266, 0.11553228], [0.29054036, -0.10093209, -0.585091], [0.42820039, 0.39929883, -0.30681813],
    [-0.63586493, -0.08196441, -0.16090403], [-0.43181082, -0.14729417, 0.47830957], [-0.044666, 0.27973214, 0.59723308],
    [0.22552417, -0.34462544, 0.50794659], [0.63889212, -0.16914906, -0.01190108], [-0.22552415, 0.34462545, -0.50794659],
    [0.49054666, 0.26880703, 0.35219206], [0.25233084, -0.59706653, -0.12951142], [0.03415394, 0.65858341, 0.04513958]])


def load_kernels(radius, num_kpoints, dimension=3, fixed='center'):
    """kernel_points.py:389-455 for the stored disposition: unit kernel + N(0, 0.01) noise, scaled by `radius`, rotated
    by a random angle about z (numpy's global RNG, like the reference).  Returns (K, 3) float32."""
    if (num_kpoints, dimension, fixed) != (15, 3, 'center'):
        raise NotImplementedError("only the k_015_center_3D disposition is available (the kernel-point optimiser of "
                                  "kernel_points.py is not reproduced); pass kernel_points or load a checkpoint")
    theta = np.random.rand() * 2 * np.pi
    c, s_ = np.cos(theta), np.sin(theta)
    R = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1]], dtype=np.float32)
    pts = K015_CENTER_3D.astype(np.float32) + np.random.normal(scale=0.01, size=K015_CENTER_3D.shape)
    return np.matmul(radius * pts, R).astype(np.float32)


_mode = threading.local()


@contextlib.contextmanager
def differentiable(chunk_rows=0, fused_norm=False):
    """Inside this context, with grad mode on, `KPConv.forward`, `maxpool` and `nearest_upsample` run the same forward
    kernels as outside it and return tensors with a `grad_fn` whenever `s_feats` / `weights` / `bias` (or `x`) require
    grad; `KPConvFPN.forward` no longer switches grad off.  The transformer stack consults the same switch
    (gaussreg_amd.transformer, .rpe_attention, .embedding), and so do log-Sinkhorn (gaussreg_amd.sinkhorn), the dim-0
    `ops.index_select` of a float32 tensor that requires grad, and `model.GeoTransformer.forward`, whose training branch runs
    only in here: backbone, transformer, patch gather and fine matching become differentiable together.
    Points, kernel points and indices get no gradient: a `q_points` / `s_points` that requires grad raises ValueError.
    Outside the context every call is inference, as before.  Thread-local.  `chunk_rows` > 0 overrides the number of
    queries the KPConv backward processes per chunk (tests).
    `fused_norm=True` (opt-in) also runs the backbone's GroupNorm layers in HIP, forward and backward
    (kpconv_blocks.GroupNorm: gr_group_norm_train / gr_group_norm_backward, with the residual add and the LeakyReLU of a
    block's tail fused); `kpconv_blocks.norm_segments` is then accepted, so several pairs train in one pass.  With the
    default every layer takes the torch path it took before, bit for bit."""
    old = getattr(_mode, "state", None)
    _mode.state = (True, int(chunk_rows), bool(fused_norm))
    try:
        yield
    finally:
        _mode.state = old


def differentiable_active():
    """True inside `differentiable()` while grad mode is on."""
    return getattr(_mode, "state", None) is not None and torch.is_grad_enabled()


def fused_norm_active():
    """True inside `differentiable(fused_norm=True)` while grad mode is on."""
    state = getattr(_mode, "state", None)
    return state is not None and state[2] and torch.is_grad_enabled()


def no_grad_unless_differentiable(fn):
    """Decorator of the forwards that are inference-only outside the context: `@torch.no_grad()` unless
    `differentiable_active()`, in which case the call runs with autograd as it is."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        if differentiable_active():
            return fn(*args, **kwargs)
        with torch.no_grad():
            return fn(*args, **kwargs)
    return wrapper


_inv_cache = {}


def inverted_index(neighbor_indices, n, first_column_only=False):
    """The inverted neighbour index the backward kernels sum through: (edges, offsets), both int64 on the indices' device.
    `edges` lists the valid entries of `neighbor_indices` (M, H) as m * H + h, grouped by the support row they name and
    ascending inside a group (a stable sort of the flattened indices); row r owns edges[offsets[r]:offsets[r + 1]].
    One neighbour tensor serves several layers, so the result is cached per (tensor, version) for as long as that tensor
    lives: the entry goes when the tensor does, so no device memory outlives the pyramid it was built for."""
    stamp = _lib.tensor_stamp([neighbor_indices])
    key = None if stamp is None else (stamp, tuple(neighbor_indices.shape), int(n), bool(first_column_only))
    hit = _inv_cache.get(key) if key is not None else None
    if hit is not None and hit[0]() is not None:  # alive: its address and version are still its own
        return hit[1], hit[2]
    with torch.no_grad():
        M, H = neighbor_indices.shape
        flat = neighbor_indices.reshape(-1)
        eid = torch.arange(M * H, device=flat.device, dtype=torch.int64)
        if first_column_only and H > 0:
            flat, eid = neighbor_indices[:, 0].contiguous(), eid[::H].contiguous()
        valid = (flat >= 0) & (flat < n)
        keys, eid = flat[valid], eid[valid]
        keys, perm = torch.sort(keys, stable=True)
        edges = eid[perm].contiguous()
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=flat.device)
        if n > 0:
            offsets[1:] = torch.cumsum(torch.bincount(keys, minlength=n), 0)
    if key is not None:
        ref = weakref.ref(neighbor_indices)
        _inv_cache[key] = (ref, edges, offsets)
        weakref.finalize(neighbor_indices, _inv_cache_drop, key, ref)
    return edges, offsets


def _inv_cache_drop(key, ref):
    hit = _inv_cache.get(key)
    if hit is not None and hit[0] is ref:
        del _inv_cache[key]


def _kpconv_forward(f, q, s, nb, kp, wts, b, sigma, inf):
    """gr_kpconv_forward on float32 / int64 contiguous tensors of one GPU."""
    dev = f.device
    N, Cin = f.shape
    M, H = nb.shape
    K, _, Cout = wts.shape
    out = torch.empty((M, Cout), dtype=torch.float32, device=dev)
    _lib.call(dev, "gr_kpconv_forward", f, q, s, nb, N, M, H, Cin, Cout, kp, K, wts, b, float(sigma), float(inf), out,
              ws=_lib.lib().gr_kpconv_workspace_bytes(N, M, K, Cin))
    return out


class _KPConvFunction(torch.autograd.Function):
    """Forward: the inference kernels.  Backward: gr_kpconv_backward.  Nothing but the inputs is saved: WF is recomputed."""

    @staticmethod
    def forward(ctx, f, wts, b, q, s, nb, kp, sigma, inf, chunk_rows):
        f, wts = f.contiguous(), wts.contiguous()
        b = None if b is None else b.contiguous()
        ctx.save_for_backward(f, wts, q, s, nb, kp)
        ctx.has_bias, ctx.sigma, ctx.inf, ctx.chunk_rows = b is not None, float(sigma), float(inf), int(chunk_rows)
        return _kpconv_forward(f, q, s, nb, kp, wts, b, sigma, inf)

    @staticmethod
    def backward(ctx, grad_out):
        f, wts, q, s, nb, kp = ctx.saved_tensors
        dev = f.device
        N, Cin = f.shape
        M, H = nb.shape
        K, _, Cout = wts.shape
        go = grad_out.to(torch.float32).contiguous()  # .sum().backward() hands over an expanded zero-stride tensor
        need_f, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        gf = torch.empty_like(f) if need_f else None
        gw = torch.empty_like(wts) if need_w else None
        gb = torch.empty(Cout, dtype=torch.float32, device=dev) if need_b else None
        needs = (1 if need_f else 0) | (2 if need_w else 0) | (4 if need_b else 0)
        if needs:
            edges = offsets = None
            if need_f and N > 0 and M > 0 and H > 0:
                edges, offsets = inverted_index(nb, N)
            _lib.call(dev, "gr_kpconv_backward", f, q, s, nb, N, M, H, Cin, Cout, kp, K, wts, ctx.sigma, ctx.inf, go, edges,
                      offsets, gf, gw, gb, ctx.chunk_rows,
                      ws=_lib.lib().gr_kpconv_backward_workspace_bytes(N, M, H, Cin, Cout, K, needs, ctx.chunk_rows))
        return gf, gw, gb, None, None, None, None, None, None, None


class _PoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, nb, mode):
        x = x.contiguous()
        ctx.save_for_backward(x, nb)
        ctx.mode = mode
        return _pool_forward(x, nb, mode)

    @staticmethod
    def backward(ctx, grad_out):
        x, nb = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        dev = x.device
        N, C = x.shape
        M, H = nb.shape
        go = grad_out.to(torch.float32).contiguous()
        gx = torch.empty_like(x)
        edges, offsets = inverted_index(nb, N, first_column_only=ctx.mode == 1)
        _lib.call(dev, "gr_neighbor_pool_backward", x, N, C, nb, M, H, ctx.mode, go, edges, offsets, gx, ws=M * C * 4 + 256)
        return gx, None, None


def _no_point_grad(**points):
    for name, t in points.items():
        if t.requires_grad:
            raise ValueError(f"{name} requires grad, but the HIP KPConv has no gradient with respect to the points")


class KPConv(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, radius, sigma, bias=False, dimension=3, inf=1e6,
                 eps=1e-9, kernel_points=None):
        super().__init__()
        self.kernel_size, self.in_channels, self.out_channels = kernel_size, in_channels, out_channels
        self.radius, self.sigma, self.dimension, self.inf, self.eps = radius, sigma, dimension, inf, eps
        self.weights = nn.Parameter(torch.zeros(kernel_size, in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter('bias', None)
        nn.init.kaiming_uniform_(self.weights, a=math.sqrt(5))  # kpconv.py:68
        if self.bias is not None:
            fan_in, _ = nn.init._calculate_fan_in_and_fan_out(self.weights)
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)
        self._kernel_points_ready = True
        if kernel_points is not None:
            kp = torch.as_tensor(kernel_points).float()
        else:
            try:
                kp = torch.from_numpy(load_kernels(radius, kernel_size, dimension=dimension, fixed='center')).float()
            except NotImplementedError:
                kp = torch.zeros(kernel_size, dimension)  # placeholder until a checkpoint fills it
                self._kernel_points_ready = False
        self.register_buffer('kernel_points', kp)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        if prefix + 'kernel_points' in state_dict:
            self._kernel_points_ready = True
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    @no_grad_unless_differentiable
    def forward(self, s_feats, q_points, s_points, neighbor_indices):
        """Inside `differentiable()` the same kernels run through one autograd Function; the conversions around it are torch
        ops with their own grad."""
        if not self._kernel_points_ready:
            raise RuntimeError("KPConv.kernel_points is uninitialised: no stored disposition for kernel_size=%d; pass "
                               "kernel_points= or load a state dict that carries them" % self.kernel_size)
        train = differentiable_active()
        if train:
            _no_point_grad(q_points=q_points, s_points=s_points)
        dev = _lib.require_gpu()
        out_device = s_feats.device
        f = _lib.to_device(s_feats, dev, torch.float32)
        dev = f.device
        q, s = _lib.to_device(q_points, dev, torch.float32), _lib.to_device(s_points, dev, torch.float32)
        nb = neighbor_indices.to(device=dev, dtype=torch.int64).contiguous()
        kp = _lib.to_device(self.kernel_points, dev, torch.float32)
        wts = _lib.to_device(self.weights, dev, torch.float32)
        b = None if self.bias is None else _lib.to_device(self.bias, dev, torch.float32)
        if train:
            out = _KPConvFunction.apply(f, wts, b, q, s, nb, kp, float(self.sigma), float(self.inf), _mode.state[1])
        else:
            out = _kpconv_forward(f, q, s, nb, kp, wts, b, self.sigma, self.inf)
        return _lib.like_input(out, out_device)


def _pool_forward(xx, nb, mode):
    """gr_neighbor_pool on a float32 contiguous tensor and int64 indices of one GPU."""
    dev = xx.device
    N, C = xx.shape
    M, H = nb.shape
    out = torch.empty((M, C), dtype=torch.float32, device=dev)
    _lib.call(dev, "gr_neighbor_pool", xx, N, C, nb, M, H, mode, out)
    return out


@no_grad_unless_differentiable
def _pool(x, neighbor_indices, mode):
    dev = _lib.require_gpu()
    out_device = x.device
    xx = _lib.to_device(x, dev, torch.float32)
    dev = xx.device
    nb = neighbor_indices.to(device=dev, dtype=torch.int64).contiguous()
    out = _PoolFunction.apply(xx, nb, mode) if differentiable_active() else _pool_forward(xx, nb, mode)
    return _lib.like_input(out, out_device)


def maxpool(x, neighbor_indices):
    """kpconv/functional.py:54-67.  Inside `differentiable()` the gradient goes to the neighbour row that attained the
    maximum (the lowest column on a tie; dropped where the zero shadow row won)."""
    return _pool(x, neighbor_indices, 0)


def nearest_upsample(x, upsample_indices):
    """kpconv/functional.py:6-22 (only the first neighbour column is used)."""
    return _pool(x, upsample_indices, 1)
