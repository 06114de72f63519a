"""Mirror of geotransformer/modules/geotransformer/geotransformer.py:9-73 (GeometricStructureEmbedding) and
geotransformer/modules/transformer/positional_embedding.py:8-34 (SinusoidalPositionalEmbedding).
`forward` runs one fused HIP kernel per cloud (gaussreg_amd/csrc/geo_embedding.hip); state-dict keys are the
reference's (`embedding.div_term` is a buffer, `proj_d.{weight,bias}`, `proj_a.{weight,bias}`).

Inference by default.  Inside `gaussreg_amd.kpconv.differentiable()` the forward is the same kernel (the same values) inside
an autograd Function whose backward gives `proj_d` and `proj_a` their gradients from `gr_geo_embedding_backward`
(gaussreg_amd/csrc/geo_embedding_backward.hip): it re-walks the forward's pairs with the forward's own device code
(neighbour sets and indices bit for bit the forward's) and forms the two (C x C) weight gradients as fp32-MFMA products
against sinusoid rows generated on the fly; one call per cloud, the clouds of a batch accumulated in index order.  Once per
cloud and step, not once per layer.  `GeometricStructureEmbedding.grad_impl = "torch"` (or a hidden_dim that is no multiple
of 32) selects the older chunked torch recomputation, `_projection_grads`.  Points get no gradient."""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .kpconv import differentiable_active

GRAD_CHUNK_BYTES = 32 << 20   # the backward's recomputation: (rows, N, angle_k, C) temporaries of about this size


def _sinusoid(idx, div):
    om = idx.unsqueeze(-1) * div
    return torch.stack([torch.sin(om), torch.cos(om)], dim=-1).flatten(-2)     # (sin, cos) interleaved


def _projection_grads(p, go, wd, bd, wa, ba, div, sigma_d, factor_a, k, mean):
    """The fallback of the backward (`grad_impl = "torch"`, or hidden_dim % 32 != 0).
    One cloud: p (N,3), go (N,N,C) -> the gradients of out = proj_d(sin(d_idx)) + reduce_k proj_a(sin(a_idx)) with
    respect to (wd, bd, wa, ba), float32.  The indices follow geotransformer.py:38-53 with the kernel's neighbour rule
    (ascending distance, lowest index first, the first entry dropped); rows are taken in ascending chunks.
    The distances and the neighbour sets are RECOMPUTED here in torch fp32, not taken from the forward kernel: where two
    neighbours are equidistant within fp32 rounding, or a point's distance to itself does not round to exactly 0, this may
    pick another neighbour than the forward did and so differentiate a slightly different function; the
    HIP backward has no such limitation.  On clouds whose distances are exact in fp32 both sides agree."""
    N, C = p.shape[0], wd.shape[0]
    leaves = [t.detach().clone().requires_grad_(True) for t in (wd, bd, wa, ba)]
    grads = [torch.zeros_like(t) for t in leaves]
    if N == 0:
        return grads
    with torch.no_grad():
        x2 = (p * p).sum(1)
        dist = (x2[:, None] - 2.0 * (p @ p.t()) + x2[None, :]).clamp_min(0.0).sqrt()
        d_idx = dist / sigma_d
        if k > 0:
            knn = torch.sort(dist, dim=1, stable=True)[1][:, 1:k + 1]
            ref = p[knn] - p[:, None, :]                                       # (N, k, 3)
    rows = max(1, int(GRAD_CHUNK_BYTES // max(1, 3 * N * max(k, 1) * C * 4)))
    for r0 in range(0, N, rows):
        r1 = min(N, r0 + rows)
        with torch.no_grad():
            if k > 0:
                anc = p[None, :, :] - p[r0:r1, None, :]                        # (rows, N, 3)
                r = ref[r0:r1, None, :, :].expand(-1, N, -1, -1)
                a = anc[:, :, None, :].expand(-1, -1, r.shape[2], -1)
                sin = torch.linalg.norm(torch.cross(r, a, dim=-1), dim=-1)
                cos = (r * a).sum(-1)
                a_idx = torch.atan2(sin, cos) * factor_a                       # (rows, N, k)
        with torch.enable_grad():
            out = torch.nn.functional.linear(_sinusoid(d_idx[r0:r1], div), leaves[0], leaves[1])
            if k > 0:
                a_emb = torch.nn.functional.linear(_sinusoid(a_idx, div), leaves[2], leaves[3])
                out = out + (a_emb.mean(dim=2) if mean else a_emb.max(dim=2)[0])
            used = leaves if k > 0 else leaves[:2]
            for g, d in zip(grads, torch.autograd.grad(out, used, go[r0:r1])):
                g += d
    return grads


def _hip_projection_grads(m, p, go, wa, ba, div, table_a):
    """p (B,N,3), go (B,N,N,C) on the GPU -> [grad_wd, grad_bd, grad_wa, grad_ba], float32, summed over the batch by the
    kernel itself (accumulate = b > 0: cloud 0 writes, the others add, in index order)."""
    dev = p.device
    (B, N, _), C, k = p.shape, go.shape[-1], int(m.angle_k)
    shapes = ((C, C), (C,), (C, C), (C,))
    if B == 0:
        return [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes]
    gwd, gbd, gwa, gba = (torch.empty(s, dtype=torch.float32, device=dev) for s in shapes)
    nbytes = _lib.lib().gr_geo_embedding_backward_workspace_bytes(N, C, k)
    rows = 0 if table_a is None else table_a.shape[0]
    for b in range(B):
        _lib.call(dev, "gr_geo_embedding_backward", p[b], N, go[b], table_a, rows, float(m.TABLE_INV_H), wa, ba, div, C,
                  float(m.sigma_d), float(m.factor_a), k, 1 if m.reduction_a == 'mean' else 0, int(b > 0),
                  gwd, gbd, gwa, gba, ws=nbytes)
    return [gwd, gbd, gwa, gba]


class _GeoEmbeddingFunction(torch.autograd.Function):
    """Forward: the HIP kernel, whichever mode the module is in.  Backward: gr_geo_embedding_backward per cloud
    (`grad_impl == "hip"`, hidden_dim % 32 == 0), else _projection_grads per cloud."""

    @staticmethod
    def forward(ctx, module, points, wd, bd, wa, ba):
        out = module._forward_kernel(points)
        ctx.module = module
        ctx.hip = module._hip_backward()
        ctx.table_a = None
        if ctx.hip and module.reduction_a == 'max' and int(module.angle_k) > 0:
            # the 'max' winners come from the F_a table of THESE weights: the one the table-mode forward has just used; the
            # gemm modes build it here on demand (cached like the forward's; inference tensors rebuild every call)
            ctx.table_a = module._function_tables(out.device if out.is_cuda else _lib.require_gpu())[1]
        ctx.save_for_backward(points, wd, bd, wa, ba)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        points, wd, bd, wa, ba = ctx.saved_tensors
        m = ctx.module
        dev = grad_out.device if grad_out.is_cuda else _lib.require_gpu()
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        go, p, div = f(grad_out), f(points), f(m.embedding.div_term)
        if ctx.hip:
            total = _hip_projection_grads(m, p, go, f(wa), f(ba), div, ctx.table_a)
        else:
            total = None
            for b in range(p.shape[0]):
                g = _projection_grads(p[b], go[b], f(wd), f(bd), f(wa), f(ba), div, float(m.sigma_d), float(m.factor_a),
                                      int(m.angle_k), m.reduction_a == 'mean')
                total = g if total is None else [t + x for t, x in zip(total, g)]
            if total is None:
                total = [torch.zeros_like(f(t)) for t in (wd, bd, wa, ba)]
        grads = [t.to(device=w.device, dtype=w.dtype) for t, w in zip(total, (wd, bd, wa, ba))]
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


class SinusoidalPositionalEmbedding(nn.Module):
    def __init__(self, d_model):
        super().__init__()
        if d_model % 2 != 0:
            raise ValueError(f'Sinusoidal positional encoding with odd d_model: {d_model}')
        self.d_model = d_model
        div_indices = torch.arange(0, d_model, 2).float()
        div_term = torch.exp(div_indices * (-np.log(10000.0) / d_model))
        self.register_buffer('div_term', div_term)

    @torch.no_grad()
    def forward(self, emb_indices):
        """(*) -> (*, d_model), (sin, cos) interleaved; plain tensor ops (the fused kernel never materialises this)."""
        omegas = emb_indices.reshape(-1, 1, 1) * self.div_term.view(1, -1, 1)
        emb = torch.cat([torch.sin(omegas), torch.cos(omegas)], dim=2)
        return emb.view(*emb_indices.shape, self.d_model)


class GeometricStructureEmbedding(nn.Module):
    TABLE_INV_H = 32.0        # table step 1/32 of an embedding index: interpolation error ~ 2e-8
    TABLE_X_MAX_D = 256.0     # distance indices up to 256 (= 51 m at sigma_d 0.2) come from the table, beyond: direct evaluation
    grad_impl = "hip"         # the backward inside differentiable(): "hip" (gr_geo_embedding_backward) or "torch" (_projection_grads)

    def __init__(self, hidden_dim, sigma_d, sigma_a, angle_k, reduction_a='max', fp32_mfma=False, mode="table"):
        """mode="table" (default): the two projections are tabulated as functions of their scalar index once per set of
        weights (fp64) and interpolated in the kernel -- gr_geo_embedding_table; "gemm": the fused sinusoid -> matrix-core
        kernel (`fp32_mfma=True` runs it on fp32 MFMAs instead of the split-bf16 scheme)."""
        super().__init__()
        if mode not in ("table", "gemm"):
            raise ValueError("mode must be 'table' or 'gemm'")
        self.mode = "gemm" if fp32_mfma else mode
        self._tables = None
        self.fp32_mfma = bool(fp32_mfma)
        self.sigma_d = sigma_d
        self.sigma_a = sigma_a
        self.factor_a = 180.0 / (self.sigma_a * np.pi)
        self.angle_k = angle_k
        self.embedding = SinusoidalPositionalEmbedding(hidden_dim)
        self.proj_d = nn.Linear(hidden_dim, hidden_dim)
        self.proj_a = nn.Linear(hidden_dim, hidden_dim)
        self.reduction_a = reduction_a
        if self.reduction_a not in ['max', 'mean']:
            raise ValueError(f'Unsupported reduction mode: {self.reduction_a}.')

    @torch.no_grad()
    def _function_tables(self, dev):
        """F_d(x) = proj_d(embedding(x)) and F_a(x) = proj_a(embedding(x)) on the grid x = (j - 1) / TABLE_INV_H, evaluated
        in fp64 and stored as fp32 (rows x hidden_dim); rebuilt when a weight changes (version counters) or moves."""
        ps = (self.proj_d.weight, self.proj_d.bias, self.proj_a.weight, self.proj_a.bias, self.embedding.div_term)
        stamp = _lib.tensor_stamp(ps)          # None: inference tensors, no version counters -> rebuild every call
        stamp = None if stamp is None else stamp + (str(dev),)
        if stamp is None or self._tables is None or self._tables[0] != stamp:
            div = self.embedding.div_term.detach().to(dev, torch.float64)

            def table(lin, x_max):
                rows = int(x_max * self.TABLE_INV_H) + 4
                x = (torch.arange(rows, device=dev, dtype=torch.float64) - 1.0) / self.TABLE_INV_H
                om = x[:, None] * div[None, :]
                emb = torch.stack([torch.sin(om), torch.cos(om)], dim=2).reshape(rows, -1)    # (sin, cos) interleaved
                return (emb @ lin.weight.detach().to(dev, torch.float64).t()
                        + lin.bias.detach().to(dev, torch.float64)).to(torch.float32).contiguous()

            x_max_a = float(np.pi * self.factor_a) + 1.0
            self._tables = (stamp, table(self.proj_d, self.TABLE_X_MAX_D), table(self.proj_a, x_max_a))
        return self._tables[1], self._tables[2]

    def _hip_backward(self):
        """Which backward `differentiable()` uses: the HIP kernel needs hidden_dim % 32 == 0 (its MFMA slabs); any other
        width takes the torch recomputation, as `grad_impl = "torch"` does."""
        if self.grad_impl not in ("hip", "torch"):
            raise ValueError("grad_impl must be 'hip' or 'torch'")
        return self.grad_impl == "hip" and self.proj_d.weight.shape[0] % 32 == 0

    def forward(self, points):
        """points (B, N, 3) -> embeddings (B, N, N, hidden_dim), geotransformer.py:57-73.  Inside `differentiable()` the
        result carries the gradient of proj_d / proj_a (HIP backward: gr_geo_embedding_backward, see `grad_impl`); points
        that require grad raise ValueError."""
        if differentiable_active():
            if points.requires_grad:
                raise ValueError("points require grad, but the structure embedding has no gradient with respect to the points")
            return _GeoEmbeddingFunction.apply(self, points, self.proj_d.weight, self.proj_d.bias, self.proj_a.weight,
                                               self.proj_a.bias)
        with torch.no_grad():
            return self._forward_kernel(points)

    def _forward_kernel(self, points):
        dev = _lib.require_gpu()
        L = _lib.lib()
        if points.dim() != 3 or points.shape[-1] != 3:
            raise ValueError("points must be (B, N, 3)")
        out_device = points.device
        p = _lib.to_device(points, dev, torch.float32)
        dev = p.device
        B, N, _ = p.shape
        C = self.proj_d.weight.shape[0]
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        wd, bd, wa, ba, div = f(self.proj_d.weight), f(self.proj_d.bias), f(self.proj_a.weight), f(self.proj_a.bias), \
            f(self.embedding.div_term)
        out = torch.empty((B, N, N, C), dtype=torch.float32, device=dev)
        table = self.mode == "table" and C % 4 == 0
        # both entry points end in: weights, C, scales, angle_k, reduction flags, the element's output
        tail = (wd, bd, wa, ba, div, C, float(self.sigma_d), float(self.factor_a), int(self.angle_k),
                (1 if self.reduction_a == 'mean' else 0) | (2 if self.fp32_mfma and not table else 0))
        if table:
            td, ta = self._function_tables(dev)
            tail = (td, td.shape[0], ta, ta.shape[0], float(self.TABLE_INV_H)) + tail
        nbytes = L.gr_geo_embedding_workspace_bytes(N, int(self.angle_k))
        for b in range(B):
            _lib.call(dev, "gr_geo_embedding_table" if table else "gr_geo_embedding", p[b], N, *tail, out[b], ws=nbytes)
        return _lib.like_input(out, out_device)
