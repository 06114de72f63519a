"""Mirror of geotransformer/modules/sinkhorn/learnable_sinkhorn.py on one fused HIP kernel.  Keeps the learnable `alpha`
parameter (state-dict key `alpha`) like the reference.

Inference by default.  Inside `gaussreg_amd.differentiable()` (grad mode on) the same forward kernel runs inside one
`torch.autograd.Function` -- the values are those of inference, bit for bit -- whose backward is one launch of
gr_sinkhorn_backward (csrc/sinkhorn.hip): `scores` and `alpha` receive gradients, the masks do not."""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .kpconv import differentiable_active, no_grad_unless_differentiable


def _sinkhorn_forward(s, rm, cm, alpha, iters, inf, drop, out=None):
    """gr_sinkhorn on contiguous float32 / bool tensors of one GPU -> (B, M+1, N+1), or (B, M, N) with `drop`."""
    B, M, N = s.shape
    if out is None:
        out = torch.empty((B, M, N) if drop else (B, M + 1, N + 1), dtype=torch.float32, device=s.device)
    _lib.call(s.device, "gr_sinkhorn", s, B, M, N, rm, cm, alpha, iters, inf, int(drop), out,
              ws=_lib.lib().gr_sinkhorn_workspace_bytes(B))
    return out


class _SinkhornFunction(torch.autograd.Function):
    """Forward: the inference kernel.  Backward: gr_sinkhorn_backward, which repeats the iterations itself -- saved are only
    the inputs, by reference."""

    @staticmethod
    def forward(ctx, s, alpha, rm, cm, iters, inf, drop):
        ctx.save_for_backward(s, alpha, rm, cm)
        ctx.args = (iters, inf, drop)
        return _sinkhorn_forward(s, rm, cm, alpha, iters, inf, drop)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        s, alpha, rm, cm = ctx.saved_tensors
        iters, inf, drop = ctx.args
        B, M, N = s.shape
        g = grad_out.to(torch.float32).contiguous()
        grad_scores = torch.empty_like(s)
        per_matrix = torch.empty((B,), dtype=torch.float32, device=s.device)
        _lib.call(s.device, "gr_sinkhorn_backward", s, B, M, N, rm, cm, alpha, iters, inf, int(drop), g, grad_scores,
                  per_matrix, ws=_lib.lib().gr_sinkhorn_backward_workspace_bytes(B, M, N, iters))
        return grad_scores, per_matrix.sum().reshape(alpha.shape), None, None, None, None, None


class LearnableLogOptimalTransport(nn.Module):
    def __init__(self, num_iterations, inf=1e12):
        super().__init__()
        self.num_iterations = num_iterations
        self.register_parameter('alpha', torch.nn.Parameter(torch.tensor(1.0)))
        self.inf = inf

    @no_grad_unless_differentiable
    def forward(self, scores, row_masks=None, col_masks=None, drop_dustbin=False, out=None):
        """scores (B, M, N) -> matching scores (B, M+1, N+1), learnable_sinkhorn.py:20-66.
        Extensions (the reference has neither argument): `drop_dustbin=True` returns (B, M, N), the matrix without its dustbin
        row and column -- what model.py:197-198 slices off right after the call; `out`: a preallocated contiguous float32
        CUDA tensor of that shape to write into (inference only).
        Inside `differentiable()` the result carries a grad_fn when `scores` or `alpha` require grad; a CPU or float64
        `scores` is converted differentiably, so the gradient arrives in the caller's tensor."""
        dev = _lib.require_gpu()
        if differentiable_active():
            if out is not None:
                raise ValueError("LearnableLogOptimalTransport: `out=` cannot be combined with training (differentiable())")
            s = scores if scores.is_cuda else scores.to(dev)
            s = s.to(torch.float32).contiguous()                      # (no detach: autograd carries the conversion)
            dev = s.device
            rm = None if row_masks is None else row_masks.to(device=dev, dtype=torch.bool).contiguous()
            cm = None if col_masks is None else col_masks.to(device=dev, dtype=torch.bool).contiguous()
            alpha = self.alpha.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
            res = _SinkhornFunction.apply(s, alpha, rm, cm, int(self.num_iterations), float(self.inf), bool(drop_dustbin))
            return res if scores.is_cuda else res.to(scores.device)
        out_device = scores.device
        s = _lib.to_device(scores, dev, torch.float32)
        dev = s.device
        B, M, N = s.shape
        rm = None if row_masks is None else row_masks.to(device=dev, dtype=torch.bool).contiguous()
        cm = None if col_masks is None else col_masks.to(device=dev, dtype=torch.bool).contiguous()
        alpha = self.alpha.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        shape = (B, M, N) if drop_dustbin else (B, M + 1, N + 1)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise ValueError("out must be a contiguous float32 tensor of shape %s on %s" % (shape, dev))
        _lib.call(dev, "gr_sinkhorn", s, B, M, N, rm, cm, alpha, int(self.num_iterations), float(self.inf),
                  int(bool(drop_dustbin)), out, ws=_lib.lib().gr_sinkhorn_workspace_bytes(B))
        return _lib.like_input(out, out_device)

    def __repr__(self):
        return self.__class__.__name__ + '(num_iterations={})'.format(self.num_iterations)
