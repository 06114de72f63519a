"""Test helper (not collected): the GroupNorm of a (N, C) point-feature matrix (geotransformer/modules/kpconv/modules.py:32-50:
statistics per group of C / G channels over ALL rows), per row segment, with the optional residual add and LeakyReLU that
follow it in the backbone's blocks (modules.py:75, :135-138), restated with plain torch ops in any dtype and differentiable
by torch autograd: float64 inputs give the truth of the gradient tests.  `stock_composition` is the fp32 path training takes
without the fused kernels -- transpose, nn.GroupNorm's functional form, add, leaky_relu -- whose error against that truth is
the yardstick.  Nothing here shares code with gaussreg_amd or oracle/.
"""
import torch


def _segments(n, seg_off):
    if seg_off is None:
        return [(0, n)]
    off = [int(v) for v in seg_off]
    return list(zip(off[:-1], off[1:]))


def group_norm_ref(x, groups, weight=None, bias=None, eps=1e-5, negative_slope=None, residual=None, seg_off=None):
    """x (N, C); seg_off: None or B + 1 ascending row offsets.  Biased variance, as nn.GroupNorm."""
    n, c = x.shape
    rows = []
    for a, b in _segments(n, seg_off):
        if b == a:
            continue
        xs = x[a:b].reshape(b - a, groups, c // groups)
        mean = xs.mean(dim=(0, 2), keepdim=True)
        var = ((xs - mean) ** 2).mean(dim=(0, 2), keepdim=True)
        rows.append(((xs - mean) / torch.sqrt(var + eps)).reshape(b - a, c))
    y = torch.cat(rows, 0) if rows else x.new_zeros((0, c))
    if weight is not None:
        y = y * weight
    if bias is not None:
        y = y + bias
    if residual is not None:
        y = y + residual
    if negative_slope is not None:
        y = torch.where(y > 0, y, y * negative_slope)
    return y


def stock_composition(x, groups, weight=None, bias=None, eps=1e-5, negative_slope=None, residual=None, seg_off=None):
    """What GroupNorm.forward / ResidualBlock.forward run under grad mode without the fused path, once per segment."""
    n, c = x.shape
    rows = []
    for a, b in _segments(n, seg_off):
        if b == a:
            continue
        # torch.group_norm is what torch.nn.functional.group_norm calls after its Python-side size check, which refuses a
        # single row ("Expected more than 1 value per channel"); the single-row cases of the tests need the operator itself
        y = torch.group_norm(x[a:b].t().unsqueeze(0), groups, weight, bias, eps, False)
        rows.append(y.squeeze(0).t())
    y = torch.cat(rows, 0) if rows else x.new_zeros((0, c))
    if residual is not None:
        y = y + residual
    return y if negative_slope is None else torch.nn.functional.leaky_relu(y, negative_slope)


def grads(fn, x, groups, weight, bias, eps, negative_slope, residual, seg_off, grad_out, dtype):
    """Autograd of `fn` (one of the two above) in `dtype` on `x.device`: (out, grad_x, grad_residual, grad_gamma, grad_beta) as
    float64 tensors, None where the input is None."""
    t = lambda a: None if a is None else a.detach().to(dtype).requires_grad_(True)
    xs, w, b, r = t(x), t(weight), t(bias), t(residual)
    out = fn(xs, groups, w, b, eps, negative_slope, r, seg_off)
    leaves = [l for l in (xs, r, w, b) if l is not None]
    got = iter(torch.autograd.grad(out, leaves, grad_out.to(dtype), allow_unused=True))
    res = [out.detach().double()]
    for l in (xs, r, w, b):
        if l is None:
            res.append(None)
        else:
            g = next(got)
            res.append(torch.zeros_like(l).double() if g is None else g.double())
    return tuple(res)
