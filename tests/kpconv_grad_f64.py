"""Test helper (not collected): torch restatements of KPConv.forward (geotransformer/modules/kpconv/kpconv.py:90-120), maxpool
(functional.py:54-67) and nearest_upsample (functional.py:6-22) in the reference's association, dtype-generic and
differentiable by torch autograd: float64 inputs give the truth of the gradient tests, float32 inputs give the rounding
error a stock-torch fp32 implementation has against it.  Nothing here shares code with gaussreg_amd or oracle/.
"""
import torch


def kpconv_ref(s_feats, q_points, s_points, neighbor_indices, kernel_points, weights, sigma, bias=None, inf=1e6):
    s_points = torch.cat([s_points, s_points.new_zeros((1, 3)) + inf], 0)                 # shadow point at +inf
    neighbors = s_points[neighbor_indices] - q_points.unsqueeze(1)                               # (M, H, 3)
    differences = neighbors.unsqueeze(2) - kernel_points                                         # (M, H, K, 3)
    sq_distances = torch.sum(differences ** 2, dim=3)
    neighbor_weights = torch.clamp(1 - torch.sqrt(sq_distances) / sigma, min=0.0).transpose(1, 2)  # (M, K, H)
    s_feats = torch.cat((s_feats, s_feats.new_zeros((1, s_feats.shape[1]))), 0)                          # zero shadow row
    neighbor_feats = s_feats[neighbor_indices]                                                   # (M, H, C)
    weighted_feats = torch.matmul(neighbor_weights, neighbor_feats).permute(1, 0, 2)             # (K, M, C)
    output_feats = torch.sum(torch.matmul(weighted_feats, weights), dim=0)                       # (M, C_out)
    neighbor_num = torch.sum(torch.gt(torch.sum(neighbor_feats, dim=-1), 0.0), dim=-1)
    neighbor_num = torch.max(neighbor_num, torch.ones_like(neighbor_num))
    output_feats = output_feats / neighbor_num.unsqueeze(1)
    if bias is not None:
        output_feats = output_feats + bias
    return output_feats


def maxpool_ref(x, neighbor_indices):
    x = torch.cat((x, x.new_zeros((1, x.shape[1]))), 0)
    return x[neighbor_indices].max(1)[0]


def nearest_upsample_ref(x, upsample_indices):
    x = torch.cat((x, x.new_zeros((1, x.shape[1]))), 0)
    return x[upsample_indices[:, 0]]


def kpconv_grads(x, sigma, grad_out, dtype, device="cpu"):
    """Autograd of kpconv_ref in `dtype` on the arrays of kpconv_cases.build: (out, grad_f, grad_w, grad_b or None) as
    float64 NumPy arrays."""
    t = lambda a, g=False: torch.from_numpy(a).to(device=device, dtype=dtype).requires_grad_(g)
    f, w = t(x["f"], True), t(x["w"], True)
    b = None if x["b"] is None else t(x["b"], True)
    idx = torch.from_numpy(x["idx"]).to(device)
    out = kpconv_ref(f, t(x["qp"]), t(x["sp"]), idx, t(x["kp"]), w, sigma, b)
    go = torch.as_tensor(grad_out).to(device=device, dtype=dtype)
    leaves = [f, w] + ([b] if b is not None else [])
    grads = torch.autograd.grad(out, leaves, go, allow_unused=True)
    grads = [torch.zeros_like(l) if g is None else g for l, g in zip(leaves, grads)]
    np64 = lambda a: a.detach().double().cpu().numpy()
    return np64(out), np64(grads[0]), np64(grads[1]), (np64(grads[2]) if b is not None else None)
