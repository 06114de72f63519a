"""Test helper (not collected): a differentiable torch restatement of LearnableLogOptimalTransport
(geotransformer/modules/sinkhorn/learnable_sinkhorn.py:13-66) in float64 or float32, and the reverse recurrence of
csrc/sinkhorn.hip's backward written out in float64.  tests/test_sinkhorn_grad_f64_reference.py pins both (CPU);
tests/test_gpu_sinkhorn_backward.py compares gr_sinkhorn_backward with them.

The upstream gradient G counts on the live entries only (no masked row, no masked column): the loss is sum(G * out) over
them.  With that, the gradient of every masked entry of the padded matrix is exactly zero."""
import numpy as np
import torch


def live_mask(B, M, N, row_masks, col_masks):
    """(B, M+1, N+1) bool tensor: entries on no masked row or column; the dustbins are never masked."""
    rl = torch.ones((B, M + 1), dtype=torch.bool)
    cl = torch.ones((B, N + 1), dtype=torch.bool)
    if row_masks is not None:
        rl[:, :M] = torch.as_tensor(np.asarray(row_masks, bool))
    if col_masks is not None:
        cl[:, :N] = torch.as_tensor(np.asarray(col_masks, bool))
    return rl, cl, rl.unsqueeze(2) & cl.unsqueeze(1)


def forward(scores, alpha, row_masks, col_masks, num_iterations, inf=1e12, keep=None, marginal_dtype=None):
    """scores (B, M, N) and alpha (0-d) torch tensors of one dtype -> (B, M+1, N+1), learnable_sinkhorn.py:20-66 op for op.
    `keep`: a dict that receives the padded matrix 'Z' (with retain_grad when it requires grad).
    `marginal_dtype`: the dtype the log-marginals and the normaliser are evaluated in before they join the scores (default:
    the scores' own).  The reference module builds them in float32 whatever the scores are (learnable_sinkhorn.py:49-61:
    `.float()` counts, `torch.empty` buffers), so its float64 evaluation is reproduced with torch.float32 here."""
    B, M, N = scores.shape
    dtype = scores.dtype
    rl, cl, live = live_mask(B, M, N, row_masks, col_masks)
    padded_col = alpha.expand(B, M, 1)
    padded_row = alpha.expand(B, 1, N + 1)
    Z = torch.cat([torch.cat([scores, padded_col], dim=-1), padded_row], dim=1).masked_fill(~live, -inf)
    if keep is not None:
        if Z.requires_grad:
            Z.retain_grad()
        keep["Z"] = Z
    mdt = dtype if marginal_dtype is None else marginal_dtype
    nvr = rl[:, :M].to(mdt).sum(1)
    nvc = cl[:, :N].to(mdt).sum(1)
    norm = -torch.log(nvr + nvc)
    log_mu = norm.unsqueeze(1).repeat(1, M + 1)
    log_mu[:, M] = torch.log(nvc) + norm
    log_mu[~rl] = -inf
    log_nu = norm.unsqueeze(1).repeat(1, N + 1)
    log_nu[:, N] = torch.log(nvr) + norm
    log_nu[~cl] = -inf
    log_mu, log_nu, norm = log_mu.to(dtype), log_nu.to(dtype), norm.to(dtype)
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(num_iterations):
        u = log_mu - torch.logsumexp(Z + v.unsqueeze(1), dim=2)
        v = log_nu - torch.logsumexp(Z + u.unsqueeze(2), dim=1)
    return Z + u.unsqueeze(2) + v.unsqueeze(1) - norm.reshape(-1, 1, 1)


def pad_grad(G, B, M, N, drop):
    """(B, M+1, N+1) float64 NumPy upstream gradient; with `drop` G is (B, M, N) and the dustbins get zero."""
    G = np.asarray(G, np.float64)
    if not drop:
        return G
    out = np.zeros((B, M + 1, N + 1))
    out[:, :M, :N] = G
    return out


def grads_autograd(scores, alpha, row_masks, col_masks, num_iterations, G, dtype=torch.float64, drop=False, inf=1e12):
    """-> (grad_scores (B, M, N), grad_alpha, sum |gZ| over the live dustbin entries), float64 NumPy, by torch autograd of
    `forward` run in `dtype`."""
    B, M, N = np.asarray(scores).shape
    s = torch.tensor(np.asarray(scores), dtype=dtype, requires_grad=True)
    a = torch.tensor(float(alpha), dtype=dtype, requires_grad=True)
    keep = {}
    out = forward(s, a, row_masks, col_masks, num_iterations, inf, keep)
    live = live_mask(B, M, N, row_masks, col_masks)[2]
    g = torch.tensor(pad_grad(G, B, M, N, drop), dtype=dtype)
    zero = torch.zeros((), dtype=dtype)
    (torch.where(live, out, zero) * torch.where(live, g, zero)).sum().backward()
    gZ = keep["Z"].grad.double()
    dust = torch.zeros_like(live)
    dust[:, M, :] = True
    dust[:, :, N] = True
    return s.grad.double().numpy(), float(a.grad.double()), float(gZ[dust & live].abs().sum())


def grads_recurrence(scores, alpha, row_masks, col_masks, num_iterations, G, drop=False, inf=1e12):
    """The reverse sweep the kernel implements, in float64 NumPy -> (grad_scores, grad_alpha)."""
    scores = np.asarray(scores, np.float64)
    B, M, N = scores.shape
    rl, cl, live = (t.numpy() for t in live_mask(B, M, N, row_masks, col_masks))
    Z = np.full((B, M + 1, N + 1), float(alpha))
    Z[:, :M, :N] = scores
    Z[~live] = -inf
    nvr, nvc = rl[:, :M].sum(1).astype(np.float64), cl[:, :N].sum(1).astype(np.float64)
    norm = -np.log(nvr + nvc)
    log_mu = np.repeat(norm[:, None], M + 1, 1)
    log_mu[:, M] = np.log(nvc) + norm
    log_nu = np.repeat(norm[:, None], N + 1, 1)
    log_nu[:, N] = np.log(nvr) + norm

    def lse(x, axis):
        m = x.max(axis=axis, keepdims=True)
        return (m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True))).squeeze(axis)

    us, vs = [np.zeros((B, M + 1))], [np.zeros((B, N + 1))]
    for _ in range(num_iterations):                      # masked rows / columns keep 0: they take no part below
        us.append(np.where(rl, log_mu - lse(Z + vs[-1][:, None, :], 2), 0.0))
        vs.append(np.where(cl, log_nu - lse(Z + us[-1][:, :, None], 1), 0.0))
    gZ = np.where(live, pad_grad(G, B, M, N, drop), 0.0)
    gu, gv = gZ.sum(2), gZ.sum(1)
    with np.errstate(over="ignore"):
        for t in range(num_iterations, 0, -1):
            Q = np.where(live, np.exp(Z + us[t][:, :, None] + vs[t][:, None, :] - log_nu[:, None, :]), 0.0)
            gZ -= gv[:, None, :] * Q
            gu = gu - (gv[:, None, :] * Q).sum(2)
            P = np.where(live, np.exp(Z + us[t][:, :, None] + vs[t - 1][:, None, :] - log_mu[:, :, None]), 0.0)
            gZ -= gu[:, :, None] * P
            gv = -(gu[:, :, None] * P).sum(1)
            gu = np.zeros_like(gu)
    return gZ[:, :M, :N].copy(), float(gZ[:, M, :].sum() + gZ[:, :M, N].sum())
