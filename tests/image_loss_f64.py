"""Float64 restatement of the photometric loss gaussreg_amd.image_loss computes (the public 3DGS loss_utils formulas):

    loss_v = (1 - lam) * l1 + lam * (1 - ssim_mean),   S = sum_p w_p,
    l1 = sum_{c,p} w_p |x - y| / (C S),   ssim_mean = sum_{c,p} w_p ssim / (C S)

with the 11 x 11 Gaussian window (sigma 1.5; fp32-rounded taps widened to double), zero padding 5, C1 = 0.01^2, C2 = 0.03^2.
`loss_terms` is the value (differentiable by autograd), `backward` the hand-derived gradient to x, `conv_loss` the same
value composed from five grouped F.conv2d calls in any dtype -- the stock-torch composition the GPU tests use as the fp32
yardstick.  Works on any device.
"""
import numpy as np
import torch
import torch.nn.functional as F

C1 = 0.01 ** 2
C2 = 0.03 ** 2
RADIUS = 5


def window():
    """The 11 taps: float64 Gaussian, normalised to sum 1, rounded once to fp32."""
    i = np.arange(11, dtype=np.float64)
    g = np.exp(-(i - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(np.float32)


def _taps(ref):
    return torch.from_numpy(window().astype(np.float64)).to(ref.device)


def blur(t):
    """g g^T window means of a (V, C, H, W) float64 tensor, zero padded, as two passes of shifted slices."""
    g = _taps(t)
    H, W = t.shape[-2:]
    p = F.pad(t, (RADIUS, RADIUS, 0, 0))
    t = sum(g[k] * p[..., :, k:k + W] for k in range(11))
    p = F.pad(t, (0, 0, RADIUS, RADIUS))
    return sum(g[k] * p[..., k:k + H, :] for k in range(11))


def _as4(x, y, w):
    if x.dim() == 3:
        x, y = x[None], y[None]
        if w is not None and w.dim() == 2:
            w = w[None]
    if w is None:
        w = torch.ones(x.shape[0], x.shape[2], x.shape[3], dtype=x.dtype, device=x.device)
    return x, y, w


def ssim_parts(x, y):
    mx, my = blur(x), blur(y)
    sxx = blur(x * x) - mx * mx
    syy = blur(y * y) - my * my
    sxy = blur(x * y) - mx * my
    A1, A2 = 2 * mx * my + C1, 2 * sxy + C2
    B1, B2 = mx * mx + my * my + C1, sxx + syy + C2
    return mx, my, A1, A2, B1, B2


def ssim_map(x, y):
    _, _, A1, A2, B1, B2 = ssim_parts(x, y)
    return (A1 * A2) / (B1 * B2)


def _normalise(l1_sum, ss_sum, S, C, lam):
    ok = S > 0
    den = torch.where(ok, C * S, torch.ones_like(S))
    l1 = torch.where(ok, l1_sum / den, torch.zeros_like(S))
    ss = torch.where(ok, ss_sum / den, torch.zeros_like(S))
    loss = torch.where(ok, (1 - lam) * l1 + lam * (1 - ss), torch.zeros_like(S))
    return loss, torch.stack([l1, ss, S], dim=1)


def loss_terms(x, y, w=None, lam=0.2):
    """(loss (V,), terms (V, 3) = l1, ssim_mean, S) in the dtype of x (float64 for the reference)."""
    x, y, w = _as4(x, y, w)
    C = x.shape[1]
    S = w.sum(dim=(1, 2))
    l1_sum = (w[:, None] * (x - y).abs()).sum(dim=(1, 2, 3))
    ss_sum = (w[:, None] * ssim_map(x, y)).sum(dim=(1, 2, 3))
    return _normalise(l1_sum, ss_sum, S, C, lam)


def backward(x, y, w=None, lam=0.2, dL=None):
    """Hand-derived d (sum_v dL_v loss_v) / d x; sign(0) = 0 in the L1 term; zeros for a view with S = 0."""
    squeeze = x.dim() == 3
    x, y, w = _as4(x, y, w)
    V, C = x.shape[:2]
    if dL is None:
        dL = torch.ones(V, dtype=x.dtype, device=x.device)
    mx, my, A1, A2, B1, B2 = ssim_parts(x, y)
    ssim = (A1 * A2) / (B1 * B2)
    dsxy = 2 * A1 / (B1 * B2)
    dsx = -ssim / B2
    dmu = 2 * my * A2 / (B1 * B2) - ssim * 2 * mx / B1 - 2 * mx * dsx - my * dsxy
    wm = w[:, None]
    dssim = blur(wm * dmu) + 2 * x * blur(wm * dsx) + y * blur(wm * dsxy)
    S = w.sum(dim=(1, 2))
    scale = torch.where(S > 0, dL / (C * torch.where(S > 0, S, torch.ones_like(S))), torch.zeros_like(S))
    g = scale[:, None, None, None] * ((1 - lam) * wm * torch.sign(x - y) - lam * dssim)
    return g[0] if squeeze else g


def conv_blur(t):
    C = t.shape[1]
    g = torch.from_numpy(window()).to(device=t.device, dtype=t.dtype)
    k = (g[:, None] * g[None, :]).expand(C, 1, 11, 11).contiguous()
    return F.conv2d(t, k, padding=RADIUS, groups=C)


def conv_loss(x, y, w=None, lam=0.2):
    """The stock-torch composition in the dtype of x: five grouped conv2d with the 2-D window, then elementwise passes."""
    x, y, w = _as4(x, y, w)
    C = x.shape[1]
    mx, my = conv_blur(x), conv_blur(y)
    sxx = conv_blur(x * x) - mx * mx
    syy = conv_blur(y * y) - my * my
    sxy = conv_blur(x * y) - mx * my
    ssim = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    S = w.sum(dim=(1, 2))
    l1_sum = (w[:, None] * (x - y).abs()).sum(dim=(1, 2, 3))
    ss_sum = (w[:, None] * ssim).sum(dim=(1, 2, 3))
    return _normalise(l1_sum, ss_sum, S, C, lam)


def numpy_direct(x, y, w=None, lam=0.2):
    """Non-separable 121-tap double loops over one (C, H, W) pair (numpy float64): (loss, l1, ssim_mean, S)."""
    g = window().astype(np.float64)
    C, H, W = x.shape
    w = np.ones((H, W)) if w is None else w
    l1_sum = ss_sum = 0.0
    for c in range(C):
        for i in range(H):
            for j in range(W):
                ex = ey = exx = eyy = exy = 0.0
                for a in range(11):
                    ii = i + a - RADIUS
                    if ii < 0 or ii >= H:
                        continue
                    for b in range(11):
                        jj = j + b - RADIUS
                        if jj < 0 or jj >= W:
                            continue
                        k = g[a] * g[b]
                        u, v = x[c, ii, jj], y[c, ii, jj]
                        ex += k * u
                        ey += k * v
                        exx += k * u * u
                        eyy += k * v * v
                        exy += k * u * v
                sxx, syy, sxy = exx - ex * ex, eyy - ey * ey, exy - ex * ey
                s = ((2 * ex * ey + C1) * (2 * sxy + C2)) / ((ex * ex + ey * ey + C1) * (sxx + syy + C2))
                ss_sum += w[i, j] * s
                l1_sum += w[i, j] * abs(x[c, i, j] - y[c, i, j])
    S = w.sum()
    if S == 0:
        return 0.0, 0.0, 0.0, 0.0
    l1, ss = l1_sum / (C * S), ss_sum / (C * S)
    return (1 - lam) * l1 + lam * (1 - ss), l1, ss, S
