"""Test helper (not collected): float64 reference for the rasterizer's depth and alpha maps, on top of raster_torch64.

No second statement of the compositing: the maps are colour channels of raster_torch64.composite.  With the per-Gaussian
colour replaced by (z, 1, 0) and a black background, row 0 is depth = sum w_i z_i and row 1 is alpha = sum w_i = 1 - T.
z is the differentiable float64 view-space depth of the visible Gaussians, so autograd carries dL/dz to means3D."""
import torch

import raster_torch64 as rt


def view_z(cam, means3D):
    """Differentiable float64 view-space depth of every Gaussian (third row of the world-to-view matrix)."""
    p = means3D.to(torch.float64)
    Vm = torch.as_tensor(cam["viewmatrix"], dtype=torch.float64, device=p.device).reshape(4, 4).T
    return p @ Vm[2, :3] + Vm[2, 3]


def aux_pre(cam, pre, means3D):
    """`pre` (raster_torch64.preprocess) with the colours replaced by (z, 1, 0)."""
    z = view_z(cam, means3D)[pre["order"]]
    pre2 = dict(pre)
    pre2["rgb"] = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1)
    return pre2


def composite_aux(cam, pre, means3D, pix):
    """-> (depth (n,), alpha (n,)) of the pixels with flat indices `pix` (differentiable)."""
    c = rt.composite(aux_pre(cam, pre, means3D), [0.0, 0.0, 0.0], pix)
    return c[0], c[1]


def render(cam, bg, chunk=4096, **inputs):
    """-> (image (3, H, W), depth (H, W), alpha (H, W), radii (P,)), float64."""
    pre = rt.preprocess(cam, **inputs)
    W, H = pre["W"], pre["H"]
    dev = inputs["means3D"].device
    cols, ds, als = [], [], []
    for s in range(0, H * W, chunk):
        pix = torch.arange(s, min(s + chunk, H * W), device=dev)
        cols.append(rt.composite(pre, bg, pix))
        d, a = composite_aux(cam, pre, inputs["means3D"], pix)
        ds.append(d)
        als.append(a)
    return torch.cat(cols, 1).reshape(3, H, W), torch.cat(ds).reshape(H, W), torch.cat(als).reshape(H, W), pre["radii"]


def grads(cam, bg, g_color, g_depth, g_alpha, chunk=4096, **inputs):
    """Reference gradients of sum(color g_color) + sum(depth g_depth) + sum(alpha g_alpha) (any g_* may be None):
    (dict name -> float64 gradient, image (3, H, W), depth (H, W), alpha (H, W), radii, z_max of the visible Gaussians)."""
    leaves = {}
    for k, v in inputs.items():
        if k in rt.NAMES and v is not None:
            leaves[k] = v.detach().to(torch.float64).clone().requires_grad_(True)
    P = inputs["means3D"].shape[0]
    dev = inputs["means3D"].device
    leaves["means2D"] = torch.zeros((P, 3), dtype=torch.float64, device=dev, requires_grad=True)
    other = {k: v for k, v in inputs.items() if k not in rt.NAMES}
    pre = rt.preprocess(cam, **leaves, **other)
    W, H = pre["W"], pre["H"]

    def flat(g, n):
        return None if g is None else g.detach().to(torch.float64).reshape(n, H * W)
    gc, gd, ga = flat(g_color, 3), flat(g_depth, 1), flat(g_alpha, 1)
    img = torch.empty((3, H * W), dtype=torch.float64, device=dev)
    depth = torch.empty(H * W, dtype=torch.float64, device=dev)
    alpha = torch.empty(H * W, dtype=torch.float64, device=dev)
    tensors = list(leaves.values())
    acc = [torch.zeros_like(t) for t in tensors]
    for s in range(0, H * W, chunk):
        pix = torch.arange(s, min(s + chunk, H * W), device=dev)
        c = rt.composite(pre, bg, pix)
        d, a = composite_aux(cam, pre, leaves["means3D"], pix)
        img[:, pix], depth[pix], alpha[pix] = c.detach(), d.detach(), a.detach()
        loss = 0.0 * c.sum()
        if gc is not None:
            loss = loss + (c * gc[:, pix]).sum()
        if gd is not None:
            loss = loss + (d * gd[0, pix]).sum()
        if ga is not None:
            loss = loss + (a * ga[0, pix]).sum()
        gs = torch.autograd.grad(loss, tensors, retain_graph=True, allow_unused=True)
        for t, g in zip(acc, gs):
            if g is not None:
                t += g
    out = {k: None for k in rt.NAMES}
    for k, t in zip(leaves, acc):
        out[k] = t
    with torch.no_grad():
        zv = view_z(cam, leaves["means3D"])[pre["order"]]
        z_max = zv.max().item() if zv.numel() else 0.0
    return out, img.reshape(3, H, W), depth.reshape(H, W), alpha.reshape(H, W), pre["radii"], z_max
