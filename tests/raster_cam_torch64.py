"""Test helper (not collected): float64 reference gradients with respect to the camera tensors.

raster_torch64.preprocess and raster_aux_torch64.view_z read `viewmatrix`, `projmatrix` and `campos` of the camera dict
through torch.as_tensor, which keeps the autograd graph.  This module only puts float64 leaves into the dict and
accumulates their gradients over chunks of pixels; the renderer itself is the one of those two modules."""
import torch

import raster_aux_torch64 as ra
import raster_torch64 as rt

CAM_NAMES = ("viewmatrix", "projmatrix", "campos")


def with_leaves(cam, dev):
    """-> (camera dict whose three camera entries are float64 leaves on `dev`, in the logical layout of the originals,
    dict name -> leaf)."""
    d = dict(cam)
    leaves = {}
    for k in CAM_NAMES:
        leaves[k] = torch.as_tensor(cam[k]).detach().to(device=dev, dtype=torch.float64).clone().requires_grad_(True)
        d[k] = leaves[k]
    return d, leaves


def loss_terms(cam, pre, means3D, bg, pix, gc, gd, ga):
    """sum(color gc) + sum(depth gd) + sum(alpha ga) over the pixels `pix` (gc (3, HW), gd / ga (HW,), each may be None)."""
    loss = 0.0
    if gc is not None:
        loss = loss + (rt.composite(pre, bg, pix) * gc[:, pix]).sum()
    if gd is not None or ga is not None:
        d, a = ra.composite_aux(cam, pre, means3D, pix)
        if gd is not None:
            loss = loss + (d * gd[pix]).sum()
        if ga is not None:
            loss = loss + (a * ga[pix]).sum()
    return loss


def loss_value(cam, bg, g_color=None, g_depth=None, g_alpha=None, chunk=4096, **inputs):
    """The scalar loss for a plain camera dict (no graph): what central differences evaluate."""
    with torch.no_grad():
        pre = rt.preprocess(cam, **inputs)
        W, H = pre["W"], pre["H"]
        dev = inputs["means3D"].device
        gc, gd, ga = _flat(g_color, 3, H * W), _flat(g_depth, 0, H * W), _flat(g_alpha, 0, H * W)
        total = 0.0
        for s in range(0, H * W, chunk):
            pix = torch.arange(s, min(s + chunk, H * W), device=dev)
            total = total + float(loss_terms(cam, pre, inputs["means3D"], bg, pix, gc, gd, ga))
        return total


def _flat(g, n, hw):
    if g is None:
        return None
    g = g.detach().to(torch.float64)
    return g.reshape(n, hw) if n else g.reshape(hw)


def grads(cam, bg, g_color=None, g_depth=None, g_alpha=None, chunk=4096, pixels=None, **inputs):
    """Reference gradients of sum(color g_color) + sum(depth g_depth) + sum(alpha g_alpha) with respect to the camera:
    dict name -> float64 tensor in the shape of cam[name].  `pixels` (flat indices): composite only these (the g_* must be
    zero elsewhere)."""
    dev = inputs["means3D"].device
    camd, leaves = with_leaves(cam, dev)
    pre = rt.preprocess(camd, **inputs)
    W, H = pre["W"], pre["H"]
    gc, gd, ga = _flat(g_color, 3, H * W), _flat(g_depth, 0, H * W), _flat(g_alpha, 0, H * W)
    tensors = list(leaves.values())
    acc = [torch.zeros_like(t) for t in tensors]
    allpix = torch.arange(H * W, device=dev) if pixels is None else torch.as_tensor(pixels, device=dev).reshape(-1)
    for s in range(0, allpix.numel(), chunk):
        pix = allpix[s:s + chunk]
        loss = loss_terms(camd, pre, inputs["means3D"], bg, pix, gc, gd, ga)
        if not (isinstance(loss, torch.Tensor) and loss.requires_grad):
            continue
        gs = torch.autograd.grad(loss, tensors, retain_graph=True, allow_unused=True)
        for a, g in zip(acc, gs):
            if g is not None:
                a += g
    return dict(zip(leaves, acc))
