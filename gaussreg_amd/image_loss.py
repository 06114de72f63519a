"""Photometric loss of Gaussian-splatting training on the fused HIP kernels of csrc/image_loss.hip.

    loss = photometric_loss(image, target, lambda_dssim=0.2, weight=None)   # (1 - l) L1 + l (1 - SSIM), mean over views
    s = ssim(img1, img2)                                                   # the mean SSIM alone

Images are (V, C, H, W) or (C, H, W) fp32 with C in {1, 3}; `weight` is an optional (V, H, W) or (H, W) map of per-pixel
weights >= 0 (for example a rendered alpha map, detached) that scales the SSIM map and the L1 term -- the 11 x 11 windows
still read every pixel.  The gradient goes to the first image only; target and weight are constants.  INTEGRATION.md has
the definition.  There is no CPU fallback.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _prepare(image, target, weight):
    for name, t in (("image", image), ("target", target)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
    if target.requires_grad or (weight is not None and weight.requires_grad):
        raise ValueError("the image loss is differentiated with respect to `image` only: detach target and weight")
    if not (image.is_cuda and target.is_cuda and (weight is None or weight.is_cuda)):
        raise _lib.HipLibraryError("gaussreg_amd.image_loss needs tensors on an MI355X; there is no CPU fallback")
    if image.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError("image and target must be float32")
    if image.shape != target.shape or image.dim() not in (3, 4):
        raise ValueError(f"image {tuple(image.shape)} and target {tuple(target.shape)} must both be (V, C, H, W) or (C, H, W)")
    if image.dim() == 3:
        image, target = image[None], target[None]
        if weight is not None and weight.dim() == 2:
            weight = weight[None]
    V, C, H, W = image.shape
    if C not in (1, 3) or V < 1 or H < 1 or W < 1:
        raise ValueError(f"image shape {tuple(image.shape)}: C must be 1 or 3 and no dimension empty")
    if weight is not None:
        if weight.dtype != torch.float32 or tuple(weight.shape) != (V, H, W) or weight.device != image.device:
            raise ValueError(f"weight must be float32 of shape {(V, H, W)} on the image's device")
        weight = weight.contiguous()
    if target.device != image.device:
        raise ValueError("image and target are on different devices")
    return image, target.contiguous(), weight


class _ImageLoss(torch.autograd.Function):
    """(loss_v or ssim_mean_v) per view; backward through gr_image_loss_backward."""

    @staticmethod
    def forward(ctx, image, target, weight, lambda_dssim, want_ssim):
        L = _lib.lib()
        x = image.detach().contiguous()
        V, C, H, W = x.shape
        dev = x.device
        need_grad = ctx.needs_input_grad[0]
        loss = torch.empty(V, dtype=torch.float32, device=dev)
        terms = torch.empty(V, 3, dtype=torch.float32, device=dev)
        keep_bytes = int(L.gr_image_loss_keep_bytes(V, C, H, W)) if need_grad else 0
        keep = torch.empty(keep_bytes // 4, dtype=torch.float32, device=dev) if need_grad else None
        ws_bytes = int(L.gr_image_loss_workspace_bytes(V, C, H, W))
        if ws_bytes == 0:
            raise ValueError(f"image loss: unsupported shape {(V, C, H, W)} (V * C <= 65535)")
        _lib.call(dev, "gr_image_loss_forward", x, target, weight, V, C, H, W, ctypes.c_float(lambda_dssim), loss, terms, keep,
                  keep_bytes, ws=ws_bytes)
        ctx.lambda_dssim = lambda_dssim
        ctx.want_ssim = want_ssim
        ctx.has_weight = weight is not None
        if need_grad:
            ctx.save_for_backward(x, target, terms, keep, *([weight] if weight is not None else []))
        ctx.mark_non_differentiable(terms)
        out = terms[:, 1].clone() if want_ssim else loss
        return out, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_terms):
        x, target, terms, keep = ctx.saved_tensors[:4]
        weight = ctx.saved_tensors[4] if ctx.has_weight else None
        V, C, H, W = x.shape
        dev = x.device
        # loss_v = (1 - lambda) l1 + lambda (1 - ssim_mean): at lambda = 1, d ssim_mean = -d loss_v
        g = (-grad_out if ctx.want_ssim else grad_out).to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        _lib.call(dev, "gr_image_loss_backward", x, target, weight, V, C, H, W, ctypes.c_float(ctx.lambda_dssim), keep,
                  keep.numel() * 4, terms, g, dx, None, 0)  # (no workspace: NULL, 0)
        return dx, None, None, None, None


def _reduce(per_view, reduction):
    if reduction == "mean":
        return per_view.mean()
    if reduction == "none":
        return per_view
    raise ValueError(f"reduction must be 'mean' or 'none', not {reduction!r}")


def photometric_loss_terms(image, target, lambda_dssim=0.2, weight=None):
    """(loss (V,), terms (V, 3) = l1, ssim_mean, S per view); the terms carry no gradient."""
    lam = float(lambda_dssim)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_dssim {lam} outside [0, 1]")
    image4, target4, weight3 = _prepare(image, target, weight)
    return _ImageLoss.apply(image4, target4, weight3, lam, False)


def photometric_loss(image, target, lambda_dssim=0.2, weight=None, reduction="mean"):
    """(1 - lambda_dssim) * L1 + lambda_dssim * (1 - SSIM) per view; 'mean' over the views or 'none' -> (V,)."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be 'mean' or 'none', not {reduction!r}")
    return _reduce(photometric_loss_terms(image, target, lambda_dssim, weight)[0], reduction)


def ssim(img1, img2, weight=None, reduction="mean"):
    """Mean SSIM per view (weighted by `weight`), with the gradient to img1."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be 'mean' or 'none', not {reduction!r}")
    image4, target4, weight3 = _prepare(img1, img2, weight)
    return _reduce(_ImageLoss.apply(image4, target4, weight3, 1.0, True)[0], reduction)
