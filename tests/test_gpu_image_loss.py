"""GPU: gaussreg_amd.image_loss (csrc/image_loss.hip) against the float64 restatement tests/image_loss_f64.py.

Bound.  For every case e_hip = |library - float64| and e_t32 = |stock-torch fp32 composition - float64| (five grouped
conv2d with the 2-D window plus autograd, same device): absolute for the per-view loss and the terms, ||d||_2 / ||f64||_2
for dL/dimage.  Asserted: e_hip <= 4 e_t32 + floor, floor = 8 fp32 epsilons of the quantity's scale.  The scale of loss,
l1 and ssim_mean is max(1, |value|): each is an average of per-pixel quantities of order one (SSIM itself is formed as a
ratio of terms near 1 before `1 - ssim` cancels it), so its rounding error does not shrink with the value; the scale of S
is S; the gradient error is already relative (scale 1).  Every figure is printed before it is asserted
(docs/image_loss_f64_errors.md has the recorded table).
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_loss_f64 as R
from gaussreg_amd import _lib, image_loss

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 2.0 ** -23
FACTOR = 4.0
TILE_H, TILE_W = 16, 32  # csrc/image_loss.hip
SIZES = [(1, 1), (5, 7), (11, 11), (37, 53), (240, 320), (480, 640), (3 * TILE_H, 3 * TILE_W),
         (3 * TILE_H + 1, 3 * TILE_W + 1)]


def bits(t):
    return t.contiguous().view(torch.int32)


def uniform(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(shape, generator=g, device="cuda") * (hi - lo) + lo


def hip_eval(x, y, w, lam, dL):
    x = x.clone().requires_grad_(True)
    loss, terms = image_loss.photometric_loss_terms(x, y, lam, w)
    (loss * dL).sum().backward()
    return loss.detach(), terms.detach(), x.grad


def t32_eval(x, y, w, lam, dL):
    x = x.clone().requires_grad_(True)
    loss, terms = R.conv_loss(x, y, w, lam)
    (loss * dL).sum().backward()
    return loss.detach(), terms.detach(), x.grad


def f64_eval(x, y, w, lam, dL):
    xd, yd = x.double(), y.double()
    wd = None if w is None else w.double()
    loss, terms = R.loss_terms(xd, yd, wd, lam)
    return loss, terms, R.backward(xd, yd, wd, lam, dL.double())


def check_case(name, x, y, w=None, lam=0.2, seed=0):
    """Print, then assert, e_hip <= 4 e_t32 + floor for loss, the three terms and the gradient."""
    V = x.shape[0]
    dL = uniform((V,), 900 + seed, 0.5, 1.5)
    ref = f64_eval(x, y, w, lam, dL)
    hip = hip_eval(x, y, w, lam, dL)
    t32 = t32_eval(x, y, w, lam, dL)
    rows = []

    def absolute(a, r):
        return (a.double() - r).abs().max().item()

    for label, r, h, t, scale in (
            ("loss", ref[0], hip[0], t32[0], ref[0].abs().clamp(min=1).max().item()),
            ("l1", ref[1][:, 0], hip[1][:, 0], t32[1][:, 0], ref[1][:, 0].abs().clamp(min=1).max().item()),
            ("ssim_mean", ref[1][:, 1], hip[1][:, 1], t32[1][:, 1], ref[1][:, 1].abs().clamp(min=1).max().item()),
            ("S", ref[1][:, 2], hip[1][:, 2], t32[1][:, 2], ref[1][:, 2].abs().max().item())):
        rows.append((label, absolute(h, r), absolute(t, r), 8 * EPS * scale))
    gn = ref[2].norm().item()
    if gn > 0:
        rows.append(("grad", (hip[2].double() - ref[2]).norm().item() / gn, (t32[2].double() - ref[2]).norm().item() / gn,
                     8 * EPS))
    else:
        assert torch.count_nonzero(hip[2]) == 0
    for label, e_hip, e_t32, floor in rows:
        print(f"IMAGE_LOSS_ERR {name} {label} e_hip={e_hip:.3e} e_t32={e_t32:.3e} floor={floor:.3e} "
              f"ratio={e_hip / max(e_t32, 1e-300):.3g}")
    for label, e_hip, e_t32, floor in rows:
        assert e_hip <= FACTOR * e_t32 + floor, (name, label, e_hip, e_t32, floor)
    return hip


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("V", [1, 4, 32])
def test_uniform_images(V, C, H, W):
    x = uniform((V, C, H, W), 1)
    y = uniform((V, C, H, W), 2)
    check_case(f"uniform[{V}x{C}x{H}x{W}]", x, y)


@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
def test_lambda_values(lam):
    x, y = uniform((4, 3, 37, 53), 3), uniform((4, 3, 37, 53), 4)
    check_case(f"lambda[{lam}]", x, y, lam=lam)


def test_close_images():
    y = uniform((4, 3, 240, 320), 5)
    x = (y + 0.02 * (uniform((4, 3, 240, 320), 6) - 0.5)).clamp(0, 1)
    check_case("close", x, y)


@pytest.mark.parametrize("a,b", [(0.3, 0.7), (0.5, 0.5), (0.0, 1.0)])
def test_constant_images(a, b):
    x = torch.full((4, 3, 37, 53), a, device="cuda")
    y = torch.full((4, 3, 37, 53), b, device="cuda")
    check_case(f"constant[{a},{b}]", x, y)


@pytest.mark.parametrize("C", [1, 3])
def test_values_outside_unit_interval(C):
    x, y = uniform((4, C, 240, 320), 7, -2.0, 3.0), uniform((4, C, 240, 320), 8, -2.0, 3.0)
    check_case(f"outside[{C}]", x, y)


# ---------------------------------------------------------------------------------------------- renders

def _scene(points=20000):
    from gaussreg_amd import synthetic
    g = synthetic.gaussians_c2(points, 0)
    return {k: torch.from_numpy(g[k]).cuda() for k in ("means3D", "opacities", "shs", "scales", "rotations")}


def _render(scene, V, W, H, shift=0.0, grad=False):
    """(color, alpha, camera leaves) of V ring cameras, each moved by `shift` along x."""
    from gaussreg_amd import synthetic
    from gaussreg_amd.rasterizer import GaussianRasterizationSettings, rasterize_views
    sets, leaves = [], []
    for c in synthetic.camera_ring(V, W, H, seed=3):
        vm = torch.from_numpy(np.ascontiguousarray(c["viewmatrix"]))
        pm = torch.from_numpy(np.ascontiguousarray(c["projmatrix"]))
        if shift:
            delta = torch.eye(4)
            delta[3, 0] = shift  # row-vector convention: the view-space translation sits in the last row
            full = torch.linalg.inv(vm.double()) @ pm.double()
            vm = vm @ delta
            pm = (vm.double() @ full).float()
        vm, pm = vm.cuda(), pm.cuda()
        vm.requires_grad_(grad)
        leaves.append(vm)
        sets.append(GaussianRasterizationSettings(H, W, c["tanfovx"], c["tanfovy"], torch.zeros(3, device="cuda"), 1.0, vm, pm,
                                                  3, torch.from_numpy(c["campos"]).cuda(), False, False))
    color, _, _, _, alpha = rasterize_views(sets, scene["means3D"], scene["opacities"], shs=scene["shs"],
                                            scales=scene["scales"], rotations=scene["rotations"], render_depth=True)
    return color, alpha, leaves


def test_render_against_perturbed_render():
    scene = _scene()
    with torch.no_grad():
        target, alpha, _ = _render(scene, 4, 320, 240)
        image, _, _ = _render(scene, 4, 320, 240, shift=0.01)
    assert (image - target).abs().max().item() > 1e-3
    check_case("render", image.contiguous(), target.contiguous())
    check_case("render+alpha", image.contiguous(), target.contiguous(), w=alpha[:, 0].contiguous())


# ---------------------------------------------------------------------------------------------- weight

def test_half_plane_weight():
    x, y = uniform((4, 3, 37, 53), 11), uniform((4, 3, 37, 53), 12)
    w = torch.zeros(4, 37, 53, device="cuda")
    w[:, :, :26] = 1.0
    _, _, grad = check_case("halfplane", x, y, w=w)
    # without the SSIM term a pixel of weight 0 receives nothing at all
    xg = x.clone().requires_grad_(True)
    image_loss.photometric_loss(xg, y, 0.0, weight=w).backward()
    assert torch.count_nonzero(xg.grad[:, :, :, 26:]) == 0
    assert torch.count_nonzero(xg.grad[:, :, :, :26]) == xg.grad[:, :, :, :26].numel()
    # with it, only pixels within the window's reach of a weighted pixel do
    assert torch.count_nonzero(grad[:, :, :, 26 + 5:]) == 0 and torch.count_nonzero(grad[:, :, :, 26:26 + 5]) > 0


def test_random_weight():
    x, y = uniform((4, 3, 240, 320), 13), uniform((4, 3, 240, 320), 14)
    check_case("weight", x, y, w=uniform((4, 240, 320), 15))


# ---------------------------------------------------------------------------------------------- exact statements

@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("V", [1, 4, 32])
def test_identical_images_give_exactly_zero(V, C, H, W):
    assert C * H * W < 2 ** 24
    x = uniform((V, C, H, W), 21, -0.5, 1.5)
    loss, terms = image_loss.photometric_loss_terms(x, x.clone(), 0.2)
    assert torch.all(bits(loss) == 0), loss
    assert torch.all(terms[:, 1] == 1.0) and torch.all(terms[:, 0] == 0.0) and torch.all(terms[:, 2] == H * W)
    assert image_loss.photometric_loss(x, x.clone()).item() == 0.0
    assert torch.all(image_loss.ssim(x, x.clone(), reduction="none") == 1.0)


def test_view_without_weight():
    x = uniform((3, 3, 37, 53), 22).requires_grad_(True)
    y = uniform((3, 3, 37, 53), 23)
    w = torch.ones(3, 37, 53, device="cuda")
    w[1] = 0.0
    loss = image_loss.photometric_loss(x, y, 0.2, weight=w, reduction="none")
    loss.sum().backward()
    assert bits(loss)[1].item() == 0 and loss[0].item() > 0 and loss[2].item() > 0
    assert torch.all(bits(x.grad[1]) == 0) and torch.count_nonzero(x.grad[0]) > 0


@pytest.mark.parametrize("C,H,W", [(3, 37, 53), (1, 240, 320), (3, 480, 640)])
def test_reproducible_batch_independent_and_ones_weight(C, H, W):
    V = 4
    x, y = uniform((V, C, H, W), 24), uniform((V, C, H, W), 25)
    dL = uniform((V,), 26, 0.5, 1.5)
    w = uniform((V, H, W), 27)
    for weight in (None, w):
        a = hip_eval(x, y, weight, 0.2, dL)
        b = hip_eval(x, y, weight, 0.2, dL)
        for p, q in zip(a, b):
            assert torch.equal(bits(p), bits(q))
        for v in range(V):
            one = hip_eval(x[v:v + 1], y[v:v + 1], None if weight is None else weight[v:v + 1], 0.2, dL[v:v + 1])
            assert torch.equal(bits(one[0]), bits(a[0][v:v + 1]))
            assert torch.equal(bits(one[1]), bits(a[1][v:v + 1]))
            assert torch.equal(bits(one[2]), bits(a[2][v:v + 1]))
        # a (C, H, W) input is the V = 1 call
        three = image_loss.photometric_loss(x[0], y[0], 0.2, weight=None if weight is None else weight[0], reduction="none")
        assert torch.equal(bits(three), bits(a[0][:1]))
    none = hip_eval(x, y, None, 0.2, dL)
    ones = hip_eval(x, y, torch.ones(V, H, W, device="cuda"), 0.2, dL)
    for p, q in zip(none, ones):
        assert torch.equal(bits(p), bits(q))


def test_ssim_entry_point():
    x, y = uniform((4, 3, 37, 53), 28), uniform((4, 3, 37, 53), 29)
    xg = x.clone().requires_grad_(True)
    s = image_loss.ssim(xg, y, reduction="none")
    _, terms = image_loss.photometric_loss_terms(x, y, 1.0)
    assert torch.equal(bits(s), bits(terms[:, 1]))
    s.sum().backward()
    ref = -R.backward(x.double(), y.double(), None, 1.0)
    xt = x.clone().requires_grad_(True)
    R.conv_loss(xt, y, None, 1.0)[1][:, 1].sum().backward()  # the fp32 composition's ssim_mean
    e_hip = ((xg.grad.double() - ref).norm() / ref.norm()).item()
    e_t32 = ((xt.grad.double() - ref).norm() / ref.norm()).item()
    print(f"IMAGE_LOSS_ERR ssim_entry grad e_hip={e_hip:.3e} e_t32={e_t32:.3e} floor={8 * EPS:.3e} ratio={e_hip / e_t32:.3g}")
    assert e_hip <= FACTOR * e_t32 + 8 * EPS
    assert image_loss.ssim(x, y).item() == pytest.approx(s.mean().item())


def test_argument_errors():
    x, y = uniform((2, 3, 8, 8), 30), uniform((2, 3, 8, 8), 31)
    with pytest.raises(ValueError):
        image_loss.photometric_loss(x, y.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        image_loss.photometric_loss(x, y, weight=torch.ones(2, 8, 8, device="cuda", requires_grad=True))
    with pytest.raises(ValueError):
        image_loss.photometric_loss(x, y, reduction="sum")
    with pytest.raises(ValueError):
        image_loss.photometric_loss(uniform((2, 2, 8, 8), 1), uniform((2, 2, 8, 8), 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_loss.photometric_loss(x.cpu(), y.cpu())
    assert image_loss.photometric_loss(x, y, reduction="none").shape == (2,)
    assert image_loss.photometric_loss(x, y).shape == ()


# ---------------------------------------------------------------------------------------------- C ABI

def test_forward_without_keep_buffer_has_the_same_bits():
    L = _lib.lib()
    V, C, H, W = 4, 3, 37, 53
    x, y = uniform((V, C, H, W), 32), uniform((V, C, H, W), 33)
    dev = x.device
    ws = torch.empty(int(L.gr_image_loss_workspace_bytes(V, C, H, W)), dtype=torch.uint8, device=dev)
    kb = int(L.gr_image_loss_keep_bytes(V, C, H, W))
    assert kb == 3 * 4 * V * C * H * W and ws.numel() > 0
    keep = torch.empty(kb, dtype=torch.uint8, device=dev)
    out = []
    for k, nbytes, terms in ((None, 0, None), (keep, kb, torch.empty(V, 3, device=dev))):
        loss = torch.empty(V, device=dev)
        _lib.check(L.gr_image_loss_forward(_lib.ptr(x), _lib.ptr(y), None, V, C, H, W, ctypes.c_float(0.2), _lib.ptr(loss),
                                           _lib.ptr(terms), _lib.ptr(k), nbytes, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        out.append(loss)
    assert torch.equal(bits(out[0]), bits(out[1]))
    assert torch.equal(bits(out[0]), bits(image_loss.photometric_loss(x, y, reduction="none")))
    # errors: negative code + message
    loss = torch.empty(V, device=dev)
    rc = L.gr_image_loss_forward(_lib.ptr(x), _lib.ptr(y), None, V, 2, H, W, ctypes.c_float(0.2), _lib.ptr(loss), None, None, 0,
                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    assert rc == -1 and b"C in {1, 3}" in L.gr_last_error()
    rc = L.gr_image_loss_forward(_lib.ptr(x), _lib.ptr(y), None, V, C, H, W, ctypes.c_float(0.2), _lib.ptr(loss), None, None, 0,
                                 _lib.ptr(ws), 16, _lib.stream_ptr(dev))
    assert rc == -3
    assert L.gr_image_loss_workspace_bytes(V, 2, H, W) == 0


# ---------------------------------------------------------------------------------------------- autograd chain

def test_chain_through_the_rasterizer():
    scene = _scene()
    with torch.no_grad():
        target, alpha, _ = _render(scene, 2, 160, 120)
    weight = alpha[:, 0].contiguous()

    color, _, leaves = _render(scene, 2, 160, 120, shift=0.01, grad=True)
    image_loss.photometric_loss(color, target, 0.2, weight=weight).backward()
    chained = [v.grad.clone() for v in leaves]
    assert all(g is not None and torch.count_nonzero(g) > 0 for g in chained)

    # by hand: this module's dL/dimage fed to the rasterizer's backward
    color2, _, leaves2 = _render(scene, 2, 160, 120, shift=0.01, grad=True)
    assert torch.equal(bits(color2), bits(color))
    leaf = color2.detach().clone().requires_grad_(True)
    image_loss.photometric_loss(leaf, target, 0.2, weight=weight).backward()
    color2.backward(leaf.grad)
    for a, b in zip(chained, leaves2):
        assert torch.equal(bits(a), bits(b.grad))


# ---------------------------------------------------------------------------------------------- example

def test_example_dssim_descends_and_is_deterministic():
    cmd = [sys.executable, os.path.join(ROOT, "examples", "refine_registration.py"), "--synthetic", "--loss", "dssim", "--steps",
           "20", "--points", "20000", "--width", "160", "--height", "120"]
    outs = []
    for _ in range(2):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(r.stdout)
    losses = {int(m.group(1)): float(m.group(2)) for m in re.finditer(r"step\s+(\d+)\s+loss\s+([0-9.eE+-]+)", outs[0])}
    assert 0 in losses and 19 in losses, outs[0]
    assert losses[19] < losses[0], losses
    assert outs[0] == outs[1]
