"""CPU pins of tests/image_loss_f64.py, the float64 restatement tests/test_gpu_image_loss.py compares
gaussreg_amd.image_loss against: a direct 121-tap numpy loop, torch's gradcheck, the conv2d composition, and the algebraic
properties of SSIM.  Also: the window table compiled into csrc/image_loss.hip is the one the restatement uses."""
import os
import re

import numpy as np
import pytest
import torch

import image_loss_f64 as R
from gaussreg_amd import image_loss  # noqa: F401  (the module these pins exist for)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _pair(C, H, W, seed, V=None):
    g = torch.Generator().manual_seed(seed)
    shape = (C, H, W) if V is None else (V, C, H, W)
    return torch.rand(shape, generator=g, dtype=torch.float64), torch.rand(shape, generator=g, dtype=torch.float64)


def _weight(V, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((V, H, W), generator=g, dtype=torch.float64)


def test_window_is_normalised_and_symmetric():
    g = R.window()
    assert g.dtype == np.float32 and g.shape == (11,)
    assert np.array_equal(g, g[::-1])
    assert abs(g.astype(np.float64).sum() - 1.0) < 1e-7


def test_kernel_window_table_is_the_reference_window():
    src = open(os.path.join(ROOT, "gaussreg_amd", "csrc", "image_loss.hip")).read()
    body = src[src.index("IMAGE_LOSS_WINDOW_BEGIN"):src.index("IMAGE_LOSS_WINDOW_END")]
    taps = np.array([np.float32(t) for t in re.findall(r"(\d\.\d+e-\d+)f", body)], np.float32)
    assert np.array_equal(taps.view(np.uint32), R.window().view(np.uint32))


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (11, 11), (23, 17)])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("weighted", [False, True])
def test_against_direct_numpy_loop(H, W, C, weighted):
    x, y = _pair(C, H, W, 10 * H + W + C)
    w = _weight(1, H, W, 5)[0] if weighted else None
    loss, terms = R.loss_terms(x, y, w, 0.2)
    want = R.numpy_direct(x.numpy(), y.numpy(), None if w is None else w.numpy(), 0.2)
    got = (loss[0].item(), terms[0, 0].item(), terms[0, 1].item(), terms[0, 2].item())
    assert np.allclose(got, want, rtol=0, atol=1e-13), (got, want)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("weighted", [False, True])
def test_gradcheck_and_analytic_backward(C, weighted):
    V, H, W = 2, 9, 13
    x, y = _pair(C, H, W, 40 + C, V=V)
    w = _weight(V, H, W, 6) if weighted else None
    dL = torch.tensor([0.7, -1.3], dtype=torch.float64)
    x.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: R.loss_terms(t, y, w, 0.2)[0], (x,), eps=1e-6, atol=1e-7, rtol=1e-6)
    (auto,) = torch.autograd.grad((R.loss_terms(x, y, w, 0.2)[0] * dL).sum(), x)
    hand = R.backward(x.detach(), y, w, 0.2, dL)
    assert (auto - hand).abs().max().item() <= 1e-13 * max(1.0, auto.abs().max().item())


def test_backward_sign_of_zero_and_empty_weight():
    x, y = _pair(3, 6, 8, 3, V=2)
    x[0, :, 2, 3] = y[0, :, 2, 3]
    g = R.backward(x, y, None, 0.0)  # lambda = 0: L1 alone
    assert torch.all(g[0, :, 2, 3] == 0) and torch.all(g[0, :, 0, 0] != 0)
    w = torch.ones(2, 6, 8, dtype=torch.float64)
    w[1] = 0
    loss, terms = R.loss_terms(x, y, w, 0.2)
    assert loss[1].item() == 0.0 and torch.all(terms[1] == 0)
    assert torch.all(R.backward(x, y, w, 0.2)[1] == 0)


def test_ssim_of_an_image_with_itself_is_one():
    x, _ = _pair(3, 17, 19, 7, V=2)
    assert torch.all(R.ssim_map(x, x) == 1.0)
    loss, terms = R.loss_terms(x, x, None, 0.2)
    assert torch.all(loss.abs() <= 1e-15) and torch.all((terms[:, 1] - 1).abs() <= 1e-15)


def test_ssim_is_symmetric():
    x, y = _pair(3, 17, 19, 8, V=2)
    assert (R.ssim_map(x, y) - R.ssim_map(y, x)).abs().max().item() <= 1e-15
    a, b = R.loss_terms(x, y, None, 0.2)[0], R.loss_terms(y, x, None, 0.2)[0]
    assert (a - b).abs().max().item() <= 1e-15


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("weighted", [False, True])
def test_equals_conv2d_composition(C, weighted):
    V, H, W = 2, 21, 30
    x, y = _pair(C, H, W, 60 + C, V=V)
    w = _weight(V, H, W, 9) if weighted else None
    a, ta = R.loss_terms(x, y, w, 0.2)
    b, tb = R.conv_loss(x, y, w, 0.2)
    assert (a - b).abs().max().item() <= 1e-12
    assert ((ta - tb).abs() / tb.abs().clamp(min=1)).max().item() <= 1e-12
    x.requires_grad_(True)
    (gb,) = torch.autograd.grad(R.conv_loss(x, y, w, 0.2)[0].sum(), x)
    assert (gb - R.backward(x.detach(), y, w, 0.2)).abs().max().item() <= 1e-12


def test_module_refuses_cpu_tensors_and_target_grad():
    x, y = torch.rand(3, 8, 8), torch.rand(3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_loss.photometric_loss(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_loss.ssim(x, y)
    with pytest.raises(ValueError):
        image_loss.photometric_loss(x, y.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        image_loss.photometric_loss(x, y, weight=torch.ones(8, 8, requires_grad=True))
