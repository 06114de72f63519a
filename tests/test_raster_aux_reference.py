"""CPU: known answers that pin tests/raster_aux_torch64.py, the float64 reference of the depth and alpha maps the GPU tests
(tests/test_gpu_rasterizer_depth.py) compare against.

This file tests the reference, not the feature: it touches no kernel and no rasterizer keyword, so it passes on any tree that
holds the helper.  The tests that need the feature are tests/test_gpu_rasterizer_depth.py and
tests/test_raster_aux_resources.py."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import raster_aux_torch64 as ra  # noqa: E402
import raster_torch64 as rt  # noqa: E402
from gaussreg_amd import synthetic  # noqa: E402

W, H = 33, 33  # the optical axis meets pixel (16, 16) exactly


def on_axis(zs, ops, scale=0.05):
    n = len(zs)
    return dict(means3D=torch.tensor([[0.0, 0.0, z] for z in zs], dtype=torch.float64),
                opacities=torch.tensor(ops, dtype=torch.float64).reshape(n, 1),
                colors_precomp=torch.ones((n, 3), dtype=torch.float64),
                scales=torch.full((n, 3), scale, dtype=torch.float64),
                rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]] * n, dtype=torch.float64))


def cam():
    return rt.camera_dict(synthetic.camera(W, H), W, H)


def test_one_gaussian_on_the_axis():
    for op, z0 in ((0.6, 2.0), (1.0, 3.5)):  # opacity 1 meets the 0.99 clamp
        _, depth, alpha, radii = ra.render(cam(), [0.0, 0.0, 0.0], **on_axis([z0], [op]))
        assert int(radii[0]) > 0
        a = min(op, 0.99)
        assert abs(alpha[16, 16].item() - a) <= 1e-12
        assert abs(depth[16, 16].item() - a * z0) <= 1e-12
        assert alpha[0, 0].item() == 0.0 and depth[0, 0].item() == 0.0  # out of reach: nothing blended


def test_two_gaussians_front_to_back():
    z1, z2, o1, o2 = 3.0, 1.5, 0.5, 0.7  # given back to front: the order comes from the depth
    _, depth, alpha, _ = ra.render(cam(), [0.0, 0.0, 0.0], **on_axis([z1, z2], [o1, o2]))
    assert abs(alpha[16, 16].item() - (o2 + (1 - o2) * o1)) <= 1e-12
    assert abs(depth[16, 16].item() - (o2 * z2 + (1 - o2) * o1 * z1)) <= 1e-12


def test_alpha_is_one_minus_transmittance_of_the_colour_composite():
    g = synthetic.gaussians_c2(400, 3)
    t = {k: torch.from_numpy(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    t["colors_precomp"] = torch.ones((400, 3))
    c = rt.camera_dict(synthetic.camera(64, 48), 64, 48)
    img, depth, alpha, _ = ra.render(c, [0.0, 0.0, 0.0], **t)  # white on black: every channel is sum w_i = 1 - T
    assert (img[0] - alpha).abs().max().item() <= 1e-12
    assert alpha.max().item() > 0.5 and (alpha == 0).any()
    assert (depth >= 0).all() and depth.max().item() > 0.2


def test_depth_gradient_reaches_means_through_the_view_row():
    c = cam()
    t = on_axis([2.0], [0.6])
    g_d = torch.zeros((H, W), dtype=torch.float64)
    g_d[16, 16] = 1.0
    g, _, depth, _, _, z_max = ra.grads(c, [0.0, 0.0, 0.0], None, g_d, None, **t)
    assert abs(z_max - 2.0) <= 1e-12
    # at the centre pixel the Gaussian's footprint is stationary: d depth / d z = alpha (+ 0 from the shape)
    eps = 1e-6
    t2 = on_axis([2.0 + eps], [0.6])
    _, d2, _, _ = ra.render(c, [0.0, 0.0, 0.0], **t2)
    fd = (d2[16, 16].item() - depth[16, 16].item()) / eps
    assert abs(g["means3D"][0, 2].item() - fd) <= 1e-5 * abs(fd)
    assert abs(g["opacities"][0, 0].item() - 2.0) <= 1e-9  # d(op z0)/d op
    assert math.isfinite(g["scales"].abs().sum().item())


def test_view_z_with_a_rotated_and_translated_camera():
    # Camera at C = (1, 2, -1) looking along world +x: its axes in world coordinates are x = (0, 0, -1), y = (0, 1, 0),
    # z = (1, 0, 0) (the columns of R_c2w).  View-space depth by hand: z = (p - C) . (1, 0, 0) = p_x - 1.
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    c = rt.camera_dict(synthetic.camera(W, H, R_c2w=R, C=np.array([1.0, 2.0, -1.0])), W, H)
    pts = torch.tensor([[4.0, 2.0, -1.0], [4.0, 2.5, -1.5], [5.5, -3.0, 7.0], [0.0, 2.0, -1.0]], dtype=torch.float64)
    assert torch.allclose(ra.view_z(c, pts), torch.tensor([3.0, 3.0, 4.5, -1.0], dtype=torch.float64), rtol=0, atol=1e-12)
    # a row / column or translation mix-up of the view matrix would give p_z + 1 = 0 or p_x + 1 = 5 for the first point
    t = on_axis([0.0], [0.6])
    t["means3D"] = pts[:1].clone()  # on the optical axis of this camera, 3 in front of it
    _, depth, alpha, radii = ra.render(c, [0.0, 0.0, 0.0], **t)
    assert int(radii[0]) > 0
    assert abs(alpha[16, 16].item() - 0.6) <= 1e-12 and abs(depth[16, 16].item() - 0.6 * 3.0) <= 1e-12
    g_d = torch.zeros((H, W), dtype=torch.float64)
    g_d[16, 16] = 1.0
    g = ra.grads(c, [0.0, 0.0, 0.0], None, g_d, None, **t)[0]["means3D"][0]
    # moving the Gaussian along the viewing direction (world x) changes its depth one for one: d depth / d p_x = alpha there
    # plus the footprint's change, which a finite difference takes along
    eps = 1e-6
    t2 = dict(t, means3D=pts[:1] + torch.tensor([[eps, 0.0, 0.0]], dtype=torch.float64))
    fd = (ra.render(c, [0.0, 0.0, 0.0], **t2)[1][16, 16].item() - depth[16, 16].item()) / eps
    assert abs(g[0].item() - fd) <= 1e-5 * abs(fd) and abs(fd) > 0.3
