"""CPU: the float64 torch restatement of the rasterizer (tests/raster_torch64.py), which the GPU backward tests take their
reference gradients from, is pinned here first: its image agrees with the independent NumPy renderer
(oracle/rasterizer_np64.py), and its autograd passes torch.autograd.gradcheck on a tiny scene."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import raster_torch64 as rt  # noqa: E402
from gaussreg_amd import synthetic  # noqa: E402
from oracle import rasterizer_np64  # noqa: E402


def _scene(P, W, H, seed, deg):
    g = synthetic.gaussians_c2(P, seed, sh_degree=max(deg, 0))
    cam = synthetic.camera(W, H)
    return g, cam


@pytest.mark.parametrize("mode", ["sh3_sr", "sh0_cov", "precomp_sr"])
def test_image_matches_np64(mode):
    W, H, P = 72, 56, 3000
    deg = 3 if mode == "sh3_sr" else 0
    g, cam = _scene(P, W, H, 7, deg)
    bg = np.array([0.2, 0.4, 0.6])
    kw = {}
    if mode == "precomp_sr":
        kw["colors_precomp"] = np.random.default_rng(1).random((P, 3)).astype(np.float32)
    else:
        kw["shs"] = g["shs"]
    if mode == "sh0_cov":
        q = g["rotations"].astype(np.float64)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
                      np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
                      np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
        M = R * g["scales"].astype(np.float64)[:, None, :]
        S = M @ np.transpose(M, (0, 2, 1))
        kw["cov3D_precomp"] = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
    else:
        kw["scales"], kw["rotations"] = g["scales"], g["rotations"]
    ref, rradii, _ = rasterizer_np64.render(g["means3D"], g["opacities"], viewmatrix=cam["viewmatrix"],
                                            projmatrix=cam["projmatrix"], campos=cam["campos"], bg=bg, W=W, H=H,
                                            tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], sh_degree=deg, **kw)
    t = {k: torch.from_numpy(np.asarray(v)).double() for k, v in kw.items()}
    img, radii = rt.render(rt.camera_dict(cam, W, H), bg, means3D=torch.from_numpy(g["means3D"]).double(),
                           opacities=torch.from_numpy(g["opacities"]).double(), sh_degree=deg, **t)
    img = img.detach().numpy()
    assert np.array_equal(radii.numpy(), rradii)
    diff = np.abs(img - ref).max(0)
    # documented threshold flips (alpha = 1/255, T = 1e-4 decided in another rounding order): isolated pixels only
    assert (diff > 1e-9).mean() <= 0.005, (diff > 1e-9).mean()
    assert np.median(diff) <= 1e-12


def test_gradcheck_tiny_scene():
    W, H = 20, 18
    rng = np.random.default_rng(3)
    P = 5
    cam = synthetic.camera(W, H)
    means = np.stack([rng.uniform(-0.3, 0.3, P), rng.uniform(-0.25, 0.25, P), rng.uniform(2.0, 3.0, P)], 1)
    f8 = torch.float64
    m = torch.tensor(means, dtype=f8, requires_grad=True)
    op = torch.tensor(rng.uniform(0.3, 0.6, (P, 1)), dtype=f8, requires_grad=True)
    sc = torch.tensor(rng.uniform(0.05, 0.09, (P, 3)), dtype=f8, requires_grad=True)
    q = rng.normal(size=(P, 4))
    rot = torch.tensor(q / np.linalg.norm(q, axis=1, keepdims=True), dtype=f8, requires_grad=True)
    sh = torch.tensor(rng.normal(0.5, 0.2, (P, 4, 3)), dtype=f8, requires_grad=True)
    m2 = torch.zeros((P, 3), dtype=f8, requires_grad=True)
    camd = rt.camera_dict(cam, W, H)
    bg = [0.1, 0.2, 0.3]
    img, _ = rt.render(camd, bg, means3D=m, opacities=op, shs=sh, scales=sc, rotations=rot, means2D=m2, sh_degree=1,
                       scale_modifier=0.9)
    # the scene stays away from the alpha = 1/255 and saturation thresholds on every pixel it touches: the
    # gradient is smooth there and finite differences see the same decisions
    assert img.min() > 0.0

    def f(m, op, sh, sc, rot, m2):
        return rt.render(camd, bg, means3D=m, opacities=op, shs=sh, scales=sc, rotations=rot, means2D=m2, sh_degree=1,
                         scale_modifier=0.9)[0]
    assert torch.autograd.gradcheck(f, (m, op, sh, sc, rot, m2), eps=1e-7, atol=1e-5, rtol=1e-4)


def test_grads_chunked_equals_whole():
    W, H, P = 40, 36, 300
    g, cam = _scene(P, W, H, 2, 3)
    t = {k: torch.from_numpy(g[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    go = torch.from_numpy(np.random.default_rng(0).normal(size=(3, H, W)))
    camd = rt.camera_dict(cam, W, H)
    a, ia, _ = rt.grads(camd, [0.3, 0.3, 0.3], go, chunk=97, sh_degree=3, **t)
    b, ib, _ = rt.grads(camd, [0.3, 0.3, 0.3], go, chunk=W * H, sh_degree=3, **t)
    assert torch.equal(ia, ib)
    for k in a:
        if a[k] is not None:
            assert torch.allclose(a[k], b[k], rtol=1e-10, atol=1e-13), k
