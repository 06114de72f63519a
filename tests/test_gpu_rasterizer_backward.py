"""GPU: autograd through the HIP rasterizer (gr_raster_render_keep + gr_raster_backward) against float64 reference
gradients (tests/raster_torch64.py, pinned by tests/test_raster_torch64_reference.py), plus the contract: the forward
under grad is bit-identical to the no-grad one, batched views sum in view order, backward is bitwise reproducible."""
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
from gaussreg_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, rasterize_views  # noqa: E402

pytestmark = pytest.mark.gpu
BG = [0.25, 0.5, 0.1]
MOD = 0.9
NAMES = ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")


def settings(cam, W, H, deg, bg=BG, mod=MOD):
    d = torch.device("cuda")
    return GaussianRasterizationSettings(H, W, cam["tanfovx"], cam["tanfovy"], torch.tensor(bg, device=d), mod,
                                         torch.from_numpy(cam["viewmatrix"]).to(d), torch.from_numpy(cam["projmatrix"]).to(d),
                                         deg, torch.from_numpy(cam["campos"]).to(d), False, False)


def cov_from(scales, rotations, mod):
    q = rotations.astype(np.float64)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    M = R * (scales.astype(np.float64) * mod)[:, None, :]
    S = M @ np.transpose(M, (0, 2, 1))
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


def scene(P, seed, mode, deg=3):
    g = synthetic.gaussians_c2(P, seed, sh_degree=max(deg, 0))
    t = {"means3D": g["means3D"], "opacities": g["opacities"]}
    if mode.startswith("precomp"):
        t["colors_precomp"] = np.random.default_rng(seed + 5).random((P, 3)).astype(np.float32)
    else:
        t["shs"] = g["shs"]
    if mode.endswith("cov"):
        t["cov3D_precomp"] = cov_from(g["scales"], g["rotations"], MOD)
    else:
        t["scales"], t["rotations"] = g["scales"], g["rotations"]
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in t.items()}


def gpu_grads(rs, t, gout, fast_exp=None, means2D=True):
    leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    m2 = torch.zeros_like(leaves["means3D"], requires_grad=True) if means2D else None
    img, radii = GaussianRasterizer(rs, fast_exp=fast_exp)(
        leaves["means3D"], m2, leaves["opacities"], shs=leaves.get("shs"), colors_precomp=leaves.get("colors_precomp"),
        scales=leaves.get("scales"), rotations=leaves.get("rotations"), cov3D_precomp=leaves.get("cov3D_precomp"))
    (img * gout).sum().backward()
    out = {k: v.grad for k, v in leaves.items()}
    out["means2D"] = m2.grad if means2D else None
    return out, img.detach(), radii


def ref_grads(cam, W, H, t, gout, deg, mod=MOD):
    kw = dict(t)
    mod_ref = mod
    if "cov3D_precomp" in kw:
        mod_ref = 1.0  # the precomputed covariance already holds the modifier
    g, img, radii = rt.grads(rt.camera_dict(cam, W, H), BG, gout, chunk=2048, sh_degree=deg, scale_modifier=mod_ref, **kw)
    return g, img, radii


def check_close(g, r, radii, name):
    g = g.double().reshape(g.shape[0], -1)
    r = r.reshape(r.shape[0], -1)
    rel = (torch.linalg.norm(g - r) / torch.linalg.norm(r).clamp_min(1e-30)).item()
    assert rel <= 1e-3, f"{name}: |g - g64| / |g64| = {rel:.3e}"
    vis = radii > 0
    if vis.any():
        rn = torch.linalg.norm(r, dim=1)
        err = torch.linalg.norm(g - r, dim=1)
        ok = err <= 1e-3 * rn + 1e-6 * rn.max()
        frac = ok[vis].double().mean().item()
        assert frac >= 0.99, f"{name}: only {frac:.4f} of visible Gaussians within bounds"


def compare_all(t, W, H, cam, deg, seed=0, fast_exp=None):
    rs = settings(cam, W, H, deg)
    gout = torch.from_numpy(np.random.default_rng(seed).normal(size=(3, H, W))).cuda().float()
    gg, img, radii = gpu_grads(rs, t, gout, fast_exp=fast_exp)
    rg, rimg, rradii = ref_grads(cam, W, H, t, gout.double(), deg)
    diff = (img.double() - rimg).abs().amax(0)
    assert (diff > 1e-4).double().mean().item() <= 1e-3  # isolated fp32 / fp64 threshold flips only
    for k in list(t) + ["means2D"]:
        check_close(gg[k], rg[k], rradii, k)
    return gg, rg


@pytest.mark.parametrize("mode,deg", [("sh_sr", 0), ("sh_sr", 3), ("sh_cov", 3), ("precomp_sr", 3), ("precomp_cov", 3)])
def test_gradients_match_float64_reference(mode, deg):
    W, H, P = 120, 88, 2500
    t = scene(P, 11, mode, deg)
    compare_all(t, W, H, synthetic.camera(W, H), deg)


def test_gradients_large_scene_odd_size():
    W, H, P = 262, 198, 10000  # not multiples of 16
    t = scene(P, 3, "sh_sr", 3)
    compare_all(t, W, H, synthetic.camera(W, H), 3, seed=1)


def test_gradients_fast_exp():
    W, H, P = 120, 88, 2500
    t = scene(P, 12, "sh_sr", 3)
    compare_all(t, W, H, synthetic.camera(W, H), 3, seed=2, fast_exp=True)


def test_wide_rectangles_marker_path():
    # 1040 px = 65 tiles: large Gaussians whose rectangles are wider than the 26-bit packing holds (RECT_MARKER26)
    W, H, P = 1040, 40, 60
    rng = np.random.default_rng(4)
    cam = synthetic.camera(W, H)
    means = np.stack([rng.uniform(-0.8, 0.8, P), rng.uniform(-0.02, 0.02, P), rng.uniform(1.5, 2.5, P)], 1)
    sc = np.stack([rng.uniform(0.2, 0.6, P), rng.uniform(0.005, 0.02, P), rng.uniform(0.005, 0.02, P)], 1)
    q = np.tile([1.0, 0.0, 0.0, 0.0], (P, 1)) + rng.normal(0, 0.05, (P, 4))
    t = {"means3D": means, "opacities": rng.uniform(0.05, 0.4, (P, 1)), "colors_precomp": rng.random((P, 3)),
         "scales": sc, "rotations": q}
    t = {k: torch.from_numpy(np.asarray(v, np.float32)).cuda() for k, v in t.items()}
    compare_all(t, W, H, cam, 0, seed=3)


def test_behind_near_plane_gets_zero():
    W, H, P = 96, 72, 1500
    t = scene(P, 5, "sh_sr", 3)
    t["means3D"][:200, 2] = torch.linspace(-1.0, 0.19, 200, device="cuda")  # z <= 0.2: culled
    gg, _ = compare_all(t, W, H, synthetic.camera(W, H), 3, seed=4)
    for k in gg:
        if gg[k] is not None:
            assert torch.count_nonzero(gg[k][:200]) == 0, k


def test_forward_under_grad_is_bit_identical_and_deterministic():
    W, H, P = 200, 150, 8000
    t = scene(P, 6, "sh_sr", 3)
    rs = settings(synthetic.camera(W, H), W, H, 3)
    with torch.no_grad():
        img0, r0 = GaussianRasterizer(rs)(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"],
                                          rotations=t["rotations"])
    gout = torch.from_numpy(np.random.default_rng(9).normal(size=(3, H, W))).cuda().float()
    a, img1, r1 = gpu_grads(rs, t, gout)
    b, img2, _ = gpu_grads(rs, t, gout)
    assert torch.equal(img0.view(torch.int32), img1.view(torch.int32)) and torch.equal(r0, r1)
    assert torch.equal(img1.view(torch.int32), img2.view(torch.int32))
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_multiview_is_sum_of_single_views():
    W, H, P, V = 128, 96, 4000, 4
    t = scene(P, 8, "sh_sr", 3)
    cams = synthetic.camera_ring(V, W, H, seed=2)
    sets = [settings(c, W, H, 3) for c in cams]
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=(V, 3, H, W))).cuda().float()
    leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    m2 = torch.zeros((V, P, 3), device="cuda", requires_grad=True)
    img, radii, _ = rasterize_views(sets, leaves["means3D"], leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
                                    rotations=leaves["rotations"], means2D=m2)
    (img * gout).sum().backward()
    with torch.no_grad():
        img0, _, _ = rasterize_views(sets, t["means3D"], t["opacities"], shs=t["shs"], scales=t["scales"],
                                     rotations=t["rotations"])
    assert torch.equal(img.detach().view(torch.int32), img0.view(torch.int32))
    acc = {k: torch.zeros_like(v) for k, v in t.items()}
    for v in range(V):
        g1, _, _ = gpu_grads(sets[v], t, gout[v])
        for k in acc:
            acc[k] += g1[k]
        assert torch.allclose(m2.grad[v], g1["means2D"], rtol=0, atol=1e-6 * g1["means2D"].abs().max().item() + 1e-30)
    for k in acc:
        scale = acc[k].abs().max().item()
        assert torch.allclose(leaves[k].grad, acc[k], rtol=0, atol=1e-6 * scale + 1e-30), k


def test_edge_cases():
    W, H = 64, 48
    cam = synthetic.camera(W, H)
    rs = settings(cam, W, H, 3)
    # P = 0
    e = {k: torch.zeros((0,) + s, device="cuda", requires_grad=True) for k, s in
         (("m", (3,)), ("o", (1,)), ("sh", (16, 3)), ("s", (3,)), ("r", (4,)))}
    img, radii = GaussianRasterizer(rs)(e["m"], None, e["o"], shs=e["sh"], scales=e["s"], rotations=e["r"])
    img.sum().backward()
    assert e["m"].grad.shape == (0, 3)
    # everything culled, opacities without grad, fp16 inputs
    t = scene(500, 2, "sh_sr", 3)
    t["means3D"][:, 2] = -1.0
    m = t["means3D"].clone().requires_grad_(True)
    img, radii = GaussianRasterizer(rs)(m, None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    img.sum().backward()
    assert int(radii.max()) == 0 and torch.count_nonzero(m.grad) == 0
    t = scene(800, 3, "sh_sr", 3)
    m16 = t["means3D"].half().requires_grad_(True)
    sh = t["shs"].clone().requires_grad_(True)
    op = t["opacities"].clone()
    img, _ = GaussianRasterizer(rs)(m16, None, op, shs=sh, scales=t["scales"], rotations=t["rotations"])
    img.sum().backward()
    assert m16.grad is not None and m16.grad.dtype == torch.float16 and op.grad is None
    assert torch.isfinite(m16.grad.float()).all() and sh.grad.abs().sum() > 0
    assert img.grad_fn is not None


def test_adam_recovers_colours():
    W, H, P = 96, 72, 2000
    t = scene(P, 13, "precomp_sr", 3)
    rs = settings(synthetic.camera(W, H), W, H, 0)
    with torch.no_grad():
        target, _ = GaussianRasterizer(rs)(t["means3D"], None, t["opacities"], colors_precomp=t["colors_precomp"],
                                           scales=t["scales"], rotations=t["rotations"])
    col = torch.full_like(t["colors_precomp"], 0.5).requires_grad_(True)
    opt = torch.optim.Adam([col], lr=0.05)
    losses = []
    for _ in range(200):
        opt.zero_grad()
        img, _ = GaussianRasterizer(rs)(t["means3D"], None, t["opacities"], colors_precomp=col, scales=t["scales"],
                                        rotations=t["rotations"])
        loss = ((img - target) ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] <= losses[0] / 10, (losses[0], losses[-1])


# ---- production-size paths: more than 64 chunks of 2 048 depth-ordered Gaussians (a tile's list spans several 64-chunk
# windows: the render backward walks back across them, the KEEP forward's n_contrib counts across them) and more than
# 1 024 blocks of 256 (view, Gaussian) pairs (the slot-base scan carries across its iterations)

def dense_small_scene(P, W, H, seed):
    """P small, faint Gaussians filling the frustum at depths 2 .. 4: every pixel sees ~100 of them and stays far from
    saturation, so its last blended entry lies deep in its tile's list."""
    rng = np.random.default_rng(seed)
    cam = synthetic.camera(W, H)
    z = rng.uniform(2.0, 4.0, P)
    x = rng.uniform(-1.05, 1.05, P) * cam["tanfovx"] * z
    y = rng.uniform(-1.05, 1.05, P) * cam["tanfovy"] * z
    q = rng.normal(size=(P, 4))
    t = {"means3D": np.stack([x, y, z], 1), "opacities": rng.uniform(0.01, 0.05, (P, 1)),
         "colors_precomp": rng.random((P, 3)), "scales": rng.uniform(0.002, 0.008, (P, 3)),
         "rotations": q / np.linalg.norm(q, axis=1, keepdims=True)}
    return cam, {k: torch.from_numpy(np.asarray(v, np.float32)).cuda() for k, v in t.items()}


def multi_window_state(img, V, H, W):
    """final_T of the autograd forward (kept on the autograd node)"""
    return img.grad_fn.state[:V * H * W]


def check_colour_linearity(sets, t, seed):
    """With colors_precomp the image is affine in the colours for fixed blend decisions: sum(dL/dc * dc) must equal
    L(c + dc) - L(c) up to fp32 rounding of the images."""
    V = len(sets)
    W, H = sets[0].image_width, sets[0].image_height
    rng = np.random.default_rng(seed)
    gout = torch.from_numpy(rng.normal(size=(V, 3, H, W))).cuda().float()
    dc = torch.from_numpy(rng.normal(0.0, 0.05, t["colors_precomp"].shape)).cuda().float()
    col = t["colors_precomp"].clone().requires_grad_(True)
    img, radii, _ = rasterize_views(sets, t["means3D"], t["opacities"], colors_precomp=col, scales=t["scales"],
                                    rotations=t["rotations"])
    (img * gout).sum().backward()
    with torch.no_grad():
        img2, _, _ = rasterize_views(sets, t["means3D"], t["opacities"], colors_precomp=t["colors_precomp"] + dc,
                                     scales=t["scales"], rotations=t["rotations"])
    d_lin = (col.grad.double() * dc.double()).sum().item()
    d_img = ((img2.double() - img.detach().double()) * gout.double()).sum().item()
    assert abs(d_lin - d_img) <= 1e-4 * abs(d_img) + 1e-3, (d_lin, d_img)
    return img, radii


def test_colour_linearity_many_chunks():
    W, H, P = 128, 96, 300_000  # 147 chunks, 1 172 scan blocks
    cam, t = dense_small_scene(P, W, H, 21)
    sets = [settings(cam, W, H, 0)]
    img, radii = check_colour_linearity(sets, t, 0)
    assert int((radii > 0).sum()) > 2 * 64 * 2048  # visible Gaussians span more than two 64-chunk windows
    assert multi_window_state(img, 1, H, W).median().item() > 1e-2  # pixels far from saturation: deep n_contrib


@pytest.mark.parametrize("V", [1, 4])
def test_colour_linearity_c2_1m(V):
    W, H, P = 640, 480, 1_000_000  # the benchmark scene: 489 chunks, 3 907 x V scan blocks
    g = synthetic.gaussians_c2(P, 0)
    t = {k: torch.from_numpy(g[k]).cuda() for k in ("means3D", "opacities", "scales", "rotations")}
    t["colors_precomp"] = torch.from_numpy(np.random.default_rng(1).random((P, 3)).astype(np.float32)).cuda()
    sets = [settings(c, W, H, 0) for c in synthetic.camera_ring(V, W, H)]
    check_colour_linearity(sets, t, V)


def test_many_chunks_match_float64_reference():
    """All gradients at 300 k Gaussians against the float64 reference, the loss restricted to three tiles (the reference
    composites only their pixels; every visible Gaussian still takes part in their depth order)."""
    W, H, P = 128, 96, 300_000
    cam, t = dense_small_scene(P, W, H, 22)
    rs = settings(cam, W, H, 0)
    gout = torch.zeros((3, H, W), device="cuda")
    pix = []
    for tx, ty in ((0, 0), (3, 2), (7, 5)):
        yy, xx = torch.meshgrid(torch.arange(ty * 16, ty * 16 + 16), torch.arange(tx * 16, tx * 16 + 16), indexing="ij")
        pix.append((yy * W + xx).reshape(-1))
    pix = torch.cat(pix).cuda()
    rng = torch.Generator(device="cuda").manual_seed(5)
    gout.view(3, -1)[:, pix] = torch.randn((3, pix.numel()), device="cuda", generator=rng)
    gg, img, radii = gpu_grads(rs, t, gout)
    rg, rimg, rradii = rt.grads(rt.camera_dict(cam, W, H), BG, gout.double(), chunk=32, pixels=pix, sh_degree=0,
                                scale_modifier=MOD, **t)
    diff = (img.double() - rimg).abs().amax(0).view(-1)[pix]
    assert (diff > 1e-4).double().mean().item() <= 1e-2
    for k in list(t) + ["means2D"]:
        check_close(gg[k], rg[k], rradii, k)


def test_multiview_many_blocks_is_sum_of_single_views():
    W, H, P, V = 128, 96, 300_000, 2  # P * V = 600 k pairs: 2 344 scan blocks
    _, t = dense_small_scene(P, W, H, 23)
    cams = synthetic.camera_ring(V, W, H, seed=4)
    sets = [settings(c, W, H, 0) for c in cams]
    gout = torch.from_numpy(np.random.default_rng(6).normal(size=(V, 3, H, W))).cuda().float()
    leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    img, _, _ = rasterize_views(sets, leaves["means3D"], leaves["opacities"], colors_precomp=leaves["colors_precomp"],
                                scales=leaves["scales"], rotations=leaves["rotations"])
    (img * gout).sum().backward()
    acc = {k: torch.zeros_like(v) for k, v in t.items()}
    for v in range(V):
        g1, _, _ = gpu_grads(sets[v], t, gout[v], means2D=False)
        for k in acc:
            acc[k] += g1[k]
    for k in acc:
        scale = acc[k].abs().max().item()
        assert torch.allclose(leaves[k].grad, acc[k], rtol=0, atol=1e-6 * scale + 1e-30), k


def test_image_under_grad_is_a_tensor_of_its_own():
    W, H, P = 64, 48, 500
    t = scene(P, 4, "precomp_sr", 0)
    col = t["colors_precomp"].clone().requires_grad_(True)
    img, _ = GaussianRasterizer(settings(synthetic.camera(W, H), W, H, 0))(
        t["means3D"], None, t["opacities"], colors_precomp=col, scales=t["scales"], rotations=t["rotations"])
    out = img.clamp(0, 1)
    out.clamp_(0, 0.5)  # in-place on a result derived from the image
    img.mul_(1.0)        # and on the image itself, as upstream's output allows
    img.sum().backward()
    assert col.grad is not None


def test_means2D_shape_is_checked_at_the_call():
    W, H, P = 64, 48, 100
    t = scene(P, 4, "precomp_sr", 0)
    sets = [settings(c, W, H, 0) for c in synthetic.camera_ring(2, W, H)]
    m = t["means3D"].clone().requires_grad_(True)
    with pytest.raises(ValueError, match="means2D"):
        rasterize_views(sets, m, t["opacities"], colors_precomp=t["colors_precomp"], scales=t["scales"],
                        rotations=t["rotations"], means2D=torch.zeros((P, 3), device="cuda", requires_grad=True))
