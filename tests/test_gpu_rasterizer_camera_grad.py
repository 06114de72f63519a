"""GPU: gradients of the rasterizer with respect to the camera tensors (viewmatrix, projmatrix, campos; HIP:
gr_raster_backward_cam) against the float64 reference of tests/raster_cam_torch64.py (pinned against central differences
by tests/test_raster_cam_reference.py), plus the contract: exact zeros where the forward reads nothing, per-view
independence and bitwise reproducibility, nothing else changes bit for bit, any dtype / strides / device of the camera
tensors, prebuilt ViewBatch and cached GaussianRasterizer, and a pose refinement end to end.

Bound of every comparison with the reference: the project's gradient tolerance, |g - g64| <= 1e-3 |g64| in norm per
tensor (measured on an MI355X: 4.1e-6 .. 4.1e-5)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import raster_cam_torch64 as rc  # noqa: E402
import raster_torch64 as rt  # noqa: E402
from gaussreg_amd import pose, synthetic  # noqa: E402
from gaussreg_amd.rasterizer import (GaussianRasterizationSettings, GaussianRasterizer, ViewBatch,  # noqa: E402
                                     rasterize_views)

pytestmark = pytest.mark.gpu
BG = [0.25, 0.5, 0.1]
MOD = 0.9
CAMS = rc.CAM_NAMES


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def cam_leaves(cam, grad=True, dtype=torch.float32):
    """The camera tensors on the device as synthetic.camera lays them out (transposed views: NOT contiguous)."""
    d = torch.device("cuda")
    return {k: torch.from_numpy(cam[k]).to(d, dtype).requires_grad_(grad) for k in CAMS}


def settings(cam, W, H, deg, leaves):
    return GaussianRasterizationSettings(H, W, cam["tanfovx"], cam["tanfovy"], torch.tensor(BG, device="cuda"), MOD,
                                         leaves["viewmatrix"], leaves["projmatrix"], deg, leaves["campos"], False, False)


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


def kwargs(t):
    return dict(shs=t.get("shs"), colors_precomp=t.get("colors_precomp"), scales=t.get("scales"),
                rotations=t.get("rotations"), cov3D_precomp=t.get("cov3D_precomp"))


def off_axis(W, H):
    return synthetic.camera_ring(2, W, H, seed=1)[1]


def gouts(seed, H, W, depth, V=None):
    rng = np.random.default_rng(seed)
    lead = () if V is None else (V,)
    f = lambda *s: torch.from_numpy(rng.normal(size=lead + s)).cuda().float()  # noqa: E731
    return (f(3, H, W), f(1, H, W), f(1, H, W)) if depth else (f(3, H, W), None, None)


def render_loss(rs, t, g, depth, gauss_grad=False):
    """One camera through GaussianRasterizer; -> (outputs, Gaussian leaves or None)."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()} if gauss_grad else None
    src = leaves if gauss_grad else t
    out = GaussianRasterizer(rs, render_depth=depth)(src["means3D"], None, src["opacities"], **kwargs(src))
    loss = (out[0] * g[0]).sum()
    if depth:
        loss = loss + (out[2] * g[1]).sum() + (out[3] * g[2]).sum()
    return out, loss, leaves


def reference(cam, W, H, t, g, deg, pixels=None, chunk=2048):
    mod = 1.0 if "cov3D_precomp" in t else MOD  # the precomputed covariance already holds the modifier
    return rc.grads(rt.camera_dict(cam, W, H), BG, g_color=g[0], g_depth=g[1], g_alpha=g[2], chunk=chunk, pixels=pixels,
                    sh_degree=deg, scale_modifier=mod, **t)


def check_close(g, r, name):
    rel = (torch.linalg.norm(g.double() - r) / torch.linalg.norm(r).clamp_min(1e-30)).item()
    print(f"{name}: |g - g64| / |g64| = {rel:.3e}")
    assert rel <= 1e-3, f"{name}: |g - g64| / |g64| = {rel:.3e}"


def check_zero_pattern(cl, has_sh):
    assert torch.count_nonzero(cl["viewmatrix"].grad[:, 3]) == 0
    assert torch.count_nonzero(cl["projmatrix"].grad[:, 2]) == 0
    assert torch.count_nonzero(cl["viewmatrix"].grad[:, :3]) == 12
    if not has_sh:
        assert torch.count_nonzero(cl["campos"].grad) == 0


def compare(t, W, H, cam, deg, depth, seed=0):
    cl = cam_leaves(cam)
    g = gouts(seed, H, W, depth)
    _, loss, _ = render_loss(settings(cam, W, H, deg, cl), t, g, depth)
    loss.backward()
    ref = reference(cam, W, H, t, g, deg)
    for k in CAMS:
        assert cl[k].grad is not None, k
        assert cl[k].grad.shape == cl[k].shape and cl[k].grad.dtype == cl[k].dtype
        if k == "campos" and "shs" not in t:
            assert torch.count_nonzero(ref[k]) == 0
            continue
        check_close(cl[k].grad, ref[k], k)
    check_zero_pattern(cl, "shs" in t)


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("mode,deg", [("sh_sr", 0), ("sh_sr", 3), ("sh_cov", 3), ("precomp_sr", 3), ("precomp_cov", 3)])
def test_camera_gradients_match_float64_reference(mode, deg, depth):
    W, H, P = 120, 88, 2500
    compare(scene(P, 11, mode, deg), W, H, off_axis(W, H), deg, depth)


@pytest.mark.parametrize("depth", [False, True])
def test_camera_gradients_large_scene_odd_size(depth):
    W, H, P = 262, 198, 10000  # not multiples of 16
    compare(scene(P, 3, "sh_sr", 3), W, H, off_axis(W, H), 3, depth, seed=1)


def test_production_size_many_workgroups():
    """The C2 scene at 300 k Gaussians (1 172 workgroups of partial sums per view), 640 x 480, the loss on three tiles."""
    W, H, P = 640, 480, 300_000
    t = scene(P, 0, "sh_sr", 3)
    cam = off_axis(W, H)
    pix = []
    for tx, ty in ((3, 2), (20, 15), (33, 24)):
        yy, xx = torch.meshgrid(torch.arange(ty * 16, ty * 16 + 16), torch.arange(tx * 16, tx * 16 + 16), indexing="ij")
        pix.append((yy * W + xx).reshape(-1))
    pix = torch.cat(pix).cuda()
    gen = torch.Generator(device="cuda").manual_seed(5)
    g = [torch.zeros((3, H, W), device="cuda"), torch.zeros((1, H, W), device="cuda"), torch.zeros((1, H, W), device="cuda")]
    for x in g:
        x.view(x.shape[0], -1)[:, pix] = torch.randn((x.shape[0], pix.numel()), device="cuda", generator=gen)
    cl = cam_leaves(cam)
    _, loss, _ = render_loss(settings(cam, W, H, 3, cl), t, g, True)
    loss.backward()
    ref = reference(cam, W, H, t, g, 3, pixels=pix, chunk=32)
    for k in CAMS:
        check_close(cl[k].grad, ref[k], k)
    check_zero_pattern(cl, True)


def multiview(sets, t, g, depth):
    res = rasterize_views(sets, t["means3D"], t["opacities"], render_depth=depth, **kwargs(t))
    loss = (res[0] * g[0]).sum()
    if depth:
        loss = loss + (res[3] * g[1]).sum() + (res[4] * g[2]).sum()
    loss.backward()
    return res


@pytest.mark.parametrize("depth", [False, True])
def test_views_are_independent_and_runs_are_bitwise_equal(depth):
    W, H, P, V = 128, 96, 4000, 4
    t = scene(P, 8, "sh_sr", 3)
    cams = synthetic.camera_ring(V, W, H, seed=2)
    g = gouts(5, H, W, depth, V=V)
    runs = []
    for _ in range(2):
        cls = [cam_leaves(c) for c in cams]
        multiview([settings(c, W, H, 3, cl) for c, cl in zip(cams, cls)], t, g, depth)
        runs.append(cls)
    for v in range(V):
        cl1 = cam_leaves(cams[v])
        multiview([settings(cams[v], W, H, 3, cl1)], t, [None if x is None else x[v:v + 1] for x in g], depth)
        for k in CAMS:
            assert torch.count_nonzero(runs[0][v][k].grad) > 0, (v, k)
            assert torch.equal(bits(runs[0][v][k].grad), bits(runs[1][v][k].grad)), (v, k)
            assert torch.equal(bits(runs[0][v][k].grad), bits(cl1[k].grad)), (v, k)


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("mode", ["sh_sr", "precomp_cov"])
def test_nothing_else_changes(mode, depth):
    """Forward outputs and Gaussian gradients of a call whose cameras require grad are bit-identical to the call with
    detached cameras (which runs gr_raster_backward / gr_raster_backward_aux as before).
    That the detached call in turn reproduces the results from before camera gradients existed is not something a test
    can see from inside one build: it rests on the comparison of instruction streams recorded in DESIGN.md 3.3.3 (the
    kernels of those two entry points are unchanged, instruction for instruction)."""
    W, H, P = 200, 150, 8000
    t = scene(P, 6, mode, 3)
    cam = off_axis(W, H)
    g = gouts(9, H, W, depth)
    res = []
    for grad in (True, False):
        cl = cam_leaves(cam, grad=grad)
        out, loss, leaves = render_loss(settings(cam, W, H, 3, cl), t, g, depth, gauss_grad=True)
        loss.backward()
        res.append((out, leaves, cl))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(bits(a.float()) if a.dtype != torch.int32 else a, bits(b.float()) if b.dtype != torch.int32 else b)
    for k in res[0][1]:
        assert torch.equal(bits(res[0][1][k].grad), bits(res[1][1][k].grad)), k
    assert all(res[1][2][k].grad is None for k in CAMS) and all(res[0][2][k].grad is not None for k in CAMS)
    with torch.no_grad():  # and the forward-only path
        cl = cam_leaves(cam, grad=True)
        out = GaussianRasterizer(settings(cam, W, H, 3, cl), render_depth=depth)(t["means3D"], None, t["opacities"],
                                                                                **kwargs(t))
    assert out[0].grad_fn is None and torch.equal(bits(out[0]), bits(res[0][0][0]))


def test_dtype_strides_and_device_of_the_camera_tensors():
    W, H, P = 120, 88, 2500
    t = scene(P, 11, "sh_sr", 3)
    cam = off_axis(W, H)
    g = gouts(0, H, W, True)

    def run(cl):
        _, loss, _ = render_loss(settings(cam, W, H, 3, cl), t, g, True)
        loss.backward()
        return cl
    base = run(cam_leaves(cam))
    assert not base["viewmatrix"].is_contiguous()  # synthetic.camera's transposed views
    contig = run({k: torch.from_numpy(np.ascontiguousarray(cam[k])).cuda().requires_grad_(True) for k in CAMS})
    f64 = run(cam_leaves(cam, dtype=torch.float64))
    cpu = run({k: torch.from_numpy(cam[k]).clone().requires_grad_(True) for k in CAMS})
    flat = run({k: torch.from_numpy(np.ascontiguousarray(cam[k])).cuda().reshape(-1).requires_grad_(True) for k in CAMS})
    for k in CAMS:
        assert contig[k].grad.is_contiguous() and torch.equal(bits(contig[k].grad), bits(base[k].grad)), k
        assert f64[k].grad.dtype == torch.float64 and torch.equal(f64[k].grad.float(), base[k].grad), k
        assert cpu[k].grad.device.type == "cpu" and torch.equal(cpu[k].grad, base[k].grad.cpu()), k
        assert flat[k].grad.shape == flat[k].shape and torch.equal(flat[k].grad, base[k].grad.reshape(-1)), k
    # one tensor with grad is enough, the others get none
    only = cam_leaves(cam, grad=False)
    only["projmatrix"].requires_grad_(True)
    run(only)
    assert torch.equal(bits(only["projmatrix"].grad), bits(base["projmatrix"].grad))
    assert only["viewmatrix"].grad is None and only["campos"].grad is None


def test_prebuilt_view_batch_and_cached_rasterizer():
    W, H, P = 120, 88, 2500
    t = scene(P, 11, "sh_sr", 3)
    cams = synthetic.camera_ring(3, W, H, seed=4)
    g = gouts(1, H, W, False, V=3)
    cls = [cam_leaves(c) for c in cams]
    multiview([settings(c, W, H, 3, cl) for c, cl in zip(cams, cls)], t, g, False)
    cls2 = [cam_leaves(c) for c in cams]
    vb = ViewBatch([settings(c, W, H, 3, cl) for c, cl in zip(cams, cls2)])
    for _ in range(2):  # reused: gradients accumulate on the leaves as with any autograd input
        multiview(vb, t, g, False)
    for a, b in zip(cls, cls2):
        for k in CAMS:
            assert torch.equal(bits(a[k].grad + a[k].grad), bits(b[k].grad)), k
    # a cached GaussianRasterizer whose camera is updated in place between two steps renders the new camera
    cl = cam_leaves(cams[1])
    r = GaussianRasterizer(settings(cams[1], W, H, 3, cl))
    g1 = gouts(2, H, W, False)
    img_a, _ = r(t["means3D"], None, t["opacities"], **kwargs(t))
    (img_a * g1[0]).sum().backward()
    grad_a = {k: cl[k].grad.clone() for k in CAMS}
    with torch.no_grad():
        for k in CAMS:
            cl[k].copy_(torch.from_numpy(cams[2][k]).cuda())
            cl[k].grad = None
    img_b, _ = r(t["means3D"], None, t["opacities"], **kwargs(t))
    (img_b * g1[0]).sum().backward()
    fresh = cam_leaves(cams[2])
    img_c, _ = GaussianRasterizer(settings(cams[2], W, H, 3, fresh))(t["means3D"], None, t["opacities"], **kwargs(t))
    (img_c * g1[0]).sum().backward()
    assert torch.equal(bits(img_b), bits(img_c)) and not torch.equal(bits(img_a), bits(img_b))
    for k in CAMS:
        assert torch.equal(bits(cl[k].grad), bits(fresh[k].grad)), k
        assert not torch.equal(bits(cl[k].grad), bits(grad_a[k])), k


def rotation_angle(Ra, Rb):
    c = (torch.trace(Ra.T @ Rb).item() - 1.0) / 2.0
    return math.acos(max(-1.0, min(1.0, c)))


def test_adam_refines_a_perturbed_pose():
    """30 Adam steps on (rotation vector, centre) through pose.camera_tensors against the image of the true camera.  The
    step size is a tenth of the perturbation (no step can overshoot by more than that); nothing else is tuned."""
    W, H, P = 160, 120, 5000
    t = scene(P, 14, "sh_sr", 3)
    cam = synthetic.camera(W, H)
    d = torch.device("cuda")
    R_true = torch.from_numpy(synthetic.rot_yx(0.1, -0.05)).float().to(d)
    C_true = torch.tensor([0.1, -0.05, 0.05], device=d)

    def render(R, C):
        vm, pm, cp = pose.camera_tensors(R, C, cam["tanfovx"], cam["tanfovy"])
        rs = GaussianRasterizationSettings(H, W, cam["tanfovx"], cam["tanfovy"], torch.tensor(BG, device=d), MOD, vm, pm, 3,
                                           cp, False, False)
        return GaussianRasterizer(rs)(t["means3D"], None, t["opacities"], **kwargs(t))[0]
    with torch.no_grad():
        target = render(R_true, C_true)
    pert = 0.02
    w0 = torch.tensor([pert, -pert, pert], device=d)
    R_start = R_true @ pose.so3_exp(w0)
    C_start = C_true + torch.tensor([pert, pert, -pert], device=d)
    w = torch.zeros(3, device=d, requires_grad=True)
    dc = torch.zeros(3, device=d, requires_grad=True)
    opt = torch.optim.Adam([w, dc], lr=pert / 10)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = (render(R_start @ pose.so3_exp(w), C_start + dc) - target).abs().mean()
        loss.backward()
        assert w.grad is not None and dc.grad is not None and torch.isfinite(w.grad).all()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        final = (render(R_start @ pose.so3_exp(w), C_start + dc) - target).abs().mean().item()
        rot0, rot1 = rotation_angle(R_true, R_start), rotation_angle(R_true, R_start @ pose.so3_exp(w))
        tr0, tr1 = (C_start - C_true).norm().item(), (C_start + dc - C_true).norm().item()
    print(f"loss {losses[0]:.5f} -> {final:.5f}, rotation {rot0:.5f} -> {rot1:.5f} rad, translation {tr0:.5f} -> {tr1:.5f}")
    assert final < losses[0]
    assert rot1 < rot0 and tr1 < tr0


def test_example_script_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_registration.py"), "--synthetic",
                        "--points", "20000", "--steps", "40"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rotation error" in r.stdout and "translation error" in r.stdout
