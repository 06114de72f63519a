"""CPU: the float64 reference for the camera gradients (tests/raster_cam_torch64.py) against central differences, the
pose helpers of gaussreg_amd/pose.py, and the C ABI of gr_raster_backward_cam.

Bound of the finite-difference checks: 1e-5 relative in norm per tensor.  With step 1e-7 on float64 values of order one,
central differences carry a truncation error of order step^2 and a rounding error of order eps |L| / step ~ 1e-9 |L|; the
colour case was measured at 2.1e-7 (viewmatrix), 2.1e-9 (projmatrix), 8.5e-8 (campos) when the bound was set, and here at
9.7e-8, 2.1e-9, 9.2e-8; colour + depth + alpha at 4.1e-9, 1.5e-9, 1.1e-7.  1e-5 is two orders above that and far below
what a sign, transpose or missing-term error gives (order one)."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import raster_cam_torch64 as rc  # noqa: E402
import raster_torch64 as rt  # noqa: E402
from gaussreg_amd import pose, synthetic  # noqa: E402

BG = [0.25, 0.5, 0.1]
W, H, P, DEG = 64, 48, 400, 3
STEP = 1e-7
BOUND = 1e-5


def _scene():
    g = synthetic.gaussians_c2(P, 11)
    return {k: torch.from_numpy(g[k]).double() for k in ("means3D", "opacities", "shs", "scales", "rotations")}


def _camera():
    cam = rt.camera_dict(synthetic.camera_ring(2, W, H, seed=1)[1], W, H)
    for k in rc.CAM_NAMES:  # float64 copies in logical layout: the finite differences perturb these
        cam[k] = torch.from_numpy(np.ascontiguousarray(cam[k])).double()
    return cam


def _central_differences(cam, name, **kw):
    base = cam[name]
    out = torch.zeros_like(base)
    flat = out.view(-1)
    for e in range(base.numel()):
        vals = []
        for sign in (1.0, -1.0):
            c = dict(cam)
            t = base.clone()
            t.view(-1)[e] += sign * STEP
            c[name] = t
            vals.append(rc.loss_value(c, BG, **kw))
        flat[e] = (vals[0] - vals[1]) / (2.0 * STEP)
    return out


def _check(cam, g, **kw):
    for name in rc.CAM_NAMES:
        fd = _central_differences(cam, name, **kw)
        rel = (torch.linalg.norm(g[name] - fd) / torch.linalg.norm(fd)).item()
        print(f"{name}: |autograd - central differences| / |central differences| = {rel:.3e}")
        assert rel <= BOUND, (name, rel)
    # the entries the forward never reads
    assert torch.count_nonzero(g["viewmatrix"][:, 3]) == 0
    assert torch.count_nonzero(g["projmatrix"][:, 2]) == 0
    for name, cols in (("viewmatrix", (0, 1, 2)), ("projmatrix", (0, 1, 3))):
        assert all(torch.count_nonzero(g[name][:, c]) == 4 for c in cols), name
    assert torch.count_nonzero(g["campos"]) == 3


def test_colour_reference_matches_central_differences():
    t, cam = _scene(), _camera()
    gout = torch.from_numpy(np.random.default_rng(0).normal(size=(3, H, W)))
    kw = dict(g_color=gout, sh_degree=DEG, scale_modifier=0.9, **t)
    _check(cam, rc.grads(cam, BG, **kw), **kw)


def test_depth_alpha_reference_matches_central_differences():
    t, cam = _scene(), _camera()
    rng = np.random.default_rng(1)
    kw = dict(g_color=torch.from_numpy(rng.normal(size=(3, H, W))), g_depth=torch.from_numpy(rng.normal(size=(H, W))),
              g_alpha=torch.from_numpy(rng.normal(size=(H, W))), sh_degree=DEG, scale_modifier=0.9, **t)
    _check(cam, rc.grads(cam, BG, **kw), **kw)


def test_campos_gradient_is_zero_with_precomputed_colours():
    t, cam = _scene(), _camera()
    del t["shs"]
    t["colors_precomp"] = torch.from_numpy(np.random.default_rng(2).random((P, 3)))
    gout = torch.from_numpy(np.random.default_rng(3).normal(size=(3, H, W)))
    g = rc.grads(cam, BG, g_color=gout, sh_degree=0, scale_modifier=0.9, **t)
    assert torch.count_nonzero(g["campos"]) == 0 and torch.count_nonzero(g["viewmatrix"]) == 12


def _ring_poses(V, seed):
    """(R_c2w, C) of synthetic.camera_ring's cameras: the same draws."""
    rng = np.random.default_rng(1000 + seed)
    poses = [(np.eye(3), np.zeros(3))]
    for _ in range(1, V):
        yaw, pitch = rng.uniform(-0.25, 0.25), rng.uniform(-0.15, 0.15)
        C = rng.uniform(-0.4, 0.4, 3) * np.array([1.0, 0.6, 0.5])
        poses.append((synthetic.rot_yx(yaw, pitch), C))
    return poses


def test_camera_tensors_equal_synthetic_camera():
    V = 6
    cams = synthetic.camera_ring(V, W, H, seed=3)
    for cam, (R, C) in zip(cams, _ring_poses(V, 3)):
        vm, pm, cp = pose.camera_tensors(torch.from_numpy(R), torch.from_numpy(C), cam["tanfovx"], cam["tanfovy"])
        for got, want in ((vm, cam["viewmatrix"]), (pm, cam["projmatrix"]), (cp, cam["campos"])):
            want = torch.from_numpy(np.ascontiguousarray(want)).double()
            # synthetic.camera rounds its float64 result to fp32 once: half an fp32 ulp, relative to the entry (entries are
            # of order one; a few ulps of float64 cancellation in the products are far below that)
            assert got.shape == want.shape
            assert torch.all((got - want).abs() <= 2.0 ** -24 * want.abs().clamp_min(1.0) + 1e-12)
    # differentiable in the pose
    R = torch.from_numpy(_ring_poses(2, 3)[1][0]).requires_grad_(True)
    C = torch.from_numpy(_ring_poses(2, 3)[1][1]).requires_grad_(True)
    vm, pm, cp = pose.camera_tensors(R, C, 0.5, 0.4)
    (vm.sum() + pm.sum() + cp.sum()).backward()
    assert R.grad is not None and C.grad is not None


def test_similarity_camera_defining_identity():
    rng = np.random.default_rng(7)
    Rc, Cc = _ring_poses(3, 5)[2]  # float64 throughout: projmatrix is exactly viewmatrix times the perspective matrix
    vm, pm, _ = pose.camera_tensors(torch.from_numpy(Rc), torch.from_numpy(Cc), 0.6, 0.45)
    s = 1.3
    R = pose.so3_exp(torch.tensor([0.2, -0.1, 0.3], dtype=torch.float64))
    t = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    assert torch.allclose(R @ R.T, torch.eye(3, dtype=torch.float64), atol=1e-14)
    vm2, pm2, cp2, depth_factor = pose.similarity_camera(vm, s, R, t, projmatrix=pm)
    X = torch.from_numpy(rng.normal(size=(100, 3)) * 2.0)
    ones = torch.ones((100, 1), dtype=torch.float64)
    moved = s * X @ R.T + t
    old_view = torch.cat([moved, ones], 1) @ vm      # the transformed point seen from the old camera
    new_view = torch.cat([X, ones], 1) @ vm2         # the original point seen from the new one
    assert torch.allclose(old_view[:, :3], float(depth_factor) * new_view[:, :3], rtol=0, atol=1e-12)
    assert float(depth_factor) == s
    # same pixel: the homogeneous projections are proportional
    old_h = torch.cat([moved, ones], 1) @ pm
    new_h = torch.cat([X, ones], 1) @ pm2
    # (float64 rounding times the size of the quotient: points near the camera plane have a small w)
    assert torch.allclose(old_h[:, :2] / old_h[:, 3:4], new_h[:, :2] / new_h[:, 3:4], rtol=1e-9, atol=1e-12)
    # the new camera is rigid and campos is its centre
    assert torch.allclose(vm2[:3, :3] @ vm2[:3, :3].T, torch.eye(3, dtype=torch.float64), atol=1e-14)
    centre_view = torch.cat([cp2, torch.ones(1, dtype=torch.float64)]) @ vm2
    assert torch.allclose(centre_view[:3], torch.zeros(3, dtype=torch.float64), atol=1e-14)
    assert math.isclose(float(vm2[3, 3]), 1.0)


def test_cam_entry_points_in_header_exports_and_ctypes_table():
    from gaussreg_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "gaussreg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    build.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gr_raster_backward_cam_bytes", "gr_raster_backward_cam"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    # the argument list is gr_raster_backward_aux's plus the three camera outputs in front of the scratch buffer
    aux, cam = _lib.SIGNATURES["gr_raster_backward_aux"][1], _lib.SIGNATURES["gr_raster_backward_cam"][1]
    assert len(cam) == len(aux) + 3 and cam[:len(aux) - 3] == aux[:-3] and cam[-3:] == aux[-3:]
    m = re.search(r"#define\s+GR_RASTER_BWD_COLOR_ONLY\s+(\d+)", text)
    from gaussreg_amd import rasterizer
    assert m and int(m.group(1)) == rasterizer.BWD_COLOR_ONLY
    # scratch: the camera partials (27 floats per view and 256 Gaussians) come on top of the slot layout the flags select
    nr = (ctypes.c_int64 * 2)(1000, 0)
    Lc = _lib.lib()
    extra = Lc.gr_raster_backward_cam_bytes(5000, 1, 64, 48, nr, 0) - Lc.gr_raster_backward_aux_bytes(5000, 1, 64, 48, nr)
    assert 27 * 4 * 20 <= extra <= 27 * 4 * 20 + 512  # (buffers are carved at 256-byte boundaries)
    extra = (Lc.gr_raster_backward_cam_bytes(5000, 1, 64, 48, nr, rasterizer.BWD_COLOR_ONLY) -
             Lc.gr_raster_backward_bytes(5000, 1, 64, 48, nr))
    assert 27 * 4 * 20 <= extra <= 27 * 4 * 20 + 512
