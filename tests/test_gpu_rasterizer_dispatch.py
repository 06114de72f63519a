"""GPU: which C entry points a rasterizer call enters.  The other rasterizer tests compare results, and would pass if, say,
every backward went through gr_raster_backward_cam with null camera outputs; this one replaces `_lib.lib` by a proxy that
forwards to the real library and records the tracked calls, for {colour, render_depth} x {no grad, Gaussian grad, camera
grad}, through rasterize_views (two views) and through GaussianRasterizer (one camera).

Not tracked: gr_raster_render_ex, gr_raster_geom_bytes, gr_raster_bin_bytes, gr_raster_forward_finish (whether they appear
depends on the size hint and the pipe)."""
import os
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussreg_amd import _lib, synthetic  # noqa: E402
from gaussreg_amd.rasterizer import (BWD_COLOR_ONLY, GaussianRasterizationSettings, GaussianRasterizer,  # noqa: E402
                                     rasterize_views)

pytestmark = pytest.mark.gpu
P, DEG, W, H = 300, 1, 64, 48
TRACKED = ("gr_raster_forward", "gr_raster_preprocess", "gr_raster_render_keep", "gr_raster_render_aux",
           "gr_raster_backward", "gr_raster_backward_aux", "gr_raster_backward_cam",
           "gr_raster_backward_bytes", "gr_raster_backward_aux_bytes", "gr_raster_backward_cam_bytes")
# positions in the argument lists of include/gaussreg_hip.h
RENDER_AUX_STATE = 11
CAM_BYTES_FLAGS = 5
CAM_DDEPTH, CAM_DALPHA, CAM_FLAGS = 19, 20, 21


class Recorder:
    """Stands in for the loaded library: every symbol is the real one, the tracked ones note (name, arguments) first."""

    def __init__(self, real):
        self.real = real
        self.calls = []

    def __getattr__(self, name):
        f = getattr(self.real, name)
        if name not in TRACKED:
            return f

        def recorded(*args):
            self.calls.append((name, args))
            return f(*args)
        return recorded


@pytest.fixture
def recorder(monkeypatch):
    monkeypatch.setenv("GR_RASTER_PIPELINE", "0")
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    return rec


def is_null(p):
    return p is None or getattr(p, "value", p) in (None, 0)


def scene(gauss_grad):
    g = synthetic.gaussians_c2(P, 3, sh_degree=DEG)
    return {k: torch.from_numpy(g[k]).cuda().requires_grad_(gauss_grad)
            for k in ("means3D", "opacities", "shs", "scales", "rotations")}


def settings(cam, cam_grad):
    leaves = [torch.from_numpy(cam[k]).cuda().requires_grad_(cam_grad) for k in ("viewmatrix", "projmatrix", "campos")]
    return GaussianRasterizationSettings(H, W, cam["tanfovx"], cam["tanfovy"], torch.zeros(3, device="cuda"), 1.0,
                                         leaves[0], leaves[1], DEG, leaves[2], False, False)


def check(calls, depth, grad):
    """`calls` against the table of entry points per combination: each listed name once, no other tracked name."""
    names = sorted(n for n, _ in calls)
    args = dict(calls)
    if grad == "none":
        expect = ["gr_raster_preprocess", "gr_raster_render_aux"] if depth else ["gr_raster_forward"]
    else:
        family = "gr_raster_backward" + ("_cam" if grad == "camera" else "_aux" if depth else "")
        expect = ["gr_raster_preprocess", "gr_raster_render_aux" if depth else "gr_raster_render_keep", family,
                  family + "_bytes"]
    assert names == sorted(expect), (depth, grad, names)
    if depth:
        assert is_null(args["gr_raster_render_aux"][RENDER_AUX_STATE]) == (grad == "none")
    if grad == "camera":
        a, b = args["gr_raster_backward_cam"], args["gr_raster_backward_cam_bytes"]
        if depth:
            assert b[CAM_BYTES_FLAGS] == 0 and not a[CAM_FLAGS] & BWD_COLOR_ONLY
        else:
            assert b[CAM_BYTES_FLAGS] == BWD_COLOR_ONLY and a[CAM_FLAGS] & BWD_COLOR_ONLY
            assert is_null(a[CAM_DDEPTH]) and is_null(a[CAM_DALPHA])


def loss_of(maps):
    return sum((m * m).sum() for m in maps)


@pytest.mark.parametrize("grad", ["none", "gaussian", "camera"])
@pytest.mark.parametrize("depth", [False, True])
def test_entry_points_of_rasterize_views(recorder, depth, grad):
    V = 2
    t = scene(grad != "none")
    sets = [settings(c, grad == "camera") for c in synthetic.camera_ring(V, W, H, seed=1)]
    res = rasterize_views(sets, t["means3D"], t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
                          fast_exp=False, render_depth=depth)
    maps = (res[0], res[3], res[4]) if depth else (res[0],)
    assert res[0].shape == (V, 3, H, W) and res[1].shape == (V, P) and all(m.shape[2:] == (H, W) for m in maps)
    assert (res[0].grad_fn is None) == (grad == "none")
    if grad != "none":
        loss_of(maps).backward()
    torch.cuda.synchronize()
    check(recorder.calls, depth, grad)


@pytest.mark.parametrize("grad", ["none", "gaussian", "camera"])
@pytest.mark.parametrize("depth", [False, True])
def test_entry_points_of_gaussian_rasterizer(recorder, depth, grad):
    t = scene(grad != "none")
    rast = GaussianRasterizer(settings(synthetic.camera(W, H), grad == "camera"), fast_exp=False, render_depth=depth)
    res = rast(t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    maps = (res[0], res[2], res[3]) if depth else (res[0],)
    assert len(res) == (4 if depth else 2) and res[0].shape == (3, H, W) and res[1].shape == (P,)
    assert all(m.shape == (1, H, W) for m in maps[1:])
    assert (res[0].grad_fn is None) == (grad == "none")
    if grad != "none":
        loss_of(maps).backward()
    torch.cuda.synchronize()
    check(recorder.calls, depth, grad)
