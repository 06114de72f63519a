"""GPU parity of the multi-view preprocess (one thread per Gaussian looping over the cameras) on its rarer paths: wide
rectangles that take the RECT_MARKER26 fallback, far depths that take the full-key sort, Gaussian counts that leave a
partial last wave, and a scale modifier that changes between the views of one call (cov3D is rebuilt from the inputs
there).  Images and radii stay BIT-EXACT to oracle/rasterizer_oracle.c."""
import numpy as np
import pytest
import torch

from helpers import raster_scene, oracle_render

pytestmark = pytest.mark.gpu


def _settings(cam, scale_modifier=1.0, bg=(0.1, 0.3, 0.2)):
    from gaussreg_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=cam["image_height"], image_width=cam["image_width"], tanfovx=cam["tanfovx"],
        tanfovy=cam["tanfovy"], bg=torch.tensor(bg, dtype=torch.float32, device="cuda"), scale_modifier=scale_modifier,
        viewmatrix=torch.from_numpy(cam["viewmatrix"]).cuda(), projmatrix=torch.from_numpy(cam["projmatrix"]).cuda(),
        sh_degree=3, campos=torch.from_numpy(cam["campos"]).cuda(), prefiltered=False, debug=False)


def _check_views(g, cams, mods=None, bg=(0.1, 0.3, 0.2)):
    """All cameras in one rasterize_views call; every image and radii row must equal the oracle's bit for bit.
    Returns the oracle's radii per view."""
    from gaussreg_amd.rasterizer import rasterize_views
    mods = mods or [1.0] * len(cams)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in g.items()}
    imgs, radii, _ = rasterize_views([_settings(c, m, bg) for c, m in zip(cams, mods)], d["means3D"], d["opacities"],
                                     shs=d["shs"], scales=d["scales"], rotations=d["rotations"])
    imgs, radii = imgs.cpu().numpy(), radii.cpu().numpy()
    want_radii = []
    for v, (cam, m) in enumerate(zip(cams, mods)):
        want, wr, _ = oracle_render(g, cam, bg=bg, scale_modifier=m)
        assert np.array_equal(radii[v], wr), f"view {v}: radii"
        got = np.ascontiguousarray(imgs[v])
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, (f"view {v} of {len(cams)}: {len(bad)} of {got.size} values differ; first at {bad[0]}: "
                               f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")
        want_radii.append(wr)
    return want_radii


@pytest.mark.parametrize("V", [3, 9])
def test_wide_rectangles_multi_view(V):
    # 1232 px = 77 tiles: a few screen-filling Gaussians (rectangles wider than 63 tiles) among small ones, seen by
    # several cameras (V >= 8 takes the XCD-affine binning)
    W, H, P = 1232, 48, 700
    g, cams = raster_scene(P, W, H, seed=31, V=V)
    g["scales"][:8] = np.float32([2.0, 0.05, 0.05])
    g["means3D"][:8, :2] *= 0.2
    wr = _check_views(g, cams)
    assert sum(int(r[:8].max() > 64 * 16 // 2) for r in wr) >= 2


@pytest.mark.parametrize("V", [2, 9])
def test_far_depths_multi_view(V):
    # the scene and the camera centres scaled by 4000: depths of ~12 km, past the 27-bit rebased key
    P, W, H = 1000, 96, 80
    g, cams = raster_scene(P, W, H, seed=13, V=V)
    k = np.float32(4000.0)
    g["means3D"] = (g["means3D"] * k).astype(np.float32)
    g["scales"] = (g["scales"] * k).astype(np.float32)
    cams = [dict(c) for c in cams]
    for c in cams:   # view = [R^T | -R^T C], stored transposed: the last ROW holds the translation
        vm = c["viewmatrix"].copy()
        vm[3, :3] *= k
        proj = c["projmatrix"].T.astype(np.float64) @ np.linalg.inv(c["viewmatrix"].T.astype(np.float64))
        c["viewmatrix"] = vm
        c["projmatrix"] = (proj @ vm.T.astype(np.float64)).T.astype(np.float32)
        c["campos"] = (c["campos"] * k).astype(np.float32)
    wr = _check_views(g, cams)
    assert all(r.max() > 0 for r in wr)


@pytest.mark.parametrize("P,V", [(1000, 8), (4133, 11)])
def test_partial_last_wave_many_views(P, V):
    # P not a multiple of 64: the last wave's records are written cooperatively by lanes past the end
    g, cams = raster_scene(P, 88, 72, seed=P, V=V)
    _check_views(g, cams)


def test_scale_modifier_changes_between_views():
    # cov3D is built once per Gaussian and rebuilt from scales / rotations only where the modifier changes; the runs of
    # equal modifiers, a change back to an earlier value and a first view that sees nothing all go through one call
    P, W, H, V = 3000, 96, 72, 7
    g, cams = raster_scene(P, W, H, seed=17, V=V)
    cams = [dict(c) for c in cams]
    c0 = dict(cams[0])
    vm = c0["viewmatrix"].copy()
    vm[3, 2] -= np.float32(100.0)   # camera moved 100 units forward along its axis: every Gaussian is behind it
    proj = c0["projmatrix"].T.astype(np.float64) @ np.linalg.inv(c0["viewmatrix"].T.astype(np.float64))
    c0["viewmatrix"] = vm
    c0["projmatrix"] = (proj @ vm.T.astype(np.float64)).T.astype(np.float32)
    cams[0] = c0
    mods = [0.5, 1.0, 1.0, 1.7, 1.7, 1.0, 0.8]
    wr = _check_views(g, cams, mods)
    assert wr[0].max() == 0 and all(r.max() > 0 for r in wr[1:])
