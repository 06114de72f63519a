"""GPU parity at the edges of the blend's LDS layout (per-entry records, two list entries per step, a pad entry for odd
lists, batches of 256 entries cut out of windows of 64 depth chunks): the image stays BIT-EXACT to
oracle/rasterizer_oracle.c."""
import numpy as np
import pytest
import torch

from helpers import raster_scene, oracle_render

pytestmark = pytest.mark.gpu


def _settings(cam, bg):
    from gaussreg_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=cam["image_height"], image_width=cam["image_width"], tanfovx=cam["tanfovx"],
        tanfovy=cam["tanfovy"], bg=torch.tensor(bg, dtype=torch.float32, device="cuda"), scale_modifier=1.0,
        viewmatrix=torch.from_numpy(cam["viewmatrix"]).cuda(), projmatrix=torch.from_numpy(cam["projmatrix"]).cuda(),
        sh_degree=3, campos=torch.from_numpy(cam["campos"]).cuda(), prefiltered=False, debug=False)


def _render_all(g, cams, bg=(0.2, 0.4, 0.6)):
    """Every camera in one call; each image must equal the oracle's bit for bit."""
    from gaussreg_amd.rasterizer import rasterize_views
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in g.items()}
    imgs, radii, _ = rasterize_views([_settings(c, bg) for c in cams], d["means3D"], d["opacities"], shs=d["shs"],
                                     scales=d["scales"], rotations=d["rotations"])
    imgs = imgs.cpu().numpy()
    radii = radii.cpu().numpy()
    for v, cam in enumerate(cams):
        want, want_r, _ = oracle_render(g, cam, bg=bg)
        assert np.array_equal(radii[v], want_r), f"view {v}: radii"
        got = np.ascontiguousarray(imgs[v])
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, (f"view {v}: {len(bad)} of {got.size} values differ; first at {bad[0]}: "
                               f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")
    return imgs


@pytest.mark.parametrize("W,H", [(37, 29), (101, 53), (17, 15)])
def test_image_sizes_not_multiples_of_16(W, H):
    g, cams = raster_scene(4000, W, H, seed=W)
    _render_all(g, cams)


@pytest.mark.parametrize("P", [1, 2, 3, 7])
def test_few_entries_single_and_odd_lists(P):
    # a handful of large Gaussians: tiles whose lists hold one entry or an odd number of them
    g, cams = raster_scene(P, 96, 64, seed=P)
    g["scales"] = (g["scales"] * 8.0).astype(np.float32)
    g["opacities"][:] = 0.9
    _render_all(g, cams)


def test_long_lists_over_many_chunk_windows_and_batches():
    # 300 k faint Gaussians over a 64 x 48 image: ~150 depth chunks (more than one window of 64 chunks), several hundred
    # entries per tile (several batches of 256), and no pixel saturates early, so every walk runs to the end
    P = 300_000
    g, cams = raster_scene(P, 64, 48, seed=5)
    g["opacities"][:] = 0.012
    _render_all(g, cams)


def test_zero_and_nan_opacity_entries():
    P = 20_000
    g, cams = raster_scene(P, 80, 64, seed=9)
    op = g["opacities"]
    op[0::7] = 0.0
    op[3::11] = np.nan
    _render_all(g, cams)


@pytest.mark.parametrize("V", [1, 32])
def test_view_batches(V):
    g, cams = raster_scene(30_000, 72, 40, seed=V, V=V)
    _render_all(g, cams)
