"""GPU: the 256-thread tile scatter counts its tiles with a per-wave 2-D difference grid (four corner adds per rectangle
into the wave's cursor row, two prefix passes) instead of walking every rectangle; everything behind the counts -- segment
starts, cursors, the point list, the image -- is as before.

Every case renders five views through rasterize_views (more than four views select the 256-thread scatter that scans its own
segments), once with lane-ordered LDS atomics and once with ballot ranking, and compares image (bit for bit), radii and
num_rendered of every view with oracle.capi.rasterize_forward.  The five views are the same central camera and the Gaussians
are flat discs facing it, with opacities of 0.6 and more: their alpha >= 1/255 level set reaches past the reference's 3 sigma
square, so the rectangles the device bins are the reference's and num_rendered is the oracle's count, not only a lower bound.

Cases: one tile; 2 x 3 and 3 x 2 tiles (an even and an odd number of tile columns take different prefix passes; an odd
number of tiles pads the cursor row); more than 64 tile rows under both passes and more than 64 word columns (a second round
of lanes); 640 x 480 with rectangles that end on the right and bottom tile edge (their far corners are left out of the grid)
and with Gaussians over the whole image; marker rectangles, among them far off-screen centres with huge radii; 2 048 and
2 049 Gaussians on one tile (512 per wave on one cell, -512 next to it; a second chunk of one entry); a first chunk of more
than 65 535 instances; a chunk past the staging block (written straight to memory)."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.gpu

TILE, CHUNK, V = 16, 2048, 5
TAN = math.tan(math.radians(30.0))
RIM = 0.3163  # sqrt(0.1) rounded up: what the reference's radius of a disc carries on top of sigma^2


def _discs(W, H, px, py, r3, op, seed):
    """Flat discs facing the central camera: centre (px, py) in pixels, 3 sigma = r3 pixels, Gaussian k of the arrays is the
    k-th nearest, and the reference's radius is ceil(r3) (r3 >= 2.5).  Ids are shuffled."""
    rng = np.random.default_rng(seed)
    n = len(px)
    px, py, r3 = (np.asarray(a, np.float64) for a in (px, py, r3))
    z = 1.5 + 1e-3 * np.arange(n)
    foc = W / (2.0 * TAN)
    # (the reference's larger eigenvalue of a disc is sigma^2 + sqrt(0.1), its floor under the root; 0.3 is the low-pass)
    s = np.sqrt((r3 / 3.0) ** 2 - RIM - 0.3) * z / foc
    means = np.stack([z * TAN * ((2 * px + 1) / W - 1), z * (TAN * H / W) * ((2 * py + 1) / H - 1), z], -1)
    perm = rng.permutation(n)
    g = dict(means3D=np.zeros((n, 3)), scales=np.zeros((n, 3)), rotations=np.zeros((n, 4)), opacities=np.zeros((n, 1)))
    g["means3D"][perm] = means
    g["scales"][perm] = np.stack([s, s, 1e-3 * s], -1)
    g["rotations"][:, 0] = 1.0
    g["opacities"][perm, 0] = np.broadcast_to(op, (n,))
    shs = rng.normal(0.0, 0.2, (n, 16, 3))
    shs[:, 0, :] = rng.normal(0.5, 0.5, (n, 3))
    g["shs"] = shs
    g = {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in g.items()}
    return g, dict(px=px, py=py, perm=perm)


def _ref_rects(W, H, info, radii):
    """(x0, y0, w, h) in tiles of the reference's square, nearest first, from the constructed centres and the oracle's radii."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rad = radii[info["perm"]].astype(np.float64)
    px, py = info["px"], info["py"]
    x0, x1 = np.clip(np.trunc((px - rad) / TILE), 0, gx), np.clip(np.trunc((px + rad + TILE - 1) / TILE), 0, gx)
    y0, y1 = np.clip(np.trunc((py - rad) / TILE), 0, gy), np.clip(np.trunc((py + rad + TILE - 1) / TILE), 0, gy)
    vis = rad > 0
    return np.stack([x0, y0, (x1 - x0) * vis, (y1 - y0) * vis], -1).astype(np.int64)


def _binned_as_the_reference(W, H, px, py, r3, op):
    """True where the rectangle the preprocess bins is certainly the reference's square.  The preprocess intersects the
    square (radius ceil(3 sigma)) with the box of the alpha >= 1/255 level set, half side sqrt(2 ln(255 opacity)) sigma and a
    little more, cut to whole pixels and tiles.  That cut only grows with the half side, so a box 0.3 px smaller than the
    real one that still covers the square's tiles settles it (a disc: sigma = r3 / 3 on both axes; where the preprocess does
    not tighten at all it bins the square anyway)."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rad = np.ceil(r3)
    half = np.sqrt(2.0 * np.log(255.0 * op) * ((r3 / 3.0) ** 2 - RIM)) - 0.3
    ok = np.ones(len(px), bool)
    live = np.ones(len(px), bool)
    for c, n in ((px, gx), (py, gy)):
        lo, hi = np.clip(np.trunc((c - rad) / TILE), 0, n), np.clip(np.trunc((c + rad + TILE - 1) / TILE), 0, n)
        tlo = np.maximum(lo, np.floor(np.ceil(c - half) / TILE))
        thi = np.maximum(np.minimum(hi, np.floor(np.floor(c + half) / TILE) + 1), tlo)
        ok &= (tlo == lo) & (thi == hi)
        live &= hi > lo
    return ok | ~live


def _mixed(W, H, n, seed, r_lo=2.5, r_hi=40.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-8, W + 8, n), rng.uniform(-8, H + 8, n), rng.uniform(r_lo, r_hi, n), rng.uniform(0.6, 0.95, n)


def _build(name):
    """-> (W, H, Gaussians, check(rects, gx, gy)): check asserts that the case holds what it is named for."""
    if name in ("16x16", "17x33", "47x31", "16x1040", "32x1040"):
        W, H = (int(t) for t in name.split("x"))
        px, py, r3, op = _mixed(W, H, 300 if name == "16x16" else 1000, 1, 2.5, 30.0)
        r3[::50] = 4.0 * max(W, H)  # some over the whole image

        def check(r, gx, gy):
            assert ((r[:, 2] == gx) & (r[:, 3] == gy)).any() and (r[:, 2] * r[:, 3] > 0).sum() > 200
    elif name == "640x480-edges":
        W, H = 640, 480
        px, py, r3, op = _mixed(W, H, 3000, 2)
        r3[:40] = 2000.0                                  # the whole image
        r3[40:400] = np.linspace(70.0, 160.0, 360)        # sides above 8 tiles
        px[400:700], py[700:1000] = W - 2.6, H - 2.6      # end on the right / bottom tile edge

        def check(r, gx, gy):
            live = r[:, 2] * r[:, 3] > 0
            assert ((r[:, 2] == gx) & (r[:, 3] == gy)).sum() >= 40
            assert (live & (r[:, 0] + r[:, 2] == gx) & (r[:, 2] < gx)).sum() >= 300
            assert (live & (r[:, 1] + r[:, 3] == gy) & (r[:, 3] < gy)).sum() >= 300
            assert (live & (r[:, 0] + r[:, 2] == gx) & (r[:, 1] + r[:, 3] == gy) & (r[:, 2] * r[:, 3] < gx * gy)).any()
            assert ((np.maximum(r[:, 2], r[:, 3]) > 8) & (r[:, 2] < gx)).sum() >= 300
    elif name == "2080x32-markers":
        W, H = 2080, 32  # 130 x 2 tiles: 65 word columns
        px, py, r3, op = _mixed(W, H, 600, 3)
        px[:20], r3[:20] = -1e5, 1e5 + np.linspace(1030.0, 2000.0, 20)   # far off screen, 65 tiles and more into the image
        px[20:40], r3[20:40] = W / 2, 3.0 * W                            # the whole image
        px[40:60], r3[40:60] = np.linspace(2040.0, 2075.0, 20), 12.0     # x0 past 126

        def check(r, gx, gy):
            live = r[:, 2] * r[:, 3] > 0
            assert (live & (r[:, 0] == 0) & (r[:, 2] > 63) & (r[:, 2] < gx)).sum() >= 10
            assert (r[:, 2] == gx).sum() >= 20 and (live & (r[:, 0] > 126)).sum() >= 10
    elif name.startswith("one-tile"):
        W, H, n = (int(t) for t in name.split("-")[2:])
        rng = np.random.default_rng(4)
        tx, ty = (W // TILE) // 2, (H // TILE) // 2
        px, py = TILE * tx + rng.uniform(5.0, 10.0, n), TILE * ty + rng.uniform(5.0, 10.0, n)
        r3, op = rng.uniform(2.5, 3.5, n), rng.uniform(0.6, 0.95, n)

        def check(r, gx, gy):
            assert (r == np.array([tx, ty, 1, 1])).all() and len(r) == n
    elif name == "big-chunk":
        W, H = 320, 240
        rng = np.random.default_rng(5)
        n = 2048 + 500
        px, py = rng.uniform(60.0, W - 60.0, n), rng.uniform(60.0, H - 60.0, n)
        r3, op = rng.uniform(50.0, 58.0, n), rng.uniform(0.6, 0.9, n)
        r3[2048:] = rng.uniform(2.5, 20.0, 500)

        def check(r, gx, gy):
            assert (r[:CHUNK, 2] * r[:CHUNK, 3] >= 33).all() and (r[:CHUNK, 2] * r[:CHUNK, 3]).sum() > 65535
    elif name == "past-staging":
        W, H = 640, 480
        px, py, r3, op = _mixed(W, H, 3000, 6, 16.0, 30.0)

        def check(r, gx, gy):
            first = int((r[:CHUNK, 2] * r[:CHUNK, 3]).sum())
            # six workgroups per CU share 160 KB of LDS: the staging block holds what the cursor rows leave of a sixth
            assert (160 * 1024 // 6 - 512 - 4 * gx * gy * 2) // 2 < first <= 65535, first
    else:
        raise KeyError(name)
    r3 = np.floor(r3) + 0.1 + 0.8 * (r3 - np.floor(r3))  # (the radius ceil(3 sigma) is not decided by rounding)
    op = np.where(_binned_as_the_reference(W, H, px, py, r3, op), op, 0.99)
    keep = _binned_as_the_reference(W, H, px, py, r3, op)
    px, py, r3, op = px[keep], py[keep], r3[keep], op[keep]
    g, info = _discs(W, H, px, py, r3, op, seed=len(name))
    return W, H, g, info, check


CASES = ["16x16", "17x33", "47x31", "16x1040", "32x1040", "640x480-edges", "2080x32-markers", "one-tile-64-48-2048",
         "one-tile-64-48-2049", "one-tile-48-48-2049", "big-chunk", "past-staging"]


@functools.lru_cache(maxsize=None)
def case(name):
    """The scene and the oracle's (image, radii, count); computed once, shared by both rankings, never written to."""
    from gaussreg_amd import synthetic
    from oracle import capi
    W, H, g, info, check = _build(name)
    cam = synthetic.camera(W, H)
    want = capi.rasterize_forward(g["means3D"], g["opacities"], shs=g["shs"], scales=g["scales"], rotations=g["rotations"],
                                  viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], campos=cam["campos"],
                                  bg=np.zeros(3, np.float32), W=W, H=H, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                  sh_degree=3)
    rects = _ref_rects(W, H, info, want[1])
    check(rects, (W + TILE - 1) // TILE, (H + TILE - 1) // TILE)
    assert want[2] > 0
    return W, H, g, cam, want


@pytest.mark.parametrize("ballot", [0, 1], ids=["lane-ordered", "ballot"])
@pytest.mark.parametrize("name", CASES)
def test_grid_counts_render_the_oracle_image(name, ballot):
    import torch
    from gaussreg_amd import _lib
    from gaussreg_amd.rasterizer import GaussianRasterizationSettings, rasterize_views
    W, H, g, cam, (wimg, wrad, wnr) = case(name)
    sets = [GaussianRasterizationSettings(H, W, cam["tanfovx"], cam["tanfovy"], torch.zeros(3, device="cuda"), 1.0,
                                          torch.from_numpy(cam["viewmatrix"]).cuda(), torch.from_numpy(cam["projmatrix"]).cuda(),
                                          3, torch.from_numpy(cam["campos"]).cuda(), False, False) for _ in range(V)]
    t = {k: torch.from_numpy(v).cuda() for k, v in g.items()}
    L = _lib.lib()
    old = L.gr_raster_ballot_ranking(ballot)
    try:
        img, radii, nr = rasterize_views(sets, t["means3D"], t["opacities"], shs=t["shs"], scales=t["scales"],
                                         rotations=t["rotations"])
        img, radii = img.cpu().numpy(), radii.cpu().numpy()
    finally:
        L.gr_raster_ballot_ranking(old)
    for v in range(V):
        assert int(nr[v]) == int(wnr), (v, int(nr[v]), int(wnr))
        assert np.array_equal(radii[v], wrad), v
        diff = int((img[v].view(np.uint32) != wimg.view(np.uint32)).sum())
        assert diff == 0, (v, diff)
