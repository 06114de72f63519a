"""GPU: the bucket depth sort of calls of MORE than four views (depth_sort.hip: per-wave key ranges of preprocess_many_kernel
reduced by ds_range_kernel, top-digit pass, buckets in two size classes with the XCD-affine mapping from eight views on, chunk
totals out of the bucket launch instead of chunk_total_kernel).

White box: the order a frame leaves in the geometry buffer (gr_raster_debug_geom_layout) -- ids, rectangles, visible counts --
equals the one of the three-pass sort (pinned through gr_raster_debug_bucket_cooldown(1 << 20)) bit for bit, and equals
numpy's stable sort of (depth field, id).  Black box: images and radii of the two are equal bit for bit.
Shapes: the smallest that reach every branch (view counts around the group of eight of the XCD mapping, Gaussian counts around
the 2 048-entry chunk, buckets around the two caps)."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL_CAP, LARGE_CAP, BINS = 4032, 7936, 512  # depth_sort.hip: MANY_CAP, MSD_CAP, DS_BINS
W, H = 64, 48
_bin = {}


def _cams(V, away=()):
    from gaussreg_amd import synthetic
    cams = synthetic.camera_ring(V, W, H, seed=3)
    for v in away:  # looks down -z: nothing of the scene in front of it
        cams[v] = synthetic.camera(W, H, R_c2w=synthetic.rot_yx(math.pi, 0.0))
    return cams


def _frame(g, cams, pinned):
    """One gr_raster_forward call of len(cams) views on a caller-owned geometry buffer; pinned: the three-pass sort."""
    from gaussreg_amd import _lib
    from gaussreg_amd.rasterizer import GaussianRasterizationSettings, ViewBatch
    L = _lib.lib()
    V, P = len(cams), g["means3D"].shape[0]
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in g.items()}
    sets = [GaussianRasterizationSettings(H, W, c["tanfovx"], c["tanfovy"], torch.zeros(3), 1.0, torch.from_numpy(c["viewmatrix"]),
                                          torch.from_numpy(c["projmatrix"]), 3, torch.from_numpy(c["campos"]), False, False)
            for c in cams]
    gbytes = L.gr_raster_geom_bytes(P, V, W, H)
    off = (ctypes.c_int64 * 4)()
    assert L.gr_raster_debug_geom_layout(P, V, W, H, off) == 4
    geom = torch.zeros(gbytes + 256, dtype=torch.uint8, device="cuda")
    if "b" not in _bin:
        _bin["b"] = torch.empty(1 << 27, dtype=torch.uint8, device="cuda")
    binb = _bin["b"]
    color = torch.empty((V, 3, H, W), dtype=torch.float32, device="cuda")
    radii = torch.empty((V, P), dtype=torch.int32, device="cuda")
    nr = (ctypes.c_int64 * (V + 1))()
    vb = ViewBatch(sets)
    L.gr_raster_debug_bucket_cooldown(1 << 20 if pinned else 0)
    try:
        rc = L.gr_raster_forward(P, 16, _lib.ptr(t["means3D"]), _lib.ptr(t["shs"]), None, _lib.ptr(t["opacities"]),
                                 _lib.ptr(t["scales"]), _lib.ptr(t["rotations"]), None, vb.array, V, _lib.ptr(radii),
                                 _lib.ptr(geom), gbytes, _lib.ptr(binb), binb.numel(), _lib.ptr(color), 0, nr,
                                 _lib.stream_ptr(torch.device("cuda")))
        torch.cuda.synchronize()
        left = L.gr_raster_debug_bucket_cooldown(-1)
    finally:
        L.gr_raster_debug_bucket_cooldown(0)
    assert rc == 0, rc
    gh = geom.cpu().numpy()
    return dict(field=gh[off[0]: off[0] + 4 * V * P].view(np.uint32).reshape(V, P).copy(),
                order=gh[off[1]: off[1] + 4 * V * P].view(np.int32).reshape(V, P).copy(),
                rects=gh[off[2]: off[2] + 4 * V * P].view(np.uint32).reshape(V, P).copy(),
                nvis=gh[off[3]: off[3] + 4 * V].view(np.int32).copy(), color=color.cpu().numpy(), radii=radii.cpu().numpy(),
                rendered=[int(nr[v]) for v in range(V)], cooldown=left)


def _largest_bucket(field_row):
    """the largest bucket of the top-digit pass of one view, as ds_range_kernel and the scatter cut them"""
    f = field_row[field_row != 0].astype(np.int64)
    if f.size == 0:
        return 0, 0
    span = int(f.max() - f.min())
    shift = max(0, span.bit_length() - 9) if span else 0
    return int(np.bincount((f - f.min()) >> shift, minlength=BINS).max()), shift


def _check(g, cams, expect_cooldown=0):
    """bucket path against the three-pass sort and against numpy; returns the bucket-path frame"""
    got, want = _frame(g, cams, pinned=False), _frame(g, cams, pinned=True)
    V = len(cams)
    assert want["cooldown"] == (1 << 20) - 1  # the call COULD have taken the bucket sort: it ran the waiting period down
    assert got["cooldown"] == expect_cooldown
    assert np.array_equal(got["field"], want["field"])
    assert np.array_equal(got["nvis"], want["nvis"])
    assert got["rendered"] == want["rendered"]
    for v in range(V):
        n = int(got["nvis"][v])
        vis = np.flatnonzero(got["field"][v])
        assert n == vis.size, (v, n, vis.size)
        ref = vis[np.argsort(got["field"][v][vis], kind="stable")]
        assert np.array_equal(got["order"][v, :n], ref), f"view {v}: not the stable (field, id) order"
        assert np.array_equal(got["order"][v, :n], want["order"][v, :n]), f"view {v}: ids"
        assert np.array_equal(got["rects"][v, :n], want["rects"][v, :n]), f"view {v}: rectangles"
    assert np.array_equal(got["color"].view(np.uint32), want["color"].view(np.uint32))
    assert np.array_equal(got["radii"], want["radii"])
    return got


@pytest.mark.parametrize("V", [5, 8, 9, 33])
@pytest.mark.parametrize("P", [1, 63, 2047, 2049, 40000])
def test_many_views_equal_the_three_pass_sort_and_numpy(V, P):
    from gaussreg_amd import synthetic
    got = _check(synthetic.gaussians_c2(P, seed=P % 7, sh_degree=3), _cams(V))
    if P >= 2047:
        assert got["nvis"].max() > 0


def test_a_view_with_nothing_visible():
    from gaussreg_amd import synthetic
    got = _check(synthetic.gaussians_c2(5000, seed=1, sh_degree=3), _cams(9, away=(2, 8)))
    assert got["nvis"][2] == 0 and got["nvis"][8] == 0 and got["nvis"][0] > 1000
    assert not got["color"][2].any()


def _slab(P, n_slab, depth0, width, seed):
    """n_slab Gaussians inside `width` of depth at depth0 plus one very near and one far: the key range is wide, so the slab
    lands in one bucket; the others spread over the box as usual"""
    from gaussreg_amd import synthetic
    rng = np.random.default_rng(seed)
    g = synthetic.gaussians_c2(P, seed=seed, sh_degree=3)
    m = g["means3D"]
    m[:n_slab, 0] = (rng.random(n_slab) - 0.5) * 2.0
    m[:n_slab, 1] = (rng.random(n_slab) - 0.5) * 1.4
    m[:n_slab, 2] = depth0 + rng.random(n_slab) * width
    m[n_slab] = (0.0, 0.0, 0.3)
    m[n_slab + 1] = (0.3, 0.3, 60.0)
    g["means3D"] = m.astype(np.float32)
    return g


def _same_camera(V):
    from gaussreg_amd import synthetic
    return [synthetic.camera(W, H) for _ in range(V)]


def test_all_depths_equal_span_zero_ties_by_id():
    from gaussreg_amd import synthetic
    P = 12000  # one bucket of every view holds everything: above both caps, no overflow (id order is the order)
    rng = np.random.default_rng(4)
    g = synthetic.gaussians_c2(P, seed=8, sh_degree=3)
    g["means3D"][:, 0] = (rng.random(P) - 0.5) * 2.0
    g["means3D"][:, 1] = (rng.random(P) - 0.5) * 1.4
    g["means3D"][:, 2] = 2.5
    g["means3D"] = g["means3D"].astype(np.float32)
    got = _check(g, _same_camera(9))
    for v in range(9):
        n, shift = _largest_bucket(got["field"][v])
        assert shift == 0 and n == got["nvis"][v] and n > LARGE_CAP
        assert np.array_equal(got["order"][v, :n], np.sort(got["order"][v, :n]))


def test_a_bucket_above_the_small_cap_takes_the_listed_class():
    g = _slab(9000, 6000, 3.0, 0.002, seed=12)
    got = _check(g, _same_camera(5) + _cams(4))
    n, shift = _largest_bucket(got["field"][0])
    assert SMALL_CAP < n <= LARGE_CAP and shift > 0, (n, shift)


def test_a_bucket_above_the_large_cap_falls_back_and_the_cooldown_is_kept_then_cleared():
    from gaussreg_amd import _lib, synthetic
    L = _lib.lib()
    g = _slab(24000, 20000, 3.0, 0.002, seed=13)
    cams = _same_camera(3) + _cams(6)
    got = _check(g, cams, expect_cooldown=256)  # the overflow was seen: three passes for this frame and for a while
    n, shift = _largest_bucket(got["field"][0])
    assert n > LARGE_CAP and shift > 0, (n, shift)
    # inside the period a call takes the three-pass sort and runs the period down by one
    L.gr_raster_debug_bucket_cooldown(256)
    from gaussreg_amd.rasterizer import rasterize_views, GaussianRasterizationSettings
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in g.items()}
    sets = [GaussianRasterizationSettings(H, W, c["tanfovx"], c["tanfovy"], torch.zeros(3, device="cuda"), 1.0,
                                          torch.from_numpy(c["viewmatrix"]).cuda(), torch.from_numpy(c["projmatrix"]).cuda(), 3,
                                          torch.from_numpy(c["campos"]).cuda(), False, False) for c in cams]
    color, radii, _ = rasterize_views(sets, t["means3D"], t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    assert np.array_equal(color.cpu().numpy().view(np.uint32), got["color"].view(np.uint32))
    assert np.array_equal(radii.cpu().numpy(), got["radii"])
    assert L.gr_raster_debug_bucket_cooldown(0) == 255
    # cleared: a scene that fits takes the bucket sort again and leaves no period behind
    _check(synthetic.gaussians_c2(3000, seed=3, sh_degree=3), cams)
    assert L.gr_raster_debug_bucket_cooldown(-1) == 0


def test_a_depth_beyond_the_compact_keys_takes_the_full_key_path():
    from gaussreg_amd import synthetic
    g = synthetic.gaussians_c2(5000, seed=5, sh_degree=3)
    g["means3D"][7] = (0.0, 0.0, 9000.0)   # >= 8192: the far flag, the call orders again on all 32 depth bits
    g["means3D"][11] = (0.1, 0.1, 20000.0)
    got = _check(g, _cams(9))
    assert int(got["field"].max()) >= np.float32(8192.0).view(np.uint32)  # the fields are the full depth bits now
    assert got["radii"][0, 7] > 0


def test_ballot_ranking_on_the_many_view_path():
    from gaussreg_amd import _lib, synthetic
    L = _lib.lib()
    old = L.gr_raster_ballot_ranking(1)
    try:
        assert L.gr_raster_lds_atomics_lane_ordered() == 0
        _check(synthetic.gaussians_c2(2049, seed=2, sh_degree=3), _cams(9))
        got = _check(_slab(9000, 6000, 3.0, 0.002, seed=12), _same_camera(5))
        assert _largest_bucket(got["field"][0])[0] > SMALL_CAP
    finally:
        L.gr_raster_ballot_ranking(old)
