"""GPU: the tile binning output, word for word.

White box: after gr_raster_preprocess + gr_raster_render_ex on caller-owned buffers, the point list (bin buffer) and every row
of seg_off (geometry buffer) equal what numpy builds from the same frame's depth order, rectangles and visible counts
(gr_raster_debug_geom_layout): chunk-major, tiles in order inside a chunk, depth order inside every (chunk, tile) segment.
Covers the few-view path (count + scan launches), the many-view path (chunk totals only, the scatter scans its own segments),
the deferred frames of gr_raster_forward (the scatter that scans behind the bucket depth sort; with GR_NO_MAILBOX=1 the counts
that come back behind an event), chunk rows too long for one scan launch (more than 2 048 x 2 048 Gaussians), empty views,
partial chunks, rectangles up to and past 8 tiles a side, marker rectangles, chunks past the staging block and chunks of more
than 65 535 instances -- each with the lane-ordered LDS atomics and with ballot ranking."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.gpu

TILE, CHUNK, MARKER = 16, 2048, 127 | (127 << 7)


def _align(x, a=256):
    return (x + a - 1) // a * a


def _settings(cam):
    from gaussreg_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=cam["image_height"], image_width=cam["image_width"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.zeros(3, dtype=torch.float32, device="cuda"), scale_modifier=1.0,
        viewmatrix=torch.from_numpy(cam["viewmatrix"]).cuda(), projmatrix=torch.from_numpy(cam["projmatrix"]).cuda(),
        sh_degree=3, campos=torch.from_numpy(cam["campos"]).cuda(), prefiltered=False, debug=False)


def _scene(P, seed, grow):
    from gaussreg_amd import synthetic
    g = synthetic.gaussians_c2(P, seed=seed, sh_degree=3)
    if grow:
        g["scales"] = (g["scales"] + np.float32(grow)).astype(np.float32)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in g.items()}


def _cams(V, W, H, seed, empty):
    from gaussreg_amd import synthetic
    cams = synthetic.camera_ring(V, W, H, seed=seed)
    for v in empty:  # looking away from the scene: nothing visible
        cams[v] = synthetic.camera(W, H, R_c2w=synthetic.rot_yx(math.pi, 0.0))
    return [_settings(c) for c in cams]


def _expected(gh, off, P, V, W, H):
    """numpy: the point list and seg_off of one frame from its depth order / rectangles / visible counts."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tiles, nchunk = gx * gy, (P + CHUNK - 1) // CHUNK
    rec = gh[: 64 * P * V].view(np.float32).reshape(V, P, 4, 4)  # (the records come first in the geometry buffer)
    order = gh[off[1]: off[1] + 4 * V * P].view(np.int32).reshape(V, P)
    rects = gh[off[2]: off[2] + 4 * V * P].view(np.uint32).reshape(V, P)
    nvis = gh[off[3]: off[3] + 4 * V].view(np.int32)
    base, lists, segs, markers = 0, [], np.zeros((V, nchunk, tiles + 1), np.int64), 0
    for v in range(V):
        n = int(nvis[v])
        ids, r = order[v, :n].astype(np.int64), rects[v, :n].astype(np.int64)
        x0, y0, w, h = r & 127, (r >> 7) & 127, (r >> 14) & 63, (r >> 20) & 63
        m = r == MARKER
        markers += int(m.sum())
        if m.any():  # rebuilt from the record as get_rect does (fp32, truncation, clamp)
            px, py = rec[v, ids[m], 0, 0], rec[v, ids[m], 0, 1]
            rad = rec[v, ids[m], 3, 0].view(np.int32).astype(np.float32)
            t16, t15 = np.float32(TILE), np.float32(TILE - 1)
            lo_x = np.clip(((px - rad) / t16).astype(np.int64), 0, gx)
            lo_y = np.clip(((py - rad) / t16).astype(np.int64), 0, gy)
            hi_x = np.clip(((px + rad + t15) / t16).astype(np.int64), 0, gx)
            hi_y = np.clip(((py + rad + t15) / t16).astype(np.int64), 0, gy)
            x0[m], y0[m], w[m], h[m] = lo_x, lo_y, hi_x - lo_x, hi_y - lo_y
        cnt = w * h
        tot = int(cnt.sum())
        t = np.repeat(np.arange(n), cnt)
        k = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        tile = (y0[t] + k // w[t]) * gx + x0[t] + k % w[t]
        ck = t // CHUNK
        lists.append(ids[t[np.argsort((ck * tiles + tile) * CHUNK + t % CHUNK, kind="stable")]])
        start = np.concatenate([[0], np.cumsum(np.bincount(ck * tiles + tile, minlength=nchunk * tiles))])
        segs[v, :, :tiles] = base + start[:-1].reshape(nchunk, tiles)
        segs[v, :, tiles] = base + start[tiles::tiles]
        base += tot
    return np.concatenate(lists) if lists else np.zeros(0, np.int64), segs, base, markers


def _chunk_peak(segs):
    return int((segs[:, :, -1] - segs[:, :, 0]).max()) if segs.size else 0


def _check_frame(L, geom, binb, P, V, W, H, nr, min_visible=None):
    off = (ctypes.c_int64 * 4)()
    assert L.gr_raster_debug_geom_layout(P, V, W, H, off) == 4
    torch.cuda.synchronize()
    gh = geom.cpu().numpy()
    if min_visible is not None:  # every view's depth order is longer than this
        assert int(gh[off[3]: off[3] + 4 * V].view(np.int32).min()) > min_visible
    want_pl, want_seg, R, markers = _expected(gh, off, P, V, W, H)
    assert [int(nr[v]) for v in range(V)] == [int(want_seg[v, -1, -1] - want_seg[v, 0, 0]) for v in range(V)]
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tiles, nchunk = gx * gy, (P + CHUNK - 1) // CHUNK
    # seg_off follows the rectangles and the chunk tile counts in the geometry buffer (carve_geom, 256-byte aligned)
    seg_at = _align(_align(off[2] + 4 * V * P) + 2 * V * nchunk * tiles)
    got_seg = gh[seg_at: seg_at + 4 * V * nchunk * (tiles + 1)].view(np.uint32).reshape(V, nchunk, tiles + 1)
    assert np.array_equal(got_seg.astype(np.int64), want_seg)
    got_pl = binb[: 4 * R].cpu().numpy().view(np.int32)
    assert np.array_equal(got_pl.astype(np.int64), want_pl)
    return R, markers, _chunk_peak(want_seg)


def _run_plain(P, W, H, V, seed, grow, empty, scene=None, min_visible=None):
    from gaussreg_amd import _lib
    from gaussreg_amd.rasterizer import ViewBatch
    L = _lib.lib()
    t = scene if scene is not None else _scene(P, seed, grow)
    vb = ViewBatch(_cams(V, W, H, seed, empty))
    st = _lib.stream_ptr(torch.device("cuda"))
    gbytes = L.gr_raster_geom_bytes(P, V, W, H)
    geom = torch.zeros(gbytes, dtype=torch.uint8, device="cuda")
    radii = torch.empty((V, P), dtype=torch.int32, device="cuda")
    color = torch.empty((V, 3, H, W), dtype=torch.float32, device="cuda")
    nr = (ctypes.c_int64 * (V + 1))()
    _lib.check(L.gr_raster_preprocess(P, 16, _lib.ptr(t["means3D"]), _lib.ptr(t["shs"]), None, _lib.ptr(t["opacities"]),
                                      _lib.ptr(t["scales"]), _lib.ptr(t["rotations"]), None, vb.array, V, _lib.ptr(radii),
                                      _lib.ptr(geom), gbytes, nr, st))
    total = sum(int(nr[v]) for v in range(V))
    bbytes = L.gr_raster_bin_bytes(total, W, H, V)
    binb = torch.full((bbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    _lib.check(L.gr_raster_render_ex(P, vb.array, V, nr, _lib.ptr(geom), gbytes, _lib.ptr(binb), bbytes, _lib.ptr(color), 0,
                                     st))
    return _check_frame(L, geom, binb, P, V, W, H, nr, min_visible)


def _run_deferred(P, W, H, V, seed, grow, frames=5, scene=None, last_only=False, bin_bytes=64 << 20, min_visible=None):
    """gr_raster_forward on one buffer set: the first frames of a process are plain (checked), the later ones deferred (a few
    views per call).  last_only: compare the last frame alone (a deferred one all the same)."""
    from gaussreg_amd import _lib
    from gaussreg_amd.rasterizer import ViewBatch
    L = _lib.lib()
    t = scene if scene is not None else _scene(P, seed, grow)
    vb = ViewBatch(_cams(V, W, H, seed, ()))
    st = _lib.stream_ptr(torch.device("cuda"))
    gbytes = L.gr_raster_geom_bytes(P, V, W, H)
    geom = torch.zeros(gbytes, dtype=torch.uint8, device="cuda")
    radii = torch.empty((V, P), dtype=torch.int32, device="cuda")
    color = torch.empty((V, 3, H, W), dtype=torch.float32, device="cuda")
    binb = torch.empty(bin_bytes, dtype=torch.uint8, device="cuda")
    nr = (ctypes.c_int64 * (V + 1))()
    for f in range(frames):
        rc = L.gr_raster_forward(P, 16, _lib.ptr(t["means3D"]), _lib.ptr(t["shs"]), None, _lib.ptr(t["opacities"]),
                                 _lib.ptr(t["scales"]), _lib.ptr(t["rotations"]), None, vb.array, V, _lib.ptr(radii),
                                 _lib.ptr(geom), gbytes, _lib.ptr(binb), binb.numel(), _lib.ptr(color), 0, nr, st)
        _lib.check(rc)
        if f == frames - 1 or not last_only:
            out = _check_frame(L, geom, binb, P, V, W, H, nr, min_visible)
    return out


# (P, W, H, V, seed, scale growth, empty views): P not a multiple of 64 or of 2 048 throughout
CASES = [
    (20011, 640, 480, 1, 1, 0.0, ()),
    (30001, 640, 480, 3, 2, 0.0, (1,)),
    (9001, 640, 480, 8, 3, 0.0, (0, 5)),
    (12347, 640, 480, 32, 4, 0.0, (7,)),
    (6007, 640, 480, 8, 5, 0.05, ()),       # rectangles of 3 .. 8 and more tiles a side; chunks past the staging block
    (4099, 320, 240, 3, 6, 1.5, ()),        # rectangles of the whole image: chunks of more than 65 535 instances
    (4099, 320, 240, 8, 6, 1.5, (2,)),
    (3001, 2048, 128, 3, 7, 1.0, ()),       # 128 tiles wide: rectangles past 63 tiles / x0 past 126 (marker rectangles)
    (3001, 2048, 128, 8, 7, 1.0, ()),
]


def _ids(c):
    return "P%d-%dx%d-V%d-g%g" % (c[0], c[1], c[2], c[3], c[5])


@pytest.mark.parametrize("ballot", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=[_ids(c) for c in CASES])
def test_binning_matches_numpy_word_for_word(case, ballot):
    from gaussreg_amd import _lib
    L = _lib.lib()
    old = L.gr_raster_ballot_ranking(ballot)
    try:
        P, W, H, V, seed, grow, empty = case
        R, markers, peak = _run_plain(P, W, H, V, seed, grow, empty)
        assert R > 0
        if W == 2048:
            assert markers > 0
        if grow >= 1.5:
            assert peak > 65535
        if grow == 0.05:
            assert peak > 8192  # more than the many-view staging block holds
    finally:
        L.gr_raster_ballot_ranking(old if old in (0, 1) else 0)


@pytest.mark.parametrize("ballot", [0, 1])
@pytest.mark.parametrize("case", [(20011, 640, 480, 1, 1, 0.0), (30001, 640, 480, 3, 2, 0.02), (4099, 320, 240, 2, 6, 1.5)],
                         ids=["V1", "V3", "V2-big"])
def test_deferred_frames_bin_word_for_word(case, ballot):
    from gaussreg_amd import _lib
    L = _lib.lib()
    old = L.gr_raster_ballot_ranking(ballot)
    try:
        _run_deferred(*case)
    finally:
        L.gr_raster_ballot_ranking(old if old in (0, 1) else 0)


# Chunk rows too long for one scan launch: 2 050 chunks (neither a multiple of 64 nor of 2 048) -- chunk_max_kernel, the
# multi-launch exclusive_scan_i32 and the chunk maximum that travels in a word of its own.
LONG_P = 2048 * 2048 + 2049
LONG_W, LONG_H = 64, 64  # 16 tiles: the numpy side stays small


def _long_scene(V, seed):
    """LONG_P Gaussians that are visible in every one of the V views: a small scene is projected once, the Gaussians with a
    radius in every view are kept and repeated on the device.  Copies have equal depths: ties go by id, the documented rule."""
    from gaussreg_amd import _lib
    from gaussreg_amd.rasterizer import ViewBatch
    L = _lib.lib()
    P0 = 20011
    t = _scene(P0, seed, 0.0)
    vb = ViewBatch(_cams(V, LONG_W, LONG_H, seed, ()))
    gbytes = L.gr_raster_geom_bytes(P0, V, LONG_W, LONG_H)
    geom = torch.zeros(gbytes, dtype=torch.uint8, device="cuda")
    radii = torch.empty((V, P0), dtype=torch.int32, device="cuda")
    nr = (ctypes.c_int64 * (V + 1))()
    _lib.check(L.gr_raster_preprocess(P0, 16, _lib.ptr(t["means3D"]), _lib.ptr(t["shs"]), None, _lib.ptr(t["opacities"]),
                                      _lib.ptr(t["scales"]), _lib.ptr(t["rotations"]), None, vb.array, V, _lib.ptr(radii),
                                      _lib.ptr(geom), gbytes, nr, _lib.stream_ptr(torch.device("cuda"))))
    keep = (radii > 0).all(dim=0)
    n = int(keep.sum())
    assert n > 1000
    reps = (LONG_P + n - 1) // n
    return {k: v[keep].repeat((reps,) + (1,) * (v.dim() - 1))[:LONG_P].contiguous() for k, v in t.items()}


@pytest.mark.parametrize("ballot", [0, 1])
def test_long_chunk_rows_plain_one_view(ballot):
    from gaussreg_amd import _lib
    L = _lib.lib()
    old = L.gr_raster_ballot_ranking(ballot)
    try:
        R, _, _ = _run_plain(LONG_P, LONG_W, LONG_H, 1, 8, 0.0, (), scene=_long_scene(1, 8), min_visible=2048 * 2048)
        assert R > 2048 * 2048
    finally:
        L.gr_raster_ballot_ranking(old if old in (0, 1) else 0)


@pytest.mark.parametrize("ballot", [0, 1])
def test_long_chunk_rows_deferred_two_views(ballot):
    """The fifth frame of the process at the latest is a deferred one: its counts come back behind an event (rows this long
    are not mailed), the chunk maximum in the last word."""
    from gaussreg_amd import _lib
    L = _lib.lib()
    old = L.gr_raster_ballot_ranking(ballot)
    try:
        R, _, _ = _run_deferred(LONG_P, LONG_W, LONG_H, 2, 9, 0.0, scene=_long_scene(2, 9), last_only=True, bin_bytes=256 << 20,
                                min_visible=2048 * 2048)
        assert R > 2 * 2048 * 2048
    finally:
        L.gr_raster_ballot_ranking(old if old in (0, 1) else 0)


@pytest.mark.parametrize("ballot", [0, 1])
def test_deferred_frames_counts_by_event(ballot):
    """GR_NO_MAILBOX=1 (read once per process, so in a child process): the counts of a deferred frame come back by a copy on
    a side stream and an event; with GR_RASTER_BALLOT_RANKING=1 beside it every frame of the process is a deferred one."""
    env = dict(os.environ, GR_NO_MAILBOX="1")
    if ballot:
        env["GR_RASTER_BALLOT_RANKING"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "event"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "event path compared" in r.stdout


def test_every_frame_verified_on_the_device():
    """GR_RASTER_VERIFY=1 (set before the library loads, so in a child process): the on-device list check runs on every frame."""
    env = dict(os.environ, GR_RASTER_VERIFY="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "verify"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "verified" in r.stdout


if __name__ == "__main__" and sys.argv[1:] == ["verify"]:
    for c in (CASES[2], CASES[3], CASES[4], CASES[6], CASES[8]):
        _run_plain(*c)
    _run_deferred(30001, 640, 480, 3, 2, 0.02)
    print("verified")

if __name__ == "__main__" and sys.argv[1:] == ["event"]:
    assert os.environ.get("GR_NO_MAILBOX") == "1"
    _run_deferred(20011, 640, 480, 1, 1, 0.0)
    _run_deferred(30001, 640, 480, 3, 2, 0.02)
    print("event path compared")
