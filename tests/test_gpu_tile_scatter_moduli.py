"""GPU: the tile scatter's residue-class walk with the exact per-axis moduli (Mx = largest width, My = largest height of a
64-Gaussian step), on a constructed scene.

A 176 x 144 image (11 x 9 tiles: an odd row of tiles, so the cursor row is padded and two tiles share an LDS word) and
3 000 flat, camera-facing Gaussians whose tile rectangles in the first camera are chosen one by one: every 64 depth-consecutive
Gaussians form one step of the walk, and the steps are built so that the (largest width, largest height) pairs (1,1), (2,3),
(3,2), (3,3), (4,3), (5,5), (7,6), (8,8) and more occur, one step holds a side of more than 8 tiles, one step takes its largest
width and its largest height from different lanes, one step puts all its Gaussians on the same tile at the same depth, and
rectangles start in every residue modulo 3, 5, 6 and 7 and touch or cross all four image borders.  The test reads the
rectangles back from the device and asserts that all of this is really there.

Checked per view against oracle.capi.rasterize_forward: the image bit for bit, radii, and the instance count -- equal to the
oracle's in the first camera, where the scene is built so that the level-set tightening of the rectangles drops nothing; the
other four cameras of the five-view case see the scene from elsewhere, there the count is the library's documented "at most
the reference's" and equals the sum of the rectangles the device reports.  One camera runs the 1 024-thread scatter, five
cameras the 256-thread one that scans its own segments, each with lane-ordered LDS atomics and with ballot ranking.  In the
five-view case the first chunk (32 steps, the large rectangles) is larger than any staging block and goes straight to memory;
the second one and the 300-Gaussian case are staged.  A child process repeats every case under GR_RASTER_VERIFY=1, where the
device-side check of every (chunk, tile) list runs on every frame."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

pytestmark = pytest.mark.gpu

W, H, TILE, CHUNK, STEP = 176, 144, 16, 2048, 64
GX, GY = W // TILE, H // TILE
P_FULL, P_SMALL = 3000, 300
REQUIRED = [(1, 1), (2, 3), (3, 2), (3, 3), (4, 3), (5, 5), (7, 6), (8, 8)]
EXTRA = [(6, 6), (2, 2), (4, 4), (1, 2), (5, 4), (6, 7), (3, 4), (8, 7), (2, 1), (5, 6)]
# the largest staging block the many-view scatter can have, in instances (six workgroups per CU share 160 KB of LDS)
STAGE_MAX = (160 * 1024 // 6 - 512) // 2


def _model_rects(px, py, s, z, op):
    """fp32 numpy model of the rectangle the reference computes (the square of radius ceil(3 sigma)) and of the tightened one
    the preprocess emits, for flat Gaussians (scales s, s, 1e-3 s; identity rotation) seen by the central camera.  Returns
    (ref, tight), each (x0, y0, x1, y1) in tiles, and a flag: no decision of the model is close to flipping."""
    f32 = np.float32
    foc = f32(W / (2.0 * math.tan(math.radians(30.0))))
    tanx = f32(math.tan(math.radians(30.0)))
    tany = f32(tanx * H / W)
    x = z * tanx * ((2 * px + 1) / f32(W) - 1)
    y = z * tany * ((2 * py + 1) / f32(H) - 1)
    sz2 = (f32(1e-3) * s) ** 2
    jx, jy = foc * x / (z * z), foc * y / (z * z)
    a = (foc / z) ** 2 * s * s + jx * jx * sz2 + f32(0.3)
    c = (foc / z) ** 2 * s * s + jy * jy * sz2 + f32(0.3)
    b = jx * jy * sz2
    det, mid = a * c - b * b, f32(0.5) * (a + c)
    root = np.sqrt(np.maximum(f32(0.1), mid * mid - det))
    l1, l2 = mid + root, mid - root
    r3 = f32(3.0) * np.sqrt(np.maximum(l1, l2))
    rad = np.ceil(r3)
    firm = np.abs(r3 - np.round(r3)) > 0.03

    def span(lo_px, hi_px, n):  # (int) casts truncate; the clamp to [0, n] makes that a floor where it matters
        return np.clip(np.trunc(lo_px / TILE), 0, n), np.clip(np.trunc(hi_px / TILE), 0, n)
    rx0, rx1 = span(px - rad, px + rad + (TILE - 1), GX)
    ry0, ry1 = span(py - rad, py + rad + (TILE - 1), GY)
    pcm = np.log(f32(255.0) * op) + f32(2e-3)
    kc = f32(1.001) / (f32(0.5) / l1 - f32(2e-6))
    cp = pcm + f32(2e-6) * (pcm * kc)
    out = []
    for dh in (0.0, -0.25, 0.25):
        hx = np.sqrt(2 * cp * a) * f32(1.001) + f32(1e-2) + f32(dh)
        hy = np.sqrt(2 * cp * c) * f32(1.001) + f32(1e-2) + f32(dh)
        tx0 = np.maximum(rx0, np.floor(np.ceil(px - hx) / TILE))
        ty0 = np.maximum(ry0, np.floor(np.ceil(py - hy) / TILE))
        tx1 = np.maximum(np.minimum(rx1, np.floor(np.floor(px + hx) / TILE) + 1), tx0)
        ty1 = np.maximum(np.minimum(ry1, np.floor(np.floor(py + hy) / TILE) + 1), ty0)
        out.append(np.stack([tx0, ty0, tx1, ty1], -1))
    # the reference's own boundaries: a tile edge within 0.05 px of px -+ rad would make the fp32 division decide
    for e in (px - rad, px + rad + (TILE - 1), py - rad, py + rad + (TILE - 1)):
        fr = e / TILE - np.floor(e / TILE)
        firm &= (fr > 0.004) & (fr < 0.996)
    firm &= (out[0] == out[1]).all(-1) & (out[0] == out[2]).all(-1) & (l2 >= 0.35) & (det > 0)
    return np.stack([rx0, ry0, rx1, ry1], -1), out[0], firm


def _step_specs(rng):
    """Per step the 64 wanted rectangles (X0, Y0, w, h) in tiles, before clamping to the image, and whether the step's
    Gaussians share one depth."""
    def place(w, h, inside):
        lx = 0 if inside or w < 2 else -1  # (one tile may hang out of the image; a one-tile side stays inside: all visible)
        ly = 0 if inside or h < 2 else -1
        return (int(rng.integers(lx, GX - w + 1 - lx)), int(rng.integers(ly, GY - h + 1 - ly)), w, h)

    def plain(mw, mh):
        lanes = [place(mw, mh, True), place(mw, mh, True)]  # the largest shape, unclamped, twice
        while len(lanes) < STEP:
            w = int(rng.integers(max(1, mw - 2), mw + 1))
            h = int(np.clip(w + rng.integers(-1, 2), max(1, mh - 2), mh))
            if abs(w - h) > 1:
                w = h + (1 if w > h else -1)
            lanes.append(place(min(w, mw), h, False))
        return lanes
    specs = [(plain(*s), False) for s in REQUIRED]
    big = plain(3, 3)
    big[5] = (1, 0, 10, 9)  # a side of more than 8 tiles: the step is walked one Gaussian at a time
    big[40] = (0, 0, 9, 9)
    specs.append((big, False))
    split = [place(3, 2, True) if i % 3 == 0 else place(2, 3, True) if i % 3 == 1 else place(2, 2, False)
             for i in range(STEP)]  # Mx = 3 from one lane, My = 3 from another, no 3 x 3 rectangle in the step
    specs.append((split, False))
    same = [(int(rng.integers(3, 6)), int(rng.integers(2, 5)), 3, 3) for _ in range(STEP)]  # all contain tile (5, 4)
    specs.append((same, True))
    for i, s in enumerate(EXTRA + REQUIRED):
        specs.append((plain(*s), i % 4 == 1))
    # the tail (the second chunk and the 300-Gaussian case, which starts here): small shapes, a staged chunk
    tail = [(3, 3), (2, 3), (3, 2), (1, 1), (2, 2), (3, 3), (4, 3), (2, 3), (1, 2), (3, 3), (2, 2), (3, 2), (2, 1), (3, 3),
            (1, 1), (2, 2), (3, 2), (3, 3)]
    for i, s in enumerate(tail):
        specs.append((plain(*s), i % 5 == 2))
    assert len(specs) == (P_FULL + STEP - 1) // STEP
    return specs


@functools.lru_cache(maxsize=None)
def scene():
    """The constructed scene (numpy, fp32), the same on every call: Gaussian k of the depth order gets id perm[k]."""
    rng = np.random.default_rng(20240610)
    specs = _step_specs(rng)
    want, z = [], []
    for si, (lanes, tie) in enumerate(specs):
        for li, r in enumerate(lanes):
            want.append(r)
            z.append(1.5 + 0.02 * si + (0.0 if tie else 1e-4 * li))
    want, z = np.array(want[:P_FULL], np.int64), np.array(z[:P_FULL], np.float32)
    n = len(want)
    X0, Y0, w, h = want.T
    goal = np.stack([np.clip(X0, 0, GX), np.clip(Y0, 0, GY), np.clip(X0 + w, 0, GX), np.clip(Y0 + h, 0, GY)], -1)
    px, py, s, op = (np.zeros(n, np.float32) for _ in range(4))
    todo = np.arange(n)
    foc = W / (2.0 * math.tan(math.radians(30.0)))
    for _ in range(4000):
        if todo.size == 0:
            break
        m = todo.size
        big, small = np.maximum(w[todo], h[todo]), np.minimum(w[todo], h[todo])
        r3 = rng.uniform(np.maximum(2.6, 8.0 * big - 15.0), 8.0 * small + 1.0)
        cpx = rng.uniform(TILE * X0[todo], TILE * (X0[todo] + w[todo])).astype(np.float32)
        cpy = rng.uniform(TILE * Y0[todo], TILE * (Y0[todo] + h[todo])).astype(np.float32)
        cs = (np.sqrt(np.maximum((r3 / 3.0) ** 2 - 0.3163 - 0.3, 0.02)) * z[todo] / foc).astype(np.float32)
        cop = rng.uniform(0.6, 0.95, m).astype(np.float32)
        ref, tight, firm = _model_rects(cpx, cpy, cs, z[todo], cop)
        ok = firm & (ref == goal[todo]).all(-1) & (tight == goal[todo]).all(-1)
        hit = todo[ok]
        px[hit], py[hit], s[hit], op[hit] = cpx[ok], cpy[ok], cs[ok], cop[ok]
        todo = todo[~ok]
    assert todo.size == 0, "no placement found for %d rectangles, e.g. %s" % (todo.size, want[todo[:3]].tolist())
    tanx = np.float32(math.tan(math.radians(30.0)))
    tany = np.float32(tanx * H / W)
    means = np.stack([z * tanx * ((2 * px + 1) / np.float32(W) - 1), z * tany * ((2 * py + 1) / np.float32(H) - 1), z], -1)
    perm = rng.permutation(n)
    g = dict(means3D=np.zeros((n, 3), np.float32), scales=np.zeros((n, 3), np.float32),
             rotations=np.zeros((n, 4), np.float32), opacities=np.zeros((n, 1), np.float32))
    g["means3D"][perm] = means
    g["scales"][perm] = np.stack([s, s, np.float32(1e-3) * s], -1)
    g["rotations"][:, 0] = 1.0
    g["opacities"][perm, 0] = op
    shs = rng.normal(0.0, 0.2, (n, 16, 3))
    shs[:, 0, :] = rng.normal(0.5, 0.5, (n, 3))
    g["shs"] = shs.astype(np.float32)
    g = {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in g.items()}
    return g, perm, goal


def subset(p):
    """The last p Gaussians of the depth order (the small shapes of the tail), ids renumbered in their old order."""
    g, perm, goal = scene()
    keep = np.sort(perm[P_FULL - p:])
    return {k: np.ascontiguousarray(v[keep]) for k, v in g.items()}


def cameras(V):
    from gaussreg_amd import synthetic
    return synthetic.camera_ring(V, W, H, seed=11)  # (view 0 is the central camera the scene is built for)


@functools.lru_cache(maxsize=None)
def oracle_views(p, V):
    """(image, radii, instance count) per view from the oracle; computed once per (scene size, view count)."""
    from oracle import capi
    g = scene()[0] if p == P_FULL else subset(p)
    out = []
    for c in cameras(V):
        out.append(capi.rasterize_forward(g["means3D"], g["opacities"], shs=g["shs"], scales=g["scales"],
                                          rotations=g["rotations"], viewmatrix=c["viewmatrix"], projmatrix=c["projmatrix"],
                                          campos=c["campos"], bg=np.zeros(3, np.float32), W=W, H=H, tanfovx=c["tanfovx"],
                                          tanfovy=c["tanfovy"], sh_degree=3))
    return out


def _device_frame(p, V):
    """gr_raster_preprocess + gr_raster_render_ex on caller-owned buffers.  Returns the image, radii, the instance counts and
    per view the depth-ordered rectangles (x0, y0, w, h) the device binned."""
    import torch
    from gaussreg_amd import _lib
    from gaussreg_amd.rasterizer import GaussianRasterizationSettings, ViewBatch
    L = _lib.lib()
    g = scene()[0] if p == P_FULL else subset(p)
    t = {k: torch.from_numpy(v).cuda() for k, v in g.items()}
    sets = [GaussianRasterizationSettings(H, W, c["tanfovx"], c["tanfovy"], torch.zeros(3, device="cuda"), 1.0,
                                          torch.from_numpy(c["viewmatrix"]).cuda(), torch.from_numpy(c["projmatrix"]).cuda(), 3,
                                          torch.from_numpy(c["campos"]).cuda(), False, False) for c in cameras(V)]
    vb = ViewBatch(sets)
    st = _lib.stream_ptr(torch.device("cuda"))
    gbytes = L.gr_raster_geom_bytes(p, V, W, H)
    geom = torch.zeros(gbytes, dtype=torch.uint8, device="cuda")
    radii = torch.empty((V, p), dtype=torch.int32, device="cuda")
    color = torch.empty((V, 3, H, W), dtype=torch.float32, device="cuda")
    nr = (ctypes.c_int64 * (V + 1))()
    _lib.check(L.gr_raster_preprocess(p, 16, _lib.ptr(t["means3D"]), _lib.ptr(t["shs"]), None, _lib.ptr(t["opacities"]),
                                      _lib.ptr(t["scales"]), _lib.ptr(t["rotations"]), None, vb.array, V, _lib.ptr(radii),
                                      _lib.ptr(geom), gbytes, nr, st))
    total = sum(int(nr[v]) for v in range(V))
    bbytes = L.gr_raster_bin_bytes(total, W, H, V)
    binb = torch.full((bbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    _lib.check(L.gr_raster_render_ex(p, vb.array, V, nr, _lib.ptr(geom), gbytes, _lib.ptr(binb), bbytes, _lib.ptr(color), 0,
                                     st))
    torch.cuda.synchronize()
    off = (ctypes.c_int64 * 4)()
    assert L.gr_raster_debug_geom_layout(p, V, W, H, off) == 4
    gh = geom.cpu().numpy()
    order = gh[off[1]: off[1] + 4 * V * p].view(np.int32).reshape(V, p)
    raw = gh[off[2]: off[2] + 4 * V * p].view(np.uint32).reshape(V, p).astype(np.int64)
    nvis = gh[off[3]: off[3] + 4 * V].view(np.int32)
    rects = []
    for v in range(V):
        r = raw[v, : nvis[v]]
        assert not (r == (127 | (127 << 7))).any()  # (an 11 x 9 image: every rectangle fits the packing)
        rects.append(np.stack([r & 127, (r >> 7) & 127, (r >> 14) & 63, (r >> 20) & 63], -1))
    return color.cpu().numpy(), radii.cpu().numpy(), [int(nr[v]) for v in range(V)], rects, order


def _assert_scene_covers(rc, many_views):
    """From the rectangles the device binned in the first camera: every step shape this test is about is there."""
    assert len(rc) == P_FULL  # all visible: the steps are the ones the scene was built in
    x0, y0, w, h = rc.T
    steps = [slice(i, min(i + STEP, P_FULL)) for i in range(0, P_FULL, STEP)]
    shapes = [(int(w[s].max()), int(h[s].max())) for s in steps]
    for need in REQUIRED + [(6, 6), (6, 7), (5, 6)]:
        assert need in shapes, (need, shapes)
    assert any(max(s) > 8 for s in shapes)
    assert any(mx <= 8 and my <= 8 and not ((w[s] == mx) & (h[s] == my)).any() for s, (mx, my) in zip(steps, shapes)), \
        "no step takes its moduli from different lanes"
    for m in (3, 5, 6, 7):
        assert set(x0 % m) == set(range(m)) and set(y0 % m) == set(range(m)), m
    assert (x0 == 0).any() and (y0 == 0).any() and (x0 + w == GX).any() and (y0 + h == GY).any()
    # clamped at a border: narrower than its step's other rectangles of the same wanted shape would be; at least the corners
    assert ((x0 == 0) & (y0 == 0)).any() and ((x0 + w == GX) & (y0 + h == GY)).any()
    crowd = [int(((x0[s] <= 5) & (5 < x0[s] + w[s]) & (y0[s] <= 4) & (4 < y0[s] + h[s])).sum()) for s in steps]
    assert max(crowd) == STEP, crowd  # a whole step on one tile
    per_chunk = [int((w[i: i + CHUNK] * h[i: i + CHUNK]).sum()) for i in range(0, P_FULL, CHUNK)]
    if many_views:  # the first chunk cannot be staged, the second one is
        assert per_chunk[0] > STAGE_MAX and per_chunk[1] <= STAGE_MAX // 2, per_chunk


def run_case(p, V, ballot):
    from gaussreg_amd import _lib
    L = _lib.lib()
    old = L.gr_raster_ballot_ranking(ballot)
    try:
        img, radii, nr, rects, order = _device_frame(p, V)
    finally:
        L.gr_raster_ballot_ranking(old if old in (0, 1) else 0)
    want = oracle_views(p, V)
    for v in range(V):
        wimg, wrad, wnr = want[v]
        assert np.array_equal(radii[v], wrad), v
        assert nr[v] == int((rects[v][:, 2] * rects[v][:, 3]).sum()) and 0 < nr[v] <= wnr, (v, nr[v], wnr)
        assert np.array_equal(img[v].view(np.uint32), wimg.view(np.uint32)), \
            (v, int((img[v].view(np.uint32) != wimg.view(np.uint32)).sum()))
    assert nr[0] == want[0][2], (nr[0], want[0][2])  # first camera: built so that the tightening drops nothing
    if p == P_FULL:
        g, perm, goal = scene()
        _assert_scene_covers(rects[0], V > 4)
        got = np.stack([rects[0][:, 0], rects[0][:, 1], rects[0][:, 0] + rects[0][:, 2], rects[0][:, 1] + rects[0][:, 3]], -1)
        # same depth order up to the ties, and within a tie ascending ids
        assert np.array_equal(np.sort(order[0]), np.arange(P_FULL))
        z = g["means3D"][order[0], 2]
        assert (np.diff(z) >= 0).all() and (np.diff(order[0])[np.diff(z) == 0] > 0).all()
        inv = np.empty(P_FULL, np.int64)
        inv[perm] = np.arange(P_FULL)
        assert np.array_equal(got, goal[inv[order[0]]])  # the rectangles are the ones the scene was built for


CASES = [(P_FULL, 1), (P_FULL, 5), (P_SMALL, 1), (P_SMALL, 5)]


@pytest.mark.parametrize("ballot", [0, 1], ids=["lane-ordered", "ballot"])
@pytest.mark.parametrize("p,V", CASES, ids=["P%d-V%d" % c for c in CASES])
def test_exact_moduli_walk_matches_the_oracle(p, V, ballot):
    run_case(p, V, ballot)


def test_all_cases_with_the_device_side_list_check():
    """GR_RASTER_VERIFY=1 (read when the library loads, so in a child process): verify_tile_lists_kernel runs on every frame."""
    env = dict(os.environ, GR_RASTER_VERIFY="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "verify"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "verified %d" % (2 * len(CASES)) in r.stdout


if __name__ == "__main__" and sys.argv[1:] == ["verify"]:
    for case in CASES:
        for rank in (0, 1):
            run_case(case[0], case[1], rank)
    print("verified %d" % (2 * len(CASES)))
