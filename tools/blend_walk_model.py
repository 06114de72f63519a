"""CPU model of what blend_kernel actually reads of a tile's list on bench.py's scene: where the tile saturates, how many
256-entry batches it runs, how full they are, how many 4 x 4-pixel cells an entry reaches, and how many walk steps (two
list entries each) a wave spends per batch when it owns a row of four cells (the kernel's assignment) or a 2 x 2 block.

    python tools/blend_walk_model.py [P W H [camera index ...]]      (default: 1000000 640 480 0 16, 30 sample tiles each)

Uses only gaussreg_amd.synthetic and oracle.capi.raster_preprocess (no GPU).  The lists are the binning's: the tightened
rectangles (tools/binning_rounds.py), depth order, chunks of 2 048 Gaussians, windows of 64 chunks, batches cut inside a
window.  Per pixel the blend's rules in float64 (skip alpha < 1/255 and power > 0, stop before T (1 - alpha) < 1e-4); the
cell-reach test is the kernel's circle and per-axis test with the cull radius kc = 2 lambda_max and the level-set
half-extents, without their fp32 margins.  A wave's steps in a batch = the largest number of entry pairs any of its pixels
walks through its cell's list; a pixel that saturated earlier walks none, and the tile stops at the first batch boundary
where all 256 pixels are saturated."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from gaussreg_amd import synthetic  # noqa: E402
from oracle import capi  # noqa: E402
from binning_rounds import device_rects  # noqa: E402

TILE, CELL, BATCH, CHUNK, WINDOW = 16, 4, 256, 2048, 64
ROWS = [[4 * r + k for k in range(4)] for r in range(4)]                       # wave r: cells 4 r .. 4 r + 3
BLOCKS = [[8 * (b // 2) + 2 * (b % 2) + k for k in (0, 1, 4, 5)] for b in range(4)]  # wave b: a 2 x 2 block of cells


def tile_walk(tx, ty, ids, win, pp):
    """ids: the tile's list (depth order), win: the window each entry belongs to.  Returns the tile's figures."""
    n = len(ids)
    co = pp["conic_opacity"][ids].astype(np.float64)
    cx, cy = pp["xy"][ids, 0].astype(np.float64), pp["xy"][ids, 1].astype(np.float64)
    xs = tx * TILE + np.arange(TILE, dtype=np.float64)
    ys = ty * TILE + np.arange(TILE, dtype=np.float64)
    dx = cx[:, None, None] - xs[None, None, :]
    dy = cy[:, None, None] - ys[None, :, None]
    power = -0.5 * (co[:, 0, None, None] * dx * dx + co[:, 2, None, None] * dy * dy) - co[:, 1, None, None] * dx * dy
    alpha = np.minimum(0.99, co[:, 3, None, None] * np.exp(np.minimum(power, 0.0)))
    hit = (power <= 0.0) & (alpha >= 1.0 / 255.0)                 # (n, 16, 16): the entry is blended or saturates the pixel
    t_after = np.cumprod(np.where(hit, 1.0 - alpha, 1.0), axis=0)
    sat = hit & (t_after < 1e-4)
    stop = np.where(sat.any(0), sat.argmax(0), n)                 # per pixel: index of the entry that saturates it (n: none)
    # cell reach
    dc = co[:, 0] * co[:, 2] - co[:, 1] ** 2
    a, c, b = co[:, 2] / dc, co[:, 0] / dc, -co[:, 1] / dc
    mid = 0.5 * (a + c)
    l1 = mid + np.sqrt(np.maximum(0.1, mid * mid - (a * c - b * b)))
    pc = np.log(255.0 * co[:, 3])
    rc2 = pc * 2.0 * l1
    lo = np.arange(0, TILE, CELL, dtype=np.float64)
    ex = np.maximum(np.maximum(tx * TILE + lo[None, :] - cx[:, None], cx[:, None] - (tx * TILE + lo[None, :] + CELL - 1)), 0.0)
    ey = np.maximum(np.maximum(ty * TILE + lo[None, :] - cy[:, None], cy[:, None] - (ty * TILE + lo[None, :] + CELL - 1)), 0.0)
    reach = ((ex[:, None, :] ** 2 + ey[:, :, None] ** 2 <= rc2[:, None, None]) & (ex[:, None, :] ** 2 <= 2 * pc[:, None, None] * a[:, None, None])
             & (ey[:, :, None] ** 2 <= 2 * pc[:, None, None] * c[:, None, None])).reshape(n, 16)  # cell = 4 * cell row + cell column
    stop_cell = stop.reshape(4, CELL, 4, CELL).transpose(0, 2, 1, 3).reshape(16, CELL * CELL)  # (cell, pixel of the cell)
    # batches
    starts = []
    for wdw in np.unique(win):
        i0, i1 = np.searchsorted(win, wdw), np.searchsorted(win, wdw, side="right")
        starts += [(s, min(s + BATCH, i1)) for s in range(i0, i1, BATCH)]
    batches, entries, steps_row, steps_blk, steps_eq, read_to = 0, 0, 0.0, 0.0, 0.0, 0
    for s, e in starts:
        if (stop < s).all():
            break
        batches += 1
        entries += e - s
        read_to = e
        r = reach[s:e]
        rank = np.cumsum(r, axis=0)                               # position + 1 of an entry in its cell's list
        walked = np.zeros(16)
        for cell in range(16):
            live = stop_cell[cell] >= s
            if not live.any():
                continue
            st = stop_cell[cell][live]
            # a live pixel walks its cell's list up to and including the entry that saturates it, or to the end of the list
            upto = np.where(st < e, rank[np.minimum(st, e - 1) - s, cell], rank[-1, cell] if len(rank) else 0)
            walked[cell] = np.ceil(upto.max() / 2.0)
        steps_row += sum(max(walked[c] for c in wv) for wv in ROWS)
        steps_blk += sum(max(walked[c] for c in wv) for wv in BLOCKS)
        steps_eq += walked.sum() / 4.0
    sat_at = int(stop.max()) + 1 if (stop < n).all() else n
    return dict(n=n, sat_frac=sat_at / max(n, 1), saturates=bool((stop < n).all()), batches=batches, entries=entries,
                read_frac=read_to / max(n, 1), cells=float(reach[:read_to].sum(1).mean()) if read_to else 0.0,
                steps_row=steps_row, steps_blk=steps_blk, steps_eq=steps_eq)


def main(P=1_000_000, W=640, H=480, *cams):
    cams = list(cams) or [0, 16]
    per_cam = 30
    g = synthetic.gaussians_c2(P, seed=0, sh_degree=3)
    ring = synthetic.camera_ring(32, W, H, seed=0)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rng = np.random.default_rng(0)
    rows = []
    for ci in cams:
        c = ring[ci]
        pp = capi.raster_preprocess(g["means3D"], g["opacities"], shs=g["shs"], scales=g["scales"], rotations=g["rotations"],
                                    viewmatrix=c["viewmatrix"], projmatrix=c["projmatrix"], campos=c["campos"], W=W, H=H,
                                    tanfovx=c["tanfovx"], tanfovy=c["tanfovy"], sh_degree=3)
        x0, y0, w, h, live = device_rects(pp, W, H)
        order = np.flatnonzero(live)
        order = order[np.argsort(pp["depths"][order], kind="stable")]
        ox0, oy0, ow, oh = x0[order], y0[order], w[order], h[order]
        for t in rng.choice(gx * gy, size=min(per_cam, gx * gy), replace=False):
            tx, ty = int(t % gx), int(t // gx)
            m = np.flatnonzero((ox0 <= tx) & (tx < ox0 + ow) & (oy0 <= ty) & (ty < oy0 + oh))
            if len(m):
                rows.append(tile_walk(tx, ty, order[m], m // CHUNK // WINDOW, pp))
    k = len(rows)
    tot = {f: sum(r[f] for r in rows) for f in ("n", "batches", "entries", "steps_row", "steps_blk", "steps_eq")}
    print(f"tiles {k}  list length {tot['n'] / k:.0f}  saturating tiles {sum(r['saturates'] for r in rows)}")
    print("saturation point (share of the list at which all 256 pixels are below T = 1e-4): mean %.1f %%, quartiles %s"
          % (100 * np.mean([r["sat_frac"] for r in rows]),
             [round(100 * float(q), 1) for q in np.percentile([r["sat_frac"] for r in rows], [25, 50, 75])]))
    print(f"entries read per tile {tot['entries'] / k:.0f} ({100 * tot['entries'] / tot['n']:.1f} % of the list: "
          f"{100 - 100 * tot['entries'] / tot['n']:.1f} % of the instances are never read)")
    print(f"batches per tile {tot['batches'] / k:.2f}   entries per batch {tot['entries'] / tot['batches']:.0f}   "
          f"with full 256-entry batches {tot['entries'] / k / BATCH:.2f} batches per tile "
          f"(saves {tot['batches'] / k - tot['entries'] / k / BATCH:.2f})")
    print(f"cells reached per entry read {np.mean([r['cells'] for r in rows]):.2f} of 16")
    nb = tot["batches"]
    print(f"wave-steps per batch (four waves)   rows {tot['steps_row'] / nb:.1f}   2 x 2 blocks {tot['steps_blk'] / nb:.1f}   "
          f"all cells equal {tot['steps_eq'] / nb:.1f}")


if __name__ == "__main__":
    main(*[int(x) for x in sys.argv[1:]])
