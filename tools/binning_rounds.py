"""CPU model of the tile scatter's residue-class walk: how many rounds (one LDS atomic per lane at most) a step of 64
depth-consecutive Gaussians costs under different choices of the moduli, on bench.py's scene and cameras.

    python tools/binning_rounds.py [P W H [camera index ...]]      (default: 1000000 640 480 0 9 18 27 of the 32 bench cameras)

Uses only gaussreg_amd.synthetic and oracle.capi.raster_preprocess (no GPU).  The rectangles are the ones preprocess_kernel
emits: the reference square (radius = ceil(3 sigma_max)) intersected with the bounding box of the alpha >= 1/255 level set,
rebuilt here from the oracle's conic, opacity, centre and radius.  A step whose largest side exceeds 8 tiles is walked one
Gaussian at a time on the device; it counts one round per tile row of each of its Gaussians in every column below."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from gaussreg_amd import synthetic  # noqa: E402
from oracle import capi  # noqa: E402

TILE, STEP = 16, 64
WAVE_STEPS = 8  # steps of a wave of the 256-thread scatter: a quarter of a 2 048-Gaussian chunk


def device_rects(pp, W, H):
    """(x0, y0, w, h) per Gaussian as preprocess_kernel packs them (fp32 throughout); w = h = 0 where nothing is binned."""
    f32 = np.float32
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    px, py = pp["xy"][:, 0], pp["xy"][:, 1]
    rad = pp["radii"].astype(f32)
    co = pp["conic_opacity"]
    with np.errstate(all="ignore"):
        dc = co[:, 0] * co[:, 2] - co[:, 1] * co[:, 1]  # det(conic) = 1 / det(cov)
        a, b, c = co[:, 2] / dc, -co[:, 1] / dc, co[:, 0] / dc
        det, mid = a * c - b * b, f32(0.5) * (a + c)
        root = np.sqrt(np.maximum(f32(0.1), mid * mid - det))
        l1, l2 = mid + root, mid - root
        x0 = np.clip(np.trunc((px - rad) / TILE), 0, gx)
        y0 = np.clip(np.trunc((py - rad) / TILE), 0, gy)
        x1 = np.clip(np.trunc((px + rad + (TILE - 1)) / TILE), 0, gx)
        y1 = np.clip(np.trunc((py + rad + (TILE - 1)) / TILE), 0, gy)
        live = (pp["radii"] > 0) & ((x1 - x0) * (y1 - y0) > 0)
        pcm = np.log(f32(255.0) * co[:, 3]) + f32(2e-3)
        kc = f32(1.001) / (f32(0.5) / l1 - f32(2e-6))
        cp = pcm + f32(2e-6) * (pcm * kc)
        hx = np.sqrt(2 * cp * a) * f32(1.001) + f32(1e-2)
        hy = np.sqrt(2 * cp * c) * f32(1.001) + f32(1e-2)
        tight = live & (det > 0) & (l2 >= 0.29) & (l1 < 1e4) & (pcm > 0)
        tx0 = np.maximum(x0, np.floor(np.ceil(px - hx) / TILE))
        ty0 = np.maximum(y0, np.floor(np.ceil(py - hy) / TILE))
        tx1 = np.maximum(np.minimum(x1, np.floor(np.floor(px + hx) / TILE) + 1), tx0)
        ty1 = np.maximum(np.minimum(y1, np.floor(np.floor(py + hy) / TILE) + 1), ty0)
    x0, y0, x1, y1 = (np.where(tight, t, r) for t, r in ((tx0, x0), (ty0, y0), (tx1, x1), (ty1, y1)))
    w, h = np.where(live, x1 - x0, 0).astype(np.int64), np.where(live, y1 - y0, 0).astype(np.int64)
    return x0.astype(np.int64), y0.astype(np.int64), w, h, live


def step_rounds(w, h):
    """w, h: (steps, 64), zero in dead lanes.  Rounds of each step under the four walks + the step's largest side."""
    mx, my = w.max(1), h.max(1)
    md = np.maximum(mx, my)
    wide = (h * (w > 0)).sum(1)  # one Gaussian at a time, a round per tile row
    pow2 = np.where(md <= 2, 2, np.where(md <= 4, 4, 8)) ** 2
    small = md <= 8
    inst = (w * h).sum(1)
    return dict(now=np.where(small, pow2, wide), square=np.where(small, md * md, wide), rect=np.where(small, mx * my, wide),
                bound=inst / STEP), md, inst


def main(P=1_000_000, W=640, H=480, *cams):
    cams = list(cams) or [0, 9, 18, 27]
    g = synthetic.gaussians_c2(P, seed=0, sh_degree=3)
    ring = synthetic.camera_ring(32, W, H, seed=0)
    acc = {k: 0.0 for k in ("now", "square", "rect", "bound")}
    sides = np.zeros(6, np.int64)
    n_steps = n_inst = n_vis = 0
    for ci in cams:
        c = ring[ci]
        pp = capi.raster_preprocess(g["means3D"], g["opacities"], shs=g["shs"], scales=g["scales"], rotations=g["rotations"],
                                    viewmatrix=c["viewmatrix"], projmatrix=c["projmatrix"], campos=c["campos"], W=W, H=H,
                                    tanfovx=c["tanfovx"], tanfovy=c["tanfovy"], sh_degree=3)
        x0, y0, w, h, live = device_rects(pp, W, H)
        order = np.flatnonzero(live)
        order = order[np.argsort(pp["depths"][order], kind="stable")]  # depth order, ties by id
        n = len(order)
        pad = (-n) % STEP
        ws = np.concatenate([w[order], np.zeros(pad, np.int64)]).reshape(-1, STEP)
        hs = np.concatenate([h[order], np.zeros(pad, np.int64)]).reshape(-1, STEP)
        ws, hs = ws[(ws * hs).sum(1) > 0], hs[(ws * hs).sum(1) > 0]
        r, md, inst = step_rounds(ws, hs)
        for k in acc:
            acc[k] += float(r[k].sum())
        sides += np.bincount(np.minimum(md, 5), minlength=6)
        n_steps += len(md)
        n_inst += int(inst.sum())
        n_vis += n
        print(f"camera {ci:2d}: visible {n}  instances {int(inst.sum())} ({inst.sum() / max(n, 1):.2f} per visible Gaussian)  "
              f"rounds per step now {r['now'].mean():.2f}  exact square {r['square'].mean():.2f}  "
              f"exact rectangle {r['rect'].mean():.2f}  bound {r['bound'].mean():.2f}")
    print(f"all: steps {n_steps}  instances per visible Gaussian {n_inst / max(n_vis, 1):.2f}")
    print("largest side in the step (tiles)  1: %.2f %%  2: %.2f %%  3: %.2f %%  4: %.2f %%  >= 5: %.2f %%"
          % tuple(100.0 * sides[1:6] / max(n_steps, 1)))
    print("rounds per step   now (2 / 4 / 8 squared) %.2f   exact square %.2f   exact rectangle %.2f   lower bound %.2f"
          % tuple(acc[k] / max(n_steps, 1) for k in ("now", "square", "rect", "bound")))
    # Phase A of the 256-thread scatter no longer walks: per step four corner adds into the wave's difference grid, and per
    # wave (WAVE_STEPS steps) the two prefix passes over its cursor row -- a read and a write per grid row and lane round down
    # the columns, the same per word (cell, for an odd gx) along the rows (+ a pass over the words that splits the halves,
    # for an odd gx).  The walk of phase A cost the rounds of the exact rectangle; phase C still does.
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    up = lambda a, b: (a + b - 1) // b  # noqa: E731
    if gx % 2 == 0:
        prefix = 2 * gy * up(gx // 2, STEP) + 2 * (gx // 2) * up(gy, STEP)
    else:
        prefix = 2 * up((gx * gy + 1) // 2, STEP) + 2 * gy * up(gx, STEP) + 2 * gx * up(gy, STEP)
    print("phase A, LDS instructions per step   walk (exact rectangle) %.2f   grid: 4 corner adds + %d prefix / %d steps = %.2f"
          "   (%d x %d tiles)" % (acc["rect"] / max(n_steps, 1), prefix, WAVE_STEPS, 4 + prefix / WAVE_STEPS, gx, gy))


if __name__ == "__main__":
    main(*[int(x) for x in sys.argv[1:]])
