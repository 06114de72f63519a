"""GPU: the walk step of blend_kernel on hand-placed scenes -- one 16 x 16 tile or two (32 x 16), Gaussians centred on chosen
pixels with chosen footprints, so that the cell lists have chosen lengths and a pixel saturates at a chosen entry of a pair.
Outputs are compared bit for bit with oracle.capi.rasterize_forward unless a test says otherwise; final_T and n_contrib
against a per-pixel walk in numpy (walk() below: the oracle's operation sequence, checked here against the oracle's image).

Dropped, as the oracle itself gives no fixed answer to compare with: nothing (every special-value scene below renders to the
same bits twice on the CPU; test_special_values checks that first)."""
import math

import numpy as np
import pytest
import torch

from gaussreg_amd import synthetic

pytestmark = pytest.mark.gpu

Z0 = 2.0


def cam_of(W, H):
    return synthetic.camera(W, H)


class Scene:
    """Gaussians given front to back: entry k sits at depth Z0 + 0.01 k, so the tile lists keep the order they are given in."""

    def __init__(self, W, H):
        self.W, self.H, self.cam = W, H, cam_of(W, H)
        self.rows = []

    def add(self, px, py, sigma_px, op, col):
        z = Z0 + 0.01 * len(self.rows)
        tanx, tany = self.cam["tanfovx"], self.cam["tanfovy"]
        x = ((2 * px + 1) / self.W - 1) * tanx * z
        y = ((2 * py + 1) / self.H - 1) * tany * z
        s = sigma_px * z / (self.W / (2 * tanx))
        self.rows.append((x, y, z, s, op, tuple(col) if np.ndim(col) else (col, col, col)))
        return self

    def arrays(self):
        r = self.rows
        n = len(r)
        return dict(means3D=np.array([[a[0], a[1], a[2]] for a in r], np.float32).reshape(n, 3),
                    opacities=np.array([a[4] for a in r], np.float32).reshape(n, 1),
                    colors_precomp=np.array([a[5] for a in r], np.float32).reshape(n, 3),
                    scales=np.array([[a[3]] * 3 for a in r], np.float32).reshape(n, 3),
                    rotations=np.tile(np.float32([1, 0, 0, 0]), (n, 1)))


def cam_kw(sc, bg):
    c = sc.cam
    return dict(viewmatrix=c["viewmatrix"], projmatrix=c["projmatrix"], campos=c["campos"], bg=np.asarray(bg, np.float32),
                W=sc.W, H=sc.H, tanfovx=c["tanfovx"], tanfovy=c["tanfovy"])


def oracle(sc, bg=(0.0, 0.0, 0.0), arrays=None):
    from oracle import capi
    g = arrays or sc.arrays()
    return capi.rasterize_forward(g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"],
                                  rotations=g["rotations"], **cam_kw(sc, bg))


def settings(sc, bg):
    from gaussreg_amd.rasterizer import GaussianRasterizationSettings
    c = sc.cam
    return GaussianRasterizationSettings(sc.H, sc.W, c["tanfovx"], c["tanfovy"], torch.tensor(bg, dtype=torch.float32), 1.0,
                                         torch.from_numpy(c["viewmatrix"].copy()), torch.from_numpy(c["projmatrix"].copy()), 0,
                                         torch.from_numpy(c["campos"].copy()), False, False)


def gpu(sc, bg=(0.0, 0.0, 0.0), arrays=None, grad=False, **kw):
    from gaussreg_amd.rasterizer import GaussianRasterizer
    t = {k: torch.from_numpy(v).cuda() for k, v in (arrays or sc.arrays()).items()}
    if grad:
        t["colors_precomp"].requires_grad_(True)
    return GaussianRasterizer(settings(sc, bg), **kw)(t["means3D"], None, t["opacities"], colors_precomp=t["colors_precomp"],
                                                      scales=t["scales"], rotations=t["rotations"])


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def assert_bits(got, want, what):
    g, w = bits(got), bits(want)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} of {g.size} values differ, first at {tuple(bad[0])}: " \
                          f"{g[tuple(bad[0])]:#x} vs {w[tuple(bad[0])]:#x}"


def check(sc, bg=(0.1, 0.3, 0.7), what=""):
    want, wr, _ = oracle(sc, bg)
    img, radii = gpu(sc, bg)
    assert np.array_equal(radii.cpu().numpy(), wr), what
    assert_bits(img, want, what)
    return want


def broad(sc, n, op, col=None, px=7.5, py=7.5, sigma=20.0):
    """n Gaussians that reach every pixel of the tile around (px, py) with nearly their full opacity"""
    rng = np.random.default_rng(len(sc.rows) + n)
    for _ in range(n):
        sc.add(px, py, sigma, op, rng.random(3) if col is None else col)
    return sc


# ---- list lengths: the pad entry of odd lists, the read one step ahead of the last pair, a second batch of one entry

@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257])
def test_list_lengths(n):
    sc = broad(Scene(16, 16), n, 0.012)   # alpha ~ 0.012 > 1/255 on every pixel; 257 of them leave T ~ 0.05: no saturation
    want = check(sc, what=f"{n} entries in every cell list")
    assert want.std() > 0
    sc2 = broad(Scene(32, 16), n, 0.012, px=15.5)   # both tiles, every cell
    check(sc2, what=f"{n} entries, two tiles")


# ---- where in a pair a pixel saturates.  Opacity 0.8 leaves T = 0.2^k: 3.2e-4 after five entries, the sixth (index 5,
# entry 1 of its pair) saturates; a first entry of 0.96 moves everything one entry forward (index 4, entry 0 of its pair).
# The falloff over the tile moves the position by an entry or two from pixel to pixel, so one scene holds several cases.

def _saturating(first_op, n_after, tail_col):
    sc = Scene(16, 16)
    sc.add(7.5, 7.5, 20.0, first_op, (0.2, 0.5, 0.9))
    broad(sc, 4, 0.8)
    for _ in range(n_after):
        sc.add(7.5, 7.5, 20.0, 0.8, tail_col)
    return sc


@pytest.mark.parametrize("first_op,n_after", [(0.96, 3), (0.8, 3), (0.96, 1), (0.8, 1), (0.96, 0), (0.8, 0)])
def test_saturation_position(first_op, n_after):
    # a bright colour behind the saturating entry: it must not reach the image
    want = check(_saturating(first_op, n_after, (1000.0, 1000.0, 1000.0)), bg=(0.0, 0.0, 0.0),
                 what=f"first opacity {first_op}, {n_after} entries behind")
    if n_after:
        assert float(want.max()) < 10.0


def test_no_saturation():
    check(broad(Scene(16, 16), 6, 0.3), what="six entries, T stays above 0.1")


# ---- pairs of which only one entry passes alpha >= 1/255 / power <= 0, differently for neighbouring pixels of one cell

def test_mixed_ok_within_pairs():
    sc = Scene(32, 16)
    rng = np.random.default_rng(5)
    for k in range(40):
        if k % 2 == (k // 8) % 2:   # entry 0 or entry 1 of the pair is the narrow one, alternating every four pairs
            sc.add(float(rng.uniform(0, 32)), float(rng.uniform(0, 16)), float(rng.uniform(0.4, 1.6)), 0.9, rng.random(3))
        else:
            sc.add(15.5, 7.5, 30.0, 0.05, rng.random(3))
    sc.add(3.0, 3.0, 25.0, 0.0042, (0.9, 0.1, 0.4))   # barely above 1/255 near its centre only
    sc.add(12.2, 9.7, 25.0, 0.0041, (0.3, 0.8, 0.1))
    check(sc, what="narrow and broad entries alternating")


# ---- inf / NaN / -0.0

def _special_scenes():
    out = {}
    sc = broad(Scene(16, 16), 3, 0.2)
    sc.add(4.0, 4.0, 1.0, 0.7, (math.inf, 0.5, -math.inf))      # reaches a few pixels; the others skip it and keep their bits
    broad(sc, 3, 0.2)
    out["inf colour"] = (sc, (0.1, 0.3, 0.7))
    sc = broad(Scene(16, 16), 2, 0.2)
    sc.add(10.0, 6.0, 1.0, math.nan, (0.5, 0.6, 0.7))          # fminf(0.99, NaN) = 0.99: it blends wherever power <= 0
    sc.add(3.0, 11.0, 1.0, 0.6, (math.nan, 0.25, math.nan))     # NaN into the image of the pixels it reaches
    broad(sc, 3, 0.2)
    out["NaN opacity"] = (sc, (0.1, 0.3, 0.7))
    # the product colour * weight underflows to -0.0; with a background of -0.0 it reaches the image as -0.0, and
    # the entries a pixel skips afterwards must leave it
    sc = Scene(16, 16)
    sc.add(7.5, 7.5, 20.0, 0.02, (-1.4e-45, -1.4e-45, -1.4e-45))
    sc.add(2.0, 2.0, 0.8, 0.9, (0.5, 0.5, 0.5))
    sc.add(12.0, 11.0, 0.8, 0.9, (0.5, 0.5, 0.5))
    sc.add(7.5, 7.5, 20.0, 0.003, (5.0, 5.0, 5.0))              # alpha < 1/255 everywhere: skipped by every pixel
    out["minus zero"] = (sc, (-0.0, -0.0, -0.0))
    return out


@pytest.mark.parametrize("name", ["inf colour", "NaN opacity", "minus zero"])
def test_special_values(name):
    sc, bg = _special_scenes()[name]
    a, ra, _ = oracle(sc, bg)
    b, rb, _ = oracle(sc, bg)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(ra, rb), "the oracle itself is not reproducible here"
    if name == "minus zero":
        assert (bits(a) == np.int32(-2 ** 31)).any(), "the scene does not leave -0.0 in the image"
    else:
        assert (~np.isfinite(a)).any() and np.isfinite(a).any()
    img, radii = gpu(sc, bg)
    assert np.array_equal(radii.cpu().numpy(), ra)
    assert_bits(img, a, name)   # NaN for NaN included: the same operations on the same operands give the same payload


# ---- about 600 entries: three batches of the tile's list

def _three_batches():
    sc = Scene(16, 16)
    rng = np.random.default_rng(9)
    for k in range(600):
        if k % 3 == 0:
            sc.add(7.5, 7.5, 20.0, 0.006, rng.random(3))
        else:
            sc.add(float(rng.uniform(-1, 17)), float(rng.uniform(-1, 17)), float(rng.uniform(1.0, 4.0)), 0.03, rng.random(3))
    return sc


def test_three_batches():
    check(_three_batches(), what="600 entries")


# ---- KEEP: final_T and n_contrib of the autograd forward

def _fma(a, b, c):
    # a * b is exact in float64 (24 + 24 bits); the sum rounds once to 53 bits and once more to 24: walk() is checked
    # against the oracle's image for the scenes it is used on
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def walk(sc, bg=(0.0, 0.0, 0.0)):
    """The oracle's blend loop per pixel on the oracle's preprocessed records: (image, final_T, n_contrib).  Valid for one
    tile row where every Gaussian's rectangle covers every tile (asserted): the tile's list is then all of them by depth."""
    from oracle import capi
    g = sc.arrays()
    kw = cam_kw(sc, bg)
    kw.pop("bg")
    pre = capi.raster_preprocess(g["means3D"], g["opacities"], colors_precomp=g["colors_precomp"], scales=g["scales"],
                                 rotations=g["rotations"], **kw)
    tiles = ((sc.W + 15) // 16) * ((sc.H + 15) // 16)
    assert (pre["tiles_touched"] == tiles).all()
    order = np.argsort(pre["depths"], kind="stable")
    f = np.float32
    img = np.zeros((3, sc.H, sc.W), f)
    fT = np.ones((sc.H, sc.W), f)
    nc = np.zeros((sc.H, sc.W), np.int32)
    for py in range(sc.H):
        for px in range(sc.W):
            T, C = f(1.0), [f(0.0)] * 3
            for k, i in enumerate(order):
                dx, dy = f(pre["xy"][i, 0] - f(px)), f(pre["xy"][i, 1] - f(py))
                c = pre["conic_opacity"][i]
                q = _fma(f(c[0] * dx), dx, f(f(c[2] * dy) * dy))
                power = _fma(f(-0.5), q, -f(f(c[1] * dx) * dy))
                if power > 0:
                    continue
                alpha = min(f(0.99), f(c[3] * capi.exp_det(power)[0]))
                if alpha < f(1.0) / f(255.0):
                    continue
                test_T = f(T * f(f(1.0) - alpha))
                if test_T < f(0.0001):
                    break
                w = f(alpha * T)
                C = [_fma(g["colors_precomp"][i, ch], w, C[ch]) for ch in range(3)]
                T = test_T
                nc[py, px] = k + 1
            fT[py, px] = T
            img[:, py, px] = [_fma(T, f(bg[ch]), C[ch]) for ch in range(3)]
    return img, fT, nc


@pytest.mark.parametrize("which", ["entry 0", "entry 1", "none", "odd"])
def test_keep_state(which):
    sc = {"entry 0": lambda: _saturating(0.96, 2, (0.3, 0.3, 0.3)), "entry 1": lambda: _saturating(0.8, 2, (0.3, 0.3, 0.3)),
          "none": lambda: broad(Scene(32, 16), 6, 0.3, px=15.5, sigma=30.0),
          "odd": lambda: broad(Scene(16, 16), 3, 0.5)}[which]()
    want, _, R = oracle(sc)
    w_img, w_T, w_n = walk(sc)
    assert_bits(w_img, want, "the numpy walk against the oracle's image")
    img, radii = gpu(sc, grad=True)
    assert_bits(img, want, "image of the autograd forward")
    hw = sc.W * sc.H
    state = img.grad_fn.state
    assert_bits(state[:hw].reshape(sc.H, sc.W), w_T, "final_T")
    assert np.array_equal(state[hw:2 * hw].view(torch.int32).reshape(sc.H, sc.W).cpu().numpy(), w_n), "n_contrib"
    if which != "none":
        assert (w_n < len(sc.rows)).any() or which == "odd"


# ---- AUX (render_depth=True)

def test_depth_and_alpha_maps():
    sc = _saturating(0.8, 2, (0.3, 0.3, 0.3))
    g = sc.arrays()
    plain, _ = gpu(sc)
    img, radii, depth, alpha = gpu(sc, render_depth=True)
    assert_bits(img, plain, "colour with the maps against the plain render")
    # depth runs the red channel's operations on z: the oracle's red channel of the scene with red := z is its exact value
    # (the view matrix is the identity: view-space z is means3D z); alpha = 1 - final_T of the walk.  Both bit for bit,
    # which is inside any bar in float64.
    gz = dict(g, colors_precomp=np.repeat(g["means3D"][:, 2:3], 3, 1))
    want_z, _, _ = oracle(sc, arrays=gz)
    assert_bits(depth[0], want_z[0], "depth")
    _, w_T, _ = walk(sc)
    assert_bits(alpha[0], np.float32(1.0) - w_T, "alpha")


# ---- fast_exp=True: the bar of tests/test_gpu_rasterizer_fast.py against the exact image

def test_fast_exp():
    sc = _three_batches()
    want, _, _ = oracle(sc, (0.1, 0.2, 0.3))
    fast, _ = gpu(sc, (0.1, 0.2, 0.3), fast_exp=True)
    f, e = fast.cpu().numpy().astype(np.float64), want.astype(np.float64)
    d = np.abs(f - e)
    outside = (d > 1e-6 + 1e-5 * np.abs(e)).any(axis=0).sum()
    assert outside <= 1e-3 * sc.W * sc.H, f"{outside} pixels outside 1e-6 + 1e-5 rel of the exact image"
    assert d.mean() < 1e-6 and d.max() < 8e-3, (d.mean(), d.max())
