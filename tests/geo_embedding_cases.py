"""Test helper (not collected): the seeded case table of tests/test_gpu_geo_embedding_f64.py, shared with the CPU file
tests/test_geo_embedding_f64_reference.py, which asserts the admission rule for every dyadic case.

Dyadic clouds.  Coordinates are small integers times a power of two.  Every fp32 product and sum of the squared distance
x2 - 2 xy + y2, of the differences, of the cross product and of the dot product is then exact in any association, so fp32
and float64 agree on the distances, on the neighbour sets and on every tie, and the diagonal is exactly zero: the float64
bar of helpers.assert_as_exact_as_reference applies to every element of the output, diagonal included.

Marked cases.  An fp32 sine of an argument ~ x carries an absolute error ~ 6e-8 x from the rounding of the argument
alone, so no fp32 implementation meets 1e-5 of the scale against float64 once index * div_term passes ~ 100.  div_term[0]
is 1, so a case is `marked` exactly when its largest float64 distance index exceeds MARK_INDEX; a marked case keeps the
bars against the reference's fp32 values and against the reference's own error.  The CPU file asserts that the marking
follows from the indices.

Modes: "table" (the default), "gemm" (mode="gemm": split-bf16, or the fp32 kernel where C > 512) and "fp32"
(fp32_mfma=True).  A configuration runs in every mode its width allows unless it names its modes.
"""
import zlib
from collections import namedtuple

import numpy as np

MARK_INDEX = 100.0
TABLE_INV_H = 32.0
TABLE_X_MAX_D = 256.0

Config = namedtuple("Config", "name cloud C k red sigma_d sigma_a wscale modes path dyadic marked")
Case = namedtuple("Case", "name cfg mode")


def _seed(name):
    return zlib.crc32(name.encode())


def modes_for(C):
    return tuple(m for m, ok in (("table", C % 4 == 0), ("gemm", C % 16 == 0), ("fp32", C % 32 == 0)) if ok)


def kernel_of(C, mode):
    if mode == "table":
        return "table"
    return "split-bf16" if mode == "gemm" and C <= 512 else "fp32-mfma"


# ------------------------------------------------------------------------------------------------------------ clouds
def _grid(n, den, cells, seed, dups=()):
    """n distinct points of the integer lattice [0, cells)^3 times 1 / den; dups = ((src, dst), ...) copies point src to dst."""
    rng = np.random.default_rng(seed)
    seen, pts = set(), []
    while len(pts) < n:
        p = tuple(int(v) for v in rng.integers(0, cells, 3))
        if p not in seen:
            seen.add(p)
            pts.append(p)
    q = np.array(pts, np.float64) / den
    for src, dst in dups:
        q[dst] = q[src]
    return q


def build_cloud(spec):
    """(N, 3) float64 array of values that are exact in fp32."""
    kind = spec[0]
    if kind == "grid":                       # ("grid", n, den, cells, seed[, dups])
        return _grid(*spec[1:])
    if kind == "lattice":                    # regular lattice: exact ties at every neighbour rank
        _, nx, ny, nz, step = spec
        g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
        return g.astype(np.float64) * step
    if kind == "line":                       # collinear along (1, 2, 2) / den: every angle is exactly 0 or pi
        _, n, den, span, seed = spec
        t = np.random.default_rng(seed).choice(span, n, replace=False)
        return t[:, None] * np.array([1.0, 2.0, 2.0]) / den
    if kind == "plane":                      # coplanar: z = x + y on the grid
        _, n, den, cells, seed = spec
        p = _grid(n, den, cells, seed)
        p[:, 2] = p[:, 0] + p[:, 1]
        assert len(np.unique(p, axis=0)) == n, "the seed gives two points over one (x, y): take another"
        return p
    if kind == "table_edge":
        # quarter-metre units, sigma_d = 1/4: the distance index of (origin, p) is sqrt(|p|^2) with |p|^2 an integer n.
        # floor(32 sqrt(n)) = 8190, 8191 (inside), 8192 at n = 65536 (t = 0) and 65537 (the last cell the table serves:
        # m + 3 = rows - 1), 65552 (float64 just below 8193 / 32, fp32 rounds onto it), 65553 (direct), then far beyond.
        far = [(255, 22, 3), (255, 21, 8), (256, 0, 0), (256, 1, 0), (256, 4, 0), (256, 4, 1), (257, 0, 0), (300, 40, 9)]
        near = [(0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 1, 3), (2, 2, 1), (3, 0, 2)]
        return np.array(near + far, np.float64) / 4.0
    if kind == "generic":                    # not dyadic: index noise by design
        _, n, seed, box = spec
        return (np.random.default_rng(seed).random((n, 3)) * np.array(box)).astype(np.float32).astype(np.float64)
    raise ValueError(kind)


def build_params(C, wscale, seed):
    """nn.Linear's default initialisation (U(-1/sqrt(C), 1/sqrt(C)) for weight and bias) times wscale, and the
    sinusoid's div_term, as the fp32 values the module holds."""
    rng = np.random.default_rng(seed)
    b = wscale / np.sqrt(C)
    u = lambda *s: rng.uniform(-b, b, s).astype(np.float32)
    div = np.exp(np.arange(0, C, 2, dtype=np.float32) * np.float32(-np.log(10000.0) / C)).astype(np.float32)
    return {"w_d": u(C, C), "b_d": u(C), "w_a": u(C, C), "b_a": u(C), "div": div}


def build(cfg):
    return build_cloud(cfg.cloud), build_params(cfg.C, cfg.wscale, _seed(cfg.name))


# ------------------------------------------------------------------------------------------------------------ table
CONFIGS = []


def _cfg(name, cloud, C, k, red="max", sigma_d=0.2, sigma_a=15, wscale=1.0, modes=None, path="", dyadic=True, marked=False):
    CONFIGS.append(Config(name, cloud, C, k, red, sigma_d, sigma_a, wscale, modes or modes_for(C), path, dyadic, marked))


G4 = lambda n, s: ("grid", n, 32, 128, s)          # 1/32 grid over 4 m: indices up to 35
G8 = lambda n, s: ("grid", n, 32, 256, s)          # 1/32 grid over 8 m: indices up to 69

# widths
_cfg("w4", G4(40, 1), 4, 3, path="table only: one float4 per pair")
_cfg("w20", G4(41, 2), 20, 2, "mean", path="table only: 5 of 64 lanes")
_cfg("w16", G4(33, 3), 16, 3, path="split: one K slab")
_cfg("w48", G4(37, 4), 48, 2, "mean", path="split only among the GEMMs: 3 slabs")
_cfg("w32", G4(35, 5), 32, 3, path="fp32: one K slab")
_cfg("w64", G8(50, 6), 64, 3, path="N^2 = 2500, ragged")
_cfg("w128", G8(48, 7), 128, 1, path="N^2 = 2304 = 18 row blocks")
_cfg("w256", G8(45, 8), 256, 3, path="one full column block, N^2 = 2025 ragged")
_cfg("w320", G4(24, 9), 320, 2, path="partial second column block (64 of 256)")
_cfg("w320-mean", G4(19, 10), 320, 3, "mean", path="partial second column block, mean")
_cfg("w512", G4(20, 11), 512, 3, "mean", path="two column blocks")
_cfg("w544", G4(18, 12), 544, 2, path="C > 512: gemm flags reach the fp32 kernel, third column block of 32")
# angle_k and the reduction
_cfg("k0", G4(30, 20), 64, 0, path="no angular term")
_cfg("k1", G4(30, 21), 64, 1, path="reduction over one")
_cfg("k2-max", G4(30, 22), 64, 2)
_cfg("k2-mean", G4(30, 22), 64, 2, "mean")
_cfg("k3-mean", G4(30, 23), 64, 3, "mean")
_cfg("k8-max", G4(31, 24), 64, 8, path="GE_KMAX")
_cfg("k8-mean", G4(31, 24), 64, 8, "mean", path="GE_KMAX, mean")
# sizes
_cfg("n1-k0", G4(1, 30), 32, 0, path="N = 1: one pair")
_cfg("n2-k0", G4(2, 31), 32, 0, path="N = 2")
_cfg("n2-k1", G4(2, 32), 32, 1, path="N = 2 = angle_k + 1")
_cfg("n4-k3", G4(4, 33), 64, 3, "mean", path="N = angle_k + 1: every other point is a neighbour")
_cfg("n9-k8", G4(9, 34), 32, 8, path="N = GE_KMAX + 1")
_cfg("n16", G4(16, 35), 64, 3, path="N^2 = 256: two full row blocks")
_cfg("n128", G8(128, 36), 32, 2, "mean", path="N^2 = 16384: 128 full row blocks")
_cfg("n67", G8(67, 37), 48, 2, path="N^2 = 4489, ragged")
_cfg("demo-n767", G8(767, 38), 32, 1, modes=("table",), path="demo size, default mode (width and k trimmed for time)")
# parameters
_cfg("sigma-dyadic", G8(40, 40), 64, 3, sigma_d=0.25, sigma_a=10, path="sigma_d 1/4: exact distance indices; sigma_a 10")
_cfg("sigma-small", ("grid", 40, 32, 64, 41), 64, 2, "mean", sigma_d=0.05, sigma_a=20, path="sigma_d 0.05 over 2 m, sigma_a 20")
_cfg("sigma-large", G8(40, 42), 32, 3, sigma_d=1.5, sigma_a=45, path="indices below 10, angular indices below 4")
_cfg("weights-x4", G4(36, 43), 64, 3, wscale=4.0, path="weights and biases 4 x the default initialisation")
_cfg("weights-x4-c256", G4(26, 44), 256, 2, "mean", wscale=4.0)
_cfg("weights-x8-c20", G4(30, 45), 20, 3, wscale=8.0)
# table boundaries and large indices (all marked: index > 100)
_cfg("table-edge", ("table_edge",), 64, 2, sigma_d=0.25, marked=True,
     path="distance indices at floor(32 x) = 8190 .. 8193 and beyond: both sides of the table / direct switch")
_cfg("table-edge-c320", ("table_edge",), 320, 3, "mean", sigma_d=0.25, marked=True, path="the switch with two column passes")
_cfg("far-1500", ("grid", 40, 4, 200, 50), 64, 2, sigma_d=0.0625, marked=True,
     path="50 m cloud, indices up to ~1400 < 2^11: direct evaluation / sincos_moderate")
_cfg("far-2800", ("grid", 40, 4, 200, 50), 64, 2, sigma_d=0.03125, marked=True,
     path="indices up to ~2800: workgroups on either side of the 2^11 switch to sincosf")
_cfg("far-2800-c16", ("grid", 40, 4, 200, 50), 16, 3, "mean", sigma_d=0.03125, marked=True, path="the same, one slab")
# ties and degenerate geometry
_cfg("duplicates", ("grid", 32, 32, 128, 60, ((3, 17), (20, 5), (9, 10))), 64, 3,
     path="exact duplicates; rows 17 and 10 drop their lower twin and keep themselves: reference vector 0, atan2(0, 0)")
_cfg("duplicates-mean", ("grid", 32, 32, 128, 60, ((3, 17), (20, 5), (9, 10))), 32, 2, "mean")
_cfg("triplicate-k1", ("grid", 12, 32, 128, 61, ((2, 7), (2, 11))), 32, 1, path="three coincident points, k = 1")
_cfg("lattice-k3", ("lattice", 4, 3, 3, 0.25), 64, 3, path="regular lattice: ties at the k-th neighbour in every row")
_cfg("lattice-k2-mean", ("lattice", 3, 3, 3, 0.5), 32, 2, "mean")
_cfg("lattice-k8", ("lattice", 3, 3, 2, 0.125), 32, 8, path="ties, GE_KMAX")
_cfg("collinear", ("line", 24, 32, 60, 62), 64, 3, path="angles exactly 0 and pi: the top of the angular table")
_cfg("collinear-mean", ("line", 17, 32, 60, 63), 32, 2, "mean", sigma_a=10)
_cfg("coplanar", ("plane", 30, 32, 64, 65), 64, 3, path="every cross product is parallel to one normal")
# generic clouds: fp32 restatement off the diagonal at 5e-5; the float64 figures are recorded only
_cfg("generic-c320", ("generic", 30, 70, (6.0, 5.0, 3.0)), 320, 2, dyadic=False)
_cfg("generic-c48-k8", ("generic", 40, 71, (6.0, 5.0, 3.0)), 48, 8, "mean", dyadic=False)
_cfg("generic-c20", ("generic", 60, 72, (4.0, 4.0, 2.0)), 20, 1, dyadic=False)
_cfg("generic-c512", ("generic", 21, 73, (6.0, 5.0, 3.0)), 512, 3, dyadic=False)

CASES = [Case(f"{c.name}-{m}", c, m) for c in CONFIGS for m in c.modes]
BY_NAME = {c.name: c for c in CONFIGS}

# three clouds of one size for the B = 3 call through the module
BATCH = [("grid", 29, 32, 128, 80), ("grid", 29, 32, 128, 81, ((4, 12),)), ("lattice", 29, 1, 1, 0.125)]
