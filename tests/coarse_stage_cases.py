"""Test helper (not collected): the seeded case tables of tests/test_gpu_coarse_stage_f64.py, shared with the CPU file
tests/test_coarse_stage_f64_reference.py, which walks both tables through their admission rules.

Pairwise distance (csrc/superpoint_matching.hip).  Three kernels: pairwise_kernel (64 x 64 tiles) below 192 tiles of
128 x 128 over the whole batch, pairwise_big_kernel from there on, in its ALIGNED instantiation (C % 16 == 0 and 16-byte
pointers) or not, and inside the latter the `vec` branch (C % 4 == 0, 16-byte pointers) or the scalar one.  `kernel_of`
restates that choice; every case names the kernel it is meant for and the CPU file checks the two against each other.
Bound: |gpu - f64| <= PD_BOUND * s_ij, s_ij = |x_i|^2 + |y_j|^2, or 2 + 2 |x_i| |y_j| when `normalized`.
PD_BOUND is four times the worst float32 figure of this table (the admission rule of this project: the float32
restatement lies within 0.25 of the bound), the float32 figure being the larger of the reference's own expression in
torch float32 and the ascending-k chain the kernels compute; see PD_F32_WORST.  It may not exceed 1e-5, the tolerance
tests/test_gpu_matching.py applies to this operator.

Point to node (csrc/point_to_node.hip).  A decision -- which of two nodes owns a point, which of two members comes first
-- is clear when its float64 gap exceeds 2 * PD_BOUND * (|node|^2 + |p|^2): each of the two distances is the same expanded
form and may be off by the pairwise bound.  Clear decisions are compared exactly, unclear ones as sets
(coarse_stage_f64.compare_partition).  Caps: a planted case has no unclear decision at all (its exact ties are bit-equal
operands, which any arithmetic orders by index); the room case at most 1 % of its points and 2 % of its rows.  The
float32 oracle (oracle/matching_np.py) must pass the same comparison before a kernel is called."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import coarse_stage_f64 as F

# worst |f32 - f64| / s_ij over PD_CASES x normalized 0 / 1, measured on the CPU by test_every_pairwise_case_is_admitted
# (torch float32: PD_F32_TORCH; ascending-k chain: PD_F32_CHAIN); the bound is four times the larger
PD_F32_TORCH = 3.58e-7
PD_F32_CHAIN = 9.68e-7
PD_F32_WORST = max(PD_F32_TORCH, PD_F32_CHAIN)
PD_BOUND = 4.0 * PD_F32_WORST
assert PD_BOUND <= 1e-5

PB_T, PB_K, PD_SWITCH = 128, 16, 192  # superpoint_matching.hip: big tile, its k-slab, pd_use_big's tile count


def _seed(name):
    return zlib.crc32(name.encode())


def kernel_of(B, n, m, C, aligned16=True):
    """The kernel gr_pairwise_distance_batch launches (and the branch its fetch takes)."""
    if -(-n // PB_T) * -(-m // PB_T) * B < PD_SWITCH:
        return "small"
    if C % PB_K == 0 and aligned16:
        return "big_aligned"
    return "big_vec" if C % 4 == 0 and aligned16 else "big_scalar"


# kind: "gauss" N(0,1) rows -- with normalized=True these are the un-normalised rows whose xy exceeds 1, so the clamp fires;
#       "unit" unit rows, every 7th row of y an exact copy of a row of x;
#       "room" (C = 3) coordinates in [0, 4)^3, y = x rows moved by 1e-3, every 5th an exact copy: heavy cancellation
PdCase = namedtuple("PdCase", "name kernel B n m C kind channel_first misaligned")


def _pd(kernel, B, n, m, C, kind="gauss", channel_first=False, misaligned=False, tag=""):
    name = f"{kernel}_{B}x{n}x{m}x{C}_{kind}{tag}"
    return PdCase(name, kernel, B, n, m, C, kind, channel_first, misaligned)


def _pd_table():
    t = []
    for (B, n, m, C), kinds in (((1, 1, 1, 1), ("gauss", "unit")), ((1, 64, 64, 32), ("gauss", "unit")),
                                ((1, 65, 63, 33), ("gauss", "unit")), ((1, 31, 97, 3), ("gauss", "room")),
                                ((1, 200, 130, 256), ("gauss", "unit")), ((1, 40, 50, 1024), ("gauss", "unit")),
                                ((191, 5, 7, 20), ("gauss", "unit"))):
        t += [_pd("small", B, n, m, C, k) for k in kinds]
    t.append(_pd("small", 3, 50, 70, 17, "gauss", channel_first=True, tag="_cf"))
    for C in (15, 16, 17, 20, 31, 32, 33):
        kern = kernel_of(192, 5, 7, C)
        t += [_pd(kern, 192, 5, 7, C, "gauss"), _pd(kern, 192, 5, 7, C, "unit")]
    t += [_pd("big_aligned", 192, 128, 128, 32, "unit"), _pd("big_aligned", 96, 129, 128, 48, "gauss"),
          _pd("big_aligned", 192, 127, 1, 16, "gauss"), _pd("big_aligned", 192, 1, 129, 16, "unit"),
          _pd("big_aligned", 1, 1700, 1700, 16, "gauss"), _pd("big_scalar", 1, 1665, 1700, 3, "room"),
          _pd("big_vec", 2, 1300, 1200, 36, "unit"),
          # C % 16 == 0, yet x and y start one float into their storage: neither ALIGNED nor vec
          _pd("big_scalar", 192, 5, 7, 16, "gauss", misaligned=True, tag="_off4")]
    return t


PD_CASES = _pd_table()
PD_BY_NAME = {c.name: c for c in PD_CASES}
assert len(PD_BY_NAME) == len(PD_CASES)
PD_NAN_CASES = ["small_1x65x63x33_gauss", "big_aligned_192x5x7x16_gauss", "big_vec_192x5x7x20_gauss",
                "big_scalar_192x5x7x17_gauss", "big_aligned_96x129x128x48_gauss"]


def build_pairwise(case):
    """-> x (B, n, C), y (B, m, C) float32, channel-last (the test transposes for channel_first)."""
    rng = np.random.default_rng(_seed(case.name))
    B, n, m, C = case.B, case.n, case.m, case.C
    if case.kind == "room":
        x = rng.random((B, n, C)) * 4.0
        y = x[:, rng.integers(0, n, m)] + rng.normal(0, 1e-3, (B, m, C))
        x, y = x.astype(np.float32), y.astype(np.float32)
        src = rng.integers(0, n, m)
        y[:, ::5] = x[:, src[::5]]
    else:
        x, y = rng.normal(size=(B, n, C)), rng.normal(size=(B, m, C))
        if case.kind == "unit":
            x /= np.linalg.norm(x, axis=-1, keepdims=True)
            y /= np.linalg.norm(y, axis=-1, keepdims=True)
        x, y = x.astype(np.float32), y.astype(np.float32)
        if case.kind == "unit":
            src = rng.integers(0, n, m)
            y[:, ::7] = x[:, src[::7]]
    return x, y


def pairwise_ratio(got, want, scale):
    """max |got - want| / (PD_BOUND * s_ij); inf if an entry is not finite or negative."""
    got = np.asarray(got, np.float64)
    if not (np.isfinite(got).all() and (got >= 0).all()):
        return np.inf
    return float((np.abs(got - want) / scale).max() / PD_BOUND) if got.size else 0.0


@functools.lru_cache(maxsize=None)
def pairwise_reference(name, normalized):
    """-> (x, y, float64 result, s_ij); read-only."""
    x, y = build_pairwise(PD_BY_NAME[name])
    want, scale = F.pairwise_distance(x, y, normalized), F.pairwise_scale(x, y, normalized)
    for a in (x, y, want, scale):
        a.setflags(write=False)
    return x, y, want, scale


def pairwise_f32_figures(name, normalized):
    """-> (torch float32, ascending-k chain): worst |f32 - f64| / s_ij, not divided by the bound."""
    x, y, want, scale = pairwise_reference(name, normalized)
    return tuple(float((np.abs(fn(x, y, normalized).astype(np.float64) - want) / scale).max())
                 for fn in (F.pairwise_fp32_torch, F.pairwise_fp32_chain))


# ================================================================================================== point to node
def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def grid_sites(M):
    """The M half-integer grid points nearest the origin, nearest first (ties: lexicographic)."""
    r = np.arange(-10, 10) + 0.5
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    order = np.lexsort((g[:, 2], g[:, 1], g[:, 0], (g * g).sum(1)))
    return g[order[:M]]


def _ladder(rng, c):
    """c squared distances on a uniform ladder over [0.001, 0.081], shuffled."""
    d2 = 0.001 + 0.08 * (np.arange(c) / max(c - 1, 1))
    return rng.permutation(d2)


PLANTED_COUNTS = [2047, 2048, 2049, 3968, 3969, 63, 64, 65, 127, 128, 129, 1, 0, 0]
PLANTED_SLOTS = {4: 1023, 3: 1024, 2: 2048, 1: 0, 0: 1025}  # site -> node index, the five largest


def _plant(rng, sites, counts, slots):
    """Members at site + sqrt(d2) u with d2 on the site's ladder (< 0.081: every other site is at least 0.51 away); points
    and nodes shuffled, then the sites of `slots` moved to the node indices given.  -> points, nodes (float32), the planted
    owner of every point."""
    M = len(sites)
    pts, own = [], []
    for s, c in enumerate(counts):
        pts.append(sites[s] + np.sqrt(_ladder(rng, c))[:, None] * _unit(rng, c))
        own.append(np.full(c, s))
    pts, own = np.concatenate(pts), np.concatenate(own)
    perm = rng.permutation(len(pts))
    pts, own = pts[perm], own[perm]
    where = rng.permutation(M)                      # where[s] = node index of site s
    for s, slot in slots.items():
        other = int(np.nonzero(where == slot)[0][0])
        where[other], where[s] = where[s], slot
    nodes = np.empty((M, 3))
    nodes[where] = sites
    return pts.astype(np.float32), nodes.astype(np.float32), where[own]


# The room cloud seeded by its name has 14 unclear points and 44 rows with an unclear position (cap: 30 rows); it was reseeded,
# by these float64 CPU figures alone: seven further seeds gave 26 .. 32 rows, "/1" is the first of them and gives 7 and 28.
RESEEDED = {"room": "/1"}


@functools.lru_cache(maxsize=None)
def cloud(name):
    """-> (points (N, 3), nodes (M, 3)) float32, read-only.
    planted   2049 nodes, about 17.7 k points: node sizes at every edge of select_kernel's three regimes, the large nodes
              at indices in the first, second and third LDS round of assign_kernel
    ties      44 nodes: points repeated inside a one-wave node, an LDS-sort node and a multi-round node; two nodes repeated
              at higher indices
    room      1500 nodes sampled from 6000 random points of a room centred on the origin
    small3    130 points / 3 nodes;  nonodes  40 points / no node;  empty;  n1030  1030 nodes (two LDS rounds)"""
    rng = np.random.default_rng(_seed("p2n_" + name + RESEEDED.get(name, "")))
    if name == "planted":
        M = 2049
        counts = PLANTED_COUNTS + [int(v) for v in rng.integers(0, 4, M - len(PLANTED_COUNTS))]
        pts, nodes, _ = _plant(rng, grid_sites(M), counts, PLANTED_SLOTS)
    elif name == "ties":
        M = 40
        counts = [2100, 70, 40] + [int(v) for v in rng.integers(0, 30, M - 3)]
        pts, nodes, own = _plant(rng, grid_sites(M), counts, {0: 17, 1: 3, 2: 30})
        for node, reps in ((17, 9), (3, 5), (30, 5)):        # repeat members of the three nodes, at scattered indices
            mem = np.nonzero(own == node)[0]
            srcs = rng.choice(mem, reps, replace=False)
            extra = np.repeat(pts[srcs], rng.integers(1, 4, reps), axis=0)
            at = np.sort(rng.integers(0, len(pts), len(extra)))
            pts, own = np.insert(pts, at, extra, axis=0), np.insert(own, at, node)
        nodes = np.concatenate([nodes, nodes[[17, 3]], nodes[[17]], grid_sites(M + 1)[-1:].astype(np.float32)])
    elif name == "room":
        pts = ((rng.random((6000, 3)) - 0.5) * [4.0, 3.0, 2.5]).astype(np.float32)
        nodes = pts[rng.permutation(6000)[:1500]] + rng.normal(0, 0.02, (1500, 3)).astype(np.float32)
    elif name == "small3":
        pts, nodes, _ = _plant(rng, grid_sites(3), [70, 59, 1], {})
    elif name == "nonodes":
        pts, nodes = rng.random((40, 3)).astype(np.float32), np.zeros((0, 3), np.float32)
    elif name == "empty":
        pts, nodes = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
    elif name == "n1030":
        M = 1030
        counts = [int(v) for v in rng.integers(0, 5, M)]
        counts[0], counts[1] = 300, 200
        pts, nodes, _ = _plant(rng, grid_sites(M), counts, {0: 1029, 1: 1024})
    else:
        raise KeyError(name)
    pts.setflags(write=False)
    nodes.setflags(write=False)
    return pts, nodes


# name -> (cloud, the point_limit values it runs with, cap on unclear points, cap on rows not compared position by position)
P2N_CASES = {"planted": ("planted", (128, 1, 64, 1024, 1000), 0.0, 0.0),
             "ties": ("ties", (32, 1, 128, 1024), 0.0, 0.0),
             "room": ("room", (64,), 0.01, 0.02),
             "n1030": ("n1030", (128,), 0.0, 0.0),
             "small3": ("small3", (128,), 0.0, 0.0)}
STACK = ("planted", "small3", "nonodes", "empty", "n1030")
STACK_K = 128


@functools.lru_cache(maxsize=None)
def p2n_reference(name):
    pts, nodes = cloud(P2N_CASES[name][0])
    return F.partition(pts, nodes)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle import matching_np as M
    pts, nodes = cloud(P2N_CASES[name][0])
    K = min(max(P2N_CASES[name][1]), pts.shape[0])
    return M.point_to_node_partition(pts, nodes, K)[:4]


def p2n_check(name, K, got):
    """compare_partition under the case's caps -> (unclear points, loose rows)."""
    cname, _, cap_p, cap_r = P2N_CASES[name]
    pts, nodes = cloud(cname)
    ref = p2n_reference(name)
    unclear, loose = F.compare_partition(got, pts, nodes, ref, K, PD_BOUND)
    assert unclear <= cap_p * ref["N"], f"{name}: {unclear} of {ref['N']} points are unclear (cap {cap_p:g})"
    assert loose <= cap_r * ref["M"], f"{name}: {loose} of {ref['M']} rows are not compared position by position (cap {cap_r:g})"
    return unclear, loose


@functools.lru_cache(maxsize=None)
def p2n_admitted(name, K):
    """The float32 oracle alone passes the comparison (a row of the oracle at K is its row at the largest K, cut)."""
    p2n, masks, idx, kmask = _oracle(name)
    return p2n_check(name, K, (p2n, masks, np.ascontiguousarray(idx[:, :K]), np.ascontiguousarray(kmask[:, :K])))
