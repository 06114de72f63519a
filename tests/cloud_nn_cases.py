"""The cloud pairs of the cross-cloud nearest-neighbour tests: pair(name) -> (query, support) fp32 numpy, RADII[name] = the
two radii the capped searches and the pair searches use.  The radii are fixed numbers of the order of the point spacing
(small: few rows have a hit; large: most rows have tens), never taken from a result."""
import functools

import numpy as np

from gaussreg_amd import synthetic

RADII = {"tiny_1_1": (0.3, 2.0), "tiny_5_1": (0.3, 2.0), "tiny_5_3": (0.3, 2.0),
         "uniform_257_4097": (0.05, 0.2), "uniform_4097_257": (0.05, 0.2), "half_8192": (0.05, 0.1),
         "same_4096": (0.04, 0.12), "disjoint_4096": (0.05, 0.2),
         "c2_support": (0.1, 0.3), "c2_query": (0.1, 0.3), "blobs": (0.05, 0.2),
         "identical_clouds": (0.0, 0.08), "dyadic": (0.125, 0.25), "one_point_support": (1.0, 5.0),
         "line": (0.1, 0.5), "plane": (0.05, 0.3),
         "outliers_query": (0.05, 0.2), "outliers_support": (0.05, 0.2), "outliers_both": (0.05, 0.2),
         "translated": (0.05, 0.2), "between_clusters": (0.5, 45.0)}
NAMES = tuple(RADII)
TINY = ("tiny_1_1", "tiny_5_1", "tiny_5_3")
BOX = np.array([4.0, 3.0, 2.5]), np.array([0.0, 0.0, 3.0])   # synthetic.gaussians_c2's box: extent, centre


def _outliers(rng, p):
    far = rng.choice(p.shape[0], p.shape[0] // 100 + 1, replace=False)
    p[far[:-1]] *= np.float32(100.0)
    p[far[-1]] = np.float32(1e6)
    return p


def half_pair():
    """The pair the float64 checks are stated for: q first, then s, from default_rng(7)."""
    rng = np.random.default_rng(7)
    q = rng.random((8192, 3))
    s = rng.random((8192, 3)) + [0.5, 0, 0]
    return q.astype(np.float32), s.astype(np.float32)


@functools.lru_cache(maxsize=None)
def pair(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    u = lambda n: rng.random((n, 3)).astype(np.float32)
    if name.startswith("tiny_") or name.startswith("uniform_"):
        nq, ns = map(int, name.split("_")[1:])
        return u(nq), u(ns)
    if name == "half_8192":
        return half_pair()
    if name == "same_4096":
        return u(4096), u(4096)
    if name == "disjoint_4096":
        return u(4096), (u(4096) + np.array([10.0, 0, 0], np.float32)).astype(np.float32)
    if name in ("c2_support", "c2_query"):
        c2 = synthetic.gaussians_c2(8192, seed=4)["means3D"].astype(np.float32)
        box = ((rng.random((4096, 3)) - 0.5) * BOX[0] + BOX[1]).astype(np.float32)
        return (box, c2) if name == "c2_support" else (c2[:4096].copy(), np.concatenate([box, box[::-1] + np.float32(0.01)]))
    if name == "blobs":
        centres = rng.random((6, 3))
        s = centres[rng.integers(0, 6, 8192)] + rng.normal(0.0, 0.02, (8192, 3))
        return u(2048), s.astype(np.float32)
    if name == "identical_clouds":
        s = u(3000)
        return s.copy(), s
    if name == "dyadic":   # a lattice of eighths: exact distances, planted ties, duplicate support points
        lat = lambda n: (rng.integers(0, 32, (n, 3)) / 8.0).astype(np.float32)
        s = lat(2048)
        s[1024:1124] = s[:100]
        return lat(1024), s
    if name == "one_point_support":
        return (u(500) * np.float32(4.0) - np.float32(2.0)), np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (1000, 1))
    if name == "line":
        t = rng.random((1000, 1)).astype(np.float32)
        s = (np.array([[1.0, 2.0, -0.5]], np.float32) + t * np.array([[0.0, 3.0, 0.0]], np.float32)).astype(np.float32)
        return (u(500) * np.float32(3.0) + np.array([0.0, 2.0, -1.5], np.float32)).astype(np.float32), s
    if name == "plane":
        s = u(1000)
        s[:, 2] = 0.75
        return u(500), s
    if name.startswith("outliers_"):
        q, s = u(4096), u(4096)
        if name in ("outliers_query", "outliers_both"):
            q = _outliers(rng, q)
        if name in ("outliers_support", "outliers_both"):
            s = _outliers(rng, s)
        return q, s
    if name == "between_clusters":
        # the support is two unit cubes 100 apart, the queries lie between them: inside the support's box, so only the faces
        # bound their search, and the y and z faces of the 13-cell grid are near while the neighbours are 40 away -- a query
        # whose cell is off-centre in y or z is still unbounded after 8 shells and takes the wave-per-query scan
        s = u(8192)
        s[4096:, 0] += np.float32(100.0)
        q = u(512)
        q[:, 0] = q[:, 0] * np.float32(20.0) + np.float32(40.0)
        return q, s
    if name == "translated":
        return (u(2000) + np.float32(1e4)).astype(np.float32), (u(2000) + np.float32(1e4)).astype(np.float32)
    raise KeyError(name)
