"""Test helper (not collected): the seeded case table of tests/test_gpu_node_correspondences.py, shared with the CPU file
tests/test_training_targets_reference.py, which walks it through the admission rule: on every case the node pairs whose
float64 counts differ between the thresholds r^2 - tau and r^2 + tau (node_corr_f64.py) are at most 1 % of the emitted
pairs, so that all but a sliver of every case is compared bit for bit.

A case is a dict of float32 / bool NumPy arrays: ref_nodes (M,3), src_nodes (N,3), ref_knn_points (M,K,3), src_knn_points
(N,K,3), transform (4,4), pos_radius, and the four masks (or None)."""
import functools
import zlib

import numpy as np

from helpers import load_golden

POS_RADIUS = 0.05
ADMIT = 0.01     # undecided node pairs / emitted node pairs


def numpy_partition(points, nodes, K):
    """point_to_node_partition (pointcloud_partition.py:61-111) in NumPy: every point goes to its nearest node, a node keeps
    the K of its points that are nearest to it.  -> (node_masks (M,), knn_points (M,K,3) padded with zero points,
    knn_masks (M,K))."""
    points, nodes = np.asarray(points, np.float64), np.asarray(nodes, np.float64)
    d2 = ((nodes[:, None, :] - points[None, :, :]) ** 2).sum(-1)             # (M, P)
    owner = d2.argmin(0)
    M = nodes.shape[0]
    knn = np.zeros((M, K, 3), np.float32)
    km = np.zeros((M, K), bool)
    for i in range(M):
        mine = np.nonzero(owner == i)[0]
        mine = mine[np.argsort(d2[i, mine], kind="stable")][:K]
        knn[i, :len(mine)] = points[mine]
        km[i, :len(mine)] = True
    return km.any(1), knn, km


def _rigid(rng, scale=1.0):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3] = scale * q
    T[:3, 3] = rng.uniform(-1.0, 1.0, 3)
    return T


def _to_src(T, p_ref):
    """Points of the source frame that `T` maps onto `p_ref` (float64)."""
    return (p_ref - T[:3, 3]) @ np.linalg.inv(T[:3, :3]).T


def _patches(name, M, N, K, noise=0.02, scale=1.0):
    """Reference patches scattered in a 1 m box (half width 0.12 m, so neighbours overlap in part); source patch j is the
    reference patch j % M moved by `noise` per point, shuffled, in the frame of a random similarity transform."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    T = _rigid(rng, scale)
    ref_nodes = rng.uniform(0.0, 1.0, (M, 3))
    ref_knn = ref_nodes[:, None, :] + rng.uniform(-0.12, 0.12, (M, K, 3))
    pick = np.arange(N) % M
    moved = ref_knn[pick] + rng.normal(0.0, noise, (N, K, 3))
    for j in range(N):
        moved[j] = moved[j][rng.permutation(K)]
    src_nodes = _to_src(T, ref_nodes[pick] + rng.normal(0.0, 0.01, (N, 3)))
    src_knn = _to_src(T, moved)
    f = np.float32
    return dict(ref_nodes=ref_nodes.astype(f), src_nodes=src_nodes.astype(f), ref_knn_points=ref_knn.astype(f),
                src_knn_points=src_knn.astype(f), transform=T.astype(f), pos_radius=POS_RADIUS, ref_masks=None, src_masks=None,
                ref_knn_masks=None, src_knn_masks=None), rng


def _plain(name, M, N, K, **kw):
    return _patches(name, M, N, K, **kw)[0]


def _masked_nodes(name):
    c, rng = _patches(name, 21, 19, 16)
    c["ref_masks"], c["src_masks"] = rng.random(21) < 0.6, rng.random(19) < 0.6
    return c


def _partial_masks(name):
    """Patches padded with zero points behind a false mask, as point_to_node_partition pads them.  The translation is put
    on a reference point, so a padded source point (T 0 = t) would land inside the radius if its mask were ignored, and the
    padded reference points (0) get partners the same way: source points are placed on T^-1 0."""
    c, rng = _patches(name, 11, 9, 24)
    T = c["transform"].astype(np.float64)
    c["ref_knn_points"][0, :3] = (T[:3, 3] + rng.normal(0.0, 0.01, (3, 3))).astype(np.float32)   # next to t = T 0
    c["src_knn_points"][1, :3] = _to_src(T, rng.normal(0.0, 0.01, (3, 3))).astype(np.float32)    # mapped next to 0
    rkm, skm = np.ones((11, 24), bool), np.ones((9, 24), bool)
    for m, pts in ((rkm, c["ref_knn_points"]), (skm, c["src_knn_points"])):
        for i in range(m.shape[0]):
            keep = int(rng.integers(4, 25))
            m[i, keep:] = False
            pts[i, keep:] = 0.0
    c["ref_knn_masks"], c["src_knn_masks"] = rkm, skm
    return c


def _full_masked_patch(name):
    c, rng = _patches(name, 8, 8, 16)
    rkm, skm = np.ones((8, 16), bool), np.ones((8, 16), bool)
    rkm[2] = False          # valid nodes (the node masks stay true) without a valid point
    skm[5] = False
    c["ref_knn_masks"], c["src_knn_masks"] = rkm, skm
    c["ref_masks"], c["src_masks"] = np.ones(8, bool), np.ones(8, bool)
    return c


def _far(name):
    c, _ = _patches(name, 6, 5, 16)
    c["transform"][:3, 3] += 50.0
    return c


def _golden(prefix):
    g = load_golden("training.npz")
    c = {k: g[f"{prefix}_{k}"] for k in ("ref_nodes", "src_nodes", "ref_knn_points", "src_knn_points", "transform", "ref_masks",
                                         "src_masks", "ref_knn_masks", "src_knn_masks")}
    c["pos_radius"] = float(g[f"{prefix}_pos_radius"])
    return c


def _room(name):
    """Two independent samplings of one 4 x 3 x 2.5 m room (gaussreg_amd.pair_pipeline.synthetic_room_pair), about 150
    superpoints a side from a 0.72 m voxel grid, patches of the 64 nearest points; the source is shrunk by 1.25, so the
    transform is a similarity with rotation, translation and scale."""
    import torch
    from gaussreg_amd.pair_pipeline import synthetic_room_pair
    ref, src, T = synthetic_room_pair(7, 20000, torch.device("cpu"))
    ref, src, T = ref.numpy().astype(np.float64), src.numpy().astype(np.float64), T.numpy().astype(np.float64)
    s = 1.25
    src, T = src / s, T.copy()
    T[:3, :3] *= s

    def nodes_of(p, voxel):
        key = np.floor(p / voxel).astype(np.int64)
        _, inv = np.unique(key, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        out = np.zeros((inv.max() + 1, 3))
        np.add.at(out, inv, p)
        return out / np.bincount(inv)[:, None]
    out = dict(transform=T.astype(np.float32), pos_radius=POS_RADIUS)
    for side, p, voxel in (("ref", ref, 0.72), ("src", src, 0.72 / s)):
        nodes = nodes_of(p, voxel)
        nm, knn, km = numpy_partition(p, nodes, 64)
        out[f"{side}_nodes"], out[f"{side}_masks"] = nodes.astype(np.float32), nm
        out[f"{side}_knn_points"], out[f"{side}_knn_masks"] = knn, km
    return out


BUILDERS = {
    "one": lambda n: _plain(n, 1, 1, 1, noise=0.01),
    "k3": lambda n: _plain(n, 9, 7, 3),
    "k64": lambda n: _plain(n, 9, 7, 64),
    "k65": lambda n: _plain(n, 9, 7, 65),
    "k128": lambda n: _plain(n, 9, 7, 128),
    "k129": lambda n: _plain(n, 9, 7, 129),
    "k256": lambda n: _plain(n, 9, 7, 256, scale=0.8),
    "37x5": lambda n: _plain(n, 37, 5, 16),
    "5x70": lambda n: _plain(n, 5, 70, 16),            # more than one block of 64 source nodes per wave
    "masked_nodes": _masked_nodes,
    "partial_masks": _partial_masks,
    "full_masked_patch": _full_masked_patch,
    "far": _far,
    "golden_lattice": lambda n: _golden("nc_lattice"),
    "golden_self": lambda n: _golden("nc_self"),
    "room": _room,
}
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def build(name):
    return BUILDERS[name](name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 restatement of the case, computed once and shared (read-only)."""
    import node_corr_f64
    c = build(name)
    return node_corr_f64.node_correspondences_f64(
        c["ref_nodes"], c["src_nodes"], c["ref_knn_points"], c["src_knn_points"], c["transform"], c["pos_radius"],
        c["ref_masks"], c["src_masks"], c["ref_knn_masks"], c["src_knn_masks"])
