"""The cloud pairs of the ICP tests: case(name) -> dict(src, ref fp32 numpy; T0 (4, 4) fp32; max_dist; with_scale; and T_gt
(4, 4) float64 where there is a planted truth).  Fixed seeds throughout; nothing here is taken from a result."""
import functools

import numpy as np

import cloud_nn_cases

ROOM = ("room_sim", "room_rigid", "room_small", "room_far")
EDGE_SRC = (0, 1, 2, 3, 127, 128, 129, 257, 4097)


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def similarity(R, t, s=1.0):
    T = np.eye(4)
    T[:3, :3] = s * np.asarray(R, np.float64)
    T[:3, 3] = t
    return T


def apply64(T, p):
    return np.asarray(p, np.float64) @ T[:3, :3].T + T[:3, 3]


def _box_surface(rng, n, lo, hi):
    """n points on the surface of the box [lo, hi], area-weighted over its six faces."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    e = hi - lo
    area = np.array([e[1] * e[2], e[1] * e[2], e[0] * e[2], e[0] * e[2], e[0] * e[1], e[0] * e[1]])
    face = rng.choice(6, n, p=area / area.sum())
    p = lo + rng.random((n, 3)) * e
    axis, side = face // 2, face % 2
    p[np.arange(n), axis] = np.where(side == 0, lo[axis], hi[axis])
    return p


def room_points(n, seed):
    """A 4 x 3 x 2.5 room and a 1 x 0.6 x 0.8 box in its corner at the origin: 5/6 of the points on the room, 1/6 on the box."""
    rng = np.random.default_rng(seed)
    nb = n // 6
    return np.concatenate([_box_surface(rng, n - nb, (0, 0, 0), (4.0, 3.0, 2.5)),
                           _box_surface(rng, nb, (0, 0, 0), (1.0, 0.6, 0.8))])


def _room(n, scale, max_dist, shift=0.0, perturbation=1.0, seed=11):
    rng = np.random.default_rng(seed + 1)
    pts = room_points(n, seed)
    ref = pts[pts[:, 0] < 2.6] + shift
    part = pts[pts[:, 0] > 1.4]
    part = part + rng.normal(0.0, 0.002, part.shape) + shift
    T_gt = similarity(rotation((1, 2, 3), 25.0), (0.5, -0.3, 0.2), scale)
    if shift:   # the same motion about the shifted origin, so that the pair is room_sim moved as a whole
        T_gt[:3, 3] += shift - T_gt[:3, :3] @ np.full(3, shift)
    src = apply64(np.linalg.inv(T_gt), part)
    c = ref.mean(0)
    sp = 1.0 + (0.02 if scale != 1.0 else 0.0) * perturbation
    P = similarity(rotation((3, -1, 2), 4.0 * perturbation), np.zeros(3), sp)
    P[:3, 3] = c - P[:3, :3] @ c + np.array([0.04, -0.03, 0.02]) * perturbation
    T0 = (P @ T_gt).astype(np.float32)
    T0[3] = (0, 0, 0, 1)
    return dict(src=np.ascontiguousarray(src, np.float32), ref=np.ascontiguousarray(ref, np.float32), T0=T0, T_gt=T_gt,
                max_dist=max_dist, with_scale=scale != 1.0)


def _uniform(n_src, n_ref, seed, max_dist=0.2):
    rng = np.random.default_rng(seed)
    ref = rng.random((n_ref, 3)).astype(np.float32)
    src = (rng.random((n_src, 3)) * 0.9 + 0.05).astype(np.float32)
    T0 = similarity(rotation((1, 1, 0), 2.0), (0.01, -0.02, 0.015)).astype(np.float32)
    return dict(src=src, ref=ref, T0=T0, T_gt=None, max_dist=max_dist, with_scale=False)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "room_sim":
        return _room(12288, 1.25, 0.1)
    if name == "room_rigid":
        return _room(12288, 1.0, 0.1)
    if name == "room_small":
        return _room(1500, 0.8, 0.25)
    if name == "room_far":
        return _room(12288, 1.25, 0.1, shift=1000.0, perturbation=0.5)
    if name == "lattice_exact":
        # eighths in [0, 4)^3 with duplicates in ref; src = every third ref point taken back through the exact similarity
        # x -> 2 Rz(90 deg) x + t: every product and sum of the fp32 transform is exact, so every d is exactly 0
        rng = np.random.default_rng(5)
        ref = (rng.integers(0, 32, (2048, 3)) / 8.0).astype(np.float32)
        ref[1024:1124] = ref[:100]
        Rq = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        t = np.array([0.5, -1.25, 2.0])
        T = similarity(Rq, t, 2.0)
        pick = ref[1024:1124:3].astype(np.float64)          # duplicates: the tie goes to the lower j
        pick = np.concatenate([pick, ref[::3].astype(np.float64)])
        src = ((pick - t) @ Rq) / 2.0                       # Rq^T (p - t) / 2, exact
        assert (apply64(T, src) == pick).all()
        return dict(src=np.ascontiguousarray(src, np.float32), ref=ref, T0=T.astype(np.float32), T_gt=T, max_dist=0.25,
                    with_scale=True)
    if name.startswith("edge_src_"):
        return _uniform(int(name.split("_")[2]), 4097, 21)
    if name.startswith("edge_ref_"):           # a one-cell grid
        return _uniform(300, int(name.split("_")[2]), 22, max_dist=2.0)
    if name == "disjoint":                    # nothing within the cap: n = 0
        d = _uniform(500, 1000, 23, max_dist=0.05)
        d["ref"] = (d["ref"] + np.float32(10.0)).astype(np.float32)
        return d
    if name == "collinear":                   # matched points on one line, with scale
        rng = np.random.default_rng(24)
        t = rng.random((400, 1))
        ref = (np.array([[1.0, 2.0, -0.5]]) + t * np.array([[0.6, 3.0, -1.2]])).astype(np.float32)
        s = rng.random((200, 1))
        src = (np.array([[1.0, 2.0, -0.5]]) + s * np.array([[0.6, 3.0, -1.2]])).astype(np.float32)
        T0 = similarity(np.eye(3), (0.01, 0.0, -0.01)).astype(np.float32)
        return dict(src=src, ref=ref, T0=T0, T_gt=None, max_dist=0.3, with_scale=True)
    if name == "between_clusters":
        # cloud_nn_cases' pair: queries between two far clusters stay unbounded after MAX_SHELLS shells; the cap of 45
        # lets them match, so they take the wave-per-query scan AND enter the sums
        q, s = cloud_nn_cases.pair("between_clusters")
        return dict(src=q, ref=s, T0=np.eye(4, dtype=np.float32), T_gt=None, max_dist=45.0, with_scale=False)
    raise KeyError(name)


EDGES = tuple(f"edge_src_{n}" for n in EDGE_SRC) + ("edge_ref_1", "edge_ref_2", "disjoint", "collinear", "between_clusters")
