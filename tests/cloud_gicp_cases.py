"""The cloud pairs of the generalised-ICP tests: those of tests/cloud_icp_plane_cases.py with the plane-prior covariances of
the float64 twin's normals for BOTH clouds (k = 8, the point itself included), so the ICP kernels are tested apart from the
normals and covariance kernels; and two pairs of their own:

aniso      room_rigid's reference and 4 097 of its source points with general SPD covariances R S^2 R^T of seeded synthetic
           Gaussians: scales log-uniform in [0.02, 0.6] (ratios <= 30, so cond(M) <= 1e3), random rotations -- every
           off-diagonal entry and the congruence A Cs A^T matter at T0's rotation.
singular   room_rigid with the covariance rows of a fifth of the reference points matched at T0, and of all their source
           partners, set to zero: those pairs have M = 0.

case(name) -> dict(src, ref, src_cov, ref_cov fp32 numpy; T0 (4, 4) fp32; max_dist; max_iterations; T_gt or None)."""
import functools

import numpy as np

import cloud_gicp_f64 as G
import cloud_icp_f64 as R0
import cloud_icp_plane_cases as P
import cloud_normals_f64
import scene_init_f64

EPSILON = 1e-3
ROOM = P.ROOM
CUT = ("cut_2", "cut_3", "cut_4")       # either side of the three pairs the loop needs
EDGES = P.EDGES
OWN = ("aniso", "singular")
ALL = ROOM + EDGES + CUT + ("plane",) + OWN
# What the float64 loop with knn_numpy decides (docs/cloud_gicp_f64_errors.md).  These stop at t = 0 without an update: fewer
# than three pairs, or -- room_far_rigid, coordinates of 1000 -- l_min / l_max = 1.4e-14 of the solve about the origin.
DEGENERATE_AT_0 = ("edge_src_0", "edge_src_1", "edge_src_2", "disjoint", "cut_2", "room_far_rigid")
# In every other case every judged step has l_min / l_max >= JUDGED (the smallest: 4.9e-6, between_clusters), so none is
# judged by its outcome alone.
OUTCOME_ONLY = ()


def _normals(points):
    if points.shape[0] <= 8:               # too few points for eight neighbours
        return np.tile(np.array([[0, 0, 1]], np.float32), (points.shape[0], 1))
    index = scene_init_f64.knn_f32(points, 8)[1]
    return np.ascontiguousarray(cloud_normals_f64.normals_f64(points, points, index, include_self=True)["normal"])


def _prior(points):
    return np.ascontiguousarray(G.covariances_from_normals_f64(_normals(points), EPSILON).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _ref_cov(name):                         # the cut_* cases share room_rigid's reference
    return _prior(_base("room_rigid" if name.startswith("cut_") else name)["ref"])


@functools.lru_cache(maxsize=None)
def _base(name):
    if name.startswith("cut_"):
        c = dict(P._base("cut_7"))
        c["src"] = np.ascontiguousarray(c["src"][:int(name[4:])])
        return c
    return P._base(name)


def _gaussian_covariances(n, seed):
    rng = np.random.default_rng(seed)
    scales = np.exp(rng.uniform(np.log(0.02), np.log(0.6), (n, 3))).astype(np.float32)
    q = rng.normal(size=(n, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(G.gs_covariances_f64(scales, q, mode="raw")["cov"].astype(np.float32))


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "aniso":
        c = P._base("room_rigid")
        src = np.ascontiguousarray(c["src"][::c["src"].shape[0] // 4097][:4097])
        assert src.shape[0] == 4097
        return dict(src=src, ref=c["ref"], src_cov=_gaussian_covariances(4097, 41), ref_cov=_gaussian_covariances(c["ref"].shape[0], 42),
                    T0=c["T0"], T_gt=c["T_gt"], max_dist=c["max_dist"], max_iterations=30)
    if name == "singular":
        c = dict(case("room_rigid"))
        ev = R0.evaluate(c["T0"][:3], c["src"], c["ref"], np.float32(c["max_dist"] ** 2))
        hit = np.unique(ev["j"][ev["j"] >= 0])[::5]
        src_cov, ref_cov = c["src_cov"].copy(), c["ref_cov"].copy()
        ref_cov[hit] = 0.0
        src_cov[np.isin(ev["j"], hit)] = 0.0
        return dict(c, src_cov=src_cov, ref_cov=ref_cov, hit=hit, max_iterations=1)
    c = _base(name)
    its = 12 if name == "room_small_rigid" else 30 if name in ROOM + CUT + ("plane",) else 0 if name.startswith("edge_ref_") \
        else P.EDGE_ITERATIONS
    return dict(src=c["src"], ref=c["ref"], src_cov=_prior(c["src"]), ref_cov=_ref_cov(name), T0=c["T0"], T_gt=c.get("T_gt"),
                max_dist=c["max_dist"], max_iterations=its)
