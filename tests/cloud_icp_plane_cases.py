"""The cloud pairs of the point-to-plane tests: those of tests/cloud_icp_cases.py, rigid throughout, with the float64 twin's
normals of the reference (k = 8, the point itself included) -- so the ICP kernels are tested apart from the normals kernel.
case(name) -> dict(src, ref, normals fp32 numpy; T0 (4, 4) fp32; max_dist; max_iterations; T_gt or None)."""
import functools

import numpy as np

import cloud_icp_cases as C
import cloud_normals_f64
import scene_init_f64

EDGE_ITERATIONS = 6
ROOM = ("room_rigid", "room_small_rigid", "room_far_rigid")
CUT = ("cut_5", "cut_6", "cut_7")       # either side of the six pairs the solve needs
EDGES = tuple(f"edge_src_{n}" for n in C.EDGE_SRC) + ("edge_ref_1", "edge_ref_2", "disjoint", "between_clusters")


@functools.lru_cache(maxsize=None)
def _twin_normals(name):
    ref = _base(name)["ref"]
    if ref.shape[0] <= 8:                  # too few points for eight neighbours: these cases are pure evaluations
        return np.tile(np.array([[0, 0, 1]], np.float32), (ref.shape[0], 1))
    index = scene_init_f64.knn_f32(ref, 8)[1]
    return np.ascontiguousarray(cloud_normals_f64.normals_f64(ref, ref, index, include_self=True)["normal"])


@functools.lru_cache(maxsize=None)
def _base(name):
    if name == "room_small_rigid":        # sparse: float64 settles into a 2-cycle between two correspondence sets here
        return C._room(1500, 1.0, 0.25)
    if name == "room_far_rigid":          # room_far's rigid analogue: coordinates of 1000
        return C._room(12288, 1.0, 0.1, shift=1000.0, perturbation=0.5)
    if name.startswith("cut_"):
        c = dict(C.case("room_rigid"))
        # every 613th point: spread over enough faces that six of them fix a motion (l_min / l_max = 1.2e-6 in float64);
        # the cap lets every one of them find a partner, so n = 5, 6, 7
        c["src"] = np.ascontiguousarray(c["src"][::613][:int(name[4:])])
        c["max_dist"] = 2.0
        return c
    if name == "plane":                   # one exact plane: three eigenvalues of H are exactly 0
        rng = np.random.default_rng(31)
        ref = np.zeros((2000, 3), np.float32)
        ref[:, :2] = (rng.integers(0, 1024, (2000, 2)) / 256.0).astype(np.float32)
        src = np.ascontiguousarray(ref[::3] + np.array([0.0, 0.0, 0.0625], np.float32))
        return dict(src=src, ref=ref, T0=np.eye(4, dtype=np.float32), T_gt=None, max_dist=0.25, with_scale=False)
    return C.case(name)


@functools.lru_cache(maxsize=None)
def case(name):
    c = _base(name)
    its = 12 if name == "room_small_rigid" else 30 if name in ROOM + CUT + ("plane",) else 0 if name.startswith("edge_ref_") \
        else EDGE_ITERATIONS
    normals = np.tile(np.array([[0, 0, 1]], np.float32), (c["ref"].shape[0], 1)) if name == "plane" else _twin_normals(name)
    return dict(src=c["src"], ref=c["ref"], normals=normals, T0=c["T0"], T_gt=c.get("T_gt"), max_dist=c["max_dist"],
                max_iterations=its)
