"""CPU: the float64 restatement of ICP (tests/cloud_icp_f64.py) and the replay that judges the GPU, pinned without a GPU:
against a plain float64 ICP over scipy's cKDTree, and against planted errors that the replay has to reject."""
import functools

import numpy as np
import pytest

import cloud_icp_cases as C
import cloud_icp_f64 as R
import cloud_nn_cases


@functools.lru_cache(maxsize=None)
def restated(name):
    c = C.case(name)
    return R.icp_f64(c["src"], c["ref"], c["T0"], c["max_dist"], c["with_scale"])


def _kdtree_icp(src, ref, T0, max_dist, with_scale, max_iterations=30, tol=1e-6):
    """Plain ICP, float64 throughout: transform, nearest neighbour within max_dist from a k-d tree, Umeyama, the stop rule."""
    from scipy.spatial import cKDTree
    src, ref = src.astype(np.float64), ref.astype(np.float64)
    tree = cKDTree(ref)
    T, prev = np.asarray(T0, np.float64)[:3].copy(), None
    for t in range(max_iterations + 1):
        dist, j = tree.query(src @ T[:, :3].T + T[:, 3], k=1, distance_upper_bound=max_dist)
        m = np.isfinite(dist)
        now = (m.sum() / src.shape[0], np.sqrt((dist[m] ** 2).sum() / m.sum()))
        if prev and abs(now[0] - prev[0]) < tol and abs(now[1] - prev[1]) < tol:
            return T, t
        if t == max_iterations:
            return T, t
        T, prev = R.umeyama_f64(src[m], ref[j[m]], with_scale)[0], now


@pytest.mark.parametrize("name", ("room_small", "room_sim"))
def test_restatement_agrees_with_a_plain_float64_icp(name):
    pytest.importorskip("scipy.spatial")
    c, r = C.case(name), restated(name)
    T, t = _kdtree_icp(c["src"], c["ref"], c["T0"], c["max_dist"], c["with_scale"])
    assert r["status"] == R.CONVERGED and r["iterations"] == t
    assert np.abs(r["transform"][:3].astype(np.float64) - T).max() <= 1e-6


@pytest.mark.parametrize("name", ("room_small", "lattice_exact"))
def test_replay_accepts_the_restatement(name):
    c, r = C.case(name), restated(name)
    worst = R.replay(c["src"], c["ref"], c["with_scale"], c["max_dist"], 30, 1e-6, 1e-6, r["history"], r["status"], r["iterations"])
    assert worst <= 0.5     # one rounding to fp32 is 1/8 of the bound


def test_room_cases_converge_to_the_planted_motion():
    for name in ("room_small", "room_sim"):
        c, r = C.case(name), restated(name)
        before, after = R.errors(c["T0"], c["T_gt"]), R.errors(r["transform"], c["T_gt"])
        assert r["status"] == R.CONVERGED and after[0] < 0.1 * before[0] and after[1] < 0.2 * before[1], (name, before, after)


def test_lattice_is_exact():
    c, r = C.case("lattice_exact"), restated("lattice_exact")
    assert r["status"] == R.CONVERGED and r["iterations"] == 1
    assert r["history"][0, 12] == c["src"].shape[0] and r["history"][0, 13] == 0.0
    first = R.evaluate(c["T0"][:3], c["src"], c["ref"], np.float32(c["max_dist"] ** 2))
    assert (first["d"] == 0).all() and (first["j"][:34] <= np.arange(0, 100, 3)).all()    # duplicates: the lower j


# (variant, case, arguments): a case on which the planted error changes the run
def _dyadic():
    q, s = cloud_nn_cases.pair("dyadic")     # eighths: distances of exactly 1/8 = the cap
    return dict(src=q, ref=s, T0=np.eye(4, dtype=np.float32), max_dist=0.125, with_scale=False)


PLANTED = {"wrong_association": ("room_small", {}),
           "strict_cap": ("dyadic", dict(max_iterations=2)),
           "scale_in_rigid": ("room_small", dict(with_scale=False)),
           "stop_on_fitness_only": ("room_small", dict(relative_fitness=1.0)),
           "composed_increments": ("room_far", {})}     # coordinates of 1000: an fp32 product of transforms loses the bound at once


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_replay_rejects_a_planted_error(variant):
    name, kw = PLANTED[variant]
    c = _dyadic() if name == "dyadic" else C.case(name)
    args = dict(with_scale=c["with_scale"], max_iterations=30, relative_fitness=1e-6, relative_rmse=1e-6)
    args.update(kw)
    r = R.icp_f64(c["src"], c["ref"], c["T0"], c["max_dist"], variant=variant, **args)
    with pytest.raises(AssertionError):
        R.replay(c["src"], c["ref"], args["with_scale"], c["max_dist"], args["max_iterations"], args["relative_fitness"],
                 args["relative_rmse"], r["history"], r["status"], r["iterations"])
    if name != "room_far":      # ... and the same arguments without the error pass (room_far: by the GPU test, it takes seconds)
        r = R.icp_f64(c["src"], c["ref"], c["T0"], c["max_dist"], **args)
        R.replay(c["src"], c["ref"], args["with_scale"], c["max_dist"], args["max_iterations"], args["relative_fitness"],
                 args["relative_rmse"], r["history"], r["status"], r["iterations"])
