"""CPU: the float64 restatement of point-to-plane ICP (tests/cloud_icp_plane_f64.py) and the replay that judges the GPU,
pinned without a GPU: the solve against numpy.linalg.lstsq, the run against the planted motion, the replay against its own
run and against five planted errors, and the refusal of a single plane."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cloud_icp_f64 as R0
import cloud_icp_plane_cases as P
import cloud_icp_plane_f64 as R


@functools.lru_cache(maxsize=None)
def restated(name):
    c = P.case(name)
    return R.icp_plane_f64(c["src"], c["ref"], c["normals"], c["T0"], c["max_dist"], c["max_iterations"])


def _replay(c, r, max_iterations):
    return R.replay(c["src"], c["ref"], c["normals"], c["max_dist"], max_iterations, 1e-6, 1e-6, r["history"], r["status"],
                    r["iterations"])


def test_eigen_solve_equals_least_squares_and_the_euler_product_is_a_rotation():
    c = P.case("room_rigid")
    ev = R0.evaluate(c["T0"][:3], c["src"], c["ref"], np.float32(c["max_dist"] ** 2))
    A, r = R.rows(c["T0"][:3], c["src"], c["ref"], c["normals"], ev)
    assert A.shape == (ev["n"], 6) and ev["n"] > 1000
    x, ratio = R.solve(A, r)
    want = np.linalg.lstsq(A, -r, rcond=None)[0]
    assert np.abs(x - want).max() <= 1e-10 and ratio >= R.JUDGED
    for angles in (x[:3], (0.3, -1.2, 2.5), (0.0, 0.0, 0.0), (np.pi / 2, np.pi / 2, -np.pi / 2)):
        Q = R.euler(*angles)
        assert np.abs(Q @ Q.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(Q) - 1.0) <= 1e-15
    # Rz Ry Rx: a quarter turn about x, then about z
    assert np.allclose(R.euler(np.pi / 2, 0.0, np.pi / 2) @ [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], atol=1e-15)
    assert np.allclose(R.euler(np.pi / 2, 0.0, np.pi / 2) @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], atol=1e-15)


def test_room_rigid_converges_to_the_planted_motion():
    c, r = P.case("room_rigid"), restated("room_rigid")
    angle, shift, _ = R0.errors(r["transform"], c["T_gt"])
    print(f"room_rigid: {r['status']} after {r['iterations']} iterations, {angle:.4f} deg, {shift:.5f} from T_gt; "
          f"l_min / l_max = {min(r['ratios']):.3g} .. {max(r['ratios']):.3g}")
    assert r["status"] == R.CONVERGED and r["iterations"] <= 10
    assert angle <= 0.05 and shift <= 0.01


@pytest.mark.parametrize("name", ("room_rigid", "room_small_rigid", "cut_7"))
def test_replay_accepts_the_restatement(name):
    c, r = P.case(name), restated(name)
    worst = _replay(c, r, c["max_iterations"])
    assert worst <= 0.5     # one rounding to fp32 is 1/8 of the bound


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_replay_rejects_a_planted_error(variant):
    c = P.case("room_small_rigid")
    r = R.icp_plane_f64(c["src"], c["ref"], c["normals"], c["T0"], c["max_dist"], 2, variant=variant)
    assert r["iterations"] >= 1
    with pytest.raises(AssertionError):
        _replay(c, r, 2)
    r = R.icp_plane_f64(c["src"], c["ref"], c["normals"], c["T0"], c["max_dist"], 2)      # the same arguments without it
    _replay(c, r, 2)


def test_a_single_plane_is_refused_at_the_start():
    c, r = P.case("plane"), restated("plane")
    assert (r["status"], r["iterations"]) == (R.DEGENERATE, 0) and r["history"][0, 12] == c["src"].shape[0]
    ev = R0.evaluate(c["T0"][:3], c["src"], c["ref"], np.float32(c["max_dist"] ** 2))
    A, _ = R.rows(c["T0"][:3], c["src"], c["ref"], c["normals"], ev)
    lam = np.linalg.eigvalsh(A.T @ A)
    assert (lam[:3] == 0.0).all() and lam[3] > 0.0          # rotation about z and the two in-plane shifts are free
    assert (r["transform"] == c["T0"]).all()
    _replay(c, r, c["max_iterations"])


def test_too_few_pairs_and_far_coordinates_are_refused():
    for name, n in (("cut_5", 5), ("cut_6", 6), ("cut_7", 7)):
        r = restated(name)
        assert r["history"][0, 12] == n
        assert (r["iterations"] == 0) == (n < R.MIN_PAIRS), (name, r["iterations"])
    # coordinates of 1000: rotations move every point by thousands, l_min / l_max ~ 1e-14 -- refused, well outside the guard
    c, r = P.case("room_far_rigid"), restated("room_far_rigid")
    assert (r["status"], r["iterations"]) == (R.DEGENERATE, 0) and r["ratios"][0] < R.REFUSE / 10
    _replay(c, r, c["max_iterations"])


def test_example_refuses_a_scale_with_the_plane_estimator():
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    for flags in (["--icp", "--icp_plane", "--icp_scale"], ["--icp_plane"]):
        r = subprocess.run([sys.executable, os.path.join(root, "examples", "register_scenes.py"), "--synthetic"] + flags,
                           capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 2 and "--icp_plane" in r.stderr, (flags, r.stderr[-500:])
