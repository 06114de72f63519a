"""CPU: the float64 twin of generalised ICP (tests/cloud_gicp_f64.py) against independent statements of the same thing -- Open3D's
written form of the system, a finite-difference gradient, the planted truth of the cases -- and the replay against the
twin's own run and against every planted error.  The covariance twins against their defining properties."""
import functools

import numpy as np
import pytest

import cloud_gicp_cases as C
import cloud_gicp_f64 as G
import cloud_icp_f64 as R0


@functools.lru_cache(maxsize=None)
def f64_run(name, variant=None, max_iterations=None):
    c = C.case(name)
    its = c["max_iterations"] if max_iterations is None else max_iterations
    return G.icp_gicp_f64(c["src"], c["ref"], c["src_cov"], c["ref_cov"], c["T0"], c["max_dist"], its, variant=variant), its


def replay(c, f, its):
    return G.replay(c["src"], c["ref"], c["src_cov"], c["ref_cov"], c["max_dist"], its, 1e-6, 1e-6, f["history"], f["status"],
                    f["iterations"])


def _matched(name):
    c = C.case(name)
    ev = R0.evaluate(c["T0"][:3], c["src"], c["ref"], np.float32(c["max_dist"] ** 2))
    return c, ev


@pytest.mark.parametrize("name", ("aniso", "room_small_rigid"))
def test_system_is_open3d_written_form(name):
    """Open3D: W^(1/2) of the symmetric W = M^-1 by eigh, three rows W^(1/2) J and three residuals W^(1/2) d per pair, JTJ and JTr."""
    c, ev = _matched(name)
    H, g, singular = G.system(c["T0"][:3], c["src"], c["ref"], c["src_cov"], c["ref_cov"], ev)
    assert not singular.any()
    p, d, M, _ = G.pairs(c["T0"][:3], c["src"], c["ref"], c["src_cov"], c["ref_cov"], ev)
    lam, V = np.linalg.eigh(np.linalg.inv(M))
    half = np.einsum("nij,nj,nkj->nik", V, np.sqrt(lam), V)
    J = np.concatenate([-G.cross_matrix(p), np.broadcast_to(np.eye(3), (len(p), 3, 3))], axis=2)
    rows, res = (half @ J).reshape(-1, 6), np.einsum("nij,nj->ni", half, d).ravel()
    JTJ, JTr = rows.T @ rows, rows.T @ res
    assert np.abs(H - JTJ).max() <= 1e-12 * np.abs(JTJ).max() and np.abs(g - JTr).max() <= 1e-12 * np.abs(JTr).max()
    # ... and the rows the twin hands to the eigen solve are these
    A, r = G.rows(c["T0"][:3], c["src"], c["ref"], c["src_cov"], c["ref_cov"], ev)
    assert np.abs(A.T @ A - H).max() <= 1e-12 * np.abs(H).max() and np.abs(A.T @ r - g).max() <= 1e-12 * np.abs(g).max()


def test_gradient_is_the_central_difference_of_the_cost():
    """2 g = d/dx sum d(x)^T W d(x) at x = 0, W held fixed, p(x) = (I + [w]x) p + t to first order (exact rotation used)."""
    c, ev = _matched("aniso")
    T = c["T0"][:3]
    _, g, _ = G.system(T, c["src"], c["ref"], c["src_cov"], c["ref_cov"], ev)
    p, d, M, _ = G.pairs(T, c["src"], c["ref"], c["src_cov"], c["ref_cov"], ev)
    W, q = np.linalg.inv(M), p - d

    def cost(x):
        moved = p @ G.euler(*x[:3]).T + x[3:]
        r = moved - q
        return float(np.einsum("ni,nij,nj->", r, W, r))

    h, grad = 1e-5, np.empty(6)
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        grad[k] = (cost(e) - cost(-e)) / (2 * h)
    assert np.abs(2 * g - grad).max() <= 1e-6 * np.abs(grad).max(), (2 * g, grad)


@pytest.mark.parametrize("name", ("room_rigid", "aniso"))
def test_float64_loop_reaches_the_planted_truth(name):
    c = C.case(name)
    f, _ = f64_run(name)
    start, end = R0.errors(c["T0"], c["T_gt"]), R0.errors(f["transform"], c["T_gt"])
    print(f"{name}: {f['status']} after {f['iterations']} iterations; T0 off by {start[0]:.3f} deg, {start[1]:.4f}; result by {end[0]:.4f} deg, {end[1]:.5f}")
    # the source carries noise of 2 mm; T0 is off by 4 degrees and 5 cm
    assert f["status"] == G.CONVERGED and f["iterations"] <= 12
    assert end[0] <= 0.1 and end[1] <= 0.01 and end[0] < start[0] / 20 and end[1] < start[1] / 5, (start, end)


@pytest.mark.parametrize("name", ("room_small_rigid", "aniso", "singular", "plane", "cut_2", "cut_3", "cut_4", "edge_src_0",
                                  "edge_src_3", "edge_src_129", "edge_ref_1", "disjoint", "between_clusters", "room_far_rigid"))
def test_replay_accepts_the_float64_run(name):
    c = C.case(name)
    f, its = f64_run(name)
    worst, lowest = replay(c, f, its)
    print(f"{name}: {f['status']} after {f['iterations']} iterations, worst error / bound = {worst:.3f}, smallest judged ratio = {lowest:.3g}")
    assert worst <= 0.25      # one rounding of the exact result is 1/8 of the bound; twice that for the translation's norm
    assert (f["iterations"] == 0 and f["status"] == G.DEGENERATE) == (name in C.DEGENERATE_AT_0)
    if name == "plane":        # one wall: point-to-plane refuses it, the plane priors of both clouds fix all six freedoms
        assert f["status"] == G.CONVERGED and f["iterations"] >= 1 and min(f["ratios"]) >= G.JUDGED


@pytest.mark.parametrize("variant", G.VARIANTS)
def test_replay_rejects_every_planted_error(variant):
    name = "singular" if variant == "singular_not_counted" else "aniso"
    c = C.case(name)
    f, its = f64_run(name, variant, 2 if name == "aniso" else None)
    assert f["iterations"] >= 1 or variant == "singular_not_counted"
    with pytest.raises(AssertionError):
        replay(c, f, its)


def test_covariance_twins():
    rng = np.random.default_rng(7)
    n, eps = 300, 1e-3
    normals = rng.normal(size=(n, 3)).astype(np.float32) * rng.uniform(0.1, 5.0, (n, 1)).astype(np.float32)
    normals[0] = 0.0
    cov = G.full(G.covariances_from_normals_f64(normals, eps))
    assert (cov[0] == np.eye(3)).all()
    v = normals[1:].astype(np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    t = np.cross(v, rng.normal(size=(n - 1, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    assert np.abs(np.einsum("nij,nj->ni", cov[1:], v) - eps * v).max() <= 1e-15      # C v = eps v
    assert np.abs(np.einsum("nij,nj->ni", cov[1:], t) - t).max() <= 1e-15            # C t = t for every tangent
    # Gaussians: the plane prior about the thinnest axis of the normalised rotation
    scales = np.exp(rng.uniform(np.log(0.01), np.log(1.0), (n, 3))).astype(np.float32)
    q = (rng.normal(size=(n, 4)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    scales[1] = 0.25                    # equal scales: the first axis
    q[2] = 0.0
    g = G.gs_covariances_f64(scales, q, mode="plane", epsilon=eps)
    assert (g["cov"][2] == [1, 0, 0, 1, 0, 1]).all() and (g["normal"][2] == 0).all() and not g["valid"][2] and g["valid"].sum() == n - 1
    ok = g["valid"]
    R = G.quaternion_matrix(q[ok].astype(np.float64) / np.linalg.norm(q[ok].astype(np.float64), axis=1, keepdims=True))
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14 and np.abs(np.linalg.det(R) - 1).max() <= 1e-14
    axis = np.argmin(scales[ok], axis=1)
    assert axis[1] == 0
    col = R[np.arange(ok.sum()), :, axis]
    nrm = g["normal"][ok]
    assert np.abs(np.abs((col * nrm).sum(1)) - 1).max() <= 1e-14
    assert (nrm[np.arange(len(nrm)), np.argmax(np.abs(nrm), axis=1)] > 0).all()
    C3 = G.full(g["cov"][ok])
    assert np.abs(np.einsum("nij,nj->ni", C3, nrm) - eps * nrm).max() <= 1e-14
    other = R[np.arange(ok.sum()), :, (axis + 1) % 3]
    assert np.abs(np.einsum("nij,nj->ni", C3, other) - other).max() <= 1e-14
    # raw: R S^2 R^T of the rotation as given, within fp32 rounding of a float64 evaluation by another route (eigh)
    unit = (q[ok].astype(np.float64) / np.linalg.norm(q[ok].astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    raw = G.full(G.gs_covariances_f64(scales[ok], unit, scale_modifier=1.5, mode="raw")["cov"])
    lam = np.linalg.eigvalsh(raw)
    want = np.sort((1.5 * scales[ok].astype(np.float64)) ** 2, axis=1)
    assert np.abs(lam - want).max() <= 8 * np.finfo(np.float32).eps * want.max()      # the fp32 quaternion is unit to 1 ulp
    Ru = G.quaternion_matrix(unit.astype(np.float64))
    S2 = np.zeros((ok.sum(), 3, 3))
    S2[:, [0, 1, 2], [0, 1, 2]] = (1.5 * scales[ok].astype(np.float64)) ** 2
    assert np.abs(raw - Ru @ S2 @ Ru.transpose(0, 2, 1)).max() <= 1e-14
