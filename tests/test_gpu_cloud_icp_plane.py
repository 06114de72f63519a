"""GPU: point-to-plane ICP (gaussreg_amd.icp.icp_point_to_plane, csrc/cloud_icp_plane.hip) against the step-by-step replay of
tests/cloud_icp_plane_f64.py.

As in tests/test_gpu_cloud_icp.py trajectories never have to agree: for every recorded t the GPU's own T_t is taken from
`history`, E(T_t) is recomputed with the numpy fp32 transform and cloud_nn.knn, U(T_t) is computed in float64 and the GPU's
T_(t+1) has to lie within 4 fp32 ulps of 1 (rotation block) and of |dt| + |t_t| (translation); the stop decision is checked
against the rule at every t.  The reference normals come from the float64 twin of the normals kernel, so the two kernels are
tested apart; one case runs estimate_normals end to end.  Measured figures: docs/cloud_icp_plane_f64_errors.md."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_icp_f64 as R0
import cloud_icp_plane_cases as P
import cloud_icp_plane_f64 as R
import gaussreg_amd
from gaussreg_amd import _lib, cloud_nn
from gaussreg_amd.icp import evaluate_registration, icp_point_to_plane
from gaussreg_amd.normals import estimate_normals

pytestmark = pytest.mark.gpu

_dev = {}


def dev(a):
    """One device copy per numpy array (the cases are cached and never written)."""
    key = id(a)
    if key not in _dev:
        _dev[key] = (a, torch.from_numpy(a).cuda())
    return _dev[key][1]


def gpu_knn(p, ref, cap):
    """The k = 1 capped search of the replay on the kernels of cloud_nn.hip: (d (N,) fp32, j (N,) int64) numpy."""
    d, j = cloud_nn._knn(torch.from_numpy(np.ascontiguousarray(p)).cuda(), dev(ref), 1, float(np.float32(cap)))
    return d[:, 0].cpu().numpy(), j[:, 0].cpu().numpy()


def same_bits(a, b):
    view = lambda x: x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(view(a), view(b))


def run(c, **kw):
    args = dict(max_dist=c["max_dist"], max_iterations=c["max_iterations"], return_correspondences=True, return_history=True)
    args.update(kw)
    return icp_point_to_plane(dev(c["src"]), dev(c["ref"]), dev(c["normals"]), c["T0"], **args)


@functools.lru_cache(maxsize=None)
def gpu_run(name):
    return run(P.case(name))


def replay(c, r, max_iterations=None, normals=None):
    return R.replay(c["src"], c["ref"], c["normals"] if normals is None else normals, c["max_dist"],
                    c["max_iterations"] if max_iterations is None else max_iterations, 1e-6, 1e-6, r.history.numpy(), r.status,
                    r.iterations, knn=gpu_knn, echo=print)


REPLAYED = P.ROOM + P.EDGES + P.CUT + ("plane",)


@pytest.mark.parametrize("name", REPLAYED)
def test_every_step_replays(name):
    c, r = P.case(name), gpu_run(name)
    worst = replay(c, r)
    print(f"{name}: {r.status} after {r.iterations} iterations, worst error / bound = {worst:.3f}")
    if name in ("edge_src_0", "edge_src_1", "edge_src_2", "edge_src_3", "disjoint", "cut_5", "plane", "room_far_rigid"):
        assert (r.status, r.iterations) == ("degenerate", 0)
    if name in ("cut_6", "cut_7"):      # six pairs are enough for the solve to be tried
        assert r.iterations >= 1
    if name == "room_small_rigid":      # float64 settles into a 2-cycle here: the estimator's behaviour, no fault
        assert r.status in ("converged", "iteration_limit")
    if name == "between_clusters":      # listed queries within the cap of a cluster are matched and so enter the sums
        assert 0 < r.history[0, 12] < c["src"].shape[0] and r.iterations >= 1


@pytest.mark.parametrize("name", REPLAYED)
def test_final_outputs_are_the_evaluation_of_the_returned_transform(name):
    c, r = P.case(name), gpu_run(name)
    T = r.transform.cpu().numpy()
    assert T.dtype == np.float32 and (T[3] == [0, 0, 0, 1]).all()
    assert r.index.shape == r.dist2.shape == (c["src"].shape[0],) and r.index.dtype == torch.int64
    ev = R0.evaluate(T[:3], c["src"], c["ref"], np.float32(c["max_dist"] ** 2), gpu_knn)
    assert np.array_equal(r.index.cpu().numpy(), ev["j"])
    assert np.array_equal(r.dist2.cpu().numpy().view(np.int32), ev["d"].view(np.int32))
    h = r.history.numpy()
    assert h.shape == (r.iterations + 1, 16) and (h[-1, :12].reshape(3, 4) == T[:3]).all()
    assert r.fitness == h[-1, 14] and r.inlier_rmse == h[-1, 15] and h[-1, 12] == ev["n"]
    assert r.converged == (r.status == "converged") and r.status in ("converged", "iteration_limit", "degenerate")
    assert r.iterations <= c["max_iterations"] and (r.status != "iteration_limit" or r.iterations == c["max_iterations"])
    # max_iterations = 0 is the pure evaluation: evaluate_registration, bit for bit
    e = evaluate_registration(dev(c["src"]), dev(c["ref"]), c["max_dist"], T, return_correspondences=True)
    zero = icp_point_to_plane(dev(c["src"]), dev(c["ref"]), dev(c["normals"]), T, max_dist=c["max_dist"], max_iterations=0,
                              return_correspondences=True)
    for x in (e, zero):
        assert x.iterations == 0 and x.status == ("degenerate" if c["src"].shape[0] == 0 else "iteration_limit")
        assert same_bits(x.transform, r.transform) and (x.fitness, x.inlier_rmse) == (r.fitness, r.inlier_rmse)
        assert torch.equal(x.index, r.index) and same_bits(x.dist2, r.dist2)


def test_degenerate_outcomes_return_the_last_valid_transform():
    for name in ("plane", "cut_5", "edge_src_0", "disjoint", "room_far_rigid"):      # at t = 0: T_0 bit for bit
        c, r = P.case(name), gpu_run(name)
        assert (r.status, r.iterations, r.converged) == ("degenerate", 0, False), name
        assert np.array_equal(r.transform.cpu().numpy().view(np.int32), c["T0"].view(np.int32)), name
    r = gpu_run("disjoint")
    assert r.fitness == 0.0 and r.inlier_rmse == 0.0 and (r.index == -1).all() and torch.isinf(r.dist2).all()
    assert gpu_run("plane").history[0, 12] == P.case("plane")["src"].shape[0]
    assert gpu_run("cut_5").history[0, 12] == 5
    for name in ("cut_6", "cut_7", "between_clusters"):      # later: the transform of the last recorded row
        r = gpu_run(name)
        if r.status == "degenerate":
            assert np.array_equal(r.transform.cpu().numpy()[:3].ravel().astype(np.float64), r.history.numpy()[-1, :12])


def test_room_rigid_converges_as_float64_does():
    c, r = P.case("room_rigid"), gpu_run("room_rigid")
    f = R.icp_plane_f64(c["src"], c["ref"], c["normals"], c["T0"], c["max_dist"], c["max_iterations"], knn=gpu_knn)
    got, want = R0.errors(r.transform.cpu().numpy(), c["T_gt"]), R0.errors(f["transform"], c["T_gt"])
    print(f"room_rigid: gpu {r.iterations} iterations, errors {got}; float64 {f['iterations']} iterations, errors {want}")
    assert r.status == "converged" and r.iterations <= 10 and f["status"] == R.CONVERGED
    assert got[0] <= 2 * want[0] and got[1] <= 2 * want[1], (got, want)


def test_zero_normal_rows_drop_out_of_the_update_but_count():
    c = P.case("room_rigid")
    r0 = gpu_run("room_rigid")
    matched = run(c, max_iterations=0).index.cpu().numpy()
    hit = np.unique(matched[matched >= 0])[::5]                     # a fifth of the reference points matched at T_0
    normals = c["normals"].copy()
    normals[hit] = 0.0
    zeroed = icp_point_to_plane(dev(c["src"]), dev(c["ref"]), torch.from_numpy(normals).cuda(), c["T0"], max_dist=c["max_dist"],
                                max_iterations=1, return_history=True)
    h = zeroed.history.numpy()
    assert h[0, 12] == r0.history.numpy()[0, 12] and h[0, 13] == r0.history.numpy()[0, 13]      # n and S count them
    # the update is the float64 update over the pairs whose normal is not zero
    ev = R0.evaluate(c["T0"][:3], c["src"], c["ref"], np.float32(c["max_dist"] ** 2), gpu_knn)
    kept = dict(ev, j=np.where(np.isin(ev["j"], hit), -1, ev["j"]))
    assert 0 < (kept["j"] >= 0).sum() < ev["n"]
    Tn, bound, ratio = R.plane_update(c["T0"][:3], c["src"], c["ref"], c["normals"], kept)
    assert ratio >= R.JUDGED and (np.abs(h[1, :12].reshape(3, 4) - Tn) <= bound).all()
    assert (h[1, :12] != r0.history.numpy()[1, :12]).any()
    replay(c, zeroed, max_iterations=1, normals=normals)


def test_estimate_normals_end_to_end():
    c = P.case("room_rigid")
    normals = estimate_normals(dev(c["ref"]), k=8)
    r = icp_point_to_plane(dev(c["src"]), dev(c["ref"]), normals, c["T0"], max_dist=c["max_dist"], return_history=True)
    replay(c, r, max_iterations=30, normals=normals.cpu().numpy())
    angle, shift, _ = R0.errors(r.transform.cpu().numpy(), c["T_gt"])
    assert r.status == "converged" and r.iterations <= 10 and angle <= 0.05 and shift <= 0.01, (r.status, r.iterations, angle, shift)


def test_two_calls_and_another_stream_give_the_same_bits():
    c = P.case("room_small_rigid")
    first, again = run(c), run(c)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = run(c)
    side.synchronize()
    for x in (again, other):
        assert same_bits(x.transform, first.transform) and torch.equal(x.index, first.index) and same_bits(x.dist2, first.dist2)
        assert (x.status, x.iterations, x.fitness, x.inlier_rmse) == (first.status, first.iterations, first.fitness, first.inlier_rmse)
        assert np.array_equal(x.history.numpy().view(np.int64), first.history.numpy().view(np.int64))


def test_non_finite_points_or_normals_raise_and_write_nothing():
    c = P.case("edge_src_257")
    src, ref, normals = dev(c["src"]), dev(c["ref"]), dev(c["normals"])
    n, m, its = src.shape[0], ref.shape[0], 4
    t0 = np.ascontiguousarray(c["T0"][:3])
    ws = torch.empty(_lib.lib().gr_cloud_icp_plane_workspace_bytes(n, m, its), dtype=torch.uint8, device="cuda")
    T = torch.full((16,), 5.0, device="cuda")
    stats = torch.full((4,), 5.0, dtype=torch.float64, device="cuda")
    index = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    dist2 = torch.full((n,), 5.0, device="cuda")
    history = torch.full((its + 1, 16), 5.0, dtype=torch.float64, device="cuda")
    status = (ctypes.c_int * 2)(-1, -1)
    nan_src, inf_ref, nan_normals = src.clone(), ref.clone(), normals.clone()
    nan_src[100, 1] = math.nan
    inf_ref[4000, 2] = math.inf
    nan_normals[4096, 2] = math.nan
    p0 = t0.ctypes.data_as(ctypes.c_void_p)
    for s, q, v, text in ((nan_src, ref, normals, b"points must be finite"), (src, inf_ref, normals, b"points must be finite"),
                          (src, ref, nan_normals, b"normals must be finite")):
        rc = _lib.lib().gr_cloud_icp_plane(s.data_ptr(), n, q.data_ptr(), v.data_ptr(), m, p0, 0.04, its, 1e-6, 1e-6, T.data_ptr(),
                                           stats.data_ptr(), index.data_ptr(), dist2.data_ptr(), history.data_ptr(), status,
                                           ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc != 0 and text in _lib.lib().gr_last_error()
    torch.cuda.synchronize()
    assert (T == 5.0).all() and (stats == 5.0).all() and (index == 5).all() and (dist2 == 5.0).all() and (history == 5.0).all()
    with pytest.raises(ValueError, match="points must be finite"):
        icp_point_to_plane(nan_src, ref, normals)
    with pytest.raises(ValueError, match="normals must be finite"):
        icp_point_to_plane(src, ref, nan_normals)


def test_errors_and_exports():
    c = P.case("room_small_rigid")
    src, ref, normals = dev(c["src"]), dev(c["ref"]), dev(c["normals"])
    assert gaussreg_amd.icp_point_to_plane is icp_point_to_plane
    with pytest.raises(ValueError, match="ref_normals"):      # the point-to-point call's arguments: a transform, a flag
        icp_point_to_plane(src, ref, c["T0"])
    with pytest.raises(ValueError, match="ref_normals"):
        icp_point_to_plane(src, ref, True)
    with pytest.raises(ValueError, match="rows"):
        icp_point_to_plane(src, ref, normals[:-1])
    with pytest.raises(ValueError, match="shape"):
        icp_point_to_plane(src, ref, normals[:, :2])
    with pytest.raises(ValueError, match="float32"):
        icp_point_to_plane(src, ref, normals.double())
    with pytest.raises(ValueError, match="contiguous"):
        icp_point_to_plane(src, ref[::2], normals[::2])
    with pytest.raises(ValueError, match="no CPU fallback"):
        icp_point_to_plane(src, ref, normals.cpu())
    with pytest.raises(ValueError, match="at least 1"):
        icp_point_to_plane(src, ref[:0], normals[:0])
    with pytest.raises(ValueError, match="max_dist"):
        icp_point_to_plane(src, ref, normals, max_dist=-0.5)
    for bad in (-1, 257, True, 1.0):
        with pytest.raises(ValueError, match="max_iterations"):
            icp_point_to_plane(src, ref, normals, max_iterations=bad)
    with pytest.raises(ValueError, match="init_transform"):
        icp_point_to_plane(src, ref, normals, np.eye(3))
    with pytest.raises(ValueError, match="max_iterations"):     # icp's positional with_scale flag has no place here
        icp_point_to_plane(src, ref, normals, c["T0"], c["max_dist"], True)


def test_example_refines_a_synthetic_pair_by_point_to_plane():
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "register_scenes.py"), "--synthetic", "--synthetic_n", "20000",
                        "--num_sample", "5000", "--icp", "--icp_plane", "--icp_dist", "0.5", "--evaluate"],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    rmse = {}
    for line in r.stdout.splitlines():
        for label in ("coarse", "refined"):
            if line.strip().startswith(f"{label} registration rmse:"):
                rmse[label] = float(line.split(":")[1])
    assert set(rmse) == {"coarse", "refined"} and "icp (point-to-plane, " in r.stdout, r.stdout
    assert math.isfinite(rmse["refined"]) and rmse["refined"] <= rmse["coarse"], rmse
