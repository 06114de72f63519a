"""GPU: point-to-point ICP (gaussreg_amd.icp, csrc/cloud_icp.hip) against the step-by-step replay of tests/cloud_icp_f64.py.

Trajectories never have to agree: for every recorded t the GPU's own T_t is taken from `history`, E(T_t) is recomputed with the
numpy fp32 transform and cloud_nn.knn (pinned to brute force by tests/test_gpu_cloud_nn.py), U(T_t) is computed in float64
and the GPU's T_(t+1) has to lie within the bound of docs/registration_f64_errors.md; the stop decision is checked against the
rule at every t.  Measured figures: docs/cloud_icp_f64_errors.md."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_icp_cases as C
import cloud_icp_f64 as R
import gaussreg_amd
from gaussreg_amd import _lib, cloud_nn, icp as icp_module
from gaussreg_amd.icp import evaluate_registration, icp

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EDGE_ITERATIONS = 6


def gpu_knn(p, ref, cap):
    """The k = 1 capped search of the replay on the kernels of cloud_nn.hip: (d (N,) fp32, j (N,) int64) numpy."""
    d, j = cloud_nn._knn(torch.from_numpy(np.ascontiguousarray(p)).cuda(), dev(ref), 1, float(np.float32(cap)))
    return d[:, 0].cpu().numpy(), j[:, 0].cpu().numpy()


_dev = {}


def dev(a):
    """One device copy per numpy cloud (the cases are cached and never written)."""
    key = id(a)
    if key not in _dev:
        _dev[key] = (a, torch.from_numpy(a).cuda())
    return _dev[key][1]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32
                                                                     else a, b.contiguous().view(torch.int32)
                                                                     if b.dtype == torch.float32 else b)


def arguments(name):
    c = C.case(name)
    # one or two reference points fix no rotation, so there the one-cell grid is exercised by the pure evaluation
    its = 30 if name in C.ROOM + ("lattice_exact",) else 0 if name.startswith("edge_ref_") else EDGE_ITERATIONS
    return dict(max_dist=c["max_dist"], with_scale=c["with_scale"], max_iterations=its, relative_fitness=1e-6, relative_rmse=1e-6)


@functools.lru_cache(maxsize=None)
def gpu_run(name):
    c = C.case(name)
    return icp(dev(c["src"]), dev(c["ref"]), c["T0"], return_correspondences=True, return_history=True, **arguments(name))


@functools.lru_cache(maxsize=None)
def f64_run(name):
    c, a = C.case(name), arguments(name)
    return R.icp_f64(c["src"], c["ref"], c["T0"], a["max_dist"], a["with_scale"], a["max_iterations"], knn=gpu_knn)


REPLAYED = C.ROOM + ("lattice_exact",) + tuple(n for n in C.EDGES if n != "collinear")


@pytest.mark.parametrize("name", REPLAYED)
def test_every_step_replays(name):
    c, a, r = C.case(name), arguments(name), gpu_run(name)
    worst = R.replay(c["src"], c["ref"], a["with_scale"], a["max_dist"], a["max_iterations"], a["relative_fitness"],
                     a["relative_rmse"], r.history.numpy(), r.status, r.iterations, knn=gpu_knn, echo=print)
    print(f"{name}: {r.status} after {r.iterations} iterations, worst error / bound = {worst:.3f}")
    if name in ("edge_src_0", "edge_src_1", "edge_src_2", "disjoint"):
        assert (r.status, r.iterations) == ("degenerate", 0)
    if name == "between_clusters":      # listed queries within the cap of a cluster are matched and so enter the sums
        assert 0 < r.history[0, 12] < c["src"].shape[0] and r.iterations >= 1


@pytest.mark.parametrize("name", REPLAYED + ("collinear",))
def test_final_outputs_are_the_evaluation_of_the_returned_transform(name):
    c, a, r = C.case(name), arguments(name), gpu_run(name)
    T = r.transform.cpu().numpy()
    assert T.dtype == np.float32 and (T[3] == [0, 0, 0, 1]).all()
    assert r.index.shape == r.dist2.shape == (c["src"].shape[0],) and r.index.dtype == torch.int64
    ev = R.evaluate(T[:3], c["src"], c["ref"], np.float32(a["max_dist"] ** 2), gpu_knn)
    assert np.array_equal(r.index.cpu().numpy(), ev["j"])
    assert np.array_equal(r.dist2.cpu().numpy().view(np.int32), ev["d"].view(np.int32))
    h = r.history.numpy()
    assert h.shape == (r.iterations + 1, 16) and (h[-1, :12].reshape(3, 4) == T[:3]).all()
    assert r.fitness == h[-1, 14] and r.inlier_rmse == h[-1, 15] and h[-1, 12] == ev["n"]
    assert r.converged == (r.status == "converged") and r.status in ("converged", "iteration_limit", "degenerate")
    assert r.iterations <= a["max_iterations"] and (r.status != "iteration_limit" or r.iterations == a["max_iterations"])
    # the pure evaluation of the same transform
    e = evaluate_registration(dev(c["src"]), dev(c["ref"]), a["max_dist"], T, return_correspondences=True)
    zero = icp(dev(c["src"]), dev(c["ref"]), T, max_dist=a["max_dist"], max_iterations=0, return_correspondences=True)
    for x in (e, zero):
        assert x.iterations == 0 and x.status == ("degenerate" if c["src"].shape[0] == 0 else "iteration_limit")
        assert same_bits(x.transform, r.transform) and (x.fitness, x.inlier_rmse) == (r.fitness, r.inlier_rmse)
        assert torch.equal(x.index, r.index) and same_bits(x.dist2, r.dist2)


@pytest.mark.parametrize("name", C.ROOM)
def test_room_cases_converge_as_float64_does(name):
    c, r, f = C.case(name), gpu_run(name), f64_run(name)
    assert r.status == "converged" and f["status"] == R.CONVERGED
    got, want = R.errors(r.transform.cpu().numpy(), c["T_gt"]), R.errors(f["transform"], c["T_gt"])
    print(f"{name}: gpu {r.iterations} iterations, errors {got}; float64 {f['iterations']} iterations, errors {want}")
    for g, w in zip(got, want):
        assert g <= 2 * w + 1e-4, (got, want)
    assert r.iterations <= f["iterations"] + 2


def test_lattice_is_exact():
    c, r = C.case("lattice_exact"), gpu_run("lattice_exact")
    n = c["src"].shape[0]
    h = r.history.numpy()
    assert (r.status, r.iterations) == ("converged", 1) and h[0, 12] == n and h[0, 13] == 0.0 and h[0, 14] == 1.0
    e = evaluate_registration(dev(c["src"]), dev(c["ref"]), c["max_dist"], c["T0"], return_correspondences=True)
    assert (e.dist2 == 0).all() and e.fitness == 1.0 and e.inlier_rmse == 0.0
    j = e.index.cpu().numpy()
    assert (j[:34] <= np.arange(0, 100, 3)).all() and (c["ref"][j] == C.apply64(c["T_gt"], c["src"])).all()   # ties: the lower j
    m = np.ones(n, bool)
    T1, s, bound = R.umeyama_f64(c["src"][m], c["ref"][j], True)
    assert (np.abs(h[1, :12].reshape(3, 4) - c["T_gt"][:3]) <= bound).all()


def test_degenerate_at_the_start_returns_the_transform_bit_for_bit():
    for name in ("disjoint", "edge_src_0", "edge_src_2"):
        c, r = C.case(name), gpu_run(name)
        assert (r.status, r.iterations, r.converged) == ("degenerate", 0, False)
        assert np.array_equal(r.transform.cpu().numpy().view(np.int32), c["T0"].view(np.int32))
    r = gpu_run("disjoint")
    assert r.fitness == 0.0 and r.inlier_rmse == 0.0 and (r.index == -1).all() and torch.isinf(r.dist2).all()


def test_collinear_points_with_scale():
    """No unique rotation: the library either refuses (degenerate) or returns a fit whose residual on the matched pairs is no
    worse than the float64 fit's, as docs/registration_f64_errors.md treats collinear sets."""
    c, a = C.case("collinear"), arguments("collinear")
    r = icp(dev(c["src"]), dev(c["ref"]), c["T0"], max_dist=a["max_dist"], with_scale=True, max_iterations=1,
            return_history=True)
    if r.status == "degenerate":
        assert r.iterations == 0
        return
    h = r.history.numpy()
    ev = R.evaluate(h[0, :12].reshape(3, 4), c["src"], c["ref"], np.float32(a["max_dist"] ** 2), gpu_knn)
    m = ev["j"] >= 0
    a64, b64 = c["src"][m].astype(np.float64), c["ref"][ev["j"][m]].astype(np.float64)
    resid = lambda T: float(np.sqrt(((a64 @ T[:, :3].T + T[:, 3] - b64) ** 2).sum(1)).max())
    fit = R.umeyama_f64(a64, b64, True)
    got, want = resid(h[1, :12].reshape(3, 4)), resid(fit[0])
    print(f"collinear: worst residual gpu {got:.3g}, float64 {want:.3g}")
    assert got <= want + 4 * float(np.spacing(np.float32(np.abs(b64).max())))


def test_two_calls_and_another_stream_give_the_same_bits():
    c, a = C.case("room_small"), arguments("room_small")
    call = lambda: icp(dev(c["src"]), dev(c["ref"]), c["T0"], return_correspondences=True, return_history=True, **a)
    first, again = call(), call()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = call()
    side.synchronize()
    for x in (again, other):
        assert same_bits(x.transform, first.transform) and torch.equal(x.index, first.index) and same_bits(x.dist2, first.dist2)
        assert (x.status, x.iterations, x.fitness, x.inlier_rmse) == (first.status, first.iterations, first.fitness, first.inlier_rmse)
        assert np.array_equal(x.history.numpy().view(np.int64), first.history.numpy().view(np.int64))


def test_relabelling_the_reference_permutes_the_result():
    c, a, r = C.case("room_small"), arguments("room_small"), gpu_run("room_small")
    ref = dev(c["ref"])
    perm = torch.randperm(ref.shape[0], generator=torch.Generator().manual_seed(1)).cuda()   # new -> old
    inverse = torch.empty_like(perm)
    inverse[perm] = torch.arange(ref.shape[0], device="cuda")
    # one step from the same start: the same pairs in another order of indices, so the same sums up to their order
    one = dict(a, max_iterations=1)
    base = icp(dev(c["src"]), ref, c["T0"], return_history=True, **one)
    moved = icp(dev(c["src"]), ref[perm].contiguous(), c["T0"], return_history=True, **one)
    e0 = evaluate_registration(dev(c["src"]), ref, a["max_dist"], c["T0"], return_correspondences=True)
    e1 = evaluate_registration(dev(c["src"]), ref[perm].contiguous(), a["max_dist"], c["T0"], return_correspondences=True)
    assert same_bits(e0.dist2, e1.dist2)      # no exact ties between distinct points in this cloud
    assert torch.equal(e1.index, torch.where(e0.index >= 0, inverse[e0.index.clamp_min(0)], -1))
    ev = R.evaluate(c["T0"][:3], c["src"], c["ref"], np.float32(a["max_dist"] ** 2), gpu_knn)
    fit = R.update(ev, c["src"], c["ref"], a["with_scale"])
    assert (np.abs(moved.history.numpy()[1, :12].reshape(3, 4) - fit[0]) <= fit[2]).all()
    assert r.history.numpy()[1, :12].tolist() == base.history.numpy()[1, :12].tolist()


def _abi(*args):
    ptrs = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    return _lib.lib().gr_cloud_icp(*ptrs, torch.cuda.current_stream().cuda_stream)


def _abi_arguments(name, max_iterations):
    c = C.case(name)
    src, ref = dev(c["src"]), dev(c["ref"])
    t0 = np.ascontiguousarray(c["T0"][:3])
    ws = torch.empty(_lib.lib().gr_cloud_icp_workspace_bytes(src.shape[0], ref.shape[0], max_iterations), dtype=torch.uint8,
                     device="cuda")
    return c, src, ref, t0, ws


def test_null_optional_outputs_and_untouched_history_rows_through_the_c_abi():
    name, its = "room_small", 30
    c, src, ref, t0, ws = _abi_arguments(name, its)
    want = gpu_run(name)
    cap = float(np.float32(c["max_dist"] ** 2))
    for with_index in (False, True):
        for with_dist in (False, True):
            for with_history in (False, True):
                T = torch.full((16,), 5.0, device="cuda")
                stats = torch.full((4,), 5.0, dtype=torch.float64, device="cuda")
                index = torch.full((src.shape[0],), 5, dtype=torch.int64, device="cuda") if with_index else None
                dist2 = torch.full((src.shape[0],), 5.0, device="cuda") if with_dist else None
                history = torch.full((its + 1, 16), math.nan, dtype=torch.float64, device="cuda") if with_history else None
                status = (ctypes.c_int * 2)(-1, -1)
                assert _abi(src, src.shape[0], ref, ref.shape[0], t0.ctypes.data_as(ctypes.c_void_p), cap, int(c["with_scale"]), its,
                            1e-6, 1e-6, T, stats, index, dist2, history, status, ws, ws.numel()) == 0
                assert (status[0], status[1]) == (_lib.ICP_DEFINES["GR_CLOUD_ICP_CONVERGED"], want.iterations)
                assert same_bits(T.view(4, 4), want.transform) and stats[:2].tolist() == [want.fitness, want.inlier_rmse]
                assert index is None or torch.equal(index, want.index)
                assert dist2 is None or same_bits(dist2, want.dist2)
                if with_history:
                    assert torch.equal(history[:want.iterations + 1].cpu(), want.history)
                    assert torch.isnan(history[want.iterations + 1:]).all()       # rows never reached are left untouched


def test_c_abi_refuses_bad_arguments_and_writes_nothing():
    c, src, ref, t0, ws = _abi_arguments("edge_src_257", 4)
    n, m = src.shape[0], ref.shape[0]
    T = torch.full((16,), 5.0, device="cuda")
    stats = torch.full((4,), 5.0, dtype=torch.float64, device="cuda")
    index = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    dist2 = torch.full((n,), 5.0, device="cuda")
    history = torch.full((5, 16), 5.0, dtype=torch.float64, device="cuda")
    status = (ctypes.c_int * 2)(-1, -1)
    p0 = t0.ctypes.data_as(ctypes.c_void_p)
    nan_t = t0.copy()
    nan_t[1, 2] = np.nan
    nan_src, inf_ref = src.clone(), ref.clone()
    nan_src[100, 1] = math.nan
    inf_ref[4000, 2] = math.inf
    tail = (T, stats, index, dist2, history, status, ws, ws.numel())
    bad = [(src, n, ref, 0, p0, 0.04, 0, 4, 1e-6, 1e-6) + tail,
           (src, -1, ref, m, p0, 0.04, 0, 4, 1e-6, 1e-6) + tail,
           (src, n, ref, m, p0, -1.0, 0, 4, 1e-6, 1e-6) + tail,
           (src, n, ref, m, p0, math.inf, 0, 4, 1e-6, 1e-6) + tail,
           (src, n, ref, m, p0, math.nan, 0, 4, 1e-6, 1e-6) + tail,
           (src, n, ref, m, p0, 0.04, 0, -1, 1e-6, 1e-6) + tail,
           (src, n, ref, m, p0, 0.04, 0, 257, 1e-6, 1e-6) + tail,
           (src, n, ref, m, nan_t.ctypes.data_as(ctypes.c_void_p), 0.04, 0, 4, 1e-6, 1e-6) + tail,
           (src, n, ref, m, p0, 0.04, 0, 4, 1e-6, 1e-6, T, stats, index, dist2, history, status, ws, 1024),
           (nan_src, n, ref, m, p0, 0.04, 0, 4, 1e-6, 1e-6) + tail,
           (src, n, inf_ref, m, p0, 0.04, 0, 4, 1e-6, 1e-6) + tail]
    for args in bad:
        assert _abi(*args) != 0, args[1:10]
        assert _lib.lib().gr_last_error()
    assert b"points must be finite" in _lib.lib().gr_last_error()
    torch.cuda.synchronize()
    assert (T == 5.0).all() and (stats == 5.0).all() and (index == 5).all() and (dist2 == 5.0).all() and (history == 5.0).all()


def test_errors():
    c = C.case("room_small")
    src, ref = dev(c["src"]), dev(c["ref"])
    with pytest.raises(ValueError, match="no CPU fallback"):
        icp(src.cpu(), ref)
    with pytest.raises(ValueError, match="no CPU fallback"):
        icp(src, ref.cpu())
    with pytest.raises(ValueError, match="float32"):
        icp(src.double(), ref)
    with pytest.raises(ValueError, match="shape"):
        icp(src[:, :2], ref)
    with pytest.raises(ValueError, match="contiguous"):
        icp(src, ref[::2])
    with pytest.raises(ValueError, match="at least 1"):
        icp(src, ref[:0])
    for bad in (-0.5, math.inf, math.nan, None):
        with pytest.raises(ValueError, match="max_dist"):
            icp(src, ref, max_dist=bad)
    for bad in (-1, 257, True, 1.0):
        with pytest.raises(ValueError, match="max_iterations"):
            icp(src, ref, max_iterations=bad)
    with pytest.raises(ValueError, match="init_transform"):
        icp(src, ref, np.eye(3))
    with pytest.raises(ValueError, match="init_transform"):
        icp(src, ref, np.full((4, 4), np.nan))
    with pytest.raises(ValueError, match="last row"):
        icp(src, ref, np.ones((4, 4)))
    nan = src.clone()
    nan[3, 0] = math.nan
    with pytest.raises(ValueError, match="points must be finite"):
        icp(nan, ref)
    with pytest.raises(ValueError, match="points must be finite"):
        evaluate_registration(ref, nan, 0.1)


def test_package_root_exports_icp():
    c = C.case("edge_src_129")
    assert gaussreg_amd.icp is icp_module and gaussreg_amd.evaluate_registration is evaluate_registration
    r = gaussreg_amd.icp(dev(c["src"]), dev(c["ref"]), c["T0"], max_dist=c["max_dist"], max_iterations=EDGE_ITERATIONS)
    assert same_bits(r.transform, gpu_run("edge_src_129").transform) and r.index is None and r.history is None


def test_example_refines_a_synthetic_pair():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "register_scenes.py"), "--synthetic", "--synthetic_n", "20000",
                        "--num_sample", "5000", "--icp", "--icp_scale", "--icp_dist", "0.5", "--evaluate"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    rmse = {}
    for line in r.stdout.splitlines():
        for label in ("coarse", "refined"):
            if line.strip().startswith(f"{label} registration rmse:"):
                rmse[label] = float(line.split(":")[1])
    assert set(rmse) == {"coarse", "refined"} and "icp (" in r.stdout, r.stdout
    assert math.isfinite(rmse["refined"]) and rmse["refined"] <= rmse["coarse"], rmse
