"""GPU: generalised ICP (gaussreg_amd.icp.icp_generalized, csrc/cloud_icp_gicp.hip) against the step-by-step replay of
tests/cloud_gicp_f64.py, and the covariance kernels (gaussreg_amd.covariances, csrc/cloud_covariances.hip) against their twins.

As in tests/test_gpu_cloud_icp_plane.py trajectories never have to agree: for every recorded t the GPU's own T_t is taken from
`history`, E(T_t) is recomputed with the numpy fp32 transform and cloud_nn.knn, U(T_t) is computed in float64 and the GPU's
T_(t+1) has to lie within 4 fp32 ulps of 1 (rotation block) and of |dt| + |t_t| (translation); the stop decision is checked
against the rule at every t.  The covariances of the cases come from the float64 twins, so the kernels are tested apart; one
case runs estimate_covariances end to end.  Measured figures: docs/cloud_gicp_f64_errors.md."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_gicp_cases as C
import cloud_gicp_f64 as G
import cloud_icp_f64 as R0
import gaussreg_amd
from gaussreg_amd import _lib, cloud_nn
from gaussreg_amd.covariances import covariances_from_gaussians, covariances_from_normals, estimate_covariances
from gaussreg_amd.icp import evaluate_registration, icp_generalized, icp_point_to_plane

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
    src_cov, ref_cov = args.pop("src_cov", None), args.pop("ref_cov", None)
    return icp_generalized(dev(c["src"]), dev(c["ref"]), dev(c["src_cov"]) if src_cov is None else src_cov,
                           dev(c["ref_cov"]) if ref_cov is None else ref_cov, c["T0"], **args)


@functools.lru_cache(maxsize=None)
def gpu_run(name):
    return run(C.case(name))


@pytest.fixture(scope="module", autouse=True)
def _release_the_cases():
    """The device copies of the cases and the cached results live as long as this module's tests, not as long as the session
    (hygiene, as in tests/test_gpu_group_norm_backward.py; DESIGN.md Known gap 14 has the open fault this is no remedy for)."""
    yield
    gpu_run.cache_clear()
    _dev.clear()


def replay(c, r, max_iterations=None, src_cov=None, ref_cov=None):
    return G.replay(c["src"], c["ref"], c["src_cov"] if src_cov is None else src_cov, c["ref_cov"] if ref_cov is None else ref_cov,
                    c["max_dist"], c["max_iterations"] if max_iterations is None else max_iterations, 1e-6, 1e-6,
                    r.history.numpy(), r.status, r.iterations, knn=gpu_knn, echo=print)


@pytest.mark.parametrize("name", C.ALL)
def test_every_step_replays(name):
    c, r = C.case(name), gpu_run(name)
    worst, lowest = replay(c, r)
    print(f"{name}: {r.status} after {r.iterations} iterations, worst error / bound = {worst:.3f}, smallest judged ratio = {lowest:.3g}")
    assert ((r.status, r.iterations) == ("degenerate", 0)) == (name in C.DEGENERATE_AT_0)
    if name in C.DEGENERATE_AT_0:
        assert np.array_equal(r.transform.cpu().numpy().view(np.int32), c["T0"].view(np.int32))
    if name in ("cut_3", "cut_4", "edge_src_3"):      # three pairs are enough for the solve to be tried
        assert r.iterations >= 1
    if name == "plane":       # one wall: point-to-plane refuses it, the priors of both clouds fix all six freedoms
        assert r.status == "converged" and r.iterations >= 1
    if name == "between_clusters":      # listed queries within the cap of a cluster are matched and so enter the sums
        assert 0 < r.history[0, 12] < c["src"].shape[0] and r.iterations >= 1


@pytest.mark.parametrize("name", C.ALL)
def test_final_outputs_are_the_evaluation_of_the_returned_transform(name):
    c, r = C.case(name), gpu_run(name)
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
    zero = icp_generalized(dev(c["src"]), dev(c["ref"]), dev(c["src_cov"]), dev(c["ref_cov"]), T, max_dist=c["max_dist"],
                           max_iterations=0, return_correspondences=True)
    for x in (e, zero):
        assert x.iterations == 0 and x.status == ("degenerate" if c["src"].shape[0] == 0 else "iteration_limit")
        assert same_bits(x.transform, r.transform) and (x.fitness, x.inlier_rmse) == (r.fitness, r.inlier_rmse)
        assert torch.equal(x.index, r.index) and same_bits(x.dist2, r.dist2)


@pytest.mark.parametrize("name", ("aniso", "room_small_rigid"))
def test_covariances_times_four_leave_the_history_bit_identical(name):
    """M, det M against trace M cubed, W, H and g all scale by a power of two; x = -H^-1 g does not change."""
    c, r = C.case(name), gpu_run(name)
    scaled = run(c, src_cov=dev(c["src_cov"]) * 4.0, ref_cov=dev(c["ref_cov"]) * 4.0)
    assert (scaled.status, scaled.iterations) == (r.status, r.iterations) and r.iterations >= 1
    assert np.array_equal(scaled.history.numpy().view(np.int64), r.history.numpy().view(np.int64))
    assert same_bits(scaled.transform, r.transform) and torch.equal(scaled.index, r.index) and same_bits(scaled.dist2, r.dist2)


def test_room_rigid_converges_as_float64_does():
    c, r = C.case("room_rigid"), gpu_run("room_rigid")
    f = G.icp_gicp_f64(c["src"], c["ref"], c["src_cov"], c["ref_cov"], c["T0"], c["max_dist"], c["max_iterations"], knn=gpu_knn)
    got, want = R0.errors(r.transform.cpu().numpy(), c["T_gt"]), R0.errors(f["transform"], c["T_gt"])
    print(f"room_rigid: gpu {r.iterations} iterations, errors {got}; float64 {f['iterations']} iterations, errors {want}")
    assert r.status == "converged" and r.iterations <= 10 and f["status"] == G.CONVERGED
    assert got[0] <= 2 * want[0] and got[1] <= 2 * want[1], (got, want)


def test_singular_pairs_drop_out_of_the_update_but_count():
    c, r0 = C.case("singular"), gpu_run("room_rigid")
    zeroed = gpu_run("singular")
    h, h0 = zeroed.history.numpy(), r0.history.numpy()
    assert h[0, 12] == h0[0, 12] and h[0, 13] == h0[0, 13]      # n and S count them
    # the update is the float64 update over the pairs whose M is not zero
    ev = R0.evaluate(c["T0"][:3], c["src"], c["ref"], np.float32(c["max_dist"] ** 2), gpu_knn)
    _, _, singular = G.system(c["T0"][:3], c["src"], c["ref"], c["src_cov"], c["ref_cov"], ev)
    assert 0 < singular.sum() < ev["n"] and singular.sum() == np.isin(ev["j"], c["hit"]).sum()
    kept = dict(ev, j=np.where(np.isin(ev["j"], c["hit"]), -1, ev["j"]))
    full = C.case("room_rigid")
    Tn, bound, ratio = G.gicp_update(c["T0"][:3], c["src"], c["ref"], full["src_cov"], full["ref_cov"], kept)
    assert ratio >= G.JUDGED and (np.abs(h[1, :12].reshape(3, 4) - Tn) <= bound).all()
    assert (h[1, :12] != h0[1, :12]).any()


def test_estimate_covariances_end_to_end():
    c = C.case("room_rigid")
    src_cov, ref_cov = estimate_covariances(dev(c["src"]), k=8), estimate_covariances(dev(c["ref"]), k=8)
    r = icp_generalized(dev(c["src"]), dev(c["ref"]), src_cov, ref_cov, c["T0"], max_dist=c["max_dist"], return_history=True)
    sc, rc = src_cov.cpu().numpy(), ref_cov.cpu().numpy()
    replay(c, r, max_iterations=30, src_cov=sc, ref_cov=rc)
    f = G.icp_gicp_f64(c["src"], c["ref"], sc, rc, c["T0"], c["max_dist"], 30, knn=gpu_knn)
    got, want = R0.errors(r.transform.cpu().numpy(), c["T_gt"]), R0.errors(f["transform"], c["T_gt"])
    print(f"end to end: gpu {r.status}, {r.iterations} iterations, errors {got}; float64 {f['iterations']} iterations, errors {want}")
    assert r.status == "converged" and r.iterations <= 10
    assert got[0] <= 2 * want[0] and got[1] <= 2 * want[1], (got, want)


def test_two_calls_and_another_stream_give_the_same_bits():
    c = C.case("room_small_rigid")
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


def test_non_finite_covariances_raise_and_write_nothing():
    c = C.case("edge_src_257")
    src, ref, src_cov, ref_cov = dev(c["src"]), dev(c["ref"]), dev(c["src_cov"]), dev(c["ref_cov"])
    n, m, its = src.shape[0], ref.shape[0], 4
    t0 = np.ascontiguousarray(c["T0"][:3])
    ws = torch.empty(_lib.lib().gr_cloud_gicp_workspace_bytes(n, m, its), dtype=torch.uint8, device="cuda")
    T = torch.full((16,), 5.0, device="cuda")
    stats = torch.full((4,), 5.0, dtype=torch.float64, device="cuda")
    index = torch.full((n,), 5, dtype=torch.int64, device="cuda")
    dist2 = torch.full((n,), 5.0, device="cuda")
    history = torch.full((its + 1, 16), 5.0, dtype=torch.float64, device="cuda")
    status = (ctypes.c_int * 2)(-1, -1)
    nan_src, nan_src_cov, inf_ref_cov = src.clone(), src_cov.clone(), ref_cov.clone()
    nan_src[100, 1] = math.nan
    nan_src_cov[256, 5] = math.nan          # the last entry of the last row
    inf_ref_cov[4096, 0] = math.inf
    p0 = t0.ctypes.data_as(ctypes.c_void_p)
    for s, cs, cr, text in ((nan_src, src_cov, ref_cov, b"points must be finite"), (src, nan_src_cov, ref_cov, b"covariances must be finite"),
                            (src, src_cov, inf_ref_cov, b"covariances must be finite")):
        rc = _lib.lib().gr_cloud_gicp(s.data_ptr(), n, cs.data_ptr(), ref.data_ptr(), cr.data_ptr(), m, p0, 0.04, its, 1e-6, 1e-6,
                                      T.data_ptr(), stats.data_ptr(), index.data_ptr(), dist2.data_ptr(), history.data_ptr(), status,
                                      ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc != 0 and text in _lib.lib().gr_last_error()
    torch.cuda.synchronize()
    assert (T == 5.0).all() and (stats == 5.0).all() and (index == 5).all() and (dist2 == 5.0).all() and (history == 5.0).all()
    with pytest.raises(ValueError, match="points must be finite"):
        icp_generalized(nan_src, ref, src_cov, ref_cov)
    with pytest.raises(ValueError, match="covariances must be finite"):
        icp_generalized(src, ref, nan_src_cov, ref_cov)
    with pytest.raises(ValueError, match="covariances must be finite"):
        icp_generalized(src, ref, src_cov, inf_ref_cov)


def neighbours_in_fp32(got, want64):
    """Every entry of `got` (fp32) is the float64 value rounded to fp32, or the fp32 value next to it."""
    want = want64.astype(np.float32)
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    return bool(((got == want) | (got == lo) | (got == hi)).all())


def _gaussians(n, seed):
    rng = np.random.default_rng(seed)
    scales = np.exp(rng.uniform(np.log(0.01), np.log(1.0), (n, 3))).astype(np.float32)
    q = (rng.normal(size=(n, 4)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    scales[1] = 0.25                                   # equal scales: the first axis
    scales[2, 1] = scales[2, 2] = scales[2].min()      # the second and third equal and smallest: the second
    q[3] = 0.0                                         # a zero quaternion
    q[4] = (0.0, 1.0, 0.0, 0.0)                        # a half turn about x: the y and z axes are negated
    scales[4] = (0.5, 0.01, 0.3)
    q[5] = (1.0, 0.0, 0.0, 0.0)                        # exact axes
    scales[5] = (0.01, 0.2, 0.3)
    return scales, q


def test_covariances_from_normals_against_the_twin():
    rng = np.random.default_rng(17)
    normals = (rng.normal(size=(1027, 3)) * rng.uniform(0.1, 5.0, (1027, 1))).astype(np.float32)
    normals[0] = 0.0                                   # an invalid row of the normals kernel
    normals[1] = (0.0, -2.0, 0.0)                      # a negative largest component: C does not see the sign
    normals[2] = (0.0, 0.0, 1.0)
    for eps in (1e-3, 0.25):
        got = covariances_from_normals(torch.from_numpy(normals).cuda(), eps).cpu().numpy()
        assert got.shape == (1027, 6) and got.dtype == np.float32
        assert neighbours_in_fp32(got, G.covariances_from_normals_f64(normals, eps))
        assert (got[0] == [1, 0, 0, 1, 0, 1]).all() and np.array_equal(got[1], np.float32([1, 0, 0, 1.0 - (1.0 - eps), 0, 1]))
    bad = normals.copy()
    bad[7, 1], bad[9, 0] = math.nan, math.inf
    got = covariances_from_normals(torch.from_numpy(bad).cuda()).cpu().numpy()
    rows = ~np.isfinite(got).all(1)
    assert rows[7] and rows[9] and rows.sum() == 2      # its own row, no other
    assert covariances_from_normals(torch.empty((0, 3), device="cuda")).shape == (0, 6)


def test_covariances_from_gaussians_plane_against_the_twin():
    scales, q = _gaussians(1027, 19)
    for eps in (1e-3, 0.25):
        cov, normals, valid = covariances_from_gaussians(torch.from_numpy(scales).cuda(), torch.from_numpy(q).cuda(), mode="plane",
                                                         epsilon=eps, return_normals=True)
        want = G.gs_covariances_f64(scales, q, mode="plane", epsilon=eps)
        assert neighbours_in_fp32(cov.cpu().numpy(), want["cov"]) and neighbours_in_fp32(normals.cpu().numpy(), want["normal"])
        assert valid.dtype == torch.bool and np.array_equal(valid.cpu().numpy(), want["valid"])
        cov, normals = cov.cpu().numpy(), normals.cpu().numpy()
        assert (cov[3] == [1, 0, 0, 1, 0, 1]).all() and (normals[3] == 0).all() and not valid[3] and valid.sum() == 1026
        assert (normals[5] == [1, 0, 0]).all()
        assert (normals[4] == [0, 1, 0]).all()          # the axis is (0, -1, 0): flipped so that its largest component is positive
        big = normals[np.arange(1027), np.argmax(np.abs(normals), axis=1)]
        assert (big[valid.cpu().numpy()] > 0).all()
    only = covariances_from_gaussians(torch.from_numpy(scales).cuda(), torch.from_numpy(q).cuda())
    assert isinstance(only, torch.Tensor) and only.shape == (1027, 6)


def test_raw_covariances_render_as_scales_and_rotations_do():
    from gaussreg_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from helpers import raster_scene
    P, W, H, mod = 500, 64, 48, 1.7
    g, cams = raster_scene(P, W, H, seed=5)
    cam = cams[0]
    d = {k: torch.from_numpy(v).cuda() for k, v in g.items()}
    settings = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.tensor((0.1, 0.3, 0.7), dtype=torch.float32, device="cuda"), scale_modifier=mod,
        viewmatrix=torch.from_numpy(cam["viewmatrix"]).cuda(), projmatrix=torch.from_numpy(cam["projmatrix"]).cuda(), sh_degree=3,
        campos=torch.from_numpy(cam["campos"]).cuda(), prefiltered=False, debug=False)
    want_img, want_radii = GaussianRasterizer(settings)(means3D=d["means3D"], means2D=None, opacities=d["opacities"], shs=d["shs"],
                                                        scales=d["scales"], rotations=d["rotations"])
    cov, normals, valid = covariances_from_gaussians(d["scales"].contiguous(), d["rotations"].contiguous(), scale_modifier=mod,
                                                     mode="raw", return_normals=True)
    img, radii = GaussianRasterizer(settings)(means3D=d["means3D"], means2D=None, opacities=d["opacities"], shs=d["shs"],
                                              cov3D_precomp=cov)
    assert (want_radii > 0).sum() > 50 and torch.equal(radii, want_radii) and same_bits(img, want_img)
    # raw mode's normals are PLANE mode's
    _, plane_normals, plane_valid = covariances_from_gaussians(d["scales"].contiguous(), d["rotations"].contiguous(), mode="plane",
                                                               return_normals=True)
    assert same_bits(normals, plane_normals) and torch.equal(valid, plane_valid)
    want = G.gs_covariances_f64(g["scales"], g["rotations"], scale_modifier=mod, mode="raw")["cov"]
    # fp32: three roundings per entry of R, one for s R, and a sum of three products whose magnitudes add up to at most the
    # trace <= 3 max |entry|: ~10 eps of each term, 32 eps of the largest entry
    assert np.abs(cov.cpu().numpy() - want).max() <= 32 * np.finfo(np.float32).eps * np.abs(want).max()


def _whole_room():
    """tests/cloud_icp_cases.py's room, all of it as the reference -- the overlap of room_rigid holds no face across x, which
    exact face normals cannot do without -- and every other point, with 2 mm of noise, as the source; T0 off by 2 degrees."""
    import cloud_icp_cases as CI
    rng = np.random.default_rng(29)
    pts = CI.room_points(6000, 13)
    T_gt = CI.similarity(CI.rotation((1, 2, 3), 25.0), (0.5, -0.3, 0.2))
    part = pts[::2] + rng.normal(0.0, 0.002, pts[::2].shape)
    src = np.ascontiguousarray(CI.apply64(np.linalg.inv(T_gt), part), np.float32)
    T0 = (CI.similarity(CI.rotation((3, -1, 2), 2.0), (0.02, -0.015, 0.01)) @ T_gt).astype(np.float32)
    T0[3] = (0, 0, 0, 1)
    return src, np.ascontiguousarray(pts, np.float32), T0, T_gt


def test_gaussian_axis_normals_on_room_faces_feed_point_to_plane():
    """Flat Gaussians planted on the faces of a room: the thinnest axis is the face axis, exactly, whatever the in-plane
    rotation; and icp_point_to_plane takes these normals with no search (float64 reaches 0.005 degrees and 0.3 mm here)."""
    src, ref, T0, T_gt = _whole_room()
    # the face of every reference point: the coordinate that sits exactly on a face of the room or the box
    faces = ((0, 0.0), (1, 0.0), (2, 0.0), (0, 4.0), (1, 3.0), (2, 2.5), (0, 1.0), (1, 0.6), (2, 0.8))
    axis = np.full(ref.shape[0], -1)
    for a, value in faces:
        axis = np.where((axis < 0) & (ref[:, a] == np.float32(value)), a, axis)
    assert (axis >= 0).all()
    rng = np.random.default_rng(23)
    n, rows = ref.shape[0], np.arange(ref.shape[0])
    # thin along the face axis, turned about that axis by any angle: column `axis` of R is the unit vector, with no rounding
    scales = rng.uniform(0.02, 0.1, (n, 3)).astype(np.float32)
    scales[rows, axis] = 0.001
    half = rng.uniform(0.0, np.pi, n)
    q = np.zeros((n, 4), np.float32)
    q[:, 0], q[rows, 1 + axis] = np.cos(half), np.sin(half)
    q *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)      # not normalised: the kernel does that
    cov, normals, valid = covariances_from_gaussians(torch.from_numpy(scales).cuda(), torch.from_numpy(q).cuda(), return_normals=True)
    want = np.eye(3, dtype=np.float32)[axis]
    assert valid.all() and np.array_equal(normals.cpu().numpy(), want) and len(set(axis.tolist())) == 3
    assert np.array_equal(cov.cpu().numpy(), G.covariances_from_normals_f64(want).astype(np.float32))
    r = icp_point_to_plane(torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(), normals, T0, max_dist=0.1)
    angle, shift, _ = R0.errors(r.transform.cpu().numpy(), T_gt)
    assert r.status == "converged" and 1 <= r.iterations <= 10 and angle <= 0.05 and shift <= 0.01, (r.status, r.iterations, angle, shift)


def test_errors_and_exports():
    c = C.case("room_small_rigid")
    src, ref, sc, rc = dev(c["src"]), dev(c["ref"]), dev(c["src_cov"]), dev(c["ref_cov"])
    assert gaussreg_amd.icp_generalized is icp_generalized and gaussreg_amd.estimate_covariances is estimate_covariances
    assert gaussreg_amd.covariances_from_normals is covariances_from_normals
    assert gaussreg_amd.covariances_from_gaussians is covariances_from_gaussians
    with pytest.raises(ValueError, match="src_covariances"):      # the point-to-plane call's arguments: normals, a transform
        icp_generalized(src, ref, rc[:, :3].contiguous(), c["T0"])
    with pytest.raises(ValueError, match="ref_covariances"):
        icp_generalized(src, ref, sc, True)
    with pytest.raises(ValueError, match="rows"):
        icp_generalized(src, ref, sc[:-1], rc)
    with pytest.raises(ValueError, match="rows"):
        icp_generalized(src, ref, sc, rc[:-1])
    with pytest.raises(ValueError, match="shape"):
        icp_generalized(src, ref, sc, rc[:, :5])
    with pytest.raises(ValueError, match="float32"):
        icp_generalized(src, ref, sc.double(), rc)
    with pytest.raises(ValueError, match="contiguous"):
        icp_generalized(src, ref, sc, rc.t().contiguous().t())
    with pytest.raises(ValueError, match="no CPU fallback"):
        icp_generalized(src, ref, sc, rc.cpu())
    with pytest.raises(ValueError, match="at least 1"):
        icp_generalized(src, ref[:0], sc, rc[:0])
    with pytest.raises(ValueError, match="max_dist"):
        icp_generalized(src, ref, sc, rc, max_dist=-0.5)
    for bad in (-1, 257, True, 1.0):
        with pytest.raises(ValueError, match="max_iterations"):
            icp_generalized(src, ref, sc, rc, max_iterations=bad)
    with pytest.raises(ValueError, match="init_transform"):
        icp_generalized(src, ref, sc, rc, np.eye(3))
    with pytest.raises(ValueError, match="epsilon"):
        covariances_from_normals(src, epsilon=1.5)
    with pytest.raises(ValueError, match="mode"):
        covariances_from_gaussians(src, torch.zeros((src.shape[0], 4), device="cuda"), mode="surface")
    with pytest.raises(ValueError, match="rotations"):
        covariances_from_gaussians(src, src)


def test_example_refines_a_synthetic_pair_by_generalised_icp():
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "register_scenes.py"), "--synthetic", "--synthetic_n", "20000",
                        "--num_sample", "5000", "--icp", "--icp_generalized", "--icp_dist", "0.5", "--evaluate"],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    rmse = {}
    for line in r.stdout.splitlines():
        for label in ("coarse", "refined"):
            if line.strip().startswith(f"{label} registration rmse:"):
                rmse[label] = float(line.split(":")[1])
    assert set(rmse) == {"coarse", "refined"} and "icp (generalised, " in r.stdout, r.stdout
    assert math.isfinite(rmse["refined"]) and rmse["refined"] <= rmse["coarse"], rmse
