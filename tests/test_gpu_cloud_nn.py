"""GPU: gaussreg_amd.cloud_nn against the brute-force restatements of tests/cloud_nn_f64.py -- bit equality with the fp32
enumeration (capped and uncapped, every k path, the fallback, padding, ties), the ordered pair list, float64 on the pair
the checks are stated for, and the C ABI's refusals."""
import ctypes
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_nn_cases as C
import cloud_nn_f64 as R
import gaussreg_amd
from gaussreg_amd import _lib, cloud_nn

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KS = (1, 3, 8)
INF = math.inf


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def clouds(name):
    q, s = C.pair(name)
    return torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda()


@functools.lru_cache(maxsize=None)
def expected(name, radius):
    """The fp32 brute force with 8 neighbours, once per (pair, cap); a test takes the first k columns."""
    q, s = clouds(name)
    return R.knn_f32_torch(q, s, 8, INF if radius is None else float(R.r2_of(radius)))


def check_bits(name, k, radius):
    q, s = clouds(name)
    dist, index = expected(name, radius)
    got_d, got_i = cloud_nn.knn(q, s, k, radius)
    assert got_d.dtype == torch.float32 and got_i.dtype == torch.int64
    assert got_d.shape == (q.shape[0], k) and got_i.shape == (q.shape[0], k)
    bad = (got_i != index[:, :k]).any(dim=1).sum().item()
    assert bad == 0, f"{name} k={k} radius={radius}: {bad} rows with other neighbours"
    assert same_bits(got_d, dist[:, :k])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", [n for n in C.NAMES if n not in C.TINY])
def test_uncapped_is_bit_equal(name, k):
    check_bits(name, k, None)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", [n for n in C.NAMES if n not in C.TINY])
def test_capped_is_bit_equal(name, which, k):
    check_bits(name, k, C.RADII[name][which])


@pytest.mark.parametrize("radius", (None, 0.3, 2.0))
@pytest.mark.parametrize("name", C.TINY)
def test_tiny_clouds_pad_their_rows(name, radius):
    check_bits(name, 8, radius)
    q, s = clouds(name)
    got_d, got_i = cloud_nn.knn(q, s, 8, radius)
    ns = s.shape[0]
    assert (got_i[:, ns:] == -1).all() and torch.isinf(got_d[:, ns:]).all()
    if radius is None:
        assert (got_i[:, :ns] >= 0).all()


def test_disjoint_clouds():
    """Ten extents apart: every capped row is empty, every uncapped row is found by the fallback."""
    q, s = clouds("disjoint_4096")
    for radius in C.RADII["disjoint_4096"]:
        d, i = cloud_nn.knn(q, s, 3, radius)
        assert (i == -1).all() and torch.isinf(d).all()
    d, i = cloud_nn.knn(q, s, 3)
    assert (i >= 0).all() and (d > 64.0).all()


def test_identical_clouds_find_themselves():
    q, s = clouds("identical_clouds")
    d, i = cloud_nn.knn(q, s, 1)
    assert (d == 0).all() and torch.equal(i[:, 0], torch.arange(q.shape[0], device="cuda"))


def test_duplicate_support_points_lower_index_wins():
    q, s = clouds("dyadic")
    d, i = cloud_nn.knn(s[:100].contiguous(), s, 2)
    assert (d == 0).all()
    assert torch.equal(i[:, 0], torch.arange(100, device="cuda")) and (i[:, 1] > i[:, 0]).all()


def test_no_queries():
    s = clouds("plane")[1]
    q = torch.empty((0, 3), device="cuda")
    d, i = cloud_nn.knn(q, s, 3, 0.1)
    assert d.shape == (0, 3) and i.shape == (0, 3)
    assert cloud_nn.radius_pairs(q, s, 0.1).shape == (0, 2)
    assert cloud_nn.nearest(q, s).shape == (0,)


# ---- radius_pairs ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", C.NAMES)
def test_radius_pairs_equal_the_brute_force(name, which):
    q, s = clouds(name)
    radius = C.RADII[name][which]
    want = R.pairs_f32_torch(q, s, R.r2_of(radius))
    got = cloud_nn.radius_pairs(q, s, radius)
    assert got.dtype == torch.int64 and got.shape == want.shape, (got.shape, want.shape)
    assert torch.equal(got, want)
    if name == "disjoint_4096":
        assert got.shape[0] == 0
    if name == "blobs" and which == 1:  # the wave-ordered long rows
        assert torch.bincount(want[:, 0]).max().item() > 1024
    if name == "identical_clouds" and which == 0:
        assert got.shape[0] >= q.shape[0]


# ---- float64 ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def half_f64():
    q, s = C.half_pair()
    d64, i64 = R.knn_f64(q, s, 8)
    d32, i32 = R.knn_f32(q, s, 8)
    return q, s, d64, i64, d32, i32


def test_against_float64():
    q, s, d64, i64, d32, i32 = half_f64()
    assert np.array_equal(i32, i64)
    own = np.abs(d32.astype(np.float64) - d64) / d64
    print("fp32 brute force against float64: max relative error", own.max())
    assert own.max() <= 2.5e-7
    got_d, got_i = cloud_nn.knn(torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda(), 8)
    assert np.array_equal(got_i.cpu().numpy(), i64)
    err = np.abs(got_d.cpu().numpy().astype(np.float64) - d64) / d64
    print("kernel against float64: max relative error", err.max())
    assert err.max() <= 4 * own.max()


def test_overlap_equals_float64():
    q, s = C.half_pair()
    want = R.overlap_f64(q, s, None, 0.05)
    assert want == 4239 / 8192      # 0.5175 to four places
    qd, sd = torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda()
    assert cloud_nn.compute_overlap(qd, sd, None, 0.05) == want
    assert gaussreg_amd.compute_overlap(qd, sd, positive_radius=0.05) == want
    # the capped search behind it decides as the uncapped one does
    assert int((cloud_nn.nearest(qd, sd).double() < 0.05).sum()) / 8192 == want


def _transform(seed, angle, shift):
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K
    T[:3, 3] = shift
    return T


SLACK = 2.0 ** -20


def test_wrappers_against_float64():
    """ref = q; src = s moved by the inverse of gt, so that gt brings the pair back to the one above.  gt is a quarter turn
    about z: it moves fp32 coordinates without rounding, in fp32 as in float64, so that the counts below differ from
    float64's by the rounding of the distance alone (2.5e-7 relative, above) and the 2^-20 margin is the right one."""
    q, s = C.half_pair()
    q, n = q[:2048].copy(), 2048          # a quarter of the queries keeps the float64 distance matrix small
    gt = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    src = R.apply_transform_f64(s, np.linalg.inv(gt)).astype(np.float32)
    assert np.array_equal(R.apply_transform_f64(src, gt), s.astype(np.float64))
    est = gt @ _transform(2, 0.01, [0.004, -0.003, 0.002])
    ref_d, src_d = torch.from_numpy(q).cuda(), torch.from_numpy(src).cuda()
    r = 0.05
    # correspondences: exact wherever float64 separates the distance from the radius by more than 2^-20 relative
    want, d = R.correspondences_f64(q, src, gt, r)
    got = cloud_nn.get_correspondences(ref_d, src_d, gt, r).cpu().numpy()
    unsure = np.abs(d - r * r) <= SLACK * r * r
    assert unsure.sum() <= 1e-3 * max(len(want), 1)
    keep = lambda p: p[~unsure[p[:, 0], p[:, 1]]]
    assert np.array_equal(keep(got), keep(want))
    assert got.shape[0] > n and np.all(np.diff(got[:, 0] * 8192 + got[:, 1]) > 0)
    # overlap under the transform
    near = R.nearest_f64(q, R.apply_transform_f64(src, gt))[0]
    unsure = np.abs(near - r) <= SLACK * r
    assert unsure.mean() <= 1e-3
    got_overlap = cloud_nn.compute_overlap(ref_d, src_d, gt, r)
    assert abs(got_overlap - float(np.mean(near < r))) <= unsure.sum() / n
    # chamfer, rmse, residual: means of fp32 distances between points of size ~1 that were transformed in fp32: a coordinate
    # is off by a few 2^-24, a distance by no more than the coordinates it comes from, well under 1e-5; the means no more
    raw = q
    cd = cloud_nn.compute_modified_chamfer_distance(ref_d, ref_d, src_d, gt, est)
    assert abs(cd - R.chamfer_f64(raw, q, src, gt, est)) <= 1e-5
    assert abs(cloud_nn.compute_registration_rmse(src_d, gt, est) - R.rmse_f64(src, gt, est)) <= 1e-5
    # correspondences of a matcher: the nearest src point of every ref point under est
    _, j = cloud_nn.nearest(ref_d, cloud_nn.apply_transform(src_d, est), return_index=True)
    src_corr = src[j.cpu().numpy()]
    res = R.residuals_f64(q, src_corr, gt)
    unsure = np.abs(res - r) <= SLACK * r
    assert unsure.mean() <= 1e-3
    src_corr_d = torch.from_numpy(src_corr).cuda()
    ir = cloud_nn.compute_inlier_ratio(ref_d, src_corr_d, gt, r)
    assert abs(ir - float(np.mean(res < r))) <= unsure.sum() / n
    assert abs(cloud_nn.compute_correspondence_residual(ref_d, src_corr_d, gt) - res.mean()) <= 1e-5
    ev = cloud_nn.evaluate_correspondences(ref_d, src_corr_d, gt, r)
    assert set(ev) == {"overlap", "inlier_ratio", "residual", "num_corr"} and ev["num_corr"] == n
    assert ev["inlier_ratio"] == ir and 0.0 < ev["overlap"] <= 1.0


# ---- properties -----------------------------------------------------------------------------------------------------------------

def test_capped_equals_uncapped_within_the_cap():
    q, s = clouds("half_8192")
    full_d, full_i = cloud_nn.knn(q, s, 8)
    for radius in C.RADII["half_8192"]:
        d, i = cloud_nn.knn(q, s, 8, radius)
        inside = full_d <= float(R.r2_of(radius))
        assert torch.equal(i, torch.where(inside, full_i, -1))
        assert same_bits(d, torch.where(inside, full_d, INF))


def test_relabelling_permutes_the_result():
    q, s = clouds("half_8192")
    d, i = cloud_nn.knn(q, s, 8, 0.1)
    perm = torch.randperm(s.shape[0], generator=torch.Generator().manual_seed(1)).cuda()   # new -> old
    inverse = torch.empty_like(perm)
    inverse[perm] = torch.arange(s.shape[0], device="cuda")
    d2, i2 = cloud_nn.knn(q, s[perm].contiguous(), 8, 0.1)
    assert same_bits(d, d2)
    assert torch.equal(i2, torch.where(i >= 0, inverse[i.clamp_min(0)], -1))


def test_two_calls_and_another_stream_give_the_same_bits():
    q, s = clouds("outliers_both")
    first = cloud_nn.knn(q, s, 8), cloud_nn.radius_pairs(q, s, 0.2)
    again = cloud_nn.knn(q, s, 8), cloud_nn.radius_pairs(q, s, 0.2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = cloud_nn.knn(q, s, 8), cloud_nn.radius_pairs(q, s, 0.2)
    side.synchronize()
    for (d, i), p in (again, other):
        assert same_bits(d, first[0][0]) and torch.equal(i, first[0][1]) and torch.equal(p, first[1])


def _abi(name, *args):
    ptrs = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    return getattr(_lib.lib(), name)(*ptrs, torch.cuda.current_stream().cuda_stream)


def test_every_combination_of_outputs_through_the_c_abi():
    q, s = clouds("uniform_257_4097")
    want_d, want_i = expected("uniform_257_4097", None)
    ws = torch.empty(_lib.lib().gr_cloud_knn_workspace_bytes(257, 4097, 3), dtype=torch.uint8, device="cuda")
    for with_d in (False, True):
        for with_i in (False, True):
            d = torch.full((257, 3), 5.0, device="cuda") if with_d else None
            i = torch.full((257, 3), 5, dtype=torch.int64, device="cuda") if with_i else None
            assert _abi("gr_cloud_knn", q, 257, s, 4097, 3, INF, d, i, ws, ws.numel()) == 0
            torch.cuda.synchronize()
            assert d is None or same_bits(d, want_d[:, :3])
            assert i is None or torch.equal(i, want_i[:, :3])
    # the pair search: the per-query counts are optional
    want = R.pairs_f32_torch(q, s, R.r2_of(0.2))
    ws = torch.empty(_lib.lib().gr_cloud_radius_workspace_bytes(257, 4097), dtype=torch.uint8, device="cuda")
    for with_count in (False, True):
        count = torch.full((257,), -1, dtype=torch.int32, device="cuda") if with_count else None
        total = ctypes.c_int64(-1)
        assert _abi("gr_cloud_radius_count", q, 257, s, 4097, float(R.r2_of(0.2)), count, ctypes.byref(total), ws, ws.numel()) == 0
        assert total.value == want.shape[0]
        assert count is None or torch.equal(count.long(), torch.bincount(want[:, 0], minlength=257))
        scratch = torch.empty(total.value, dtype=torch.int32, device="cuda")
        pairs = torch.empty((total.value, 2), dtype=torch.int64, device="cuda")
        assert _abi("gr_cloud_radius_pairs", q, 257, s, 4097, float(R.r2_of(0.2)), total.value, scratch, pairs, ws, ws.numel()) == 0
        torch.cuda.synchronize()
        assert torch.equal(pairs, want)
    # a total other than the one the workspace holds is refused before anything is written
    assert _abi("gr_cloud_radius_pairs", q, 257, s, 4097, float(R.r2_of(0.2)), total.value - 1, scratch, pairs, ws, ws.numel()) != 0


def test_c_abi_refuses_bad_arguments():
    q, s = clouds("uniform_257_4097")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    d = torch.full((257, 8), 5.0, device="cuda")
    i = torch.full((257, 8), 5, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(0)
    nan_q, nan_s = q.clone(), s.clone()
    nan_q[100, 1] = math.nan
    nan_s[4000, 2] = math.inf
    bad = [("gr_cloud_knn", (q, 257, s, 4097, 0, INF, d, i, ws, ws.numel())),
           ("gr_cloud_knn", (q, 257, s, 4097, 9, INF, d, i, ws, ws.numel())),
           ("gr_cloud_knn", (q, 257, s, 0, 1, INF, d, i, ws, ws.numel())),
           ("gr_cloud_knn", (q, -1, s, 4097, 1, INF, d, i, ws, ws.numel())),
           ("gr_cloud_knn", (q, 257, s, 4097, 1, -1.0, d, i, ws, ws.numel())),
           ("gr_cloud_knn", (q, 257, s, 4097, 1, math.nan, d, i, ws, ws.numel())),
           ("gr_cloud_knn", (q, 257, s, 4097, 1, INF, d, i, ws, 1024)),
           ("gr_cloud_knn", (nan_q, 257, s, 4097, 1, INF, d, i, ws, ws.numel())),
           ("gr_cloud_knn", (q, 257, nan_s, 4097, 1, INF, d, i, ws, ws.numel())),
           ("gr_cloud_radius_count", (q, 257, s, 0, 0.01, None, ctypes.byref(total), ws, ws.numel())),
           ("gr_cloud_radius_count", (q, 257, s, 4097, -0.01, None, ctypes.byref(total), ws, ws.numel())),
           ("gr_cloud_radius_count", (q, 257, s, 4097, 0.01, None, ctypes.byref(total), ws, 1024)),
           ("gr_cloud_radius_count", (nan_q, 257, s, 4097, 0.01, None, ctypes.byref(total), ws, ws.numel())),
           ("gr_cloud_radius_count", (q, 257, nan_s, 4097, 0.01, None, ctypes.byref(total), ws, ws.numel()))]
    for name, args in bad:
        assert _abi(name, *args) != 0, (name, args[1:6])
        assert _lib.lib().gr_last_error()
    torch.cuda.synchronize()
    assert (d == 5.0).all() and (i == 5).all()     # nothing was written


def test_errors():
    q, s = clouds("plane")
    for k in (0, 9, True, 1.0):
        with pytest.raises(ValueError, match="k = "):
            cloud_nn.knn(q, s, k)
    with pytest.raises(ValueError, match="no CPU fallback"):
        cloud_nn.knn(q.cpu(), s)
    with pytest.raises(ValueError, match="no CPU fallback"):
        cloud_nn.radius_pairs(q, s.cpu(), 0.1)
    with pytest.raises(ValueError, match="float32"):
        cloud_nn.knn(q.double(), s)
    with pytest.raises(ValueError, match="shape"):
        cloud_nn.knn(q[:, :2], s)
    with pytest.raises(ValueError, match="contiguous"):
        cloud_nn.knn(q, s[::2])
    with pytest.raises(ValueError, match="at least 1"):
        cloud_nn.knn(q, s[:0])
    with pytest.raises(ValueError, match="max_dist"):
        cloud_nn.knn(q, s, 1, -0.5)
    bad = q.clone()
    bad[3, 0] = math.nan
    with pytest.raises(ValueError, match="points must be finite"):
        cloud_nn.knn(bad, s)
    with pytest.raises(ValueError, match="points must be finite"):
        cloud_nn.radius_pairs(s, bad, 0.1)


# ---- aliases and the example -----------------------------------------------------------------------------------------------------

def test_numpy_aliases_return_numpy_and_match():
    from geotransformer.utils import pointcloud, registration
    q, s = C.pair("uniform_257_4097")
    qd, sd = clouds("uniform_257_4097")
    T = _transform(3, 0.2, [0.1, 0.0, -0.1])
    dist, idx = pointcloud.get_nearest_neighbor(q, s, return_index=True)
    assert isinstance(dist, np.ndarray) and isinstance(idx, np.ndarray) and idx.dtype == np.int64
    want_d, want_i = cloud_nn.nearest(qd, sd, return_index=True)
    assert np.array_equal(dist, want_d.cpu().numpy()) and np.array_equal(idx, want_i.cpu().numpy())
    assert isinstance(pointcloud.get_nearest_neighbor(q, s), np.ndarray)
    corr = registration.get_correspondences(q, s, T, 0.1)
    assert isinstance(corr, np.ndarray) and corr.dtype == np.int64
    assert np.array_equal(corr, cloud_nn.get_correspondences(qd, sd, T, 0.1).cpu().numpy())
    assert registration.compute_overlap(q, s, T, 0.1) == cloud_nn.compute_overlap(qd, sd, T, 0.1)
    assert registration.compute_overlap(q, s) == cloud_nn.compute_overlap(qd, sd)
    gt = _transform(4, 0.21, [0.1, 0.01, -0.1])
    assert registration.compute_modified_chamfer_distance(q, q, s, gt, T) == \
        cloud_nn.compute_modified_chamfer_distance(qd, qd, sd, gt, T)
    assert registration.compute_registration_rmse(s, gt, T) == cloud_nn.compute_registration_rmse(sd, gt, T)
    assert registration.compute_inlier_ratio(q, s[:257], T, 0.3) == cloud_nn.compute_inlier_ratio(qd, sd[:257].contiguous(), T, 0.3)
    assert registration.compute_correspondence_residual(q, s[:257], T) == \
        cloud_nn.compute_correspondence_residual(qd, sd[:257].contiguous(), T)
    assert registration.evaluate_correspondences(q, s[:257], T, 0.3)["num_corr"] == 257
    # tensors in, tensors out
    assert isinstance(registration.get_correspondences(qd, sd, T, 0.1), torch.Tensor)


def test_package_root_exports_the_reference_names():
    for name in cloud_nn.REFERENCE_NAMES:
        assert getattr(gaussreg_amd, name) is getattr(cloud_nn, name)


def test_example_evaluates_a_synthetic_pair():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "register_scenes.py"), "--synthetic", "--evaluate"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    for line in r.stdout.splitlines():
        for key in ("overlap", "inlier ratio", "modified chamfer distance"):
            if line.strip().startswith(key):
                found[key] = float(line.split(":")[1].split()[0])
    assert set(found) == {"overlap", "inlier ratio", "modified chamfer distance"}, r.stdout
    assert all(math.isfinite(v) for v in found.values()), found
    assert 0.0 <= found["overlap"] <= 1.0 and 0.0 <= found["inlier ratio"] <= 1.0
