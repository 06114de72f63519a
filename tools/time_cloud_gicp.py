"""Time of generalised ICP and of the covariance kernels (gaussreg_amd.icp.icp_generalized, gaussreg_amd.covariances) on the
half-overlapping pairs of tools/time_cloud_icp.py, with `icp_point_to_plane` and the same loop composed from `cloud_nn.knn`
and torch float64 timed in the same run beside it.

  pair          uniform unit cubes, the reference moved by half an extent (50 % overlap); the source starts 1 degree and
                0.002 away from the identity, max_dist = 2 (1 / N)^(1/3); normals by estimate_normals(k=8), covariances
                from them (the plane prior, epsilon = 1e-3) for both clouds
  covariances   the kernels' own times are the library's "cloud_covariances" / "gs_covariances" event timers; their bytes
                are what they ask for -- 12 B read and 24 B written per normal; 28 B read and 24 B (+ 12 B + 1 B with the
                normals and the validity) written per Gaussian -- set against the 8.0 TB/s HBM peak of the MI355X
  icp           each call runs `--iterations` iterations with the stop test disabled (relative_* = 0); a run that ends early
                (degenerate) is reported with the iterations it did.  Device events on one stream around each whole call (a
                call includes its read-back), 2 warm-up rounds, median / min / max of `--reps` rounds, one process
  composed      the generalised update written with what the package had before: one knn call per iteration (grid and
                query order rebuilt), the 3x3 inverses and the 6x6 sums in torch float64, torch.linalg.solve, one read-back
  presorted     the library reads src_cov through the original source index every round; an ordered copy, gathered once
                into the loop's cell order, is not built.  What it could win is estimated here instead: the same pair with the
                source rows (points and covariances) permuted beforehand into the lexicographic cell order of a grid of
                about one point per cell, so that the indexed reads are roughly sequential -- the same matches, the same
                arithmetic.  An estimate, not a bound: the loop orders by the reference's quantile grid, not this one, and
                the presort also makes the one-off gather of src cheaper
  room          the iterations each estimator needs on the room_rigid pair of tests/cloud_gicp_cases.py

    python tools/time_cloud_gicp.py [--sizes 100000 1000000] [--iterations 30] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussreg_amd import _lib, cloud_nn  # noqa: E402
from gaussreg_amd.covariances import covariances_from_gaussians, covariances_from_normals, estimate_covariances  # noqa: E402
from gaussreg_amd.icp import icp_generalized, icp_point_to_plane  # noqa: E402
from gaussreg_amd.normals import estimate_normals  # noqa: E402
from time_cloud_icp import library_timer, pair, stats, timed  # noqa: E402

HBM_PEAK = 8.0e12
K = 8


def full(c6):
    return c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].double().reshape(-1, 3, 3)


def cross_matrix(p):
    K3 = torch.zeros((p.shape[0], 3, 3), dtype=p.dtype, device=p.device)
    K3[:, 0, 1], K3[:, 0, 2], K3[:, 1, 0] = -p[:, 2], p[:, 1], p[:, 2]
    K3[:, 1, 2], K3[:, 2, 0], K3[:, 2, 1] = -p[:, 0], -p[:, 1], p[:, 0]
    return K3


def composed(src, ref, src_cov, ref_cov, T0, max_dist, iterations):
    """Generalised ICP from the package's older parts; rigid, no stop test."""
    T = torch.as_tensor(T0, device=src.device)
    Cs, Ct = full(src_cov), full(ref_cov)
    eye = torch.eye(3, dtype=torch.float64, device=src.device)
    for _ in range(iterations + 1):
        p = ((T[:3, 0] * src[:, :1] + T[:3, 1] * src[:, 1:2]) + T[:3, 2] * src[:, 2:3]) + T[:3, 3]
        d2, j = cloud_nn.knn(p.contiguous(), ref, 1, max_dist)
        m = j[:, 0] >= 0
        n = int(m.sum())                                   # the read-back of this iteration
        if n < 3:
            break
        A = T[:3, :3].double()
        pm, q = p[m].double(), ref[j[m, 0]].double()
        W = torch.linalg.inv(Ct[j[m, 0]] + A @ Cs[m] @ A.T)
        J = torch.cat([-cross_matrix(pm), eye.expand(n, 3, 3)], dim=2)
        JW = J.transpose(1, 2) @ W
        x = -torch.linalg.solve((JW @ J).sum(0), (JW @ (pm - q)[:, :, None]).sum(0)[:, 0])
        ca, sa, cb, sb, cg, sg = (f(x[k]) for k in range(3) for f in (torch.cos, torch.sin))
        dT = torch.eye(4, dtype=torch.float64, device=src.device)
        dT[:3, :3] = torch.stack([cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, sg * cb, sg * sb * sa + cg * ca,
                                  sg * sb * ca - cg * sa, -sb, cb * sa, cb * ca]).reshape(3, 3)
        dT[:3, 3] = x[3:]
        T = (dT @ T.double()).float()
    return T


def cell_order(points):
    """The permutation that sorts `points` by (z, y, x) cell of a uniform grid of about one point per cell."""
    D = max(1, round(points.shape[0] ** (1 / 3)))
    lo, hi = points.min(0).values, points.max(0).values
    c = ((points - lo) / (hi - lo) * D).long().clamp_(0, D - 1)
    return torch.argsort((c[:, 2] * D + c[:, 1]) * D + c[:, 0], stable=True)


def kernel_time(name, call, reps):
    _lib.lib().gr_timing_enable(1)
    _lib.lib().gr_timing_reset()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    ms = library_timer(name)
    _lib.lib().gr_timing_enable(0)
    return ms


def room():
    import cloud_gicp_cases
    c = cloud_gicp_cases.case("room_rigid")
    src, ref = torch.from_numpy(c["src"]).cuda(), torch.from_numpy(c["ref"]).cuda()
    a = icp_point_to_plane(src, ref, estimate_normals(ref, k=K), c["T0"], max_dist=c["max_dist"])
    b = icp_generalized(src, ref, estimate_covariances(src, k=K), estimate_covariances(ref, k=K), c["T0"], max_dist=c["max_dist"])
    print(json.dumps({"pair": "room_rigid", "point_to_plane": {"status": a.status, "iterations": a.iterations,
                                                               "inlier_rmse": round(a.inlier_rmse, 6)},
                      "generalized": {"status": b.status, "iterations": b.iterations, "inlier_rmse": round(b.inlier_rmse, 6)}}),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composed_reps", type=int, default=2, help="rounds of the composed loop (it is slow)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    for N in args.sizes:
        src, ref, T0, r = pair(N, dev)
        its = args.iterations
        base = {"N": N, "iterations": its, "max_dist": round(r, 5)}
        ref_normals, src_normals = estimate_normals(ref, k=K), estimate_normals(src, k=K)
        g = torch.Generator(device="cpu").manual_seed(1)
        scales = (torch.rand((N, 3), generator=g) * 0.1 + 0.01).to(dev)
        rotations = torch.randn((N, 4), generator=g).to(dev)
        kernels = (("covariances_from_normals", "cloud_covariances", lambda: covariances_from_normals(ref_normals), 12 + 24),
                   ("covariances_from_gaussians(plane)", "gs_covariances", lambda: covariances_from_gaussians(scales, rotations), 28 + 24),
                   ("covariances_from_gaussians(plane, return_normals)", "gs_covariances",
                    lambda: covariances_from_gaussians(scales, rotations, return_normals=True), 28 + 24 + 12 + 1),
                   ("covariances_from_gaussians(raw)", "gs_covariances", lambda: covariances_from_gaussians(scales, rotations, mode="raw"),
                    28 + 24))
        for label, timer, call, per_row in kernels:
            call()
            ms = kernel_time(timer, call, args.reps)
            asked = N * per_row
            print(json.dumps({"N": N, "call": label, "ms_kernel": round(ms, 4), "bytes_requested": asked,
                              "TBps_requested": round(asked / (ms * 1e-3) / 1e12, 3),
                              "of_hbm_peak": round(asked / (ms * 1e-3) / HBM_PEAK, 3)}), flush=True)
        src_cov, ref_cov = covariances_from_normals(src_normals), covariances_from_normals(ref_normals)
        perm = cell_order(src)
        src_p, src_cov_p = src[perm].contiguous(), src_cov[perm].contiguous()
        calls = {"icp_generalized": lambda k=its: icp_generalized(src, ref, src_cov, ref_cov, T0, max_dist=r, max_iterations=k,
                                                                  relative_fitness=0.0, relative_rmse=0.0),
                 "icp_generalized, source presorted": lambda k=its: icp_generalized(src_p, ref, src_cov_p, ref_cov, T0, max_dist=r,
                                                                                    max_iterations=k, relative_fitness=0.0,
                                                                                    relative_rmse=0.0),
                 "icp_point_to_plane": lambda k=its: icp_point_to_plane(src, ref, ref_normals, T0, max_dist=r, max_iterations=k,
                                                                        relative_fitness=0.0, relative_rmse=0.0)}
        for name, call in calls.items():
            res, t = timed(call, args.reps, 2)
            _, t0 = timed(lambda: call(0), args.reps, 2)
            whole, zero = statistics.median(t), statistics.median(t0)
            print(json.dumps({**base, "call": name, "status": res.status, "done": res.iterations, "fitness": round(res.fitness, 4),
                              **stats(t), "ms_evaluation_only": round(zero, 3),
                              "ms_per_iteration": round((whole - zero) / max(res.iterations, 1), 4)}), flush=True)
        Tc, t = timed(lambda: composed(src, ref, src_cov, ref_cov, T0, r, its), args.composed_reps, 1)
        Tg = calls["icp_generalized"]().transform
        print(json.dumps({**base, "call": "composed (cloud_nn.knn + torch float64)", **stats(t),
                          "max_abs_difference_to_icp_generalized": float((Tc - Tg).abs().max())}), flush=True)
    room()


if __name__ == "__main__":
    main()
