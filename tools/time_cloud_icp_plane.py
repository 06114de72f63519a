"""Time of PCA normals and point-to-plane ICP (gaussreg_amd.normals, gaussreg_amd.icp.icp_point_to_plane) on the
half-overlapping pairs of tools/time_cloud_icp.py, with point-to-point `icp` timed in the same run beside them.

  pair      uniform unit cubes, the reference moved by half an extent (50 % overlap); the source starts 1 degree and 0.002
            away from the identity, max_dist = 2 (1 / N)^(1/3), rigid fit
  normals   estimate_normals(ref, k=8): scene_init.knn, then the normals kernel.  The kernel's own time is the library's
            "cloud_normals" event timer; its bytes are what it asks for -- per point K indices of 8 B, K + 1 points of 12 B and
            one normal of 12 B written -- set against the 8.0 TB/s HBM peak of the MI355X.  Neighbouring queries share
            neighbours, so the bytes that reach HBM are fewer: the figure is a request rate, not a DRAM rate.
  icp       both estimators run `--iterations` iterations with the stop test disabled (relative_* = 0); a run that ends early
            (degenerate) is reported with the iterations it did.  Device events on one stream around each whole call (a call
            includes its read-back), 2 warm-up rounds, median / min / max of `--reps` rounds, one process.
  room      the iterations each estimator needs on the room_rigid pair of tests/cloud_icp_cases.py (12 288 points, a 4 degree
            and 13 cm perturbation, max_dist 0.1) under the default stop rule.

    python tools/time_cloud_icp_plane.py [--sizes 100000 1000000] [--iterations 30] [--reps 5]
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

from gaussreg_amd import _lib, scene_init  # noqa: E402
from gaussreg_amd.icp import icp, icp_point_to_plane  # noqa: E402
from gaussreg_amd.normals import estimate_normals, normals_from_neighbors  # noqa: E402
from time_cloud_icp import library_timer, pair, stats, timed  # noqa: E402

HBM_PEAK = 8.0e12
K = 8


def room():
    import cloud_icp_cases
    c = cloud_icp_cases.case("room_rigid")
    src, ref = torch.from_numpy(c["src"]).cuda(), torch.from_numpy(c["ref"]).cuda()
    a = icp(src, ref, c["T0"], max_dist=c["max_dist"])
    b = icp_point_to_plane(src, ref, estimate_normals(ref, k=K), c["T0"], max_dist=c["max_dist"])
    print(json.dumps({"pair": "room_rigid", "point_to_point": {"status": a.status, "iterations": a.iterations,
                                                               "inlier_rmse": round(a.inlier_rmse, 6)},
                      "point_to_plane": {"status": b.status, "iterations": b.iterations, "inlier_rmse": round(b.inlier_rmse, 6)}}),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda")
    for N in args.sizes:
        src, ref, T0, r = pair(N, dev)
        its = args.iterations
        base = {"N": N, "iterations": its, "max_dist": round(r, 5)}
        normals, tn = timed(lambda: estimate_normals(ref, k=K), args.reps, 2)
        (_, table), tk = timed(lambda: scene_init.knn(ref, K), args.reps, 2)
        _lib.lib().gr_timing_enable(1)
        _lib.lib().gr_timing_reset()
        for _ in range(args.reps):
            normals_from_neighbors(ref, table, include_self=True)
        kernel_ms = library_timer("cloud_normals")
        _lib.lib().gr_timing_enable(0)
        asked = N * (8 * K + 12 * (K + 1) + 12)
        print(json.dumps({**base, "call": f"estimate_normals(k={K})", **stats(tn), "ms_knn_alone": round(statistics.median(tk), 3),
                          "ms_normals_kernel": round(kernel_ms, 4), "bytes_requested": asked,
                          "TBps_requested": round(asked / (kernel_ms * 1e-3) / 1e12, 3),
                          "of_hbm_peak": round(asked / (kernel_ms * 1e-3) / HBM_PEAK, 3)}), flush=True)
        calls = {"icp_point_to_plane": lambda k=its: icp_point_to_plane(src, ref, normals, T0, max_dist=r, max_iterations=k,
                                                                        relative_fitness=0.0, relative_rmse=0.0),
                 "icp": lambda k=its: icp(src, ref, T0, max_dist=r, max_iterations=k, relative_fitness=0.0, relative_rmse=0.0)}
        for name, call in calls.items():
            res, t = timed(call, args.reps, 2)
            _, t0 = timed(lambda: call(0), args.reps, 2)
            whole, zero = statistics.median(t), statistics.median(t0)
            print(json.dumps({**base, "call": name, "status": res.status, "done": res.iterations, "fitness": round(res.fitness, 4),
                              **stats(t), "ms_evaluation_only": round(zero, 3),
                              "ms_per_iteration": round((whole - zero) / max(res.iterations, 1), 4)}), flush=True)
    room()


if __name__ == "__main__":
    main()
