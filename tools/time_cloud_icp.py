"""Time of point-to-point ICP (gaussreg_amd.icp: grid built once, match / sums / fold per iteration, one read-back) on
half-overlapping pairs of N x N points, beside the same loop composed from what the library offered before it:
cloud_nn.knn + torch fp64 sums + torch.linalg.svd, one read-back per iteration.

  pair   uniform unit cubes, the reference moved by half an extent (50 % overlap); the source starts 1 degree and 0.002 away
         from the identity, max_dist = 2 (1 / N)^(1/3), rigid fit

Both run `--iterations` iterations with the stop test disabled (relative_* = 0).  Device events on one stream around each
whole call (a call includes its host read-backs), 2 warm-up rounds, median / min / max of `--reps` rounds, one process.  The
split of the fused call into "cloud_icp_grid" and "cloud_icp_iterate" comes from the library's own event timers
(gr_timing_*), in rounds of their own.

    python tools/time_cloud_icp.py [--sizes 100000 1000000] [--iterations 30] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from gaussreg_amd import _lib, cloud_nn  # noqa: E402
from gaussreg_amd.icp import icp  # noqa: E402


def pair(N, dev):
    rng = np.random.default_rng(0)
    src = rng.random((N, 3)).astype(np.float32)
    ref = (rng.random((N, 3)) + [0.5, 0, 0]).astype(np.float32)
    a = np.deg2rad(1.0)
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T0[:3, 3] = [0.002, -0.001, 0.001]
    return torch.from_numpy(src).to(dev), torch.from_numpy(ref).to(dev), T0, 2.0 * (1.0 / N) ** (1 / 3)


def composed(src, ref, T0, max_dist, iterations):
    """The loop as it could be written before: one knn call (grid and query order rebuilt), torch fp64 sums, SVD and one
    read-back (the matched count) per iteration.  Rigid fit; no stop test."""
    T = torch.as_tensor(T0, device=src.device)
    src64 = src.double()
    for _ in range(iterations + 1):
        p = ((T[:3, 0] * src[:, :1] + T[:3, 1] * src[:, 1:2]) + T[:3, 2] * src[:, 2:3]) + T[:3, 3]
        d2, j = cloud_nn.knn(p.contiguous(), ref, 1, max_dist)
        m = j[:, 0] >= 0
        n = int(m.sum())                                   # the read-back of this iteration
        if n < 3:
            break
        a, b = src64[m], ref[j[m, 0]].double()
        ca, cb = a.mean(0), b.mean(0)
        H = (a - ca).T @ (b - cb)
        U, _, Vt = torch.linalg.svd(H)
        D = torch.eye(3, dtype=torch.float64, device=src.device)
        D[2, 2] = torch.sign(torch.linalg.det(Vt.T @ U.T))
        R = Vt.T @ D @ U.T
        T = torch.eye(4, dtype=torch.float64, device=src.device)
        T[:3, :3], T[:3, 3] = R, cb - R @ ca
        T = T.float()
    return T


def timed(fn, reps, warmup):
    times = []
    for r in range(warmup + reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        if r >= warmup:
            times.append(start.elapsed_time(stop))
    return out, times


def stats(times):
    return {"ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3)}


def library_timer(name):
    total, calls = ctypes.c_double(0), ctypes.c_int64(0)
    _lib.lib().gr_timing_read(name.encode(), ctypes.byref(total), ctypes.byref(calls))
    return total.value / max(calls.value, 1)


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
        fused = lambda k=its: icp(src, ref, T0, max_dist=r, max_iterations=k, relative_fitness=0.0, relative_rmse=0.0)
        res, t = timed(fused, args.reps, 2)
        _, t0 = timed(lambda: fused(0), args.reps, 2)
        whole, zero = statistics.median(t), statistics.median(t0)
        base = {"N": N, "iterations": its, "max_dist": round(r, 5)}
        print(json.dumps({**base, "call": "icp", "status": res.status, "done": res.iterations, "fitness": round(res.fitness, 4),
                          **stats(t), "ms_evaluation_only": round(zero, 3), "ms_per_iteration": round((whole - zero) / its, 4)}),
              flush=True)
        _lib.lib().gr_timing_enable(1)
        _lib.lib().gr_timing_reset()
        for _ in range(args.reps):
            fused()
        print(json.dumps({**base, "call": "icp, library timers", "ms_cloud_icp_grid": round(library_timer("cloud_icp_grid"), 3),
                          "ms_cloud_icp_iterate": round(library_timer("cloud_icp_iterate"), 3)}), flush=True)
        _lib.lib().gr_timing_enable(0)
        _, tc = timed(lambda: composed(src, ref, T0, r, its), args.reps, 2)
        _, tk = timed(lambda: cloud_nn.knn(src, ref, 1, r), args.reps, 2)
        print(json.dumps({**base, "call": "composed: knn + torch sums + svd", **stats(tc),
                          "ms_per_iteration": round(statistics.median(tc) / (its + 1), 4),
                          "ratio_composed_over_icp": round(statistics.median(tc) / whole, 2)}), flush=True)
        print(json.dumps({**base, "call": "one capped knn k=1", **stats(tk)}), flush=True)


if __name__ == "__main__":
    main()
