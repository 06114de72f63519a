"""Time of the cross-cloud search (gaussreg_amd.cloud_nn: quantile grid over the support, shell search, wave fallback) on
pairs of N x N points, beside a chunked stock-torch brute force and scipy's cKDTree on the host where they can run.

  half       uniform unit cubes, the support moved by half an extent: 50 % overlap
  clustered  the means of synthetic.gaussians_c2 (two seeds), the support moved by half the box's x extent
  disjoint   uniform unit cubes ten extents apart, uncapped only: every query goes through the fallback

Per pair: knn(k=1) capped at r = 2 (volume / N)^(1/3) (a radius that leaves the overlap at about 50 %), knn(k=1) uncapped,
radius_pairs at r.  Device events around each whole call (a call includes its host read-back), 2 warm-up rounds, median /
min / max of `--reps` rounds, one process.  The brute force (row chunks of a chunk x N distance matrix and min) is timed up
to `--brute-max` points, the k-d tree (build + capped query, up to 16 threads) up to `--tree-max`, once each.

    python tools/time_cloud_nn.py [--sizes 100000 1000000] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from gaussreg_amd import cloud_nn, synthetic  # noqa: E402


def pairs(N, dev):
    rng = np.random.default_rng(0)
    u = lambda: rng.random((N, 3)).astype(np.float32)
    c2 = lambda seed: synthetic.gaussians_c2(N, seed=seed)["means3D"].astype(np.float32)
    out = {"half": (u(), u() + np.array([0.5, 0, 0], np.float32), 1.0),
           "clustered": (c2(0), c2(1) + np.array([2.0, 0, 0], np.float32), 30.0),
           "disjoint": (u(), u() + np.array([10.0, 0, 0], np.float32), 1.0)}
    return {k: (torch.from_numpy(q).to(dev), torch.from_numpy(np.ascontiguousarray(s, np.float32)).to(dev), 2.0 * (v / N) ** (1 / 3))
            for k, (q, s, v) in out.items()}


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


def brute_force(q, s, chunk=1024):
    out = torch.empty(q.shape[0], device=q.device)
    for b in range(0, q.shape[0], chunk):
        c = q[b:b + chunk]
        d = (s[None, :, 0] - c[:, None, 0]) ** 2
        d += (s[None, :, 1] - c[:, None, 1]) ** 2
        d += (s[None, :, 2] - c[:, None, 2]) ** 2
        out[b:b + chunk] = d.min(dim=1).values
    return out


def stats(times):
    return {"ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--brute-max", type=int, default=100_000, help="largest N at which the torch brute force is timed")
    ap.add_argument("--tree-max", type=int, default=1_000_000, help="largest N at which scipy's cKDTree is timed")
    args = ap.parse_args()
    dev = torch.device("cuda")
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    for N in args.sizes:
        for name, (q, s, r) in pairs(N, dev).items():
            base = {"pair": name, "N": N}
            if name != "disjoint":
                (d2, _), t = timed(lambda: cloud_nn.knn(q, s, 1, r), args.reps, 2)
                print(json.dumps({**base, "call": "knn k=1 capped", "radius": round(r, 5),
                                  "overlap": round(float(torch.isfinite(d2).float().mean()), 4), **stats(t)}), flush=True)
            (full, _), t = timed(lambda: cloud_nn.knn(q, s, 1), args.reps, 2)
            print(json.dumps({**base, "call": "knn k=1 uncapped", **stats(t)}), flush=True)
            if name != "disjoint":
                p, t = timed(lambda: cloud_nn.radius_pairs(q, s, r), args.reps, 2)
                print(json.dumps({**base, "call": "radius_pairs", "radius": round(r, 5), "pairs": p.shape[0], **stats(t)}), flush=True)
                del p
            if N <= args.brute_max:
                want, t = timed(lambda: brute_force(q, s), 1, 1)
                print(json.dumps({**base, "call": "torch brute force k=1", "ms": round(t[0], 1),
                                  "largest_relative_difference": float(((full[:, 0] - want).abs() / want.clamp_min(1e-12)).max())}),
                      flush=True)
            if cKDTree is not None and N <= args.tree_max and name != "disjoint":
                qh, sh = q.cpu().numpy(), s.cpu().numpy()
                t0 = time.perf_counter()
                cKDTree(sh).query(qh, k=1, distance_upper_bound=r, workers=min(16, os.cpu_count() or 1))
                print(json.dumps({**base, "call": "cKDTree build + capped query (host)", "ms": round(1e3 * (time.perf_counter() - t0), 1)}),
                      flush=True)


if __name__ == "__main__":
    main()
