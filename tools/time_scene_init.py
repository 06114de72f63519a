"""Time of mean_knn_dist2(points, k=3) (gaussreg_amd.scene_init: quantile grid, shell search) on three clouds, beside a
chunked stock-torch brute force where N allows it.

  a  uniform in the unit cube
  b  clustered: the means of synthetic.gaussians_c2
  c  cloud a with 1 % of the points moved out to 100 x the extent

Per cloud and N: device events around each call (the call includes its one host read-back), 2 warm-up rounds, median /
min / max of `--reps` rounds; points per second from the median.  The brute force (row chunks of a chunk x N distance
matrix and torch.topk) is timed once, up to `--brute-max` points.  The first cloud's result is compared with it when both ran.

    python tools/time_scene_init.py [--sizes 100000 1000000] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from gaussreg_amd import synthetic  # noqa: E402
from gaussreg_amd.scene_init import mean_knn_dist2  # noqa: E402


def clouds(N, dev):
    rng = np.random.default_rng(0)
    a = rng.random((N, 3)).astype(np.float32)
    b = synthetic.gaussians_c2(N, seed=0)["means3D"]
    c = a.copy()
    far = rng.choice(N, N // 100, replace=False)
    c[far] = (c[far] - np.float32(0.5)) * np.float32(100.0)
    return {name: torch.from_numpy(p).to(dev) for name, p in (("a uniform", a), ("b clustered", b), ("c outliers", c))}


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


def brute_force(p, chunk=1024):
    out = torch.empty(p.shape[0], device=p.device)
    for b in range(0, p.shape[0], chunk):
        q = p[b:b + chunk]
        d = (p[None, :, 0] - q[:, None, 0]) ** 2
        d += (p[None, :, 1] - q[:, None, 1]) ** 2
        d += (p[None, :, 2] - q[:, None, 2]) ** 2
        d[torch.arange(q.shape[0], device=p.device), torch.arange(b, b + q.shape[0], device=p.device)] = float("inf")
        out[b:b + chunk] = d.topk(3, dim=1, largest=False).values.sum(dim=1) / 3.0
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--brute-max", type=int, default=100_000, help="largest N at which the torch brute force is timed")
    args = ap.parse_args()
    dev = torch.device("cuda")
    for N in args.sizes:
        for name, p in clouds(N, dev).items():
            got, times = timed(lambda: mean_knn_dist2(p, 3), args.reps, 2)
            row = {"cloud": name, "N": N, "ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3),
                   "ms_max": round(max(times), 3), "points_per_s": round(N / (statistics.median(times) * 1e-3))}
            if N <= args.brute_max:
                want, brute = timed(lambda: brute_force(p), 1, 1)
                row["torch_brute_force_ms"] = round(brute[0], 1)
                row["largest_relative_difference"] = float(((got - want).abs() / want.clamp_min(1e-12)).max())
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
