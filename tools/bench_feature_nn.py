"""Time gr_feature_nn against what it replaces, on the GPU.

    python tools/bench_feature_nn.py [--shapes 8192x8192x256,25000x25000x256,200000x200000x32] [--rounds 7] [--json PATH]

Per shape (n x m x c, N(0,1) features from a seed), medians with min - max of device-event times around whole calls, after
warm-up rounds, the variants of a round taken in turn so that drift hits all of them alike:
  rows       feature_nn.nearest                       (nearest row of y for every row of x)
  both       feature_nn.mutual_nearest                (both directions, one kernel)
  composed   ops.pairwise_distance + torch.min over both dimensions, in row chunks of at most --chunk_bytes of matrix; the
             column minimum is folded across chunks with torch.minimum (indices are not tracked across chunks: the
             composition is given that for free)
  cdist      torch.cdist + min over both dimensions, chunked the same way
TFLOP/s counts 2 n m c operations per call.  A run without a GPU fails: there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def chunked(dist, x, y, rows):
    """min over both dimensions of dist(x chunk, y), chunk by chunk; -> (row min, row argmin, column min)."""
    rmin, rarg, cmin = [], [], None
    for lo in range(0, x.shape[0], rows):
        d = dist(x[lo:lo + rows], y)
        v, i = torch.min(d, dim=1)
        rmin.append(v)
        rarg.append(i)
        c = torch.min(d, dim=0).values
        cmin = c if cmin is None else torch.minimum(cmin, c)
        del d
    return torch.cat(rmin), torch.cat(rarg), cmin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192x8192x256,25000x25000x256,200000x200000x32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk_bytes", type=float, default=4e9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from gaussreg_amd import _lib, feature_nn, ops
    dev = _lib.require_gpu()
    results = []
    for shape in args.shapes.split(","):
        n, m, c = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(n + m + c)
        x = torch.randn(n, c, device=dev, generator=g)
        y = torch.randn(m, c, device=dev, generator=g)
        flop = 2.0 * n * m * c
        rows = max(1, min(n, int(args.chunk_bytes / (4.0 * m))))
        variants = {"rows": lambda: feature_nn.nearest(x, y), "both": lambda: feature_nn.mutual_nearest(x, y),
                    "composed": lambda: chunked(ops.pairwise_distance, x, y, rows),
                    "cdist": lambda: chunked(torch.cdist, x, y, rows)}
        times = {k: [] for k in variants}
        for r in range(args.warmup + args.rounds):
            for k, fn in variants.items():
                t = timed(fn)
                if r >= args.warmup:
                    times[k].append(t)
        # faster and different is not faster: the fused rows against the composition's
        d2, _ = feature_nn.nearest(x, y)
        assert torch.equal(d2, chunked(ops.pairwise_distance, x, y, rows)[0]), "fused and composed minima differ"
        row = {"n": n, "m": m, "c": c, "chunk_rows": rows, "rounds": args.rounds}
        for k, t in times.items():
            t = np.array(t)
            row[k] = {"ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                      "tflops": flop / float(np.median(t)) / 1e9}
        for k in ("composed", "cdist"):
            row[k + "_over_both"] = row[k]["ms"] / row["both"]["ms"]
        results.append(row)
        print(json.dumps(row), flush=True)
        del x, y
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
