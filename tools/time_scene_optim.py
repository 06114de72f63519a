"""Time of the scene optimiser's step (gaussreg_amd.scene_optim.GaussianAdam, one launch) beside torch.optim.Adam over the
same six parameter tensors of a 3DGS scene (SH degree 3: 59 floats per Gaussian), and of the densification statistics.

Per variant: device events around `--inner` back-to-back steps, 3 warm-up rounds, median of `--reps` rounds (>= 20).
  hip dense                      GaussianAdam.step()
  hip mask f, random / block     GaussianAdam.step(mask) with a fraction f of the Gaussians visible, drawn at random or as
                                 one contiguous block of indices (rows of 12 - 180 bytes: random rows still touch most
                                 128-byte lines of the short-row tensors, a block is the best case)
  hip radii f                    the same random visibility given as the rasterizer's (1, P) int32 radii
  torch default / foreach=False / fused=True   (fused only where this torch build has it)
  stats V                        DensifyStats.update at V views
Achieved bytes / s = 1 652 B (59 floats x (4 reads + 3 writes) x 4 B) per VISIBLE Gaussian over the median time; the HBM
fraction is that over 8 TB/s.  For the statistics: V x 16 B read per Gaussian + 12 B read and written where seen.  Every
timed step runs under an alarm: a step that does not finish in `--limit` seconds ends the process, so nothing starts
after a failure.

    python tools/time_scene_optim.py [--P 1000000] [--reps 20] [--inner 10]
"""
import argparse
import json
import os
import signal
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from gaussreg_amd.scene_optim import DensifyStats, GaussianAdam  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3}
FLOATS = 59
BYTES_PER_GAUSSIAN = FLOATS * 7 * 4


def timed(fn, reps, inner, limit, warmup=3):
    """Median / min / max milliseconds per call of fn()."""
    signal.alarm(limit)  # default disposition: the process ends if this step hangs
    out = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            out.append(a.elapsed_time(b) / inner)
    signal.alarm(0)
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


def scene(P, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    params = {n: torch.randn((P,) + s, generator=gen, device=dev).requires_grad_(True) for n, s in SHAPES.items()}
    for p in params.values():
        p.grad = 1e-3 * torch.randn(p.shape, generator=gen, device=dev)
    return params, [{"params": [params[n]], "lr": LRS[n], "name": n} for n in SHAPES]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--fractions", default="0.1,0.25,0.5")
    ap.add_argument("--stats-views", default="1,32")
    args = ap.parse_args()
    assert args.reps >= 20
    P, dev = args.P, torch.device("cuda")
    res = {"P": P, "floats_per_gaussian": FLOATS, "reps": args.reps, "inner": args.inner, "ms_per_step": {}, "bytes_per_s": {},
           "hbm_fraction": {}}

    def record(name, t, visible_fraction=None):
        res["ms_per_step"][name] = t
        if visible_fraction is not None:
            rate = BYTES_PER_GAUSSIAN * P * visible_fraction / (t["median"] * 1e-3)
            res["bytes_per_s"][name], res["hbm_fraction"][name] = rate, rate / HBM_PEAK

    _, groups = scene(P, dev, 0)
    opt = GaussianAdam(groups, eps=1e-15)
    record("hip_dense", timed(lambda: opt.step(), args.reps, args.inner, args.limit), 1.0)
    gen = torch.Generator(device=dev).manual_seed(1)
    for f in [float(x) for x in args.fractions.split(",")]:
        random_mask = torch.rand(P, generator=gen, device=dev) < f
        block_mask = torch.arange(P, device=dev) < int(f * P)
        radii = (random_mask.to(torch.int32) * 5)[None].contiguous()
        record(f"hip_mask_{f}_random", timed(lambda: opt.step(visibility=random_mask), args.reps, args.inner, args.limit),
               random_mask.float().mean().item())
        record(f"hip_radii_{f}_random", timed(lambda: opt.step(visibility=radii), args.reps, args.inner, args.limit),
               random_mask.float().mean().item())
        record(f"hip_mask_{f}_block", timed(lambda: opt.step(visibility=block_mask), args.reps, args.inner, args.limit),
               block_mask.float().mean().item())
    del opt, groups
    torch.cuda.empty_cache()
    for name, kw in (("torch_default", {}), ("torch_foreach_false", {"foreach": False}), ("torch_fused", {"fused": True})):
        _, groups = scene(P, dev, 0)
        try:
            topt = torch.optim.Adam(groups, eps=1e-15, **kw)
            topt.step()
        except (RuntimeError, TypeError, ValueError) as e:  # this torch build has no such variant
            res["ms_per_step"][name] = f"not available: {str(e).splitlines()[0][:120]}"
            continue
        record(name, timed(lambda: topt.step(), args.reps, args.inner, args.limit), 1.0)
        del topt, groups
        torch.cuda.empty_cache()
    for V in [int(v) for v in args.stats_views.split(",")]:
        stats = DensifyStats(P, dev)
        grad = 1e-3 * torch.randn((V, P, 3), generator=gen, device=dev)
        radii = torch.randint(-1, 30, (V, P), generator=gen, device=dev, dtype=torch.int32)
        t = timed(lambda: stats.update(grad, radii), args.reps, args.inner, args.limit)
        seen_any = (radii > 0).any(0).float().mean().item()
        rate = P * (16.0 * V + 24.0 * seen_any) / (t["median"] * 1e-3)
        res["ms_per_step"][f"stats_V{V}"] = t
        res["bytes_per_s"][f"stats_V{V}"], res["hbm_fraction"][f"stats_V{V}"] = rate, rate / HBM_PEAK
        del stats, grad, radii
    print(json.dumps(res))


if __name__ == "__main__":
    main()
