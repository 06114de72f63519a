"""Cost of the camera gradients in the rasterizer backward, with tools/bench_raster_backward.py's method: the C2 scene
(1 M Gaussians, SH degree 3, 640 x 480), `backward()` alone between device events (the forward runs outside the timed
region), after a warm-up, at V = 1 and V = 32 views per call.  The backward with camera tensors that require grad and the
backward without alternate in one process; every Gaussian input requires grad in both.  `--depth`: the same with the depth
and alpha maps in the loss.  Prints one JSON line (milliseconds per call: median and range over `--reps` rounds).

    python tools/bench_raster_camera_grad.py [--P 1000000] [--views 1,32] [--reps 5] [--depth]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from gaussreg_amd import synthetic  # noqa: E402
from gaussreg_amd.rasterizer import GaussianRasterizationSettings, ViewBatch, rasterize_views  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--views", default="1,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depth", action="store_true")
    args = ap.parse_args()
    W, H = 640, 480
    d = torch.device("cuda")
    g = synthetic.gaussians_c2(args.P, 0)
    t = {k: torch.from_numpy(v).to(d) for k, v in g.items()}
    res = {"scene": f"C2 P={args.P} SH3 {W}x{H}", "render_depth": args.depth, "backward_ms_per_call": {}}
    for V in [int(v) for v in args.views.split(",")]:
        cams = synthetic.camera_ring(V, W, H)

        def batch(grad):
            return ViewBatch([GaussianRasterizationSettings(
                H, W, c["tanfovx"], c["tanfovy"], torch.zeros(3, device=d), 1.0,
                torch.from_numpy(c["viewmatrix"]).to(d).requires_grad_(grad),
                torch.from_numpy(c["projmatrix"]).to(d).requires_grad_(grad), 3,
                torch.from_numpy(c["campos"]).to(d).requires_grad_(grad), False, False) for c in cams])
        vbs = {"with_camera": batch(True), "without_camera": batch(False)}
        leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()}
        gout = torch.randn((V, 3, H, W), device=d)
        gmap = torch.randn((V, 1, H, W), device=d)

        def backward_ms(vb):
            out = rasterize_views(vb, leaves["means3D"], leaves["opacities"], leaves["shs"], scales=leaves["scales"],
                                  rotations=leaves["rotations"], render_depth=args.depth)
            loss_terms = [out[0], out[3], out[4]] if args.depth else [out[0]]
            grads = [gout, gmap, gmap] if args.depth else [gout]
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.autograd.backward(loss_terms, grads)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)

        times = {k: [] for k in vbs}
        for rep in range(args.reps + 1):
            for k, vb in vbs.items():
                ms = backward_ms(vb)
                if rep > 0:  # (round 0 is the warm-up)
                    times[k].append(ms)
        res["backward_ms_per_call"][str(V)] = {
            k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        del leaves
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
