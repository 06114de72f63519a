"""Time of the fused L1 + D-SSIM loss (gaussreg_amd.image_loss) beside the stock-torch fp32 composition of the same
formula (five grouped conv2d + elementwise passes + autograd) and beside the rasterizer it judges, in one process.

Per shape (V x 3 x 480 x 640 at V = 1 and V = 32 by default): forward without a keep buffer (the image does not require
grad), forward with the keep buffer, forward with keep + backward; device events around `--inner` back-to-back calls,
3 warm-up rounds, median of `--reps` rounds (>= 20).  The rasterizer figures are the C2 scene's forward and forward +
backward at the same view count, from the same run.  The achieved HBM fraction is algorithmic bytes / time / 8 TB/s:
forward without keep reads 2 images (+ weight); forward with keep also writes 3 maps; the backward (forward + backward
minus forward with keep) reads 5 and writes 1.  Every timed step runs under an alarm: a step that does not finish in
`--limit` seconds ends the process.

The stock-torch composition is `conv_loss` of tests/image_loss_f64.py, the same function the GPU tests use as their fp32
yardstick: this tool puts tests/ on sys.path to import it and has to follow if that file moves.

    python tools/time_image_loss.py [--views 1,32] [--reps 20] [--P 1000000] [--weight]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import image_loss_f64 as R  # noqa: E402  (conv_loss: the stock-torch composition)
from gaussreg_amd import image_loss, synthetic  # noqa: E402
from gaussreg_amd.rasterizer import GaussianRasterizationSettings, ViewBatch, rasterize_views  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="1,32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--weight", action="store_true", help="pass a (V, H, W) weight map")
    ap.add_argument("--no-raster", action="store_true")
    args = ap.parse_args()
    assert args.reps >= 20
    C, H, W = 3, 480, 640
    d = torch.device("cuda")
    res = {"shape": f"Vx{C}x{H}x{W}", "weight": args.weight, "reps": args.reps, "inner": args.inner, "ms_per_call": {},
           "hbm_fraction": {}}
    scene = None
    if not args.no_raster:
        g = synthetic.gaussians_c2(args.P, 0)
        scene = {k: torch.from_numpy(v).to(d) for k, v in g.items()}
    for V in [int(v) for v in args.views.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(V)
        x = torch.rand((V, C, H, W), generator=gen, device=d)
        y = torch.rand((V, C, H, W), generator=gen, device=d)
        w = torch.rand((V, H, W), generator=gen, device=d) if args.weight else None
        xg = x.clone().requires_grad_(True)
        row = {}

        def both(loss_fn):
            xg.grad = None
            loss_fn(xg).backward()

        row["hip_forward_no_keep"] = timed(lambda: image_loss.photometric_loss(x, y, 0.2, weight=w), args.reps, args.inner, args.limit)
        row["hip_forward_keep"] = timed(lambda: image_loss.photometric_loss(xg, y, 0.2, weight=w), args.reps, args.inner,
                                        args.limit)
        row["hip_forward_backward"] = timed(lambda: both(lambda t: image_loss.photometric_loss(t, y, 0.2, weight=w)), args.reps,
                                            args.inner, args.limit)
        row["torch_forward"] = timed(lambda: R.conv_loss(x, y, w, 0.2)[0].mean(), args.reps, args.inner, args.limit)
        row["torch_forward_backward"] = timed(lambda: both(lambda t: R.conv_loss(t, y, w, 0.2)[0].mean()), args.reps, args.inner,
                                              args.limit)
        n = 4 * V * C * H * W
        read_bytes = 2 * n + (4 * V * H * W if args.weight else 0)
        bwd_ms = row["hip_forward_backward"]["median"] - row["hip_forward_keep"]["median"]
        res["hbm_fraction"][str(V)] = {
            "forward_no_keep": read_bytes / (row["hip_forward_no_keep"]["median"] * 1e-3) / HBM_PEAK,
            "forward_keep": (read_bytes + 3 * n) / (row["hip_forward_keep"]["median"] * 1e-3) / HBM_PEAK,
            "backward": 6 * n / (bwd_ms * 1e-3) / HBM_PEAK, "backward_ms": bwd_ms}
        if scene is not None:
            cams = synthetic.camera_ring(V, W, H)
            vb = ViewBatch([GaussianRasterizationSettings(
                H, W, c["tanfovx"], c["tanfovy"], torch.zeros(3, device=d), 1.0, torch.from_numpy(c["viewmatrix"]).to(d),
                torch.from_numpy(c["projmatrix"]).to(d), 3, torch.from_numpy(c["campos"]).to(d), False, False) for c in cams])
            leaves = {k: v.clone().requires_grad_(True) for k, v in scene.items()}
            gout = torch.randn((V, C, H, W), device=d)

            def render(src):
                return rasterize_views(vb, src["means3D"], src["opacities"], src["shs"], scales=src["scales"],
                                       rotations=src["rotations"])[0]

            def render_no_grad():
                with torch.no_grad():
                    render(scene)

            row["raster_forward"] = timed(render_no_grad, args.reps, 1, args.limit)
            row["raster_forward_backward"] = timed(lambda: render(leaves).backward(gout), args.reps, 1, args.limit)
            del leaves
        res["ms_per_call"][str(V)] = row
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
