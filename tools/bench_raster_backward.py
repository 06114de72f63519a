"""Rasterizer backward on the C2 scene (1 M Gaussians, SH degree 3, 640 x 480): per view, the no-grad forward, the
keep-state (autograd) forward and the backward (`loss.backward()` alone: events around it, the forward outside), timed with
device events after a warm-up, at V = 1 and V = 32 views per call; the backward's kernels from the library's per-kernel event
timers with a byte model and its fraction of HBM peak.  (For a kernel trace, run it under
`rocprofv3 --kernel-trace --stats -- python tools/bench_raster_backward.py --iters 3`.)
Prints one JSON line.

    python tools/bench_raster_backward.py [--P 1000000] [--views 1,32] [--iters 5]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from gaussreg_amd import _lib, synthetic  # noqa: E402
from gaussreg_amd.rasterizer import GaussianRasterizationSettings, ViewBatch, rasterize_views  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s
KERNELS = ("raster_bwd_slots", "raster_bwd_render", "raster_bwd_preprocess")


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--views", default="1,32")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    W, H = 640, 480
    d = torch.device("cuda")
    g = synthetic.gaussians_c2(args.P, 0)
    t = {k: torch.from_numpy(v).to(d) for k, v in g.items()}
    L = _lib.lib()
    res = {"scene": f"C2 P={args.P} SH3 {W}x{H}", "per_view_ms": {}}
    for V in [int(v) for v in args.views.split(",")]:
        cams = synthetic.camera_ring(V, W, H)
        vb = ViewBatch([GaussianRasterizationSettings(H, W, c["tanfovx"], c["tanfovy"], torch.zeros(3, device=d), 1.0,
                                                      torch.from_numpy(c["viewmatrix"]).to(d),
                                                      torch.from_numpy(c["projmatrix"]).to(d), 3,
                                                      torch.from_numpy(c["campos"]).to(d), False, False) for c in cams])
        leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()}
        gout = torch.randn((V, 3, H, W), device=d)

        def fwd_nograd():
            with torch.no_grad():
                rasterize_views(vb, t["means3D"], t["opacities"], t["shs"], scales=t["scales"], rotations=t["rotations"])

        state = {}

        def fwd_keep():
            state["img"] = rasterize_views(vb, leaves["means3D"], leaves["opacities"], leaves["shs"], scales=leaves["scales"],
                                           rotations=leaves["rotations"])[0]

        def fwd_bwd():
            fwd_keep()
            state["img"].backward(gout)
            state.clear()

        def bwd_only(iters):  # the forward runs outside the timed region; one graph alive at a time
            tot = 0.0
            for it in range(iters + 1):
                state.clear()
                fwd_keep()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                state["img"].backward(gout)
                b.record()
                torch.cuda.synchronize()
                if it > 0:  # (the first one is the warm-up)
                    tot += a.elapsed_time(b)
            state.clear()
            return tot / iters

        f0 = timed(fwd_nograd, args.iters)
        f1 = timed(lambda: (state.clear(), fwd_keep()), args.iters)
        state.clear()
        fb = bwd_only(args.iters)
        _, _, nr = rasterize_views(vb, t["means3D"], t["opacities"], t["shs"], scales=t["scales"], rotations=t["rotations"])
        R = sum(nr)
        # per-kernel times of the backward (library event timers) over a few more iterations
        L.gr_timing_enable(1)
        L.gr_timing_reset()
        for _ in range(args.iters):
            fwd_bwd()
        torch.cuda.synchronize()
        kt = {}
        for n in KERNELS:
            tot, cnt = ctypes.c_double(0), ctypes.c_int64(0)
            L.gr_timing_read(n.encode(), ctypes.byref(tot), ctypes.byref(cnt))
            kt[n] = tot.value / max(cnt.value, 1)
        L.gr_timing_enable(0)
        P, px = args.P, V * W * H
        # byte model (compulsory traffic): slots = 36 B per (tile, Gaussian) instance
        bytes_model = {
            "raster_bwd_slots": V * P * (4 + 4) + 36 * R,                    # rect_raw in, slot base out, slot memset
            "raster_bwd_render": R * (4 + 48 + 4 + 8 + 36) + px * (4 + 4 + 12),  # list id, record, rect, base, slot out; pixel state
            "raster_bwd_preprocess": 36 * R + V * P * 12 + P * (12 + 4 + 192 + 12 + 16) * 2,  # slots, rect/base, inputs + grads
        }
        res["per_view_ms"][str(V)] = {
            "forward_nograd": f0 / V, "forward_keep": f1 / V, "backward": fb / V,
            "backward_over_forward": fb / f0, "instances_per_view": R / V,
            "kernels_ms_per_call": kt,
            "hbm_fraction": {n: (bytes_model[n] / (kt[n] * 1e-3)) / HBM_PEAK if kt[n] > 0 else None for n in KERNELS},
            "bytes_per_call": bytes_model,
        }
        del leaves, state
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
