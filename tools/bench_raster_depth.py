"""Cost of the depth and alpha maps at the headline shape (1 M Gaussians, SH 3, 640 x 480, bit-exact mode), 32 views per call
and one view per call.  One process, the variants alternate, every window is warmed up, device-synchronised and at least
`--seconds` long; `--rounds` windows per variant give the spread.

    python tools/bench_raster_depth.py [--views 32 1] [--seconds 1.0] [--rounds 3] [--trace-only]

Variants:
  colour_default   rasterize_views as callers get it (speculative single-entry forward)          -- "nothing got slower"
  colour_serial    gr_raster_preprocess + gr_raster_render_ex, serial: what the depth path adds to
  depth_forward    rasterize_views(render_depth=True), no grad
  fwd_bwd_colour   forward + backward, loss on the image
  fwd_bwd_all      forward + backward with render_depth=True, loss on image, depth and alpha
`--trace-only`: a few iterations of each variant and nothing else, for `rocprofv3 --kernel-trace --stats -- python ...`
(kernel times of the blend / render-backward instances with and without the maps).  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussreg_amd import _lib, synthetic  # noqa: E402
from gaussreg_amd.rasterizer import GaussianRasterizationSettings, ViewBatch, rasterize_views  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[32, 1])
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    W, H, P = 640, 480, args.gaussians
    g = synthetic.gaussians_c2(P, seed=0, sh_degree=3)
    t = {k: torch.from_numpy(g[k]).to(dev) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    L = _lib.lib()
    result = {"gaussians": P, "width": W, "height": H, "views": {}}
    for V in args.views:
        cams = synthetic.camera_ring(V, W, H, seed=0)
        vb = ViewBatch([GaussianRasterizationSettings(
            H, W, c["tanfovx"], c["tanfovy"], torch.zeros(3, device=dev), 1.0, torch.from_numpy(c["viewmatrix"]).to(dev),
            torch.from_numpy(c["projmatrix"]).to(dev), 3, torch.from_numpy(c["campos"]).to(dev), False, False) for c in cams])
        kw = dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
        leaves = {k: v.clone().requires_grad_(True) for k, v in t.items()}
        kwg = dict(shs=leaves["shs"], scales=leaves["scales"], rotations=leaves["rotations"])
        g_c = torch.randn((V, 3, H, W), device=dev)
        g_d = torch.randn((V, 1, H, W), device=dev)
        g_a = torch.randn((V, 1, H, W), device=dev)

        def colour_default():
            with torch.no_grad():
                rasterize_views(vb, t["means3D"], t["opacities"], **kw)

        def colour_serial():
            st = _lib.stream_ptr(dev)
            nr = (ctypes.c_int64 * (V + 1))()
            color = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
            radii = torch.empty((V, P), dtype=torch.int32, device=dev)
            gbytes = L.gr_raster_geom_bytes(P, V, W, H) + 256
            geom = torch.empty(gbytes, dtype=torch.uint8, device=dev)
            _lib.check(L.gr_raster_preprocess(P, 16, _lib.ptr(t["means3D"]), _lib.ptr(t["shs"]), None, _lib.ptr(t["opacities"]),
                                              _lib.ptr(t["scales"]), _lib.ptr(t["rotations"]), None, vb.array, V,
                                              _lib.ptr(radii), _lib.ptr(geom), gbytes, nr, st))
            total = sum(int(nr[v]) for v in range(V))
            binb = torch.empty(L.gr_raster_bin_bytes(total, W, H, V) + 256, dtype=torch.uint8, device=dev)
            _lib.check(L.gr_raster_render_ex(P, vb.array, V, nr, _lib.ptr(geom), gbytes, _lib.ptr(binb), binb.numel(),
                                             _lib.ptr(color), 0, st))

        def depth_forward():
            with torch.no_grad():
                rasterize_views(vb, t["means3D"], t["opacities"], render_depth=True, **kw)

        def fwd_bwd_colour():
            for v in leaves.values():
                v.grad = None
            img, _, _ = rasterize_views(vb, leaves["means3D"], leaves["opacities"], **kwg)
            (img * g_c).sum().backward()

        def fwd_bwd_all():
            for v in leaves.values():
                v.grad = None
            img, _, _, d, a = rasterize_views(vb, leaves["means3D"], leaves["opacities"], render_depth=True, **kwg)
            ((img * g_c).sum() + (d * g_d).sum() + (a * g_a).sum()).backward()

        variants = [colour_default, colour_serial, depth_forward, fwd_bwd_colour, fwd_bwd_all]
        if args.trace_only:
            for f in variants:
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            continue
        times = {f.__name__: [] for f in variants}
        for f in variants:  # warm-up: allocator, binning hints, the first-frame self-checks
            for _ in range(4):
                f()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for f in variants:
                n = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                while True:
                    f()
                    n += 1
                    if n % 4 == 0 or V > 1:
                        torch.cuda.synchronize()
                        if time.perf_counter() - t0 >= args.seconds:
                            break
                torch.cuda.synchronize()
                times[f.__name__].append((time.perf_counter() - t0) / n * 1e3)
        result["views"][str(V)] = {k: {"ms_per_call_median": round(sorted(v)[len(v) // 2], 4), "min": round(min(v), 4),
                                       "max": round(max(v), 4)} for k, v in times.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
