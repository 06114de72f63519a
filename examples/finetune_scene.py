"""Fine-tune a Gaussian-splatting scene on images: the 3DGS training step on this library's kernels.

    python examples/finetune_scene.py --synthetic [--optimizer torch]
    python examples/finetune_scene.py --synthetic --from-points 5000

`--synthetic` (needs no data): the synthetic C2 scene is the truth and is rendered once from a ring of cameras.  The scene
is then perturbed (DC colours, logit opacities, log scales) and fitted back to those images, one view per step:

    rasterize_views (with a means2D tensor) -> photometric_loss -> backward
    GaussianAdam.step(visibility=radii)      # one launch; Gaussians the view did not see keep parameters and moments
    DensifyStats.update(means2D.grad, radii)  # what a densify / prune step would read

The raw parameters, their activations (in torch) and the learning rates are upstream 3DGS's: `xyz`, `f_dc`, `f_rest`,
logit `opacity`, log `scaling`, unnormalised `rotation`.  `--densify-every N` (off by default) runs
gaussreg_amd.scene_densify.densify_and_prune on those statistics every N steps until `--densify-until`, with upstream's
thresholds, and `--opacity-reset-every M` its reset_opacity; the loop then goes on with the returned tensors.  `--optimizer torch` runs the same loop on torch.optim.Adam
(dense: every Gaussian moves every step), for comparison.  Prints the loss and the PSNR over all views before and after.

`--from-points M` trains from a point cloud instead of a perturbed scene: M of the truth's means (a seeded subset) with
their DC colours as RGB play the SfM cloud, gaussreg_amd.scene_init.gaussians_from_points (upstream's create_from_pcd: the
exact 3-nearest-neighbour kernel gives the initial scales) builds the scene, and the loop runs with densification on and
upstream's exponential schedule (scene_init.expon_lr, times the scene's extent) on the `xyz` learning rate.
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from gaussreg_amd import synthetic  # noqa: E402
from gaussreg_amd.image_loss import photometric_loss  # noqa: E402
from gaussreg_amd.rasterizer import GaussianRasterizationSettings, ViewBatch, rasterize_views  # noqa: E402
from gaussreg_amd.scene_densify import densify_and_prune, reset_opacity  # noqa: E402
from gaussreg_amd.scene_init import SH_C0, expon_lr, gaussians_from_points  # noqa: E402
from gaussreg_amd.scene_optim import DensifyStats, GaussianAdam  # noqa: E402

# upstream 3DGS arguments/__init__.py (position_lr_init without the scene-extent factor, feature_lr, feature_lr / 20, ...)
LEARNING_RATES = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20.0, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3}
SH_DEGREE = 3
# upstream's position_lr_init / _final / _delay_mult / _max_steps, for --from-points
POSITION_LR = dict(lr_init=1.6e-4, lr_final=1.6e-6, lr_delay_mult=0.01, max_steps=30_000)


def raw_parameters(g, dev):
    """Upstream's raw parameter tensors from an activated scene (numpy dict of synthetic.gaussians_c2)."""
    t = {k: torch.from_numpy(v).to(dev) for k, v in g.items()}
    return {"xyz": t["means3D"].clone(), "f_dc": t["shs"][:, :1].contiguous(), "f_rest": t["shs"][:, 1:].contiguous(),
            "opacity": torch.logit(t["opacities"]), "scaling": torch.log(t["scales"]), "rotation": t["rotations"].clone()}


def render(raw, views, means2D=None):
    return rasterize_views(views, raw["xyz"], torch.sigmoid(raw["opacity"]), shs=torch.cat((raw["f_dc"], raw["f_rest"]), dim=1),
                           scales=torch.exp(raw["scaling"]), rotations=torch.nn.functional.normalize(raw["rotation"], dim=1),
                           means2D=means2D)[:2]


def finetune(points=20_000, views=4, steps=200, width=320, height=240, optimizer="hip", seed=0, log=None, densify_every=0,
             densify_until=None, opacity_reset_every=0, densify_grad_threshold=2e-4, min_opacity=5e-3, percent_dense=0.01,
             max_screen_size=None, from_points=0):
    """-> dict: loss / psnr before and after over all views, the raw parameters at the start and at the end, the per-step
    visibility (steps, P) bool, and the DensifyStats.  With densify_every > 0 (GaussianAdam only) the Gaussian count
    changes: instead of the per-step visibility the dict holds `densifications` (step, P_old, P_new, counts per event),
    `counts` (the Gaussian count after each event), `raw` (the live tensors by name) and `one_view` (the view batches).
    from_points = M > 0: start from gaussians_from_points on M of the truth's means instead of the perturbed truth, with
    densification on (every `densify_every` steps, 100 if that is 0) and expon_lr on the xyz group."""
    dev = torch.device("cuda")
    raw = raw_parameters(synthetic.gaussians_c2(points, seed, SH_DEGREE), dev)
    bg = torch.zeros(3, device=dev)
    cams = synthetic.camera_ring(views, width, height, seed=3)
    settings = [GaussianRasterizationSettings(height, width, c["tanfovx"], c["tanfovy"], bg, 1.0,
                                              torch.from_numpy(c["viewmatrix"]).to(dev), torch.from_numpy(c["projmatrix"]).to(dev),
                                              SH_DEGREE, torch.from_numpy(c["campos"]).to(dev), False, False) for c in cams]
    all_views = ViewBatch(settings)
    one_view = [ViewBatch([s]) for s in settings]
    with torch.no_grad():
        target = render(raw, all_views)[0]
        if from_points:
            if not 3 < from_points <= points:
                raise ValueError(f"from_points = {from_points} outside (3, points = {points}]")
            subset = torch.randperm(points, generator=torch.Generator().manual_seed(seed + 3))[:from_points].to(dev)
            cloud = raw["xyz"][subset].contiguous()
            colors = (raw["f_dc"][subset, 0] * SH_C0 + 0.5).clamp_(0.0, 1.0)
        else:
            gen = torch.Generator(device=dev).manual_seed(seed + 1)
            raw["f_dc"] += 0.15 * torch.randn(raw["f_dc"].shape, generator=gen, device=dev)
            raw["opacity"] += 0.5 * torch.randn(raw["opacity"].shape, generator=gen, device=dev)
            raw["scaling"] += 0.1 * torch.randn(raw["scaling"].shape, generator=gen, device=dev)
    if from_points:
        raw = gaussians_from_points(cloud, colors, SH_DEGREE)
        points = from_points
        densify_every = densify_every or 100
    for p in raw.values():
        p.requires_grad_(True)

    def evaluate():
        with torch.no_grad():
            image = render(raw, all_views)[0]
            mse = ((image - target) ** 2).mean().item()
            return photometric_loss(image, target, 0.2).item(), -10.0 * math.log10(max(mse, 1e-20))

    groups = [{"params": [raw[name]], "lr": lr, "name": name} for name, lr in LEARNING_RATES.items()]
    if optimizer == "hip":
        opt = GaussianAdam(groups, eps=1e-15)
    else:
        opt = torch.optim.Adam(groups, eps=1e-15)
    stats = DensifyStats(points, dev)
    start = {name: p.detach().clone() for name, p in raw.items()}
    before = evaluate()
    densify = densify_every > 0
    if densify and optimizer != "hip":
        raise ValueError("densification runs on GaussianAdam (--optimizer hip)")
    if densify:
        extent = (raw["xyz"].detach() - raw["xyz"].detach().mean(0)).norm(dim=1).max().item() * 1.1  # the scene's radius, for upstream's cameras_extent
        noise_gen = torch.Generator(device=dev).manual_seed(seed + 2)
    events, counts = [], []
    seen = None if densify else torch.zeros((steps, points), dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(steps):
        v = step % views
        if from_points:
            opt.param_groups[0]["lr"] = extent * expon_lr(step, **POSITION_LR)
        means2D = torch.zeros((1, points, 3), device=dev, requires_grad=True)
        image, radii = render(raw, one_view[v], means2D)
        loss = photometric_loss(image, target[v:v + 1], 0.2)
        loss.backward()
        if optimizer == "hip":
            opt.step(visibility=radii)
        else:
            opt.step()
        stats.update(means2D.grad, radii)
        opt.zero_grad(set_to_none=True)
        if not densify:
            seen[step] = radii[0] > 0
        if log and (step % 50 == 0 or step == steps - 1):
            log(f"  step {step:4d}  view {v}  loss {loss.item():.6f}  visible {int((radii[0] > 0).sum())} / {points}")
        done = step + 1
        if densify and done % densify_every == 0 and done < steps and (densify_until is None or done <= densify_until):
            r = densify_and_prune(opt, stats, densify_grad_threshold, min_opacity, extent, max_screen_size=max_screen_size,
                                  percent_dense=percent_dense, generator=noise_gen)
            for name in raw:  # the loop goes on with the tensors the optimiser now holds
                raw[name] = r.tensors[name]
            events.append({"step": done, "P_old": points, "P_new": r.P_new, "counts": r.counts})
            counts.append(r.P_new)
            if log:
                log(f"  step {done:4d}  densified: {points} -> {r.P_new} Gaussians (kept {r.counts[0]}, cloned {r.counts[1]}, "
                    f"split {r.counts[2]})")
            points = r.P_new
        if densify and opacity_reset_every > 0 and done % opacity_reset_every == 0 and done < steps:
            reset_opacity(opt)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    after = evaluate()
    out = {"before": before, "after": after, "start": start, "end": {name: p.detach() for name, p in raw.items()}, "seen": seen,
           "stats": stats, "optimizer": opt, "seconds": seconds}
    if densify:
        del out["seen"]
        out.update(densifications=events, counts=counts, raw=raw, one_view=one_view)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--synthetic", action="store_true", help="synthetic scene and its own renders as targets (the only mode)")
    ap.add_argument("--points", type=int, default=20_000)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--optimizer", choices=("hip", "torch"), default="hip",
                    help="GaussianAdam with the view's radii as visibility, or torch.optim.Adam over every Gaussian")
    ap.add_argument("--densify-every", type=int, default=0, help="densify and prune every N steps (0: never; hip optimizer)")
    ap.add_argument("--densify-until", type=int, default=None, help="last step at which to densify (default: no limit)")
    ap.add_argument("--opacity-reset-every", type=int, default=0, help="reset the opacities every M steps (0: never)")
    ap.add_argument("--densify-grad-threshold", type=float, default=2e-4, help="upstream's densify_grad_threshold")
    ap.add_argument("--min-opacity", type=float, default=5e-3, help="prune below this opacity")
    ap.add_argument("--percent-dense", type=float, default=0.01, help="clone / split boundary as a fraction of the extent")
    ap.add_argument("--max-screen-size", type=float, default=None, help="prune above this screen radius (and 0.1 x extent)")
    ap.add_argument("--from-points", type=int, default=0, metavar="M",
                    help="start from a cloud of M of the truth's points (scene_init.gaussians_from_points), densification on")
    args = ap.parse_args()
    if not args.synthetic:
        ap.error("only --synthetic is implemented: load a scene with gaussreg_amd.gs_io and follow finetune()")
    r = finetune(args.points, args.views, args.steps, args.width, args.height, args.optimizer, log=print,
                 densify_every=args.densify_every, densify_until=args.densify_until, opacity_reset_every=args.opacity_reset_every,
                 densify_grad_threshold=args.densify_grad_threshold, min_opacity=args.min_opacity,
                 percent_dense=args.percent_dense, max_screen_size=args.max_screen_size, from_points=args.from_points)
    print(f"before: loss {r['before'][0]:.6f}  PSNR {r['before'][1]:.2f} dB")
    print(f"after:  loss {r['after'][0]:.6f}  PSNR {r['after'][1]:.2f} dB   ({args.steps} steps, {args.optimizer} Adam, "
          f"{1e3 * r['seconds'] / max(args.steps, 1):.2f} ms per step)")
    st = r["stats"]
    print(f"densification statistics: {int((st.denom > 0).sum())} of {st.denom.shape[0]} Gaussians seen, "
          f"largest mean screen-space gradient {st.mean_grad().max().item():.3e}, largest radius {int(st.max_radii.max())}")


if __name__ == "__main__":
    main()
