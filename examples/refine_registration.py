"""Render-and-compare refinement of a similarity transform between two Gaussian-splatting scenes.

Rendering scene B moved by x -> s R x + t from a camera gives the same image as rendering the unmoved B from a rigidly
moved camera, with the depth map scaled by s (gaussreg_amd.pose.similarity_camera).  So a coarse registration can be
refined on images with one camera gradient per view, without pushing the transform through every Gaussian:

    python examples/refine_registration.py --synthetic

`--synthetic` (needs no data): the scene is the synthetic C2 scene, the "true" transform is known, the coarse estimate is
the truth perturbed by a small rotation, translation and scale.  The fixed scene is rendered once from a ring of cameras
under the true transform (colour and depth: what scene A would show); Adam then runs on a 7-parameter correction
(rotation vector, translation, log scale) of the coarse estimate with an L1 colour + depth loss through
rasterize_views(..., render_depth=True).  Prints the transform error before and after.

`--loss dssim` replaces the L1 colour term by the 3DGS photometric loss, 0.8 L1 + 0.2 (1 - SSIM)
(gaussreg_amd.image_loss.photometric_loss), weighted per pixel by the alpha map of the target render: where the fixed
scene shows nothing, the colours are not compared.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from gaussreg_amd import pose, synthetic  # noqa: E402
from gaussreg_amd.image_loss import photometric_loss  # noqa: E402
from gaussreg_amd.rasterizer import GaussianRasterizationSettings, rasterize_views  # noqa: E402


def rotation_angle(Ra, Rb):
    c = (torch.trace(Ra.T @ Rb).item() - 1.0) / 2.0
    return math.acos(max(-1.0, min(1.0, c)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--synthetic", action="store_true", help="synthetic scene and a known transform (the only mode)")
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--loss", choices=("l1", "dssim"), default="l1",
                    help="colour term: plain L1, or the alpha-weighted L1 + D-SSIM photometric loss")
    args = ap.parse_args()
    if not args.synthetic:
        ap.error("only --synthetic is implemented: pass two registered scenes through the library calls shown here")
    dev = torch.device("cuda")
    W, H, V = args.width, args.height, args.views
    g = synthetic.gaussians_c2(args.points, 0)
    scene = {k: torch.from_numpy(g[k]).to(dev) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    cams = synthetic.camera_ring(V, W, H, seed=3)
    bg = torch.zeros(3, device=dev)
    views = [torch.from_numpy(c["viewmatrix"]).to(dev).contiguous() for c in cams]
    projs = [torch.from_numpy(c["projmatrix"]).to(dev).contiguous() for c in cams]

    def render(s, R, t):
        sets, factor = [], None
        for c, vm, pm in zip(cams, views, projs):
            vm2, pm2, cp2, factor = pose.similarity_camera(vm, s, R, t, projmatrix=pm)
            sets.append(GaussianRasterizationSettings(H, W, c["tanfovx"], c["tanfovy"], bg, 1.0, vm2, pm2, 3, cp2, False,
                                                      False))
        color, _, _, depth, alpha = rasterize_views(sets, scene["means3D"], scene["opacities"], shs=scene["shs"],
                                                scales=scene["scales"], rotations=scene["rotations"], render_depth=True)
        return color, depth * factor, alpha

    # the known transform and a coarse estimate of it
    s_true = torch.tensor(1.1, device=dev)
    R_true = pose.so3_exp(torch.tensor([0.05, -0.1, 0.08], device=dev))
    t_true = torch.tensor([0.1, -0.05, 0.08], device=dev)
    R0 = R_true @ pose.so3_exp(torch.tensor([0.02, 0.015, -0.02], device=dev))
    t0 = t_true + torch.tensor([0.03, -0.02, 0.02], device=dev)
    s0 = s_true * 1.02
    with torch.no_grad():
        target_c, target_d, target_alpha = render(s_true, R_true, t_true)
    target_alpha = target_alpha[:, 0].contiguous()

    w = torch.zeros(3, device=dev, requires_grad=True)
    dt = torch.zeros(3, device=dev, requires_grad=True)
    ls = torch.zeros((), device=dev, requires_grad=True)

    def current():
        return s0 * torch.exp(ls), R0 @ pose.so3_exp(w), t0 + dt

    def errors():
        with torch.no_grad():
            s, R, t = current()
            return rotation_angle(R_true, R), (t - t_true).norm().item(), abs(s.item() / s_true.item() - 1.0)

    e0 = errors()
    print(f"before: rotation error {e0[0]:.5f} rad, translation error {e0[1]:.5f}, scale error {e0[2]:.5f}")
    opt = torch.optim.Adam([w, dt, ls], lr=2e-3)
    for step in range(args.steps):
        opt.zero_grad()
        c, d, _ = render(*current())
        if args.loss == "dssim":
            colour = photometric_loss(c, target_c, 0.2, weight=target_alpha)
        else:
            colour = (c - target_c).abs().mean()
        loss = colour + 0.1 * (d - target_d).abs().mean()
        loss.backward()
        opt.step()
        if step % 25 == 0 or step == args.steps - 1:
            print(f"  step {step:4d}  loss {loss.item():.6f}")
    e1 = errors()
    print(f"after:  rotation error {e1[0]:.5f} rad, translation error {e1[1]:.5f}, scale error {e1[2]:.5f}")


if __name__ == "__main__":
    main()
