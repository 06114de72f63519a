"""The fused HIP GroupNorm of the training path against the stock composition it replaces, layer by layer and in the whole
backbone and training step.

    python tools/time_group_norm_backward.py [--points 30000] [--repeat 20] [--skip-step]

  * per layer shape of the demo pyramid (G = 32): forward + backward of kpconv_blocks.GroupNorm inside
    differentiable(fused_norm=True) against the same module inside differentiable() -- transpose, nn.GroupNorm, (add,)
    leaky_relu and their autograd -- once as norm + LeakyReLU and once as the residual tail (norm + shortcut + LeakyReLU).
    Device events around `repeat` calls after a warm-up.  Bytes the fused kernels move (fp32 matrix passes of N x C):
    norm + act: forward 3 (statistics read, apply read + write), backward 7 (pass 1 reads x, out, grad_out; pass 2 reads them
    again and writes grad_x); tail: forward 4, backward 7 (pass 1 also writes dy to grad_residual, pass 2 reads x and dy only).
  * KPConvFPN forward + backward at init_dim 64 on one pair: time and peak allocated memory, both ways;
  * one whole training step of model.GeoTransformer, both ways.
The default differentiable() path is bit for bit the path of the commit before the fused kernels, so "torch" below is that
commit measured on the same machine in the same process.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import gaussreg_amd  # noqa: E402
from gaussreg_amd import pair_pipeline  # noqa: E402
from gaussreg_amd.data import precompute_data_stack_mode  # noqa: E402
from gaussreg_amd.kpconv import differentiable  # noqa: E402
from gaussreg_amd.kpconv_blocks import GroupNorm  # noqa: E402
from gaussreg_amd.loss import OverallLoss  # noqa: E402
from gaussreg_amd.model import GeoTransformer, make_cfg  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, MI355X


def events_ms(fn, repeat):
    fn()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeat):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeat


def layer(n, c, groups, tail, repeat):
    dev = torch.device("cuda", 0)
    norm = GroupNorm(groups, c).to(dev)
    x = torch.randn(n, c, device=dev, requires_grad=True)
    res = torch.randn(n, c, device=dev, requires_grad=True) if tail else None
    go = torch.randn(n, c, device=dev)
    leaves = [x, norm.norm.weight, norm.norm.bias] + ([res] if tail else [])

    def run(fused):
        with differentiable(fused_norm=fused):
            out = norm(x, 0.1, residual=res)
        torch.autograd.grad(out, leaves, go)

    t_torch, t_hip = events_ms(lambda: run(False), repeat), events_ms(lambda: run(True), repeat)
    passes = 11 if tail else 10
    gbs = passes * 4.0 * n * c / (t_hip * 1e-3)
    print(f"  {n:6d} x {c:4d} {'tail' if tail else 'norm'}: torch {t_torch:7.3f} ms   fused {t_hip:7.3f} ms   x {t_torch / t_hip:5.2f}   "
          f"fused moves {passes * 4.0 * n * c / 2**20:7.1f} MiB: {gbs / 1e9:7.1f} GB/s = {100 * gbs / HBM_PEAK:4.1f} % of HBM peak"
          f"{'   SLOWER' if t_hip > t_torch else ''}")


def clock_ms(fn, repeat):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeat):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / repeat


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=30000)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true", help="leave the whole training step out")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = make_cfg()
    groups = cfg.backbone.group_norm
    ref, src, T = pair_pipeline.synthetic_room_pair(0, args.points, dev)
    d = precompute_data_stack_mode(torch.cat([ref, src]).contiguous(), torch.tensor([args.points, args.points]), 5, 0.025, 0.0625,
                                   pair_pipeline.NEIGHBOR_LIMITS)
    d["features"] = torch.ones((2 * args.points, 4), device=dev)
    d["transform"] = T
    rows = [int(p.shape[0]) for p in d["points"]]
    print(f"pyramid rows per level: {rows}; GroupNorm with {groups} groups; {args.repeat} calls per figure")
    print("forward + backward of one GroupNorm layer:")
    shapes = [(rows[0], 64), (rows[0], 128), (49505, 64), (28020, 128), (9034, 256), (1534, 512), (1534, 1024)]
    for n, c in shapes:
        for tail in (False, True):
            layer(n, c, groups, tail, args.repeat)

    torch.manual_seed(0)
    net = GeoTransformer(cfg).to(dev).train()

    def backbone(fused):
        net.zero_grad(set_to_none=True)
        with differentiable(fused_norm=fused):
            outs = net.backbone(d["features"], d)
        sum((o ** 2).sum() for o in outs).backward()

    print("KPConvFPN forward + backward, one pair:")
    for fused in (False, True):
        ms = clock_ms(lambda: backbone(fused), args.repeat)
        net.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        backbone(fused)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev)
        print(f"  {'fused norms' if fused else 'torch norms'}: {ms:7.2f} ms   peak allocated {peak / 2**20:7.0f} MiB "
              f"({(peak - base) / 2**20:.0f} MiB above what was held before)")

    if args.skip_step:
        return
    crit = OverallLoss(cfg)

    def step(fused):
        net.zero_grad(set_to_none=True)
        with gaussreg_amd.differentiable(fused_norm=fused):
            out = net(d)
            loss = crit(out, d)
        loss["loss"].backward()

    print("one training step (forward, losses, backward; no optimiser):")
    for fused in (False, True):
        print(f"  {'fused norms' if fused else 'torch norms'}: {clock_ms(lambda: step(fused), max(args.repeat // 4, 3)):7.2f} ms")


if __name__ == "__main__":
    main()
