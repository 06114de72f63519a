"""A few training steps of the coarse-registration network on one synthetic scene pair.

    python examples/train_registration.py --synthetic

`--synthetic` (needs no data): two independent samplings of one room, the source moved by a known rigid transform
(gaussreg_amd.pair_pipeline.synthetic_room_pair), collated into the network's five-level pyramid.  Each step runs
`GeoTransformer` in training mode inside `gaussreg_amd.differentiable()`: the ground-truth superpoint correspondences come
from one HIP call, the gradient flows through backbone, transformer, feature gather and Sinkhorn, the loss is
`OverallLoss` (circle loss on the superpoints + negative log-likelihood on the Sinkhorn output), the optimiser Adam with
the reference's learning rate.  Prints the losses and the `Evaluator` metrics of every step.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import gaussreg_amd  # noqa: E402
from gaussreg_amd.data import precompute_data_stack_mode  # noqa: E402
from gaussreg_amd.loss import Evaluator, OverallLoss  # noqa: E402
from gaussreg_amd.model import GeoTransformer, make_cfg  # noqa: E402
from gaussreg_amd.pair_pipeline import NEIGHBOR_LIMITS, synthetic_room_pair  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--synthetic", action="store_true", help="a synthetic room pair with a known transform (the only mode)")
    ap.add_argument("--points", type=int, default=6000, help="points per cloud")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fused-norm", action="store_true",
                    help="run the backbone's GroupNorm layers in HIP in training too (differentiable(fused_norm=True))")
    args = ap.parse_args()
    if not args.synthetic:
        ap.error("only --synthetic is implemented: feed your own pairs through the calls shown here")
    dev = torch.device("cuda")
    cfg = make_cfg()
    torch.manual_seed(args.seed)
    ref, src, transform = synthetic_room_pair(args.seed, args.points, dev)
    b = cfg.backbone
    data = precompute_data_stack_mode(torch.cat([ref, src]), torch.tensor([ref.shape[0], src.shape[0]]), b.num_stages,
                                      b.init_voxel_size, b.init_radius, NEIGHBOR_LIMITS)
    data["features"] = torch.ones((ref.shape[0] + src.shape[0], b.input_dim), device=dev)
    data["transform"] = transform
    net = GeoTransformer(cfg).to(dev).train()
    criterion, evaluator = OverallLoss(cfg), Evaluator(cfg)
    optimizer = torch.optim.Adam(net.parameters(), lr=args.lr)
    for step in range(args.steps):
        optimizer.zero_grad(set_to_none=True)
        with gaussreg_amd.differentiable(fused_norm=args.fused_norm):
            out = net(data)
            loss = criterion(out, data)
        loss["loss"].backward()
        optimizer.step()
        metrics = evaluator(out, data)
        loss = {k: v.detach() for k, v in loss.items()}
        print("step %d  loss %.4f  c_loss %.4f  f_loss %.4f  |  gt pairs %d  PIR %.3f  IR %.3f  RRE %.2f deg  RTE %.3f  RMSE %.3f  RR %.0f"
              % (step, float(loss["loss"]), float(loss["c_loss"]), float(loss["f_loss"]), out["gt_node_corr_indices"].shape[0],
                 float(evaluator.evaluate_coarse(out)), float(evaluator.evaluate_fine(out, data)), float(metrics["RRE"]),
                 float(metrics["RTE"]), float(metrics["RMSE"]), float(metrics["RR"])))


if __name__ == "__main__":
    main()
