"""gr_node_correspondences at the demo shape, against a stock-torch transcription of the reference function, and one whole
training step split by section.

    python tools/time_node_correspondences.py [--points 30000] [--repeat 20]

On the coarse level of the 2 x 30 000-point demo pyramid (about 767 x 767 superpoints, K = 128) it prints
  * the candidate pairs that survive the reference's enclosing-sphere test, and the emitted pairs;
  * the HIP call: time per call (device events around `repeat` calls after a warm-up, the read-back of the count
    included), its workspace and output bytes;
  * the torch transcription (matching.py:231-315 op for op, the expanded distance form and all) on the same GPU: time and
    peak allocated memory above the inputs; and whether the two agree (they may differ on point pairs within fp32 error of
    the radius: the transcription's distance form is the less exact one);
  * one training step of model.GeoTransformer: forward split into targets / backbone / the rest, the loss split into the
    circle loss and the fine loss, and the backward -- host clock around a device synchronise per section.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import gaussreg_amd  # noqa: E402
from gaussreg_amd import _lib, pair_pipeline  # noqa: E402
from gaussreg_amd.data import precompute_data_stack_mode  # noqa: E402
from gaussreg_amd.loss import OverallLoss  # noqa: E402
from gaussreg_amd.matching import get_node_correspondences  # noqa: E402
from gaussreg_amd.model import GeoTransformer, make_cfg  # noqa: E402
from gaussreg_amd.ops import index_select, point_to_node_partition  # noqa: E402


def torch_node_correspondences(ref_nodes, src_nodes, ref_knn_points, src_knn_points, transform, pos_radius, ref_masks, src_masks,
                               ref_knn_masks, src_knn_masks, stats=None):
    """The reference function in stock torch, op for op."""
    def apply(p):
        return p @ transform[:3, :3].T + transform[:3, 3]

    def pdist(x, y):
        return (x.pow(2).sum(-1).unsqueeze(-1) - 2 * x @ y.transpose(-1, -2) + y.pow(2).sum(-1).unsqueeze(-2)).clamp(min=0.0)
    src_nodes, src_knn_points = apply(src_nodes), apply(src_knn_points)
    node_mask_mat = ref_masks.unsqueeze(1) & src_masks.unsqueeze(0)
    ref_d = torch.linalg.norm(ref_knn_points - ref_nodes.unsqueeze(1), dim=-1).masked_fill_(~ref_knn_masks, 0.0).max(1)[0]
    src_d = torch.linalg.norm(src_knn_points - src_nodes.unsqueeze(1), dim=-1).masked_fill_(~src_knn_masks, 0.0).max(1)[0]
    dist_mat = torch.sqrt(pdist(ref_nodes, src_nodes))
    intersect = torch.gt(ref_d.unsqueeze(1) + src_d.unsqueeze(0) + pos_radius - dist_mat, 0) & node_mask_mat
    sel_ref, sel_src = torch.nonzero(intersect, as_tuple=True)
    if stats is not None:
        stats["candidates"] = int(sel_ref.shape[0])
    rkm, skm = ref_knn_masks[sel_ref], src_knn_masks[sel_src]
    rkp, skp = ref_knn_points[sel_ref], src_knn_points[sel_src]
    point_mask = rkm.unsqueeze(2) & skm.unsqueeze(1)
    d = pdist(rkp, skp).masked_fill_(~point_mask, 1e12)
    hit = torch.lt(d, pos_radius ** 2)
    ref_cnt = torch.count_nonzero(hit.sum(-1), dim=-1).float()
    src_cnt = torch.count_nonzero(hit.sum(-2), dim=-1).float()
    overlaps = (ref_cnt / rkm.sum(-1).float() + src_cnt / skm.sum(-1).float()) / 2
    keep = torch.gt(overlaps, 0)
    return torch.stack([sel_ref[keep], sel_src[keep]], dim=1), overlaps[keep]


def events_ms(fn, repeat):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeat):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeat


def clock_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=30000)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--torch-repeat", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = make_cfg()
    ref, src, T = pair_pipeline.synthetic_room_pair(0, args.points, dev)
    d = precompute_data_stack_mode(torch.cat([ref, src]).contiguous(), torch.tensor([args.points, args.points]), 5, 0.025, 0.0625,
                                   pair_pipeline.NEIGHBOR_LIMITS)
    d["features"] = torch.ones((2 * args.points, 4), device=dev)
    d["transform"] = T
    K = cfg.model.num_points_in_patch
    nc, nf = int(d["lengths"][-1][0]), int(d["lengths"][1][0])
    sides = []
    for pc, pf in ((d["points"][-1][:nc], d["points"][1][:nf]), (d["points"][-1][nc:], d["points"][1][nf:])):
        _, nm, idx, km = point_to_node_partition(pf, pc, K)
        sides.append((pc.contiguous(), index_select(torch.cat([pf, torch.zeros_like(pf[:1])], 0), idx, dim=0), nm, km))
    (rn, rk, rnm, rkm), (sn, sk, snm, skm) = sides
    M, N = rn.shape[0], sn.shape[0]
    r = cfg.model.ground_truth_matching_radius
    print(f"coarse level of the 2 x {args.points} pair: {M} x {N} superpoints, K = {K}, radius {r}")

    hip = lambda: get_node_correspondences(rn, sn, rk, sk, T, r, rnm, snm, rkm, skm)   # noqa: E731
    hi, ho = hip()
    ms = events_ms(hip, args.repeat)
    ws = _lib.lib().gr_node_correspondences_workspace_bytes(M, N, K)
    print(f"HIP   : {ms:8.3f} ms per call   workspace {ws / 2**20:.2f} MiB   output buffers {M * N * 20 / 2**20:.2f} MiB   "
          f"emitted pairs {hi.shape[0]}")

    stats = {}
    tr = lambda: torch_node_correspondences(rn, sn, rk, sk, T, r, rnm, snm, rkm, skm, stats)   # noqa: E731
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    ti, to = tr()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    tms = events_ms(tr, args.torch_repeat)
    print(f"torch : {tms:8.3f} ms per call   peak memory above the inputs {peak / 2**20:.1f} MiB   candidate pairs after the "
          f"sphere test {stats['candidates']} of {M * N} ({100.0 * stats['candidates'] / (M * N):.2f} %)   emitted pairs {ti.shape[0]}")
    hs, ts = set(map(tuple, hi.tolist())), set(map(tuple, ti.tolist()))
    both = sorted(hs & ts)
    dh = {p: float(v) for p, v in zip(map(tuple, hi.tolist()), ho.tolist())}
    dt = {p: float(v) for p, v in zip(map(tuple, ti.tolist()), to.tolist())}
    differ = sum(dh[p] != dt[p] for p in both)
    print(f"agreement: {len(both)} pairs in both lists, {len(hs - ts)} only HIP, {len(ts - hs)} only torch, {differ} common pairs "
          f"with another overlap (point pairs within the expanded form's fp32 error of the radius)")
    print(f"speed-up HIP over torch: {tms / ms:.1f} x")

    # ---- one training step, by section
    torch.manual_seed(0)
    net = GeoTransformer(cfg).to(dev).train()
    crit = OverallLoss(cfg)
    for rep in range(2):    # the first pass warms every shape up
        with gaussreg_amd.differentiable():
            out, t_fwd = clock_ms(lambda: net(d))
            c_loss, t_c = clock_ms(lambda: crit.coarse_loss(out))
            f_loss, t_f = clock_ms(lambda: crit.fine_loss(out, d))
            loss = c_loss + f_loss
        _, t_bwd = clock_ms(lambda: loss.backward())
    with gaussreg_amd.differentiable():
        feats = out["ref_feats_c"].detach().requires_grad_(True)
        o2 = dict(out, ref_feats_c=feats, src_feats_c=out["src_feats_c"].detach())
        cl, _ = clock_ms(lambda: crit.coarse_loss(o2))
    _, t_cb = clock_ms(lambda: cl.backward())
    _, t_targets = clock_ms(hip)
    with gaussreg_amd.differentiable():
        _, t_backbone = clock_ms(lambda: net.backbone(d["features"], d))
    total = t_fwd + t_c + t_f + t_bwd
    print(f"training step ({M} x {N} superpoints, {out['matching_scores'].shape[0]} target patches): {total:.1f} ms")
    print(f"  forward        {t_fwd:8.2f} ms   (targets {t_targets:.2f} ms, backbone {t_backbone:.2f} ms)")
    print(f"  circle loss    {t_c:8.2f} ms   (its own backward {t_cb:.2f} ms; forward + backward {100 * (t_c + t_cb) / total:.1f} % of the step)")
    print(f"  fine loss      {t_f:8.2f} ms")
    print(f"  backward       {t_bwd:8.2f} ms")


if __name__ == "__main__":
    main()
