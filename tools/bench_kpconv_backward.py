"""KPConv forward + backward at the distinct layer shapes of KPConvFPN on the synthetic demo pyramid (the sizes of
tests/golden/demo_shapes.npz), and the backbone as a whole: HIP forward, HIP forward + backward (inside
gaussreg_amd.kpconv.differentiable()) and the reference's formulation in stock torch fp32 with autograd, on the same GPU in
the same process, alternating; peak allocated memory of each.  The backward is also timed with one gradient at a time
(bias / weights / features) for the share of each part.

    python tools/bench_kpconv_backward.py [--reps 7] [--skip-backbone]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests", "golden"))
import numpy as np
import torch

from gen_golden_ext import room_pair
from gaussreg_amd import kpconv, kpconv_blocks
from gaussreg_amd.data import precompute_data_stack_mode
from gaussreg_amd.kpconv import KPConv, differentiable

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--skip-backbone", action="store_true")
args = ap.parse_args()


def once(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(fns, reps):
    """Median per-call time of every function, the functions taking turns (a drift of the clocks hits all alike)."""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(once(fn))
    return [sorted(t)[len(t) // 2] for t in ts]


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def torch_kpconv(f, q, s, nb, kpts, weights, sigma, bias=None, inf=1e6):
    s2 = torch.cat([s, s.new_zeros((1, 3)) + inf], 0)
    nbp = s2[nb] - q[:, None]
    w = (1 - ((nbp[:, :, None] - kpts) ** 2).sum(3).sqrt() / sigma).clamp(min=0).transpose(1, 2)
    nf = torch.cat([f, f.new_zeros((1, f.shape[1]))], 0)[nb]
    o = (torch.matmul(w, nf).permute(1, 0, 2) @ weights).sum(0)
    o = o / (nf.sum(-1) > 0).sum(-1).clamp(min=1)[:, None]
    return o if bias is None else o + bias


def torch_maxpool(x, nb):
    return torch.cat((x, x.new_zeros((1, x.shape[1]))), 0)[nb].max(1)[0]


def torch_upsample(x, nb):
    return torch.cat((x, x.new_zeros((1, x.shape[1]))), 0)[nb[:, 0]]


ref, src = room_pair(30000, 0)
pts = torch.from_numpy(np.concatenate([ref, src])).cuda()
d = precompute_data_stack_mode(pts, torch.tensor([30000, 30000]), 5, 0.025, 0.0625, [89, 30, 43, 49, 49])
P, NB, SUB = d["points"], d["neighbors"], d["subsampling"]
g = torch.Generator(device="cuda").manual_seed(0)
kp = torch.randn(15, 3) * 0.03
# the distinct KPConv shapes of the 14 layers: (name, layers of that shape, query level, support level, neighbours, channels)
layers = [("1_1", 1, 0, 0, NB[0], 1, 64), ("1_2", 1, 0, 0, NB[0], 32, 32), ("2_1s", 1, 1, 0, SUB[0], 32, 32),
          ("2_2/3", 2, 1, 1, NB[1], 64, 64), ("3_1s", 1, 2, 1, SUB[1], 64, 64), ("3_2/3", 2, 2, 2, NB[2], 128, 128),
          ("4_1s", 1, 3, 2, SUB[2], 128, 128), ("4_2/3", 2, 3, 3, NB[3], 256, 256), ("5_1s", 1, 4, 3, SUB[3], 256, 256),
          ("5_2/3", 2, 4, 4, NB[4], 512, 512)]
L = kpconv._lib.lib()
tot = np.zeros(3)
for name, count, ql, sl, nb, cin, cout in layers:
    q, s = P[ql], P[sl]
    sigma = 0.05 * (2 ** sl)
    conv = KPConv(cin, cout, 15, 0.0625 * 2 ** sl, sigma, bias=True, kernel_points=kp * 2 ** sl).cuda()
    f = torch.relu(torch.randn(s.shape[0], cin, device="cuda", generator=g)).requires_grad_(cin > 1)  # layer 1_1: constant input
    go = torch.randn(q.shape[0], cout, device="cuda", generator=g)
    params = [conv.weights, conv.bias]

    def clear():
        f.grad = None
        for p in params:
            p.grad = None

    def hip_fwd():
        with torch.no_grad():
            conv(f, q, s, nb)

    def hip_fb():
        clear()
        with differentiable():
            conv(f, q, s, nb).backward(go)

    def torch_fb():
        clear()
        torch_kpconv(f, q, s, nb, conv.kernel_points, conv.weights, sigma, conv.bias).backward(go)

    def only(which):
        flags = [(p, p.requires_grad) for p in [f] + params]
        def run():
            for (p, _), on in zip(flags, which):
                p.requires_grad_(on and (p is not f or cin > 1))
            clear()
            with differentiable():
                conv(f, q, s, nb).backward(go)
            for p, was in flags:
                p.requires_grad_(was)
        return run

    t_fwd, t_fb, t_torch = alternate([hip_fwd, hip_fb, torch_fb], args.reps)
    parts = alternate([only((False, False, True)), only((False, True, False))] + ([only((True, False, False))] if cin > 1 else []),
                      args.reps)
    m_fwd, m_fb, m_torch = peak_mb(hip_fwd), peak_mb(hip_fb), peak_mb(torch_fb)
    tot += count * np.array([t_fwd, t_fb, t_torch])
    ws = L.gr_kpconv_backward_workspace_bytes(s.shape[0], q.shape[0], nb.shape[1], cin, cout, 15, 7 if cin > 1 else 6, 0) / 2 ** 20
    share = " ".join(f"{n} {max(t - t_fwd, 0):.3f}" for n, t in zip(("bias", "weights", "feats"), parts))
    print(f"encoder{name:6s} x{count} M={q.shape[0]:6d} N={s.shape[0]:6d} H={nb.shape[1]:3d} {cin:3d}->{cout:3d}: HIP fwd {t_fwd:.3f} ms, "
          f"fwd+bwd {t_fb:.3f} ms, torch fwd+bwd {t_torch:.3f} ms (x{t_torch / t_fb:.2f}) | peak MB: HIP fwd {m_fwd:.0f}, fwd+bwd {m_fb:.0f}, "
          f"torch {m_torch:.0f} | bwd workspace {ws:.0f} MB | backward alone by gradient (ms): {share}", flush=True)
print(f"all 14 KPConv layers: HIP fwd {tot[0]:.2f} ms, HIP fwd+bwd {tot[1]:.2f} ms, torch fwd+bwd {tot[2]:.2f} ms per pair", flush=True)

if not args.skip_backbone:
    torch.manual_seed(0)
    model = kpconv_blocks.KPConvFPN(1, 256, 64, 15, 0.0625, 0.05, 32).cuda()
    feats = torch.ones(P[0].shape[0], 1, device="cuda")
    hip_ops = (KPConv.forward, kpconv_blocks.maxpool, kpconv_blocks.nearest_upsample)
    torch_ops = (lambda self, f, q, s, nb: torch_kpconv(f, q, s, nb, self.kernel_points, self.weights, self.sigma, self.bias),
                 torch_maxpool, torch_upsample)

    def backbone(ops, train):
        def run():
            KPConv.forward, kpconv_blocks.maxpool, kpconv_blocks.nearest_upsample = ops
            try:
                model.zero_grad(set_to_none=True)
                if not train:
                    model(feats, d)
                    return
                with differentiable():
                    sum((o ** 2).sum() for o in model(feats, d)).backward()
            finally:
                KPConv.forward, kpconv_blocks.maxpool, kpconv_blocks.nearest_upsample = hip_ops
        return run

    fns = [backbone(hip_ops, False), backbone(hip_ops, True), backbone(torch_ops, True)]
    t = alternate(fns, max(3, args.reps // 2))
    m = [peak_mb(fn) for fn in fns]
    print(f"KPConvFPN (init_dim 64), one pair: HIP inference {t[0]:.2f} ms / {m[0]:.0f} MB, HIP fwd+bwd {t[1]:.2f} ms / {m[1]:.0f} MB, "
          f"torch fwd+bwd {t[2]:.2f} ms / {m[2]:.0f} MB (x{t[2] / t[1]:.2f} time, x{m[2] / m[1]:.2f} memory)")
