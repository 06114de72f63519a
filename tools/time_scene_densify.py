"""Time of densify_and_prune (gaussreg_amd.scene_densify: one classification pass, one gather pass) beside upstream 3DGS's
procedure composed from stock torch ops (clone by `cat`, split by `cat`, two prunes by mask, over the six parameter tensors
and their twelve moments) on the same GPU in the same process.  SH degree 3: 59 floats per Gaussian, six groups with state.

The statistics are set so that about 10 % of the Gaussians are cloned, 10 % split and 5 % pruned.  Per variant: device
events around each call, 3 warm-up rounds, median / min / max of `--reps` rounds (>= 20).  Every round starts from the
same scene (the optimiser is rebuilt outside the timed region).
  plan         gr_gs_densify_plan without the read-back (three launches)
  apply        gr_gs_densify_apply (one launch) into preallocated tensors
  whole        densify_and_prune(...): allocation of the new tensors, plan, read-back of the counts, apply, state re-keyed
  torch        the cat / mask composition, given the same noise
  noise        torch.randn((P, 2, 3)), which `whole` and `torch` both take as an input
Byte model of the apply: per output row 708 B written; 708 B read for a kept original (parameters and both moments),
236 B for a new row (parameters only), plus 5 B of plan per row.  The HBM share is against the 8 TB/s peak; DESIGN.md 3.7
measured 6.3 TB/s for a float4 copy.  Every timed region runs under an alarm.

    python tools/time_scene_densify.py [--P 1000000] [--reps 20]
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

from gaussreg_amd import _lib  # noqa: E402
from gaussreg_amd.scene_densify import densify_and_prune  # noqa: E402
from gaussreg_amd.scene_optim import DensifyStats, GaussianAdam  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
FLOATS = 59
EXTENT, MAX_GRAD, MIN_OPACITY = 4.0, 2e-4, 5e-3


def scene(P, dev, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand(P, generator=gen, device=dev)
    params = {n: torch.randn((P,) + s, generator=gen, device=dev) for n, s in SHAPES.items()}
    # 10 % clone (small, large gradient), 10 % split (large, large gradient), 5 % transparent
    small = torch.rand(P, generator=gen, device=dev) < 0.5
    params["scaling"] = torch.log(torch.where(small, 0.02, 0.1)[:, None] * (0.5 + 0.5 * torch.rand((P, 3), generator=gen, device=dev)))
    params["opacity"] = torch.where(u < 0.05, -8.0, 1.0)[:, None].contiguous()
    selected = torch.rand(P, generator=gen, device=dev) < 0.2
    stats = (torch.where(selected, 1e-3, 1e-5).contiguous(), torch.ones(P, dtype=torch.int32, device=dev),
             torch.zeros(P, dtype=torch.int32, device=dev))
    moments = {n: (0.01 * torch.randn(p.shape, generator=gen, device=dev), 1e-4 * torch.rand(p.shape, generator=gen, device=dev))
               for n, p in params.items()}
    return params, moments, stats


def optimiser(params, moments, stats_tensors):
    tensors = {n: p.clone().requires_grad_(True) for n, p in params.items()}
    opt = GaussianAdam([{"params": [t], "lr": 1e-3, "name": n} for n, t in tensors.items()], eps=1e-15)
    for n, t in tensors.items():
        opt.state[t] = {"step": torch.tensor(5.0), "exp_avg": moments[n][0].clone(), "exp_avg_sq": moments[n][1].clone()}
    P = stats_tensors[0].shape[0]
    stats = DensifyStats(P, stats_tensors[0].device)
    stats.grad_accum, stats.denom, stats.max_radii = (t.clone() for t in stats_tensors)
    return tensors, opt, stats


def torch_composition(tensors, state, stats_tensors, noise):
    """Upstream's densify_and_prune from stock torch ops; tensors / state: name -> tensor / [exp_avg, exp_avg_sq]."""
    grad_accum, denom, radii = stats_tensors
    P = grad_accum.shape[0]
    grads = grad_accum / denom
    grads[grads.isnan()] = 0.0

    def postfix(new):
        for n in tensors:
            tensors[n] = torch.cat((tensors[n], new[n]), dim=0)
            state[n] = [torch.cat((t, torch.zeros_like(new[n])), dim=0) for t in state[n]]

    def prune(mask):
        keep = ~mask
        for n in tensors:
            tensors[n] = tensors[n][keep]
            state[n] = [t[keep] for t in state[n]]

    def world():
        return torch.exp(tensors["scaling"]).max(dim=1).values

    sel = (grads >= MAX_GRAD) & (world() <= 0.01 * EXTENT)
    postfix({n: t[sel] for n, t in tensors.items()})
    padded = torch.zeros(tensors["xyz"].shape[0], device=grads.device)
    padded[:P] = grads
    sel = (padded >= MAX_GRAD) & (world() > 0.01 * EXTENT)
    src = torch.nonzero(sel)[:, 0]
    new = {n: t[sel].repeat((2,) + (1,) * (t.dim() - 1)) for n, t in tensors.items()}
    stds = torch.exp(new["scaling"])
    samples = stds * torch.cat((noise[src, 0], noise[src, 1]))
    q = torch.nn.functional.normalize(new["rotation"], dim=1)
    r, x, y, z = q.unbind(1)
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)), dim=1).view(-1, 3, 3)
    new["xyz"] = torch.bmm(R, samples.unsqueeze(-1)).squeeze(-1) + new["xyz"]
    new["scaling"] = torch.log(stds / 1.6)
    postfix(new)
    prune(torch.cat((sel, torch.zeros(2 * src.shape[0], dtype=torch.bool, device=sel.device))))
    prune(torch.sigmoid(tensors["opacity"]).squeeze(-1) < MIN_OPACITY)
    n_new = tensors["xyz"].shape[0]
    return n_new, (torch.zeros(n_new, device=grads.device), torch.zeros(n_new, dtype=torch.int32, device=grads.device),
                   torch.zeros(n_new, dtype=torch.int32, device=grads.device))


def timed(setup, fn, reps, limit, warmup=3):
    signal.alarm(limit)  # default disposition: the process ends if a round hangs
    out = []
    for r in range(warmup + reps):
        args = setup()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(*args)
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            out.append(a.elapsed_time(b))
        del args
    signal.alarm(0)
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=120)
    args = ap.parse_args()
    assert args.reps >= 20
    P, dev = args.P, torch.device("cuda")
    params, moments, stats_tensors = scene(P, dev)
    noise = torch.randn((P, 2, 3), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    res = {"P": P, "floats_per_gaussian": FLOATS, "reps": args.reps, "ms": {}}

    def whole_setup():
        return optimiser(params, moments, stats_tensors)[1:]

    first = densify_and_prune(*whole_setup(), MAX_GRAD, MIN_OPACITY, EXTENT, noise=noise)
    counts, P_new = first.counts, first.P_new
    res["counts"], res["P_new"] = list(counts), P_new
    res["ms"]["whole"] = timed(whole_setup, lambda opt, stats: densify_and_prune(opt, stats, MAX_GRAD, MIN_OPACITY, EXTENT, noise=noise),
                               args.reps, args.limit)

    # the two halves through the C ABI, on preallocated buffers
    L = _lib.lib()
    stream = _lib.stream_ptr(dev)
    source = torch.empty(2 * P, dtype=torch.int32, device=dev)
    kind = torch.empty(2 * P, dtype=torch.uint8, device=dev)
    counts_dev = torch.empty(4, dtype=torch.int32, device=dev)
    nbytes = L.gr_gs_densify_plan_workspace_bytes(P)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def plan():
        _lib.check(L.gr_gs_densify_plan(_lib.ptr(params["scaling"]), _lib.ptr(params["opacity"]), _lib.ptr(stats_tensors[0]),
                                        _lib.ptr(stats_tensors[1]), _lib.ptr(stats_tensors[2]), P, MAX_GRAD, MIN_OPACITY, EXTENT,
                                        0.01, 0, 0.0, _lib.ptr(source), _lib.ptr(kind), _lib.ptr(counts_dev), None, _lib.ptr(ws),
                                        nbytes, stream))

    res["ms"]["plan"] = timed(lambda: (), plan, args.reps, args.limit)
    assert counts_dev.tolist() == list(counts)
    new = {n: [torch.empty((P_new,) + s, device=dev) for _ in range(3)] for n, s in SHAPES.items()}
    roles = {"xyz": _lib.GS_DENSIFY_XYZ, "scaling": _lib.GS_DENSIFY_SCALING}
    table = (_lib.GsDensifyGroup * len(SHAPES))(*[
        _lib.GsDensifyGroup(_lib.ptr(params[n]), _lib.ptr(new[n][0]), _lib.ptr(moments[n][0]), _lib.ptr(new[n][1]),
                            _lib.ptr(moments[n][1]), _lib.ptr(new[n][2]), params[n].numel() // P, roles.get(n, 0)) for n in SHAPES])

    def apply():
        _lib.check(L.gr_gs_densify_apply(table, len(SHAPES), P, P_new, _lib.ptr(source), _lib.ptr(kind), _lib.ptr(params["scaling"]),
                                         _lib.ptr(params["rotation"]), _lib.ptr(noise), stream))

    res["ms"]["apply"] = timed(lambda: (), apply, args.reps, args.limit)
    for n in SHAPES:
        assert torch.equal(new[n][0].view(torch.int32), first.tensors[n].detach().view(torch.int32)), n
    kept = counts[0]
    apply_bytes = P_new * (FLOATS * 12 + 5) + kept * FLOATS * 12 + (P_new - kept) * FLOATS * 4
    res["apply_bytes"] = apply_bytes
    res["apply_bytes_per_s"] = apply_bytes / (res["ms"]["apply"]["median"] * 1e-3)
    res["apply_hbm_fraction"] = res["apply_bytes_per_s"] / HBM_PEAK
    del new, table

    def torch_setup():
        return ({n: p.clone() for n, p in params.items()}, {n: [m.clone(), v.clone()] for n, (m, v) in moments.items()},
                tuple(t.clone() for t in stats_tensors), noise)

    n_torch, _ = torch_composition(*torch_setup())
    assert n_torch == P_new, (n_torch, P_new)
    res["ms"]["torch"] = timed(torch_setup, torch_composition, args.reps, args.limit)
    res["ms"]["noise"] = timed(lambda: (), lambda: torch.randn((P, 2, 3), device=dev), args.reps, args.limit)
    res["torch_over_whole"] = res["ms"]["torch"]["median"] / res["ms"]["whole"]["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
