"""RPE attention forward and forward + backward at the demo size (N = M = 767, C = 256, H = 4), and the whole
GeometricTransformer (hidden 256, 4 heads, self / cross x 3, angle_k 3, 'max'): the HIP path inside
gaussreg_amd.kpconv.differentiable() against the reference's composition in stock torch fp32 with autograd, on the same
GPU in the same process, alternating; peak allocated memory of each.  The row pass of the backward is also reported as a
fraction of HBM peak against the bytes it must move (one embedding read, plus one write when grad_embed is wanted), from
the library's per-kernel event timing.  Per cloud, the structure embedding's backward alone: the HIP kernel against the
torch recomputation (`grad_impl`), its kernel time and share of the fp32 MFMA peak, peak memory, and how far the two paths'
gradients are apart.

    python tools/bench_rpe_attention_backward.py [--reps 7] [--n 767] [--skip-stack]
"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch
import torch.nn.functional as F

from gaussreg_amd import _lib
from gaussreg_amd.kpconv import differentiable
from gaussreg_amd.rpe_attention import RPEMultiHeadAttention
from gaussreg_amd.transformer import GeometricTransformer

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--n", type=int, default=767)
ap.add_argument("--skip-stack", action="store_true")
args = ap.parse_args()
HBM_PEAK = 8.0e12
N, C, H = args.n, 256, 4


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


def kernel_ms(fn, name):
    """Average duration of the kernel `name` over one call of fn (gr_timing_*: HIP events around the launch)."""
    L = _lib.lib()
    fn()
    L.gr_timing_reset()
    L.gr_timing_enable(1)
    fn()
    torch.cuda.synchronize()
    ms, calls = ctypes.c_double(0), ctypes.c_int64(0)
    L.gr_timing_read(name.encode(), ctypes.byref(ms), ctypes.byref(calls))
    L.gr_timing_enable(0)
    return ms.value / max(calls.value, 1)


def torch_rpe_attention(att, q, k, v, emb):
    """rpe_transformer.py:51-72 as written: the embedding is projected, then contracted with q."""
    ch = C // H
    qp = att.proj_q(q).view(-1, H, ch).transpose(0, 1)
    kp = att.proj_k(k).view(-1, H, ch).transpose(0, 1)
    vp = att.proj_v(v).view(-1, H, ch).transpose(0, 1)
    pp = att.proj_p(emb).view(emb.shape[0], emb.shape[1], H, ch).permute(2, 0, 1, 3)
    s = (torch.einsum("hnc,hmc->hnm", qp, kp) + torch.einsum("hnc,hnmc->hnm", qp, pp)) / ch ** 0.5
    p = torch.softmax(s, dim=-1)
    return torch.matmul(p, vp).transpose(0, 1).reshape(-1, C), p


torch.manual_seed(0)
att = RPEMultiHeadAttention(C, H).cuda()
x = torch.randn(1, N, C, device="cuda")
go = torch.randn(1, N, C, device="cuda")
emb = torch.randn(1, N, N, C, device="cuda") * 0.7


def hip_forward():
    with torch.no_grad():
        att(x, x, x, emb)


def hip_fwd_bwd(emb_grad):
    def run():
        att.zero_grad(set_to_none=True)
        xx, ee = x.clone().requires_grad_(True), emb.detach().requires_grad_(emb_grad)
        with differentiable():
            hid, _ = att(xx, xx, xx, ee)
        hid.backward(go)
    return run


def torch_forward():
    with torch.no_grad():
        torch_rpe_attention(att, x[0], x[0], x[0], emb[0])


def torch_fwd_bwd(emb_grad):
    def run():
        att.zero_grad(set_to_none=True)
        xx, ee = x[0].clone().requires_grad_(True), emb[0].detach().requires_grad_(emb_grad)
        hid, _ = torch_rpe_attention(att, xx, xx, xx, ee)
        hid.backward(go[0])
    return run


fns = [hip_forward, hip_fwd_bwd(False), hip_fwd_bwd(True), torch_forward, torch_fwd_bwd(False), torch_fwd_bwd(True)]
names = ["HIP forward", "HIP fwd+bwd", "HIP fwd+bwd +grad_embed", "torch forward", "torch fwd+bwd", "torch fwd+bwd +grad_embed"]
times = alternate(fns, args.reps)
print(f"RPE attention N = M = {N}, C = {C}, H = {H} (embedding {N * N * C * 4 / 1e6:.0f} MB)")
for name, t, fn in zip(names, times, fns):
    print(f"  {name:28s} {t:8.3f} ms   peak {peak_mb(fn):8.1f} MB")
for emb_grad in (False, True):
    ms = kernel_ms(hip_fwd_bwd(emb_grad), "rpe_attention_backward_rows")
    moved = N * N * C * 4 * (2 if emb_grad else 1)
    print(f"  row pass{' +grad_embed' if emb_grad else '':12s} {ms:8.3f} ms   {moved / 1e6:.0f} MB -> {moved / ms / 1e9:.2f} TB/s = "
          f"{100 * moved / (ms * 1e-3) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak")
print(f"  column pass            {kernel_ms(hip_fwd_bwd(False), 'rpe_attention_backward_cols'):8.3f} ms")

if not args.skip_stack:
    del emb
    torch.manual_seed(1)
    blocks = ["self", "cross"] * 3
    model = GeometricTransformer(1024, 256, C, H, blocks, 0.2, 15, 3, reduction_a="max").cuda()
    p0, p1 = torch.rand(1, N, 3, device="cuda") * 8, torch.rand(1, N, 3, device="cuda") * 8
    f0, f1 = torch.randn(1, N, 1024, device="cuda"), torch.randn(1, N, 1024, device="cuda")
    g0, g1 = torch.randn(1, N, 256, device="cuda"), torch.randn(1, N, 256, device="cuda")

    def hip_stack():
        model.zero_grad(set_to_none=True)
        with differentiable():
            o0, o1 = model(p0, p1, f0, f1)
        torch.autograd.backward([o0, o1], [g0, g1])

    def hip_stack_forward():
        with torch.no_grad():
            model(p0, p1, f0, f1)

    def torch_embedding(e, p):
        with torch.no_grad():
            dist = torch.cdist(p, p)
            knn = dist.topk(e.angle_k + 1, dim=1, largest=False)[1][:, 1:]
            ref = (p[knn] - p[:, None])[:, None].expand(-1, p.shape[0], -1, -1)
            anc = (p[None] - p[:, None])[:, :, None].expand(-1, -1, e.angle_k, -1)
            a_idx = torch.atan2(torch.linalg.norm(torch.cross(ref, anc, dim=-1), dim=-1), (ref * anc).sum(-1)) * e.factor_a
            d_idx = dist / e.sigma_d
        sin = lambda idx: torch.stack([torch.sin(idx[..., None] * e.embedding.div_term), torch.cos(idx[..., None] * e.embedding.div_term)],
                                      -1).flatten(-2)
        return e.proj_d(sin(d_idx)) + e.proj_a(sin(a_idx)).max(dim=2)[0]

    def torch_layer_tail(layer, hid, x_in):
        hid = layer.attention.norm(layer.attention.linear(hid) + x_in)
        return layer.output.norm(hid + layer.output.squeeze(F.relu(layer.output.expand(hid))))

    def torch_stack():
        model.zero_grad(set_to_none=True)
        e0, e1 = torch_embedding(model.embedding, p0[0]), torch_embedding(model.embedding, p1[0])
        a, b = model.in_proj(f0[0]), model.in_proj(f1[0])
        ch = C // H
        for layer, block in zip(model.transformer.layers, blocks):
            att_ = layer.attention.attention
            if block == "self":
                a = torch_layer_tail(layer, torch_rpe_attention(att_, a, a, a, e0)[0], a)
                b = torch_layer_tail(layer, torch_rpe_attention(att_, b, b, b, e1)[0], b)
            else:
                def cross(q, k):
                    qp, kp, vp = (lin(t).view(-1, H, ch).transpose(0, 1) for lin, t in
                                  ((att_.proj_q, q), (att_.proj_k, k), (att_.proj_v, k)))
                    p = torch.softmax(torch.einsum("hnc,hmc->hnm", qp, kp) / ch ** 0.5, -1)
                    return torch.matmul(p, vp).transpose(0, 1).reshape(-1, C)
                a = torch_layer_tail(layer, cross(a, b), a)
                b = torch_layer_tail(layer, cross(b, a), b)
        torch.autograd.backward([model.out_proj(a), model.out_proj(b)], [g0[0], g1[0]])

    ts = alternate([hip_stack_forward, hip_stack, torch_stack], max(3, args.reps // 2))
    print(f"GeometricTransformer, two clouds of {N}, hidden {C}, {H} heads, {blocks}")
    for name, t, fn in zip(["HIP forward", "HIP fwd+bwd", "torch fwd+bwd"], ts, [hip_stack_forward, hip_stack, torch_stack]):
        print(f"  {name:28s} {t:8.2f} ms   peak {peak_mb(fn):8.1f} MB")
    # ---- the structure embedding's backward alone, per cloud: the HIP kernel against the torch recomputation
    # (GeometricStructureEmbedding.grad_impl), alternating; the path is chosen when the forward builds the graph
    from gaussreg_amd.embedding import GeometricStructureEmbedding
    FP32_MFMA_PEAK = 157.3e12
    k = model.embedding.angle_k
    for red in ("max", "mean"):
        emb_mod = GeometricStructureEmbedding(C, 0.2, 15, k, reduction_a=red).cuda()
        emb_mod.load_state_dict(model.embedding.state_dict())
        params = list(emb_mod.parameters())
        graphs = {}
        for impl in ("hip", "torch"):
            emb_mod.grad_impl = impl
            with differentiable():
                graphs[impl] = emb_mod(p0)
        emb_mod.grad_impl = "hip"
        ge = torch.randn_like(graphs["hip"])
        run = {impl: (lambda e=e: torch.autograd.grad(e, params, ge, retain_graph=True)) for impl, e in graphs.items()}
        t_hip, t_torch = alternate([run["hip"], run["torch"]], max(3, args.reps // 2))
        ms = kernel_ms(run["hip"], "geo_embedding_backward")
        flop = 2.0 * N * N * C * C * (1 + (k if red == "max" else 1))
        g_hip, g_torch = run["hip"](), run["torch"]()
        rel = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(g_hip, g_torch))
        print(f"  structure embedding backward, one cloud, '{red}': HIP {t_hip:8.3f} ms (peak {peak_mb(run['hip']):7.1f} MB)   "
              f"torch recomputation {t_torch:8.2f} ms (peak {peak_mb(run['torch']):7.1f} MB)")
        print(f"    kernels (GEMM + reduction) {ms:8.3f} ms = {flop / 1e9:.0f} GFLOP at {flop / (ms * 1e-3) / 1e12:.1f} TFLOP/s = "
              f"{100 * flop / (ms * 1e-3) / FP32_MFMA_PEAK:.0f} % of the fp32 MFMA peak; largest relative difference of the two "
              f"paths' gradients {rel:.2e}")
        del graphs, run, ge, g_hip, g_torch
