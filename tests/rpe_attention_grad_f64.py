"""Test helper (not collected): the transformer stack restated in torch, so that torch autograd differentiates it.

  rpe_attention          RPEMultiHeadAttention.forward   rpe_transformer.py:34-72
  rpe_transformer_layer  RPETransformerLayer             rpe_transformer.py:75-132 + output_layer.py:6-21
  transformer_layer      TransformerLayer                vanilla_transformer.py:15-132
  geo_embedding          GeometricStructureEmbedding     geotransformer.py:26-73 (the formulas of tests/geo_embedding_f64.py)
  geometric_transformer  GeometricTransformer            geotransformer.py:76-155 + conditional_transformer.py:73-117

Written from the reference's formulas in the reference's association: the (N,M,C) embedding goes through proj_p FIRST and
is then contracted with q.  One batch element per call (q (N,C), points (N,3), ...).  `params` maps the reference's
state-dict names to torch tensors; their dtype is the dtype of the evaluation (float64: the truth of the GPU gradient
tests; float32: "the reference's own rounding error" side of the bar).  Nothing here shares code with gaussreg_amd or
oracle/.  tests/test_rpe_attention_grad_f64_reference.py pins the forward values against the NumPy restatements, runs
gradcheck and compares the gradients with those of the reference's own modules.
"""
import numpy as np
import torch
import torch.nn.functional as F


TAPS = None   # a dict while `tapped()` is active: state-dict name of a Linear -> the outputs it produced, in call order


class tapped:
    """`with tapped() as taps:` records the output of every Linear evaluated inside, so that `grads(..., taps=taps)` can
    report, per bias, the size of the terms its gradient sums: bias_terms[name] = max_c sum_rows |dY[row, c]|.  A bias
    gradient that is zero by the softmax's shift invariance (proj_k.bias and proj_p.bias without factors or weights, the two
    biases of the structure embedding) has only that scale: its float64 value is rounding noise around 0."""

    def __enter__(self):
        global TAPS
        TAPS = {}
        return TAPS

    def __exit__(self, *exc):
        global TAPS
        TAPS = None


def _lin(x, params, name):
    y = x @ params[name + ".weight"].t() + params[name + ".bias"]
    if TAPS is not None:
        TAPS.setdefault(name, []).append(y)
    return y


def _heads(x, h):
    return x.reshape(x.shape[0], h, -1).transpose(0, 1)            # (rows, C) -> (H, rows, ch)


def _softmax_scores(s, key_weights, key_masks, attention_factors):
    if attention_factors is not None:
        s = attention_factors.unsqueeze(0) * s
    if key_weights is not None:
        s = s * key_weights[None, None, :]
    if key_masks is not None:
        s = s.masked_fill(key_masks[None, None, :], float("-inf"))
    return torch.softmax(s, dim=-1)


def rpe_attention(params, q, k, v, emb, key_weights=None, key_masks=None, attention_factors=None, *, num_heads, prefix=""):
    """-> hidden (N,C), scores (H,N,M)."""
    h = num_heads
    (n, c), m = q.shape, k.shape[0]
    ch = c // h
    qp, kp, vp = (_heads(_lin(x, params, prefix + name), h) for x, name in ((q, "proj_q"), (k, "proj_k"), (v, "proj_v")))
    pp = _lin(emb.reshape(n * m, c), params, prefix + "proj_p").reshape(n, m, h, ch).permute(2, 0, 1, 3)   # (H, N, M, ch)
    s_p = torch.einsum("hnc,hnmc->hnm", qp, pp)
    s_e = torch.einsum("hnc,hmc->hnm", qp, kp)
    p = _softmax_scores((s_e + s_p) / ch ** 0.5, key_weights, key_masks, attention_factors)
    return torch.matmul(p, vp).transpose(0, 1).reshape(n, c), p


def attention(params, q, k, v, key_masks=None, *, num_heads, prefix=""):
    """MultiHeadAttention (vanilla_transformer.py:35-69) -> hidden (N,C), scores (H,N,M)."""
    h = num_heads
    n, c = q.shape
    qp, kp, vp = (_heads(_lin(x, params, prefix + name), h) for x, name in ((q, "proj_q"), (k, "proj_k"), (v, "proj_v")))
    p = _softmax_scores(torch.einsum("hnc,hmc->hnm", qp, kp) / (c // h) ** 0.5, None, key_masks, None)
    return torch.matmul(p, vp).transpose(0, 1).reshape(n, c), p


def _norm(x, params, name):
    return F.layer_norm(x, (x.shape[-1],), params[name + ".weight"], params[name + ".bias"], 1e-5)


def _attention_output(params, x, prefix):
    grown = _lin(torch.relu(_lin(x, params, prefix + "expand")), params, prefix + "squeeze")
    return _norm(x + grown, params, prefix + "norm")


def rpe_transformer_layer(params, x, mem, emb, key_masks=None, *, num_heads, prefix=""):
    hid, sc = rpe_attention(params, x, mem, mem, emb, key_masks=key_masks, num_heads=num_heads,
                            prefix=prefix + "attention.attention.")
    hid = _norm(_lin(hid, params, prefix + "attention.linear") + x, params, prefix + "attention.norm")
    return _attention_output(params, hid, prefix + "output."), sc


def transformer_layer(params, x, mem, key_masks=None, *, num_heads, prefix=""):
    hid, sc = attention(params, x, mem, mem, key_masks=key_masks, num_heads=num_heads, prefix=prefix + "attention.attention.")
    hid = _norm(_lin(hid, params, prefix + "attention.linear") + x, params, prefix + "attention.norm")
    return _attention_output(params, hid, prefix + "output."), sc


def embedding_indices(points, sigma_d, sigma_a, k):
    """tests/geo_embedding_f64.embedding_indices in torch: d_idx (N,N), a_idx (N,N,k).  No gradient (geotransformer.py:25)."""
    with torch.no_grad():
        p = points
        x2 = (p * p).sum(1)
        dist = (x2[:, None] - 2 * (p @ p.t()) + x2[None, :]).clamp_min(0).sqrt()
        knn = torch.sort(dist, dim=1, stable=True)[1][:, 1:k + 1]
        n = p.shape[0]
        r = (p[knn] - p[:, None, :])[:, None, :, :].expand(n, n, knn.shape[1], 3)
        a = (p[None, :, :] - p[:, None, :])[:, :, None, :].expand(n, n, knn.shape[1], 3)
        sin = torch.linalg.norm(torch.cross(r, a, dim=-1), dim=-1)
        cos = (r * a).sum(-1)
        return dist / sigma_d, torch.atan2(sin, cos) * (180.0 / (sigma_a * np.pi))


def _sinusoid(idx, div):
    om = idx.unsqueeze(-1) * div
    return torch.stack([torch.sin(om), torch.cos(om)], dim=-1).flatten(-2)      # (sin, cos) interleaved


def geo_embedding(params, points, sigma_d, sigma_a, k, reduction, prefix=""):
    """points (N,3) -> (N,N,C).  `embedding.div_term` holds fp32 values in every dtype, as the module's buffer does.
    (The margin by which reduction 'max' picks its winner: tests/transformer_grad_cases.max_margin.)"""
    dtype = params[prefix + "proj_d.weight"].dtype
    d_idx, a_idx = embedding_indices(points.to(dtype), sigma_d, sigma_a, k)
    div = params[prefix + "embedding.div_term"].to(dtype)
    out = _lin(_sinusoid(d_idx, div), params, prefix + "proj_d")
    if k > 0:
        a = _lin(_sinusoid(a_idx, div), params, prefix + "proj_a")                # (N, N, k, C)
        out = out + (a.max(dim=2)[0] if reduction == "max" else a.mean(dim=2))
    return out


def geometric_transformer(params, ref_points, src_points, ref_feats, src_feats, *, num_heads, blocks, sigma_d, sigma_a,
                          angle_k, reduction_a):
    """One pair: points (N,3) / (M,3), feats (N,Cin) / (M,Cin) -> (N,Cout), (M,Cout).  Sequential cross blocks."""
    e0 = geo_embedding(params, ref_points, sigma_d, sigma_a, angle_k, reduction_a, prefix="embedding.")
    e1 = geo_embedding(params, src_points, sigma_d, sigma_a, angle_k, reduction_a, prefix="embedding.")
    f0, f1 = _lin(ref_feats, params, "in_proj"), _lin(src_feats, params, "in_proj")
    for i, block in enumerate(blocks):
        pre = f"transformer.layers.{i}."
        if block == "self":
            f0, _ = rpe_transformer_layer(params, f0, f0, e0, num_heads=num_heads, prefix=pre)
            f1, _ = rpe_transformer_layer(params, f1, f1, e1, num_heads=num_heads, prefix=pre)
        else:
            f0, _ = transformer_layer(params, f0, f1, num_heads=num_heads, prefix=pre)
            f1, _ = transformer_layer(params, f1, f0, num_heads=num_heads, prefix=pre)
    return _lin(f0, params, "out_proj"), _lin(f1, params, "out_proj")


def to_params(state_dict, dtype, requires_grad=True):
    """numpy / torch state dict -> {name: leaf tensor of `dtype`}; buffers (div_term) get no grad."""
    out = {}
    for name, v in state_dict.items():
        t = torch.as_tensor(np.asarray(v)).to(dtype).clone()
        out[name] = t.requires_grad_(requires_grad and not name.endswith("div_term"))
    return out


def grads(outputs, upstream, wrt, taps=None):
    """torch.autograd.grad over a list of (output, upstream) pairs -> list of numpy float64 arrays (zeros where unused).
    With `taps` (see `tapped`): also {linear name + '.bias': max_c sum_rows |dY[row, c]|}."""
    outs = [o for o in outputs]
    ups = [torch.as_tensor(np.asarray(u)).to(o.dtype) for o, u in zip(outs, upstream)]
    tap_list = [] if taps is None else [(name, y) for name, ys in taps.items() for y in ys]
    gs = torch.autograd.grad(outs, list(wrt) + [y for _, y in tap_list], ups, allow_unused=True)
    res = [(torch.zeros_like(w) if g is None else g).detach().double().numpy() for g, w in zip(gs, wrt)]
    if taps is None:
        return res
    terms = {}
    for (name, y), g in zip(tap_list, gs[len(wrt):]):
        if g is not None:
            t = g.detach().double().abs().reshape(-1, g.shape[-1]).sum(0)
            terms[name + ".bias"] = terms.get(name + ".bias", 0) + t
    return res, {k: v.max().item() for k, v in terms.items()}
