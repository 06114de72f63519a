"""Test helper (not collected): one training step of the registration network restated in plain torch -- the training branch
of GeoTransformer.forward (experiments/geotransformer.gaussian_splatting.indoor/model.py:69-222) and OverallLoss
(loss.py:10-92) -- in the dtype of the parameters it is given.  float64 parameters give the truth of
tests/test_gpu_training_step_f64.py, float32 parameters the rounding error a stock-torch float32 step has against it.

Assembled from the restatements the suite already has (tests/kpconv_grad_f64.py, tests/rpe_attention_grad_f64.py,
tests/sinkhorn_grad_f64.py) and torch's own group_norm; the blocks (modules.py:53-225), the backbone's wiring
(backbone.py:95-212), the glue of the model and the formulas of the losses are restated here.  Nothing here calls a
gaussreg_amd operator or HIP.

Everything discrete is an INPUT (`case`), so every dtype differentiates the same function as the code under test:

    points, neighbors, subsampling, upsampling   lists per pyramid level; lengths (levels, 2)
    features (N, Cin), transform (4, 4)
    ref_knn_idx, src_knn_idx                     (superpoints, K) patch tables of point_to_node_partition (pad = #points_f)
    ref_knn_masks, src_knn_masks                 (superpoints, K) bool
    overlaps                                     (M, N) dense ground-truth overlap matrix
    ref_ci, src_ci                               (P,) the selected target pairs
    labels                                       (P, K+1, K+1) bool, FineMatchingLoss's labels

`hp` holds the hyper-parameters (training_step_cases.hyper(cfg)).  `variant` plants one of the glue errors the yardstick
must reject (tests/test_training_step_f64_reference.py): 'no_scale' (the 1/sqrt(C) of the scores omitted), 'swap_patches'
(ref and src exchanged in the patch gather), 'shadow_row0' (every gather of a padded feature matrix -- maxpool,
nearest_upsample, the patches -- reads row 0 where it should read the zero shadow row; in the patch gather alone the error
would be invisible, the padded slots being masked in Sinkhorn).
"""
import numpy as np
import torch
import torch.nn.functional as F

import rpe_attention_grad_f64 as tf64
import sinkhorn_grad_f64
from kpconv_grad_f64 import kpconv_ref, maxpool_ref, nearest_upsample_ref

SLOPE = 0.1          # LeakyReLU of every block (modules.py:70, :126, :196)
VARIANTS = (None, "no_scale", "swap_patches", "shadow_row0")


def to_params(state_dict, dtype):
    """State dict -> leaf tensors of `dtype`; buffers (kernel_points, div_term) take no gradient."""
    p = tf64.to_params({k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in state_dict.items()}, dtype)
    for name, t in p.items():
        if name.endswith("kernel_points"):
            t.requires_grad_(False)
    return p


def parameter_names(params):
    return [n for n, t in params.items() if t.requires_grad]


# --------------------------------------------------------------------------------------------------------- backbone
def _group_norm(x, p, name, groups):
    y = F.group_norm(x.t().unsqueeze(0), groups, p[name + ".weight"], p[name + ".bias"], 1e-5)   # (1, C, N): modules.py:45-50
    return y.squeeze(0).t()


def _unary(p, pre, x, groups, relu=True):
    y = _group_norm(x @ p[pre + "mlp.weight"].t() + p[pre + "mlp.bias"], p, pre + "norm.norm", groups)
    return F.leaky_relu(y, SLOPE) if relu else y


def _kpconv(p, pre, x, q, s, nb, sigma):
    return kpconv_ref(x, q, s, nb, p[pre + "kernel_points"], p[pre + "weights"], sigma, p.get(pre + "bias"))


def _conv_block(p, pre, x, q, s, nb, groups, sigma):
    return F.leaky_relu(_group_norm(_kpconv(p, pre + "KPConv.", x, q, s, nb, sigma), p, pre + "norm.norm", groups), SLOPE)


def _row0(idx, n, on):
    """The planted error 'shadow_row0': a padded slot (index n, the zero shadow row) reads row 0 instead."""
    return torch.where(idx >= n, torch.zeros_like(idx), idx) if on else idx


def _residual(p, pre, x, q, s, nb, groups, sigma, strided=False, row0=False):
    h = _unary(p, pre + "unary1.", x, groups) if pre + "unary1.mlp.weight" in p else x
    h = F.leaky_relu(_group_norm(_kpconv(p, pre + "KPConv.", h, q, s, nb, sigma), p, pre + "norm_conv.norm", groups), SLOPE)
    h = _unary(p, pre + "unary2.", h, groups, relu=False)
    sc = maxpool_ref(x, _row0(nb, x.shape[0], row0)) if strided else x
    if pre + "unary_shortcut.mlp.weight" in p:
        sc = _unary(p, pre + "unary_shortcut.", sc, groups, relu=False)
    return F.leaky_relu(h + sc, SLOPE)


def backbone(p, feats, case, groups, sigma, pre="backbone.", row0=False):
    """backbone.py:164-212 -> [feats at level 1 (fine), level 2, level 3, level 4 (coarse)]."""
    up_ref = lambda x, idx: nearest_upsample_ref(x, _row0(idx, x.shape[0], row0))
    dtype = feats.dtype
    pts = [torch.as_tensor(a).to(dtype) for a in case["points"]]
    nb, sub, up = ([torch.as_tensor(a).long() for a in case[k]] for k in ("neighbors", "subsampling", "upsampling"))
    res = lambda name, x, q, s, idx, mult, strided=False: _residual(p, pre + name + ".", x, q, s, idx, groups, sigma * mult, strided, row0)
    f1 = _conv_block(p, pre + "encoder1_1.", feats, pts[0], pts[0], nb[0], groups, sigma)
    f1 = res("encoder1_2", f1, pts[0], pts[0], nb[0], 1)
    f2 = res("encoder2_1", f1, pts[1], pts[0], sub[0], 1, True)
    f2 = res("encoder2_3", res("encoder2_2", f2, pts[1], pts[1], nb[1], 2), pts[1], pts[1], nb[1], 2)
    f3 = res("encoder3_1", f2, pts[2], pts[1], sub[1], 2, True)
    f3 = res("encoder3_3", res("encoder3_2", f3, pts[2], pts[2], nb[2], 4), pts[2], pts[2], nb[2], 4)
    f4 = res("encoder4_1", f3, pts[3], pts[2], sub[2], 4, True)
    f4 = res("encoder4_3", res("encoder4_2", f4, pts[3], pts[3], nb[3], 8), pts[3], pts[3], nb[3], 8)
    f5 = res("encoder5_1", f4, pts[4], pts[3], sub[3], 8, True)
    f5 = res("encoder5_3", res("encoder5_2", f5, pts[4], pts[4], nb[4], 16), pts[4], pts[4], nb[4], 16)
    l4 = _unary(p, pre + "decoder4.", torch.cat([up_ref(f5, up[3]), f4], 1), groups)
    l3 = _unary(p, pre + "decoder3.", torch.cat([up_ref(l4, up[2]), f3], 1), groups)
    l2 = torch.cat([up_ref(l3, up[1]), f2], 1) @ p[pre + "decoder2.mlp.weight"].t() + p[pre + "decoder2.mlp.bias"]
    return [l2, l3, l4, f5]


# ----------------------------------------------------------------------------------------------------------- losses
def coarse_loss(ref_feats, src_feats, overlaps, c):
    """loss.py:22-40 + circle_loss.py:44-86: the overlap-weighted circle loss on the superpoint feature distances."""
    dists = torch.sqrt((2.0 - 2.0 * ref_feats @ src_feats.t()).clamp(min=0.0))
    overlaps = overlaps.to(dists.dtype)
    pos, neg = overlaps > c["positive_overlap"], overlaps == 0
    rows = (pos.sum(1) > 0) & (neg.sum(1) > 0)
    cols = (pos.sum(0) > 0) & (neg.sum(0) > 0)
    far = 1e5
    w_pos = ((dists - far * (~pos).to(dists.dtype) - c["positive_optimal"]).clamp(min=0.0) * torch.sqrt(overlaps * pos)).detach()
    w_neg = (c["negative_optimal"] - (dists + far * (~neg).to(dists.dtype))).clamp(min=0.0).detach()
    s = c["log_scale"]
    e_pos, e_neg = s * (dists - c["positive_margin"]) * w_pos, s * (c["negative_margin"] - dists) * w_neg
    loss_row = F.softplus(torch.logsumexp(e_pos, 1) + torch.logsumexp(e_neg, 1)) / s
    loss_col = F.softplus(torch.logsumexp(e_pos, 0) + torch.logsumexp(e_neg, 0)) / s
    return (loss_row[rows].mean() + loss_col[cols].mean()) / 2, dists


def fine_labels(ref_pts, src_pts, ref_masks, src_masks, transform, radius):
    """loss.py:56-67 in the dtype of the points -> (labels (P, K+1, K+1) bool, squared distances (P, K, K))."""
    src = src_pts @ transform[:3, :3].t() + transform[:3, 3]
    d2 = ((ref_pts ** 2).sum(-1)[:, :, None] - 2.0 * ref_pts @ src.transpose(1, 2) + (src ** 2).sum(-1)[:, None, :]).clamp(min=0.0)
    corr = (d2 < radius ** 2) & ref_masks[:, :, None] & src_masks[:, None, :]
    P, K1, K2 = corr.shape
    labels = torch.zeros((P, K1 + 1, K2 + 1), dtype=torch.bool)
    labels[:, :-1, :-1] = corr
    labels[:, :-1, -1] = (corr.sum(2) == 0) & ref_masks
    labels[:, -1, :-1] = (corr.sum(1) == 0) & src_masks
    return labels, d2


# ------------------------------------------------------------------------------------------------------------- step
def _gather_rows(feats, idx, variant):
    """index_select of the matrix padded with a zero row (model.py:178-181)."""
    if variant == "shadow_row0":
        return feats[_row0(idx, feats.shape[0], True)]
    return torch.cat([feats, feats.new_zeros((1, feats.shape[1]))], 0)[idx]


def training_step(params, case, hp, variant=None, keep=None, reference_marginals=False):
    """-> {'loss', 'c_loss', 'f_loss'} (0-d tensors of the parameters' dtype, on the graph).  `keep`: a dict that receives
    the intermediate tensors feats_f, feats_c, ref_feats_c, src_feats_c (normalised), scores, matching_scores.
    `reference_marginals`: Sinkhorn's log-marginals rounded to float32 as the reference module rounds them in every dtype
    (sinkhorn_grad_f64.forward, `marginal_dtype`): what reproduces the reference's float64 numbers digit for digit."""
    assert variant in VARIANTS
    dtype = params["optimal_transport.alpha"].dtype
    t = lambda a: torch.as_tensor(np.asarray(a))
    lengths = np.asarray(case["lengths"])
    n_c, n_f = int(lengths[-1][0]), int(lengths[1][0])
    feats_list = backbone(params, t(case["features"]).to(dtype), case, hp["group_norm"], hp["init_sigma"],
                          row0=variant == "shadow_row0")
    feats_f, feats_c = feats_list[0], feats_list[-1]
    points_c = t(case["points"][-1]).to(dtype)
    g = hp["geotransformer"]
    sub = {k[len("transformer."):]: v for k, v in params.items() if k.startswith("transformer.")}
    ref_c, src_c = tf64.geometric_transformer(sub, points_c[:n_c], points_c[n_c:], feats_c[:n_c], feats_c[n_c:],
                                              num_heads=g["num_heads"], blocks=g["blocks"], sigma_d=g["sigma_d"],
                                              sigma_a=g["sigma_a"], angle_k=g["angle_k"], reduction_a=g["reduction_a"])
    ref_c, src_c = F.normalize(ref_c, p=2, dim=1), F.normalize(src_c, p=2, dim=1)
    c_loss, dists = coarse_loss(ref_c, src_c, t(case["overlaps"]), hp["coarse_loss"])
    # patches of the target pairs (model.py:171-193)
    ref_f, src_f = feats_f[:n_f], feats_f[n_f:]
    ref_ci, src_ci = t(case["ref_ci"]).long(), t(case["src_ci"]).long()
    ref_idx, src_idx = t(case["ref_knn_idx"]).long()[ref_ci], t(case["src_knn_idx"]).long()[src_ci]
    ref_m, src_m = t(case["ref_knn_masks"]).bool()[ref_ci], t(case["src_knn_masks"]).bool()[src_ci]
    if variant == "swap_patches":       # each side's patch rows read from the other cloud's features
        ref_f, src_f = src_f, ref_f
        ref_idx, src_idx = ref_idx.clamp(max=ref_f.shape[0]), src_idx.clamp(max=src_f.shape[0])
    ref_k, src_k = _gather_rows(ref_f, ref_idx, variant), _gather_rows(src_f, src_idx, variant)
    scores = torch.einsum("bnd,bmd->bnm", ref_k, src_k)
    if variant != "no_scale":
        scores = scores / feats_f.shape[1] ** 0.5
    matching = sinkhorn_grad_f64.forward(scores, params["optimal_transport.alpha"], ref_m.numpy(), src_m.numpy(),
                                         hp["num_sinkhorn_iterations"],
                                         marginal_dtype=torch.float32 if reference_marginals else None)
    f_loss = -matching[t(case["labels"]).bool()].mean()
    if keep is not None:
        keep.update(feats_f=feats_f, feats_c=feats_c, ref_feats_c=ref_c, src_feats_c=src_c, feat_dists=dists, scores=scores,
                    matching_scores=matching)
    w = hp["loss"]
    return {"loss": w["weight_coarse_loss"] * c_loss + w["weight_fine_loss"] * f_loss, "c_loss": c_loss, "f_loss": f_loss}


def gradients(params, loss, taps=None, retain_graph=False):
    """Gradient of `loss` in every parameter -> {name: float64 tensor, or None where the loss does not reach it}.  With the
    `taps` of rpe_attention_grad_f64.tapped(): also {transformer bias name: scale of the terms its gradient sums}."""
    names = parameter_names(params)
    tap_list = [] if taps is None else [(name, y) for name, ys in taps.items() for y in ys]
    gs = torch.autograd.grad(loss, [params[n] for n in names] + [y for _, y in tap_list], allow_unused=True,
                             retain_graph=retain_graph)
    out = {n: (None if g is None else g.detach().double()) for n, g in zip(names, gs)}
    if taps is None:
        return out
    terms = {}
    for (name, _), g in zip(tap_list, gs[len(names):]):
        if g is not None:
            key = "transformer." + name + ".bias"
            terms[key] = terms.get(key, 0) + g.detach().double().abs().reshape(-1, g.shape[-1]).sum(0)
    return out, {k: v.max().item() for k, v in terms.items()}


def run(state_dict, case, hp, dtype, which="loss", variant=None, keep=None, reference_marginals=False):
    """One step in `dtype` -> (losses {name: float}, grads {name: float64 tensor or None}, bias terms).  `which`: the loss
    that is differentiated; a tuple of names gives a tuple of (grads, terms) pairs from the one forward."""
    params = to_params(state_dict, dtype)
    with tf64.tapped() as taps:
        losses = training_step(params, case, hp, variant=variant, keep=keep, reference_marginals=reference_marginals)
    values = {k: float(v.detach().double()) for k, v in losses.items()}
    if isinstance(which, tuple):
        return values, tuple(gradients(params, losses[w], taps=taps, retain_graph=True) for w in which)
    grads, terms = gradients(params, losses[which], taps=taps)
    return values, grads, terms
